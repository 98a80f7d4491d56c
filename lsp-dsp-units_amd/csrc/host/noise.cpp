// The word arithmetic under the noise banks (csrc/noise.hip) that needs no device: Randomizer::init(seed)
// (src/main/util/Randomizer.cpp:86-99), construct() and update_settings() of lsp::dspu::MLS (src/main/noise/MLS.cpp:89-103, :153-179) on a
// mi_mls_settings_t, and the closed form of the MLS register over GF(2) that csrc/mls_device.h describes: per register width the rows
// of one tile and the powers M^(2^p) of the transition matrix.
#include "mi_common.h"
#include "mls_device.h"

#include <cstdint>
#include <mutex>
#include <vector>

namespace
{
    // Randomizer.cpp:35-57
    const uint32_t MUL1[16] = { 0x43ca16c1, 0x451222f3, 0x465e0183, 0x47f27263, 0x4212ffe9, 0x4433f6ad, 0x40f31425, 0x412318bb,
                                0x48f39cbf, 0x49b18a45, 0x4d341bbf, 0x4e93a169, 0x4bacd5e5, 0x4c55e139, 0x4f11db4d, 0x4a901f8b };
    const uint32_t MUL2[16] = { 0x4c37c68f, 0x4d59b853, 0x4ef1d1e9, 0x4fe16c01, 0x40fc2271, 0x44e335c1, 0x450fc1bb, 0x48cc3d07,
                                0x493737a9, 0x4182e63f, 0x42198197, 0x43fc5611, 0x4ac116eb, 0x4b0faf0d, 0x46777db9, 0x4730a64d };
    const uint32_t ADDERS[16] = { 0x000551ff, 0x000633f5, 0x00011fcf, 0x00021b81, 0x00075af1, 0x00080be5, 0x000330a7, 0x00040d0b,
                                  0x000c2521, 0x000dd113, 0x0009eea5, 0x000ae007, 0x00092df5, 0x000b42bd, 0x000e1b15, 0x000f054d };

    // The feedback taps of a primitive polynomial for every register width 1 .. 64, as a mask over the state: the table of
    // W. Stahnke, "Primitive Binary Polynomials", Math. Comp. 27 (1973), that MLS.cpp:36-58 uses for a 64-bit mls_t
    const uint64_t TAPS[64] = {
        1, 3, 3, 3, 5, 3, 3, 99, 17, 9, 5, 153, 27, 6147, 3, 45,
        9, 129, 99, 9, 5, 3, 33, 27, 9, 387, 387, 9, 5, 98307, 9, 402653187,
        8193, 49155, 5, 2049, 5125, 99, 17, 2621445, 9, 12582915, 99, 201326595, 27, 3145731, 33, 402653187,
        513, 201326595, 98307, 9, 98307, 206158430211ull, 16777217, 6291459, 129, 524289, 6291459, 3, 98307, 216172782113783811ull, 3, 27 };

    using mi_mls::MLS_MAX_BITS; using mi_mls::MLS_TILE; using mi_mls::MLS_POWERS; using mi_mls::MLS_TABLE_WORDS;

    // the row vector v times B: the xor of the rows of B that v selects
    inline uint64_t vecmat(uint64_t v, const uint64_t *B)
    {
        uint64_t out = 0;
        for (; v != 0; v &= v - 1)
            out ^= B[__builtin_ctzll(v)];
        return out;
    }

    inline uint64_t host_matvec(const uint64_t *A, uint64_t v)
    {
        uint64_t out = 0;
        for (uint32_t k = 0; k < 64; ++k)
            out |= uint64_t(__builtin_parityll(A[k] & v)) << k;
        return out;
    }

    // bit k of the next state is bit k + 1 of this one; the top bit of the register is the parity of the taps (:213-218)
    void transition(uint32_t n_bits, uint64_t *M)
    {
        for (uint32_t k = 0; k < 64; ++k)
            M[k] = (k + 1 < n_bits) ? uint64_t(1) << (k + 1) : (k + 1 == n_bits) ? TAPS[n_bits - 1] : 0;
    }

    void build_table(uint32_t n_bits, uint64_t *table)
    {
        uint64_t *rows = table, *powers = table + MLS_TILE;
        transition(n_bits, powers);
        uint64_t r = 1;                                     // row 0 of the identity
        for (uint32_t i = 0; i < MLS_TILE; ++i)
        {
            rows[i] = r;
            r = vecmat(r, powers);
        }
        for (uint32_t p = 1; p < MLS_POWERS; ++p)
            for (uint32_t k = 0; k < 64; ++k)
                powers[p * 64 + k] = vecmat(powers[(p - 1) * 64 + k], powers + (p - 1) * 64);
    }
}

namespace mi_mls
{
    const uint64_t *taps() { return TAPS; }

    const uint64_t *host_tables()
    {
        static std::vector<uint64_t> tables;
        static std::once_flag once;
        std::call_once(once, []
        {
            tables.resize(size_t(MLS_MAX_BITS) * MLS_TABLE_WORDS);
            for (uint32_t w = 1; w <= MLS_MAX_BITS; ++w)
                build_table(w, tables.data() + size_t(w - 1) * MLS_TABLE_WORDS);
        });
        return tables.data();
    }

    uint64_t host_advance(uint32_t n_bits, uint64_t state, uint64_t count)
    {
        const uint64_t *powers = host_tables() + size_t(n_bits - 1) * MLS_TABLE_WORDS + MLS_TILE;
        uint32_t p = 0;
        for (; count != 0 && p < MLS_POWERS; count >>= 1, ++p)
            if (count & 1)
                state = host_matvec(powers + p * 64, state);
        if (count == 0)
            return state;
        uint64_t P[64], Q[64];                              // beyond the table: square on
        for (uint32_t k = 0; k < 64; ++k)
            P[k] = vecmat(powers[(MLS_POWERS - 1) * 64 + k], powers + (MLS_POWERS - 1) * 64);
        for (; count != 0; count >>= 1)
        {
            if (count & 1)
                state = host_matvec(P, state);
            for (uint32_t k = 0; k < 64; ++k)
                Q[k] = vecmat(P[k], P);
            memcpy(P, Q, sizeof(P));
        }
        return state;
    }
}

extern "C" {

int mi_lcg_seed_words(uint32_t seed, mi_lcg_state_t *s)
{
    MI_REQUIRE(s != nullptr, MI_EINVAL, "mi_lcg_seed_words: NULL state");
    for (uint32_t i = 0; i < 4; ++i)
    {
        const uint32_t reseed = (i > 0) ? (seed << (i * 8)) | (seed >> ((4 - i) * 8)) : seed;      // :90
        s->add[i] = ADDERS[reseed & 0x0f];
        s->mul1[i] = MUL1[(reseed >> 4) & 0x0f];
        s->mul2[i] = MUL2[(reseed >> 8) & 0x0f];
        s->last[i] = reseed ^ (seed >> 4);
    }
    s->buf_id = 0;
    return MI_OK;
}

int mi_mls_settings_init(mi_mls_settings_t *s)                                              // construct(), :89-103
{
    MI_REQUIRE(s != nullptr, MI_EINVAL, "mi_mls_settings_init: NULL settings");
    *s = mi_mls_settings_t();
    s->n_bits = MLS_MAX_BITS;
    s->output_mask = 1;
    s->amplitude = 1.0f;
    s->sync = 1;
    return MI_OK;
}

int mi_mls_settings_update(mi_mls_settings_t *s)                                            // update_settings(), :153-179
{
    MI_REQUIRE(s != nullptr, MI_EINVAL, "mi_mls_settings_update: NULL settings");
    if (!s->sync)
        return MI_OK;
    s->n_bits = (s->n_bits < 1) ? 1 : (s->n_bits > MLS_MAX_BITS) ? MLS_MAX_BITS : s->n_bits;
    s->feedback_bit = s->n_bits - 1;
    s->feedback_mask = uint64_t(1) << s->feedback_bit;
    s->active_mask = (s->n_bits == MLS_MAX_BITS) ? ~uint64_t(0) : ~(~uint64_t(0) << s->n_bits);
    s->taps_mask = TAPS[s->n_bits - 1];
    s->state &= s->active_mask;
    if (s->state == 0)                                      // the state cannot be 0: all active bits then
        s->state |= s->active_mask;
    s->sync = 0;
    return MI_OK;
}

int mi_mls_tables(uint32_t n_bits, uint64_t *rows, uint64_t *powers)
{
    MI_REQUIRE(n_bits >= 1 && n_bits <= MLS_MAX_BITS, MI_EINVAL, "mi_mls_tables: %u bits; a register has 1 .. 64", n_bits);
    const uint64_t *t = mi_mls::host_tables() + size_t(n_bits - 1) * MLS_TABLE_WORDS;
    if (rows != nullptr)
        memcpy(rows, t, MLS_TILE * sizeof(uint64_t));
    if (powers != nullptr)
        memcpy(powers, t + MLS_TILE, size_t(MLS_POWERS) * 64 * sizeof(uint64_t));
    return MI_OK;
}

int mi_mls_advance(uint32_t n_bits, uint64_t state, uint64_t count, uint64_t *result)
{
    MI_REQUIRE(n_bits >= 1 && n_bits <= MLS_MAX_BITS && result != nullptr, MI_EINVAL, "mi_mls_advance: bad argument");
    *result = mi_mls::host_advance(n_bits, state, count);
    return MI_OK;
}

} // extern "C"
