// The maximum-length-sequence register of lsp::dspu::MLS (reference: src/main/noise/MLS.cpp:208-221) in closed form over GF(2), with
// nothing of a bank in it.  The register shifts right and its output is bit 0, so the update is linear: s' = M s with 64 x 64 bit
// matrices kept as 64 row words, (A v) bit k = parity(A[k] & v).  From that:
//     sample i of a call   parity(rows[i] & s0), rows[i] = row 0 of M^i
//     the state n samples on   M^n s0 = the product of the powers M^(2^p) over the set bits p of n
// Both depend on the register width alone, so one table per width 1 .. 64 serves every channel of every bank:
//     [ rows[MLS_TILE] | M^(2^0)[64] | M^(2^1)[64] | ... | M^(2^(MLS_POWERS - 1))[64] ]      MLS_TABLE_WORDS words
// The host builds all 64 once (csrc/host/noise.cpp); a device copy is made per device at the first use.
#pragma once
#include <cstdint>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif

namespace mi_mls
{
    constexpr uint32_t MLS_MAX_BITS = 64;                   // sizeof(mls_t) * 8 with mls_t = uint64_t
    constexpr uint32_t MLS_TILE_LOG2 = 10, MLS_TILE = 1u << MLS_TILE_LOG2;     // samples whose rows the table holds
    constexpr uint32_t MLS_POWERS = 27;                     // a call is shorter than 2^27 samples
    constexpr uint32_t MLS_TABLE_WORDS = MLS_TILE + MLS_POWERS * 64;

    // the tables of all widths, [MLS_MAX_BITS][MLS_TABLE_WORDS], width w at index w - 1 (host memory; built at the first call)
    const uint64_t *host_tables();
    // the feedback taps of the widths 1 .. 64, width w at index w - 1
    const uint64_t *taps();
    // M^count state for a register of n_bits (1 .. 64), any count
    uint64_t host_advance(uint32_t n_bits, uint64_t state, uint64_t count);

#if defined(__HIPCC__)
    __device__ __forceinline__ const uint64_t *rows_of(const uint64_t *table)                 { return table; }
    __device__ __forceinline__ const uint64_t *power_of(const uint64_t *table, uint32_t p)    { return table + MLS_TILE + p * 64; }

    // progress()'s output from the state i samples back: 1 or 0
    __device__ __forceinline__ uint32_t bit(uint64_t row, uint64_t state) { return uint32_t(__popcll(row & state)) & 1u; }

    // A s is formed by one whole wave of 64 lanes: lane k forms bit k from its word A[k], a ballot collects them.
    // M^(first * 2^p0) state over the set bits of `first` (below 2^N, the same in every lane): by one whole wave.  The lane's words of
    // all the powers it needs are asked for before the first is used: one memory latency, then ballots on registers.
    template <uint32_t N>
    __device__ __forceinline__ uint64_t jump(const uint64_t *table, uint64_t state, uint32_t first, uint32_t p0, uint32_t lane)
    {
        uint64_t word[N];
        #pragma unroll
        for (uint32_t j = 0; j < N; ++j)
            word[j] = ((first >> j) & 1u) ? power_of(table, p0 + j)[lane] : 0;
        #pragma unroll
        for (uint32_t j = 0; j < N; ++j)
            if ((first >> j) & 1u)
                state = __ballot(bit(word[j], state) != 0);
        return state;
    }
#endif
} // namespace mi_mls
