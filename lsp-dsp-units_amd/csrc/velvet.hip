// mi_velvet_bank -- `channels` x lsp::dspu::Velvet (reference: src/main/noise/Velvet.cpp): sparse-impulse noise over a Randomizer and
// an MLS per channel.  The arithmetic of a draw and of the register sits in randomizer_device.h and mls_device.h.
//
//   velvet_kernel<OP, VEC>   one wave per channel.  How many draws a segment takes depends on the draws, so nobody but the wave that
//       interprets them knows how far the four generator chains have to run: its lanes 0 .. 3 run them, VN_CHUNK draws at a time and
//       only when draws are asked for (need()), into a ring of VN_RING raw draws in LDS in draw order (draw d of a call belongs to
//       generator (nBufID + d) & 3).  The chains may run ahead of what is consumed: after a draw vLast IS the raw draw, so the state
//       that goes back is read from the ring at the last draw that each generator was asked for.
//       A call is `count` samples in segments of `seg` (the whole call for overwrite; 256, BUF_LIM_SIZE, with a source); a segment
//       restarts scan and idx, and the draws and the MLS go on.
//       OVN, OVNA   the draw of window `scan` is 2 * scan (position; 2 * scan + 1 is its spike), or scan with the uncrushed MLS core,
//           so a wave evaluates 64 windows at once: lanes 0 .. 59 own a window, lanes 60 .. 63 are the next batch's first four, looked
//           at only.  A ballot finds the first idx >= count: the draw that ends the segment, and with it the draws and MLS samples
//           taken.  Later writes win in the reference; here a window is dropped if one of the next three valid windows has its idx (a
//           window four on lies at least 2 W - 2.5 > 1 further: every idx below 2^24 is rounded by at most half a sample), which
//           makes the writes independent of their order.
//       ARN         the steps of 64 draws are formed at once, the positions are a serial sum with a truncation per step (not
//           associative): a uniform scan over the lanes' steps, eight at a time until idx >= count.  Positions rise strictly.
//       TRN         dense, four samples per lane as the LCG bank's uniform; crushed, the sign draws come `n` draws later: from the
//           ring for a segment of up to 256, in a second pass over dst (every lane reads what it wrote itself) for a longer one.
//       A segment of up to 256 samples is put together in an LDS tile and goes out as one coalesced row, the source read first (dst
//       may be src); a longer one has no source: dst is filled, then -- behind a barrier -- the spikes are scattered into it.
//       MLS spikes: sample i after the batch's state is the parity of rows[i] & state; the state moves by the powers M^(2^p) that a
//       lane holds in registers.  update_settings() is lazy as in the reference: the masked state is what spikes are taken from,
//       and it is written back, with bSync cleared, only if a spike was taken.
//       LDS: 4096 bytes of ring + 1024 bytes of tile per wave.
//
// A state that the host gives (init, set_state) travels in the channel's record and is taken by the next launch; a pending
// Velvet::init() of the MLS is applied BY THE KERNEL, against the nState that only the device knows (MLS.cpp:114-130).
#include "bank_core.h"
#include "mls_device.h"
#include "randomizer_device.h"

#include <chrono>
#include <cmath>
#include <vector>

#pragma clang fp contract(off)

namespace mi_mls { int device_tables(const uint64_t **tables); }     // noise.hip

namespace
{
    constexpr uint32_t PER = 4;
    constexpr uint32_t VN_RING = 1024, VN_MASK = VN_RING - 1;   // raw draws in LDS
    constexpr uint32_t VN_CHUNK = 128;                          // draws per round of the chains: 32 steps of each generator
    constexpr uint32_t VN_SEG = 256;                            // BUF_LIM_SIZE, and the tile: 64 lanes x 4
    constexpr uint32_t VN_OWN = 60, VN_AHEAD = 3;               // windows a batch owns; windows looked ahead at for "later wins"
    constexpr uint32_t VN_NONE = 0xFFFFFFFFu;
    constexpr uint32_t VN_POWERS = 7;                           // M^1 .. M^64 in registers
    constexpr size_t   COUNT_LIMIT = MI_VN_MAX_COUNT + 1;
    enum { MLS_KEEP, MLS_GIVEN, MLS_INIT };
    static_assert(VN_OWN + VN_AHEAD < 64 && 2 * VN_SEG + VN_CHUNK + 2 * 64 < VN_RING && VN_RING % VN_CHUNK == 0, "a batch's windows in a wave, its draws in the ring");

    struct velvet_params
    {
        uint32_t mul1[4], mul2[4], add[4];
        uint32_t last[4], buf_id, rand_known;                   // rand_known: vLast and nBufID are these, not the device's
        uint32_t mls_known, mls_sync;                           // MLS_GIVEN: the MLS is mls_bits, mls_state, mls_sync, upd_bits
        uint64_t mls_bits, mls_state;                           // MLS_INIT: the last pending init's n_bits and seed ...
        uint64_t first_bits, first_state;                       // ... the first one's, which meet the device's nBits and nState ...
        uint32_t upd_bits, forced;                              // ... and forced: two pending inits differed, bSync whatever the device holds
        uint32_t core, type, crush;
        float    width, delta, prob, amplitude, offset;
        uint32_t enabled;                                       // 0: the row is not written, the state and what is pending stay
        uint32_t pad;
    };
    struct velvet_state
    {
        uint32_t last[4], buf_id, sync;                         // vLast, nBufID; bSync
        uint64_t mls_state, n_bits;                             // nState, nBits
        uint32_t upd_bits, pad[5];                              // nBits at the last update_settings(), 0: never (all masks 0)
    };
    static_assert(sizeof(velvet_params) == 160 && sizeof(velvet_state) == 64, "16-byte multiples");

    // size_t(x) where it is defined; out of range and NaN saturate (and end the segment)
    __device__ __forceinline__ uint32_t to_index(float x)
    {
        return (x >= 0.0f && x < 4294967296.0f) ? uint32_t(x) : VN_NONE;
    }

    // What lanes 0 .. 3 wrote to LDS is there for all 64: the workgroup is ONE wave, whose LDS operations execute in the order they
    // were issued, so all that is needed is that the compiler keeps that order.  (__syncthreads() would also wait for every global
    // store that is still on its way, once per tile: measured, that wait and not the chain was what a call cost.)
    __device__ __forceinline__ void wave_sync()
    {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }

    // the four values v of samples i0 .. i0 + 3 of a segment of n: dst = v, src + v or src * v, the source read first
    template <int OP, bool VEC>
    __device__ __forceinline__ void put4(float *out, const float *in, uint32_t i0, uint32_t n, float (&v)[PER])
    {
        const bool whole = i0 + PER <= n;
        if (OP != MI_OSC_OVERWRITE)
        {
            float s[PER] = { 0.0f, 0.0f, 0.0f, 0.0f };
            if (VEC && whole)
            {
                const float4 q = *reinterpret_cast<const float4 *>(in + i0);
                s[0] = q.x, s[1] = q.y, s[2] = q.z, s[3] = q.w;
            }
            else
                for (uint32_t k = 0; k < PER && i0 + k < n; ++k)
                    s[k] = in[i0 + k];
            #pragma unroll
            for (uint32_t k = 0; k < PER; ++k)
                v[k] = (OP == MI_OSC_ADD) ? s[k] + v[k] : s[k] * v[k];     // add3 / mul3
        }
        if (VEC && whole)
            *reinterpret_cast<float4 *>(out + i0) = make_float4(v[0], v[1], v[2], v[3]);
        else
            for (uint32_t k = 0; k < PER && i0 + k < n; ++k)
                out[i0 + k] = v[k];
    }

    // M^n state, n <= 127 and the same in every lane, from the lane's words of M^1 .. M^64: by one whole wave
    __device__ __forceinline__ uint64_t mls_move(const uint64_t (&pw)[VN_POWERS], uint64_t state, uint32_t n)
    {
        #pragma unroll
        for (uint32_t p = 0; p < VN_POWERS; ++p)
            if ((n >> p) & 1u)
                state = __ballot(mi_mls::bit(pw[p], state) != 0);
        return state;
    }

    template <int OP, bool VEC>
    __global__ __launch_bounds__(64) void velvet_kernel(float *dst, const float *src, size_t dst_stride, size_t src_stride, uint32_t count,
                                                        uint32_t seg, velvet_params *params, velvet_state *state, const uint64_t *__restrict__ tables)
    {
        __shared__ uint32_t ring[VN_RING];
        __shared__ __attribute__((aligned(16))) float tile[VN_SEG];
        const uint32_t lane = threadIdx.x, ch = blockIdx.x, g = lane & 3u;
        const velvet_params P = params[ch];
        if (!P.enabled)                                         // the workgroup is this one wave
            return;
        const velvet_state S = state[ch];
        const uint32_t type = P.type, crush = P.crush;
        const float W = P.width, A = P.amplitude, off = P.offset, prob = P.prob;
        const bool uses_mls = P.core == MI_VN_CORE_MLS && !crush && type < MI_VN_VELVET_TRN;   // get_spike(), :137-148
        const uint32_t m = uses_mls ? 1u : 2u;                  // draws per window or step

        // ---- the Randomizer: lanes 0 .. 3 are its generators
        const uint32_t buf0 = (P.rand_known ? P.buf_id : S.buf_id) & 3u;
        // (the generator's own words straight from memory: an index into the copies would put them into scratch)
        const uint32_t mul1 = params[ch].mul1[g], mul2 = params[ch].mul2[g], add = params[ch].add[g];
        const uint32_t given = params[ch].last[g], kept = state[ch].last[g], last0 = P.rand_known ? given : kept;
        const uint32_t first = (g - buf0) & 3u;                 // this generator's first draw of the call; every fourth one from there
        uint32_t last = last0, made = 0, taken = 0;             // draws made (a multiple of VN_CHUNK), draws consumed
        // draws [0, hi) of the call are in the ring (hi is the same in every lane)
        auto need = [&](uint32_t hi)
        {
            for (; made < hi; made += VN_CHUNK)
                if (lane < 4)
                {
                    // a chunk starts at a multiple of VN_CHUNK and does not wrap: the stores' offsets are constants, and nothing but the
                    // step itself is on the chain
                    uint32_t *w = ring + (made & VN_MASK) + first;
                    #pragma unroll 8
                    for (uint32_t i = 0; i < VN_CHUNK / 4; ++i)
                    {
                        last = mi_rand::step(last, mul1, mul2, add);
                        w[4 * i] = last;
                    }
                }
            wave_sync();
        };
        auto rv_at = [&](uint32_t d) { return mi_rand::linear(ring[d & VN_MASK]); };

        // ---- the MLS: a pending init meets the device's nBits and nState (set_n_bits, set_state: MLS.cpp:114-130)
        uint64_t n_bits = S.n_bits, mls = S.mls_state;
        uint32_t sync = S.sync, upd_bits = S.upd_bits;
        if (P.mls_known == MLS_GIVEN)
            n_bits = P.mls_bits, mls = P.mls_state, sync = P.mls_sync, upd_bits = P.upd_bits;
        else if (P.mls_known == MLS_INIT)
        {
            sync |= uint32_t(P.first_bits != n_bits) | uint32_t(P.first_state != mls) | P.forced;
            n_bits = P.mls_bits, mls = P.mls_state;
        }
        // update_settings(), :153-179, as the first spike would run it: `run` is the state that spikes are taken from
        const uint32_t width_bits = (n_bits < 1) ? 1u : (n_bits > mi_mls::MLS_MAX_BITS) ? mi_mls::MLS_MAX_BITS : uint32_t(n_bits);
        const uint64_t active = (width_bits == mi_mls::MLS_MAX_BITS) ? ~uint64_t(0) : ~(~uint64_t(0) << width_bits);
        uint64_t run = sync ? (((mls & active) != 0) ? (mls & active) : active) : mls;
        bool spiked = false;
        uint64_t row = 0, pw[VN_POWERS] = { 0, 0, 0, 0, 0, 0, 0 };
        if (uses_mls)
        {
            const uint64_t *table = tables + size_t(width_bits - 1) * mi_mls::MLS_TABLE_WORDS;
            row = mi_mls::rows_of(table)[lane];
            #pragma unroll
            for (uint32_t p = 0; p < VN_POWERS; ++p)
                pw[p] = mi_mls::power_of(table, p)[lane];
        }
        // the spike of window or step `w` of the segment that began at draw d0; with the MLS, `w` is this lane's
        auto spike_of = [&](uint32_t d0, uint32_t w) -> float
        {
            if (uses_mls)
                return mi_mls::bit(row, run) ? 1.0f : -1.0f;    // process_single() at amplitude 1, offset 0
            const float rv = rv_at(d0 + 2 * w + 1);
            if (crush)
                return (rv > prob) ? 1.0f : -1.0f;              // get_crushed_spike(), :150-153
            return 2.0f * roundf(rv) - 1.0f;
        };

        for (uint32_t at = 0; at < count; at += seg)
        {
            const uint32_t n = (count - at < seg) ? count - at : seg, d0 = taken;
            float *out = dst + size_t(ch) * dst_stride + at;
            const float *in = (OP != MI_OSC_OVERWRITE) ? src + size_t(ch) * src_stride + at : nullptr;
            const bool tiled = OP != MI_OSC_OVERWRITE || n <= VN_SEG;
            if (type == MI_VN_VELVET_TRN)                       // :228-252
            {
                const float k = __fdiv_rn(W, W - 1.0f);
                const uint32_t tiles = (n + VN_SEG - 1) / VN_SEG;
                const bool two_passes = crush && !tiled;
                for (uint32_t pass = 0; pass < (two_passes ? 2u : 1u); ++pass)
                    for (uint32_t t = 0; t < tiles; ++t)
                    {
                        const uint32_t i0 = t * VN_SEG + lane * PER, base = d0 + pass * n;
                        need((crush && tiled) ? d0 + 2 * n : base + (((t + 1) * VN_SEG < n) ? (t + 1) * VN_SEG : n));
                        if (i0 >= n)
                            continue;
                        float v[PER];
                        if (pass == 0)
                        {
                            #pragma unroll
                            for (uint32_t j = 0; j < PER; ++j)
                                v[j] = roundf(k * (rv_at(base + i0 + j) - 0.5f));
                        }
                        else                                    // what this lane wrote in the first pass
                            for (uint32_t j = 0; j < PER; ++j)
                                v[j] = (i0 + j < n) ? out[i0 + j] : 0.0f;
                        if (crush && (tiled || pass == 1))
                        {
                            const uint32_t signs = tiled ? d0 + n : base;
                            #pragma unroll
                            for (uint32_t j = 0; j < PER; ++j)
                                v[j] = ((rv_at(signs + i0 + j) > prob) ? -1.0f : 1.0f) * fabsf(v[j]);
                        }
                        if (two_passes && pass == 0)
                        {
                            for (uint32_t j = 0; j < PER && i0 + j < n; ++j)
                                out[i0 + j] = v[j];
                            continue;
                        }
                        #pragma unroll
                        for (uint32_t j = 0; j < PER; ++j)
                            v[j] = v[j] * A, v[j] = v[j] + off;  // mul_k2, add_k2
                        put4<OP, VEC>(out, in, i0, n, v);
                    }
                taken = d0 + (crush ? 2 * n : n);
                continue;
            }

            // ---- OVN, OVNA, ARN and the default: zero fill, spikes, amplitude and offset
            float fill = 0.0f * A;
            fill = fill + off;
            if (tiled)
                *reinterpret_cast<float4 *>(tile + lane * PER) = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            else
                for (uint32_t i0 = lane * PER; i0 < n; i0 += 64 * PER)
                {
                    float v[PER] = { fill, fill, fill, fill };
                    put4<MI_OSC_OVERWRITE, VEC>(out, nullptr, i0, n, v);
                }
            wave_sync();
            // a long segment's spikes go to dst itself, where the fill has to be behind them: a barrier, with its wait for the fill's
            // stores, before the first spike -- by then the first batch's draws have been made while the stores were on their way
            bool filled = tiled;
            auto spike_to = [&](bool mine, uint32_t idx, float s)
            {
                if (!filled)
                    __syncthreads();
                filled = true;
                if (!mine)
                    return;
                if (tiled)
                    tile[idx] = s;
                else
                {
                    float v = s * A;
                    v = v + off;
                    out[idx] = v;
                }
            };
            if (type == MI_VN_VELVET_OVN || type == MI_VN_VELVET_OVNA)     // :159-204
            {
                const float k = (type == MI_VN_VELVET_OVN) ? W - 1.0f : W;
                for (uint32_t b = 0;; ++b)
                {
                    const uint32_t scan = b * VN_OWN + lane;
                    need(d0 + m * (b * VN_OWN + 64));
                    const uint32_t idx = to_index(float(scan) * W + rv_at(d0 + m * scan) * k);
                    const uint64_t over = __ballot(idx >= n);
                    const uint32_t end = over ? uint32_t(__builtin_ctzll(over)) : 64u;     // the first window that ends the segment
                    bool later = false;
                    #pragma unroll
                    for (uint32_t a = 1; a <= VN_AHEAD; ++a)
                    {
                        const uint32_t other = __shfl_down(idx, a);
                        later |= lane + a < end && other == idx;
                    }
                    spike_to(lane < VN_OWN && lane < end && !later, idx, spike_of(d0, scan));
                    const uint32_t done = (end < VN_OWN) ? end : VN_OWN;
                    if (uses_mls && done != 0)
                        run = mls_move(pw, run, done), spiked = true;
                    if (end < VN_OWN)
                    {
                        taken = d0 + m * (b * VN_OWN + end) + 1;    // the draw that broke the loop is consumed
                        break;
                    }
                }
            }
            else if (type == MI_VN_VELVET_ARN)                  // :206-226
            {
                const float k = 2.0f * P.delta * (W - 1.0f), c = 1.0f + (1.0f - P.delta) * (W - 1.0f);
                // idx is kept as the float that the reference converts it to: below 2^24 float(idx) is exact and truncf(x) is
                // float(size_t(x)), and from 2^24 on (out of range and NaN included) the segment is over, count being at most 2^24
                const float nf = float(n);
                float idx = 0.0f;
                for (uint32_t b = 0;; ++b)
                {
                    need(d0 + m * (b + 1) * 64);
                    const float step = c + k * rv_at(d0 + m * (b * 64 + lane));
                    const int step_bits = __float_as_int(step);
                    float pos = nf;
                    for (uint32_t j0 = 0; j0 < 64 && idx < nf; j0 += 8)
                    {
                        #pragma unroll
                        for (uint32_t j = 0; j < 8; ++j)
                        {
                            const float s = __int_as_float(__builtin_amdgcn_readlane(step_bits, int(j0 + j)));
                            idx = truncf(idx + s);
                            pos = (lane == j0 + j) ? idx : pos;
                        }
                    }
                    const uint64_t over = __ballot(!(pos < nf));
                    const uint32_t end = over ? uint32_t(__builtin_ctzll(over)) : 64u;
                    spike_to(lane < end, (lane < end) ? uint32_t(pos) : 0u, spike_of(d0, b * 64 + lane));
                    if (uses_mls && end != 0)
                        run = mls_move(pw, run, end), spiked = true;
                    if (end < 64)
                    {
                        taken = d0 + m * (b * 64 + end) + 1;
                        break;
                    }
                }
            }
            if (tiled)
            {
                wave_sync();
                const uint32_t i0 = lane * PER;
                if (i0 < n)
                {
                    const float4 q = *reinterpret_cast<const float4 *>(tile + i0);
                    float v[PER] = { q.x, q.y, q.z, q.w };
                    #pragma unroll
                    for (uint32_t j = 0; j < PER; ++j)
                        v[j] = v[j] * A, v[j] = v[j] + off;
                    put4<OP, VEC>(out, in, i0, n, v);
                }
                wave_sync();                                    // the tile is free for the next segment
            }
        }

        // ---- what goes back: vLast of a generator is its last draw that was consumed, nBufID the next draw's generator
        wave_sync();
        if (lane < 4)
            state[ch].last[g] = (taken > first) ? ring[(first + ((taken - 1 - first) & ~3u)) & VN_MASK] : last0;
        if (lane == 0)
        {
            velvet_state &s = state[ch];
            s.buf_id = (buf0 + taken) & 3u;
            s.sync = spiked ? 0u : sync;
            s.mls_state = spiked ? run : mls;
            s.n_bits = spiked ? uint64_t(width_bits) : n_bits;
            s.upd_bits = (spiked && sync) ? width_bits : upd_bits;
            params[ch].rand_known = 0;
            params[ch].mls_known = MLS_KEEP;
        }
    }
} // namespace

struct mi_velvet_bank : mi_bank::tables<velvet_params, velvet_state>
{
    std::vector<uint8_t> inited;                                // init() or set_state() has given the channel a nBufID
    uint32_t             uninited = 0;                          // channels without one
    bool                 any_known = false;                     // a record carries a state that no launch has taken yet
    uint32_t             disabled = 0;                          // channels that are switched off
    const uint64_t      *d_tables = nullptr;                    // the device's MLS tables, not the bank's
};

namespace
{
    #define VELVET_LAUNCH(op, vec, grid, st, ...) \
        do { \
            hipEvent_t ev0 = nullptr, ev1 = nullptr; \
            mi::take_profile_events(&ev0, &ev1); \
            const dim3 block(64); \
            if (op == MI_OSC_ADD && vec)        MI_LAUNCH((velvet_kernel<MI_OSC_ADD, true>), grid, block, 0, st, ev0, ev1, __VA_ARGS__); \
            else if (op == MI_OSC_ADD)          MI_LAUNCH((velvet_kernel<MI_OSC_ADD, false>), grid, block, 0, st, ev0, ev1, __VA_ARGS__); \
            else if (op == MI_OSC_MUL && vec)   MI_LAUNCH((velvet_kernel<MI_OSC_MUL, true>), grid, block, 0, st, ev0, ev1, __VA_ARGS__); \
            else if (op == MI_OSC_MUL)          MI_LAUNCH((velvet_kernel<MI_OSC_MUL, false>), grid, block, 0, st, ev0, ev1, __VA_ARGS__); \
            else if (vec)                       MI_LAUNCH((velvet_kernel<MI_OSC_OVERWRITE, true>), grid, block, 0, st, ev0, ev1, __VA_ARGS__); \
            else                                MI_LAUNCH((velvet_kernel<MI_OSC_OVERWRITE, false>), grid, block, 0, st, ev0, ev1, __VA_ARGS__); \
        } while (0)

    void give_rand(mi_velvet_bank *b, uint32_t channel, const mi_lcg_state_t &s)
    {
        velvet_params &p = b->params[channel];
        memcpy(p.mul1, s.mul1, sizeof(p.mul1)); memcpy(p.mul2, s.mul2, sizeof(p.mul2)); memcpy(p.add, s.add, sizeof(p.add));
        memcpy(p.last, s.last, sizeof(p.last));
        p.buf_id = s.buf_id, p.rand_known = 1;
        b->uninited += uint32_t(b->inited[channel]) - uint32_t(s.buf_id != MI_LCG_UNSET);
        b->inited[channel] = s.buf_id != MI_LCG_UNSET;
        b->any_known = true;
        b->up.touch(channel);
    }

    // MLS::set_n_bits(n_bits) and MLS::set_state(seed) on the record of a channel
    void give_mls_init(mi_velvet_bank *b, uint32_t channel, uint64_t n_bits, uint64_t seed)
    {
        velvet_params &p = b->params[channel];
        const uint32_t differs = uint32_t(n_bits != p.mls_bits) | uint32_t(seed != p.mls_state);
        if (p.mls_known == MLS_GIVEN)                           // the host knows the MLS: the rule is applied here
            p.mls_sync |= differs;
        else if (p.mls_known == MLS_INIT)
            p.forced |= differs;
        else
            p.mls_known = MLS_INIT, p.first_bits = n_bits, p.first_state = seed, p.forced = 0;
        p.mls_bits = n_bits, p.mls_state = seed;
        b->any_known = true;
        b->up.touch(channel);
    }

    template <class T> void set_word(mi_velvet_bank *b, uint32_t channel, T &field, T value)
    {
        if (memcmp(&field, &value, sizeof(T)) != 0)
            field = value, b->up.touch(channel);
    }
    inline float limit01(float v) { return (v < 0.0f) ? 0.0f : (v > 1.0f) ? 1.0f : v; }     // lsp_limit(v, 0.0f, 1.0f)
} // namespace

extern "C" {

int mi_velvet_bank_create(mi_velvet_bank_t **bank, uint32_t channels)
{
    int r = mi_bank::open(bank, "mi_velvet_bank_create", channels);
    if (r != MI_OK)
        return r;
    mi_velvet_bank *b = *bank;
    *bank = nullptr;
    b->channels = channels;
    b->inited.assign(channels, 0);
    b->uninited = channels;
    velvet_params p = velvet_params();                          // construct(), Velvet.cpp:48-63
    p.buf_id = MI_LCG_UNSET, p.mls_known = MLS_KEEP;
    p.core = MI_VN_CORE_MLS, p.type = MI_VN_VELVET_OVN, p.crush = 0, p.prob = 0.5f;
    p.width = 10.0f, p.delta = 0.5f, p.amplitude = 1.0f, p.offset = 0.0f, p.enabled = 1;
    velvet_state s = velvet_state();                            // Randomizer.cpp:69-80, MLS.cpp:89-103
    s.buf_id = MI_LCG_UNSET, s.sync = 1, s.n_bits = mi_mls::MLS_MAX_BITS;
    r = mi_bank::alloc(*b, "mi_velvet_bank_create", p, s);
    if (r == MI_OK)
        r = mi_mls::device_tables(&b->d_tables);
    if (r != MI_OK)
    {
        mi_bank::destroy(b);
        return r;
    }
    *bank = b;
    return MI_OK;
}

int mi_velvet_bank_destroy(mi_velvet_bank_t *b)
{
    return mi_bank::destroy(b);
}

#define VELVET_CHANNEL(name) \
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_velvet_bank_" name ": NULL bank"); \
    MI_REQUIRE(channel < b->channels, MI_EINVAL, "mi_velvet_bank_" name ": channel %u out of range", channel); \
    velvet_params &p = b->params[channel]

int mi_velvet_bank_init(mi_velvet_bank_t *b, uint32_t channel, uint32_t randseed, uint32_t mls_n_bits, uint64_t mls_seed)    // :111-121
{
    VELVET_CHANNEL("init");
    (void)p;
    mi_lcg_state_t s;
    mi_lcg_seed_words(randseed, &s);
    give_rand(b, channel, s);
    give_mls_init(b, channel, uint8_t(mls_n_bits), mls_seed);
    return MI_OK;
}

int mi_velvet_bank_init_time(mi_velvet_bank_t *b, uint32_t channel)                         // :123-130, Randomizer.cpp:101-106
{
    VELVET_CHANNEL("init_time");
    (void)p;
    const auto now = std::chrono::system_clock::now().time_since_epoch();
    const uint64_t ns = uint64_t(std::chrono::duration_cast<std::chrono::nanoseconds>(now).count());
    mi_lcg_state_t s;
    mi_lcg_seed_words(uint32_t((ns / 1000000000ull) ^ (ns % 1000000000ull)), &s);
    give_rand(b, channel, s);
    return MI_OK;
}

int mi_velvet_bank_set_core_type(mi_velvet_bank_t *b, uint32_t channel, uint32_t core)
{
    VELVET_CHANNEL("set_core_type");
    set_word(b, channel, p.core, core);
    return MI_OK;
}

int mi_velvet_bank_set_velvet_type(mi_velvet_bank_t *b, uint32_t channel, uint32_t type)
{
    VELVET_CHANNEL("set_velvet_type");
    set_word(b, channel, p.type, type);
    return MI_OK;
}

int mi_velvet_bank_set_velvet_window_width(mi_velvet_bank_t *b, uint32_t channel, float width)
{
    VELVET_CHANNEL("set_velvet_window_width");
    MI_REQUIRE(std::isfinite(width), MI_EINVAL, "mi_velvet_bank_set_velvet_window_width: the width is not finite");
    set_word(b, channel, p.width, (width > 2.0f) ? width : 2.0f);                           // lsp_max(width, MIN_WINDOW_WIDTH)
    return MI_OK;
}

int mi_velvet_bank_set_delta_value(mi_velvet_bank_t *b, uint32_t channel, float delta)
{
    VELVET_CHANNEL("set_delta_value");
    set_word(b, channel, p.delta, limit01(delta));
    return MI_OK;
}

int mi_velvet_bank_set_crush_probability(mi_velvet_bank_t *b, uint32_t channel, float prob)
{
    VELVET_CHANNEL("set_crush_probability");
    set_word(b, channel, p.prob, limit01(prob));
    return MI_OK;
}

int mi_velvet_bank_set_amplitude(mi_velvet_bank_t *b, uint32_t channel, float amplitude)
{
    VELVET_CHANNEL("set_amplitude");
    set_word(b, channel, p.amplitude, amplitude);
    return MI_OK;
}

int mi_velvet_bank_set_offset(mi_velvet_bank_t *b, uint32_t channel, float offset)
{
    VELVET_CHANNEL("set_offset");
    set_word(b, channel, p.offset, offset);
    return MI_OK;
}

int mi_velvet_bank_set_crush(mi_velvet_bank_t *b, uint32_t channel, int crush)
{
    VELVET_CHANNEL("set_crush");
    set_word(b, channel, p.crush, uint32_t(crush != 0));
    return MI_OK;
}

// segmented: an overwrite cut into segments of BUF_LIM_SIZE, as a caller's loop of process_overwrite(tmp, <= 256) makes it
static int velvet_process(const char *entry, mi_velvet_bank *b, float *dst, const float *src, size_t count, size_t dst_stride, size_t src_stride,
                          uint32_t op, bool segmented, void *stream)
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "%s: NULL bank", entry);
    MI_REQUIRE(op <= MI_OSC_MUL, MI_EINVAL, "%s: no operation %u", entry, op);
    if (op == MI_OSC_OVERWRITE)
        src = nullptr;
    if (count == 0)
        return MI_OK;
    int r = mi_bank::check_rows(entry, b->channels, count, COUNT_LIMIT,
                                { { dst, dst_stride, count, mi_bank::REQUIRED | mi_bank::OUTPUT }, { src, src_stride, count, 0 } });
    if (r != MI_OK)
        return r;
    for (uint32_t ch = 0; b->uninited != 0 && ch < b->channels; ++ch)
        MI_REQUIRE(b->inited[ch] || !b->params[ch].enabled, MI_ESTATE, "%s: channel %u was never init()ed", entry, ch);
    if (b->disabled == b->channels)                         // nobody's process() is called
        return MI_OK;
    hipStream_t st = mi::as_stream(stream);
    if (src == nullptr && op == MI_OSC_MUL)                 // noise * 0: fill_zero and not a draw, :290-295
    {
        if (b->channels == 1)                               // one row: its stride says nothing
            MI_HIP_CHECK(hipMemsetAsync(dst, 0, count * sizeof(float), st));
        else if (b->disabled == 0)
            MI_HIP_CHECK(hipMemset2DAsync(dst, dst_stride * sizeof(float), 0, count * sizeof(float), b->channels, st));
        else
            for (uint32_t ch = 0; ch < b->channels; ++ch)
                if (b->params[ch].enabled)
                    MI_HIP_CHECK(hipMemsetAsync(dst + size_t(ch) * dst_stride, 0, count * sizeof(float), st));
        return MI_OK;
    }
    r = mi_bank::upload(*b, "mi_velvet_bank", st);
    if (r != MI_OK)
        return r;
    // with a source the call is cut into segments of BUF_LIM_SIZE; without one (overwrite, add to nothing) it is one segment
    const uint32_t mode = (src == nullptr) ? uint32_t(MI_OSC_OVERWRITE) : op;
    const uint32_t seg = (src == nullptr && !segmented) ? uint32_t(count) : VN_SEG;
    const bool vec = mi::aligned16(dst, dst_stride, b->channels) && (src == nullptr || mi::aligned16(src, src_stride, b->channels));
    const dim3 grid(b->channels);
    VELVET_LAUNCH(mode, vec, grid, st, dst, src, dst_stride, src_stride, uint32_t(count), seg, b->d_params, b->d_state, b->d_tables);
    MI_HIP_CHECK(hipGetLastError());
    bool left = false;
    for (uint32_t ch = 0; b->any_known && ch < b->channels; ++ch)  // as the kernel leaves the records
    {
        velvet_params &p = b->params[ch];
        if (p.enabled)
            p.rand_known = 0, p.mls_known = MLS_KEEP;
        else
            left |= p.rand_known != 0 || p.mls_known != MLS_KEEP;
    }
    b->any_known = left;
    return MI_OK;
}

int mi_velvet_bank_process(mi_velvet_bank_t *b, float *dst, const float *src, size_t count, size_t dst_stride, size_t src_stride, uint32_t op,
                           void *stream)
{
    return velvet_process("mi_velvet_bank_process", b, dst, src, count, dst_stride, src_stride, op, false, stream);
}

int mi_velvet_bank_process_segmented(mi_velvet_bank_t *b, float *dst, size_t count, size_t dst_stride, void *stream)
{
    return velvet_process("mi_velvet_bank_process_segmented", b, dst, nullptr, count, dst_stride, 0, MI_OSC_OVERWRITE, true, stream);
}

int mi_velvet_bank_set_row_enabled(mi_velvet_bank_t *b, uint32_t channel, int enabled)
{
    VELVET_CHANNEL("set_row_enabled");
    const uint32_t on = enabled != 0;
    if (p.enabled != on)
        b->disabled += p.enabled - on, p.enabled = on, b->up.touch(channel);
    return MI_OK;
}

int mi_velvet_bank_commit(mi_velvet_bank_t *b, void *stream)
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_velvet_bank_commit: NULL bank");
    return mi_bank::upload(*b, "mi_velvet_bank", mi::as_stream(stream));
}

int mi_velvet_bank_reserve(mi_velvet_bank_t *b, size_t count)
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_velvet_bank_reserve: NULL bank");
    MI_REQUIRE(count < COUNT_LIMIT, MI_EINVAL, "mi_velvet_bank_reserve: count %zu too large", count);
    return MI_OK;
}

int mi_velvet_bank_get_state(mi_velvet_bank_t *b, uint32_t channel, mi_velvet_state_t *state, void *stream)
{
    VELVET_CHANNEL("get_state");
    MI_REQUIRE(state != nullptr, MI_EINVAL, "mi_velvet_bank_get_state: NULL state");
    velvet_state s;
    int r = mi_bank::get_state(b, "mi_velvet_bank_get_state", channel, &s, stream);    // refuses a capturing stream
    if (r != MI_OK)
        return r;
    *state = mi_velvet_state_t();
    mi_lcg_state_t &rs = state->rand;
    memcpy(rs.mul1, p.mul1, sizeof(p.mul1)); memcpy(rs.mul2, p.mul2, sizeof(p.mul2)); memcpy(rs.add, p.add, sizeof(p.add));
    memcpy(rs.last, p.rand_known ? p.last : s.last, sizeof(rs.last));
    rs.buf_id = p.rand_known ? p.buf_id : s.buf_id;
    if (p.mls_known == MLS_GIVEN)                               // what the next launch will take, as the kernel takes it
        s.n_bits = p.mls_bits, s.mls_state = p.mls_state, s.sync = p.mls_sync, s.upd_bits = p.upd_bits;
    else if (p.mls_known == MLS_INIT)
    {
        s.sync |= uint32_t(p.first_bits != s.n_bits) | uint32_t(p.first_state != s.mls_state) | p.forced;
        s.n_bits = p.mls_bits, s.mls_state = p.mls_state;
    }
    mi_mls_settings_t &ms = state->mls;
    mi_mls_settings_init(&ms);
    ms.n_bits = s.n_bits, ms.state = s.mls_state, ms.sync = s.sync;
    if (s.upd_bits != 0)
    {
        ms.feedback_bit = s.upd_bits - 1;
        ms.feedback_mask = uint64_t(1) << ms.feedback_bit;
        ms.active_mask = (s.upd_bits == mi_mls::MLS_MAX_BITS) ? ~uint64_t(0) : ~(~uint64_t(0) << s.upd_bits);
        ms.taps_mask = mi_mls::taps()[s.upd_bits - 1];
    }
    return MI_OK;
}

int mi_velvet_bank_set_state(mi_velvet_bank_t *b, uint32_t channel, const mi_velvet_state_t *state, void *stream)
{
    VELVET_CHANNEL("set_state");
    MI_REQUIRE(state != nullptr, MI_EINVAL, "mi_velvet_bank_set_state: NULL state");
    MI_REQUIRE(state->rand.buf_id <= 3 || state->rand.buf_id == MI_LCG_UNSET, MI_EINVAL,
               "mi_velvet_bank_set_state: nBufID %u is neither 0 .. 3 nor unset", state->rand.buf_id);
    const mi_mls_settings_t &ms = state->mls;
    const uint64_t upd = (ms.feedback_mask != 0) ? ms.feedback_bit + 1 : 0;
    MI_REQUIRE(upd <= mi_mls::MLS_MAX_BITS, MI_EINVAL, "mi_velvet_bank_set_state: nFeedbackBit %llu", (unsigned long long)ms.feedback_bit);
    // a register that is in use (bSync clear) is one that update_settings() left: its width, and no bit beyond it
    MI_REQUIRE(ms.sync != 0 || (upd != 0 && ms.n_bits == upd && (upd == mi_mls::MLS_MAX_BITS || (ms.state >> upd) == 0)), MI_EINVAL,
               "mi_velvet_bank_set_state: bSync is clear and nBits %llu, nState %#llx are not what update_settings() leaves",
               (unsigned long long)ms.n_bits, (unsigned long long)ms.state);
    const int r = mi::refuse_state_access(mi::as_stream(stream));
    if (r != MI_OK)
        return r;
    give_rand(b, channel, state->rand);
    p.mls_known = MLS_GIVEN, p.mls_bits = ms.n_bits, p.mls_state = ms.state, p.mls_sync = ms.sync != 0, p.upd_bits = uint32_t(upd);
    return MI_OK;
}

} // extern "C"
