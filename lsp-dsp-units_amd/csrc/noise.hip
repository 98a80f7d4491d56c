// mi_lcg_bank and mi_mls_bank -- `channels` x lsp::dspu::LCG and `channels` x lsp::dspu::MLS (reference: src/main/noise/LCG.cpp,
// src/main/noise/MLS.cpp, src/main/util/Randomizer.cpp): the noise sources as device banks.  The arithmetic of a draw and of the
// register sits in randomizer_device.h and mls_device.h; what is here is how a bank spreads it over a launch.
//
//   lcg_kernel<OP, VEC>      one workgroup of five waves per LCG_GROUP = 4 channels.  A Randomizer is four generators whose map is not
//       affine: no jump-ahead, a channel is four serial chains, and their latency is what a call costs.  Wave 0 is the producer, one
//       lane per (channel, generator): per chunk of LCG_CHUNK samples it runs its chain and leaves the raw draws in LDS in draw order
//       (draw d of a call belongs to generator (nBufID + d) & 3).  Waves 1 .. 4 are the transform, one channel each: a lane takes four
//       adjacent samples, a wave one coalesced row of 256 samples per chunk; the channel is uniform in a wave, so its record sits in
//       SGPRs and the switch on the distribution is a scalar branch.  The draws are double-buffered: in round c the producer makes
//       chunk c while the transform works on chunk c - 1, one barrier per round.  The producer writes vLast and nBufID back at the end;
//       no other workgroup touches them.
//       Four channels and not the sixteen a wave of producer lanes could take: the chain is bound by latency, so idle producer lanes
//       cost nothing, and four times as many workgroups spread the transform over four times as many CUs (DESIGN.md 3.25 has both).
//       LDS: 2 x 4 rows of 2 * 256 draws (exponential and Gaussian take two per sample) + 4 words, 16 512 bytes; the 4 words put the
//       rows that the producer's lanes write at once into different banks.
//   mls_kernel<OP, VEC>      grid (spans of MLS_SPAN = 4 tiles of MLS_TILE = 1024 samples, channels); the first tile's state is
//       M^(span * 4096) s0 over the set bits of the span index, the next tiles' by M^1024 (every wave forms them for itself: 64 lanes, one
//       ballot per power, the lane's words of all powers asked for up front; no LDS and no barrier); a lane owns four adjacent samples
//       of every tile: four row words -- the same in every tile --, four popcounts.
//   mls_advance_kernel       one wave per channel, behind the tiles on the stream: nState = M^count s0, and a state that came in the
//       record is marked as taken.  A follow-up launch as the oscillator's: ordered by the stream, no atomics, capturable.
//
// OP is overwrite, add or mul; add and mul read their four src values before anything is stored, so dst may be src.  A state that
// the host gives (init, set_state, an MLS update) travels in the channel's record with known == 1 and is taken by the next launch.
#include "bank_core.h"
#include "mls_device.h"
#include "randomizer_device.h"

#include <chrono>
#include <mutex>
#include <vector>

#pragma clang fp contract(off)

namespace
{
    constexpr int      BLOCK = 256;
    constexpr uint32_t PER = 4;
    constexpr uint32_t COUNT_BITS = 27;
    constexpr size_t   COUNT_LIMIT = size_t(1) << COUNT_BITS;   // 2 * count draws and the powers of M: sample indices are 32-bit
    constexpr uint32_t LCG_GROUP = 4, LCG_CHUNK = 256;          // channels per workgroup; samples per chunk: 64 lanes x 4
    constexpr uint32_t LCG_ROW = 2 * LCG_CHUNK + 4;             // draws of one channel and chunk in LDS, words
    constexpr int      LCG_BLOCK = 64 * (1 + LCG_GROUP);        // the producer's wave and a transform wave per channel
    using mi_mls::MLS_TILE; using mi_mls::MLS_TILE_LOG2; using mi_mls::MLS_TABLE_WORDS; using mi_mls::MLS_MAX_BITS;
    constexpr uint32_t MLS_SPAN_LOG2 = 2, MLS_SPAN = 1u << MLS_SPAN_LOG2;      // tiles per workgroup, one after the other
    static_assert(MLS_TILE == BLOCK * PER, "a workgroup's lanes cover one tile");
    static_assert(mi_mls::MLS_POWERS == COUNT_BITS, "the powers of M reach every count");

    struct lcg_params
    {
        uint32_t mul1[4], mul2[4], add[4];
        uint32_t last[4], buf_id, known;                        // known: vLast and nBufID are these, not the device's
        uint32_t dist;
        float    amplitude, offset;
        uint32_t enabled;                                       // 0: the row is not written and vLast, nBufID and known stay
        uint32_t pad[2];
    };
    struct lcg_state { uint32_t last[4], buf_id, pad[3]; };
    static_assert(sizeof(lcg_params) == 96 && sizeof(lcg_state) == 32, "16-byte multiples");

    struct mls_params
    {
        uint64_t state;                                         // nState where known
        uint32_t known, table;                                  // table: the register width - 1
        float    high, low;                                     // fAmplitude + fOffset, -fAmplitude + fOffset
        uint32_t enabled;                                       // 0: the row is not written and nState and known stay
        uint32_t pad;
    };
    struct mls_state { uint64_t state; };
    static_assert(sizeof(mls_params) == 32, "16-byte multiple");

    __device__ __forceinline__ uint32_t draws_per_sample(uint32_t dist)
    {
        return (dist == MI_LCG_EXPONENTIAL || dist == MI_LCG_GAUSSIAN) ? 2u : 1u;
    }

    // dst OP the four values of a lane: the rows of a call as every sample kernel here reads and writes them
    template <int OP, bool VEC>
    __device__ __forceinline__ void put4(float *dst, const float *src, size_t dst_stride, size_t src_stride, uint32_t ch, uint32_t i0, uint32_t n,
                                         float (&v)[PER])
    {
        float *out = dst + size_t(ch) * dst_stride + i0;
        const bool whole = i0 + PER <= n;
        if (OP != MI_OSC_OVERWRITE)
        {
            const float *in = src + size_t(ch) * src_stride + i0;
            float s[PER] = { 0.0f, 0.0f, 0.0f, 0.0f };
            if (VEC && whole)
            {
                const float4 q = *reinterpret_cast<const float4 *>(in);
                s[0] = q.x, s[1] = q.y, s[2] = q.z, s[3] = q.w;
            }
            else
                for (uint32_t k = 0; k < PER && i0 + k < n; ++k)
                    s[k] = in[k];
            #pragma unroll
            for (uint32_t k = 0; k < PER; ++k)
                v[k] = (OP == MI_OSC_ADD) ? s[k] + v[k] : s[k] * v[k];
        }
        if (VEC && whole)
            *reinterpret_cast<float4 *>(out) = make_float4(v[0], v[1], v[2], v[3]);
        else
            for (uint32_t k = 0; k < PER && i0 + k < n; ++k)
                out[k] = v[k];
    }

    // LCG::process_single, LCG.cpp:60-85, on the draws of four adjacent samples
    template <int DIST> __device__ __forceinline__ void lcg4(const uint32_t *row, uint32_t lane, float A, float off, float (&v)[PER])
    {
        if (DIST == MI_LCG_EXPONENTIAL || DIST == MI_LCG_GAUSSIAN)
        {
            const uint4 a = *reinterpret_cast<const uint4 *>(row + 8 * lane), b = *reinterpret_cast<const uint4 *>(row + 8 * lane + 4);
            const uint32_t d[8] = { a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w };
            #pragma unroll
            for (uint32_t k = 0; k < PER; ++k)
            {
                const float first = mi_rand::linear(d[2 * k]), second = mi_rand::linear(d[2 * k + 1]);
                if (DIST == MI_LCG_EXPONENTIAL)
                {
                    const float sign = (first >= 0.5f) ? 1.0f : -1.0f;
                    v[k] = sign * A * mi_rand::exponential(second) + off;
                }
                else
                    v[k] = A * mi_rand::gaussian(first, second) + off;
            }
        }
        else
        {
            const uint4 a = *reinterpret_cast<const uint4 *>(row + 4 * lane);
            const uint32_t d[4] = { a.x, a.y, a.z, a.w };
            #pragma unroll
            for (uint32_t k = 0; k < PER; ++k)
            {
                const float rv = mi_rand::linear(d[k]);
                v[k] = (DIST == MI_LCG_TRIANGULAR) ? 2.0f * A * mi_rand::triangle(rv) - 0.5f + off : 2.0f * A * (rv - 0.5f) + off;
            }
        }
    }

    template <int OP, bool VEC>
    __global__ __launch_bounds__(LCG_BLOCK) void lcg_kernel(float *dst, const float *src, size_t dst_stride, size_t src_stride, uint32_t count,
                                                            lcg_params *params, lcg_state *state, uint32_t channels)
    {
        __shared__ __attribute__((aligned(16))) uint32_t draws[2][LCG_GROUP * LCG_ROW];
        const uint32_t lane = threadIdx.x & 63u, ch0 = blockIdx.x * LCG_GROUP;
        const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
        const uint32_t chunks = (count + LCG_CHUNK - 1) / LCG_CHUNK;

        // wave 0, the producer's lane: channel ch0 + lane / 4, generator lane % 4
        const uint32_t pch = ch0 + (lane >> 2), g = lane & 3u;
        // a channel that is switched off: its producer lanes and its transform wave do nothing and still reach every barrier; a
        // workgroup with no channel switched on leaves as one (the four words are the same in every lane)
        bool any = false;
        for (uint32_t k = 0; k < LCG_GROUP; ++k)
            any |= ch0 + k < channels && params[ch0 + k].enabled != 0;
        if (!any)
            return;
        const bool producer = wave == 0 && lane < 4 * LCG_GROUP && pch < channels && params[pch].enabled != 0;
        uint32_t last = 0, mul1 = 0, mul2 = 0, add = 0, buf = 0, per = 1;
        // waves 1 .. LCG_GROUP, the transform: channel ch0 + wave - 1, uniform in the wave
        const uint32_t tch = ch0 + wave - 1;
        const bool transform = wave != 0 && tch < channels && params[tch].enabled != 0;
        uint32_t dist = 0;
        float A = 0.0f, off = 0.0f;
        if (producer)
        {
            const lcg_params &P = params[pch];
            const uint32_t known = P.known, given = P.last[g], given_buf = P.buf_id;
            const uint32_t kept = state[pch].last[g], kept_buf = state[pch].buf_id;
            mul1 = P.mul1[g], mul2 = P.mul2[g], add = P.add[g];
            last = known ? given : kept;
            buf = known ? given_buf : kept_buf;
            per = draws_per_sample(P.dist);
        }
        if (transform)
        {
            const lcg_params &P = params[tch];
            dist = P.dist, A = P.amplitude, off = P.offset;
        }
        if (wave == 0)
            __builtin_amdgcn_s_setprio(2);                      // the chain is the critical path of the workgroup
        // round c: the producer makes chunk c in draws[c & 1] while the transform turns chunk c - 1 in draws[(c - 1) & 1] into samples;
        // the barrier behind the round hands the one over and frees the other
        for (uint32_t c = 0; c <= chunks; ++c)
        {
            if (producer && c < chunks)
            {
                const uint32_t at = c * LCG_CHUNK, n = (count - at < LCG_CHUNK) ? count - at : LCG_CHUNK;
                const uint32_t D = per * n;                     // <= 2 * LCG_CHUNK: inside the row
                const uint32_t d0 = (g - buf) & 3u;             // this generator's first draw; every fourth one from there
                uint32_t *w = draws[c & 1u] + (lane >> 2) * LCG_ROW + d0;
                uint32_t steps = (d0 < D) ? (D - d0 + 3) / 4 : 0;
                for (; steps >= 4; steps -= 4, w += 16)         // four steps a round: the loop's own instructions are off the chain
                {
                    #pragma unroll
                    for (uint32_t k = 0; k < 4; ++k)
                    {
                        last = mi_rand::step(last, mul1, mul2, add);
                        w[4 * k] = last;
                    }
                }
                for (; steps > 0; --steps, w += 4)
                {
                    last = mi_rand::step(last, mul1, mul2, add);
                    w[0] = last;
                }
                buf = (buf + D) & 3u;
            }
            if (transform && c > 0)
            {
                const uint32_t at = (c - 1) * LCG_CHUNK, n = (count - at < LCG_CHUNK) ? count - at : LCG_CHUNK, i0 = lane * PER;
                if (i0 < n)
                {
                    const uint32_t *row = draws[(c - 1) & 1u] + (wave - 1) * LCG_ROW;
                    float v[PER];
                    switch (dist)
                    {
                        case MI_LCG_EXPONENTIAL:    lcg4<MI_LCG_EXPONENTIAL>(row, lane, A, off, v); break;
                        case MI_LCG_TRIANGULAR:     lcg4<MI_LCG_TRIANGULAR>(row, lane, A, off, v); break;
                        case MI_LCG_GAUSSIAN:       lcg4<MI_LCG_GAUSSIAN>(row, lane, A, off, v); break;
                        default:                    lcg4<MI_LCG_UNIFORM>(row, lane, A, off, v); break;
                    }
                    put4<OP, VEC>(dst, src, dst_stride, src_stride, tch, at + i0, count, v);
                }
            }
            __syncthreads();
        }
        if (producer)
        {
            state[pch].last[g] = last;
            if (g == 0)
            {
                state[pch].buf_id = buf;
                params[pch].known = 0;
            }
        }
    }

    template <int OP, bool VEC>
    __global__ __launch_bounds__(BLOCK) void mls_kernel(float *dst, const float *src, size_t dst_stride, size_t src_stride, uint32_t count,
                                                        const mls_params *__restrict__ params, const mls_state *__restrict__ state,
                                                        const uint64_t *__restrict__ tables)
    {
        const uint32_t ch = blockIdx.y, lane = threadIdx.x & 63u;
        const mls_params P = params[ch];
        if (!P.enabled)                                         // the whole workgroup: nobody is left waiting at a ballot
            return;
        const uint64_t kept = state[ch].state;                  // read whether needed or not: beside the record, not behind it
        const uint64_t *table = tables + size_t(P.table) * MLS_TABLE_WORDS;
        // the lane's rows are those of its place in a tile, the same for every tile; M^1024 takes a tile's state to the next one's
        const ulonglong2 *rows = reinterpret_cast<const ulonglong2 *>(mi_mls::rows_of(table) + threadIdx.x * PER);
        const ulonglong2 r01 = rows[0], r23 = rows[1];
        const uint64_t next = mi_mls::power_of(table, MLS_TILE_LOG2)[lane];
        // every lane of every wave forms the states: nobody leaves before the last ballot
        uint64_t s = mi_mls::jump<COUNT_BITS - MLS_TILE_LOG2 - MLS_SPAN_LOG2>(table, P.known ? P.state : kept, blockIdx.x,
                                                                              MLS_TILE_LOG2 + MLS_SPAN_LOG2, lane);
        #pragma unroll
        for (uint32_t t = 0; t < MLS_SPAN; ++t)
        {
            const uint32_t i0 = (blockIdx.x * MLS_SPAN + t) * MLS_TILE + threadIdx.x * PER;
            if (i0 < count)
            {
                float v[PER];
                v[0] = mi_mls::bit(r01.x, s) ? P.high : P.low;  // MLS.cpp:223-227
                v[1] = mi_mls::bit(r01.y, s) ? P.high : P.low;
                v[2] = mi_mls::bit(r23.x, s) ? P.high : P.low;
                v[3] = mi_mls::bit(r23.y, s) ? P.high : P.low;
                put4<OP, VEC>(dst, src, dst_stride, src_stride, ch, i0, count, v);
            }
            s = __ballot(mi_mls::bit(next, s) != 0);
        }
    }

    __global__ __launch_bounds__(64) void mls_advance_kernel(mls_params *params, mls_state *state, uint32_t count, const uint64_t *__restrict__ tables)
    {
        const uint32_t ch = blockIdx.x, lane = threadIdx.x;
        const mls_params P = params[ch];
        if (!P.enabled)
            return;
        const uint64_t kept = state[ch].state;
        const uint64_t s = mi_mls::jump<COUNT_BITS>(tables + size_t(P.table) * MLS_TABLE_WORDS, P.known ? P.state : kept, count, 0, lane);
        if (lane == 0)
        {
            state[ch].state = s;
            params[ch].known = 0;
        }
    }
} // namespace

namespace mi_mls
{
    // the tables of all 64 register widths on the current device: made at the first call, kept for the life of the process (the
    // velvet bank, csrc/velvet.hip, uses them too)
    int device_tables(const uint64_t **tables)
    {
        static std::mutex lock;
        static std::vector<uint64_t *> of_device;
        int dev = 0;
        MI_HIP_CHECK(hipGetDevice(&dev));
        std::lock_guard<std::mutex> hold(lock);
        if (size_t(dev) >= of_device.size())
            of_device.resize(size_t(dev) + 1, nullptr);
        if (of_device[dev] == nullptr)
        {
            const size_t bytes = size_t(MLS_MAX_BITS) * MLS_TABLE_WORDS * sizeof(uint64_t);
            uint64_t *d = nullptr;
            MI_HIP_CHECK(hipMalloc(reinterpret_cast<void **>(&d), bytes));
            const hipError_t e = hipMemcpy(d, mi_mls::host_tables(), bytes, hipMemcpyHostToDevice);
            if (e != hipSuccess)
            {
                (void)hipFree(d);
                MI_HIP_CHECK(e);
            }
            of_device[dev] = d;
        }
        *tables = of_device[dev];
        return MI_OK;
    }
} // namespace mi_mls
using mi_mls::device_tables;

struct mi_lcg_bank : mi_bank::tables<lcg_params, lcg_state>
{
    std::vector<uint8_t> inited;                                // init() or set_state() has given the channel a nBufID
    uint32_t             uninited = 0;                          // channels without one
    bool                 any_known = false;                     // a record carries a state that no launch has taken yet
    uint32_t             disabled = 0;                          // channels that are switched off
};

struct mi_mls_bank : mi_bank::tables<mls_params, mls_state>
{
    std::vector<mi_mls_settings_t> cfg;                         // cfg.state: nState when `issued` stood at base[channel]
    std::vector<uint64_t>   base;
    uint64_t                issued = 0;                         // samples launched by this bank, per channel
    const uint64_t         *d_tables = nullptr;                 // the device's, not the bank's
    bool                    touched = true;                     // a setter ran since the records were last made
    bool                    any_known = true;                   // a record carries a state that no launch has taken yet
    uint32_t                disabled = 0;                       // channels that are switched off
};

namespace
{
    // kernel<OP, VEC> by the call's operation and the alignment of its rows
    #define NOISE_LAUNCH(kernel, threads, op, vec, grid, st, ...) \
        do { \
            hipEvent_t ev0 = nullptr, ev1 = nullptr; \
            mi::take_profile_events(&ev0, &ev1); \
            const dim3 block(threads); \
            if (op == MI_OSC_ADD && vec)        MI_LAUNCH((kernel<MI_OSC_ADD, true>), grid, block, 0, st, ev0, ev1, __VA_ARGS__); \
            else if (op == MI_OSC_ADD)          MI_LAUNCH((kernel<MI_OSC_ADD, false>), grid, block, 0, st, ev0, ev1, __VA_ARGS__); \
            else if (op == MI_OSC_MUL && vec)   MI_LAUNCH((kernel<MI_OSC_MUL, true>), grid, block, 0, st, ev0, ev1, __VA_ARGS__); \
            else if (op == MI_OSC_MUL)          MI_LAUNCH((kernel<MI_OSC_MUL, false>), grid, block, 0, st, ev0, ev1, __VA_ARGS__); \
            else if (vec)                       MI_LAUNCH((kernel<MI_OSC_OVERWRITE, true>), grid, block, 0, st, ev0, ev1, __VA_ARGS__); \
            else                                MI_LAUNCH((kernel<MI_OSC_OVERWRITE, false>), grid, block, 0, st, ev0, ev1, __VA_ARGS__); \
        } while (0)

    // what both process entries ask of their arguments; *nothing: the call is done (count == 0)
    int process_checks(const char *entry, uint32_t channels, float *dst, const float *&src, size_t count, size_t dst_stride, size_t src_stride,
                       uint32_t op, bool *nothing)
    {
        MI_REQUIRE(op <= MI_OSC_MUL, MI_EINVAL, "%s: no operation %u", entry, op);
        if (op == MI_OSC_OVERWRITE)
            src = nullptr;
        else
            MI_REQUIRE(src != nullptr, MI_EINVAL, "%s: add and mul read src; it is NULL", entry);
        *nothing = count == 0;
        if (count == 0)
            return MI_OK;
        return mi_bank::check_rows(entry, channels, count, COUNT_LIMIT,
                                   { { dst, dst_stride, count, mi_bank::REQUIRED | mi_bank::OUTPUT }, { src, src_stride, count, 0 } });
    }

    bool rows_aligned(const float *dst, const float *src, size_t dst_stride, size_t src_stride, uint32_t channels)
    {
        return mi::aligned16(dst, dst_stride, channels) && (src == nullptr || mi::aligned16(src, src_stride, channels));
    }

    // ---- MLS: the host's copy of nState
    void resolve(mi_mls_bank *b, uint32_t ch)
    {
        if (b->base[ch] == b->issued)
            return;
        mi_mls_settings_t &c = b->cfg[ch];                      // samples were launched: feedback_bit + 1 is the width they ran at
        c.state = mi_mls::host_advance(uint32_t(c.feedback_bit) + 1, c.state, b->issued - b->base[ch]);
        b->base[ch] = b->issued;
    }

    // update_settings() of every channel, or (running: process() opens with it) of those that are switched on: nobody calls it
    // on an object that is left out, whose bSync and amplitude wait for the call that takes it in again
    int mls_update(mi_mls_bank *b, hipStream_t st, bool running = false)
    {
        if (!b->touched)                                        // a steady stream of calls: nothing to look at per channel
            return mi_bank::upload(*b, "mi_mls_bank", st);
        b->touched = false;
        for (uint32_t ch = 0; ch < b->channels; ++ch)
        {
            mi_mls_settings_t &c = b->cfg[ch];
            mls_params p = b->params[ch];
            if (running && !p.enabled)                          // what waits on it keeps the bank out of the steady path, nothing else does
            {
                const float high = c.amplitude + c.offset, low = -c.amplitude + c.offset;
                b->touched |= c.sync != 0 || memcmp(&high, &p.high, sizeof(float)) != 0 || memcmp(&low, &p.low, sizeof(float)) != 0;
                continue;
            }
            if (c.sync)
            {
                resolve(b, ch);
                mi_mls_settings_update(&c);
                p.known = 1, p.state = c.state, p.table = uint32_t(c.n_bits) - 1;
                b->any_known = true;
            }
            p.high = c.amplitude + c.offset, p.low = -c.amplitude + c.offset;      // MLS.cpp:226
            if (memcmp(&p, &b->params[ch], sizeof(p)) != 0)
                b->params[ch] = p, b->up.touch(ch);
        }
        return mi_bank::upload(*b, "mi_mls_bank", st);
    }
} // namespace

extern "C" {

// ---- LCG ---------------------------------------------------------------------------------------------------------------------------
int mi_lcg_bank_create(mi_lcg_bank_t **bank, uint32_t channels)
{
    int r = mi_bank::open(bank, "mi_lcg_bank_create", channels);
    if (r != MI_OK)
        return r;
    mi_lcg_bank *b = *bank;
    *bank = nullptr;
    b->channels = channels;
    b->inited.assign(channels, 0);
    b->uninited = channels;
    lcg_params p = lcg_params();
    p.buf_id = MI_LCG_UNSET, p.dist = MI_LCG_UNIFORM, p.amplitude = 1.0f;       // construct(): Randomizer.cpp:69-80, LCG.cpp:38-43
    p.enabled = 1;
    lcg_state s = lcg_state();
    s.buf_id = MI_LCG_UNSET;
    r = mi_bank::alloc(*b, "mi_lcg_bank_create", p, s);
    if (r != MI_OK)
    {
        mi_bank::destroy(b);
        return r;
    }
    *bank = b;
    return MI_OK;
}

int mi_lcg_bank_destroy(mi_lcg_bank_t *b)
{
    return mi_bank::destroy(b);
}

#define LCG_CHANNEL(name) \
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_lcg_bank_" name ": NULL bank"); \
    MI_REQUIRE(channel < b->channels, MI_EINVAL, "mi_lcg_bank_" name ": channel %u out of range", channel); \
    lcg_params &p = b->params[channel]

static void lcg_give(mi_lcg_bank *b, uint32_t channel, const mi_lcg_state_t &s)
{
    lcg_params &p = b->params[channel];
    memcpy(p.mul1, s.mul1, sizeof(p.mul1)); memcpy(p.mul2, s.mul2, sizeof(p.mul2)); memcpy(p.add, s.add, sizeof(p.add));
    memcpy(p.last, s.last, sizeof(p.last));
    p.buf_id = s.buf_id, p.known = 1;
    b->uninited += uint32_t(b->inited[channel]) - uint32_t(s.buf_id != MI_LCG_UNSET);
    b->inited[channel] = s.buf_id != MI_LCG_UNSET;
    b->any_known = true;
    b->up.touch(channel);
}

int mi_lcg_bank_init(mi_lcg_bank_t *b, uint32_t channel, uint32_t seed)
{
    LCG_CHANNEL("init");
    (void)p;
    mi_lcg_state_t s;
    mi_lcg_seed_words(seed, &s);
    lcg_give(b, channel, s);
    return MI_OK;
}

int mi_lcg_bank_init_time(mi_lcg_bank_t *b, uint32_t channel)                               // Randomizer.cpp:101-106
{
    const auto now = std::chrono::system_clock::now().time_since_epoch();
    const uint64_t ns = uint64_t(std::chrono::duration_cast<std::chrono::nanoseconds>(now).count());
    return mi_lcg_bank_init(b, channel, uint32_t((ns / 1000000000ull) ^ (ns % 1000000000ull)));
}

int mi_lcg_bank_set_distribution(mi_lcg_bank_t *b, uint32_t channel, uint32_t distribution)
{
    LCG_CHANNEL("set_distribution");
    if (p.dist != distribution)
        p.dist = distribution, b->up.touch(channel);
    return MI_OK;
}

int mi_lcg_bank_set_amplitude(mi_lcg_bank_t *b, uint32_t channel, float amplitude)
{
    LCG_CHANNEL("set_amplitude");
    if (memcmp(&p.amplitude, &amplitude, sizeof(float)) != 0)
        p.amplitude = amplitude, b->up.touch(channel);
    return MI_OK;
}

int mi_lcg_bank_set_offset(mi_lcg_bank_t *b, uint32_t channel, float offset)
{
    LCG_CHANNEL("set_offset");
    if (memcmp(&p.offset, &offset, sizeof(float)) != 0)
        p.offset = offset, b->up.touch(channel);
    return MI_OK;
}

int mi_lcg_bank_process(mi_lcg_bank_t *b, float *dst, const float *src, size_t count, size_t dst_stride, size_t src_stride, uint32_t op,
                        void *stream)
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_lcg_bank_process: NULL bank");
    bool nothing = false;
    int r = process_checks("mi_lcg_bank_process", b->channels, dst, src, count, dst_stride, src_stride, op, &nothing);
    if (r != MI_OK || nothing)
        return r;
    for (uint32_t ch = 0; b->uninited != 0 && ch < b->channels; ++ch)
        MI_REQUIRE(b->inited[ch] || !b->params[ch].enabled, MI_ESTATE, "mi_lcg_bank_process: channel %u was never init()ed", ch);
    if (b->disabled == b->channels)                             // nobody's process() is called
        return MI_OK;
    hipStream_t st = mi::as_stream(stream);
    r = mi_bank::upload(*b, "mi_lcg_bank", st);
    if (r != MI_OK)
        return r;
    const dim3 grid((b->channels + LCG_GROUP - 1) / LCG_GROUP);
    const bool vec = rows_aligned(dst, src, dst_stride, src_stride, b->channels);
    NOISE_LAUNCH(lcg_kernel, LCG_BLOCK, op, vec, grid, st, dst, src, dst_stride, src_stride, uint32_t(count), b->d_params, b->d_state, b->channels);
    MI_HIP_CHECK(hipGetLastError());
    bool left = false;
    for (uint32_t ch = 0; b->any_known && ch < b->channels; ++ch)  // as the kernel leaves the records
        if (b->params[ch].enabled)
            b->params[ch].known = 0;
        else
            left |= b->params[ch].known != 0;
    b->any_known = left;
    return MI_OK;
}

int mi_lcg_bank_set_row_enabled(mi_lcg_bank_t *b, uint32_t channel, int enabled)
{
    LCG_CHANNEL("set_row_enabled");
    const uint32_t on = enabled != 0;
    if (p.enabled != on)
        b->disabled += p.enabled - on, p.enabled = on, b->up.touch(channel);
    return MI_OK;
}

int mi_lcg_bank_commit(mi_lcg_bank_t *b, void *stream)
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_lcg_bank_commit: NULL bank");
    return mi_bank::upload(*b, "mi_lcg_bank", mi::as_stream(stream));
}

int mi_lcg_bank_get_state(mi_lcg_bank_t *b, uint32_t channel, mi_lcg_state_t *state, void *stream)
{
    LCG_CHANNEL("get_state");
    MI_REQUIRE(state != nullptr, MI_EINVAL, "mi_lcg_bank_get_state: NULL state");
    int r = mi::refuse_state_access(mi::as_stream(stream));
    if (r != MI_OK)
        return r;
    memcpy(state->mul1, p.mul1, sizeof(p.mul1)); memcpy(state->mul2, p.mul2, sizeof(p.mul2)); memcpy(state->add, p.add, sizeof(p.add));
    if (p.known)                                                // given by the host and not launched yet
    {
        memcpy(state->last, p.last, sizeof(p.last));
        state->buf_id = p.buf_id;
        return MI_OK;
    }
    lcg_state s;
    r = mi_bank::get_state(b, "mi_lcg_bank_get_state", channel, &s, stream);
    if (r != MI_OK)
        return r;
    memcpy(state->last, s.last, sizeof(s.last));
    state->buf_id = s.buf_id;
    return MI_OK;
}

int mi_lcg_bank_set_state(mi_lcg_bank_t *b, uint32_t channel, const mi_lcg_state_t *state, void *stream)
{
    LCG_CHANNEL("set_state");
    (void)p;
    MI_REQUIRE(state != nullptr, MI_EINVAL, "mi_lcg_bank_set_state: NULL state");
    MI_REQUIRE(state->buf_id <= 3 || state->buf_id == MI_LCG_UNSET, MI_EINVAL, "mi_lcg_bank_set_state: nBufID %u is neither 0 .. 3 nor unset",
               state->buf_id);
    const int r = mi::refuse_state_access(mi::as_stream(stream));
    if (r != MI_OK)
        return r;
    lcg_give(b, channel, *state);
    return MI_OK;
}

// ---- MLS ---------------------------------------------------------------------------------------------------------------------------
int mi_mls_bank_create(mi_mls_bank_t **bank, uint32_t channels)
{
    int r = mi_bank::open(bank, "mi_mls_bank_create", channels, 65535u);
    if (r != MI_OK)
        return r;
    mi_mls_bank *b = *bank;
    *bank = nullptr;
    b->channels = channels;
    mi_mls_settings_t fresh;
    mi_mls_settings_init(&fresh);
    b->cfg.assign(channels, fresh);
    b->base.assign(channels, 0);
    mls_params p = mls_params();
    p.known = 1, p.table = MLS_MAX_BITS - 1, p.high = 1.0f, p.low = -1.0f, p.enabled = 1;
    r = mi_bank::alloc(*b, "mi_mls_bank_create", p, mls_state{ 0 });
    if (r == MI_OK)
        r = device_tables(&b->d_tables);
    if (r != MI_OK)
    {
        mi_bank::destroy(b);
        return r;
    }
    *bank = b;
    return MI_OK;
}

int mi_mls_bank_destroy(mi_mls_bank_t *b)
{
    return mi_bank::destroy(b);
}

int mi_mls_bank_set_n_bits(mi_mls_bank_t *b, uint32_t channel, size_t n_bits)               // :114-121
{
    MI_BANK_SETTER("mls", "set_n_bits");
    b->touched = true;
    if (c.n_bits != n_bits)
        c.n_bits = n_bits, c.sync = 1;
    return MI_OK;
}

int mi_mls_bank_set_state(mi_mls_bank_t *b, uint32_t channel, uint64_t state)               // :123-130
{
    MI_BANK_SETTER("mls", "set_state");
    b->touched = true;
    resolve(b, channel);
    if (c.state != state)
        c.state = state, c.sync = 1;
    return MI_OK;
}

int mi_mls_bank_set_amplitude(mi_mls_bank_t *b, uint32_t channel, float amplitude)          // :132-138
{
    MI_BANK_SETTER("mls", "set_amplitude");
    b->touched = true;
    c.amplitude = amplitude;
    return MI_OK;
}

int mi_mls_bank_set_offset(mi_mls_bank_t *b, uint32_t channel, float offset)                // :140-146
{
    MI_BANK_SETTER("mls", "set_offset");
    b->touched = true;
    c.offset = offset;
    return MI_OK;
}

int mi_mls_bank_needs_update(const mi_mls_bank_t *b, uint32_t channel, int *yes)
{
    const int r = mi_bank::get_checks(b, "mi_mls_bank_needs_update", channel, yes);
    if (r == MI_OK)
        *yes = b->cfg[channel].sync ? 1 : 0;
    return r;
}

int mi_mls_bank_update_settings(mi_mls_bank_t *b, void *stream)
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_mls_bank_update_settings: NULL bank");
    return mls_update(b, mi::as_stream(stream));
}

int mi_mls_bank_commit(mi_mls_bank_t *b, void *stream)
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_mls_bank_commit: NULL bank");
    return mls_update(b, mi::as_stream(stream), true);
}

int mi_mls_bank_maximum_number_of_bits(const mi_mls_bank_t *b, size_t *bits)
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_mls_bank_maximum_number_of_bits: NULL bank");
    MI_REQUIRE(bits != nullptr, MI_EINVAL, "mi_mls_bank_maximum_number_of_bits: NULL result pointer");
    *bits = MLS_MAX_BITS;
    return MI_OK;
}

int mi_mls_bank_get_period(const mi_mls_bank_t *b, uint32_t channel, uint64_t *period)      // :199-206
{
    const int r = mi_bank::get_checks(b, "mi_mls_bank_get_period", channel, period);
    if (r == MI_OK)
        *period = (b->cfg[channel].n_bits >= MLS_MAX_BITS) ? ~uint64_t(0) : (uint64_t(1) << b->cfg[channel].n_bits) - 1;
    return r;
}

int mi_mls_bank_process(mi_mls_bank_t *b, float *dst, const float *src, size_t count, size_t dst_stride, size_t src_stride, uint32_t op,
                        void *stream)
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_mls_bank_process: NULL bank");
    bool nothing = false;
    int r = process_checks("mi_mls_bank_process", b->channels, dst, src, count, dst_stride, src_stride, op, &nothing);
    if (r != MI_OK || nothing)
        return r;
    hipStream_t st = mi::as_stream(stream);
    if (b->disabled == b->channels)                             // nobody's process() is called
        return MI_OK;
    r = mls_update(b, st, true);                                // progress() opens with it, :211
    if (r != MI_OK)
        return r;
    const dim3 grid(uint32_t((count + MLS_TILE * MLS_SPAN - 1) / (MLS_TILE * MLS_SPAN)), b->channels);
    const bool vec = rows_aligned(dst, src, dst_stride, src_stride, b->channels);
    NOISE_LAUNCH(mls_kernel, BLOCK, op, vec, grid, st, dst, src, dst_stride, src_stride, uint32_t(count), b->d_params, b->d_state, b->d_tables);
    MI_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(mls_advance_kernel, dim3(b->channels), dim3(64), 0, st, b->d_params, b->d_state, uint32_t(count), b->d_tables);
    MI_HIP_CHECK(hipGetLastError());
    bool left = false;
    for (uint32_t ch = 0; b->any_known && ch < b->channels; ++ch)  // as the advance kernel leaves the records
        if (b->params[ch].enabled)
            b->params[ch].known = 0;
        else
            left |= b->params[ch].known != 0;
    b->any_known = left;
    b->issued += count;                                         // every channel's nState is count samples on ...
    for (uint32_t ch = 0; b->disabled != 0 && ch < b->channels; ++ch)
        if (!b->params[ch].enabled)
            b->base[ch] += count;                               // ... but for those that stood still
    return MI_OK;
}

int mi_mls_bank_set_row_enabled(mi_mls_bank_t *b, uint32_t channel, int enabled)
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_mls_bank_set_row_enabled: NULL bank");
    MI_REQUIRE(channel < b->channels, MI_EINVAL, "mi_mls_bank_set_row_enabled: channel %u out of range", channel);
    mls_params &p = b->params[channel];
    const uint32_t on = enabled != 0;
    if (p.enabled != on)
        b->disabled += p.enabled - on, p.enabled = on, b->up.touch(channel), b->touched = true;
    return MI_OK;
}

int mi_mls_bank_reserve(mi_mls_bank_t *b, size_t count)
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_mls_bank_reserve: NULL bank");
    MI_REQUIRE(count < COUNT_LIMIT, MI_EINVAL, "mi_mls_bank_reserve: count %zu too large", count);
    return MI_OK;
}

int mi_mls_bank_get_settings(const mi_mls_bank_t *b, uint32_t channel, mi_mls_settings_t *settings)
{
    const int r = mi_bank::get_checks(b, "mi_mls_bank_get_settings", channel, settings);
    if (r != MI_OK)
        return r;
    resolve(const_cast<mi_mls_bank_t *>(b), channel);           // the same nState, written down
    *settings = b->cfg[channel];
    return MI_OK;
}

int mi_mls_bank_get_state(mi_mls_bank_t *b, uint32_t channel, uint64_t *state, void *stream)
{
    const int r = mi_bank::get_checks(b, "mi_mls_bank_get_state", channel, state);
    if (r != MI_OK)
        return r;
    if (b->cfg[channel].sync || b->params[channel].known)       // the host's word is the one in force
    {
        const int c = mi::refuse_state_access(mi::as_stream(stream));
        if (c != MI_OK)
            return c;
        resolve(b, channel);
        *state = b->cfg[channel].state;
        return MI_OK;
    }
    mls_state s;
    const int g = mi_bank::get_state(b, "mi_mls_bank_get_state", channel, &s, stream);
    if (g != MI_OK)
        return g;
    b->cfg[channel].state = s.state, b->base[channel] = b->issued;   // replays of a graph move the device's word behind the host's back
    *state = s.state;
    return MI_OK;
}

} // extern "C"
