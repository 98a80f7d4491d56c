// lsp::dspu::Depopper as a bank of `channels` depoppers (src/main/util/Depopper.cpp): a sliding RMS of the input (calc_rms,
// :443-462), a four-state automaton over the envelope (process, :464-562) and a look-ahead gain buffer into which a fade-out is
// patched BACKWARDS (apply_fadeout, :422-441); the gain leaves nLookCount = sFadeOut.nSamples + nRmsLen samples late.
//
// Both buffers are rings in device memory (power-of-two lengths, at least nRmsMin / nLookMin + TILE, so that the reference's
// "last nRmsMin squares" and "last nLookMin gains" are always there); nRmsOff and nLookOff are state words with the reference's
// values and decide nothing but where the RMS is re-summed.  depopper_kernel runs on the tile walk of tile_chain_device.h:
//     prepare          a helper wave per row: the tile's squares into the ring; per sample the pair (x, g) into LDS, g the square
//                      nRmsLen back (out of the same tile of src, or out of the ring).  Where the reference re-sums fRms before a
//                      sample (nRmsOff a multiple of 32, or at nRmsMax) the lane of that sample forms the serial sum itself,
//                      oldest first, folds it through the step and leaves -|fRms after the step| as x: a square never has its
//                      sign bit set, so the sign tells the chain to take the value as it is.  The sums do not depend on the
//                      chain, the lanes of a tile's refreshes run side by side.
//     chain            wave 0, lane r on row r:  fRms = |(fRms + x) - g|  (two dependent roundings), q = fRms * fRmsNorm, the
//                      automaton on q -- the thresholds are taken to the domain of q on the host (square_threshold), so the root
//                      is not in the chain -- and per sample a CODE for the gain: 0, 1, entry c of the fade-in table, or "event
//                      with `samples` = m".  The row becomes (fRms, code).
//     emit             env = sqrt_rn(fRms * fRmsNorm); the codes become gains in the ring (the fade-in table is read here);
//                      the tile's events are patched into the ring in order by the whole wave (64 entries at a time: times the
//                      fade-out table, zeros over nRmsLen entries, a zero at the event); then gain[i] = ring[i - nLookCount].
//                      A patch of an event at e touches nothing before e - nLookCount, so what is emitted for the samples up to
//                      the end of a tile is final once that tile's events are in: the output does not depend on how a stream is
//                      cut into calls.
// By the walk's invariant env or gain may be src: a tile of src is read (by prepare, twice: as the sample and as the square
// nRmsLen back, never from an earlier tile) before anything of that tile is stored.  Every state word goes back to the state
// array at the end, so process() is capturable.  env, gain and the state match tests/depopper_ref.py bit for bit.
//
// Settings: the setters act on the host's copy of the reference's fields; update_settings (every process call runs it) is
// reconfigure() -- the designer of host/depopper.cpp, the two tables and the parameter row to the device, and
// depopper_resum_kernel, which re-sums fRms over the new nRmsLen.  init() with new maxima zeroes the rings and the state.
#include "bank_core.h"
#include "depopper_bank.h"
#include "tile_chain_device.h"

#include <cstddef>
#include <vector>

#pragma clang fp contract(off)

namespace
{
    using namespace mi_tile_chain;

    enum { VEC_ENV = 1, VEC_GAIN = 2, VEC_SRC = 4 };
    enum : int32_t { ST_CLOSED, ST_FADE, ST_OPENED, ST_WAIT };                  // Depopper::state_t
    // what the chain leaves per sample for the gain
    enum : uint32_t { CODE_ZERO = 0, CODE_ONE = 1, CODE_TABLE = 0x80000000u, CODE_EVENT = 0xC0000000u, CODE_KIND = 0xC0000000u,
                      CODE_ARG = 0x3fffffffu };
    constexpr size_t COUNT_LIMIT = size_t(1) << 31;     // the kernel counts samples in 32 bits
    constexpr int ROW2 = 2 * TILE + 4;                  // floats of a row of pairs in LDS
    constexpr int32_t COUNTER_LIMIT = 1 << 30;          // set_state: what the 32-bit counters are asked to stay below

    struct device_params
    {
        float          *rms_ring, *look_ring;           // [rms_mask + 1] squares, [look_mask + 1] gains
        const float    *tab_in, *tab_out;               // crossfade(sFadeIn / sFadeOut, x), x = 0 .. n - 1
        uint32_t        rms_mask, look_mask;
        uint32_t        rms_min, rms_span, look_min, look_span;     // nRmsMin, nRmsMax - nRmsMin, nLookMin, nLookMax - nLookMin
        uint32_t        rms_len, look_count;            // nRmsLen, nLookCount
        float           rms_norm, q_in, q_out;          // fRmsNorm; the thresholds as squares
        int32_t         in_n, out_n, in_delay, out_delay;           // nSamples (not below 0), nDelay of both fades
        uint32_t        resum;                          // depopper_resum_kernel: re-sum fRms, once
    };
    struct device_state
    {
        float           rms;                            // fRms
        int32_t         state, counter, delay;          // nState, nCounter, nDelay
        uint32_t        rms_off, look_off;              // nRmsOff, nLookOff
        uint32_t        rms_pos, look_pos;              // where the next square and the next gain go in the rings
    };
    struct chain_regs { float rms; int32_t state, counter, delay; };
    struct chain_params { float norm, q_in, q_out; int32_t in_n, out_n, in_delay, out_delay; };

    // as sidechain.hip's: the correctly rounded float32 root through float64
    __device__ __forceinline__ float sqrt_rn(float q)
    {
        return float(__builtin_sqrt(double(q)));
    }

    // nRmsOff / nLookOff after n more samples: they run from lo + 1 to lo + span and start over (:446-450, :472-478)
    __host__ __device__ __forceinline__ uint32_t advance(uint32_t off, uint32_t n, uint32_t lo, uint32_t span)
    {
        return (n == 0) ? off : lo + (off - lo + n - 1u) % span + 1u;
    }

    // a sample as the ring holds it: s * s without a NaN's sign (the chain reads the sign bit as "refreshed")
    __device__ __forceinline__ float square(float s)
    {
        return __uint_as_float(__float_as_uint(s * s) & 0x7fffffffu);
    }

    // One tile of one channel, :487-549 with calc_rms's step.  A function of its own so that its instructions can be looked at.
    __device__ __noinline__ chain_regs depopper_chain_tile(lds_float *row, uint32_t n, chain_regs s, const chain_params p)
    {
        float rms = s.rms;
        int32_t st = s.state, counter = s.counter, delay = s.delay;
        auto step = [&](float &x, float &g)
        {
            const float t = fabsf((rms + x) - g);                               // :459
            rms = (__float_as_uint(x) >> 31) ? fabsf(x) : t;                    // ... or the refreshed sum through the same step
            const float q = rms * p.norm;                                       // sqrtf(q) is emit's
            const bool below_out = q < p.q_out;                                 // s < sFadeOut.fThresh
            uint32_t code;
            if (st == ST_CLOSED)                                                // :492-502
            {
                code = CODE_ZERO;
                if (!(q < p.q_in))
                {
                    delay = p.in_delay;
                    st = ST_FADE;
                    code = (0 >= p.in_n) ? CODE_ONE : CODE_TABLE;               // crossfade(&sFadeIn, 0)
                    counter = 1;
                }
            }
            else if (st == ST_FADE)                                             // :504-524
            {
                code = (counter >= p.in_n) ? CODE_ONE : (CODE_TABLE | uint32_t(counter));
                ++counter;
                if (below_out)
                {
                    if ((--delay) <= 0)
                    {
                        if (p.out_n > 0)                                        // apply_fadeout(&gbuf[i], nCounter)
                            code = CODE_EVENT | uint32_t((counter < p.out_n) ? counter : p.out_n);
                        counter = 0;
                        st = ST_WAIT;
                    }
                }
                else
                {
                    delay = p.in_delay;
                    if (counter >= p.in_n)
                        st = ST_OPENED;
                }
            }
            else if (st == ST_OPENED)                                           // :526-538
            {
                code = CODE_ONE;
                if (counter < p.out_n)
                    ++counter;
                if (below_out)
                {
                    if (p.out_n > 0)
                        code = CODE_EVENT | uint32_t((counter < p.out_n) ? counter : p.out_n);
                    st = ST_WAIT;
                    delay = p.out_delay;
                }
            }
            else                                                                // :540-544
            {
                code = CODE_ZERO;
                if ((--delay) <= 0)
                    st = ST_CLOSED;
            }
            x = rms;
            g = __uint_as_float(code);
        };
        uint32_t i = 0;
        if (n >= 4)
        {
            f32x4 a = *reinterpret_cast<lds_f32x4 *>(row), b = *reinterpret_cast<lds_f32x4 *>(row + 4);
            for (; i + 4 <= n; i += 4)
            {
                float v[8] = { a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w };
                const uint32_t next = (i + 8 <= n) ? i + 4 : i;                 // the next four pairs, before this batch's chain
                a = *reinterpret_cast<lds_f32x4 *>(row + 2 * next);
                b = *reinterpret_cast<lds_f32x4 *>(row + 2 * next + 4);
                #pragma unroll
                for (int j = 0; j < 4; ++j)
                    step(v[2 * j], v[2 * j + 1]);
                *reinterpret_cast<lds_f32x4 *>(row + 2 * i) = f32x4{ v[0], v[1], v[2], v[3] };
                *reinterpret_cast<lds_f32x4 *>(row + 2 * i + 4) = f32x4{ v[4], v[5], v[6], v[7] };
            }
        }
        for (; i < n; ++i)
        {
            float x = row[2 * i], g = row[2 * i + 1];
            step(x, g);
            row[2 * i] = x, row[2 * i + 1] = g;
        }
        return chain_regs{ rms, st, counter, delay };
    }

    __global__ __launch_bounds__(BLOCK) void depopper_kernel(float *env, float *gain, const float *src, size_t env_stride,
                                                             size_t gain_stride, size_t src_stride, uint32_t count, uint32_t channels,
                                                             const device_params *params, device_state *state, uint32_t vec)
    {
        __shared__ __attribute__((aligned(16))) float tile[2][GROUP][ROW2];     // (x, g), then (fRms, code), pair by pair
        const role me = my_role(channels);
        const uint32_t r = me.r, ch = me.ch, c = me.c;
        device_params p = {};
        device_state s0 = {};
        if (me.valid)
        {
            p = params[ch];
            s0 = state[ch];
        }
        const float *xs = src + size_t(ch) * src_stride;
        float *es = (env != nullptr) ? env + size_t(ch) * env_stride : nullptr;
        float *gs = gain + size_t(ch) * gain_stride;
        const uint32_t len = p.rms_len;

        auto prepare_tile = [&](uint32_t k)
        {
            const extent t = tile_extent(count, k);
            if (c >= t.n)
                return;
            float x[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
            if ((vec & VEC_SRC) && c + 4 <= t.n)
            {
                const float4 v = *reinterpret_cast<const float4 *>(xs + t.t0 + c);
                x[0] = v.x, x[1] = v.y, x[2] = v.z, x[3] = v.w;
            }
            else
            {
                #pragma unroll
                for (uint32_t j = 0; j < 4; ++j)
                    if (c + j < t.n)
                        x[j] = xs[t.t0 + c + j];
            }
            const uint32_t at = s0.rms_pos + t.t0;                              // the tile's first square in the ring (before the mask)
            uint32_t seen = advance(s0.rms_off, t.t0 + c, p.rms_min, p.rms_span);      // nRmsOff as calc_rms finds it at sample c
            lds_float *row = (lds_float *)&tile[k & 1][r][0];
            #pragma unroll
            for (uint32_t j = 0; j < 4; ++j)
            {
                const uint32_t i = c + j;
                if (i >= t.n)
                    break;
                const bool wrap = seen >= p.rms_min + p.rms_span;               // :446
                const bool refresh = wrap || (seen & 0x1fu) == 0;               // :454
                seen = (wrap ? p.rms_min : seen) + 1u;
                const float s2 = square(x[j]);
                const float g = (i >= len) ? square(xs[t.t0 + i - len]) : p.rms_ring[(at + i - len) & p.rms_mask];
                p.rms_ring[(at + i) & p.rms_mask] = s2;
                float v = s2;
                if (refresh)
                {
                    // dsp::h_sum over the last nRmsLen squares, oldest first, one lane: first what is older than the tile
                    float acc = 0.0f;
                    const uint32_t old = (i >= len) ? 0u : len - i;
                    for (uint32_t u = 0; u < old; ++u)
                        acc += p.rms_ring[(at + i - len + u) & p.rms_mask];
                    const float *from = xs + t.t0 + i - (len - old);
                    #pragma unroll 8
                    for (uint32_t u = 0; u < len - old; ++u)
                        acc += square(from[u]);
                    v = __uint_as_float(__float_as_uint((acc + s2) - g) | 0x80000000u);
                }
                row[2 * i] = v;
                row[2 * i + 1] = g;
            }
        };

        auto emit_tile = [&](uint32_t k)
        {
            const extent t = tile_extent(count, k);
            const lds_float *row = (const lds_float *)&tile[k & 1][r][0];
            const f32x4 a = *reinterpret_cast<const lds_f32x4 *>(row + 2 * c), b = *reinterpret_cast<const lds_f32x4 *>(row + 2 * c + 4);
            const float fr[4] = { a.x, a.z, b.x, b.z };
            const uint32_t code[4] = { __float_as_uint(a.y), __float_as_uint(a.w), __float_as_uint(b.y), __float_as_uint(b.w) };
            if (es != nullptr && c < t.n)
            {
                float e[4];
                #pragma unroll
                for (uint32_t j = 0; j < 4; ++j)
                    e[j] = sqrt_rn(fr[j] * p.rms_norm);                         // :461
                store_quad(es + t.t0 + c, e, vec & VEC_ENV, c, t.n);
            }
            // the gains as the automaton wrote them (an event's own entry is the zero of :432)
            const uint32_t at = s0.look_pos + t.t0;
            uint32_t events = 0;
            #pragma unroll
            for (uint32_t j = 0; j < 4; ++j)
            {
                if (c + j >= t.n)
                    break;
                const uint32_t kind = code[j] & CODE_KIND;
                float v = (code[j] == CODE_ONE) ? 1.0f : 0.0f;
                if (kind == CODE_TABLE)
                    v = p.tab_in[code[j] & CODE_ARG];
                events |= (kind == CODE_EVENT) ? (1u << j) : 0u;
                p.look_ring[(at + c + j) & p.look_mask] = v;
            }
            // apply_fadeout of every event of the tile, in order, the whole wave on each
            unsigned long long waiting = __ballot(events != 0);
            while (waiting != 0)
            {
                const int lane = __ffsll(waiting) - 1;
                waiting &= waiting - 1;
                const uint32_t which = __shfl(events, lane);
                #pragma unroll
                for (uint32_t j = 0; j < 4; ++j)
                {
                    const uint32_t m = __shfl(code[j], lane) & CODE_ARG;        // `samples`, at most sFadeOut.nSamples
                    if (!((which >> j) & 1u))
                        continue;
                    __threadfence_block();                                      // the entries as the wave has left them so far
                    const uint32_t event = at + uint32_t(lane) * 4 + j;
                    const uint32_t first = event - len - m;
                    for (uint32_t u = me.lane; u < m; u += 64)                  // :436-437
                    {
                        float *entry = &p.look_ring[(first + u) & p.look_mask];
                        *entry = *entry * p.tab_out[uint32_t(p.out_n) - m + u];
                    }
                    for (uint32_t u = me.lane; u <= len; u += 64)               // :440, and :432
                        p.look_ring[(event - len + u) & p.look_mask] = 0.0f;
                }
            }
            __threadfence_block();
            if (c < t.n)
            {
                float y[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
                #pragma unroll
                for (uint32_t j = 0; j < 4; ++j)
                    if (c + j < t.n)
                        y[j] = p.look_ring[(at + c + j - p.look_count) & p.look_mask];     // :553
                store_quad(gs + t.t0 + c, y, vec & VEC_GAIN, c, t.n);
            }
        };

        chain_regs regs = { s0.rms, s0.state, s0.counter, s0.delay };
        const chain_params cp = { p.rms_norm, p.q_in, p.q_out, p.in_n, p.out_n, p.in_delay, p.out_delay };
        MI_TILE_CHAIN_WALK(me, count, k, prepare_tile(k),
                           regs = depopper_chain_tile((lds_float *)&tile[k & 1][r][0], tile_extent(count, k).n, regs, cp),
                           emit_tile(k));
        if (me.valid && me.chain)
        {
            device_state s = s0;
            s.rms = regs.rms, s.state = regs.state, s.counter = regs.counter, s.delay = regs.delay;
            s.rms_off = advance(s0.rms_off, count, p.rms_min, p.rms_span);
            s.look_off = advance(s0.look_off, count, p.look_min, p.look_span);
            s.rms_pos = (s0.rms_pos + count) & p.rms_mask;
            s.look_pos = (s0.look_pos + count) & p.look_mask;
            state[ch] = s;
        }
    }

    // reconfigure()'s fRms = dsp::h_sum(&pRmsBuf[nRmsOff - nRmsLen], nRmsLen) (:267) of the channels whose row says so
    __global__ __launch_bounds__(64) void depopper_resum_kernel(device_params *params, device_state *state, uint32_t lo, uint32_t hi)
    {
        const uint32_t ch = lo + blockIdx.x * 64 + threadIdx.x;
        if (ch >= hi || params[ch].resum == 0)
            return;
        const device_params p = params[ch];
        const uint32_t pos = state[ch].rms_pos;
        float acc = 0.0f;
        for (uint32_t u = 0; u < p.rms_len; ++u)
            acc += p.rms_ring[(pos - p.rms_len + u) & p.rms_mask];
        state[ch].rms = acc;
        params[ch].resum = 0;
    }

    struct channel_host
    {
        mi_depopper::unit       u;
        std::vector<float>      tab_in, tab_out;
        float                  *d_rings = nullptr;      // the RMS ring, then the gain ring
        uint32_t                rms_cap = 0, look_cap = 0;
        float                  *d_tabs = nullptr;       // the fade-in table, then the fade-out table
        size_t                  tab_cap = 0;
        bool                    start_over = false;     // init() with new extents: rings and state are zeroed by the next update
    };

    uint32_t ring_length(int64_t least)
    {
        uint32_t n = 1;
        while (int64_t(n) < least + TILE)
            n <<= 1;
        return n;
    }
} // namespace

struct mi_depopper_bank : mi_bank::tables<device_params, device_state>
{
    static constexpr const char *NAME = "mi_depopper_bank";
    std::vector<channel_host>   ch;
};

namespace
{
    // update_settings: reconfigure() of every channel that asks for it
    int depopper_update(mi_depopper_bank *b, const char *entry, hipStream_t st)
    {
        bool any = false;
        for (const channel_host &h : b->ch)
            any = any || h.u.bReconfigure || h.start_over;
        if (!any)
            return MI_OK;
        const int cap = mi::refuse_capture(mi_depopper_bank::NAME, st);
        if (cap != MI_OK)
            return cap;
        // first the designer on copies, which touches nothing of the bank: a channel that the reference could not run refuses the
        // call, and every channel's designed fields, tables and latency stay what the device runs
        std::vector<mi_depopper::unit> designed;
        for (uint32_t c = 0; c < b->channels; ++c)
        {
            const channel_host &h = b->ch[c];
            if (!h.u.bReconfigure && !h.start_over)
                continue;
            designed.push_back(h.u);
            const char *why = mi_depopper::reconfigure(designed.back());
            MI_REQUIRE(why == nullptr, MI_EINVAL, "%s: channel %u: %s", entry, c, why);
        }
        size_t taken = 0;
        std::vector<device_state> fresh(b->channels);
        uint32_t lo = b->channels, hi = 0;
        for (uint32_t c = 0; c < b->channels; ++c)
        {
            channel_host &h = b->ch[c];
            if (!h.u.bReconfigure && !h.start_over)
                continue;
            h.u = designed[taken++];
            const mi_depopper::unit &u = h.u;
            device_params &p = b->params[c];
            if (h.start_over)
            {
                const uint32_t rms_cap = ring_length(u.nRmsMin), look_cap = ring_length(u.nLookMin);
                if (h.d_rings == nullptr || rms_cap != h.rms_cap || look_cap != h.look_cap)
                {
                    (void)hipFree(h.d_rings);                                   // waits for whatever still reads them
                    h.d_rings = nullptr;
                    MI_HIP_CHECK(hipMalloc(reinterpret_cast<void **>(&h.d_rings), (size_t(rms_cap) + look_cap) * sizeof(float)));
                    h.rms_cap = rms_cap, h.look_cap = look_cap;
                }
                MI_HIP_CHECK(hipMemsetAsync(h.d_rings, 0, (size_t(rms_cap) + look_cap) * sizeof(float), st));
                // :131-147: nState, both offsets and the buffers; nCounter and nDelay stay what they are
                const int got = mi::read_state(&fresh[c], b->d_state + c, st);
                if (got != MI_OK)
                    return got;
                fresh[c] = device_state{ 0.0f, ST_CLOSED, fresh[c].counter, fresh[c].delay, uint32_t(u.nRmsMin), uint32_t(u.nLookMin), 0, 0 };
                MI_HIP_CHECK(hipMemcpyAsync(b->d_state + c, &fresh[c], sizeof(device_state), hipMemcpyHostToDevice, st));
            }
            mi_depopper::tabulate(u.sFadeIn, h.tab_in);
            mi_depopper::tabulate(u.sFadeOut, h.tab_out);
            const size_t need = h.tab_in.size() + h.tab_out.size();
            if (need > h.tab_cap)
            {
                (void)hipFree(h.d_tabs);
                h.d_tabs = nullptr, h.tab_cap = 0;
                MI_HIP_CHECK(hipMalloc(reinterpret_cast<void **>(&h.d_tabs), need * sizeof(float)));
                h.tab_cap = need;
            }
            if (!h.tab_in.empty())
                MI_HIP_CHECK(hipMemcpyAsync(h.d_tabs, h.tab_in.data(), h.tab_in.size() * sizeof(float), hipMemcpyHostToDevice, st));
            if (!h.tab_out.empty())
                MI_HIP_CHECK(hipMemcpyAsync(h.d_tabs + h.tab_in.size(), h.tab_out.data(), h.tab_out.size() * sizeof(float),
                                            hipMemcpyHostToDevice, st));
            p.rms_ring = h.d_rings, p.look_ring = h.d_rings + h.rms_cap;
            p.tab_in = h.d_tabs, p.tab_out = (h.d_tabs != nullptr) ? h.d_tabs + h.tab_in.size() : nullptr;
            p.rms_mask = h.rms_cap - 1, p.look_mask = h.look_cap - 1;
            p.rms_min = uint32_t(u.nRmsMin), p.rms_span = uint32_t(u.nRmsMax - u.nRmsMin);
            p.look_min = uint32_t(u.nLookMin), p.look_span = uint32_t(u.nLookMax - u.nLookMin);
            p.rms_len = uint32_t(u.nRmsLen), p.look_count = uint32_t(u.nLookCount);
            p.rms_norm = u.fRmsNorm;
            p.q_in = mi_depopper::square_threshold(u.sFadeIn.fThresh), p.q_out = mi_depopper::square_threshold(u.sFadeOut.fThresh);
            p.in_n = int32_t((u.sFadeIn.nSamples > 0) ? u.sFadeIn.nSamples : 0);
            p.out_n = int32_t((u.sFadeOut.nSamples > 0) ? u.sFadeOut.nSamples : 0);
            p.in_delay = int32_t(u.sFadeIn.nDelay), p.out_delay = int32_t(u.sFadeOut.nDelay);
            p.resum = 1;
            b->up.touch(c);
            lo = (c < lo) ? c : lo, hi = (c + 1 > hi) ? c + 1 : hi;
        }
        const int r = mi_bank::upload(*b, mi_depopper_bank::NAME, st);         // waits: tables, states and rows are on the device
        if (r != MI_OK)
            return r;
        hipLaunchKernelGGL(depopper_resum_kernel, dim3((hi - lo + 63) / 64), dim3(64), 0, st, b->d_params, b->d_state, lo, hi);
        MI_HIP_CHECK(hipGetLastError());
        for (uint32_t c = lo; c < hi; ++c)
        {
            b->params[c].resum = 0;                                             // as the kernel leaves the device's row
            b->ch[c].u.bReconfigure = false, b->ch[c].start_over = false;
        }
        return MI_OK;
    }

    int channel_checks(const mi_depopper_bank *b, const char *entry, uint32_t channel)
    {
        MI_REQUIRE(b != nullptr, MI_ESTATE, "%s: NULL bank", entry);
        MI_REQUIRE(channel < b->channels, MI_EINVAL, "%s: channel %u out of range", entry, channel);
        return MI_OK;
    }

    void put_fade(mi_depopper_fade_t &d, const mi_depopper::fade_t &f)
    {
        d.mode = f.enMode, d.threshold = f.fThresh, d.time = f.fTime, d.delay = f.fDelay;
        d.samples = f.nSamples, d.delay_samples = f.nDelay;
        memcpy(d.poly, f.fPoly, sizeof(d.poly));
    }

    // the setters' fields as given (not through the setters, whose compares depend on what was set before); the RMS length clamped
    void take_settings(mi_depopper::unit &u, const mi_depopper_params_t &s)
    {
        const mi_depopper_fade_t *from[2] = { &s.fade_in, &s.fade_out };
        mi_depopper::fade_t *to[2] = { &u.sFadeIn, &u.sFadeOut };
        for (int k = 0; k < 2; ++k)
            to[k]->enMode = from[k]->mode, to[k]->fThresh = from[k]->threshold, to[k]->fTime = from[k]->time, to[k]->fDelay = from[k]->delay;
        u.fRmsLength = (s.rms_length < 0.0f) ? 0.0f : ((s.rms_length > u.fRmsMax) ? u.fRmsMax : s.rms_length);     // :370
        u.bReconfigure = true;
    }

    void put_params(mi_depopper_params_t *params, const mi_depopper::unit &u, bool pending)
    {
        put_fade(params->fade_in, u.sFadeIn);
        put_fade(params->fade_out, u.sFadeOut);
        params->sample_rate = u.nSampleRate;
        params->look_max = u.fLookMax, params->rms_max = u.fRmsMax, params->rms_length = u.fRmsLength, params->rms_norm = u.fRmsNorm;
        params->look_min_off = u.nLookMin, params->look_max_off = u.nLookMax, params->look_count = u.nLookCount;
        params->rms_min_off = u.nRmsMin, params->rms_max_off = u.nRmsMax, params->rms_len = u.nRmsLen;
        params->reconfigure = pending ? 1u : 0u;
    }
} // namespace

#define MI_DEPOPPER_SETTER(name) \
    const int r_ = channel_checks(b, "mi_depopper_bank_" name, channel); \
    if (r_ != MI_OK) \
        return r_; \
    mi_depopper::unit &u = b->ch[channel].u

extern "C" {

int mi_depopper_compute_extents(uint64_t sample_rate, float max_fade, float max_rms, mi_depopper_params_t *extents)    // :108-151
{
    MI_REQUIRE(extents != nullptr, MI_EINVAL, "mi_depopper_compute_extents: bad argument");
    mi_depopper::unit u;
    mi_depopper::construct(u);
    const char *why = nullptr;
    MI_REQUIRE(mi_depopper::init(u, sample_rate, max_fade, max_rms, &why) >= 0, MI_EINVAL, "mi_depopper_compute_extents: %s", why);
    put_params(extents, u, true);
    return MI_OK;
}

int mi_depopper_square_threshold(float threshold, float *square)
{
    MI_REQUIRE(square != nullptr, MI_EINVAL, "mi_depopper_square_threshold: bad argument");
    *square = mi_depopper::square_threshold(threshold);
    return MI_OK;
}

int mi_depopper_compute_params(const mi_depopper_params_t *settings, mi_depopper_params_t *designed, float *table_in, size_t in_capacity,
                               float *table_out, size_t out_capacity)
{
    MI_REQUIRE(settings != nullptr && designed != nullptr, MI_EINVAL, "mi_depopper_compute_params: bad argument");
    const mi_depopper_params_t given = *settings;           // (designed may be settings)
    settings = &given;
    designed->reconfigure = 1;                              // nothing designed yet
    MI_REQUIRE(settings->fade_in.mode <= MI_DEPOPPER_PARABOLIC && settings->fade_out.mode <= MI_DEPOPPER_PARABOLIC, MI_EINVAL,
               "mi_depopper_compute_params: modes %u, %u", settings->fade_in.mode, settings->fade_out.mode);
    mi_depopper::unit u;
    mi_depopper::construct(u);
    const char *why = nullptr;
    MI_REQUIRE(mi_depopper::init(u, settings->sample_rate, settings->look_max, settings->rms_max, &why) >= 0, MI_EINVAL,
               "mi_depopper_compute_params: %s", why);
    take_settings(u, *settings);
    bool written = false;
    why = mi_depopper::reconfigure(u, &written);
    put_params(designed, u, !written);
    MI_REQUIRE(why == nullptr, MI_EINVAL, "mi_depopper_compute_params: %s", why);
    std::vector<float> t;
    mi_depopper::tabulate(u.sFadeIn, t);
    if (table_in != nullptr)
        memcpy(table_in, t.data(), ((t.size() < in_capacity) ? t.size() : in_capacity) * sizeof(float));
    mi_depopper::tabulate(u.sFadeOut, t);
    if (table_out != nullptr)
        memcpy(table_out, t.data(), ((t.size() < out_capacity) ? t.size() : out_capacity) * sizeof(float));
    return MI_OK;
}

int mi_depopper_bank_create(mi_depopper_bank_t **bank, uint32_t channels)                                    // :44-94
{
    int r = mi_bank::open(bank, "mi_depopper_bank_create", channels);
    if (r != MI_OK)
        return r;
    mi_depopper_bank *b = *bank;
    b->channels = channels;
    b->ch.resize(channels);
    for (channel_host &h : b->ch)
        mi_depopper::construct(h.u);
    r = mi_bank::alloc(*b, "mi_depopper_bank_create", device_params{}, device_state{});
    if (r != MI_OK)
    {
        *bank = nullptr;
        mi_depopper_bank_destroy(b);
    }
    return r;
}

int mi_depopper_bank_destroy(mi_depopper_bank_t *b)
{
    if (b == nullptr)
        return MI_OK;
    for (channel_host &h : b->ch)
    {
        (void)hipFree(h.d_rings);
        (void)hipFree(h.d_tabs);
    }
    return mi_bank::destroy(b);
}

int mi_depopper_bank_init(mi_depopper_bank_t *b, uint32_t channel, uint64_t sample_rate, float max_fade, float max_rms)   // :108-151
{
    MI_DEPOPPER_SETTER("init");
    const char *why = nullptr;
    const int changed = mi_depopper::init(u, sample_rate, max_fade, max_rms, &why);
    MI_REQUIRE(changed >= 0, MI_EINVAL, "mi_depopper_bank_init: channel %u: %s", channel, why);
    if (changed > 0)
        b->ch[channel].start_over = true;
    return MI_OK;
}

int mi_depopper_bank_set_fade_in_mode(mi_depopper_bank_t *b, uint32_t channel, uint32_t mode, uint32_t *old)
{
    MI_DEPOPPER_SETTER("set_fade_in_mode");
    MI_REQUIRE(mode <= MI_DEPOPPER_PARABOLIC, MI_EINVAL, "mi_depopper_bank_set_fade_in_mode: mode %u", mode);
    const uint32_t was = mi_depopper::set_fade_mode(u, true, mode);
    if (old != nullptr)
        *old = was;
    return MI_OK;
}

int mi_depopper_bank_set_fade_out_mode(mi_depopper_bank_t *b, uint32_t channel, uint32_t mode, uint32_t *old)
{
    MI_DEPOPPER_SETTER("set_fade_out_mode");
    MI_REQUIRE(mode <= MI_DEPOPPER_PARABOLIC, MI_EINVAL, "mi_depopper_bank_set_fade_out_mode: mode %u", mode);
    const uint32_t was = mi_depopper::set_fade_mode(u, false, mode);
    if (old != nullptr)
        *old = was;
    return MI_OK;
}

#define MI_DEPOPPER_FLOAT_SETTER(name, call) \
    int mi_depopper_bank_##name(mi_depopper_bank_t *b, uint32_t channel, float value, float *old) \
    { \
        MI_DEPOPPER_SETTER(#name); \
        const float was = call; \
        if (old != nullptr) \
            *old = was; \
        return MI_OK; \
    }

MI_DEPOPPER_FLOAT_SETTER(set_fade_in_time, mi_depopper::set_fade_in_time(u, value))
MI_DEPOPPER_FLOAT_SETTER(set_fade_out_time, mi_depopper::set_fade_out_time(u, value))
MI_DEPOPPER_FLOAT_SETTER(set_fade_in_threshold, mi_depopper::set_fade_threshold(u, true, value))
MI_DEPOPPER_FLOAT_SETTER(set_fade_out_threshold, mi_depopper::set_fade_threshold(u, false, value))
MI_DEPOPPER_FLOAT_SETTER(set_fade_in_delay, mi_depopper::set_fade_in_delay(u, value))
MI_DEPOPPER_FLOAT_SETTER(set_fade_out_delay, mi_depopper::set_fade_out_delay(u, value))
MI_DEPOPPER_FLOAT_SETTER(set_rms_length, mi_depopper::set_rms_length(u, value))

int mi_depopper_bank_set_settings(mi_depopper_bank_t *b, uint32_t channel, const mi_depopper_params_t *settings)
{
    MI_DEPOPPER_SETTER("set_settings");
    MI_REQUIRE(settings != nullptr, MI_EINVAL, "mi_depopper_bank_set_settings: NULL settings");
    MI_REQUIRE(settings->fade_in.mode <= MI_DEPOPPER_PARABOLIC && settings->fade_out.mode <= MI_DEPOPPER_PARABOLIC, MI_EINVAL,
               "mi_depopper_bank_set_settings: modes %u, %u", settings->fade_in.mode, settings->fade_out.mode);
    const char *why = nullptr;
    const int changed = mi_depopper::init(u, settings->sample_rate, settings->look_max, settings->rms_max, &why);
    MI_REQUIRE(changed >= 0, MI_EINVAL, "mi_depopper_bank_set_settings: channel %u: %s", channel, why);
    if (changed > 0)
        b->ch[channel].start_over = true;
    mi_depopper_params_t now;
    put_params(&now, u, false);
    const bool same = memcmp(&now.fade_in, &settings->fade_in, offsetof(mi_depopper_fade_t, samples)) == 0 &&
                      memcmp(&now.fade_out, &settings->fade_out, offsetof(mi_depopper_fade_t, samples)) == 0 &&
                      memcmp(&now.rms_length, &settings->rms_length, sizeof(float)) == 0;
    if (!same || settings->reconfigure != 0)
        take_settings(u, *settings);
    return MI_OK;
}

int mi_depopper_bank_update_settings(mi_depopper_bank_t *b, void *stream)                                    // :254-270
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_depopper_bank_update_settings: NULL bank");
    return depopper_update(b, "mi_depopper_bank_update_settings", mi::as_stream(stream));
}

int mi_depopper_bank_get_params(const mi_depopper_bank_t *b, uint32_t channel, mi_depopper_params_t *params)
{
    const int r = mi_bank::get_checks(b, "mi_depopper_bank_get_params", channel, params);
    if (r != MI_OK)
        return r;
    put_params(params, b->ch[channel].u, b->ch[channel].u.bReconfigure || b->ch[channel].start_over);
    return MI_OK;
}

int mi_depopper_bank_get_fade_table(const mi_depopper_bank_t *b, uint32_t channel, uint32_t fade_out, float *table, size_t capacity,
                                    size_t *count)
{
    const int r = mi_bank::get_checks(b, "mi_depopper_bank_get_fade_table", channel, count);
    if (r != MI_OK)
        return r;
    const std::vector<float> &t = fade_out ? b->ch[channel].tab_out : b->ch[channel].tab_in;
    *count = t.size();
    if (table != nullptr)
        memcpy(table, t.data(), ((t.size() < capacity) ? t.size() : capacity) * sizeof(float));
    return MI_OK;
}

int mi_depopper_bank_latency(const mi_depopper_bank_t *b, uint32_t channel, int64_t *samples)
{
    const int r = mi_bank::get_checks(b, "mi_depopper_bank_latency", channel, samples);
    if (r == MI_OK)
        *samples = b->ch[channel].u.sFadeOut.nSamples;
    return r;
}

int mi_depopper_bank_get_state(mi_depopper_bank_t *b, uint32_t channel, mi_depopper_state_t *state, float *rms_buf, float *gain_buf,
                               void *stream)
{
    device_state s;
    hipStream_t st = mi::as_stream(stream);
    int r = mi_bank::get_checks(b, "mi_depopper_bank_get_state", channel, state);
    if (r == MI_OK)
        r = mi::refuse_state_access(st);
    if (r == MI_OK)
        r = depopper_update(b, "mi_depopper_bank_get_state", st);
    if (r == MI_OK)
        r = mi_bank::get_state(b, "mi_depopper_bank_get_state", channel, &s, stream);
    if (r != MI_OK)
        return r;
    state->rms = s.rms, state->state = uint32_t(s.state), state->counter = s.counter, state->delay = s.delay;
    state->rms_off = s.rms_off, state->look_off = s.look_off;
    const channel_host &h = b->ch[channel];
    if (rms_buf != nullptr || gain_buf != nullptr)
    {
        std::vector<float> rings(size_t(h.rms_cap) + h.look_cap);
        MI_HIP_CHECK(hipMemcpyAsync(rings.data(), h.d_rings, rings.size() * sizeof(float), hipMemcpyDeviceToHost, st));
        MI_HIP_CHECK(hipStreamSynchronize(st));
        const uint32_t rms_min = uint32_t(h.u.nRmsMin), look_min = uint32_t(h.u.nLookMin);
        for (uint32_t i = 0; rms_buf != nullptr && i < rms_min; ++i)
            rms_buf[i] = rings[(s.rms_pos - rms_min + i) & (h.rms_cap - 1)];
        for (uint32_t i = 0; gain_buf != nullptr && i < look_min; ++i)
            gain_buf[i] = rings[h.rms_cap + ((s.look_pos - look_min + i) & (h.look_cap - 1))];
    }
    return MI_OK;
}

int mi_depopper_bank_set_state(mi_depopper_bank_t *b, uint32_t channel, const mi_depopper_state_t *state, const float *rms_buf,
                               const float *gain_buf, void *stream)
{
    int r = channel_checks(b, "mi_depopper_bank_set_state", channel);
    if (r != MI_OK)
        return r;
    MI_REQUIRE(state != nullptr, MI_EINVAL, "mi_depopper_bank_set_state: NULL state");
    hipStream_t st = mi::as_stream(stream);
    r = mi::refuse_state_access(st);
    if (r == MI_OK)
        r = depopper_update(b, "mi_depopper_bank_set_state", st);       // what was set before this call does not undo it
    if (r != MI_OK)
        return r;
    const channel_host &h = b->ch[channel];
    const mi_depopper::unit &u = h.u;
    MI_REQUIRE(state->state <= uint32_t(ST_WAIT) && state->counter >= 0 && state->counter < COUNTER_LIMIT &&
               state->delay > -COUNTER_LIMIT && state->delay < COUNTER_LIMIT, MI_EINVAL,
               "mi_depopper_bank_set_state: a state of %u, a counter of %lld or a delay of %lld", state->state,
               (long long)state->counter, (long long)state->delay);
    MI_REQUIRE(state->rms_off >= u.nRmsMin && state->rms_off <= u.nRmsMax && state->look_off >= u.nLookMin && state->look_off <= u.nLookMax,
               MI_EINVAL, "mi_depopper_bank_set_state: offsets %lld, %lld outside [%lld, %lld], [%lld, %lld]", (long long)state->rms_off,
               (long long)state->look_off, (long long)u.nRmsMin, (long long)u.nRmsMax, (long long)u.nLookMin, (long long)u.nLookMax);
    device_state s;
    r = mi_bank::get_state(b, "mi_depopper_bank_set_state", channel, &s, stream);
    if (r != MI_OK)
        return r;
    if (rms_buf != nullptr)
        MI_HIP_CHECK(hipMemcpyAsync(h.d_rings, rms_buf, size_t(u.nRmsMin) * sizeof(float), hipMemcpyHostToDevice, st));
    if (gain_buf != nullptr)
        MI_HIP_CHECK(hipMemcpyAsync(h.d_rings + h.rms_cap, gain_buf, size_t(u.nLookMin) * sizeof(float), hipMemcpyHostToDevice, st));
    // a buffer that was given starts at entry 0 of its ring and ends where the next entry goes
    s.rms = state->rms, s.state = int32_t(state->state), s.counter = int32_t(state->counter), s.delay = int32_t(state->delay);
    s.rms_off = uint32_t(state->rms_off), s.look_off = uint32_t(state->look_off);
    if (rms_buf != nullptr)
        s.rms_pos = uint32_t(u.nRmsMin) & (h.rms_cap - 1);
    if (gain_buf != nullptr)
        s.look_pos = uint32_t(u.nLookMin) & (h.look_cap - 1);
    return mi_bank::set_state(b, "mi_depopper_bank_set_state", channel, s, true, st);
}

int mi_depopper_bank_process(mi_depopper_bank_t *b, float *env, float *gain, const float *src, size_t count, size_t env_stride,
                             size_t gain_stride, size_t src_stride, void *stream)                             // :464-562
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_depopper_bank_process: NULL bank");
    hipStream_t st = mi::as_stream(stream);
    const int r = depopper_update(b, "mi_depopper_bank_process", st);
    if (r != MI_OK || count == 0)
        return r;
    const int k = mi_bank::check_rows("mi_depopper_bank_process", b->channels, count, COUNT_LIMIT,
                                      { { env, env_stride, count, mi_bank::OUTPUT }, { gain, gain_stride, count, mi_bank::OUTPUT | mi_bank::REQUIRED },
                                        { src, src_stride, count, mi_bank::REQUIRED } });
    if (k != MI_OK)
        return k;
    MI_REQUIRE(env != gain, MI_EINVAL, "mi_depopper_bank_process: env and gain are the same buffer");
    const uint32_t vec = (mi::aligned16(env, env_stride, b->channels) ? VEC_ENV : 0) | (mi::aligned16(gain, gain_stride, b->channels) ? VEC_GAIN : 0) |
                         (mi::aligned16(src, src_stride, b->channels) ? VEC_SRC : 0);
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    mi::take_profile_events(&ev0, &ev1);
    MI_LAUNCH(depopper_kernel, dim3((b->channels + GROUP - 1) / GROUP), dim3(BLOCK), 0, st, ev0, ev1, env, gain, src, env_stride,
              gain_stride, src_stride, uint32_t(count), b->channels, b->d_params, b->d_state, vec);
    MI_HIP_CHECK(hipGetLastError());
    return MI_OK;
}

} // extern "C"
