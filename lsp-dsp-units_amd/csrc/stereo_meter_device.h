// What correlometer.hip and panometer.hip share on the device: lsp::dspu::Correlometer and lsp::dspu::Panometer are the same
// walk -- two rings per channel, sliding-window sums with one tail sample leaving for every head sample entering, the sums
// formed anew from the rings every `period` samples -- with different terms, steps and formulas on top.  Here are the ring
// addressing, `last` out of the tile or out of the ring, the refresh with its split where the ring wraps, and the kernel's
// body on the tile walk of tile_chain_device.h; a METER (a struct of the .hip file) supplies the rest:
//     NS, ROWS             sums per channel, LDS rows per channel (ROWS / NS per sum; the first row of sum q is q * ROWS / NS)
//     ring_value(x)        what a sample leaves in its ring
//     term(q, a, b)        the term of sum q in a refresh, of the rings' values
//     steps(rows, i, ..)   what the chain needs of sample i into the channel's rows
//     fold(q, rows, i, s)  sum q after sample i when it was s before it: a refresh's value through sample i's step
//     chain(..)            the serial part over one tile, through the file's own __noinline__ function
//     emit(p, rows, i)     the output of sample i out of the sums after it
//
// The refresh does not depend on the running sums, so the helper waves form it beside the chain and FOLD it through the step of
// the sample it precedes: at a refresh index the row holds the sum AFTER that sample, not an increment, and the chain, which
// knows the indices (first, first + period, ...), takes it as it is and goes on from there.  Nothing else is handed over.
//     period <= TILE       up to TILE / period refreshes in a tile, one per sample at period 1.  The window of each lies in
//                          hist[]: the tile's own samples and the `period` samples of the ring before them.  Lane m takes
//                          refresh m (and m + 64, ...): every sum serial, oldest first, split at that refresh's nHead.
//     period > TILE        at most one.  The wave stages the ring through hist[] in pieces of TILE (a device-scope fence first:
//                          the tile's own pushes are part of the window), lane q sums the terms of sum q.
// A row's rings are written and read by ONE wave, whose stores and loads reach memory in program order; capacity - max_period
// >= 0x400 > TILE, so a tile's pushes never overwrite what the same tile still reads.  By the walk's invariant `out` may be an
// input row.  Every product and every sum rounds once.
#pragma once
#include "tile_chain_device.h"

#pragma clang fp contract(off)

namespace mi_stereo_meter
{
    using namespace mi_tile_chain;

    constexpr uint32_t RING_EXTRA = 0x400;      // BUFFER_SIZE, Correlometer.cpp:29, Panometer.cpp:30
    constexpr uint32_t RING_ALIGN = 0x40;       // DEFAULT_ALIGN
    constexpr uint32_t MAX_PERIOD = 1u << 28;
    constexpr int HIST = 2 * TILE;              // floats of a ring's history in LDS: [TILE - period, TILE) out of the ring, [TILE, TILE + n) the tile
    constexpr int QUAD = 4;                     // chain lanes per channel: lane 4 r + q runs sum q of row r

    enum { VEC_OUT = 1, VEC_A = 2, VEC_B = 4 };

    typedef __attribute__((address_space(1))) float global_float;

    struct meter_params { uint32_t period, capacity; float norm; uint32_t law; float dflt; uint32_t pad[3]; };  // [channels] on the device
    struct meter_state { float sum[3]; uint32_t head, window; };                                                 // [channels] between calls

    // init(): align_size(max_period + BUFFER_SIZE, DEFAULT_ALIGN)
    __host__ __device__ inline uint32_t ring_capacity(uint32_t max_period)
    {
        return (max_period + RING_EXTRA + RING_ALIGN - 1) & ~(RING_ALIGN - 1);
    }

    // p < 3 * cap
    __device__ __forceinline__ uint32_t wrap(uint32_t p, uint32_t cap)
    {
        p = (p >= cap) ? p - cap : p;
        return (p >= cap) ? p - cap : p;
    }

    // LDS traffic between the lanes of ONE wave: its DS instructions execute in order, the compiler must keep them so
    __device__ __forceinline__ void wave_sync()
    {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }

    // the correctly rounded float32 square root through float64 (sidechain.hip says why the second rounding is harmless)
    __device__ __forceinline__ float sqrt_rn(float q)
    {
        return float(__builtin_sqrt(double(q)));
    }

    // The tile-relative index of the first sample of the tile at t0 that finds nWindow >= nPeriod, when nWindow was w0 <= period
    // before the call's first sample; the later ones follow `period` apart.  Not below the tile's length: none.
    __device__ __forceinline__ uint32_t first_refresh(uint32_t w0, uint32_t t0, uint32_t period)
    {
        const uint32_t u = (w0 + t0) % period;
        return (u != 0 || w0 + t0 == 0) ? period - u : 0u;
    }

    // A refresh with the ring's position at `head`: the window [tail, head) of `period` samples is one piece, or the ring's
    // last `first` samples and then its first period - first ([tail, capacity), [0, head): Correlometer.cpp:149-155)
    __device__ __forceinline__ uint32_t refresh_split(uint32_t head, uint32_t period)
    {
        return (head < period) ? period - head : period;
    }

    // the chain's lanes: 4 r + q
    struct meter_role: public role { uint32_t q; };
    template <int NS> __device__ __forceinline__ meter_role my_meter_role(uint32_t channels)
    {
        meter_role me;
        static_cast<role &>(me) = my_role(channels);
        me.q = 0;
        if (me.chain)
        {
            me.q = me.lane & uint32_t(QUAD - 1);
            me.r = me.lane / uint32_t(QUAD);
            me.ch = blockIdx.x * GROUP + me.r;
            me.valid = me.r < uint32_t(GROUP) && me.q < uint32_t(NS) && me.ch < channels;
        }
        return me;
    }

    // The chain over samples [i, to) of a sum whose step takes two rows (head and tail): h[i] = step(h[i], t[i]), in order, with
    // chain_batches' read-ahead on both.
    template <class Step> __device__ __forceinline__ void chain_batches2(lds_float *h, const lds_float *t, uint32_t i, uint32_t to, Step step)
    {
        for (; i < to && (i & 3u) != 0; ++i)
            h[i] = step(h[i], t[i]);
        if (i + BATCH <= to)
        {
            f32x4 a = *reinterpret_cast<lds_f32x4 *>(h + i), b = *reinterpret_cast<lds_f32x4 *>(h + i + 4);
            f32x4 c = *reinterpret_cast<const lds_f32x4 *>(t + i), d = *reinterpret_cast<const lds_f32x4 *>(t + i + 4);
            for (; i + BATCH <= to; i += BATCH)
            {
                float v[BATCH] = { a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w };
                const float w[BATCH] = { c.x, c.y, c.z, c.w, d.x, d.y, d.z, d.w };
                const uint32_t next = (i + 2 * BATCH <= to) ? i + BATCH : i;   // the next batch, before this one's chain
                a = *reinterpret_cast<lds_f32x4 *>(h + next);
                b = *reinterpret_cast<lds_f32x4 *>(h + next + 4);
                c = *reinterpret_cast<const lds_f32x4 *>(t + next);
                d = *reinterpret_cast<const lds_f32x4 *>(t + next + 4);
                #pragma unroll
                for (int j = 0; j < BATCH; ++j)
                    v[j] = step(v[j], w[j]);
                *reinterpret_cast<lds_f32x4 *>(h + i) = f32x4{ v[0], v[1], v[2], v[3] };
                *reinterpret_cast<lds_f32x4 *>(h + i + 4) = f32x4{ v[4], v[5], v[6], v[7] };
            }
        }
        for (; i < to; ++i)
            h[i] = step(h[i], t[i]);
    }

    // One tile of one sum: run(i, to, s) chains samples [i, to) from s; at first, first + period, ... the row already holds the
    // sum after that sample (the refresh folded through its step).
    template <class Run> __device__ __forceinline__ float chain_segments(const lds_float *row, uint32_t n, float s, uint32_t first,
                                                                         uint32_t period, Run run)
    {
        uint32_t i = 0;
        for (uint32_t seg = first; seg < n; seg += period)
        {
            (void)run(i, seg, s);
            s = row[seg];
            i = seg + 1;
        }
        return run(i, n, s);
    }

    // LDS of one kernel: tile[2][GROUP][ROWS][ROW] and hist[GROUP][2][HIST] floats, first[2][GROUP]
    template <class METER> struct meter_lds
    {
        float tile[2][GROUP][METER::ROWS][ROW] __attribute__((aligned(16)));
        float hist[GROUP][2][HIST] __attribute__((aligned(16)));
        uint32_t first[2][GROUP];
    };

    // process() of every channel: the body of both kernels
    template <class METER>
    __device__ __forceinline__ void meter_process(meter_lds<METER> &L, float *out, const float *a, const float *b, size_t out_stride,
                                                  size_t a_stride, size_t b_stride, uint32_t count, uint32_t channels,
                                                  const meter_params *params, meter_state *state, float *rings, size_t ring_stride,
                                                  uint32_t vec)
    {
        constexpr int NS = METER::NS, ROWS = METER::ROWS, PER = ROWS / NS;
        const meter_role me = my_meter_role<NS>(channels);
        const bool valid = me.valid;
        const uint32_t lane = me.lane, r = me.r, ch = me.ch, c = me.c, q = me.q;
        meter_params p = {};
        meter_state s0 = {};
        if (valid)
            p = params[ch], s0 = state[ch];
        const uint32_t cap = (p.capacity > 0) ? p.capacity : 1;
        const uint32_t P = (p.period > 0) ? p.period : 1;               // the host refuses a period of 0
        const uint32_t W0 = (s0.window < P) ? s0.window : P;
        const uint32_t head0 = s0.head % cap;
        const bool many = P <= uint32_t(TILE);                          // the windows of a tile's refreshes lie in hist[]
        float sum = (q == 0) ? s0.sum[0] : (q == 1) ? s0.sum[1] : s0.sum[2];    // the chain's (picked, not indexed: no private segment)
        uint32_t head_t = head0;                                        // a helper's: the ring position of the next tile's first sample
        const float *as = a + size_t(ch) * a_stride, *bs = b + size_t(ch) * b_stride;
        float *os = out + size_t(ch) * out_stride;
        global_float *ring_a = valid ? (global_float *)(rings + (size_t(ch) * 2) * ring_stride) : nullptr;
        global_float *ring_b = valid ? (global_float *)(rings + (size_t(ch) * 2 + 1) * ring_stride) : nullptr;
        lds_float *const ha = (lds_float *)&L.hist[r < uint32_t(GROUP) ? r : 0][0][0];
        lds_float *const hb = (lds_float *)&L.hist[r < uint32_t(GROUP) ? r : 0][1][0];

        // `len` samples of the rings from `start`, no wrap inside: the terms of sum (lane mod 4) serially, oldest first, from 0
        auto part = [&](uint32_t start, uint32_t len) -> float
        {
            const uint32_t mine = lane & uint32_t(QUAD - 1);
            float acc = 0.0f;
            for (uint32_t base = 0; base < len; base += TILE)
            {
                const uint32_t m = (len - base < uint32_t(TILE)) ? len - base : uint32_t(TILE);
                wave_sync();
                #pragma unroll
                for (uint32_t j = 0; j < 4; ++j)
                {
                    const uint32_t idx = lane + 64 * j;
                    if (idx < m)
                    {
                        ha[idx] = ring_a[start + base + idx];
                        hb[idx] = ring_b[start + base + idx];
                    }
                }
                wave_sync();
                uint32_t i = 0;
                #pragma unroll 2
                for (; i + 4 <= m; i += 4)
                {
                    const f32x4 va = *reinterpret_cast<const lds_f32x4 *>(ha + i), vb = *reinterpret_cast<const lds_f32x4 *>(hb + i);
                    acc += METER::term(mine, va.x, vb.x);
                    acc += METER::term(mine, va.y, vb.y);
                    acc += METER::term(mine, va.z, vb.z);
                    acc += METER::term(mine, va.w, vb.w);
                }
                for (; i < m; ++i)
                    acc += METER::term(mine, ha[i], hb[i]);
            }
            return acc;
        };

        auto prepare = [&](uint32_t k)
        {
            const extent t = tile_extent(count, k);
            const uint32_t t0 = t.t0, n = t.n, buf = k & 1;
            lds_float *const rows = (lds_float *)&L.tile[buf][r][0][0];
            float x[4] = { 0.0f, 0.0f, 0.0f, 0.0f }, y[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
            if (c < n)
            {
                const bool whole = c + 4 <= n;
                if ((vec & VEC_A) && whole)
                {
                    const float4 v = *reinterpret_cast<const float4 *>(as + t0 + c);
                    x[0] = v.x, x[1] = v.y, x[2] = v.z, x[3] = v.w;
                }
                else
                {
                    #pragma unroll
                    for (uint32_t j = 0; j < 4; ++j)
                        if (c + j < n)
                            x[j] = as[t0 + c + j];
                }
                if ((vec & VEC_B) && whole)
                {
                    const float4 v = *reinterpret_cast<const float4 *>(bs + t0 + c);
                    y[0] = v.x, y[1] = v.y, y[2] = v.z, y[3] = v.w;
                }
                else
                {
                    #pragma unroll
                    for (uint32_t j = 0; j < 4; ++j)
                        if (c + j < n)
                            y[j] = bs[t0 + c + j];
                }
                // into both rings
                #pragma unroll
                for (uint32_t j = 0; j < 4; ++j)
                {
                    x[j] = METER::ring_value(x[j]), y[j] = METER::ring_value(y[j]);
                    if (c + j < n)
                    {
                        const uint32_t at = wrap(head_t + c + j, cap);
                        ring_a[at] = x[j];
                        ring_b[at] = y[j];
                    }
                }
            }
            wave_sync();                                                // whoever still read hist[] for the tile before has
            *reinterpret_cast<float4 *>(&L.hist[r][0][TILE + c]) = make_float4(x[0], x[1], x[2], x[3]);
            *reinterpret_cast<float4 *>(&L.hist[r][1][TILE + c]) = make_float4(y[0], y[1], y[2], y[3]);
            if (many)
            {
                // the `period` samples before the tile: written by earlier tiles or calls (or zero)
                #pragma unroll
                for (uint32_t j = 0; j < 4; ++j)
                {
                    const uint32_t idx = lane + 64 * j;
                    if (idx < P)
                    {
                        const uint32_t at = wrap(head_t + cap - P + idx, cap);
                        ha[TILE - P + idx] = ring_a[at];
                        hb[TILE - P + idx] = ring_b[at];
                    }
                }
            }
            wave_sync();
            // the tail samples: out of this tile or out of the ring
            if (c < n)
            {
                #pragma unroll
                for (uint32_t j = 0; j < 4; ++j)
                {
                    const uint32_t i = c + j;
                    if (i < n)
                    {
                        float at, bt;
                        if (many)
                            at = ha[TILE + i - P], bt = hb[TILE + i - P];
                        else
                        {
                            const uint32_t from = wrap(head_t + i + cap - P, cap);
                            at = ring_a[from], bt = ring_b[from];
                        }
                        METER::steps(rows, i, x[j], y[j], at, bt);
                    }
                }
            }
            const uint32_t first = first_refresh(W0, t0, P);
            if (first < n)
            {
                wave_sync();                                            // the steps of the refreshes' samples are in the rows
                if (many)
                {
                    for (uint32_t ridx = first + lane * P; ridx < n; ridx += 64 * P)
                    {
                        const uint32_t split = refresh_split(wrap(head_t + ridx, cap), P);
                        const uint32_t base = uint32_t(TILE) + ridx - P;
                        float s1[NS], s2[NS];
                        #pragma unroll
                        for (int u = 0; u < NS; ++u)
                            s1[u] = s2[u] = 0.0f;
                        #pragma unroll 4
                        for (uint32_t j = 0; j < split; ++j)
                        {
                            const float va = ha[base + j], vb = hb[base + j];
                            #pragma unroll
                            for (int u = 0; u < NS; ++u)
                                s1[u] += METER::term(uint32_t(u), va, vb);
                        }
                        #pragma unroll 4
                        for (uint32_t j = split; j < P; ++j)
                        {
                            const float va = ha[base + j], vb = hb[base + j];
                            #pragma unroll
                            for (int u = 0; u < NS; ++u)
                                s2[u] += METER::term(uint32_t(u), va, vb);
                        }
                        #pragma unroll
                        for (int u = 0; u < NS; ++u)
                            rows[u * PER * ROW + ridx] = METER::fold(uint32_t(u), rows, ridx, s1[u] + s2[u]);
                    }
                }
                else
                {
                    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");  // this tile's samples before `first` are in the rings
                    const uint32_t head_r = wrap(head_t + first, cap);
                    const uint32_t split = refresh_split(head_r, P);
                    const float s1 = part((head_r >= P) ? head_r - P : cap - split, split);
                    const float s2 = part(0, P - split);
                    const uint32_t mine = lane & uint32_t(QUAD - 1);
                    if (lane < uint32_t(NS))
                        rows[mine * PER * ROW + first] = METER::fold(mine, rows, first, s1 + s2);
                }
            }
            if (lane == 0)
                L.first[buf][r] = first;
            head_t = wrap(head_t + n, cap);
        };

        auto emit = [&](uint32_t k)
        {
            const extent t = tile_extent(count, k);
            if (c >= t.n)
                return;
            const lds_float *const rows = (const lds_float *)&L.tile[k & 1][r][0][0];
            float yv[4];
            METER::emit(p, rows, c, yv);
            store_quad(os + t.t0 + c, yv, vec & VEC_OUT, c, t.n);
        };

        MI_TILE_CHAIN_WALK(me, count, k, prepare(k),
                           sum = METER::chain((lds_float *)&L.tile[k & 1][r][0][0], q, tile_extent(count, k).n, sum, L.first[k & 1][r], P),
                           emit(k));
        if (valid && me.chain)
        {
            // nWindow after `count` samples (count > 0): it falls to 0 only when a sample follows
            state[ch].sum[q] = sum;
            if (q == 0)
            {
                state[ch].head = uint32_t((uint64_t(head0) + count) % cap);
                state[ch].window = (W0 + count - 1) % P + 1;
            }
        }
    }
} // namespace mi_stereo_meter
