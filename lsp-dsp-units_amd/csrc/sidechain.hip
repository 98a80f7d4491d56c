// lsp::dspu::Sidechain as a bank of `channels` sidechains (src/main/util/Sidechain.cpp): the block overload of process()
// (:439-554) -- source selection (:183-333, the dsp:: pair primitives as the scalar overload states them, :335-437), the
// magnitude times fGain, the push into the ring, the refresh of fRmsValue every 0x2000 samples (:144-181) and the four
// detectors (:465-547).
//
// The window detectors are rms += x[i]^2 - x[i - N]^2 (RMS) and rms += x[i] - x[i - N] (UNIFORM): the increment d[i] does not
// depend on rms, so every lane can form it, and what is left of the recurrence is ONE dependent add per sample, in the
// reference's order.  The low-pass is rms += tau * (x - rms): three dependent operations.  sidechain_kernel runs everything
// in one launch on the tile walk of tile_chain_device.h:
//     chain            d[i] overwritten by the running fRmsValue in LDS
//     emit             a tile out of LDS through * interval, the square root or the clamp into `out`
//     prepare          loads, source, |.| * gain, the samples into the ring, last = x[i - N] (out of the same tile where N allows
//                      it, out of the ring otherwise), d[i] into LDS, and -- where one of the tile's samples is the 0x2000th --
//                      the refresh sum over the ring, beside the chain, handed over in LDS
// By the walk's invariant `out` may be an input row.  The ring in device memory is the reference's (capacity, position), so
// the refresh sum splits where the reference's splits.  A row's ring is written and read by ONE wave (its helper), whose stores and loads
// reach memory in program order; the capacity exceeds N by 0x200 > TILE, so a tile's samples never overwrite a sample the
// same tile still needs.  Every product and every sum rounds once (no fused multiply-add), the square root is correctly
// rounded (sqrt_rn): out, fRmsValue, nRefresh and the position match tests/sidechain_ref.py bit for bit.
//
// Inputs are finite: NaN is out of scope.  Subnormals are kept (the float32 denormal mode is on).
#include "bank_core.h"
#include "sidechain_bank.h"
#include "tile_chain_device.h"

#include <lsp-plug.in/dsp-units/units.h>

#include <cmath>
#include <new>
#include <vector>

#pragma clang fp contract(off)      // every product and every sum below rounds on its own, host and device

namespace
{
    using namespace mi_tile_chain;
    using lsp::dspu::millis_to_samples;

    constexpr int MIX_BLOCK = 256;
    constexpr uint32_t REFRESH_RATE = 0x2000;   // Sidechain.cpp:31
    constexpr uint32_t RING_EXTRA   = 0x200;    // BLOCK_SIZE, Sidechain.cpp:30: what the ring holds beyond the longest window
    constexpr uint32_t NO_REFRESH   = 0xffffffffu;
    constexpr uint32_t SEL_FIRST    = 12;       // pick_source(): the first input as it is

    enum { VEC_OUT = 1, VEC_IN0 = 2, VEC_IN1 = 4 };
    enum { P_RING = 1, P_ZERO_RMS = 2 };        // pending beside nFlags: the ring re-made, set_mode's fRmsValue = 0

    typedef __attribute__((address_space(1))) float global_float;      // a pointer out of memory is generic to the compiler otherwise

    struct device_state { float rms; uint32_t refresh, head, pad; };     // [channels] between calls
    struct ring_desc { float *ring; uint64_t stride; };                  // on the device: rings grow without the launches changing

    // preprocess(), Sidechain.cpp:183-333 with :335-437: sel = 6 * midside + nSource for two inputs, SEL_FIRST for one
    __host__ __device__ __forceinline__ float pick_source(float a, float b, uint32_t sel)
    {
        switch (sel)
        {
            case 0:  return (a + b) * 0.5f;                                 // lr_to_mid
            case 1:  return (a - b) * 0.5f;                                 // lr_to_side
            case 3:  return b;                                              // right; the side of a mid-side pair
            case 7:  return b;
            case 4:  return (fabsf(a) < fabsf(b)) ? a : b;                  // psmin3
            case 5:  return (fabsf(b) < fabsf(a)) ? a : b;                  // psmax3
            case 8:  return a + b;                                          // ms_to_left
            case 9:  return a - b;                                          // ms_to_right
            case 10: { const float l = a + b, r = a - b; return (fabsf(l) < fabsf(r)) ? l : r; }
            case 11: { const float l = a + b, r = a - b; return (fabsf(r) < fabsf(l)) ? l : r; }
            default: return a;                                              // left, the middle of a mid-side pair, one input
        }
    }

    __device__ __forceinline__ uint32_t selector(const mi_sidechain_params_t &p, bool two)
    {
        return two ? ((p.flags & MI_SCF_MIDSIDE) ? 6u : 0u) + p.source : SEL_FIRST;
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

    // The correctly rounded float32 square root whatever the compiler is told about float32 sqrt: through float64.  A float32
    // root is never nearer than 2^-50 (relative) to the middle between two float32 values, eight units of the float64 result's
    // last place, so rounding the float64 root (faithful or better) a second time gives the float32 root rounded once.
    __device__ __forceinline__ float sqrt_rn(float q)
    {
        return float(__builtin_sqrt(double(q)));
    }

    template <bool LPF> __device__ __forceinline__ float chain_step(float v, float rms, float tau)
    {
        return LPF ? rms + tau * (v - rms) : rms + v;
    }

    // samples [i, to) of one row in LDS, in place: row[i] becomes fRmsValue after sample i (Sidechain.cpp:474-479, :495-507,
    // :522-537)
    template <bool LPF> __device__ __forceinline__ float chain_run(lds_float *row, uint32_t i, uint32_t to, float rms, float tau)
    {
        chain_batches(row, i, to, [&](float v) { return rms = chain_step<LPF>(v, rms, tau); });
        return rms;
    }

    // One tile of one channel: the refresh (refresh_processing() before sample `ridx`: `rval` replaces fRmsValue) and the
    // detector's recurrence.  A function of its own so that its instructions can be looked at (tests/test_sidechain_host.py).
    __device__ __noinline__ float sidechain_chain_tile(lds_float *row, uint32_t n, float rms, uint32_t mode, float tau,
                                                       uint32_t ridx, float rval)
    {
        const bool refresh = ridx < n;
        if (mode == MI_SCM_PEAK)
            return refresh ? rval : rms;
        if (mode == MI_SCM_LPF)
            return chain_run<true>(row, 0, n, rms, tau);
        if (refresh)
        {
            (void)chain_run<false>(row, 0, ridx, rms, tau);
            return chain_run<false>(row, ridx, n, rval, tau);
        }
        return chain_run<false>(row, 0, n, rms, tau);
    }

    // stage: the whole of process(), or its second half on rows that premix() wrote (in1 is not looked at)
    __global__ __launch_bounds__(BLOCK) void sidechain_kernel(float *out, const float *in0, const float *in1, size_t out_stride,
                                                              size_t in0_stride, size_t in1_stride, uint32_t count,
                                                              uint32_t channels, uint32_t two,
                                                              const mi_sidechain_params_t *params, device_state *state,
                                                              const ring_desc *desc, uint32_t vec)
    {
        __shared__ __attribute__((aligned(16))) float tile[2][GROUP][ROW];      // d[i], then fRmsValue after sample i
        __shared__ __attribute__((aligned(16))) float xs[GROUP][TILE];          // a helper's own: the tile's samples, the refresh's terms
        __shared__ uint32_t r_idx[2][GROUP];
        __shared__ float r_val[2][GROUP];
        const role me = my_role(channels);
        const bool valid = me.valid;
        const uint32_t lane = me.lane, r = me.r, ch = me.ch, c = me.c;
        mi_sidechain_params_t p = {};
        device_state s0 = {};
        if (valid)
            p = params[ch], s0 = state[ch];
        const uint32_t cap = (p.capacity > 0) ? p.capacity : 1, N = p.reactivity, mode = p.mode;
        const uint32_t R0 = (s0.refresh < REFRESH_RATE) ? s0.refresh : REFRESH_RATE;
        const uint32_t head0 = s0.head % cap;
        const uint32_t sel = selector(p, two != 0);
        const bool window = mode == MI_SCM_RMS || mode == MI_SCM_UNIFORM, squares = mode == MI_SCM_RMS;
        float rms = s0.rms;
        uint32_t head_t = head0;                                    // a helper's: the ring position of the next tile's first sample
        const float *as = (in0 != nullptr) ? in0 + size_t(ch) * in0_stride : nullptr;
        const float *bs = (two != 0 && in1 != nullptr) ? in1 + size_t(ch) * in1_stride : nullptr;
        float *os = out + size_t(ch) * out_stride;
        global_float *ring = valid ? (global_float *)(desc->ring + size_t(ch) * desc->stride) : nullptr;

        // serial, oldest to newest, each term rounded, then each sum: `len` samples of the ring from `start`, no wrap inside.
        // Every lane of the wave forms the same sum out of LDS.
        auto part = [&](uint32_t start, uint32_t len) -> float
        {
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
                        const float q = ring[start + base + idx];
                        xs[r][idx] = squares ? q * q : fabsf(q);
                    }
                }
                wave_sync();
                uint32_t i = 0;
                for (; i + 4 <= m; i += 4)
                {
                    const f32x4 q = *reinterpret_cast<const f32x4 *>(&xs[r][i]);
                    acc += q.x; acc += q.y; acc += q.z; acc += q.w;
                }
                for (; i < m; ++i)
                    acc += xs[r][i];
            }
            return acc;
        };

        auto prepare = [&](uint32_t k)
        {
            const extent t = tile_extent(count, k);
            const uint32_t t0 = t.t0, n = t.n, buf = k & 1;
            // the source, its magnitude, the gain (:183-333, :449-450)
            float x[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
            if (c < n)
            {
                float a[4] = { 0.0f, 0.0f, 0.0f, 0.0f }, b[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
                const bool whole = c + 4 <= n;
                if (as != nullptr)
                {
                    if ((vec & VEC_IN0) && whole)
                    {
                        const float4 q = *reinterpret_cast<const float4 *>(as + t0 + c);
                        a[0] = q.x, a[1] = q.y, a[2] = q.z, a[3] = q.w;
                    }
                    else
                    {
                        #pragma unroll
                        for (uint32_t j = 0; j < 4; ++j)
                            if (c + j < n)
                                a[j] = as[t0 + c + j];
                    }
                }
                if (bs != nullptr)
                {
                    if ((vec & VEC_IN1) && whole)
                    {
                        const float4 q = *reinterpret_cast<const float4 *>(bs + t0 + c);
                        b[0] = q.x, b[1] = q.y, b[2] = q.z, b[3] = q.w;
                    }
                    else
                    {
                        #pragma unroll
                        for (uint32_t j = 0; j < 4; ++j)
                            if (c + j < n)
                                b[j] = bs[t0 + c + j];
                    }
                }
                #pragma unroll
                for (uint32_t j = 0; j < 4; ++j)
                    x[j] = fabsf(pick_source(a[j], b[j], sel)) * p.gain;
                // sBuffer.push(), :463
                #pragma unroll
                for (uint32_t j = 0; j < 4; ++j)
                    if (c + j < n)
                        ring[wrap(head_t + c + j, cap)] = x[j];
            }
            *reinterpret_cast<float4 *>(&xs[r][c]) = make_float4(x[0], x[1], x[2], x[3]);
            wave_sync();
            // the increments: last = x[i - N], out of this tile or out of the ring (written by an earlier tile or call)
            float d[4] = { x[0], x[1], x[2], x[3] };
            if (window && c < n)
            {
                #pragma unroll
                for (uint32_t j = 0; j < 4; ++j)
                {
                    const uint32_t i = c + j;
                    if (i < n)
                    {
                        const float last = (i >= N) ? xs[r][i - N] : ring[wrap(head_t + i + cap - N, cap)];
                        d[j] = squares ? x[j] * x[j] - last * last : x[j] - last;
                    }
                }
            }
            *reinterpret_cast<float4 *>(&tile[buf][r][c]) = make_float4(d[0], d[1], d[2], d[3]);
            // refresh_processing() (:144-181) before the sample that finds nRefresh at REFRESH_RATE (:455-459)
            const uint32_t u = (R0 + t0) % REFRESH_RATE;
            uint32_t ridx = (u != 0) ? REFRESH_RATE - u : (R0 + t0 > 0) ? 0u : NO_REFRESH;
            ridx = (ridx < n && mode != MI_SCM_LPF) ? ridx : NO_REFRESH;
            float rval = 0.0f;
            if (ridx != NO_REFRESH && window)
            {
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");      // this tile's samples before `ridx` are in the ring
                const uint32_t head_r = wrap(head_t + ridx, cap);       // nHead at the refresh; the window is [tail, head)
                if (head_r >= N)
                    rval = part(head_r - N, N);
                else
                {
                    const float s1 = part(cap - (N - head_r), N - head_r);     // tail .. end()
                    const float s2 = part(0, head_r);                           // begin() .. head
                    rval = s1 + s2;
                }
            }
            r_idx[buf][r] = ridx;
            r_val[buf][r] = rval;
            head_t = wrap(head_t + n, cap);
        };

        auto emit = [&](uint32_t k)
        {
            const extent t = tile_extent(count, k);
            if (c >= t.n)
                return;
            const float4 v4 = *reinterpret_cast<const float4 *>(&tile[k & 1][r][c]);
            float y[4] = { v4.x, v4.y, v4.z, v4.w };
            #pragma unroll
            for (uint32_t j = 0; j < 4; ++j)
            {
                const float v = y[j];
                if (mode == MI_SCM_RMS)
                {
                    const float q = v * p.interval;                                 // :529, :537, then ssqrt1 (:539)
                    y[j] = (q > 0.0f) ? sqrt_rn(q) : 0.0f;
                }
                else if (mode == MI_SCM_UNIFORM)
                    y[j] = (v < 0.0f) ? 0.0f : v * p.interval;                      // :500, :506
                else if (mode == MI_SCM_LPF)
                    y[j] = (v > 0.0f) ? v : 0.0f;                                   // :478
            }
            store_quad(os + t.t0 + c, y, vec & VEC_OUT, c, t.n);
        };

        MI_TILE_CHAIN_WALK(me, count, k, prepare(k),
                           rms = sidechain_chain_tile((lds_float *)&tile[k & 1][r][0], tile_extent(count, k).n, rms, mode, p.tau,
                                                      r_idx[k & 1][r], r_val[k & 1][r]),
                           emit(k));
        if (valid && me.chain)
        {
            // nRefresh after `count` samples (count > 0): it is taken modulo REFRESH_RATE only when a sample follows (:455-459)
            const uint32_t refresh = (R0 + count - 1) % REFRESH_RATE + 1;
            // RawRingBuffer::push wraps only where nHead + count > nCapacity (RawRingBuffer.cpp:110-122): a block that ends at the
            // ring's end leaves the position AT the capacity, so after count > 0 samples it lies in (0, capacity]
            const uint32_t head = uint32_t((uint64_t(head0) + count - 1) % cap) + 1;
            state[ch] = device_state{ rms, refresh, head, 0 };
        }
    }

    // the signed source of every channel (psmin3 / psmax3 for AMIN / AMAX), stateless
    __global__ __launch_bounds__(MIX_BLOCK) void sidechain_premix_kernel(float *out, const float *in0, const float *in1,
                                                                         size_t out_stride, size_t in0_stride, size_t in1_stride,
                                                                         uint32_t count, uint32_t two,
                                                                         const mi_sidechain_params_t *params)
    {
        const uint32_t ch = blockIdx.y, i = blockIdx.x * MIX_BLOCK + threadIdx.x;
        if (i >= count)
            return;
        const uint32_t sel = selector(params[ch], two != 0);
        const float a = (in0 != nullptr) ? in0[size_t(ch) * in0_stride + i] : 0.0f;
        const float b = (two != 0 && in1 != nullptr) ? in1[size_t(ch) * in1_stride + i] : 0.0f;
        out[size_t(ch) * out_stride + i] = pick_source(a, b, sel);
    }

    // set_sample_rate(), :92: lsp_max(millis_to_samples(sr, fMaxReactivity), 1) + BLOCK_SIZE in float, then size_t
    uint32_t ring_capacity(uint32_t sample_rate, float max_reactivity)
    {
        const float m = millis_to_samples(float(sample_rate), max_reactivity);
        const float c = ((m > 1.0f) ? m : 1.0f) + float(RING_EXTRA);
        return (c < 1073741824.0f) ? uint32_t(c) : 0u;                  // 0: too long
    }

    // update_settings(), :126-128
    void compute_window(uint32_t sample_rate, float reactivity, mi_sidechain_params_t &p)
    {
        const float m = millis_to_samples(float(sample_rate), reactivity);
        const int64_t react = (m < 1073741824.0f) ? int64_t(m) : 1073741824;
        p.reactivity = uint32_t((react > 1) ? react : 1);
        p.tau = 1.0f - expf(logf(float(1.0 - M_SQRT1_2)) / float(p.reactivity));
        p.interval = 1.0f / float(p.reactivity);
    }

    mi_sidechain_params_t fresh_params()
    {
        mi_sidechain_params_t p = {};
        p.reactivity = 1, p.tau = 1.0f, p.interval = 1.0f, p.capacity = 1 + RING_EXTRA;
        p.mode = MI_SCM_RMS, p.source = MI_SCS_MIDDLE, p.gain = 1.0f;
        return p;
    }

    struct channel_cfg { uint32_t sample_rate; float reactivity; uint32_t mode, source, flags; float gain; };
} // namespace

struct mi_sidechain_bank : mi_bank::tables<mi_sidechain_params_t, device_state>     // params: what update_settings computed
{
    uint32_t                                inputs = 1;
    float                                   max_reactivity = 0.0f;
    std::vector<channel_cfg>                cfg;            // the setters' values; flags: nFlags
    std::vector<uint8_t>                    pend;           // P_* of every channel
    bool                                    work = true;    // some channel has flags or pend set
    ring_desc                              *d_desc = nullptr;
    float                                  *d_ring = nullptr;       // [channels][ring_stride]
    size_t                                  ring_stride = 0;
};

namespace
{
    // rings of `stride` floats: the old rows are kept, what is new is zero
    int grow_rings(mi_sidechain_bank *b, size_t stride, hipStream_t st)
    {
        MI_REQUIRE(stride * b->channels < (size_t(1) << 33), MI_ENOMEM, "mi_sidechain_bank: %u rings of %zu samples are too much", b->channels, stride);
        float *ring = nullptr;
        MI_HIP_CHECK(hipMalloc(reinterpret_cast<void **>(&ring), stride * b->channels * sizeof(float)));
        hipError_t e = hipMemsetAsync(ring, 0, stride * b->channels * sizeof(float), st);
        if (e == hipSuccess && b->d_ring != nullptr)
            e = hipMemcpy2DAsync(ring, stride * sizeof(float), b->d_ring, b->ring_stride * sizeof(float), b->ring_stride * sizeof(float),
                                 b->channels, hipMemcpyDeviceToDevice, st);
        const ring_desc d = { ring, uint64_t(stride) };
        if (e == hipSuccess) e = hipMemcpyAsync(b->d_desc, &d, sizeof(d), hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess)
        {
            (void)hipFree(ring);
            return mi::fail(MI_EHIP, "mi_sidechain_bank: %s", hipGetErrorString(e));
        }
        (void)hipFree(b->d_ring);
        b->d_ring = ring, b->ring_stride = stride;
        return MI_OK;
    }

    // update_settings(), :119-142, of every channel with something pending, and what the setters left for the device
    int sc_update(mi_sidechain_bank *b, hipStream_t st)
    {
        if (!b->work && !b->up.any())
            return MI_OK;
        const int r = mi::refuse_capture("mi_sidechain_bank", st);
        if (r != MI_OK)
            return r;
        if (b->work)
        {
            size_t need = b->ring_stride;
            for (uint32_t ch = 0; ch < b->channels; ++ch)
                if (b->pend[ch] & P_RING)
                {
                    const size_t c = (size_t(b->params[ch].capacity) + 3) & ~size_t(3);
                    need = (c > need) ? c : need;
                }
            if (need > b->ring_stride)
            {
                const int g = grow_rings(b, need, st);
                if (g != MI_OK)
                    return g;
            }
            std::vector<device_state> hs(b->channels);
            MI_HIP_CHECK(hipMemcpyAsync(hs.data(), b->d_state, hs.size() * sizeof(device_state), hipMemcpyDeviceToHost, st));
            MI_HIP_CHECK(hipStreamSynchronize(st));
            for (uint32_t ch = 0; ch < b->channels; ++ch)
            {
                channel_cfg &c = b->cfg[ch];
                const uint8_t pd = b->pend[ch];
                if (!(c.flags & (MI_SCF_UPDATE | MI_SCF_CLEAR)) && pd == 0)
                    continue;
                bool zero = (pd & P_RING) != 0;
                if (pd & P_ZERO_RMS)
                    hs[ch].rms = 0.0f;
                if (pd & P_RING)
                    hs[ch].head = 0;
                if (c.flags & MI_SCF_UPDATE)
                {
                    compute_window(c.sample_rate, c.reactivity, b->params[ch]);
                    hs[ch].refresh = REFRESH_RATE;                      // force the function to be refreshed
                }
                if (c.flags & MI_SCF_CLEAR)
                    hs[ch].rms = 0.0f, hs[ch].refresh = 0, zero = true;
                if (zero)
                    MI_HIP_CHECK(hipMemsetAsync(b->d_ring + size_t(ch) * b->ring_stride, 0, b->ring_stride * sizeof(float), st));
                c.flags &= MI_SCF_MIDSIDE;
                b->pend[ch] = 0;
                b->up.touch(ch);
            }
            MI_HIP_CHECK(hipMemcpyAsync(b->d_state, hs.data(), hs.size() * sizeof(device_state), hipMemcpyHostToDevice, st));
            MI_HIP_CHECK(hipStreamSynchronize(st));                     // `hs` is gone after this returns
            b->work = false;
        }
        for (uint32_t ch = b->up.lo; ch < b->up.hi; ++ch)
        {
            const channel_cfg &c = b->cfg[ch];
            b->params[ch].mode = c.mode, b->params[ch].source = c.source, b->params[ch].flags = c.flags & MI_SCF_MIDSIDE, b->params[ch].gain = c.gain;
        }
        return mi_bank::upload(*b, "mi_sidechain_bank", st);
    }

    int sc_launch(mi_sidechain_bank *b, float *out, const float *in0, const float *in1, size_t count, size_t out_stride,
                  size_t in0_stride, size_t in1_stride, bool two, hipStream_t st)
    {
        const uint32_t vec = (mi::aligned16(out, out_stride, b->channels) ? VEC_OUT : 0) | (mi::aligned16(in0, in0_stride, b->channels) ? VEC_IN0 : 0) |
                             (mi::aligned16(in1, in1_stride, b->channels) ? VEC_IN1 : 0);
        hipEvent_t ev0 = nullptr, ev1 = nullptr;
        mi::take_profile_events(&ev0, &ev1);
        MI_LAUNCH(sidechain_kernel, dim3((b->channels + GROUP - 1) / GROUP), dim3(BLOCK), 0, st, ev0, ev1, out, in0, in1, out_stride,
                  in0_stride, in1_stride, uint32_t(count), b->channels, uint32_t(two ? 1 : 0), b->d_params, b->d_state, b->d_desc, vec);
        MI_HIP_CHECK(hipGetLastError());
        return MI_OK;
    }

    // the checks the three sample entries share: in0 may be missing (silence); in1 counts only beside it in a bank of two inputs
    int sc_check(const mi_sidechain_bank *b, const char *entry, const float *out, const float *in0, const float *in1, size_t count,
                 size_t out_stride, size_t in0_stride, size_t in1_stride, bool two)
    {
        const bool second = two && in0 != nullptr;
        const int r = mi_bank::check_rows(entry, b->channels, count, size_t(1) << 31,
                                          { { out, out_stride, count, mi_bank::REQUIRED | mi_bank::OUTPUT }, { in0, in0_stride, count, 0 },
                                            { second ? in1 : nullptr, in1_stride, count, 0 } });
        if (r != MI_OK)
            return r;
        MI_REQUIRE(!second || in1 != nullptr, MI_EINVAL, "%s: a bank of two inputs without the second one", entry);
        return MI_OK;
    }
} // namespace

namespace
{
    // what create() does to the new, empty bank
    int sc_init(mi_sidechain_bank *b, uint32_t channels, uint32_t inputs, float max_reactivity_ms)
    {
        b->channels = channels, b->inputs = inputs, b->max_reactivity = max_reactivity_ms;
        b->cfg.assign(channels, channel_cfg{ 0, 0.0f, MI_SCM_RMS, MI_SCS_MIDDLE, MI_SCF_UPDATE | MI_SCF_CLEAR, 1.0f });
        b->pend.assign(channels, P_RING);                           // a ring for the sample rate 0 until one is set
        b->up.lo = 0, b->up.hi = channels;
        const int r = mi_bank::alloc(*b, "mi_sidechain_bank_create", fresh_params(), device_state{});
        if (r != MI_OK)
            return r;
        hipError_t e = hipMalloc(reinterpret_cast<void **>(&b->d_desc), sizeof(ring_desc));
        if (e == hipSuccess) e = hipMemset(b->d_desc, 0, sizeof(ring_desc));
        MI_REQUIRE(e == hipSuccess, MI_EHIP, "mi_sidechain_bank_create: %s", hipGetErrorString(e));
        return MI_OK;
    }
} // namespace

namespace mi
{
    int sidechain_bank_set_params(mi_sidechain_bank_t *b, uint32_t channel, const mi_sidechain_params_t *p)
    {
        MI_REQUIRE(b != nullptr && p != nullptr && channel < b->channels, MI_EINVAL, "sidechain_bank_set_params: bad argument");
        MI_REQUIRE(p->reactivity >= 1 && p->capacity < (1u << 30) && uint64_t(p->reactivity) + RING_EXTRA <= p->capacity &&
                   p->mode <= MI_SCM_UNIFORM && p->source <= MI_SCS_AMAX, MI_EINVAL,
                   "sidechain_bank_set_params: a window of %u samples in a ring of %u, mode %u, source %u", p->reactivity, p->capacity, p->mode, p->source);
        channel_cfg &c = b->cfg[channel];
        mi_sidechain_params_t &q = b->params[channel];
        const bool ring = p->capacity != q.capacity;
        if (!ring && (c.flags & (MI_SCF_UPDATE | MI_SCF_CLEAR)) == 0 && b->pend[channel] == 0 && memcmp(&q, p, sizeof(q)) == 0)
            return MI_OK;
        q = *p;
        c.mode = p->mode, c.source = p->source, c.gain = p->gain;
        c.flags = p->flags & MI_SCF_MIDSIDE;
        b->pend[channel] = ring ? P_RING : 0;
        b->work = b->work || ring;
        b->up.touch(channel);
        return MI_OK;
    }

    int sidechain_bank_set_state(mi_sidechain_bank_t *b, uint32_t channel, float rms_value, uint32_t refresh, uint32_t position,
                                 bool zero_ring, hipStream_t st)
    {
        MI_REQUIRE(b != nullptr && channel < b->channels, MI_EINVAL, "sidechain_bank_set_state: bad argument");
        int r = mi::refuse_state_access(st);                        // before the ring's memset below could go into a capture
        if (r == MI_OK)
            r = sc_update(b, st);
        if (r != MI_OK)
            return r;
        const device_state s = { rms_value, (refresh < REFRESH_RATE) ? refresh : REFRESH_RATE,
                                 (position <= b->params[channel].capacity) ? position : position % b->params[channel].capacity, 0 };
        if (zero_ring)
            MI_HIP_CHECK(hipMemsetAsync(b->d_ring + size_t(channel) * b->ring_stride, 0, b->ring_stride * sizeof(float), st));
        return mi::write_state(b->d_state + channel, s, st);
    }
}

extern "C" {

int mi_sidechain_compute_params(uint32_t sample_rate, float max_reactivity, float reactivity, mi_sidechain_params_t *params)
{
    MI_REQUIRE(params != nullptr, MI_EINVAL, "mi_sidechain_compute_params: NULL argument");
    MI_REQUIRE(reactivity >= 0.0f && reactivity <= max_reactivity, MI_EINVAL,
               "mi_sidechain_compute_params: reactivity %g outside [0, %g]", double(reactivity), double(max_reactivity));
    *params = fresh_params();
    params->mode = params->source = 0;
    params->capacity = ring_capacity(sample_rate, max_reactivity);
    MI_REQUIRE(params->capacity > 0, MI_EINVAL, "mi_sidechain_compute_params: %g ms at %u Hz are too long", double(max_reactivity), sample_rate);
    compute_window(sample_rate, reactivity, *params);
    return MI_OK;
}

int mi_sidechain_bank_create(mi_sidechain_bank_t **bank, uint32_t channels, uint32_t inputs, float max_reactivity_ms)     // :67-86
{
    int r = mi_bank::open_checks(bank, "mi_sidechain_bank_create", channels);
    if (r != MI_OK)
        return r;
    MI_REQUIRE(inputs == 1 || inputs == 2, MI_EINVAL, "mi_sidechain_bank_create: %u inputs (1 or 2)", inputs);
    MI_REQUIRE(max_reactivity_ms >= 0.0f && max_reactivity_ms <= 1e6f, MI_EINVAL, "mi_sidechain_bank_create: maximum reactivity %g ms", double(max_reactivity_ms));
    r = mi_bank::open_new(bank, "mi_sidechain_bank_create");
    if (r != MI_OK)
        return r;
    r = sc_init(*bank, channels, inputs, max_reactivity_ms);
    if (r != MI_OK)
    {
        mi_sidechain_bank_destroy(*bank);
        *bank = nullptr;
    }
    return r;
}

int mi_sidechain_bank_destroy(mi_sidechain_bank_t *b)
{
    if (b == nullptr)
        return MI_OK;
    (void)hipFree(b->d_desc); (void)hipFree(b->d_ring);
    return mi_bank::destroy(b);
}

int mi_sidechain_bank_set_sample_rate(mi_sidechain_bank_t *b, uint32_t channel, uint32_t sample_rate)     // :88-93
{
    MI_BANK_SETTER("sidechain", "set_sample_rate");
    const uint32_t cap = ring_capacity(sample_rate, b->max_reactivity);
    MI_REQUIRE(cap > 0, MI_EINVAL, "mi_sidechain_bank_set_sample_rate: %g ms at %u Hz are too long", double(b->max_reactivity), sample_rate);
    c.sample_rate = sample_rate;
    c.flags = MI_SCF_UPDATE | MI_SCF_CLEAR;                     // :91 assigns: the mid-side flag goes too
    b->params[channel].capacity = cap;
    b->pend[channel] |= P_RING;
    b->work = true;
    return MI_OK;
}

int mi_sidechain_bank_set_reactivity(mi_sidechain_bank_t *b, uint32_t channel, float reactivity)          // :95-103
{
    MI_BANK_SETTER("sidechain", "set_reactivity");
    if (c.reactivity == reactivity || !(reactivity >= 0.0f) || reactivity > b->max_reactivity)
        return MI_OK;
    c.reactivity = reactivity;
    c.flags |= MI_SCF_UPDATE;
    b->work = true;
    return MI_OK;
}

int mi_sidechain_bank_set_stereo_mode(mi_sidechain_bank_t *b, uint32_t channel, uint32_t mode)            // :105-112
{
    MI_BANK_SETTER("sidechain", "set_stereo_mode");
    MI_REQUIRE(mode <= MI_SCSM_MIDSIDE, MI_EINVAL, "mi_sidechain_bank_set_stereo_mode: mode %u", mode);
    const uint32_t old = (c.flags & MI_SCF_MIDSIDE) ? MI_SCSM_MIDSIDE : MI_SCSM_STEREO;
    if (old == mode)
        return MI_OK;
    c.flags = (c.flags & ~uint32_t(MI_SCF_MIDSIDE)) | ((mode == MI_SCSM_MIDSIDE) ? MI_SCF_MIDSIDE : 0) | MI_SCF_CLEAR;
    b->work = true;
    return MI_OK;
}

int mi_sidechain_bank_set_source(mi_sidechain_bank_t *b, uint32_t channel, uint32_t source)               // Sidechain.h:146-149
{
    MI_BANK_SETTER("sidechain", "set_source");
    MI_REQUIRE(source <= MI_SCS_AMAX, MI_EINVAL, "mi_sidechain_bank_set_source: source %u", source);
    if (c.source == source)
        return MI_OK;
    c.source = source;
    b->up.touch(channel);
    return MI_OK;
}

int mi_sidechain_bank_set_mode(mi_sidechain_bank_t *b, uint32_t channel, uint32_t mode)                   // Sidechain.h:160-166
{
    MI_BANK_SETTER("sidechain", "set_mode");
    MI_REQUIRE(mode <= MI_SCM_UNIFORM, MI_EINVAL, "mi_sidechain_bank_set_mode: mode %u", mode);
    if (c.mode == mode)
        return MI_OK;
    c.mode = mode;
    b->pend[channel] |= P_ZERO_RMS;                             // fRmsValue = 0, no refresh
    b->work = true;
    b->up.touch(channel);
    return MI_OK;
}

int mi_sidechain_bank_set_gain(mi_sidechain_bank_t *b, uint32_t channel, float gain)                      // Sidechain.h:172-175
{
    MI_BANK_SETTER("sidechain", "set_gain");
    if (memcmp(&c.gain, &gain, sizeof(gain)) == 0)
        return MI_OK;
    c.gain = gain;
    b->up.touch(channel);
    return MI_OK;
}

int mi_sidechain_bank_clear(mi_sidechain_bank_t *b, uint32_t channel)                                     // :114-117
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_sidechain_bank_clear: NULL bank");
    MI_REQUIRE(channel < b->channels || channel == UINT32_MAX, MI_EINVAL, "mi_sidechain_bank_clear: channel %u out of range", channel);
    for (uint32_t ch = 0; ch < b->channels; ++ch)
        if (channel == UINT32_MAX || ch == channel)
            b->cfg[ch].flags |= MI_SCF_CLEAR;
    b->work = true;
    return MI_OK;
}

int mi_sidechain_bank_update_settings(mi_sidechain_bank_t *b, void *stream)                               // :119-142
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_sidechain_bank_update_settings: NULL bank");
    return sc_update(b, mi::as_stream(stream));
}

int mi_sidechain_bank_get_params(const mi_sidechain_bank_t *b, uint32_t channel, mi_sidechain_params_t *params)
{
    const int r = mi_bank::get_params(b, "mi_sidechain_bank_get_params", channel, params);
    if (r != MI_OK)
        return r;
    const channel_cfg &c = b->cfg[channel];
    params->mode = c.mode, params->source = c.source, params->flags = c.flags, params->gain = c.gain;
    return MI_OK;
}

int mi_sidechain_bank_get_state(mi_sidechain_bank_t *b, uint32_t channel, float *rms_value, uint32_t *refresh, uint32_t *position,
                                void *stream)
{
    device_state s;
    const int r = mi_bank::get_state(b, "mi_sidechain_bank_get_state", channel, &s, stream);
    if (r != MI_OK)
        return r;
    if (rms_value != nullptr) *rms_value = s.rms;
    if (refresh != nullptr) *refresh = s.refresh;
    if (position != nullptr) *position = s.head;
    return MI_OK;
}

int mi_sidechain_bank_process(mi_sidechain_bank_t *b, float *out, const float *in0, const float *in1, size_t count,
                              size_t out_stride, size_t in0_stride, size_t in1_stride, void *stream)      // :439-554
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_sidechain_bank_process: NULL bank");
    hipStream_t st = mi::as_stream(stream);
    const int r = sc_update(b, st);
    if (r != MI_OK || count == 0)
        return r;
    const bool two = b->inputs == 2;
    const int k = sc_check(b, "mi_sidechain_bank_process", out, in0, in1, count, out_stride, in0_stride, in1_stride, two);
    if (k != MI_OK)
        return k;
    return sc_launch(b, out, in0, (two && in0 != nullptr) ? in1 : nullptr, count, out_stride, in0_stride, in1_stride, two, st);
}

int mi_sidechain_bank_premix(mi_sidechain_bank_t *b, float *out, const float *in0, const float *in1, size_t count,
                             size_t out_stride, size_t in0_stride, size_t in1_stride, void *stream)       // :183-333 without abs
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_sidechain_bank_premix: NULL bank");
    hipStream_t st = mi::as_stream(stream);
    const int r = sc_update(b, st);
    if (r != MI_OK || count == 0)
        return r;
    const bool two = b->inputs == 2;
    const int k = sc_check(b, "mi_sidechain_bank_premix", out, in0, in1, count, out_stride, in0_stride, in1_stride, two);
    if (k != MI_OK)
        return k;
    MI_REQUIRE(b->channels <= 65535u, MI_EINVAL, "mi_sidechain_bank_premix: more than 65535 channels");
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    mi::take_profile_events(&ev0, &ev1);
    MI_LAUNCH(sidechain_premix_kernel, dim3(uint32_t((count + MIX_BLOCK - 1) / MIX_BLOCK), b->channels), dim3(MIX_BLOCK), 0, st, ev0, ev1,
              out, in0, (two && in0 != nullptr) ? in1 : nullptr, out_stride, in0_stride, in1_stride, uint32_t(count), uint32_t(two ? 1 : 0),
              b->d_params);
    MI_HIP_CHECK(hipGetLastError());
    return MI_OK;
}

int mi_sidechain_bank_process_premixed(mi_sidechain_bank_t *b, float *out, const float *in, size_t count, size_t out_stride,
                                       size_t in_stride, void *stream)
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_sidechain_bank_process_premixed: NULL bank");
    hipStream_t st = mi::as_stream(stream);
    const int r = sc_update(b, st);
    if (r != MI_OK || count == 0)
        return r;
    const int k = sc_check(b, "mi_sidechain_bank_process_premixed", out, in, nullptr, count, out_stride, in_stride, 0, false);
    if (k != MI_OK)
        return k;
    return sc_launch(b, out, in, nullptr, count, out_stride, in_stride, 0, false, st);
}

} // extern "C"
