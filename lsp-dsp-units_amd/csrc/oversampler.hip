// lsp::dspu::Oversampler as a bank of `channels` oversamplers (src/main/util/Oversampler.cpp): N-times Lanczos upsampling,
// the caller's work on the oversampled rows, the anti-alias low-pass and the decimation back.
//
// Upsampling is lanczos_device.h's gather with the values kept (coefficients, window, pairs, packed tap loop, tile fill
// and the planning of a launch are there, shared with truepeak.hip).  A sum starts from +0.0f, so a sum of negative zeros
// is +0; only the copied phase 0 can carry a -0 through.  State: [channels][124] on the device (nUpHead and the 12 K
// buffer of the reference hold pending sums and change no value).
//
// The taps take a = latency() (:955-1006).  For the *12BIT modes the reference says only "latency 4", the same as *X4;
// nothing here tells their kernels apart, so they take a = 4 and the *X4 table (unpinned).
//
// Kernel shape: a workgroup walks its row in tiles of inputs through LDS.  A thread owns 8 consecutive inputs and makes
// their 8 (N - 1) values phase by phase (coefficients in scalar registers, packed multiplies and adds for a <= 10, a tap
// loop over LDS for a = 62) into one LDS plane per phase; then the tile's N x 8 x BLOCK outputs leave as contiguous
// 16-byte stores, lane by lane adjacent, each lane picking its four values out of the planes.
#include "bank_core.h"
#include "lanczos_device.h"

#include <new>

#pragma clang fp contract(off)      // no fused multiply-add in the tap loops below: lanczos_device.h says why

namespace
{
    using namespace mi_lanczos;

    constexpr int      PT         = 8;                  // consecutive inputs of one thread
    constexpr int      A_MAX      = 62;                 // OVERSAMPLER_MAX_LATENCY
    constexpr int      STATE      = 2 * A_MAX;          // floats of state per channel (the first 2a are used)
    constexpr int      STAGE_BLOCK = 128;               // >= STATE
    constexpr uint32_t MAX_SPLITS = 64;                 // workgroups per row when few rows are long
    constexpr int      DOWN_BLOCK = 256;
    static_assert(STAGE_BLOCK >= STATE, "one thread per state value");

    // Oversampler::get_oversampling (:146-195) and latency (:955-1006) of a mode: modes 1 .. 30 are five groups of six
    __host__ __device__ constexpr int mode_times(uint32_t mode)
    {
        return (mode == 0 || mode > 30) ? 1 : (mode <= 6) ? 2 : (mode <= 12) ? 3 : (mode <= 18) ? 4 : (mode <= 24) ? 6 : 8;
    }
    __host__ __device__ constexpr int mode_a(uint32_t mode)
    {
        if (mode == 0 || mode > 30)
            return 0;
        const uint32_t k = (mode - 1) % 6;              // X2, X3, X4, 12BIT, 16BIT, 24BIT
        return (k == 0) ? 2 : (k == 1) ? 3 : (k == 2) ? 4 : (k == 3) ? 4 : (k == 4) ? 10 : 62;
    }

    // the device table: for each a of { 2, 3, 4, 10, 62 } phase_pairs of every N
    constexpr int LATENCIES[] = { 2, 3, 4, 10, 62 };
    constexpr int a_taps_before(int a) { return (a == 2) ? 0 : (a == 3) ? 4 : (a == 4) ? 10 : (a == 10) ? 18 : 38; }
    constexpr int TABLE_PAIRS = PHASES * (4 + 6 + 8 + 20 + 124);
    constexpr int table_offset(int n, int a) { return PHASES * a_taps_before(a) + phases_before(n) * 2 * a; }

    constexpr int block_of(int n) { return (n >= 6) ? 128 : 256; }      // 32 KB of LDS at every N

    template <int N, int A>
    struct shape
    {
        static constexpr int TAPS  = 2 * A;
        static constexpr int BLOCK = block_of(N);
        static constexpr int TILE  = BLOCK * PT;                // inputs per trip of a workgroup through LDS
        static constexpr int R     = PT + TAPS;                 // inputs behind one thread's outputs
        static constexpr int RL    = (R + 3) / 4 * 4;           // ... as whole float4 loads
        static constexpr int LIN   = TILE - PT + RL;            // lin[TAPS + p]: input p of the tile; lin[0 .. TAPS): before it
        static constexpr int PLANE = TILE + 8;                  // the planes of N = 8 half a bank row apart
        static_assert(BLOCK >= TAPS, "the carry is one value per thread");
    };

    // a <= 10: the outputs p = o .. o + 7 of phase k from r[j] = lin[o + j], the sums started from +0.0f, the values kept
    template <int N, int A>
    __device__ __forceinline__ void phases_packed(const float *lin, float *planes, const_pairs h, int o)
    {
        using S = shape<N, A>;
        constexpr int TAPS = S::TAPS;
        MI_LANCZOS_WINDOW(r, lin, o, S::RL)
        MI_LANCZOS_PAIRS(ev, od, r, S::R);
        #pragma unroll 1
        for (int k = 1; k < N; ++k)
        {
            const_pairs hk = h + (k - 1) * TAPS;
            float out[PT];
            #pragma unroll
            for (int q = 0; q < PT / 2; ++q)
            {
                MI_LANCZOS_PAIR_SUM(acc, hk, ev, od, TAPS, q, true);        // the sign of a zero is kept
                out[2 * q] = acc.x;
                out[2 * q + 1] = acc.y;
            }
            float *pl = planes + (k - 1) * S::PLANE + o;
            *reinterpret_cast<float4 *>(pl) = make_float4(out[0], out[1], out[2], out[3]);
            *reinterpret_cast<float4 *>(pl + 4) = make_float4(out[4], out[5], out[6], out[7]);
        }
    }

    // a = 62: four taps at a time over LDS; the 11 inputs behind 8 outputs and 4 taps sit in three aligned float4
    template <int N, int A>
    __device__ __forceinline__ void phases_looped(const float *lin, float *planes, const_pairs h, int o)
    {
        using S = shape<N, A>;
        constexpr int TAPS = S::TAPS;
        static_assert(TAPS % 4 == 0, "four taps per trip");
        #pragma unroll 1
        for (int k = 1; k < N; ++k)
        {
            const_pairs hk = h + (k - 1) * TAPS;
            float acc[PT];
            #pragma unroll
            for (int j = 0; j < PT; ++j)
                acc[j] = 0.0f;
            #pragma unroll 1
            for (int tb = TAPS - 4; tb >= 0; tb -= 4)
            {
                float w[12];
                const float *base = lin + (TAPS + o - tb - 4);
                #pragma unroll
                for (int j = 0; j < 3; ++j)
                {
                    const float4 v = *reinterpret_cast<const float4 *>(base + 4 * j);
                    w[4 * j] = v.x; w[4 * j + 1] = v.y; w[4 * j + 2] = v.z; w[4 * j + 3] = v.w;
                }
                #pragma unroll
                for (int tt = 3; tt >= 0; --tt)
                {
                    const float c = hk[tb + tt].x;
                    #pragma unroll
                    for (int j = 0; j < PT; ++j)
                        acc[j] = acc[j] + c * w[j + 4 - tt];    // lin[TAPS + o + j - t]
                }
            }
            float *pl = planes + (k - 1) * S::PLANE + o;
            *reinterpret_cast<float4 *>(pl) = make_float4(acc[0], acc[1], acc[2], acc[3]);
            *reinterpret_cast<float4 *>(pl + 4) = make_float4(acc[4], acc[5], acc[6], acc[7]);
        }
    }

    // One workgroup per (split, row): inputs [split * span, min(count, (split + 1) * span)) of the row, in lanczos_device.h's
    // tile walk.  dst and src are disjoint, so a later split reads the inputs before its
    // range from src; split 0 reads the state (splits == 1) or the copy oversampler_stage_kernel made of it.
    template <int N, int A>
    __global__ __launch_bounds__(block_of(N)) void oversampler_up_kernel(float *dst, const float *src, size_t dst_stride,
                                                                               size_t src_stride, uint32_t count, uint32_t span,
                                                                               uint32_t splits, float *state, const float *halo,
                                                                               const f32x2 *taps, int aligned)
    {
        using S = shape<N, A>;
        constexpr int TAPS = S::TAPS, BLOCK = S::BLOCK, TILE = S::TILE;
        __shared__ __attribute__((aligned(16))) float lin[S::LIN];
        __shared__ __attribute__((aligned(16))) float planes[(N - 1) * S::PLANE];
        const int tid = threadIdx.x;
        const uint32_t row = blockIdx.y, split = blockIdx.x;
        const float *xs = src + size_t(row) * src_stride;
        float *ys = dst + size_t(row) * dst_stride;
        const uint32_t begin = split * span, end = (count - begin < span) ? count : begin + span;
        const_pairs h = (const_pairs)taps;
        if (tid < TAPS)
            lin[tid] = (split != 0) ? xs[begin - TAPS + tid] : ((splits == 1) ? state : halo)[size_t(row) * STATE + tid];
        for (uint32_t t0 = begin; t0 < end; t0 += TILE)
        {
            const uint32_t n = (end - t0 < uint32_t(TILE)) ? end - t0 : uint32_t(TILE);
            MI_LANCZOS_FILL_TILE(lin, xs, t0, n, tid, TAPS, BLOCK, PT)
            __syncthreads();
            if constexpr (A <= 10)
                phases_packed<N, A>(lin, planes, h, tid * PT);
            else
                phases_looped<N, A>(lin, planes, h, tid * PT);
            // the next carry: the TAPS inputs before input n of this tile
            const float carry = (tid < TAPS) ? lin[n + tid] : 0.0f;
            __syncthreads();
            // output P of the tile is phase P % N of input P / N; phase 0 is the input a samples back, copied
            const uint32_t total = n * N;
            float *yt = ys + size_t(t0) * N;
            auto value = [&](uint32_t P) -> float {
                const uint32_t i = P / N, k = P % N;
                return (k == 0) ? lin[TAPS - A + i] : planes[(k - 1) * S::PLANE + i];
            };
            if (aligned)
            {
                #pragma unroll 2
                for (int it = 0; it < 2 * N; ++it)
                {
                    const uint32_t P = 4u * uint32_t(it * BLOCK + tid);
                    if (P + 3 < total)
                        *reinterpret_cast<float4 *>(yt + P) = make_float4(value(P), value(P + 1), value(P + 2), value(P + 3));
                    else if (P < total)
                        for (uint32_t e = P; e < total; ++e)
                            yt[e] = value(e);
                }
            }
            else
            {
                for (uint32_t P = uint32_t(tid); P < total; P += BLOCK)
                    yt[P] = value(P);
            }
            __syncthreads();
            if (tid < TAPS)
                lin[tid] = carry;
        }
        if (splits == 1 && tid < TAPS)
            state[size_t(row) * STATE + tid] = lin[tid];       // written by the thread that wrote it into LDS
    }

    // Before a split launch, one workgroup per row: halo[row] = the state, and the new state = the last `taps` inputs of
    // the call.  All of them are read before any is written.  (truepeak_stage_kernel is a different kernel on purpose: the
    // meter runs in place, so it has to copy the inputs before every split as well.)
    __global__ __launch_bounds__(STAGE_BLOCK) void oversampler_stage_kernel(const float *src, size_t src_stride, uint32_t count,
                                                                            uint32_t taps, float *state, float *halo)
    {
        const uint32_t tid = threadIdx.x, row = blockIdx.x;
        const float *xs = src + size_t(row) * src_stride;
        float *st = state + size_t(row) * STATE;
        float old = 0.0f, nw = 0.0f;
        if (tid < taps)
        {
            old = st[tid];
            nw = (count >= taps - tid) ? xs[count - taps + tid] : st[tid + count];
        }
        __syncthreads();
        if (tid < taps)
        {
            halo[size_t(row) * STATE + tid] = old;
            st[tid] = nw;
        }
    }

    // dsp::downsample_Nx: dst[i] = src[N i].  Four outputs per thread, one 16-byte store where the row allows it.
    __global__ __launch_bounds__(DOWN_BLOCK) void oversampler_down_kernel(float *dst, const float *src, size_t dst_stride,
                                                                          size_t src_stride, uint32_t count, uint32_t times, int aligned)
    {
        const uint32_t row = blockIdx.y;
        const uint32_t i0 = 4u * (blockIdx.x * DOWN_BLOCK + threadIdx.x);
        const float *xs = src + size_t(row) * src_stride;
        float *ys = dst + size_t(row) * dst_stride;
        if (i0 >= count)
            return;
        if (aligned && i0 + 3 < count)
        {
            const float *p = xs + size_t(i0) * times;
            *reinterpret_cast<float4 *>(ys + i0) = make_float4(p[0], p[times], p[2 * size_t(times)], p[3 * size_t(times)]);
        }
        else
        {
            for (uint32_t i = i0; i < count && i < i0 + 4; ++i)
                ys[i] = xs[size_t(i) * times];
        }
    }

    // update_t of the reference (Oversampler.h:113-120)
    enum { UP_MODE = 1 << 0, UP_SAMPLE_RATE = 1 << 2, UP_OTHER = 1 << 3, UP_ALL = UP_MODE | UP_OTHER | UP_SAMPLE_RATE };
    constexpr uint32_t FILTER_SECTIONS = 32;            // FILTER_CHAINS_MAX: what a design can hold
} // namespace

struct mi_oversampler_bank
{
    uint32_t            channels = 0;
    uint32_t            mode = MI_OM_NONE;          // nMode: the kernels follow it at once, as pFunc does
    uint32_t            sample_rate = 0;            // nSampleRate
    uint32_t            update = UP_ALL;            // nUpdate
    bool                filter = true;              // bFilter
    mi_filter_params_t  params = { MI_FLT_NONE, 1, 0.0f, 0.0f, 0.0f, 0.0f };   // sFilter's
    uint32_t            design_rate = 0;            // ... and the rate it is designed at
    mi_filter_params_t  live_params = { MI_FLT_NONE, 1, 0.0f, 0.0f, 0.0f, 0.0f };   // what the biquad bank runs
    uint32_t            live_rate = 0;
    uint32_t            sections = 0;
    mi_biquad_bank_t   *biquads = nullptr;
    float              *d_state = nullptr;          // [channels][STATE]
    float              *d_halo = nullptr;           // [channels][STATE]
    f32x2              *d_taps = nullptr;           // TABLE_PAIRS
    float              *d_scratch = nullptr;        // [channels][scratch stride] of process() and the filtered downsample()
    size_t              scratch_cap = 0;            // floats
};

namespace
{
    inline size_t round4(size_t v) { return (v + 3) & ~size_t(3); }

    bool same_params(const mi_filter_params_t &a, const mi_filter_params_t &b)
    {
        return a.nType == b.nType && a.nSlope == b.nSlope && a.fFreq == b.fFreq && a.fFreq2 == b.fFreq2 && a.fGain == b.fGain &&
               a.fQuality == b.fQuality;
    }

    // the scratch rows of a call of `count` samples at the current factor
    int os_reserve(mi_oversampler_bank *b, size_t count, hipStream_t st)
    {
        const size_t need = size_t(b->channels) * round4(count * size_t(mode_times(b->mode)));
        if (need <= b->scratch_cap)
            return MI_OK;
        bool cap = false;
        const int r = capturing(st, &cap);
        if (r != MI_OK)
            return r;
        MI_REQUIRE(!cap, MI_ESTATE, "mi_oversampler_bank: the scratch buffer has to grow; call reserve() before capturing");
        (void)hipFree(b->d_scratch);
        b->d_scratch = nullptr;
        b->scratch_cap = 0;
        MI_HIP_CHECK(hipMalloc(reinterpret_cast<void **>(&b->d_scratch), need * sizeof(float)));
        b->scratch_cap = need;
        return MI_OK;
    }

    // Oversampler::update_settings, Oversampler.cpp:128-144
    int os_update(mi_oversampler_bank *b, hipStream_t st)
    {
        const uint32_t rate = b->sample_rate * uint32_t(mode_times(b->mode));
        const bool redesign = rate != b->live_rate || !same_params(b->params, b->live_params);
        if (b->update == 0 && !redesign)
            return MI_OK;
        bool cap = false;
        int r = capturing(st, &cap);
        if (r != MI_OK)
            return r;
        MI_REQUIRE(!cap, MI_ESTATE, "mi_oversampler_bank: changed settings clear the state and re-design the filter; call "
                                    "update_settings() before capturing");
        const bool clear = (b->update & (UP_MODE | UP_SAMPLE_RATE)) != 0;
        if (clear)
            MI_HIP_CHECK(hipMemsetAsync(b->d_state, 0, size_t(b->channels) * STATE * sizeof(float), st));
        b->design_rate = rate;
        if (redesign)
        {
            mi_biquad_x1_t sec[FILTER_SECTIONS];
            uint32_t n = 0;
            int fmode = MI_FM_BYPASS;
            if (b->params.nType != MI_FLT_NONE && rate != 0)
            {
                r = mi_filter_design(&b->params, rate, sec, FILTER_SECTIONS, &n, nullptr, 0, nullptr, &fmode);
                if (r != MI_OK)
                    return r;
                MI_REQUIRE(n <= FILTER_SECTIONS, MI_ESTATE, "mi_oversampler_bank: the anti-alias design has %u sections", n);
            }
            if (fmode == MI_FM_BYPASS)
                n = 0;
            for (uint32_t c = 0; c < b->channels; ++c)
            {
                r = mi_biquad_bank_set_chains(b->biquads, c, sec, n, clear ? 1 : 0);
                if (r != MI_OK)
                    return r;
            }
            b->sections = n;
            b->live_params = b->params;
            b->live_rate = rate;
            r = mi_biquad_bank_commit(b->biquads, st);
        }
        if (r == MI_OK && clear)
            r = mi_biquad_bank_reset(b->biquads, UINT32_MAX, st);       // sFilter.clear()
        if (r != MI_OK)
            return r;
        b->update = 0;
        return MI_OK;
    }

    int os_copy(mi_oversampler_bank *b, float *dst, const float *src, size_t count, size_t dst_stride, size_t src_stride, hipStream_t st)
    {
        if (dst == src)
            return MI_OK;
        if (b->channels == 1)                                   // (one row: the strides mean nothing and may be 0)
            MI_HIP_CHECK(hipMemcpyAsync(dst, src, count * sizeof(float), hipMemcpyDeviceToDevice, st));
        else
            MI_HIP_CHECK(hipMemcpy2DAsync(dst, dst_stride * sizeof(float), src, src_stride * sizeof(float), count * sizeof(float),
                                          b->channels, hipMemcpyDeviceToDevice, st));
        return MI_OK;
    }

    template <int N, int A>
    void up_launch(mi_oversampler_bank *b, float *dst, const float *src, uint32_t count, size_t dst_stride, size_t src_stride,
                   hipStream_t st, hipEvent_t ev0, hipEvent_t ev1, int aligned)
    {
        using S = shape<N, A>;
        const split_plan plan = plan_splits(count, S::TILE, b->channels, MAX_SPLITS);
        const uint32_t splits = plan.splits, span = plan.span;
        if (splits > 1)
            hipLaunchKernelGGL(oversampler_stage_kernel, dim3(b->channels), dim3(STAGE_BLOCK), 0, st, src, src_stride, count,
                               uint32_t(S::TAPS), b->d_state, b->d_halo);
        MI_LAUNCH((oversampler_up_kernel<N, A>), dim3(splits, b->channels), dim3(S::BLOCK), 0, st, ev0, ev1, dst, src, dst_stride,
                  src_stride, count, span, splits, b->d_state, b->d_halo, b->d_taps + table_offset(N, A), aligned);
    }

    int os_upsample(mi_oversampler_bank *b, float *dst, const float *src, uint32_t count, size_t dst_stride, size_t src_stride,
                    hipStream_t st)
    {
        const int aligned = (reinterpret_cast<uintptr_t>(dst) % 16 == 0 && dst_stride % 4 == 0) ? 1 : 0;
        hipEvent_t ev0 = nullptr, ev1 = nullptr;
        mi::take_profile_events(&ev0, &ev1);
        #define MI_OS_UP(N_, A_) up_launch<N_, A_>(b, dst, src, count, dst_stride, src_stride, st, ev0, ev1, aligned)
        #define MI_OS_UP_A(N_) \
            switch (mode_a(b->mode)) \
            { \
                case 2:  MI_OS_UP(N_, 2); break; \
                case 3:  MI_OS_UP(N_, 3); break; \
                case 4:  MI_OS_UP(N_, 4); break; \
                case 10: MI_OS_UP(N_, 10); break; \
                default: MI_OS_UP(N_, 62); break; \
            }
        switch (mode_times(b->mode))
        {
            case 2:  MI_OS_UP_A(2); break;
            case 3:  MI_OS_UP_A(3); break;
            case 4:  MI_OS_UP_A(4); break;
            case 6:  MI_OS_UP_A(6); break;
            default: MI_OS_UP_A(8); break;
        }
        #undef MI_OS_UP_A
        #undef MI_OS_UP
        MI_HIP_CHECK(hipGetLastError());
        return MI_OK;
    }

    int os_decimate(mi_oversampler_bank *b, float *dst, const float *src, uint32_t count, size_t dst_stride, size_t src_stride,
                    hipStream_t st)
    {
        const int aligned = (reinterpret_cast<uintptr_t>(dst) % 16 == 0 && dst_stride % 4 == 0) ? 1 : 0;
        hipEvent_t ev0 = nullptr, ev1 = nullptr;
        mi::take_profile_events(&ev0, &ev1);
        const dim3 grid((count + 4 * DOWN_BLOCK - 1) / (4 * DOWN_BLOCK), b->channels);
        MI_LAUNCH(oversampler_down_kernel, grid, dim3(DOWN_BLOCK), 0, st, ev0, ev1, dst, src, dst_stride, src_stride, count,
                  uint32_t(mode_times(b->mode)), aligned);
        MI_HIP_CHECK(hipGetLastError());
        return MI_OK;
    }

    // rows of count x times samples.  in_place: dst may be src (process()); upsample() and downsample() refuse that themselves
    int os_check(const mi_oversampler_bank *b, const char *what, const void *dst, const void *src, size_t count, size_t dst_stride,
                 size_t src_stride, size_t dst_times, size_t src_times, bool in_place)
    {
        return mi_bank::check_rows(what, b->channels, count, size_t(1) << 27,
                                   { { dst, dst_stride, count * dst_times, mi_bank::REQUIRED | (in_place ? mi_bank::OUTPUT : 0u) },
                                     { src, src_stride, count * src_times, mi_bank::REQUIRED } });
    }
} // namespace

extern "C" {

int mi_oversampler_coefficients(uint32_t mode, float *h, size_t *count)
{
    MI_REQUIRE(count != nullptr, MI_EINVAL, "mi_oversampler_coefficients: NULL count");
    MI_REQUIRE(mode <= MI_OM_LANCZOS_8X24BIT, MI_EINVAL, "mi_oversampler_coefficients: no mode %u", mode);
    const int n = mode_times(mode), a = mode_a(mode);
    *count = (mode == MI_OM_NONE) ? 0 : size_t(n) * 2 * a;
    if (h != nullptr && mode != MI_OM_NONE)
        make_table(n, a, h);
    return MI_OK;
}

int mi_oversampler_bank_create(mi_oversampler_bank_t **bank, uint32_t channels)        // Oversampler.cpp:53-93
{
    int r = mi_bank::open(bank, "mi_oversampler_bank_create", channels, 65535u);
    if (r != MI_OK)
        return r;
    mi_oversampler_bank *b = *bank;
    *bank = nullptr;
    f32x2 *table = new (std::nothrow) f32x2[TABLE_PAIRS];
    if (table == nullptr)
    {
        delete b;
        return mi::fail(MI_ENOMEM, "mi_oversampler_bank_create: out of host memory");
    }
    b->channels = channels;
    for (int a : LATENCIES)
        for (int n : FACTORS)
            phase_pairs(n, a, table + table_offset(n, a));
    r = mi_biquad_bank_create(&b->biquads, channels, FILTER_SECTIONS);
    hipError_t e = hipSuccess;
    if (r == MI_OK)
    {
        e = hipMalloc(reinterpret_cast<void **>(&b->d_state), size_t(channels) * STATE * sizeof(float));
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&b->d_halo), size_t(channels) * STATE * sizeof(float));
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&b->d_taps), TABLE_PAIRS * sizeof(f32x2));
        if (e == hipSuccess) e = hipMemcpy(b->d_taps, table, TABLE_PAIRS * sizeof(f32x2), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemset(b->d_state, 0, size_t(channels) * STATE * sizeof(float));
    }
    delete[] table;
    if (r != MI_OK || e != hipSuccess)
    {
        mi_oversampler_bank_destroy(b);
        return (r != MI_OK) ? r : mi::fail(MI_EHIP, "mi_oversampler_bank_create: %s", hipGetErrorString(e));
    }
    *bank = b;
    return MI_OK;
}

int mi_oversampler_bank_destroy(mi_oversampler_bank_t *b)                               // Oversampler.cpp:95-106
{
    if (b == nullptr)
        return MI_OK;
    mi_biquad_bank_destroy(b->biquads);
    (void)hipFree(b->d_state); (void)hipFree(b->d_halo); (void)hipFree(b->d_taps); (void)hipFree(b->d_scratch);
    delete b;
    return MI_OK;
}

int mi_oversampler_bank_set_sample_rate(mi_oversampler_bank_t *b, uint32_t sample_rate) // Oversampler.cpp:108-126
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_oversampler_bank_set_sample_rate: NULL bank");
    if (b->sample_rate == sample_rate)
        return MI_OK;
    b->sample_rate = sample_rate;
    b->update |= UP_SAMPLE_RATE;
    const float cutoff = float(sample_rate) * 0.42f;
    b->params.fFreq = (cutoff < 20000.0f) ? cutoff : 20000.0f;      // lsp_min(OS_CUTOFF, sr * 0.42f)
    b->params.fFreq2 = b->params.fFreq;
    b->params.fGain = 1.0f;
    b->params.fQuality = 0.1f;
    b->params.nSlope = 30;
    b->params.nType = MI_FLT_BT_BWC_LOPASS;
    b->design_rate = sample_rate * uint32_t(mode_times(b->mode));
    return mi_filter_limit(&b->params, b->design_rate);              // Filter::update keeps the limited parameters
}

int mi_oversampler_bank_set_mode(mi_oversampler_bank_t *b, uint32_t mode)               // Oversampler.cpp:1055-1063
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_oversampler_bank_set_mode: NULL bank");
    MI_REQUIRE(mode <= MI_OM_LANCZOS_8X24BIT, MI_EINVAL, "mi_oversampler_bank_set_mode: no mode %u", mode);
    if (b->mode == mode)
        return MI_OK;
    b->mode = mode;
    b->update |= UP_MODE;
    return MI_OK;
}

int mi_oversampler_bank_mode(const mi_oversampler_bank_t *b, uint32_t *mode)            // Oversampler.cpp:1065-1068
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_oversampler_bank_mode: NULL bank");
    MI_REQUIRE(mode != nullptr, MI_EINVAL, "mi_oversampler_bank_mode: NULL result pointer");
    *mode = b->mode;
    return MI_OK;
}

int mi_oversampler_bank_set_filtering(mi_oversampler_bank_t *b, int on)                 // Oversampler.h:191-197
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_oversampler_bank_set_filtering: NULL bank");
    if (b->filter == (on != 0))
        return MI_OK;
    b->filter = on != 0;
    b->update |= UP_MODE;
    return MI_OK;
}

int mi_oversampler_bank_filtering(const mi_oversampler_bank_t *b, int *on)              // Oversampler.cpp:1070-1073
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_oversampler_bank_filtering: NULL bank");
    MI_REQUIRE(on != nullptr, MI_EINVAL, "mi_oversampler_bank_filtering: NULL result pointer");
    *on = b->filter ? 1 : 0;
    return MI_OK;
}

int mi_oversampler_bank_modified(const mi_oversampler_bank_t *b, int *yes)              // Oversampler.h:209-212
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_oversampler_bank_modified: NULL bank");
    MI_REQUIRE(yes != nullptr, MI_EINVAL, "mi_oversampler_bank_modified: NULL result pointer");
    *yes = (b->update != 0) ? 1 : 0;
    return MI_OK;
}

int mi_oversampler_bank_update_settings(mi_oversampler_bank_t *b, void *stream)         // Oversampler.cpp:128-144
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_oversampler_bank_update_settings: NULL bank");
    return os_update(b, mi::as_stream(stream));
}

int mi_oversampler_bank_oversampling(const mi_oversampler_bank_t *b, uint32_t *times)   // Oversampler.cpp:146-195
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_oversampler_bank_oversampling: NULL bank");
    MI_REQUIRE(times != nullptr, MI_EINVAL, "mi_oversampler_bank_oversampling: NULL result pointer");
    *times = uint32_t(mode_times(b->mode));
    return MI_OK;
}

int mi_oversampler_bank_latency(const mi_oversampler_bank_t *b, uint32_t *samples)      // Oversampler.cpp:955-1006
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_oversampler_bank_latency: NULL bank");
    MI_REQUIRE(samples != nullptr, MI_EINVAL, "mi_oversampler_bank_latency: NULL result pointer");
    *samples = uint32_t(mode_a(b->mode));
    return MI_OK;
}

int mi_oversampler_bank_max_latency(const mi_oversampler_bank_t *b, uint32_t *samples)  // Oversampler.h:281
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_oversampler_bank_max_latency: NULL bank");
    MI_REQUIRE(samples != nullptr, MI_EINVAL, "mi_oversampler_bank_max_latency: NULL result pointer");
    *samples = uint32_t(A_MAX);
    return MI_OK;
}

int mi_oversampler_bank_reserve(mi_oversampler_bank_t *b, size_t count)
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_oversampler_bank_reserve: NULL bank");
    MI_REQUIRE(count < (size_t(1) << 27), MI_EINVAL, "mi_oversampler_bank_reserve: count %zu too large", count);
    return os_reserve(b, count, nullptr);
}

int mi_oversampler_bank_set_exact(mi_oversampler_bank_t *b, int on)
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_oversampler_bank_set_exact: NULL bank");
    return mi_biquad_bank_set_exact(b->biquads, on);
}

int mi_oversampler_bank_get_filter(const mi_oversampler_bank_t *b, mi_filter_params_t *params, uint32_t *sample_rate)
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_oversampler_bank_get_filter: NULL bank");
    MI_REQUIRE(params != nullptr, MI_EINVAL, "mi_oversampler_bank_get_filter: NULL result pointer");
    *params = b->params;
    if (sample_rate != nullptr)
        *sample_rate = b->design_rate;
    return MI_OK;
}

int mi_oversampler_bank_upsample(mi_oversampler_bank_t *b, float *dst, const float *src, size_t count, size_t dst_stride,
                                 size_t src_stride, void *stream)                          // Oversampler.cpp:197-367
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_oversampler_bank_upsample: NULL bank");
    if (count == 0)
        return MI_OK;
    const size_t n = size_t(mode_times(b->mode));
    const int r = os_check(b, "mi_oversampler_bank_upsample", dst, src, count, dst_stride, src_stride, n, 1, false);
    if (r != MI_OK)
        return r;
    MI_REQUIRE(dst != src, MI_EINVAL, "mi_oversampler_bank_upsample: dst and src must not overlap");
    hipStream_t st = mi::as_stream(stream);
    if (b->mode == MI_OM_NONE)
        return os_copy(b, dst, src, count, dst_stride, src_stride, st);
    return os_upsample(b, dst, src, uint32_t(count), dst_stride, src_stride, st);
}

int mi_oversampler_bank_downsample(mi_oversampler_bank_t *b, float *dst, const float *src, size_t count, size_t dst_stride,
                                   size_t src_stride, void *stream)                        // Oversampler.cpp:369-525
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_oversampler_bank_downsample: NULL bank");
    if (count == 0)
        return MI_OK;
    const size_t n = size_t(mode_times(b->mode));
    int r = os_check(b, "mi_oversampler_bank_downsample", dst, src, count, dst_stride, src_stride, 1, n, false);
    if (r != MI_OK)
        return r;
    MI_REQUIRE(dst != src, MI_EINVAL, "mi_oversampler_bank_downsample: dst and src must not overlap");
    hipStream_t st = mi::as_stream(stream);
    if (b->mode == MI_OM_NONE)
        return os_copy(b, dst, src, count, dst_stride, src_stride, st);
    if (b->filter && b->sections != 0)
    {
        r = os_reserve(b, count, st);
        if (r != MI_OK)
            return r;
        const size_t ss = round4(count * n);
        r = mi_biquad_bank_process(b->biquads, b->d_scratch, src, count * n, ss, src_stride, stream);
        if (r != MI_OK)
            return r;
        return os_decimate(b, dst, b->d_scratch, uint32_t(count), dst_stride, ss, st);
    }
    return os_decimate(b, dst, src, uint32_t(count), dst_stride, src_stride, st);
}

int mi_oversampler_bank_process(mi_oversampler_bank_t *b, float *dst, const float *src, size_t count, size_t dst_stride,
                                size_t src_stride, mi_oversampler_callback_t callback, void *arg, void *stream)
{                                                                                           // Oversampler.cpp:527-953
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_oversampler_bank_process: NULL bank");
    if (count == 0)
        return MI_OK;
    int r = os_check(b, "mi_oversampler_bank_process", dst, src, count, dst_stride, src_stride, 1, 1, true);
    if (r != MI_OK)
        return r;
    hipStream_t st = mi::as_stream(stream);
    if (b->mode == MI_OM_NONE)                              // :731-737: the callback sees the base-rate rows, or a copy happens
    {
        r = os_copy(b, dst, src, count, dst_stride, src_stride, st);
        if (r == MI_OK && callback != nullptr)
            r = callback(dst, count, dst_stride, b->channels, stream, arg);
        return r;
    }
    r = os_reserve(b, count, st);
    if (r != MI_OK)
        return r;
    const size_t n = size_t(mode_times(b->mode)), ss = round4(count * n);
    r = os_upsample(b, b->d_scratch, src, uint32_t(count), ss, src_stride, st);
    if (r == MI_OK && callback != nullptr)
        r = callback(b->d_scratch, count * n, ss, b->channels, stream, arg);
    if (r == MI_OK && b->filter && b->sections != 0)
        r = mi_biquad_bank_process(b->biquads, b->d_scratch, b->d_scratch, count * n, ss, ss, stream);
    if (r != MI_OK)
        return r;
    return os_decimate(b, dst, b->d_scratch, uint32_t(count), dst_stride, ss, st);
}

} // extern "C"
