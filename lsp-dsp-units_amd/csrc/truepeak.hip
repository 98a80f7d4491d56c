// lsp::dspu::TruePeakMeter as a bank of `channels` meters (src/main/meters/TruePeakMeter.cpp): ITU-R BS.1770-4 Annex 2
// true peak.  Each input is upsampled N times (N from the sample rate, :85-100) by the Lanczos kernel of lsp-dsp-lib's
// lanczos_resample_Nx16bit (a = 10) and every output is the largest magnitude of its N oversampled values (reduce_Nx,
// :115-147).
//
// The oversampled values (coefficients, window, pairs, packed tap loop, tile fill) and the planning of a launch are
// lanczos_device.h's, shared with oversampler.hip.  The meter's own: the largest magnitude of every N values, kept in
// registers, and the splits of an in-place call.  State: [channels][2a] on the device.
//
// process_max: the reference's (:238-272) returns 0.0f and looks at only `to_process` of the N * to_process oversampled
// values.  Here it is what the header documents: the largest value process() would have written, with the state
// advanced exactly as process() advances it.
#include "bank_core.h"
#include "lanczos_device.h"

#include <new>

#pragma clang fp contract(off)      // no fused multiply-add in the tap loops below: lanczos_device.h says why

namespace
{
    using namespace mi_lanczos;

    constexpr int      A          = 10;                 // Lanczos a of the *16bit kernels (TRUE_PEAK_LATENCY, :34)
    constexpr int      TAPS       = 2 * A;              // inputs behind one oversampled value; the state per channel
    constexpr int      BLOCK      = 256;
    constexpr int      PER_THREAD = 8;                  // consecutive outputs of one thread (four pairs of packed lanes)
    constexpr int      TILE       = BLOCK * PER_THREAD; // inputs per trip of a workgroup through LDS
    constexpr uint32_t MAX_SPLITS = 64;                 // workgroups per row when few rows are long
    constexpr uint32_t SPLIT_ROWS = 256;                // rows up to which a row may be split
    constexpr int      STAGE_ITEMS = 6;                 // per thread of the staging kernel: (MAX_SPLITS + 1) * TAPS <= 6 * BLOCK
    static_assert((MAX_SPLITS + 1) * TAPS <= STAGE_ITEMS * BLOCK, "staging items");

    constexpr int      TABLE_PAIRS = PHASES * TAPS; // the device table: phase_pairs of every N
    __host__ __device__ constexpr int table_offset(int n) { return phases_before(n) * TAPS; }

    // TruePeakMeter::calc_oversampling_multiplier, TruePeakMeter.cpp:85-100 (TRUE_PEAK_FREQUENCY = 4 * 44100)
    uint32_t oversampling(uint32_t sr)
    {
        const uint64_t f = 4 * 44100, s = sr;
        return (s >= f) ? 0 : (s * 2 >= f) ? 2 : (s * 3 >= f) ? 3 : (s * 4 >= f) ? 4 : (s * 6 >= f) ? 6 : 8;
    }

    // One trip's worth of outputs of one thread: p = o .. o + PER_THREAD - 1 of the tile, from r[j] = lds[o + j]: the
    // largest magnitude over the phases
    template <int N>
    __device__ __forceinline__ void tile_outputs(const float *r, const_pairs h, float *out)
    {
        MI_LANCZOS_PAIRS(ev, od, r, PER_THREAD + TAPS);
        #pragma unroll
        for (int j = 0; j < PER_THREAD; ++j)
            out[j] = fabsf(r[TAPS + j - A]);                    // k = 0: y[N i] = x[i - a]
        #pragma unroll 1
        for (int k = 1; k < N; ++k)
        {
            const_pairs hk = h + (k - 1) * TAPS;
            #pragma unroll
            for (int q = 0; q < PER_THREAD / 2; ++q)
            {
                MI_LANCZOS_PAIR_SUM(acc, hk, ev, od, TAPS, q, false);       // |.| drops the sign of a zero
                out[2 * q] = fmaxf(out[2 * q], fabsf(acc.x));
                out[2 * q + 1] = fmaxf(out[2 * q + 1], fabsf(acc.y));
            }
        }
    }

    template <>
    __device__ __forceinline__ void tile_outputs<0>(const float *r, const_pairs, float *out)
    {
        #pragma unroll
        for (int j = 0; j < PER_THREAD; ++j)
            out[j] = fabsf(r[TAPS + j]);                        // dsp::abs2 (:202-205)
    }

    // One workgroup per (split, row): inputs [split * span, min(count, (split + 1) * span)) of the row, in lanczos_device.h's
    // tile walk.  The whole tile is in LDS before any output is stored, so dst may be src:
    // with one split the workgroup owns its row; with several the inputs before each split were staged beforehand
    // (truepeak_stage_kernel), and no workgroup reads inputs of another split's range.
    // MAX: no dst; the largest output of the range goes to peaks[row] (atomically when the row is split; peaks zeroed first).
    template <int N, bool MAX>
    __global__ __launch_bounds__(BLOCK) void truepeak_kernel(float *dst, const float *src, size_t dst_stride,
                                                             size_t src_stride, uint32_t count, uint32_t span, uint32_t splits,
                                                             float *state, const float *halo, const f32x2 *taps, float *peaks)
    {
        __shared__ __attribute__((aligned(16))) float lin[TILE + TAPS];
        __shared__ __attribute__((aligned(16))) float lout[MAX ? 1 : TILE];
        __shared__ float wmax[BLOCK / 64];
        const int tid = threadIdx.x;
        const uint32_t row = blockIdx.y, split = blockIdx.x;
        const float *xs = src + size_t(row) * src_stride;
        const uint32_t begin = split * span, end = (count - begin < span) ? count : begin + span;
        const_pairs h = (const_pairs)(taps + ((N > 0) ? table_offset(N) : 0));
        if (tid < TAPS)
            lin[tid] = (N == 0) ? 0.0f : (splits == 1) ? state[size_t(row) * TAPS + tid] : halo[(size_t(row) * splits + split) * TAPS + tid];
        float mx = 0.0f;
        for (uint32_t t0 = begin; t0 < end; t0 += TILE)
        {
            const uint32_t n = (end - t0 < uint32_t(TILE)) ? end - t0 : uint32_t(TILE);
            MI_LANCZOS_FILL_TILE(lin, xs, t0, n, tid, TAPS, BLOCK, PER_THREAD)
            __syncthreads();
            const int o = tid * PER_THREAD;
            MI_LANCZOS_WINDOW(r, lin, o, PER_THREAD + TAPS)
            float out[PER_THREAD];
            tile_outputs<N>(r, h, out);
            if (MAX)
            {
                #pragma unroll
                for (int j = 0; j < PER_THREAD; ++j)
                    mx = (uint32_t(o + j) < n) ? fmaxf(mx, out[j]) : mx;
            }
            else
            {
                #pragma unroll
                for (int j = 0; j < PER_THREAD; j += 4)
                    *reinterpret_cast<float4 *>(&lout[o + j]) = make_float4(out[j], out[j + 1], out[j + 2], out[j + 3]);
            }
            // the next carry: the TAPS inputs before input n of this tile
            const float carry = (tid < TAPS) ? lin[n + tid] : 0.0f;
            __syncthreads();
            if (!MAX)
            {
                float *ys = dst + size_t(row) * dst_stride + t0;
                #pragma unroll
                for (int j = 0; j < PER_THREAD; ++j)
                {
                    const uint32_t p = uint32_t(j * BLOCK + tid);
                    if (p < n)
                        ys[p] = lout[p];
                }
            }
            if (tid < TAPS)
                lin[tid] = carry;
        }
        if (N != 0 && splits == 1 && tid < TAPS)
            state[size_t(row) * TAPS + tid] = lin[tid];        // written by the thread that wrote it into LDS
        if (MAX)
        {
            #pragma unroll
            for (int d = 32; d >= 1; d >>= 1)
                mx = fmaxf(mx, __shfl_xor(mx, d, 64));
            if ((tid & 63) == 0)
                wmax[tid >> 6] = mx;
            __syncthreads();
            if (tid == 0)
            {
                float v = wmax[0];
                #pragma unroll
                for (int w = 1; w < BLOCK / 64; ++w)
                    v = fmaxf(v, wmax[w]);
                if (splits == 1)
                    peaks[row] = v;
                else                                            // non-negative floats order as their bit patterns
                    atomicMax(reinterpret_cast<unsigned int *>(peaks + row), __float_as_uint(v));
            }
        }
    }

    // Before a split launch, one workgroup per row: halo[row][s] = the TAPS inputs before split s (split 0: the state), and
    // the new state = the last TAPS inputs of the call.  All of them are read before any is written, so the state may be
    // overwritten here and the splits of an in-place call find their halos intact.  (oversampler_stage_kernel is a
    // different kernel on purpose: upsampling never runs in place, so its splits read their halos from src.)
    __global__ __launch_bounds__(BLOCK) void truepeak_stage_kernel(const float *src, size_t src_stride, uint32_t count, uint32_t span,
                                                                   uint32_t splits, float *state, float *halo)
    {
        const int tid = threadIdx.x;
        const uint32_t row = blockIdx.x, items = (splits + 1) * TAPS;
        const float *xs = src + size_t(row) * src_stride;
        float *st = state + size_t(row) * TAPS;
        float v[STAGE_ITEMS];
        #pragma unroll
        for (int i = 0; i < STAGE_ITEMS; ++i)
        {
            const uint32_t e = uint32_t(i * BLOCK + tid), s = e / TAPS, j = e % TAPS;
            float x = 0.0f;
            if (e < splits * TAPS)
                x = (s == 0) ? st[j] : xs[s * span - TAPS + j];
            else if (e < items)
                x = (count >= TAPS - j) ? xs[count - TAPS + j] : st[j + count];
            v[i] = x;
        }
        __syncthreads();
        #pragma unroll
        for (int i = 0; i < STAGE_ITEMS; ++i)
        {
            const uint32_t e = uint32_t(i * BLOCK + tid);
            if (e < splits * TAPS)
                halo[size_t(row) * splits * TAPS + e] = v[i];
            else if (e < items)
                st[e - splits * TAPS] = v[i];
        }
    }
} // namespace

struct mi_truepeak_bank
{
    uint32_t    channels = 0;
    uint32_t    sample_rate = 0;        // nSampleRate: 0 as constructed
    uint32_t    times = 0;              // nTimes
    bool        update = true;          // bUpdate
    float      *d_state = nullptr;      // [channels][TAPS]
    f32x2      *d_taps = nullptr;       // TABLE_PAIRS
    float      *d_halo = nullptr;       // [channels][MAX_SPLITS][TAPS] when channels <= SPLIT_ROWS
};

namespace
{
    int tp_clear(mi_truepeak_bank *b, hipStream_t st)
    {
        MI_HIP_CHECK(hipMemsetAsync(b->d_state, 0, size_t(b->channels) * TAPS * sizeof(float), st));
        return MI_OK;
    }

    // TruePeakMeter::update_settings, TruePeakMeter.cpp:149-189: the state is cleared only when N changes
    int tp_update(mi_truepeak_bank *b, hipStream_t st)
    {
        if (!b->update)
            return MI_OK;
        const uint32_t times = oversampling(b->sample_rate);
        if (times != b->times)
        {
            bool cap = false;
            const int r = capturing(st, &cap);
            if (r != MI_OK)
                return r;
            MI_REQUIRE(!cap, MI_ESTATE,
                       "mi_truepeak_bank: a new oversampling factor clears the state; call update_settings() before capturing");
        }
        b->update = false;
        if (times == b->times)
            return MI_OK;
        b->times = times;
        return tp_clear(b, st);
    }

    template <bool MAX>
    int tp_launch(mi_truepeak_bank *b, float *dst, const float *src, uint32_t count, size_t dst_stride, size_t src_stride,
                  float *peaks, hipStream_t st)
    {
        // no halo buffer above SPLIT_ROWS rows: there are workgroups enough, and a row stays whole
        const split_plan plan = (b->d_halo != nullptr) ? plan_splits(count, TILE, b->channels, MAX_SPLITS)
                                                           : split_plan{ 1, count };
        const uint32_t splits = plan.splits, span = plan.span;
        hipEvent_t ev0 = nullptr, ev1 = nullptr;
        mi::take_profile_events(&ev0, &ev1);
        if (splits > 1 && b->times != 0)
        {
            hipLaunchKernelGGL(truepeak_stage_kernel, dim3(b->channels), dim3(BLOCK), 0, st, src, src_stride, count, span, splits,
                               b->d_state, b->d_halo);
            MI_HIP_CHECK(hipGetLastError());
        }
        if (MAX && splits > 1)
            MI_HIP_CHECK(hipMemsetAsync(peaks, 0, size_t(b->channels) * sizeof(float), st));
        const dim3 grid(splits, b->channels);
        #define MI_TP_ARGS dst, src, dst_stride, src_stride, count, span, splits, b->d_state, b->d_halo, b->d_taps, peaks
        switch (b->times)
        {
            case 0: MI_LAUNCH((truepeak_kernel<0, MAX>), grid, dim3(BLOCK), 0, st, ev0, ev1, MI_TP_ARGS); break;
            case 2: MI_LAUNCH((truepeak_kernel<2, MAX>), grid, dim3(BLOCK), 0, st, ev0, ev1, MI_TP_ARGS); break;
            case 3: MI_LAUNCH((truepeak_kernel<3, MAX>), grid, dim3(BLOCK), 0, st, ev0, ev1, MI_TP_ARGS); break;
            case 4: MI_LAUNCH((truepeak_kernel<4, MAX>), grid, dim3(BLOCK), 0, st, ev0, ev1, MI_TP_ARGS); break;
            case 6: MI_LAUNCH((truepeak_kernel<6, MAX>), grid, dim3(BLOCK), 0, st, ev0, ev1, MI_TP_ARGS); break;
            default: MI_LAUNCH((truepeak_kernel<8, MAX>), grid, dim3(BLOCK), 0, st, ev0, ev1, MI_TP_ARGS); break;
        }
        #undef MI_TP_ARGS
        MI_HIP_CHECK(hipGetLastError());
        return MI_OK;
    }
} // namespace

extern "C" {

int mi_truepeak_coefficients(uint32_t times, float *h, size_t *count)
{
    MI_REQUIRE(count != nullptr, MI_EINVAL, "mi_truepeak_coefficients: NULL count");
    MI_REQUIRE(times == 0 || table_offset(int(times)) >= 0, MI_EINVAL, "mi_truepeak_coefficients: no kernel for %u times", times);
    *count = size_t(times) * TAPS;
    if (h != nullptr && times != 0)
        make_table(int(times), A, h);
    return MI_OK;
}

int mi_truepeak_bank_create(mi_truepeak_bank_t **bank, uint32_t channels)            // TruePeakMeter.cpp:37-82
{
    const int r = mi_bank::open(bank, "mi_truepeak_bank_create", channels, 65535u);
    if (r != MI_OK)
        return r;
    mi_truepeak_bank *b = *bank;
    *bank = nullptr;
    b->channels = channels;
    f32x2 table[TABLE_PAIRS];
    for (int n : FACTORS)
        phase_pairs(n, A, table + table_offset(n));
    hipError_t e = hipMalloc(reinterpret_cast<void **>(&b->d_state), size_t(channels) * TAPS * sizeof(float));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&b->d_taps), sizeof(table));
    if (e == hipSuccess && channels <= SPLIT_ROWS)
        e = hipMalloc(reinterpret_cast<void **>(&b->d_halo), size_t(channels) * MAX_SPLITS * TAPS * sizeof(float));
    if (e == hipSuccess) e = hipMemcpy(b->d_taps, table, sizeof(table), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(b->d_state, 0, size_t(channels) * TAPS * sizeof(float));
    if (e != hipSuccess)
    {
        mi_truepeak_bank_destroy(b);
        return mi::fail(MI_EHIP, "mi_truepeak_bank_create: %s", hipGetErrorString(e));
    }
    *bank = b;
    return MI_OK;
}

int mi_truepeak_bank_destroy(mi_truepeak_bank_t *b)                                  // TruePeakMeter.cpp:59-67
{
    if (b == nullptr)
        return MI_OK;
    (void)hipFree(b->d_state); (void)hipFree(b->d_taps); (void)hipFree(b->d_halo);
    delete b;
    return MI_OK;
}

int mi_truepeak_bank_set_sample_rate(mi_truepeak_bank_t *b, uint32_t sample_rate)     // TruePeakMeter.cpp:102-109
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_truepeak_bank_set_sample_rate: NULL bank");
    if (b->sample_rate == sample_rate)
        return MI_OK;
    b->sample_rate = sample_rate;
    b->update = true;
    return MI_OK;
}

int mi_truepeak_bank_update_settings(mi_truepeak_bank_t *b, void *stream)            // TruePeakMeter.cpp:149-189
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_truepeak_bank_update_settings: NULL bank");
    return tp_update(b, mi::as_stream(stream));
}

int mi_truepeak_bank_clear(mi_truepeak_bank_t *b, void *stream)                      // TruePeakMeter.cpp:191-195
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_truepeak_bank_clear: NULL bank");
    return tp_clear(b, mi::as_stream(stream));
}

int mi_truepeak_bank_latency(const mi_truepeak_bank_t *b, uint32_t *samples)        // TruePeakMeter.cpp:274-277
{
    MI_REQUIRE(b != nullptr && samples != nullptr, MI_EINVAL, "mi_truepeak_bank_latency: bad argument");
    *samples = (b->times != 0) ? uint32_t(A) : 0u;
    return MI_OK;
}

int mi_truepeak_bank_oversampling(const mi_truepeak_bank_t *b, uint32_t *times)
{
    MI_REQUIRE(b != nullptr && times != nullptr, MI_EINVAL, "mi_truepeak_bank_oversampling: bad argument");
    *times = b->times;
    return MI_OK;
}

int mi_truepeak_bank_process(mi_truepeak_bank_t *b, float *dst, const float *src, size_t count, size_t dst_stride,
                             size_t src_stride, void *stream)                           // TruePeakMeter.cpp:197-236
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_truepeak_bank_process: NULL bank");
    hipStream_t st = mi::as_stream(stream);
    const int r = tp_update(b, st);
    if (r != MI_OK || count == 0)
        return r;
    const int k = mi_bank::check_rows("mi_truepeak_bank_process", b->channels, count, size_t(1) << 31,
                                      { { dst, dst_stride, count, mi_bank::REQUIRED | mi_bank::OUTPUT },
                                        { src, src_stride, count, mi_bank::REQUIRED } });
    if (k != MI_OK)
        return k;
    return tp_launch<false>(b, dst, src, uint32_t(count), dst_stride, src_stride, nullptr, st);
}

int mi_truepeak_bank_process_max(mi_truepeak_bank_t *b, float *peaks, const float *src, size_t count, size_t src_stride,
                                 void *stream)                                          // TruePeakMeter.cpp:238-272
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_truepeak_bank_process_max: NULL bank");
    hipStream_t st = mi::as_stream(stream);
    const int r = tp_update(b, st);
    if (r != MI_OK)
        return r;
    MI_REQUIRE(peaks != nullptr, MI_EINVAL, "mi_truepeak_bank_process_max: NULL peaks");
    if (count == 0)
    {
        MI_HIP_CHECK(hipMemsetAsync(peaks, 0, size_t(b->channels) * sizeof(float), st));
        return MI_OK;
    }
    const int k = mi_bank::check_rows("mi_truepeak_bank_process_max", b->channels, count, size_t(1) << 31,
                                      { { src, src_stride, count, mi_bank::REQUIRED } });
    if (k != MI_OK)
        return k;
    return tp_launch<true>(b, nullptr, src, uint32_t(count), 0, src_stride, peaks, st);
}

} // extern "C"
