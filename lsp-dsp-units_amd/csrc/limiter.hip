// lsp::dspu::Limiter as a bank of `channels` limiters (src/main/dynamics/Limiter.cpp): process() (:695-784) with one
// workgroup per channel.  The reference keeps its gains in a long buffer that it walks with nHead and moves to the front now
// and then; what it ever READS of that buffer is the window of 4 ML floats at nHead (ML = nMaxLookahead behind gbuf, 3 ML
// ahead), so that window is the state and nHead a counter.  Per chunk of n <= 8192 samples of the call the kernel holds in LDS
//     win[4 ML + n]   win[j] = gbuf[j - ML]: the 4 ML kept gains, and n ones behind them (:707)
//     asc[n]          |sc|
//     tmp[n]          gbuf[i] |sc[i]| (:708), the reference's vTmpBuf
// runs the ALR follower (process_alr, :675-693: the serial envelope on one lane, the gain it gives on all of them), then the
// patch loop (:718-768): the first index of tmp's maximum (per-lane strided maxima, a wave reduction, one exchange through
// LDS), and while that maximum exceeds the threshold the gains around it times 1 - k shape[t] and tmp anew over the patched
// stretch.  shape[] is the host's table (host/limiter.cpp), read through L2: the one part of a chunk that LDS has no room for
// at ML = 3840, and the only one that is read-only.  Then gain[i] = gbuf[i - nLookahead] (:771), and the window moves on by n.
//
// THE PATCH LOOP IS A COUNTED LOOP: at most 2 n patches per chunk.  Every factor 1 - k shape[t] lies in (0, 1], a sample once
// under the threshold stays there, and the reference needs at most n patches on finite input; when the count is reached the
// loop ends with the gains as they are and the channel's overrun flag is set (the reference never returns on NaN).
//
// A patch is cut at the window's ends.  It reaches outside only when the limits of 8 samples on attack and release exceed
// the look-ahead's room (ML < 8); what the reference multiplies there is behind everything it reads, or is overwritten with
// ones before the window reaches it.
//
// Inputs are finite: NaN is out of scope.  The patch, the tmp product and k round every operation on its own; divisions are
// IEEE-rounded.
#include "bank_core.h"
#include "limiter_bank.h"
#include "tile_chain_device.h"

#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#pragma clang fp contract(off)      // every product and every sum below rounds on its own, host and device

namespace
{
    using mi_tile_chain::lds_float;
    using mi_tile_chain::chain_batches;

    constexpr int BLOCK = 512;                      // threads of a channel's workgroup
    constexpr int WAVES = BLOCK / 64;
    constexpr uint32_t CHUNK = 8192;                // BUF_GRANULARITY
    constexpr uint32_t PEAKS_MAX = 32;              // LIMITER_PEAKS_MAX
    constexpr float GAIN_LOWERING = 0.9886f;
    constexpr size_t LDS_LIMIT = 160 * 1024;

    enum { UP_SR = 1, UP_LK = 2, UP_MODE = 4, UP_OTHER = 8, UP_THRESH = 16, UP_ALR = 32, UP_ALL = 63 };   // Limiter.h:60-70
    enum { OP_REFILL = 1, OP_SCALE = 2, OP_ZERO_ENV = 4 };

    // a channel as the device reads it: the computed parameters, the ALR switch, and what update_settings() does to the window
    struct dev_params
    {
        mi_limiter_params_t p;
        uint32_t alr;               // sALR.bEnable
        uint32_t ops;               // OP_*: read by limiter_settings_kernel alone
        float gnorm;                // fReqThreshold / fThreshold of a lowered threshold
    };

    struct limiter_state
    {
        uint32_t head;              // nHead
        float env;                  // sALR.fEnvelope
        uint32_t patches, chunks;   // of the last call
        uint32_t overrun;           // sticky
        uint32_t hist;              // where the next audio sample goes in the history ring
    };

    __device__ __forceinline__ uint32_t min_u32(uint32_t a, uint32_t b) { return (a < b) ? a : b; }

    // floats of a chunk's three LDS arrays for calls of `count` samples: the window, |sc| and tmp, each a multiple of four
    __host__ __device__ inline uint32_t chunk_pad(uint32_t count) { return ((count < CHUNK ? count : CHUNK) + 3u) & ~3u; }

    // the better of two (maximum, index) pairs: the larger value, of equal values the lower index
    __device__ __forceinline__ void better(float &v, uint32_t &i, float ov, uint32_t oi)
    {
        const bool take = ov > v || (ov == v && oi < i);
        v = take ? ov : v;
        i = take ? oi : i;
    }

    // gain (audio == NULL) or dst = delayed audio * gain into `gain`
    __global__ __launch_bounds__(BLOCK) void limiter_kernel(float *gain, const float *audio, const float *sc, size_t gain_stride,
                                                            size_t audio_stride, size_t sc_stride, uint32_t count, uint32_t ml,
                                                            const dev_params *params, limiter_state *state, float *window,
                                                            float *history, const float *shapes, uint32_t shape_cap)
    {
        extern __shared__ __attribute__((aligned(16))) float lds[];
        __shared__ float red_v[WAVES];
        __shared__ uint32_t red_i[WAVES];

        const uint32_t ch = blockIdx.x, tid = threadIdx.x;
        const uint32_t pad = chunk_pad(count);
        float *const win = lds;                             // [4 ml + pad]
        float *const asc = win + 4 * ml + pad;              // [pad]
        float *const tmp = asc + pad;                       // [pad]

        const dev_params *dp = params + ch;
        const float thr = dp->p.threshold;
        const uint32_t la = min_u32(dp->p.lookahead, ml);
        const int32_t middle = dp->p.middle;
        const uint32_t release = (dp->p.release > 0) ? min_u32(uint32_t(dp->p.release), shape_cap) : 0u;
        const bool alr = dp->alr != 0;
        const float *shape = shapes + size_t(ch) * shape_cap;
        float *gwin = window + size_t(ch) * (4 * ml);
        float *hist = history + size_t(ch) * ml;
        const float *xs = sc + size_t(ch) * sc_stride;
        const float *as = (audio != nullptr) ? audio + size_t(ch) * audio_stride : nullptr;
        float *gs = gain + size_t(ch) * gain_stride;

        limiter_state s = state[ch];
        uint32_t patches = 0, chunks = 0;

        for (uint32_t c0 = 0; c0 < count; c0 += CHUNK)
        {
            const uint32_t n = min_u32(count - c0, CHUNK);
            const uint32_t wn = 4 * ml + n;                 // the window of this chunk

            // the kept gains, ones behind them (:707), |sc|
            for (uint32_t j = tid; j < wn; j += BLOCK)
                win[j] = (j < 4 * ml) ? gwin[j] : 1.0f;
            for (uint32_t i = tid; i < n; i += BLOCK)
                asc[i] = fabsf(xs[c0 + i]);
            __syncthreads();
            for (uint32_t i = tid; i < n; i += BLOCK)       // :708
                tmp[i] = win[ml + i] * asc[i];
            __syncthreads();

            if (alr)                                        // :709-713
            {
                if (tid == 0)                               // process_alr's envelope, :679-682, over tmp in place
                {
                    float e = s.env;
                    const float ta = dp->p.tau_attack, tr = dp->p.tau_release;
                    chain_batches((lds_float *)tmp, 0, n, [&](float v)
                    {
                        const float d = v - e;
                        e = e + ((v > e) ? ta : tr) * d;
                        return e;
                    });
                    s.env = e;
                }
                __syncthreads();
                const float ks = dp->p.ks, ke = dp->p.ke, g = dp->p.gain;
                const float h0 = dp->p.hermite[0], h1 = dp->p.hermite[1], h2 = dp->p.hermite[2];
                for (uint32_t i = tid; i < n; i += BLOCK)   // :684-687, then :712
                {
                    const float e = tmp[i];
                    float w = win[ml + i];
                    if (e >= ke)
                        w = w * __fdiv_rn(g, e);
                    else if (e > ks)
                        w = w * (h0 * e + h1 + __fdiv_rn(h2, e));
                    win[ml + i] = w;
                    tmp[i] = w * asc[i];
                }
                __syncthreads();
            }

            // :715-768.  AT MOST 2 n PATCHES: the loop is counted, and whoever reaches the count sets the overrun flag.
            float knee = 1.0f;
            for (uint32_t it = 0; it <= 2 * n; ++it)
            {
                // dsp::max_index: the first index of the maximum
                float v = -1.0f;
                uint32_t at = 0xffffffffu;
                for (uint32_t i = tid; i < n; i += BLOCK)
                {
                    const float t = tmp[i];
                    at = (t > v) ? i : at;
                    v = (t > v) ? t : v;
                }
                #pragma unroll
                for (int m = 32; m >= 1; m >>= 1)
                    better(v, at, __shfl_xor(v, m), __shfl_xor(at, m));
                if ((tid & 63u) == 0)
                    red_v[tid >> 6] = v, red_i[tid >> 6] = at;
                __syncthreads();
                v = red_v[0], at = red_i[0];
                #pragma unroll
                for (int w = 1; w < WAVES; ++w)
                    better(v, at, red_v[w], red_i[w]);

                if (v <= thr)                               // :723: no more peaks
                    break;
                if (it == 2 * n)
                {
                    s.overrun = 1;
                    break;
                }
                const float k = __fdiv_rn(v - (thr * knee - 0.000001f), v);          // :727
                // apply_*_patch to gbuf[peak - nMiddle + t], :609-673, and :763 over the same stretch
                const int32_t first = int32_t(ml) + int32_t(at) - middle;           // the window index of t = 0
                for (uint32_t t = tid; t < release; t += BLOCK)
                {
                    const int32_t j = first + int32_t(t);
                    if (j < 0 || j >= int32_t(wn))
                        continue;
                    const float w = win[j] * (1.0f - k * shape[t]);
                    win[j] = w;
                    const int32_t i = j - int32_t(ml);
                    if (i >= 0 && i < int32_t(n))
                        tmp[i] = w * asc[i];
                }
                ++patches;
                if (((it + 1) % PEAKS_MAX) == 0)            // :766-767
                    knee = knee * GAIN_LOWERING;
                __syncthreads();
            }

            // :771: gain[i] = gbuf[i - nLookahead]; with audio, times the stream's sample of nLookahead ago
            if (as == nullptr)
            {
                for (uint32_t i = tid; i < n; i += BLOCK)
                    gs[c0 + i] = win[ml - la + i];
            }
            else
            {
                for (uint32_t i = tid; i < n; i += BLOCK)   // the chunk's audio over |sc|, which nobody reads any more: dst may be audio
                    asc[i] = as[c0 + i];
                __syncthreads();
                for (uint32_t i = tid; i < n; i += BLOCK)
                {
                    const float a = (i >= la) ? asc[i - la] : hist[(s.hist + ml + i - la) % ml];
                    gs[c0 + i] = a * win[ml - la + i];
                }
                __syncthreads();                            // the history is read; the chunk's last ml samples go into it
                const uint32_t keep = min_u32(n, ml);
                for (uint32_t i = n - keep + tid; i < n; i += BLOCK)
                    hist[(s.hist + i) % ml] = asc[i];
                s.hist = (ml > 0) ? (s.hist + n) % ml : 0;
            }

            // :772-777: the window moves on by n
            for (uint32_t j = tid; j < 4 * ml; j += BLOCK)
                gwin[j] = win[n + j];
            s.head += n;
            if (s.head >= 8 * ml)
                s.head = 0;
            ++chunks;
            __syncthreads();                                // the next chunk reads the window back and fills LDS anew
        }
        if (tid == 0)
        {
            s.patches = patches, s.chunks = chunks;
            state[ch] = s;
        }
    }

    // what update_settings() does to the gain buffer (:402-416) and set_alr(false) to the envelope (:215-216), channels from lo on
    __global__ __launch_bounds__(256) void limiter_settings_kernel(const dev_params *params, limiter_state *state, float *window,
                                                                   uint32_t ml, uint32_t lo)
    {
        const uint32_t ch = lo + blockIdx.x;
        const uint32_t ops = params[ch].ops;
        const float gnorm = params[ch].gnorm;
        float *gwin = window + size_t(ch) * (4 * ml);
        if (ops & (OP_REFILL | OP_SCALE))
            for (uint32_t j = threadIdx.x; j < 4 * ml; j += 256)
            {
                float w = (ops & OP_REFILL) ? 1.0f : gwin[j];       // fill_one over 3 ML + 8192 >= 4 ML floats from nHead
                if ((ops & OP_SCALE) && j < ml)                     // mul_k2 over ML floats from nHead
                    w = w * gnorm;
                gwin[j] = w;
            }
        if ((ops & OP_ZERO_ENV) && threadIdx.x == 0)
            state[ch].env = 0.0f;
    }

    __global__ __launch_bounds__(256) void limiter_clear_kernel(limiter_state *state, float *window, float *history, uint32_t ml)
    {
        const uint32_t ch = blockIdx.x;
        for (uint32_t j = threadIdx.x; j < 4 * ml; j += 256)
            window[size_t(ch) * (4 * ml) + j] = 1.0f;
        for (uint32_t j = threadIdx.x; j < ml; j += 256)
            history[size_t(ch) * ml + j] = 0.0f;
        if (threadIdx.x == 0)
            state[ch] = limiter_state{ 0, 0.0f, 0, 0, 0, 0 };
    }

    // Limiter::construct, :47-73
    mi_limiter_settings_t fresh_settings()
    {
        mi_limiter_settings_t s = {};
        s.threshold = 1.0f;                 // GAIN_AMP_0_DB
        s.knee = float(0.50118);            // GAIN_AMP_M_6_DB
        s.alr_attack = 10.0f;
        s.alr_release = 50.0f;
        s.alr_knee = float(0.56234);        // GAIN_AMP_M_5_DB
        return s;
    }
} // namespace

struct mi_limiter_bank : mi_bank::tables<dev_params, limiter_state>     // params: what update_settings computed; up: of params and shapes
{
    uint32_t                            max_sample_rate = 0;
    float                               max_lookahead = 0.0f;   // fMaxLookahead, ms
    uint32_t                            ml = 0;                 // nMaxLookahead
    uint32_t                            shape_cap = 0;          // floats of a channel's table
    std::vector<mi_limiter_settings_t>  cfg;            // the setters' values; threshold is fReqThreshold
    std::vector<float>                  thr;            // fThreshold
    std::vector<uint32_t>               update;         // nUpdate
    std::vector<float>                  shapes;         // [channels][shape_cap]
    float                              *d_window = nullptr;     // [channels][4 ml]
    float                              *d_history = nullptr;    // [channels][ml]
    float                              *d_shapes = nullptr;     // [channels][shape_cap]
};

namespace
{
    // update_settings of every channel with nUpdate set; the changed stretch of the tables goes to the device, and what the
    // changes do to the gain windows follows on the stream
    int limiter_update(mi_limiter_bank *b, hipStream_t st)
    {
        for (uint32_t ch = 0; ch < b->channels; ++ch)
        {
            if (b->update[ch] == 0)
                continue;
            dev_params &d = b->params[ch];
            if (b->update[ch] & UP_SR)                                              // :403-404
                d.ops |= OP_REFILL;
            if (b->update[ch] & UP_THRESH)                                          // :409-419
            {
                if (b->cfg[ch].threshold < b->thr[ch])
                {
                    d.gnorm = b->cfg[ch].threshold / b->thr[ch];
                    d.ops |= OP_SCALE;
                }
                b->thr[ch] = b->cfg[ch].threshold;
            }
            mi_limiter_settings_t s = b->cfg[ch];
            s.threshold = b->thr[ch];
            mi_limiter_params_t p;
            mi::limiter_compute_params(s, p);
            MI_REQUIRE(p.release >= 0 && uint32_t(p.release) <= b->shape_cap && p.lookahead <= b->ml, MI_EINVAL,
                       "mi_limiter_bank: channel %u: a look-ahead of %u samples exceeds the bank's %u", ch, p.lookahead, b->ml);
            d.p = p;
            mi::limiter_compute_patch(p, b->shapes.data() + size_t(ch) * b->shape_cap);
            b->update[ch] = 0;
            b->up.touch(ch);
        }
        if (!b->up.any())
            return MI_OK;
        const int r = mi::refuse_capture("mi_limiter_bank", st);
        if (r != MI_OK)
            return r;
        const uint32_t lo = b->up.lo, n = b->up.hi - b->up.lo;
        MI_HIP_CHECK(hipMemcpyAsync(b->d_params + lo, b->params.data() + lo, size_t(n) * sizeof(dev_params), hipMemcpyHostToDevice, st));
        MI_HIP_CHECK(hipMemcpyAsync(b->d_shapes + size_t(lo) * b->shape_cap, b->shapes.data() + size_t(lo) * b->shape_cap,
                                    size_t(n) * b->shape_cap * sizeof(float), hipMemcpyHostToDevice, st));
        MI_HIP_CHECK(hipStreamSynchronize(st));                 // the host tables may change again after this returns
        bool ops = false;
        for (uint32_t ch = lo; ch < lo + n; ++ch)
        {
            ops = ops || b->params[ch].ops != 0;
            b->params[ch].ops = 0;
        }
        b->up = mi::dirty_range();
        if (ops)
        {
            hipLaunchKernelGGL(limiter_settings_kernel, dim3(n), dim3(256), 0, st, b->d_params, b->d_state, b->d_window, b->ml, lo);
            MI_HIP_CHECK(hipGetLastError());
        }
        return MI_OK;
    }

    int limiter_launch(mi_limiter_bank *b, float *gain, const float *audio, const float *sc, size_t count, size_t gain_stride,
                       size_t audio_stride, size_t sc_stride, hipStream_t st)
    {
        const size_t lds = (size_t(4) * b->ml + size_t(3) * chunk_pad(uint32_t(count))) * sizeof(float);
        hipEvent_t ev0 = nullptr, ev1 = nullptr;
        mi::take_profile_events(&ev0, &ev1);
        MI_LAUNCH(limiter_kernel, dim3(b->channels), dim3(BLOCK), lds, st, ev0, ev1, gain, audio, sc, gain_stride, audio_stride,
                  sc_stride, uint32_t(count), b->ml, b->d_params, b->d_state, b->d_window, b->d_history, b->d_shapes, b->shape_cap);
        MI_HIP_CHECK(hipGetLastError());
        return MI_OK;
    }

    constexpr size_t COUNT_LIMIT = size_t(1) << 30;     // of the samples of one call

    // what create() does to the new, empty bank
    int limiter_init(mi_limiter_bank *b, uint32_t channels, uint32_t max_sample_rate, float max_lookahead_ms, float mlf)
    {
        static_assert((size_t(4) * MI_LIMITER_MAX_LOOKAHEAD + size_t(3) * CHUNK) * sizeof(float) + 256 <= LDS_LIMIT, "the chunk's LDS");
        b->channels = channels;
        b->max_sample_rate = max_sample_rate;
        b->max_lookahead = max_lookahead_ms;
        b->ml = uint32_t(mlf);
        b->shape_cap = mi::limiter_patch_capacity(b->ml);
        b->cfg.assign(channels, fresh_settings());
        b->thr.assign(channels, 1.0f);
        b->update.assign(channels, UP_ALL);
        b->shapes.assign(size_t(channels) * b->shape_cap, 0.0f);
        const int r = mi_bank::alloc(*b, "mi_limiter_bank_create", dev_params{}, limiter_state{});
        if (r != MI_OK)
            return r;
        const size_t wbytes = size_t(channels) * (4 * b->ml) * sizeof(float), hbytes = size_t(channels) * b->ml * sizeof(float);
        hipError_t e = hipMalloc(reinterpret_cast<void **>(&b->d_window), wbytes + 16);
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&b->d_history), hbytes + 16);
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&b->d_shapes), b->shapes.size() * sizeof(float));
        if (e == hipSuccess) e = hipMemset(b->d_shapes, 0, b->shapes.size() * sizeof(float));
        // a chunk of 8192 samples at the largest ML takes all of a workgroup's LDS
        if (e == hipSuccess) e = hipFuncSetAttribute(reinterpret_cast<const void *>(limiter_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                     int(LDS_LIMIT - 256));
        if (e == hipSuccess)
        {
            hipLaunchKernelGGL(limiter_clear_kernel, dim3(channels), dim3(256), 0, nullptr, b->d_state, b->d_window, b->d_history, b->ml);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
        MI_REQUIRE(e == hipSuccess, MI_EHIP, "mi_limiter_bank_create: %s", hipGetErrorString(e));
        return MI_OK;
    }
} // namespace

extern "C" {

int mi_limiter_bank_create(mi_limiter_bank_t **bank, uint32_t channels, uint32_t max_sample_rate, float max_lookahead_ms)   // :47-109
{
    int r = mi_bank::open_checks(bank, "mi_limiter_bank_create", channels);
    if (r != MI_OK)
        return r;
    MI_REQUIRE(max_lookahead_ms >= 0.0f && max_lookahead_ms <= 1e6f, MI_EINVAL, "mi_limiter_bank_create: bad maximum look-ahead");
    const float mlf = (max_lookahead_ms * 0.001f) * float(max_sample_rate);         // millis_to_samples, :89
    MI_REQUIRE(mlf < float(MI_LIMITER_MAX_LOOKAHEAD + 1), MI_EINVAL,
               "mi_limiter_bank_create: a maximum look-ahead of %.0f samples exceeds MI_LIMITER_MAX_LOOKAHEAD = %d", double(mlf),
               MI_LIMITER_MAX_LOOKAHEAD);
    r = mi_bank::open_new(bank, "mi_limiter_bank_create");
    if (r != MI_OK)
        return r;
    r = limiter_init(*bank, channels, max_sample_rate, max_lookahead_ms, mlf);
    if (r != MI_OK)
    {
        mi_limiter_bank_destroy(*bank);
        *bank = nullptr;
    }
    return r;
}

int mi_limiter_bank_destroy(mi_limiter_bank_t *b)
{
    if (b == nullptr)
        return MI_OK;
    (void)hipFree(b->d_window); (void)hipFree(b->d_history); (void)hipFree(b->d_shapes);
    return mi_bank::destroy(b);
}

int mi_limiter_bank_set_sample_rate(mi_limiter_bank_t *b, uint32_t channel, uint32_t sample_rate)          // :154-162
{
    MI_BANK_SETTER("limiter", "set_sample_rate");
    MI_REQUIRE(sample_rate <= b->max_sample_rate, MI_EINVAL, "mi_limiter_bank_set_sample_rate: %u exceeds the bank's maximum %u",
               sample_rate, b->max_sample_rate);
    if (c.sample_rate == sample_rate)
        return MI_OK;
    c.sample_rate = sample_rate;
    b->update[channel] |= UP_SR | UP_ALR | UP_MODE;
    return MI_OK;
}

int mi_limiter_bank_set_mode(mi_limiter_bank_t *b, uint32_t channel, uint32_t mode)                        // :146-152
{
    MI_BANK_SETTER("limiter", "set_mode");
    MI_REQUIRE(mode < MI_LIMITER_MODES, MI_EINVAL, "mi_limiter_bank_set_mode: mode %u out of range", mode);
    if (c.mode == mode)
        return MI_OK;
    c.mode = mode;
    b->update[channel] |= UP_MODE;
    return MI_OK;
}

int mi_limiter_bank_set_threshold(mi_limiter_bank_t *b, uint32_t channel, float threshold, int immediate)  // :133-144
{
    MI_BANK_SETTER("limiter", "set_threshold");
    if (c.threshold == threshold)
        return MI_OK;
    c.threshold = threshold;
    if (immediate)
        b->thr[channel] = threshold;
    b->update[channel] |= UP_THRESH | UP_ALR;
    return MI_OK;
}

int mi_limiter_bank_set_attack(mi_limiter_bank_t *b, uint32_t channel, float attack)                       // :111-120
{
    MI_BANK_SETTER("limiter", "set_attack");
    if (c.attack == attack)
        return MI_OK;
    c.attack = attack;
    b->update[channel] |= UP_OTHER;
    return MI_OK;
}

int mi_limiter_bank_set_release(mi_limiter_bank_t *b, uint32_t channel, float release)                     // :122-131
{
    MI_BANK_SETTER("limiter", "set_release");
    if (c.release == release)
        return MI_OK;
    c.release = release;
    b->update[channel] |= UP_OTHER;
    return MI_OK;
}

int mi_limiter_bank_set_lookahead(mi_limiter_bank_t *b, uint32_t channel, float lookahead)                 // :164-176
{
    MI_BANK_SETTER("limiter", "set_lookahead");
    lookahead = (lookahead < b->max_lookahead) ? lookahead : b->max_lookahead;      // lsp_min
    if (c.lookahead == lookahead)
        return MI_OK;
    c.lookahead = lookahead;
    b->update[channel] |= UP_LK;
    return MI_OK;
}

int mi_limiter_bank_set_knee(mi_limiter_bank_t *b, uint32_t channel, float knee)                           // :178-187
{
    MI_BANK_SETTER("limiter", "set_knee");
    if (c.knee == knee)
        return MI_OK;
    c.knee = knee;
    b->update[channel] |= UP_ALR;
    return MI_OK;
}

int mi_limiter_bank_set_alr(mi_limiter_bank_t *b, uint32_t channel, int enable)                            // :211-218
{
    MI_BANK_SETTER("limiter", "set_alr");
    (void)c;
    dev_params &d = b->params[channel];
    d.alr = (enable != 0) ? 1 : 0;
    if (!enable)
        d.ops |= OP_ZERO_ENV;
    b->up.touch(channel);
    return MI_OK;
}

int mi_limiter_bank_set_alr_attack(mi_limiter_bank_t *b, uint32_t channel, float attack)                   // :189-198
{
    MI_BANK_SETTER("limiter", "set_alr_attack");
    if (c.alr_attack == attack)
        return MI_OK;
    c.alr_attack = attack;
    b->update[channel] |= UP_ALR;
    return MI_OK;
}

int mi_limiter_bank_set_alr_release(mi_limiter_bank_t *b, uint32_t channel, float release)                 // :200-209
{
    MI_BANK_SETTER("limiter", "set_alr_release");
    if (c.alr_release == release)
        return MI_OK;
    c.alr_release = release;
    b->update[channel] |= UP_ALR;
    return MI_OK;
}

int mi_limiter_bank_set_alr_knee(mi_limiter_bank_t *b, uint32_t channel, float knee)                       // :220-229
{
    MI_BANK_SETTER("limiter", "set_alr_knee");
    if (c.alr_knee == knee)
        return MI_OK;
    c.alr_knee = (knee > 1.0f) ? 1.0f / knee : knee;
    b->update[channel] |= UP_ALR;
    return MI_OK;
}

int mi_limiter_bank_update_settings(mi_limiter_bank_t *b, void *stream)                                     // :396-548
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_limiter_bank_update_settings: NULL bank");
    return limiter_update(b, mi::as_stream(stream));
}

int mi_limiter_bank_clear(mi_limiter_bank_t *b, void *stream)
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_limiter_bank_clear: NULL bank");
    hipLaunchKernelGGL(limiter_clear_kernel, dim3(b->channels), dim3(256), 0, mi::as_stream(stream), b->d_state, b->d_window,
                       b->d_history, b->ml);
    MI_HIP_CHECK(hipGetLastError());
    return MI_OK;
}

int mi_limiter_bank_get_params(const mi_limiter_bank_t *b, uint32_t channel, mi_limiter_params_t *params)
{
    const int r = mi_bank::get_checks(b, "mi_limiter_bank_get_params", channel, params);
    if (r == MI_OK)
        *params = b->params[channel].p;
    return r;
}

int mi_limiter_bank_get_patch(mi_limiter_bank_t *b, uint32_t channel, float *shape, size_t capacity, uint32_t *count, void *stream)
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_limiter_bank_get_patch: NULL bank");
    MI_REQUIRE(channel < b->channels && count != nullptr, MI_EINVAL, "mi_limiter_bank_get_patch: bad argument");
    hipStream_t st = mi::as_stream(stream);
    const int r = mi::refuse_state_access(st);
    if (r != MI_OK)
        return r;
    const uint32_t n = uint32_t(b->params[channel].p.release);
    *count = n;
    MI_REQUIRE(n <= capacity && (shape != nullptr || n == 0), MI_EINVAL, "mi_limiter_bank_get_patch: %u entries do not fit into %zu",
               n, capacity);
    if (n > 0)
        MI_HIP_CHECK(hipMemcpyAsync(shape, b->d_shapes + size_t(channel) * b->shape_cap, size_t(n) * sizeof(float),
                                    hipMemcpyDeviceToHost, st));
    MI_HIP_CHECK(hipStreamSynchronize(st));
    return MI_OK;
}

int mi_limiter_bank_get_latency(mi_limiter_bank_t *b, uint32_t channel, uint32_t *latency)                  // Limiter.h:314
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_limiter_bank_get_latency: NULL bank");
    MI_REQUIRE(channel < b->channels && latency != nullptr, MI_EINVAL, "mi_limiter_bank_get_latency: bad argument");
    const mi_limiter_settings_t &c = b->cfg[channel];
    *latency = uint32_t((c.lookahead * 0.001f) * float(c.sample_rate));             // :160, :173
    return MI_OK;
}

int mi_limiter_bank_get_state(mi_limiter_bank_t *b, uint32_t channel, uint32_t *head, float *envelope, uint32_t *patches,
                              uint32_t *chunks, uint32_t *overrun, void *stream)
{
    limiter_state s;
    const int r = mi_bank::get_state(b, "mi_limiter_bank_get_state", channel, &s, stream);
    if (r != MI_OK)
        return r;
    if (head != nullptr) *head = s.head;
    if (envelope != nullptr) *envelope = s.env;
    if (patches != nullptr) *patches = s.patches;
    if (chunks != nullptr) *chunks = s.chunks;
    if (overrun != nullptr) *overrun = s.overrun;
    return MI_OK;
}

int mi_limiter_bank_process(mi_limiter_bank_t *b, float *gain, const float *sc, size_t count, size_t gain_stride, size_t sc_stride,
                            void *stream)                                                                   // :695-784
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_limiter_bank_process: NULL bank");
    hipStream_t st = mi::as_stream(stream);
    const int r = limiter_update(b, st);
    if (r != MI_OK || count == 0)
        return r;
    const int k = mi_bank::check_rows("mi_limiter_bank_process", b->channels, count, COUNT_LIMIT,
                                      { { gain, gain_stride, count, mi_bank::REQUIRED | mi_bank::OUTPUT },
                                        { sc, sc_stride, count, mi_bank::REQUIRED } });
    if (k != MI_OK)
        return k;
    return limiter_launch(b, gain, nullptr, sc, count, gain_stride, 0, sc_stride, st);
}

int mi_limiter_bank_process_apply(mi_limiter_bank_t *b, float *dst, const float *audio, const float *sc, size_t count,
                                  size_t dst_stride, size_t audio_stride, size_t sc_stride, void *stream)
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_limiter_bank_process_apply: NULL bank");
    hipStream_t st = mi::as_stream(stream);
    const int r = limiter_update(b, st);
    if (r != MI_OK || count == 0)
        return r;
    const int k = mi_bank::check_rows("mi_limiter_bank_process_apply", b->channels, count, COUNT_LIMIT,
                                      { { dst, dst_stride, count, mi_bank::REQUIRED | mi_bank::OUTPUT },
                                        { audio, audio_stride, count, mi_bank::REQUIRED }, { sc, sc_stride, count, mi_bank::REQUIRED } });
    if (k != MI_OK)
        return k;
    return limiter_launch(b, dst, audio, sc, count, dst_stride, audio_stride, sc_stride, st);
}

} // extern "C"
