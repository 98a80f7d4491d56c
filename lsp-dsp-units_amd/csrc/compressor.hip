// lsp::dspu::Compressor as a bank of `channels` compressors (src/main/dynamics/Compressor.cpp): the envelope follower of
// process() (:226-259) and the two-knee gain curve of dsp::compressor_x2_gain, which the scalar overload (:297-310) states
// in full.
//
// The follower is a serial recurrence over (fEnvelope, fPeak, nHoldCounter) whose branch depends on the running value: one
// lane per channel, the state in registers for the whole call and in a device array between calls (no host positions, so
// calls can be captured into a graph and replayed).  The gain curve is element-wise.  compressor_kernel runs both in one
// launch: a workgroup owns GROUP channels and walks their rows in tiles of TILE samples through LDS, two buffers:
//     wave 0           the follower over tile k, lane c on row c, the envelope written over the input in LDS
//     waves 1 .. GROUP one row each: the gain of tile k - 1 from its envelope and the stores (16 bytes per lane where the
//                      rows allow it), then the load of tile k + 1 into the buffer just emptied
// one barrier per tile.  A tile is in LDS before anything of it is stored and tile k + 1 is loaded after tile k - 1 was
// stored, so gain, env and dst may each be the input row.  The follower's tau * d and e + ... round once each (no fused
// multiply-add): compressor_follow_tile is a function of its own so that its instructions can be looked at
// (tests/test_compressor_host.py), and the envelope matches tests/compressor_ref.py bit for bit.
//
// Inputs are finite: NaN is out of scope.  Subnormal envelopes are kept (the float32 denormal mode is on).
#include "compressor_bank.h"

#include <cmath>
#include <new>
#include <vector>

#pragma clang fp contract(off)      // every product and every sum below rounds on its own, host and device

namespace
{
    constexpr int GROUP   = 4;                  // channels of a workgroup: 1024 channels are 256 workgroups, one per CU
    constexpr int TILE    = 256;                // samples of a row per trip through LDS
    constexpr int ROW     = TILE + 4;           // floats between rows in LDS: lane c's 16-byte reads start at bank 4c
    constexpr int HELPERS = GROUP * 64;         // one wave per row for loads, gain and stores
    constexpr int BLOCK   = 64 + HELPERS;
    constexpr int BATCH   = 8;                  // samples the follower reads ahead of its chain
    constexpr int CURVE_BLOCK = 256;

    enum { VEC_IN = 1, VEC_GAIN = 2, VEC_ENV = 4, VEC_AUDIO = 8 };

    typedef float f32x4 __attribute__((ext_vector_type(4)));
    typedef __attribute__((address_space(3))) float lds_float;
    typedef __attribute__((address_space(3))) f32x4 lds_f32x4;

    struct follow_state { float e, peak; uint32_t hold; };
    struct device_state { float e, peak; uint32_t hold, pad; };     // [channels] between calls

    // Compressor.cpp:231-256 over samples [0, n) of one row in LDS, in place: row[i] becomes the envelope
    __device__ __forceinline__ void follow_step(float s, float &e, float &peak, uint32_t &hold, float ta, float tr, float rt,
                                                uint32_t nhold)
    {
        const float d = s - e;
        const bool neg = d < 0.0f;
        const float tau = (neg && e > rt) ? tr : ta;
        const float en = e + tau * d;
        const bool held = neg && hold > 0;
        const bool rearm = !neg && en >= peak;
        e = held ? e : en;
        peak = ((neg && !held) || rearm) ? en : peak;
        hold = held ? hold - 1 : rearm ? nhold : hold;
    }

    __device__ __noinline__ follow_state compressor_follow_tile(lds_float *row, uint32_t n, follow_state s, float ta, float tr,
                                                                float rt, uint32_t nhold)
    {
        float e = s.e, peak = s.peak;
        uint32_t hold = s.hold, i = 0;
        if (n >= BATCH)
        {
            f32x4 a = *reinterpret_cast<lds_f32x4 *>(row), b = *reinterpret_cast<lds_f32x4 *>(row + 4);
            for (; i + BATCH <= n; i += BATCH)
            {
                float v[BATCH] = { a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w };
                const uint32_t next = (i + 2 * BATCH <= n) ? i + BATCH : i;    // the next batch, before this one's chain
                a = *reinterpret_cast<lds_f32x4 *>(row + next);
                b = *reinterpret_cast<lds_f32x4 *>(row + next + 4);
                #pragma unroll
                for (int j = 0; j < BATCH; ++j)
                {
                    follow_step(v[j], e, peak, hold, ta, tr, rt, nhold);
                    v[j] = e;
                }
                *reinterpret_cast<lds_f32x4 *>(row + i) = f32x4{ v[0], v[1], v[2], v[3] };
                *reinterpret_cast<lds_f32x4 *>(row + i + 4) = f32x4{ v[4], v[5], v[6], v[7] };
            }
        }
        for (; i < n; ++i)
        {
            follow_step(row[i], e, peak, hold, ta, tr, rt, nhold);
            row[i] = e;
        }
        return follow_state{ e, peak, hold };
    }

    // one knee of Compressor.cpp:302-307
    __device__ __forceinline__ float knee_gain(float x, float lx, const mi_compressor_knee_t &k)
    {
        const float arg = (x >= k.end) ? lx * k.tilt[0] + k.tilt[1] : (k.herm[0] * lx + k.herm[1]) * lx + k.herm[2];
        return (x <= k.start) ? k.gain : expf(arg);
    }

    // Compressor.cpp:297-309: the gain for the envelope e
    __device__ __forceinline__ float x2_gain(float e, const mi_compressor_knee_t &k0, const mi_compressor_knee_t &k1)
    {
        const float x = fabsf(e);
        if (x <= k0.start && x <= k1.start)
            return k0.gain * k1.gain;
        const float lx = logf(x);
        return knee_gain(x, lx, k0) * knee_gain(x, lx, k1);
    }

    // gain (audio == NULL) or dst = audio * gain into `gain`, the envelope into `env` unless NULL.  vec: which of the buffers
    // have 16-byte aligned rows.
    __global__ __launch_bounds__(BLOCK) void compressor_kernel(float *gain, float *env, const float *in, const float *audio,
                                                               size_t gain_stride, size_t env_stride, size_t in_stride,
                                                               size_t audio_stride, uint32_t count, uint32_t channels,
                                                               const mi_compressor_params_t *params, device_state *state,
                                                               uint32_t vec)
    {
        __shared__ __attribute__((aligned(16))) float tile[2][GROUP][ROW];
        const int tid = threadIdx.x, lane = tid & 63;
        const bool follower = tid < 64;
        const uint32_t ch0 = blockIdx.x * GROUP;
        const uint32_t tiles = (count + TILE - 1) / TILE;

        // the follower's lane: its channel's state and taus; a helper: its row (one per wave) and its four samples of a tile
        const uint32_t r = follower ? uint32_t(lane) : uint32_t(__builtin_amdgcn_readfirstlane((tid >> 6) - 1));
        const uint32_t ch = ch0 + r;
        const bool valid = r < uint32_t(GROUP) && ch < channels;
        const uint32_t c = uint32_t(lane) * 4;
        follow_state fs = { 0.0f, 0.0f, 0 };
        float ta = 0.0f, tr = 0.0f, rt = 0.0f;
        uint32_t nhold = 0;
        mi_compressor_knee_t k0 = {}, k1 = {};
        if (valid && follower)
        {
            const device_state s = state[ch];
            fs = follow_state{ s.e, s.peak, s.hold };
            ta = params[ch].tau_attack, tr = params[ch].tau_release, rt = params[ch].release_threshold, nhold = params[ch].hold;
        }
        else if (valid)
            k0 = params[ch].k[0], k1 = params[ch].k[1];
        const float *xs = in + size_t(ch) * in_stride;
        const float *as = (audio != nullptr) ? audio + size_t(ch) * audio_stride : nullptr;
        float *gs = gain + size_t(ch) * gain_stride;
        float *es = (env != nullptr) ? env + size_t(ch) * env_stride : nullptr;

        auto load_tile = [&](uint32_t k)
        {
            const uint32_t t0 = k * TILE, n = (count - t0 < uint32_t(TILE)) ? count - t0 : uint32_t(TILE);
            float *l = &tile[k & 1][r][c];
            if ((vec & VEC_IN) && c + 4 <= n)
                *reinterpret_cast<float4 *>(l) = *reinterpret_cast<const float4 *>(xs + t0 + c);
            else
            {
                #pragma unroll
                for (uint32_t j = 0; j < 4; ++j)
                    if (c + j < n)
                        l[j] = xs[t0 + c + j];
            }
        };
        auto emit_tile = [&](uint32_t k)
        {
            const uint32_t t0 = k * TILE, n = (count - t0 < uint32_t(TILE)) ? count - t0 : uint32_t(TILE);
            if (c >= n)
                return;
            const float4 e4 = *reinterpret_cast<const float4 *>(&tile[k & 1][r][c]);
            const float e[4] = { e4.x, e4.y, e4.z, e4.w };
            const bool whole = c + 4 <= n;
            float g[4];
            #pragma unroll
            for (uint32_t j = 0; j < 4; ++j)
                g[j] = (c + j < n) ? x2_gain(e[j], k0, k1) : 0.0f;
            if (as != nullptr)
            {
                float a[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
                if ((vec & VEC_AUDIO) && whole)
                {
                    const float4 a4 = *reinterpret_cast<const float4 *>(as + t0 + c);
                    a[0] = a4.x, a[1] = a4.y, a[2] = a4.z, a[3] = a4.w;
                }
                else
                {
                    #pragma unroll
                    for (uint32_t j = 0; j < 4; ++j)
                        if (c + j < n)
                            a[j] = as[t0 + c + j];
                }
                #pragma unroll
                for (uint32_t j = 0; j < 4; ++j)
                    g[j] = a[j] * g[j];
            }
            if ((vec & VEC_GAIN) && whole)
                *reinterpret_cast<float4 *>(gs + t0 + c) = make_float4(g[0], g[1], g[2], g[3]);
            else
            {
                #pragma unroll
                for (uint32_t j = 0; j < 4; ++j)
                    if (c + j < n)
                        gs[t0 + c + j] = g[j];
            }
            if (es == nullptr)
                return;
            if ((vec & VEC_ENV) && whole)
                *reinterpret_cast<float4 *>(es + t0 + c) = e4;
            else
            {
                #pragma unroll
                for (uint32_t j = 0; j < 4; ++j)
                    if (c + j < n)
                        es[t0 + c + j] = e[j];
            }
        };

        if (valid && !follower)
            load_tile(0);
        __syncthreads();
        for (uint32_t k = 0; k < tiles; ++k)
        {
            if (follower)
            {
                if (valid)
                {
                    const uint32_t t0 = k * TILE, n = (count - t0 < uint32_t(TILE)) ? count - t0 : uint32_t(TILE);
                    fs = compressor_follow_tile((lds_float *)&tile[k & 1][r][0], n, fs, ta, tr, rt, nhold);
                }
            }
            else if (valid)
            {
                if (k > 0)
                    emit_tile(k - 1);
                if (k + 1 < tiles)
                    load_tile(k + 1);
            }
            __syncthreads();
        }
        if (valid && !follower)
            emit_tile(tiles - 1);
        if (valid && follower)
            state[ch] = device_state{ fs.e, fs.peak, fs.hold, 0 };
    }

    // Compressor::curve(float), Compressor.cpp:318-334, over rows: out = gain(|in|) * |in|
    __global__ __launch_bounds__(CURVE_BLOCK) void compressor_curve_kernel(float *out, const float *in, size_t out_stride,
                                                                           size_t in_stride, uint32_t dots,
                                                                           const mi_compressor_params_t *params)
    {
        const uint32_t ch = blockIdx.y, i = blockIdx.x * CURVE_BLOCK + threadIdx.x;
        if (i >= dots)
            return;
        const mi_compressor_knee_t k0 = params[ch].k[0], k1 = params[ch].k[1];
        const float x = fabsf(in[size_t(ch) * in_stride + i]);
        out[size_t(ch) * out_stride + i] = x2_gain(x, k0, k1) * x;
    }

    // interpolation::hermite_quadratic, src/main/misc/interpolation.cpp:103-109
    void hermite_quadratic(float *p, float x0, float y0, float k0, float x1, float k1)
    {
        p[0] = (k0 - k1) * 0.5f / (x0 - x1);
        p[1] = k0 - 2.0f * p[0] * x0;
        p[2] = y0 - (p[0] * x0 + p[1]) * x0;
    }

    inline float millis_to_samples(float sr, float time) { return (time * 0.001f) * sr; }       // units.h:116-119

    void knee(mi_compressor_knee_t &k, float start, float end, float gain, float tilt0, float tilt1)
    {
        k.start = start, k.end = end, k.gain = gain, k.tilt[0] = tilt0, k.tilt[1] = tilt1;
    }

    // Compressor::update_settings, Compressor.cpp:89-220, in host float32
    void compute_params(const mi_compressor_settings_t &s, mi_compressor_params_t &p)
    {
        const float sr = float(s.sample_rate);
        const float k707 = logf(float(1.0 - M_SQRT1_2));
        p.tau_attack = 1.0f - expf(k707 / millis_to_samples(sr, s.attack));
        p.tau_release = 1.0f - expf(k707 / millis_to_samples(sr, s.release));
        p.release_threshold = s.release_threshold;
        p.hold = uint32_t(millis_to_samples(sr, s.hold));
        mi_compressor_knee_t &k0 = p.k[0], &k1 = p.k[1];
        for (mi_compressor_knee_t *k : { &k0, &k1 })
            k->herm[0] = k->herm[1] = k->herm[2] = 0.0f;
        const float at = s.attack_threshold, bt = s.boost_threshold, kn = s.knee;
        switch (s.mode)
        {
            case MI_CM_UPWARD:
            {
                const float rr = 1.0f / s.ratio, th1 = logf(at), th2 = logf(bt), b = (rr - 1.0f) * (th2 - th1);
                knee(k0, at * kn, at / kn, 1.0f, 1.0f - rr, (rr - 1.0f) * th1);
                knee(k1, bt * kn, bt / kn, expf(b), rr - 1.0f, (1.0f - rr) * th1);
                hermite_quadratic(k0.herm, logf(k0.start), 0.0f, 0.0f, logf(k0.end), k0.tilt[0]);
                hermite_quadratic(k1.herm, logf(k1.start), b, 0.0f, logf(k1.end), k1.tilt[0]);
                break;
            }
            case MI_CM_BOOSTING:
            {
                const float rr = 1.0f / ((s.ratio > 1.0f + 1e-5f) ? s.ratio : 1.0f + 1e-5f);
                const float b = logf(bt), th1 = logf(at), th2 = th1 + b / (rr - 1.0f), eth2 = expf(th2);
                if (bt >= 1.0f)
                {
                    knee(k0, at * kn, at / kn, 1.0f, 1.0f - rr, (rr - 1.0f) * th1);
                    knee(k1, eth2 * kn, eth2 / kn, bt, rr - 1.0f, (1.0f - rr) * th1);
                    hermite_quadratic(k0.herm, logf(k0.start), 0.0f, 0.0f, logf(k0.end), k0.tilt[0]);
                    hermite_quadratic(k1.herm, logf(k1.start), b, 0.0f, logf(k1.end), k1.tilt[0]);
                }
                else
                {
                    knee(k0, at * kn, at / kn, 1.0f, rr - 1.0f, (1.0f - rr) * th1);
                    knee(k1, eth2 * kn, eth2 / kn, 1.0f, 1.0f - rr, (rr - 1.0f) * th2);
                    hermite_quadratic(k0.herm, logf(k0.start), 0.0f, 0.0f, logf(k0.end), k0.tilt[0]);
                    hermite_quadratic(k1.herm, logf(k1.start), 0.0f, 0.0f, logf(k1.end), k1.tilt[0]);
                }
                break;
            }
            case MI_CM_DOWNWARD:
            default:
            {
                const float rr = 1.0f / s.ratio, th1 = logf(at);
                knee(k0, at * kn, at / kn, 1.0f, rr - 1.0f, (1.0f - rr) * th1);
                knee(k1, 1e+10f, 1e+10f, 1.0f, 0.0f, 0.0f);                     // FLOAT_SAT_P_INF
                hermite_quadratic(k0.herm, logf(k0.start), 0.0f, 0.0f, logf(k0.end), k0.tilt[0]);
                break;
            }
        }
    }

    // Compressor::construct, Compressor.cpp:46-83
    mi_compressor_settings_t fresh_settings()
    {
        mi_compressor_settings_t s = {};
        s.mode = MI_CM_DOWNWARD;
        s.boost_threshold = float(2.5119e-4);                                   // GAIN_AMP_M_72_DB
        s.ratio = 1.0f;
        return s;
    }

    mi_compressor_params_t fresh_params()
    {
        mi_compressor_params_t p = {};
        p.k[0].gain = p.k[1].gain = 1.0f;
        return p;
    }

    bool aligned16(const void *p, size_t stride, uint32_t channels)
    {
        return p != nullptr && (reinterpret_cast<uintptr_t>(p) & 15u) == 0 && (channels == 1 || (stride & 3u) == 0);
    }

    int capturing(hipStream_t st, bool *yes)
    {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (st != nullptr)
            MI_HIP_CHECK(hipStreamIsCapturing(st, &cs));
        *yes = cs != hipStreamCaptureStatusNone;
        return MI_OK;
    }
} // namespace

struct mi_compressor_bank
{
    uint32_t                                channels = 0;
    std::vector<mi_compressor_settings_t>   cfg;            // the setters' values
    std::vector<uint8_t>                    update;         // bUpdate of every channel
    std::vector<mi_compressor_params_t>     params;         // what update_settings computed
    uint32_t                                up_lo = 0, up_hi = 0;   // channels [up_lo, up_hi) differ from the device table
    mi_compressor_params_t                 *d_params = nullptr;     // [channels]
    device_state                           *d_state = nullptr;      // [channels]
};

namespace
{
    void touch(mi_compressor_bank *b, uint32_t ch)
    {
        if (b->up_lo == b->up_hi)
            b->up_lo = ch, b->up_hi = ch + 1;
        else
            b->up_lo = (ch < b->up_lo) ? ch : b->up_lo, b->up_hi = (ch + 1 > b->up_hi) ? ch + 1 : b->up_hi;
    }

    // update_settings of every channel whose bUpdate is set; the changed stretch of the table goes to the device
    int comp_update(mi_compressor_bank *b, hipStream_t st)
    {
        for (uint32_t ch = 0; ch < b->channels; ++ch)
        {
            if (!b->update[ch])
                continue;
            compute_params(b->cfg[ch], b->params[ch]);
            b->update[ch] = 0;
            touch(b, ch);
        }
        if (b->up_lo == b->up_hi)
            return MI_OK;
        bool cap = false;
        const int r = capturing(st, &cap);
        if (r != MI_OK)
            return r;
        MI_REQUIRE(!cap, MI_ESTATE, "mi_compressor_bank: changed settings are sent to the device; call update_settings() before capturing");
        MI_HIP_CHECK(hipMemcpyAsync(b->d_params + b->up_lo, b->params.data() + b->up_lo,
                                    size_t(b->up_hi - b->up_lo) * sizeof(mi_compressor_params_t), hipMemcpyHostToDevice, st));
        MI_HIP_CHECK(hipStreamSynchronize(st));                 // the host table may change again after this returns
        b->up_lo = b->up_hi = 0;
        return MI_OK;
    }

    int comp_launch(mi_compressor_bank *b, float *gain, float *env, const float *in, const float *audio, size_t count,
                    size_t gain_stride, size_t env_stride, size_t in_stride, size_t audio_stride, hipStream_t st)
    {
        const uint32_t vec = (aligned16(in, in_stride, b->channels) ? VEC_IN : 0) | (aligned16(gain, gain_stride, b->channels) ? VEC_GAIN : 0) |
                             (aligned16(env, env_stride, b->channels) ? VEC_ENV : 0) | (aligned16(audio, audio_stride, b->channels) ? VEC_AUDIO : 0);
        hipEvent_t ev0 = nullptr, ev1 = nullptr;
        mi::take_profile_events(&ev0, &ev1);
        MI_LAUNCH(compressor_kernel, dim3((b->channels + GROUP - 1) / GROUP), dim3(BLOCK), 0, st, ev0, ev1, gain, env, in, audio,
                  gain_stride, env_stride, in_stride, audio_stride, uint32_t(count), b->channels, b->d_params, b->d_state, vec);
        MI_HIP_CHECK(hipGetLastError());
        return MI_OK;
    }
} // namespace

namespace mi
{
    int compressor_bank_set_params(mi_compressor_bank_t *b, uint32_t channel, const mi_compressor_params_t *p)
    {
        MI_REQUIRE(b != nullptr && p != nullptr && channel < b->channels, MI_EINVAL, "compressor_bank_set_params: bad argument");
        if (b->update[channel] == 0 && memcmp(&b->params[channel], p, sizeof(*p)) == 0)
            return MI_OK;
        b->params[channel] = *p;
        b->update[channel] = 0;
        touch(b, channel);
        return MI_OK;
    }

    int compressor_bank_set_state(mi_compressor_bank_t *b, uint32_t channel, float envelope, float peak, uint32_t hold, hipStream_t st)
    {
        MI_REQUIRE(b != nullptr && channel < b->channels, MI_EINVAL, "compressor_bank_set_state: bad argument");
        const device_state s = { envelope, peak, hold, 0 };
        MI_HIP_CHECK(hipMemcpyAsync(b->d_state + channel, &s, sizeof(s), hipMemcpyHostToDevice, st));
        MI_HIP_CHECK(hipStreamSynchronize(st));                 // `s` is gone after this returns
        return MI_OK;
    }
}

extern "C" {

int mi_compressor_compute_params(const mi_compressor_settings_t *settings, mi_compressor_params_t *params)
{
    MI_REQUIRE(settings != nullptr && params != nullptr, MI_EINVAL, "mi_compressor_compute_params: NULL argument");
    *params = fresh_params();
    compute_params(*settings, *params);
    return MI_OK;
}

int mi_compressor_bank_create(mi_compressor_bank_t **bank, uint32_t channels)           // Compressor.cpp:46-83
{
    MI_REQUIRE(bank != nullptr, MI_EINVAL, "mi_compressor_bank_create: NULL result pointer");
    *bank = nullptr;
    MI_REQUIRE(channels > 0 && channels <= (1u << 20), MI_EINVAL, "mi_compressor_bank_create: channels must be 1 .. 1048576");
    MI_REQUIRE(mi_dspu_device_count() > 0, MI_ENODEV, "no HIP device available (there is no CPU fallback)");
    mi_compressor_bank *b = new (std::nothrow) mi_compressor_bank();
    MI_REQUIRE(b != nullptr, MI_ENOMEM, "mi_compressor_bank_create: out of host memory");
    b->channels = channels;
    b->cfg.assign(channels, fresh_settings());
    b->update.assign(channels, 1);
    b->params.assign(channels, fresh_params());
    hipError_t e = hipMalloc(reinterpret_cast<void **>(&b->d_params), size_t(channels) * sizeof(mi_compressor_params_t));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&b->d_state), size_t(channels) * sizeof(device_state));
    if (e == hipSuccess) e = hipMemcpy(b->d_params, b->params.data(), size_t(channels) * sizeof(mi_compressor_params_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(b->d_state, 0, size_t(channels) * sizeof(device_state));
    if (e != hipSuccess)
    {
        mi_compressor_bank_destroy(b);
        return mi::fail(MI_EHIP, "mi_compressor_bank_create: %s", hipGetErrorString(e));
    }
    *bank = b;
    return MI_OK;
}

int mi_compressor_bank_destroy(mi_compressor_bank_t *b)
{
    if (b == nullptr)
        return MI_OK;
    (void)hipFree(b->d_params); (void)hipFree(b->d_state);
    delete b;
    return MI_OK;
}

#define MI_COMP_SETTER(name) \
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_compressor_bank_" name ": NULL bank"); \
    MI_REQUIRE(channel < b->channels, MI_EINVAL, "mi_compressor_bank_" name ": channel %u out of range", channel); \
    mi_compressor_settings_t &c = b->cfg[channel]

int mi_compressor_bank_set_sample_rate(mi_compressor_bank_t *b, uint32_t channel, uint32_t sample_rate)    // :420-426
{
    MI_COMP_SETTER("set_sample_rate");
    if (c.sample_rate == sample_rate)
        return MI_OK;
    c.sample_rate = sample_rate;
    b->update[channel] = 1;
    return MI_OK;
}

int mi_compressor_bank_set_mode(mi_compressor_bank_t *b, uint32_t channel, uint32_t mode)                  // :445-452
{
    MI_COMP_SETTER("set_mode");
    if (c.mode == mode)
        return MI_OK;
    c.mode = mode;
    b->update[channel] = 1;
    return MI_OK;
}

int mi_compressor_bank_set_threshold(mi_compressor_bank_t *b, uint32_t channel, float attack, float release)   // :378-385
{
    MI_COMP_SETTER("set_threshold");
    if (c.attack_threshold == attack && c.release_threshold == release)
        return MI_OK;
    c.attack_threshold = attack, c.release_threshold = release;
    b->update[channel] = 1;
    return MI_OK;
}

int mi_compressor_bank_set_boost_threshold(mi_compressor_bank_t *b, uint32_t channel, float boost)        // :387-393
{
    MI_COMP_SETTER("set_boost_threshold");
    if (c.boost_threshold == boost)
        return MI_OK;
    c.boost_threshold = boost;
    b->update[channel] = 1;
    return MI_OK;
}

int mi_compressor_bank_set_timings(mi_compressor_bank_t *b, uint32_t channel, float attack, float release)     // :395-402
{
    MI_COMP_SETTER("set_timings");
    if (c.attack == attack && c.release == release)
        return MI_OK;
    c.attack = attack, c.release = release;
    b->update[channel] = 1;
    return MI_OK;
}

int mi_compressor_bank_set_hold(mi_compressor_bank_t *b, uint32_t channel, float hold)                    // :454-461
{
    MI_COMP_SETTER("set_hold");
    hold = (hold > 0.0f) ? hold : 0.0f;
    if (c.hold == hold)
        return MI_OK;
    c.hold = hold;
    b->update[channel] = 1;
    return MI_OK;
}

int mi_compressor_bank_set_knee(mi_compressor_bank_t *b, uint32_t channel, float knee)                    // :428-435
{
    MI_COMP_SETTER("set_knee");
    knee = (knee < 0.0f) ? 0.0f : (knee > 1.0f) ? 1.0f : knee;
    if (c.knee == knee)
        return MI_OK;
    c.knee = knee;
    b->update[channel] = 1;
    return MI_OK;
}

int mi_compressor_bank_set_ratio(mi_compressor_bank_t *b, uint32_t channel, float ratio)                  // :437-443
{
    MI_COMP_SETTER("set_ratio");
    if (c.ratio == ratio)
        return MI_OK;
    c.ratio = ratio;
    b->update[channel] = 1;
    return MI_OK;
}

#undef MI_COMP_SETTER

int mi_compressor_bank_update_settings(mi_compressor_bank_t *b, void *stream)                              // :89-220
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_compressor_bank_update_settings: NULL bank");
    return comp_update(b, mi::as_stream(stream));
}

int mi_compressor_bank_clear(mi_compressor_bank_t *b, void *stream)
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_compressor_bank_clear: NULL bank");
    MI_HIP_CHECK(hipMemsetAsync(b->d_state, 0, size_t(b->channels) * sizeof(device_state), mi::as_stream(stream)));
    return MI_OK;
}

int mi_compressor_bank_get_params(const mi_compressor_bank_t *b, uint32_t channel, mi_compressor_params_t *params)
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_compressor_bank_get_params: NULL bank");
    MI_REQUIRE(channel < b->channels && params != nullptr, MI_EINVAL, "mi_compressor_bank_get_params: bad argument");
    *params = b->params[channel];
    return MI_OK;
}

int mi_compressor_bank_get_state(mi_compressor_bank_t *b, uint32_t channel, float *envelope, float *peak, uint32_t *hold,
                                 void *stream)
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_compressor_bank_get_state: NULL bank");
    MI_REQUIRE(channel < b->channels, MI_EINVAL, "mi_compressor_bank_get_state: channel %u out of range", channel);
    hipStream_t st = mi::as_stream(stream);
    device_state s;
    MI_HIP_CHECK(hipMemcpyAsync(&s, b->d_state + channel, sizeof(s), hipMemcpyDeviceToHost, st));
    MI_HIP_CHECK(hipStreamSynchronize(st));
    if (envelope != nullptr) *envelope = s.e;
    if (peak != nullptr) *peak = s.peak;
    if (hold != nullptr) *hold = s.hold;
    return MI_OK;
}

int mi_compressor_bank_process(mi_compressor_bank_t *b, float *gain, float *env, const float *in, size_t count,
                               size_t gain_stride, size_t env_stride, size_t in_stride, void *stream)     // :222-267
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_compressor_bank_process: NULL bank");
    hipStream_t st = mi::as_stream(stream);
    const int r = comp_update(b, st);
    if (r != MI_OK || count == 0)
        return r;
    MI_REQUIRE(gain != nullptr && in != nullptr, MI_EINVAL, "mi_compressor_bank_process: NULL buffer");
    MI_REQUIRE(count < (size_t(1) << 31), MI_EINVAL, "mi_compressor_bank_process: count %zu too large", count);
    MI_REQUIRE(b->channels == 1 || (gain_stride >= count && in_stride >= count && (env == nullptr || env_stride >= count)), MI_EINVAL,
               "mi_compressor_bank_process: strides (%zu, %zu, %zu) shorter than count %zu", gain_stride, env_stride, in_stride, count);
    MI_REQUIRE(gain != env, MI_EINVAL, "mi_compressor_bank_process: gain and env are the same buffer");
    MI_REQUIRE((gain != in || gain_stride == in_stride) && (env != in || env_stride == in_stride), MI_EINVAL,
               "mi_compressor_bank_process: in place with different strides");
    return comp_launch(b, gain, env, in, nullptr, count, gain_stride, env_stride, in_stride, 0, st);
}

int mi_compressor_bank_process_apply(mi_compressor_bank_t *b, float *dst, const float *audio, const float *sc, size_t count,
                                     size_t dst_stride, size_t audio_stride, size_t sc_stride, void *stream)
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_compressor_bank_process_apply: NULL bank");
    hipStream_t st = mi::as_stream(stream);
    const int r = comp_update(b, st);
    if (r != MI_OK || count == 0)
        return r;
    MI_REQUIRE(dst != nullptr && audio != nullptr && sc != nullptr, MI_EINVAL, "mi_compressor_bank_process_apply: NULL buffer");
    MI_REQUIRE(count < (size_t(1) << 31), MI_EINVAL, "mi_compressor_bank_process_apply: count %zu too large", count);
    MI_REQUIRE(b->channels == 1 || (dst_stride >= count && audio_stride >= count && sc_stride >= count), MI_EINVAL,
               "mi_compressor_bank_process_apply: strides (%zu, %zu, %zu) shorter than count %zu", dst_stride, audio_stride, sc_stride, count);
    MI_REQUIRE((dst != audio || dst_stride == audio_stride) && (dst != sc || dst_stride == sc_stride), MI_EINVAL,
               "mi_compressor_bank_process_apply: in place with different strides");
    return comp_launch(b, dst, nullptr, sc, audio, count, dst_stride, 0, sc_stride, audio_stride, st);
}

int mi_compressor_bank_curve(mi_compressor_bank_t *b, float *out, const float *in, size_t dots, size_t out_stride,
                             size_t in_stride, void *stream)                                               // :313-316
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_compressor_bank_curve: NULL bank");
    hipStream_t st = mi::as_stream(stream);
    const int r = comp_update(b, st);
    if (r != MI_OK || dots == 0)
        return r;
    MI_REQUIRE(out != nullptr && in != nullptr, MI_EINVAL, "mi_compressor_bank_curve: NULL buffer");
    MI_REQUIRE(dots < (size_t(1) << 31), MI_EINVAL, "mi_compressor_bank_curve: %zu dots are too many", dots);
    MI_REQUIRE(b->channels <= 65535u, MI_EINVAL, "mi_compressor_bank_curve: more than 65535 channels");
    MI_REQUIRE(b->channels == 1 || (out_stride >= dots && in_stride >= dots), MI_EINVAL,
               "mi_compressor_bank_curve: strides (%zu, %zu) shorter than %zu dots", out_stride, in_stride, dots);
    MI_REQUIRE(out != in || out_stride == in_stride, MI_EINVAL, "mi_compressor_bank_curve: in place with different strides");
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    mi::take_profile_events(&ev0, &ev1);
    MI_LAUNCH(compressor_curve_kernel, dim3(uint32_t((dots + CURVE_BLOCK - 1) / CURVE_BLOCK), b->channels), dim3(CURVE_BLOCK), 0, st,
              ev0, ev1, out, in, out_stride, in_stride, uint32_t(dots), b->d_params);
    MI_HIP_CHECK(hipGetLastError());
    return MI_OK;
}

} // extern "C"
