// lsp::dspu::Expander as a bank of `channels` expanders (src/main/dynamics/Expander.cpp): the envelope follower of process()
// (:252-284), which is the Compressor's statement for statement, and the one-knee gain of Expander::amplification(float)
// (:375-407), upward with a ceiling or downward with a hard floor.  dsp::uexpander_x1_gain / dexpander_x1_gain live in the
// absent lsp-dsp-lib; the scalar overload is the specification.
//
// expander_kernel runs on the tile walk of tile_chain_device.h exactly as compressor_kernel does: prepare loads the input
// tile, the chain is the follower in place in LDS (expander_follow_tile, a function of its own so that its instructions can
// be looked at, tests/test_expander_host.py), emit computes the gain from the envelope and stores.  The follower's step is
// repeated here from compressor.hip on purpose: that file stays as it is.  The channels of a workgroup may be in different
// modes: the mode is uniform over a helper wave (one row each).
//
// Inputs are finite: NaN is out of scope.  Subnormal envelopes are kept (the float32 denormal mode is on).
#include "expander_bank.h"
#include "tile_chain_device.h"

#include <lsp-plug.in/dsp-units/units.h>

#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#pragma clang fp contract(off)      // every product and every sum below rounds on its own, host and device

namespace
{
    using namespace mi_tile_chain;
    using lsp::dspu::millis_to_samples;

    constexpr int CURVE_BLOCK = 256;

    enum { VEC_IN = 1, VEC_GAIN = 2, VEC_ENV = 4, VEC_AUDIO = 8 };

    struct follow_state { float e, peak; uint32_t hold; };
    struct device_state { float e, peak; uint32_t hold, pad; };     // [channels] between calls

    // Expander.cpp:258-278, one sample
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

    // ... over samples [0, n) of one row in LDS, in place: row[i] becomes the envelope
    __device__ __noinline__ follow_state expander_follow_tile(lds_float *row, uint32_t n, follow_state s, float ta, float tr,
                                                              float rt, uint32_t nhold)
    {
        float e = s.e, peak = s.peak;
        uint32_t hold = s.hold;
        chain_batches(row, 0, n, [&](float v) { follow_step(v, e, peak, hold, ta, tr, rt, nhold); return e; });
        return follow_state{ e, peak, hold };
    }

    // Expander.cpp:375-407: the gain for the envelope e
    __device__ __forceinline__ float x1_gain(float e, const mi_expander_knee_t &k, bool upward)
    {
        float x = fabsf(e);
        if (upward)
        {
            x = (x > k.threshold) ? k.threshold : x;
            if (!(x > k.start))
                return 1.0f;
        }
        else
        {
            if (x < k.threshold)
                return 0.0f;
            if (!(x < k.end))
                return 1.0f;
        }
        const float lx = logf(x);
        const bool line = upward ? (x >= k.end) : (x <= k.start);
        return expf(line ? k.tilt[0] * lx + k.tilt[1] : (k.herm[0] * lx + k.herm[1]) * lx + k.herm[2]);
    }

    // gain (audio == NULL) or dst = audio * gain into `gain`, the envelope into `env` unless NULL.  vec: which of the buffers
    // have 16-byte aligned rows.
    __global__ __launch_bounds__(BLOCK) void expander_kernel(float *gain, float *env, const float *in, const float *audio,
                                                             size_t gain_stride, size_t env_stride, size_t in_stride,
                                                             size_t audio_stride, uint32_t count, uint32_t channels,
                                                             const mi_expander_params_t *params, device_state *state,
                                                             uint32_t vec)
    {
        __shared__ __attribute__((aligned(16))) float tile[2][GROUP][ROW];
        const role me = my_role(channels);
        const uint32_t r = me.r, ch = me.ch, c = me.c;

        // the follower's lane: its channel's state and taus; a helper: its row's knee and mode
        follow_state fs = { 0.0f, 0.0f, 0 };
        float ta = 0.0f, tr = 0.0f, rt = 0.0f;
        uint32_t nhold = 0;
        mi_expander_knee_t kn = {};
        bool upward = false;
        if (me.valid && me.chain)
        {
            const device_state s = state[ch];
            fs = follow_state{ s.e, s.peak, s.hold };
            ta = params[ch].tau_attack, tr = params[ch].tau_release, rt = params[ch].release_threshold, nhold = params[ch].hold;
        }
        else if (me.valid)
            kn = params[ch].k, upward = params[ch].upward != 0;
        const float *xs = in + size_t(ch) * in_stride;
        const float *as = (audio != nullptr) ? audio + size_t(ch) * audio_stride : nullptr;
        float *gs = gain + size_t(ch) * gain_stride;
        float *es = (env != nullptr) ? env + size_t(ch) * env_stride : nullptr;

        auto load_tile = [&](uint32_t k)
        {
            const extent t = tile_extent(count, k);
            float *l = &tile[k & 1][r][c];
            if ((vec & VEC_IN) && c + 4 <= t.n)
                *reinterpret_cast<float4 *>(l) = *reinterpret_cast<const float4 *>(xs + t.t0 + c);
            else
            {
                #pragma unroll
                for (uint32_t j = 0; j < 4; ++j)
                    if (c + j < t.n)
                        l[j] = xs[t.t0 + c + j];
            }
        };
        auto emit_tile = [&](uint32_t k)
        {
            const extent t = tile_extent(count, k);
            if (c >= t.n)
                return;
            const float4 e4 = *reinterpret_cast<const float4 *>(&tile[k & 1][r][c]);
            const float e[4] = { e4.x, e4.y, e4.z, e4.w };
            float g[4];
            #pragma unroll
            for (uint32_t j = 0; j < 4; ++j)
                g[j] = (c + j < t.n) ? x1_gain(e[j], kn, upward) : 0.0f;
            if (as != nullptr)
            {
                float a[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
                if ((vec & VEC_AUDIO) && c + 4 <= t.n)
                {
                    const float4 a4 = *reinterpret_cast<const float4 *>(as + t.t0 + c);
                    a[0] = a4.x, a[1] = a4.y, a[2] = a4.z, a[3] = a4.w;
                }
                else
                {
                    #pragma unroll
                    for (uint32_t j = 0; j < 4; ++j)
                        if (c + j < t.n)
                            a[j] = as[t.t0 + c + j];
                }
                #pragma unroll
                for (uint32_t j = 0; j < 4; ++j)
                    g[j] = a[j] * g[j];
            }
            store_quad(gs + t.t0 + c, g, vec & VEC_GAIN, c, t.n);
            if (es != nullptr)
                store_quad(es + t.t0 + c, e, vec & VEC_ENV, c, t.n);
        };

        MI_TILE_CHAIN_WALK(me, count, k, load_tile(k),
                           fs = expander_follow_tile((lds_float *)&tile[k & 1][r][0], tile_extent(count, k).n, fs, ta, tr, rt, nhold),
                           emit_tile(k));
        if (me.valid && me.chain)
            state[ch] = device_state{ fs.e, fs.peak, fs.hold, 0 };
    }

    // Expander::curve(float), Expander.cpp:333-365, over rows.  The returned level is the limited one: upward, a level above
    // the threshold comes back as threshold * gain(threshold), as the reference has it.
    __global__ __launch_bounds__(CURVE_BLOCK) void expander_curve_kernel(float *out, const float *in, size_t out_stride,
                                                                         size_t in_stride, uint32_t dots,
                                                                         const mi_expander_params_t *params)
    {
        const uint32_t ch = blockIdx.y, i = blockIdx.x * CURVE_BLOCK + threadIdx.x;
        if (i >= dots)
            return;
        const mi_expander_knee_t kn = params[ch].k;
        const bool upward = params[ch].upward != 0;
        float x = fabsf(in[size_t(ch) * in_stride + i]);
        if (upward)
            x = (x > kn.threshold) ? kn.threshold : x;
        const float g = x1_gain(x, kn, upward);
        // 0 and 1 are returned as such (return 0.0f / return x): the product with them is exact
        out[size_t(ch) * out_stride + i] = x * g;
    }

    // interpolation::hermite_quadratic, src/main/misc/interpolation.cpp:103-109
    void hermite_quadratic(float *p, float x0, float y0, float k0, float x1, float k1)
    {
        p[0] = (k0 - k1) * 0.5f / (x0 - x1);
        p[1] = k0 - 2.0f * p[0] * x0;
        p[2] = y0 - (p[0] * x0 + p[1]) * x0;
    }

    // square_roots, Expander.cpp:44-57: the larger (upward) or the smaller (downward) root of p(x) = y, picked as
    // lsp_max / lsp_min pick it (a > b ? a : b, a < b ? a : b)
    float square_root(const float *p, float y, bool larger)
    {
        const float a = p[0], b = -p[1], c = p[2] - y;
        const float d = sqrtf(b * b - 4.0f * a * c);
        const float k = 1.0f / (a + a);
        const float x1 = (b + d) * k, x2 = (b - d) * k;
        return larger ? ((x1 > x2) ? x1 : x2) : ((x1 < x2) ? x1 : x2);
    }

    // Expander::update_settings, Expander.cpp:200-245, in host float32
    void compute_params(const mi_expander_settings_t &s, mi_expander_params_t &p)
    {
        constexpr float MINIMUM_TILT = 0.001f, UPPER_THRESHOLD = 13.815510558f, LOWER_THRESHOLD = -16.118095651f;
        constexpr float MIN_LOWER_THRESHOLD = 1e-7f, MAX_UPPER_THRESHOLD = 1e+6f;
        const float sr = float(s.sample_rate);
        const float k707 = logf(float(1.0 - M_SQRT1_2));
        p.tau_attack = 1.0f - expf(k707 / millis_to_samples(sr, s.attack));
        p.tau_release = 1.0f - expf(k707 / millis_to_samples(sr, s.release));
        p.release_threshold = s.release_threshold;
        p.hold = uint32_t(millis_to_samples(sr, s.hold));
        p.upward = (s.mode == MI_EM_UPWARD) ? 1 : 0;
        mi_expander_knee_t &k = p.k;
        k.start = s.attack_threshold * s.knee;
        k.end = s.attack_threshold / s.knee;
        const float log_ks = logf(k.start), log_ke = logf(k.end), log_th = logf(s.attack_threshold);
        k.tilt[0] = s.ratio - 1.0f;
        k.tilt[1] = log_th * (1.0f - s.ratio);
        const float tilt = (k.tilt[0] > MINIMUM_TILT) ? k.tilt[0] : MINIMUM_TILT;
        if (p.upward)
        {
            hermite_quadratic(k.herm, log_ks, 0.0f, 0.0f, log_ke, k.tilt[0]);
            float ut = expf((UPPER_THRESHOLD - k.tilt[1]) / tilt);
            if (ut < k.end)
                ut = expf(square_root(k.herm, UPPER_THRESHOLD, true));
            k.threshold = (ut < MAX_UPPER_THRESHOLD) ? ut : MAX_UPPER_THRESHOLD;
        }
        else
        {
            hermite_quadratic(k.herm, log_ke, 0.0f, 0.0f, log_ks, k.tilt[0]);
            float dt = expf((LOWER_THRESHOLD - k.tilt[1]) / tilt);
            if (dt > k.start)
                dt = expf(square_root(k.herm, LOWER_THRESHOLD, false));
            k.threshold = (dt > MIN_LOWER_THRESHOLD) ? dt : MIN_LOWER_THRESHOLD;
        }
    }

    // Expander::construct, Expander.cpp:70-101
    mi_expander_settings_t fresh_settings()
    {
        mi_expander_settings_t s = {};
        s.mode = MI_EM_UPWARD;
        s.ratio = 1.0f;
        return s;
    }

    mi_expander_params_t fresh_params()
    {
        mi_expander_params_t p = {};
        p.upward = 1;
        return p;
    }
} // namespace

struct mi_expander_bank
{
    uint32_t                                channels = 0;
    std::vector<mi_expander_settings_t>     cfg;            // the setters' values
    std::vector<uint8_t>                    update;         // bUpdate of every channel
    std::vector<mi_expander_params_t>       params;         // what update_settings computed
    mi::dirty_range                         up;             // where params differs from the device table
    mi_expander_params_t                   *d_params = nullptr;     // [channels]
    device_state                           *d_state = nullptr;      // [channels]
};

namespace
{
    // update_settings of every channel whose bUpdate is set; the changed stretch of the table goes to the device
    int exp_update(mi_expander_bank *b, hipStream_t st)
    {
        for (uint32_t ch = 0; ch < b->channels; ++ch)
        {
            if (!b->update[ch])
                continue;
            compute_params(b->cfg[ch], b->params[ch]);
            b->update[ch] = 0;
            b->up.touch(ch);
        }
        return mi::upload_dirty("mi_expander_bank", b->d_params, b->params.data(), b->up, st);
    }

    int exp_launch(mi_expander_bank *b, float *gain, float *env, const float *in, const float *audio, size_t count,
                   size_t gain_stride, size_t env_stride, size_t in_stride, size_t audio_stride, hipStream_t st)
    {
        const uint32_t vec = (mi::aligned16(in, in_stride, b->channels) ? VEC_IN : 0) | (mi::aligned16(gain, gain_stride, b->channels) ? VEC_GAIN : 0) |
                             (mi::aligned16(env, env_stride, b->channels) ? VEC_ENV : 0) | (mi::aligned16(audio, audio_stride, b->channels) ? VEC_AUDIO : 0);
        hipEvent_t ev0 = nullptr, ev1 = nullptr;
        mi::take_profile_events(&ev0, &ev1);
        MI_LAUNCH(expander_kernel, dim3((b->channels + GROUP - 1) / GROUP), dim3(BLOCK), 0, st, ev0, ev1, gain, env, in, audio,
                  gain_stride, env_stride, in_stride, audio_stride, uint32_t(count), b->channels, b->d_params, b->d_state, vec);
        MI_HIP_CHECK(hipGetLastError());
        return MI_OK;
    }
} // namespace

namespace mi
{
    int expander_bank_set_params(mi_expander_bank_t *b, uint32_t channel, const mi_expander_params_t *p)
    {
        MI_REQUIRE(b != nullptr && p != nullptr && channel < b->channels, MI_EINVAL, "expander_bank_set_params: bad argument");
        if (b->update[channel] == 0 && memcmp(&b->params[channel], p, sizeof(*p)) == 0)
            return MI_OK;
        b->params[channel] = *p;
        b->update[channel] = 0;
        b->up.touch(channel);
        return MI_OK;
    }

    int expander_bank_set_state(mi_expander_bank_t *b, uint32_t channel, float envelope, float peak, uint32_t hold, hipStream_t st)
    {
        MI_REQUIRE(b != nullptr && channel < b->channels, MI_EINVAL, "expander_bank_set_state: bad argument");
        return mi::write_state(b->d_state + channel, device_state{ envelope, peak, hold, 0 }, st);
    }
}

extern "C" {

int mi_expander_compute_params(const mi_expander_settings_t *settings, mi_expander_params_t *params)
{
    MI_REQUIRE(settings != nullptr && params != nullptr, MI_EINVAL, "mi_expander_compute_params: NULL argument");
    *params = fresh_params();
    compute_params(*settings, *params);
    return MI_OK;
}

int mi_expander_bank_create(mi_expander_bank_t **bank, uint32_t channels)               // Expander.cpp:70-101
{
    MI_REQUIRE(bank != nullptr, MI_EINVAL, "mi_expander_bank_create: NULL result pointer");
    *bank = nullptr;
    MI_REQUIRE(channels > 0 && channels <= (1u << 20), MI_EINVAL, "mi_expander_bank_create: channels must be 1 .. 1048576");
    MI_REQUIRE(mi_dspu_device_count() > 0, MI_ENODEV, "no HIP device available (there is no CPU fallback)");
    mi_expander_bank *b = new (std::nothrow) mi_expander_bank();
    MI_REQUIRE(b != nullptr, MI_ENOMEM, "mi_expander_bank_create: out of host memory");
    b->channels = channels;
    b->cfg.assign(channels, fresh_settings());
    b->update.assign(channels, 1);
    b->params.assign(channels, fresh_params());
    hipError_t e = hipMalloc(reinterpret_cast<void **>(&b->d_params), size_t(channels) * sizeof(mi_expander_params_t));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&b->d_state), size_t(channels) * sizeof(device_state));
    if (e == hipSuccess) e = hipMemcpy(b->d_params, b->params.data(), size_t(channels) * sizeof(mi_expander_params_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(b->d_state, 0, size_t(channels) * sizeof(device_state));
    if (e != hipSuccess)
    {
        mi_expander_bank_destroy(b);
        return mi::fail(MI_EHIP, "mi_expander_bank_create: %s", hipGetErrorString(e));
    }
    *bank = b;
    return MI_OK;
}

int mi_expander_bank_destroy(mi_expander_bank_t *b)
{
    if (b == nullptr)
        return MI_OK;
    (void)hipFree(b->d_params); (void)hipFree(b->d_state);
    delete b;
    return MI_OK;
}

int mi_expander_bank_set_sample_rate(mi_expander_bank_t *b, uint32_t channel, uint32_t sample_rate)       // :157-163
{
    MI_BANK_SETTER("expander", "set_sample_rate");
    if (c.sample_rate == sample_rate)
        return MI_OK;
    c.sample_rate = sample_rate;
    b->update[channel] = 1;
    return MI_OK;
}

int mi_expander_bank_set_mode(mi_expander_bank_t *b, uint32_t channel, uint32_t mode)                     // :181-189
{
    MI_BANK_SETTER("expander", "set_mode");
    const uint32_t upward = (mode == MI_EM_UPWARD) ? MI_EM_UPWARD : MI_EM_DOWNWARD;
    if (c.mode == upward)
        return MI_OK;
    c.mode = upward;
    b->update[channel] = 1;
    return MI_OK;
}

int mi_expander_bank_set_threshold(mi_expander_bank_t *b, uint32_t channel, float attack, float release)  // :123-130
{
    MI_BANK_SETTER("expander", "set_threshold");
    if (c.attack_threshold == attack && c.release_threshold == release)
        return MI_OK;
    c.attack_threshold = attack, c.release_threshold = release;
    b->update[channel] = 1;
    return MI_OK;
}

int mi_expander_bank_set_timings(mi_expander_bank_t *b, uint32_t channel, float attack, float release)    // :132-139
{
    MI_BANK_SETTER("expander", "set_timings");
    if (c.attack == attack && c.release == release)
        return MI_OK;
    c.attack = attack, c.release = release;
    b->update[channel] = 1;
    return MI_OK;
}

int mi_expander_bank_set_hold(mi_expander_bank_t *b, uint32_t channel, float hold)                        // :191-198
{
    MI_BANK_SETTER("expander", "set_hold");
    hold = (hold > 0.0f) ? hold : 0.0f;
    if (c.hold == hold)
        return MI_OK;
    c.hold = hold;
    b->update[channel] = 1;
    return MI_OK;
}

int mi_expander_bank_set_knee(mi_expander_bank_t *b, uint32_t channel, float knee)                        // :165-171: no limits
{
    MI_BANK_SETTER("expander", "set_knee");
    if (c.knee == knee)
        return MI_OK;
    c.knee = knee;
    b->update[channel] = 1;
    return MI_OK;
}

int mi_expander_bank_set_ratio(mi_expander_bank_t *b, uint32_t channel, float ratio)                      // :173-179
{
    MI_BANK_SETTER("expander", "set_ratio");
    if (c.ratio == ratio)
        return MI_OK;
    c.ratio = ratio;
    b->update[channel] = 1;
    return MI_OK;
}

int mi_expander_bank_update_settings(mi_expander_bank_t *b, void *stream)                                  // :200-245
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_expander_bank_update_settings: NULL bank");
    return exp_update(b, mi::as_stream(stream));
}

int mi_expander_bank_clear(mi_expander_bank_t *b, void *stream)
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_expander_bank_clear: NULL bank");
    MI_HIP_CHECK(hipMemsetAsync(b->d_state, 0, size_t(b->channels) * sizeof(device_state), mi::as_stream(stream)));
    return MI_OK;
}

int mi_expander_bank_get_params(const mi_expander_bank_t *b, uint32_t channel, mi_expander_params_t *params)
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_expander_bank_get_params: NULL bank");
    MI_REQUIRE(channel < b->channels && params != nullptr, MI_EINVAL, "mi_expander_bank_get_params: bad argument");
    *params = b->params[channel];
    return MI_OK;
}

int mi_expander_bank_get_state(mi_expander_bank_t *b, uint32_t channel, float *envelope, float *peak, uint32_t *hold,
                               void *stream)
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_expander_bank_get_state: NULL bank");
    MI_REQUIRE(channel < b->channels, MI_EINVAL, "mi_expander_bank_get_state: channel %u out of range", channel);
    device_state s;
    const int r = mi::read_state(&s, b->d_state + channel, mi::as_stream(stream));
    if (r != MI_OK)
        return r;
    if (envelope != nullptr) *envelope = s.e;
    if (peak != nullptr) *peak = s.peak;
    if (hold != nullptr) *hold = s.hold;
    return MI_OK;
}

int mi_expander_bank_process(mi_expander_bank_t *b, float *gain, float *env, const float *in, size_t count,
                             size_t gain_stride, size_t env_stride, size_t in_stride, void *stream)       // :247-292
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_expander_bank_process: NULL bank");
    hipStream_t st = mi::as_stream(stream);
    const int r = exp_update(b, st);
    if (r != MI_OK || count == 0)
        return r;
    MI_REQUIRE(gain != nullptr && in != nullptr, MI_EINVAL, "mi_expander_bank_process: NULL buffer");
    MI_REQUIRE(count < (size_t(1) << 31), MI_EINVAL, "mi_expander_bank_process: count %zu too large", count);
    MI_REQUIRE(b->channels == 1 || (gain_stride >= count && in_stride >= count && (env == nullptr || env_stride >= count)), MI_EINVAL,
               "mi_expander_bank_process: strides (%zu, %zu, %zu) shorter than count %zu", gain_stride, env_stride, in_stride, count);
    MI_REQUIRE(gain != env, MI_EINVAL, "mi_expander_bank_process: gain and env are the same buffer");
    MI_REQUIRE((gain != in || gain_stride == in_stride) && (env != in || env_stride == in_stride), MI_EINVAL,
               "mi_expander_bank_process: in place with different strides");
    return exp_launch(b, gain, env, in, nullptr, count, gain_stride, env_stride, in_stride, 0, st);
}

int mi_expander_bank_process_apply(mi_expander_bank_t *b, float *dst, const float *audio, const float *sc, size_t count,
                                   size_t dst_stride, size_t audio_stride, size_t sc_stride, void *stream)
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_expander_bank_process_apply: NULL bank");
    hipStream_t st = mi::as_stream(stream);
    const int r = exp_update(b, st);
    if (r != MI_OK || count == 0)
        return r;
    MI_REQUIRE(dst != nullptr && audio != nullptr && sc != nullptr, MI_EINVAL, "mi_expander_bank_process_apply: NULL buffer");
    MI_REQUIRE(count < (size_t(1) << 31), MI_EINVAL, "mi_expander_bank_process_apply: count %zu too large", count);
    MI_REQUIRE(b->channels == 1 || (dst_stride >= count && audio_stride >= count && sc_stride >= count), MI_EINVAL,
               "mi_expander_bank_process_apply: strides (%zu, %zu, %zu) shorter than count %zu", dst_stride, audio_stride, sc_stride, count);
    MI_REQUIRE((dst != audio || dst_stride == audio_stride) && (dst != sc || dst_stride == sc_stride), MI_EINVAL,
               "mi_expander_bank_process_apply: in place with different strides");
    return exp_launch(b, dst, nullptr, sc, audio, count, dst_stride, 0, sc_stride, audio_stride, st);
}

int mi_expander_bank_curve(mi_expander_bank_t *b, float *out, const float *in, size_t dots, size_t out_stride,
                           size_t in_stride, void *stream)                                                 // :325-365
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_expander_bank_curve: NULL bank");
    hipStream_t st = mi::as_stream(stream);
    const int r = exp_update(b, st);
    if (r != MI_OK || dots == 0)
        return r;
    MI_REQUIRE(out != nullptr && in != nullptr, MI_EINVAL, "mi_expander_bank_curve: NULL buffer");
    MI_REQUIRE(dots < (size_t(1) << 31), MI_EINVAL, "mi_expander_bank_curve: %zu dots are too many", dots);
    MI_REQUIRE(b->channels <= 65535u, MI_EINVAL, "mi_expander_bank_curve: more than 65535 channels");
    MI_REQUIRE(b->channels == 1 || (out_stride >= dots && in_stride >= dots), MI_EINVAL,
               "mi_expander_bank_curve: strides (%zu, %zu) shorter than %zu dots", out_stride, in_stride, dots);
    MI_REQUIRE(out != in || out_stride == in_stride, MI_EINVAL, "mi_expander_bank_curve: in place with different strides");
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    mi::take_profile_events(&ev0, &ev1);
    MI_LAUNCH(expander_curve_kernel, dim3(uint32_t((dots + CURVE_BLOCK - 1) / CURVE_BLOCK), b->channels), dim3(CURVE_BLOCK), 0, st,
              ev0, ev1, out, in, out_stride, in_stride, uint32_t(dots), b->d_params);
    MI_HIP_CHECK(hipGetLastError());
    return MI_OK;
}

} // extern "C"
