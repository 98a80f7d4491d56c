// lsp::dspu::Expander as a bank of `channels` expanders (src/main/dynamics/Expander.cpp): the envelope follower of process()
// (:252-284), which is the Compressor's statement for statement, and the one-knee gain of Expander::amplification(float)
// (:375-407), upward with a ceiling or downward with a hard floor.  dsp::uexpander_x1_gain / dexpander_x1_gain live in the
// absent lsp-dsp-lib; the scalar overload is the specification.
//
// expander_kernel is follow_kernel of dynamics_device.h, the kernel that compressor_kernel is as well: prepare loads the input
// tile, the chain is the follower in place in LDS (expander_follow_tile, a function of its own so that its instructions can
// be looked at, tests/test_expander_host.py), emit computes the gain from the envelope and stores.  The channels of a
// workgroup may be in different modes: the mode is uniform over a helper wave (one row each).  The bank around the kernel is
// dynamics_bank_core.h's; this file holds the Expander's own curve, settings and setters.
//
// Inputs are finite: NaN is out of scope.  Subnormal envelopes are kept (the float32 denormal mode is on).
#include "expander_bank.h"
#include "dynamics_bank_core.h"

#include <lsp-plug.in/dsp-units/units.h>

#include <cmath>

#pragma clang fp contract(off)      // every product and every sum below rounds on its own, host and device

namespace
{
    using namespace mi_dynamics;
    using lsp::dspu::millis_to_samples;

    // the follower (Expander.cpp:258-278) over samples [0, n) of one row in LDS, in place: row[i] becomes the envelope
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

    // the Expander as follow_kernel sees it: a helper holds its row's knee and mode
    struct expander
    {
        typedef mi_expander_params_t params_t;
        struct row { mi_expander_knee_t kn; bool upward; };
        static __device__ __forceinline__ row load(const params_t &p) { return row{ p.k, p.upward != 0 }; }
        static __device__ __forceinline__ float gain(float e, const row &r) { return x1_gain(e, r.kn, r.upward); }
        static __device__ __forceinline__ follow_state follow(lds_float *tile, uint32_t n, follow_state s, float ta, float tr, float rt,
                                                              uint32_t nhold)
        {
            return expander_follow_tile(tile, n, s, ta, tr, rt, nhold);
        }
    };
    constexpr auto expander_kernel = follow_kernel<expander>;

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
} // namespace

struct mi_expander_bank : mi_bank::settings_bank<mi_expander_settings_t, mi_expander_params_t, device_state>
{
    static constexpr const char *NAME = "mi_expander_bank";

    static mi_expander_settings_t fresh_settings()                              // Expander::construct, Expander.cpp:70-101
    {
        mi_expander_settings_t s = {};
        s.mode = MI_EM_UPWARD;
        s.ratio = 1.0f;
        return s;
    }
    static mi_expander_params_t fresh_params()
    {
        mi_expander_params_t p = {};
        p.upward = 1;
        return p;
    }
    static device_state fresh_state() { return device_state{}; }
    static void compute(const mi_expander_settings_t &s, mi_expander_params_t &p) { compute_params(s, p); }
    template <class... Args> static void launch(dim3 grid, hipStream_t st, hipEvent_t ev0, hipEvent_t ev1, Args... args)
    {
        MI_LAUNCH(expander_kernel, grid, dim3(BLOCK), 0, st, ev0, ev1, args...);
    }
};

namespace mi
{
    int expander_bank_set_params(mi_expander_bank_t *b, uint32_t channel, const mi_expander_params_t *p)
    {
        return mi_bank::set_params(b, "expander_bank_set_params", channel, p);
    }

    int expander_bank_set_state(mi_expander_bank_t *b, uint32_t channel, float envelope, float peak, uint32_t hold, hipStream_t st)
    {
        return mi_bank::set_state(b, "expander_bank_set_state", channel, device_state{ envelope, peak, hold, 0 }, true, st);
    }
}

extern "C" {

int mi_expander_compute_params(const mi_expander_settings_t *settings, mi_expander_params_t *params)
{
    MI_REQUIRE(settings != nullptr && params != nullptr, MI_EINVAL, "mi_expander_compute_params: NULL argument");
    *params = mi_expander_bank::fresh_params();
    compute_params(*settings, *params);
    return MI_OK;
}

int mi_expander_bank_create(mi_expander_bank_t **bank, uint32_t channels)               // Expander.cpp:70-101
{
    return mi_bank::create(bank, "mi_expander_bank_create", channels);
}

int mi_expander_bank_destroy(mi_expander_bank_t *b)
{
    return mi_bank::destroy(b);
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
    return mi_bank::update_settings(b, "mi_expander_bank_update_settings", stream);
}

int mi_expander_bank_clear(mi_expander_bank_t *b, void *stream)
{
    return mi_bank::clear(b, "mi_expander_bank_clear", stream);
}

int mi_expander_bank_get_params(const mi_expander_bank_t *b, uint32_t channel, mi_expander_params_t *params)
{
    return mi_bank::get_params(b, "mi_expander_bank_get_params", channel, params);
}

int mi_expander_bank_get_state(mi_expander_bank_t *b, uint32_t channel, float *envelope, float *peak, uint32_t *hold,
                               void *stream)
{
    return mi_dynamics::get_follow_state(b, "mi_expander_bank_get_state", channel, envelope, peak, hold, stream);
}

int mi_expander_bank_process(mi_expander_bank_t *b, float *gain, float *env, const float *in, size_t count,
                             size_t gain_stride, size_t env_stride, size_t in_stride, void *stream)       // :247-292
{
    return mi_dynamics::process(b, "mi_expander_bank_process", gain, env, in, count, gain_stride, env_stride, in_stride, stream);
}

int mi_expander_bank_process_apply(mi_expander_bank_t *b, float *dst, const float *audio, const float *sc, size_t count,
                                   size_t dst_stride, size_t audio_stride, size_t sc_stride, void *stream)
{
    return mi_dynamics::process_apply(b, "mi_expander_bank_process_apply", dst, audio, sc, count, dst_stride, audio_stride, sc_stride,
                                      stream);
}

int mi_expander_bank_curve(mi_expander_bank_t *b, float *out, const float *in, size_t dots, size_t out_stride,
                           size_t in_stride, void *stream)                                                 // :325-365
{
    return mi_dynamics::curve(b, "mi_expander_bank_curve", out, in, dots, out_stride, in_stride, stream,
                              [&](dim3 grid, hipStream_t st, hipEvent_t ev0, hipEvent_t ev1)
    {
        MI_LAUNCH(expander_curve_kernel, grid, dim3(CURVE_BLOCK), 0, st, ev0, ev1, out, in, out_stride, in_stride, uint32_t(dots),
                  b->d_params);
    });
}

} // extern "C"
