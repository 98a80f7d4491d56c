// lsp::dspu::Compressor as a bank of `channels` compressors (src/main/dynamics/Compressor.cpp): the envelope follower of
// process() (:226-259) and the two-knee gain curve of dsp::compressor_x2_gain, which the scalar overload (:297-310) states
// in full.
//
// The follower is a serial recurrence over (fEnvelope, fPeak, nHoldCounter) whose branch depends on the running value: one
// lane per channel, the state in registers for the whole call and in a device array between calls (no host positions, so
// calls can be captured into a graph and replayed).  The gain curve is element-wise.  compressor_kernel runs both in one
// launch: it is follow_kernel of dynamics_device.h on the tile walk of tile_chain_device.h, where the chain is the follower,
// the envelope written over the input in LDS; prepare is the load of the input; emit is the gain from the envelope and the
// stores, so gain, env and dst may each be the input row.  The follower's tau * d and e + ... round once each (no fused
// multiply-add): compressor_follow_tile is a function of its own so that its instructions can be looked at
// (tests/test_compressor_host.py), and the envelope matches tests/compressor_ref.py bit for bit.  The bank around the kernel
// is dynamics_bank_core.h's; this file holds the Compressor's own curve, settings and setters.
//
// Inputs are finite: NaN is out of scope.  Subnormal envelopes are kept (the float32 denormal mode is on).
#include "compressor_bank.h"
#include "dynamics_bank_core.h"

#include <lsp-plug.in/dsp-units/units.h>

#include <cmath>

#pragma clang fp contract(off)      // every product and every sum below rounds on its own, host and device

namespace
{
    using namespace mi_dynamics;
    using lsp::dspu::millis_to_samples;

    // the follower (Compressor.cpp:231-256) over samples [0, n) of one row in LDS, in place: row[i] becomes the envelope
    __device__ __noinline__ follow_state compressor_follow_tile(lds_float *row, uint32_t n, follow_state s, float ta, float tr,
                                                                float rt, uint32_t nhold)
    {
        float e = s.e, peak = s.peak;
        uint32_t hold = s.hold;
        chain_batches(row, 0, n, [&](float v) { follow_step(v, e, peak, hold, ta, tr, rt, nhold); return e; });
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

    // the Compressor as follow_kernel sees it: a helper holds its row's two knees
    struct compressor
    {
        typedef mi_compressor_params_t params_t;
        struct row { mi_compressor_knee_t k0, k1; };
        static __device__ __forceinline__ row load(const params_t &p) { return row{ p.k[0], p.k[1] }; }
        static __device__ __forceinline__ float gain(float e, const row &r) { return x2_gain(e, r.k0, r.k1); }
        static __device__ __forceinline__ follow_state follow(lds_float *tile, uint32_t n, follow_state s, float ta, float tr, float rt,
                                                              uint32_t nhold)
        {
            return compressor_follow_tile(tile, n, s, ta, tr, rt, nhold);
        }
    };
    constexpr auto compressor_kernel = follow_kernel<compressor>;

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
} // namespace

struct mi_compressor_bank : mi_bank::settings_bank<mi_compressor_settings_t, mi_compressor_params_t, device_state>
{
    static constexpr const char *NAME = "mi_compressor_bank";

    static mi_compressor_settings_t fresh_settings()                            // Compressor::construct, Compressor.cpp:46-83
    {
        mi_compressor_settings_t s = {};
        s.mode = MI_CM_DOWNWARD;
        s.boost_threshold = float(2.5119e-4);                                   // GAIN_AMP_M_72_DB
        s.ratio = 1.0f;
        return s;
    }
    static mi_compressor_params_t fresh_params()
    {
        mi_compressor_params_t p = {};
        p.k[0].gain = p.k[1].gain = 1.0f;
        return p;
    }
    static device_state fresh_state() { return device_state{}; }
    static void compute(const mi_compressor_settings_t &s, mi_compressor_params_t &p) { compute_params(s, p); }
    template <class... Args> static void launch(dim3 grid, hipStream_t st, hipEvent_t ev0, hipEvent_t ev1, Args... args)
    {
        MI_LAUNCH(compressor_kernel, grid, dim3(BLOCK), 0, st, ev0, ev1, args...);
    }
};

namespace mi
{
    int compressor_bank_set_params(mi_compressor_bank_t *b, uint32_t channel, const mi_compressor_params_t *p)
    {
        return mi_bank::set_params(b, "compressor_bank_set_params", channel, p);
    }

    int compressor_bank_set_state(mi_compressor_bank_t *b, uint32_t channel, float envelope, float peak, uint32_t hold, hipStream_t st)
    {
        return mi_bank::set_state(b, "compressor_bank_set_state", channel, device_state{ envelope, peak, hold, 0 }, true, st);
    }
}

extern "C" {

int mi_compressor_compute_params(const mi_compressor_settings_t *settings, mi_compressor_params_t *params)
{
    MI_REQUIRE(settings != nullptr && params != nullptr, MI_EINVAL, "mi_compressor_compute_params: NULL argument");
    *params = mi_compressor_bank::fresh_params();
    compute_params(*settings, *params);
    return MI_OK;
}

int mi_compressor_bank_create(mi_compressor_bank_t **bank, uint32_t channels)           // Compressor.cpp:46-83
{
    return mi_bank::create(bank, "mi_compressor_bank_create", channels);
}

int mi_compressor_bank_destroy(mi_compressor_bank_t *b)
{
    return mi_bank::destroy(b);
}

int mi_compressor_bank_set_sample_rate(mi_compressor_bank_t *b, uint32_t channel, uint32_t sample_rate)    // :420-426
{
    MI_BANK_SETTER("compressor", "set_sample_rate");
    if (c.sample_rate == sample_rate)
        return MI_OK;
    c.sample_rate = sample_rate;
    b->update[channel] = 1;
    return MI_OK;
}

int mi_compressor_bank_set_mode(mi_compressor_bank_t *b, uint32_t channel, uint32_t mode)                  // :445-452
{
    MI_BANK_SETTER("compressor", "set_mode");
    if (c.mode == mode)
        return MI_OK;
    c.mode = mode;
    b->update[channel] = 1;
    return MI_OK;
}

int mi_compressor_bank_set_threshold(mi_compressor_bank_t *b, uint32_t channel, float attack, float release)   // :378-385
{
    MI_BANK_SETTER("compressor", "set_threshold");
    if (c.attack_threshold == attack && c.release_threshold == release)
        return MI_OK;
    c.attack_threshold = attack, c.release_threshold = release;
    b->update[channel] = 1;
    return MI_OK;
}

int mi_compressor_bank_set_boost_threshold(mi_compressor_bank_t *b, uint32_t channel, float boost)        // :387-393
{
    MI_BANK_SETTER("compressor", "set_boost_threshold");
    if (c.boost_threshold == boost)
        return MI_OK;
    c.boost_threshold = boost;
    b->update[channel] = 1;
    return MI_OK;
}

int mi_compressor_bank_set_timings(mi_compressor_bank_t *b, uint32_t channel, float attack, float release)     // :395-402
{
    MI_BANK_SETTER("compressor", "set_timings");
    if (c.attack == attack && c.release == release)
        return MI_OK;
    c.attack = attack, c.release = release;
    b->update[channel] = 1;
    return MI_OK;
}

int mi_compressor_bank_set_hold(mi_compressor_bank_t *b, uint32_t channel, float hold)                    // :454-461
{
    MI_BANK_SETTER("compressor", "set_hold");
    hold = (hold > 0.0f) ? hold : 0.0f;
    if (c.hold == hold)
        return MI_OK;
    c.hold = hold;
    b->update[channel] = 1;
    return MI_OK;
}

int mi_compressor_bank_set_knee(mi_compressor_bank_t *b, uint32_t channel, float knee)                    // :428-435
{
    MI_BANK_SETTER("compressor", "set_knee");
    knee = (knee < 0.0f) ? 0.0f : (knee > 1.0f) ? 1.0f : knee;
    if (c.knee == knee)
        return MI_OK;
    c.knee = knee;
    b->update[channel] = 1;
    return MI_OK;
}

int mi_compressor_bank_set_ratio(mi_compressor_bank_t *b, uint32_t channel, float ratio)                  // :437-443
{
    MI_BANK_SETTER("compressor", "set_ratio");
    if (c.ratio == ratio)
        return MI_OK;
    c.ratio = ratio;
    b->update[channel] = 1;
    return MI_OK;
}

int mi_compressor_bank_update_settings(mi_compressor_bank_t *b, void *stream)                              // :89-220
{
    return mi_bank::update_settings(b, "mi_compressor_bank_update_settings", stream);
}

int mi_compressor_bank_clear(mi_compressor_bank_t *b, void *stream)
{
    return mi_bank::clear(b, "mi_compressor_bank_clear", stream);
}

int mi_compressor_bank_get_params(const mi_compressor_bank_t *b, uint32_t channel, mi_compressor_params_t *params)
{
    return mi_bank::get_params(b, "mi_compressor_bank_get_params", channel, params);
}

int mi_compressor_bank_get_state(mi_compressor_bank_t *b, uint32_t channel, float *envelope, float *peak, uint32_t *hold,
                                 void *stream)
{
    return mi_dynamics::get_follow_state(b, "mi_compressor_bank_get_state", channel, envelope, peak, hold, stream);
}

int mi_compressor_bank_process(mi_compressor_bank_t *b, float *gain, float *env, const float *in, size_t count,
                               size_t gain_stride, size_t env_stride, size_t in_stride, void *stream)     // :222-267
{
    return mi_dynamics::process(b, "mi_compressor_bank_process", gain, env, in, count, gain_stride, env_stride, in_stride, stream);
}

int mi_compressor_bank_process_apply(mi_compressor_bank_t *b, float *dst, const float *audio, const float *sc, size_t count,
                                     size_t dst_stride, size_t audio_stride, size_t sc_stride, void *stream)
{
    return mi_dynamics::process_apply(b, "mi_compressor_bank_process_apply", dst, audio, sc, count, dst_stride, audio_stride, sc_stride,
                                      stream);
}

int mi_compressor_bank_curve(mi_compressor_bank_t *b, float *out, const float *in, size_t dots, size_t out_stride,
                             size_t in_stride, void *stream)                                               // :313-316
{
    return mi_dynamics::curve(b, "mi_compressor_bank_curve", out, in, dots, out_stride, in_stride, stream,
                              [&](dim3 grid, hipStream_t st, hipEvent_t ev0, hipEvent_t ev1)
    {
        MI_LAUNCH(compressor_curve_kernel, grid, dim3(CURVE_BLOCK), 0, st, ev0, ev1, out, in, out_stride, in_stride, uint32_t(dots),
                  b->d_params);
    });
}

} // extern "C"
