// lsp::dspu::Gate as a bank of `channels` gates (src/main/dynamics/Gate.cpp): the block process() (:267-367) restated per
// sample.  The follower is the Compressor's without the release threshold.  The gain is one of two cubic-Hermite curves,
// open (0) and close (1), chosen by hysteresis on the running envelope: on curve 0 an envelope above sCurves[0].sKnee.end,
// on curve 1 one below sCurves[1].sKnee.start makes the reference leave its inner loop WITHOUT advancing -- the samples
// before take the old curve, the follower then runs a second time on the same input sample under the new curve, and that
// sample's envelope and gain are the second step's (a hold counter the first step decremented is decremented again).
// dsp::gate_x1_gain lives in the absent lsp-dsp-lib; Gate::amplification(float) (:250-265) is the specification.
//
// gate_kernel runs on the tile walk of tile_chain_device.h.  Prepare loads the input tile; the chain (gate_follow_tile, a
// function of its own so that its instructions can be looked at) writes the envelope over the input in LDS and the curve
// index of every sample into bit words beside the tile, one bit per sample, eight words per row and buffer; emit, after the
// walk's barrier, takes its four bits and evaluates the knee each selects.  The input sample stays in a register for the
// second step, so the arithmetic is the reference's out-of-place call whichever buffers alias.  The bit words are the Gate's
// alone, so the kernel is its own and not follow_kernel of dynamics_device.h (the two knees held in one struct for it also
// put pick() through a selected address: 80 bytes of scratch per lane); the flags, the end of the follower's step and the
// bank around the kernel (dynamics_bank_core.h) are the shared ones.
//
// THE SAMPLE LOOP IS BOUNDED BY count ALONE: a sample is stepped again at most once, then the walk advances.  With
// sCurves[1].sKnee.start <= sCurves[0].sKnee.end and taus in [0, 1] the reference never does more; with
// inverted thresholds it may never return, and the bank differs from it there on purpose.
//
// Inputs are finite: NaN is out of scope.  Subnormal envelopes are kept (the float32 denormal mode is on).
#include "gate_bank.h"
#include "dynamics_bank_core.h"

#include <lsp-plug.in/dsp-units/units.h>

#include <cmath>

#pragma clang fp contract(off)      // every product and every sum below rounds on its own, host and device

namespace
{
    using namespace mi_dynamics;
    using lsp::dspu::millis_to_samples;

    constexpr int WORDS = TILE / 32;                                // bit words of a row: one bit per sample

    typedef __attribute__((address_space(3))) uint32_t lds_u32;

    struct gate_state { float e, peak; uint32_t hold, curve; };     // in registers, and [channels] between calls

    // Gate.cpp:284-306 (and :322-344, the same text), one sample
    __device__ __forceinline__ void follow_step(float s, float &e, float &peak, uint32_t &hold, float ta, float tr, uint32_t nhold)
    {
        const float d = s - e;
        const bool neg = d < 0.0f;
        const float en = e + (neg ? tr : ta) * d;
        MI_FOLLOW_SETTLE(e, peak, hold, neg, en, nhold);
    }

    // ... over samples [0, n) of one row in LDS, in place: row[i] becomes the envelope, bit i of bits[] the curve of sample i
    // (words [0, ceil(n / 32)) are written).  The crossing is rare: a branch, with the second step behind it.
    __device__ __noinline__ gate_state gate_follow_tile(lds_float *row, lds_u32 *bits, uint32_t n, gate_state s, float ta, float tr,
                                                        uint32_t nhold, float end0, float start1)
    {
        float e = s.e, peak = s.peak;
        uint32_t hold = s.hold, curve = s.curve;
        uint32_t idx = 0, word = 0;
        chain_batches(row, 0, n, [&](float v)
        {
            follow_step(v, e, peak, hold, ta, tr, nhold);
            const bool crossed = (curve != 0) ? (e < start1) : (e > end0);
            if (__builtin_expect(crossed, 0))
            {
                curve ^= 1u;
                follow_step(v, e, peak, hold, ta, tr, nhold);       // once, whatever it gives: the walk advances
            }
            word |= curve << (idx & 31u);
            if ((idx & 31u) == 31u)
            {
                bits[idx >> 5] = word;
                word = 0;
            }
            ++idx;
            return e;
        });
        if ((idx & 31u) != 0)
            bits[idx >> 5] = word;
        return gate_state{ e, peak, hold, curve };
    }

    // Gate.cpp:250-265 with the knee given: the gain for the envelope e
    __device__ __forceinline__ float x1_gain(float e, const mi_gate_knee_t &k)
    {
        const float x = fabsf(e);
        if (x <= k.start)
            return k.gain_start;
        if (x >= k.end)
            return k.gain_end;
        const float lx = logf(x);
        return expf(((k.herm[0] * lx + k.herm[1]) * lx + k.herm[2]) * lx + k.herm[3]);
    }

    __device__ __forceinline__ mi_gate_knee_t pick(bool close, const mi_gate_knee_t &k0, const mi_gate_knee_t &k1)
    {
        mi_gate_knee_t k;
        k.start = close ? k1.start : k0.start, k.end = close ? k1.end : k0.end;
        k.gain_start = close ? k1.gain_start : k0.gain_start, k.gain_end = close ? k1.gain_end : k0.gain_end;
        #pragma unroll
        for (int i = 0; i < 4; ++i)
            k.herm[i] = close ? k1.herm[i] : k0.herm[i];
        return k;
    }

    // gain (audio == NULL) or dst = audio * gain into `gain`, the envelope into `env` unless NULL.  vec: which of the buffers
    // have 16-byte aligned rows.
    __global__ __launch_bounds__(BLOCK) void gate_kernel(float *gain, float *env, const float *in, const float *audio,
                                                         size_t gain_stride, size_t env_stride, size_t in_stride,
                                                         size_t audio_stride, uint32_t count, uint32_t channels,
                                                         const mi_gate_params_t *params, gate_state *state, uint32_t vec)
    {
        __shared__ __attribute__((aligned(16))) float tile[2][GROUP][ROW];
        // The curve bits: written by the chain's lane of the row (a word per 32 samples), read by the row's helper wave after
        // the barrier, eight lanes on one word (a broadcast), the wave on eight consecutive words: no bank is asked twice.
        __shared__ uint32_t curve_bits[2][GROUP][WORDS];
        const role me = my_role(channels);
        const uint32_t r = me.r, ch = me.ch, c = me.c;

        // the follower's lane: its channel's state, taus and the two limits; a helper: its row's knees
        gate_state fs = { 0.0f, 0.0f, 0, 0 };
        float ta = 0.0f, tr = 0.0f, end0 = 0.0f, start1 = 0.0f;
        uint32_t nhold = 0;
        mi_gate_knee_t k0 = {}, k1 = {};
        if (me.valid && me.chain)
        {
            fs = state[ch];
            ta = params[ch].tau_attack, tr = params[ch].tau_release, nhold = params[ch].hold;
            end0 = params[ch].k[0].end, start1 = params[ch].k[1].start;
        }
        else if (me.valid)
            k0 = params[ch].k[0], k1 = params[ch].k[1];
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
            const uint32_t four = curve_bits[k & 1][r][c >> 5] >> (c & 31u);        // samples c .. c + 3: bits 0 .. 3
            float g[4];
            #pragma unroll
            for (uint32_t j = 0; j < 4; ++j)
                g[j] = (c + j < t.n) ? x1_gain(e[j], pick(((four >> j) & 1u) != 0, k0, k1)) : 0.0f;
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
                           fs = gate_follow_tile((lds_float *)&tile[k & 1][r][0], (lds_u32 *)&curve_bits[k & 1][r][0],
                                                 tile_extent(count, k).n, fs, ta, tr, nhold, end0, start1),
                           emit_tile(k));
        if (me.valid && me.chain)
            state[ch] = fs;
    }

    // Gate::curve(float, bool), Gate.cpp:212-226, over rows: out = gain(|in|) * |in| on the open or the close curve
    __global__ __launch_bounds__(CURVE_BLOCK) void gate_curve_kernel(float *out, const float *in, size_t out_stride, size_t in_stride,
                                                                     uint32_t dots, const mi_gate_params_t *params, uint32_t hyst)
    {
        const uint32_t ch = blockIdx.y, i = blockIdx.x * CURVE_BLOCK + threadIdx.x;
        if (i >= dots)
            return;
        const mi_gate_knee_t k = params[ch].k[hyst];
        const float x = fabsf(in[size_t(ch) * in_stride + i]);
        out[size_t(ch) * out_stride + i] = x * x1_gain(x, k);
    }

    // interpolation::hermite_cubic, src/main/misc/interpolation.cpp:112-131: the differences and products of float
    // arguments are float32, what is assigned to a double or meets one is double
    void hermite_cubic(float *p, float x0, float y0, float k0, float x1, float y1, float k1)
    {
        const double dx = x1 - x0;
        const double dy = y1 - y0;
        const double kx = dy / dx;
        const double xx1 = x1 * x1;
        const double xx2 = x0 + x1;
        const double a = ((k0 + k1) * dx - 2.0f * dy) / (dx * dx * dx);
        const double b = ((kx - k0) + a * ((2.0f * x0 - x1) * x0 - xx1)) / dx;
        const double c = kx - a * (xx1 + xx2 * x0) - b * xx2;
        const double d = y0 - x0 * (c + x0 * (b + x0 * a));
        p[0] = float(a), p[1] = float(b), p[2] = float(c), p[3] = float(d);
    }

    // Gate::update_settings, Gate.cpp:180-205, in host float32
    void compute_params(const mi_gate_settings_t &s, mi_gate_params_t &p)
    {
        const float sr = float(s.sample_rate);
        const float k707 = logf(float(1.0 - M_SQRT1_2));
        p.tau_attack = 1.0f - expf(k707 / millis_to_samples(sr, s.attack));
        p.tau_release = 1.0f - expf(k707 / millis_to_samples(sr, s.release));
        p.hold = uint32_t(millis_to_samples(sr, s.hold));
        p.reserved = 0;
        for (int i = 0; i < 2; ++i)
        {
            mi_gate_knee_t &k = p.k[i];
            k.start = s.threshold[i] * s.zone[i];
            k.end = s.threshold[i];
            k.gain_start = (s.reduction <= 1.0f) ? s.reduction : 1.0f;
            k.gain_end = (s.reduction <= 1.0f) ? 1.0f : 1.0f / s.reduction;
            hermite_cubic(k.herm, logf(k.start), logf(k.gain_start), 0.0f, logf(k.end), logf(k.gain_end), 0.0f);
        }
    }

} // namespace

struct mi_gate_bank : mi_bank::settings_bank<mi_gate_settings_t, mi_gate_params_t, gate_state>
{
    static constexpr const char *NAME = "mi_gate_bank";

    static mi_gate_settings_t fresh_settings()                                  // Gate::construct, Gate.cpp:41-74
    {
        mi_gate_settings_t s = {};
        s.zone[0] = s.zone[1] = 1.0f;
        return s;
    }
    static mi_gate_params_t fresh_params() { return mi_gate_params_t{}; }
    static gate_state fresh_state() { return gate_state{}; }
    static void compute(const mi_gate_settings_t &s, mi_gate_params_t &p) { compute_params(s, p); }
    template <class... Args> static void launch(dim3 grid, hipStream_t st, hipEvent_t ev0, hipEvent_t ev1, Args... args)
    {
        MI_LAUNCH(gate_kernel, grid, dim3(BLOCK), 0, st, ev0, ev1, args...);
    }
};

namespace mi
{
    int gate_bank_set_params(mi_gate_bank_t *b, uint32_t channel, const mi_gate_params_t *p)
    {
        return mi_bank::set_params(b, "gate_bank_set_params", channel, p);
    }

    int gate_bank_set_state(mi_gate_bank_t *b, uint32_t channel, float envelope, float peak, uint32_t hold, uint32_t curve, hipStream_t st)
    {
        return mi_bank::set_state(b, "gate_bank_set_state", channel, gate_state{ envelope, peak, hold, curve }, curve <= 1, st);
    }
}

extern "C" {

int mi_gate_compute_params(const mi_gate_settings_t *settings, mi_gate_params_t *params)
{
    MI_REQUIRE(settings != nullptr && params != nullptr, MI_EINVAL, "mi_gate_compute_params: NULL argument");
    *params = mi_gate_bank::fresh_params();
    compute_params(*settings, *params);
    return MI_OK;
}

int mi_gate_bank_create(mi_gate_bank_t **bank, uint32_t channels)                       // Gate.cpp:41-74
{
    return mi_bank::create(bank, "mi_gate_bank_create", channels);
}

int mi_gate_bank_destroy(mi_gate_bank_t *b)
{
    return mi_bank::destroy(b);
}

int mi_gate_bank_set_sample_rate(mi_gate_bank_t *b, uint32_t channel, uint32_t sample_rate)               // :138-144
{
    MI_BANK_SETTER("gate", "set_sample_rate");
    if (c.sample_rate == sample_rate)
        return MI_OK;
    c.sample_rate = sample_rate;
    b->update[channel] = 1;
    return MI_OK;
}

int mi_gate_bank_set_threshold(mi_gate_bank_t *b, uint32_t channel, float open, float close)              // :80-87
{
    MI_BANK_SETTER("gate", "set_threshold");
    if (c.threshold[0] == open && c.threshold[1] == close)
        return MI_OK;
    c.threshold[0] = open, c.threshold[1] = close;
    b->update[channel] = 1;
    return MI_OK;
}

int mi_gate_bank_set_zone(mi_gate_bank_t *b, uint32_t channel, float open, float close)                   // :146-153
{
    MI_BANK_SETTER("gate", "set_zone");
    if (c.zone[0] == open && c.zone[1] == close)
        return MI_OK;
    c.zone[0] = open, c.zone[1] = close;
    b->update[channel] = 1;
    return MI_OK;
}

int mi_gate_bank_set_reduction(mi_gate_bank_t *b, uint32_t channel, float reduction)                      // :105-111
{
    MI_BANK_SETTER("gate", "set_reduction");
    if (c.reduction == reduction)
        return MI_OK;
    c.reduction = reduction;
    b->update[channel] = 1;
    return MI_OK;
}

int mi_gate_bank_set_timings(mi_gate_bank_t *b, uint32_t channel, float attack, float release)            // :113-120
{
    MI_BANK_SETTER("gate", "set_timings");
    if (c.attack == attack && c.release == release)
        return MI_OK;
    c.attack = attack, c.release = release;
    b->update[channel] = 1;
    return MI_OK;
}

int mi_gate_bank_set_hold(mi_gate_bank_t *b, uint32_t channel, float hold)                                // :171-178
{
    MI_BANK_SETTER("gate", "set_hold");
    hold = (hold > 0.0f) ? hold : 0.0f;
    if (c.hold == hold)
        return MI_OK;
    c.hold = hold;
    b->update[channel] = 1;
    return MI_OK;
}

int mi_gate_bank_update_settings(mi_gate_bank_t *b, void *stream)                                          // :180-205
{
    return mi_bank::update_settings(b, "mi_gate_bank_update_settings", stream);
}

int mi_gate_bank_clear(mi_gate_bank_t *b, void *stream)
{
    return mi_bank::clear(b, "mi_gate_bank_clear", stream);
}

int mi_gate_bank_get_params(const mi_gate_bank_t *b, uint32_t channel, mi_gate_params_t *params)
{
    return mi_bank::get_params(b, "mi_gate_bank_get_params", channel, params);
}

int mi_gate_bank_get_state(mi_gate_bank_t *b, uint32_t channel, float *envelope, float *peak, uint32_t *hold, uint32_t *curve,
                           void *stream)
{
    gate_state s;
    const int r = mi_bank::get_state(b, "mi_gate_bank_get_state", channel, &s, stream);
    if (r != MI_OK)
        return r;
    if (envelope != nullptr) *envelope = s.e;
    if (peak != nullptr) *peak = s.peak;
    if (hold != nullptr) *hold = s.hold;
    if (curve != nullptr) *curve = s.curve;
    return MI_OK;
}

int mi_gate_bank_process(mi_gate_bank_t *b, float *gain, float *env, const float *in, size_t count,
                         size_t gain_stride, size_t env_stride, size_t in_stride, void *stream)           // :267-367
{
    return mi_dynamics::process(b, "mi_gate_bank_process", gain, env, in, count, gain_stride, env_stride, in_stride, stream);
}

int mi_gate_bank_process_apply(mi_gate_bank_t *b, float *dst, const float *audio, const float *sc, size_t count,
                               size_t dst_stride, size_t audio_stride, size_t sc_stride, void *stream)
{
    return mi_dynamics::process_apply(b, "mi_gate_bank_process_apply", dst, audio, sc, count, dst_stride, audio_stride, sc_stride, stream);
}

int mi_gate_bank_curve(mi_gate_bank_t *b, float *out, const float *in, size_t dots, int hyst, size_t out_stride, size_t in_stride,
                       void *stream)                                                                       // :207-226
{
    return mi_dynamics::curve(b, "mi_gate_bank_curve", out, in, dots, out_stride, in_stride, stream,
                              [&](dim3 grid, hipStream_t st, hipEvent_t ev0, hipEvent_t ev1)
    {
        MI_LAUNCH(gate_curve_kernel, grid, dim3(CURVE_BLOCK), 0, st, ev0, ev1, out, in, out_stride, in_stride, uint32_t(dots),
                  b->d_params, uint32_t(hyst != 0 ? 1 : 0));
    });
}

} // extern "C"
