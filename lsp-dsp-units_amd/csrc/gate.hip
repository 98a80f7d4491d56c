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
// second step, so the arithmetic is the reference's out-of-place call whichever buffers alias.
//
// THE SAMPLE LOOP IS BOUNDED BY count ALONE: a sample is stepped again at most once, then the walk advances.  With
// sCurves[1].sKnee.start <= sCurves[0].sKnee.end and taus in [0, 1] the reference never does more; with
// inverted thresholds it may never return, and the bank differs from it there on purpose.
//
// Inputs are finite: NaN is out of scope.  Subnormal envelopes are kept (the float32 denormal mode is on).
#include "gate_bank.h"
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
    constexpr int WORDS = TILE / 32;                                // bit words of a row: one bit per sample

    typedef __attribute__((address_space(3))) uint32_t lds_u32;

    enum { VEC_IN = 1, VEC_GAIN = 2, VEC_ENV = 4, VEC_AUDIO = 8 };

    struct gate_state { float e, peak; uint32_t hold, curve; };     // in registers, and [channels] between calls

    // Gate.cpp:284-306 (and :322-344, the same text), one sample
    __device__ __forceinline__ void follow_step(float s, float &e, float &peak, uint32_t &hold, float ta, float tr, uint32_t nhold)
    {
        const float d = s - e;
        const bool neg = d < 0.0f;
        const float en = e + (neg ? tr : ta) * d;
        const bool held = neg && hold > 0;
        const bool rearm = !neg && en >= peak;
        e = held ? e : en;
        peak = ((neg && !held) || rearm) ? en : peak;
        hold = held ? hold - 1 : rearm ? nhold : hold;
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

    // Gate::construct, Gate.cpp:41-74
    mi_gate_settings_t fresh_settings()
    {
        mi_gate_settings_t s = {};
        s.zone[0] = s.zone[1] = 1.0f;
        return s;
    }
} // namespace

struct mi_gate_bank
{
    uint32_t                            channels = 0;
    std::vector<mi_gate_settings_t>     cfg;            // the setters' values
    std::vector<uint8_t>                update;         // bUpdate of every channel
    std::vector<mi_gate_params_t>       params;         // what update_settings computed
    mi::dirty_range                     up;             // where params differs from the device table
    mi_gate_params_t                   *d_params = nullptr;     // [channels]
    gate_state                         *d_state = nullptr;      // [channels]
};

namespace
{
    // update_settings of every channel whose bUpdate is set; the changed stretch of the table goes to the device
    int gate_update(mi_gate_bank *b, hipStream_t st)
    {
        for (uint32_t ch = 0; ch < b->channels; ++ch)
        {
            if (!b->update[ch])
                continue;
            compute_params(b->cfg[ch], b->params[ch]);
            b->update[ch] = 0;
            b->up.touch(ch);
        }
        return mi::upload_dirty("mi_gate_bank", b->d_params, b->params.data(), b->up, st);
    }

    int gate_launch(mi_gate_bank *b, float *gain, float *env, const float *in, const float *audio, size_t count,
                    size_t gain_stride, size_t env_stride, size_t in_stride, size_t audio_stride, hipStream_t st)
    {
        const uint32_t vec = (mi::aligned16(in, in_stride, b->channels) ? VEC_IN : 0) | (mi::aligned16(gain, gain_stride, b->channels) ? VEC_GAIN : 0) |
                             (mi::aligned16(env, env_stride, b->channels) ? VEC_ENV : 0) | (mi::aligned16(audio, audio_stride, b->channels) ? VEC_AUDIO : 0);
        hipEvent_t ev0 = nullptr, ev1 = nullptr;
        mi::take_profile_events(&ev0, &ev1);
        MI_LAUNCH(gate_kernel, dim3((b->channels + GROUP - 1) / GROUP), dim3(BLOCK), 0, st, ev0, ev1, gain, env, in, audio,
                  gain_stride, env_stride, in_stride, audio_stride, uint32_t(count), b->channels, b->d_params, b->d_state, vec);
        MI_HIP_CHECK(hipGetLastError());
        return MI_OK;
    }
} // namespace

namespace mi
{
    int gate_bank_set_params(mi_gate_bank_t *b, uint32_t channel, const mi_gate_params_t *p)
    {
        MI_REQUIRE(b != nullptr && p != nullptr && channel < b->channels, MI_EINVAL, "gate_bank_set_params: bad argument");
        if (b->update[channel] == 0 && memcmp(&b->params[channel], p, sizeof(*p)) == 0)
            return MI_OK;
        b->params[channel] = *p;
        b->update[channel] = 0;
        b->up.touch(channel);
        return MI_OK;
    }

    int gate_bank_set_state(mi_gate_bank_t *b, uint32_t channel, float envelope, float peak, uint32_t hold, uint32_t curve, hipStream_t st)
    {
        MI_REQUIRE(b != nullptr && channel < b->channels && curve <= 1, MI_EINVAL, "gate_bank_set_state: bad argument");
        return mi::write_state(b->d_state + channel, gate_state{ envelope, peak, hold, curve }, st);
    }
}

extern "C" {

int mi_gate_compute_params(const mi_gate_settings_t *settings, mi_gate_params_t *params)
{
    MI_REQUIRE(settings != nullptr && params != nullptr, MI_EINVAL, "mi_gate_compute_params: NULL argument");
    *params = mi_gate_params_t{};
    compute_params(*settings, *params);
    return MI_OK;
}

int mi_gate_bank_create(mi_gate_bank_t **bank, uint32_t channels)                       // Gate.cpp:41-74
{
    MI_REQUIRE(bank != nullptr, MI_EINVAL, "mi_gate_bank_create: NULL result pointer");
    *bank = nullptr;
    MI_REQUIRE(channels > 0 && channels <= (1u << 20), MI_EINVAL, "mi_gate_bank_create: channels must be 1 .. 1048576");
    MI_REQUIRE(mi_dspu_device_count() > 0, MI_ENODEV, "no HIP device available (there is no CPU fallback)");
    mi_gate_bank *b = new (std::nothrow) mi_gate_bank();
    MI_REQUIRE(b != nullptr, MI_ENOMEM, "mi_gate_bank_create: out of host memory");
    b->channels = channels;
    b->cfg.assign(channels, fresh_settings());
    b->update.assign(channels, 1);
    b->params.assign(channels, mi_gate_params_t{});
    hipError_t e = hipMalloc(reinterpret_cast<void **>(&b->d_params), size_t(channels) * sizeof(mi_gate_params_t));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&b->d_state), size_t(channels) * sizeof(gate_state));
    if (e == hipSuccess) e = hipMemcpy(b->d_params, b->params.data(), size_t(channels) * sizeof(mi_gate_params_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(b->d_state, 0, size_t(channels) * sizeof(gate_state));
    if (e != hipSuccess)
    {
        mi_gate_bank_destroy(b);
        return mi::fail(MI_EHIP, "mi_gate_bank_create: %s", hipGetErrorString(e));
    }
    *bank = b;
    return MI_OK;
}

int mi_gate_bank_destroy(mi_gate_bank_t *b)
{
    if (b == nullptr)
        return MI_OK;
    (void)hipFree(b->d_params); (void)hipFree(b->d_state);
    delete b;
    return MI_OK;
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
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_gate_bank_update_settings: NULL bank");
    return gate_update(b, mi::as_stream(stream));
}

int mi_gate_bank_clear(mi_gate_bank_t *b, void *stream)
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_gate_bank_clear: NULL bank");
    MI_HIP_CHECK(hipMemsetAsync(b->d_state, 0, size_t(b->channels) * sizeof(gate_state), mi::as_stream(stream)));
    return MI_OK;
}

int mi_gate_bank_get_params(const mi_gate_bank_t *b, uint32_t channel, mi_gate_params_t *params)
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_gate_bank_get_params: NULL bank");
    MI_REQUIRE(channel < b->channels && params != nullptr, MI_EINVAL, "mi_gate_bank_get_params: bad argument");
    *params = b->params[channel];
    return MI_OK;
}

int mi_gate_bank_get_state(mi_gate_bank_t *b, uint32_t channel, float *envelope, float *peak, uint32_t *hold, uint32_t *curve,
                           void *stream)
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_gate_bank_get_state: NULL bank");
    MI_REQUIRE(channel < b->channels, MI_EINVAL, "mi_gate_bank_get_state: channel %u out of range", channel);
    gate_state s;
    const int r = mi::read_state(&s, b->d_state + channel, mi::as_stream(stream));
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
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_gate_bank_process: NULL bank");
    hipStream_t st = mi::as_stream(stream);
    const int r = gate_update(b, st);
    if (r != MI_OK || count == 0)
        return r;
    MI_REQUIRE(gain != nullptr && in != nullptr, MI_EINVAL, "mi_gate_bank_process: NULL buffer");
    MI_REQUIRE(count < (size_t(1) << 31), MI_EINVAL, "mi_gate_bank_process: count %zu too large", count);
    MI_REQUIRE(b->channels == 1 || (gain_stride >= count && in_stride >= count && (env == nullptr || env_stride >= count)), MI_EINVAL,
               "mi_gate_bank_process: strides (%zu, %zu, %zu) shorter than count %zu", gain_stride, env_stride, in_stride, count);
    MI_REQUIRE(gain != env, MI_EINVAL, "mi_gate_bank_process: gain and env are the same buffer");
    MI_REQUIRE((gain != in || gain_stride == in_stride) && (env != in || env_stride == in_stride), MI_EINVAL,
               "mi_gate_bank_process: in place with different strides");
    return gate_launch(b, gain, env, in, nullptr, count, gain_stride, env_stride, in_stride, 0, st);
}

int mi_gate_bank_process_apply(mi_gate_bank_t *b, float *dst, const float *audio, const float *sc, size_t count,
                               size_t dst_stride, size_t audio_stride, size_t sc_stride, void *stream)
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_gate_bank_process_apply: NULL bank");
    hipStream_t st = mi::as_stream(stream);
    const int r = gate_update(b, st);
    if (r != MI_OK || count == 0)
        return r;
    MI_REQUIRE(dst != nullptr && audio != nullptr && sc != nullptr, MI_EINVAL, "mi_gate_bank_process_apply: NULL buffer");
    MI_REQUIRE(count < (size_t(1) << 31), MI_EINVAL, "mi_gate_bank_process_apply: count %zu too large", count);
    MI_REQUIRE(b->channels == 1 || (dst_stride >= count && audio_stride >= count && sc_stride >= count), MI_EINVAL,
               "mi_gate_bank_process_apply: strides (%zu, %zu, %zu) shorter than count %zu", dst_stride, audio_stride, sc_stride, count);
    MI_REQUIRE((dst != audio || dst_stride == audio_stride) && (dst != sc || dst_stride == sc_stride), MI_EINVAL,
               "mi_gate_bank_process_apply: in place with different strides");
    return gate_launch(b, dst, nullptr, sc, audio, count, dst_stride, 0, sc_stride, audio_stride, st);
}

int mi_gate_bank_curve(mi_gate_bank_t *b, float *out, const float *in, size_t dots, int hyst, size_t out_stride, size_t in_stride,
                       void *stream)                                                                       // :207-226
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_gate_bank_curve: NULL bank");
    hipStream_t st = mi::as_stream(stream);
    const int r = gate_update(b, st);
    if (r != MI_OK || dots == 0)
        return r;
    MI_REQUIRE(out != nullptr && in != nullptr, MI_EINVAL, "mi_gate_bank_curve: NULL buffer");
    MI_REQUIRE(dots < (size_t(1) << 31), MI_EINVAL, "mi_gate_bank_curve: %zu dots are too many", dots);
    MI_REQUIRE(b->channels <= 65535u, MI_EINVAL, "mi_gate_bank_curve: more than 65535 channels");
    MI_REQUIRE(b->channels == 1 || (out_stride >= dots && in_stride >= dots), MI_EINVAL,
               "mi_gate_bank_curve: strides (%zu, %zu) shorter than %zu dots", out_stride, in_stride, dots);
    MI_REQUIRE(out != in || out_stride == in_stride, MI_EINVAL, "mi_gate_bank_curve: in place with different strides");
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    mi::take_profile_events(&ev0, &ev1);
    MI_LAUNCH(gate_curve_kernel, dim3(uint32_t((dots + CURVE_BLOCK - 1) / CURVE_BLOCK), b->channels), dim3(CURVE_BLOCK), 0, st,
              ev0, ev1, out, in, out_stride, in_stride, uint32_t(dots), b->d_params, uint32_t(hyst != 0 ? 1 : 0));
    MI_HIP_CHECK(hipGetLastError());
    return MI_OK;
}

} // extern "C"
