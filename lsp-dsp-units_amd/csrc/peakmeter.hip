// lsp::dspu::PeakMeter as a bank of `channels` meters (src/main/meters/PeakMeter.cpp): a peak hold/decay follower.  Per sample,
// with s = |x| (:127-155):  s >= peak: peak = s, counter = nHold;  else counter > 0: --counter;  else peak *= fTau.
//
// peakmeter_kernel runs it on the tile walk of tile_chain_device.h:
//     prepare          |x| of the input tile into LDS
//     chain            the three-branch step in place: row[i] becomes the peak after sample i
//     emit             the tile out of LDS into `dst` as it is (nothing, where dst is NULL)
// By the walk's invariant `dst` may be the input row.  At the start of every launch the chain's lane does what
// update_settings() does to the state (:124), counter = min(counter, hold): idempotent, since a counter never exceeds the hold
// it was loaded from.  At the end it writes peak and counter back, and the peak into peaks[channel] where the caller gave one.
//
// peakmeter_value_kernel is the block-rate process(value, count) (:185-205), one thread per channel; its branches are NOT the
// per-sample ones (counter >= count, and lsp_max(peak * factor, value) with the counter left alone).  The factor
// expf(logf(fTau) * float(count)) comes out of the parameter table: the HOST forms it, with the libm the reference uses (a device
// expf would not give those bits), for the `count` of the last call.  A call with another count therefore uploads, and is refused
// inside a stream capture like a setter.
//
// peak and counter match tests/peak_surge_ref.py bit for bit: one product per decay step, rounded once.  NaN and Inf samples
// behave as in the reference (the compares are the reference's, so a NaN sample never becomes the peak and a NaN peak stays);
// subnormals are kept (the float32 denormal mode is on): a decaying peak walks down through them to 0.
#include "bank_core.h"
#include "tile_chain_device.h"

#include <lsp-plug.in/dsp-units/units.h>

#include <cmath>

#pragma clang fp contract(off)      // every product below rounds on its own, host and device

namespace
{
    using namespace mi_tile_chain;
    using lsp::dspu::millis_to_samples;

    enum { VEC_DST = 1, VEC_SRC = 2 };
    constexpr int VALUE_BLOCK = 256;
    constexpr size_t COUNT_LIMIT = size_t(1) << 31;     // the kernel counts samples in 32 bits

    struct settings { uint32_t sample_rate; float hold, release; };          // nSampleRate, fHold, fRelease
    struct device_state { float peak; uint32_t counter; };                   // fPeak, nCounter: [channels] between calls

    // One tile of one channel, PeakMeter.cpp:132-150.  A function of its own so that its instructions can be looked at.
    __device__ __noinline__ device_state peakmeter_chain_tile(lds_float *row, uint32_t n, device_state s, float tau, uint32_t hold)
    {
        float peak = s.peak;
        uint32_t counter = s.counter;
        // the three branches as selects (a branch per sample costs the lane more than the product it would skip): the product is
        // formed for every sample and taken only where the reference forms it
        chain_batches(row, 0, n, [&](float v)
        {
            const bool rise = v >= peak, held = counter > 0;
            const float decayed = peak * tau;
            peak = rise ? v : (held ? peak : decayed);
            counter = rise ? hold : counter - (held ? 1u : 0u);
            return peak;
        });
        return device_state{ peak, counter };
    }

    __global__ __launch_bounds__(BLOCK) void peakmeter_kernel(float *dst, const float *src, float *peaks, size_t dst_stride,
                                                              size_t src_stride, uint32_t count, uint32_t channels,
                                                              const mi_peakmeter_params_t *params, device_state *state, uint32_t vec)
    {
        __shared__ __attribute__((aligned(16))) float tile[2][GROUP][ROW];      // |x|, then the peak after sample i
        const role me = my_role(channels);
        const uint32_t r = me.r, ch = me.ch, c = me.c;
        device_state s = { 0.0f, 0 };
        float tau = 0.0f;
        uint32_t hold = 0;
        if (me.valid && me.chain)
        {
            s = state[ch];
            tau = params[ch].tau, hold = params[ch].hold;
            s.counter = (s.counter < hold) ? s.counter : hold;                 // update_settings(), :124
        }
        const float *xs = src + size_t(ch) * src_stride;
        float *ds = (dst != nullptr) ? dst + size_t(ch) * dst_stride : nullptr;

        auto load_tile = [&](uint32_t k)
        {
            const extent t = tile_extent(count, k);
            float x[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
            if ((vec & VEC_SRC) && c + 4 <= t.n)
            {
                const float4 q = *reinterpret_cast<const float4 *>(xs + t.t0 + c);
                x[0] = q.x, x[1] = q.y, x[2] = q.z, x[3] = q.w;
            }
            else
            {
                #pragma unroll
                for (uint32_t j = 0; j < 4; ++j)
                    if (c + j < t.n)
                        x[j] = xs[t.t0 + c + j];
            }
            *reinterpret_cast<float4 *>(&tile[k & 1][r][c]) = make_float4(fabsf(x[0]), fabsf(x[1]), fabsf(x[2]), fabsf(x[3]));
        };
        auto emit_tile = [&](uint32_t k)
        {
            const extent t = tile_extent(count, k);
            if (ds == nullptr || c >= t.n)
                return;
            const float4 v4 = *reinterpret_cast<const float4 *>(&tile[k & 1][r][c]);
            const float y[4] = { v4.x, v4.y, v4.z, v4.w };
            store_quad(ds + t.t0 + c, y, vec & VEC_DST, c, t.n);
        };

        MI_TILE_CHAIN_WALK(me, count, k, load_tile(k),
                           s = peakmeter_chain_tile((lds_float *)&tile[k & 1][r][0], tile_extent(count, k).n, s, tau, hold),
                           emit_tile(k));
        if (me.valid && me.chain)
        {
            state[ch] = s;
            if (peaks != nullptr)
                peaks[ch] = s.peak;
        }
    }

    // process(value, count), PeakMeter.cpp:185-205, of every channel; p.factor is expf(logf(fTau) * float(count)) for this count
    __global__ __launch_bounds__(VALUE_BLOCK) void peakmeter_value_kernel(float *peaks, const float *values, uint32_t count,
                                                                          uint32_t channels, const mi_peakmeter_params_t *params,
                                                                          device_state *state)
    {
        const uint32_t ch = blockIdx.x * VALUE_BLOCK + threadIdx.x;
        if (ch >= channels)
            return;
        const mi_peakmeter_params_t p = params[ch];
        device_state s = state[ch];
        s.counter = (s.counter < p.hold) ? s.counter : p.hold;                  // update_settings(), :124
        const float value = fabsf(values[ch]);
        if (value >= s.peak)
            s.peak = value, s.counter = p.hold;
        else if (s.counter >= count)
            s.counter -= count;
        else
        {
            const float decayed = s.peak * p.factor;
            s.peak = (decayed > value) ? decayed : value;                       // lsp_max: a NaN product gives `value`
        }
        state[ch] = s;
        if (peaks != nullptr)
            peaks[ch] = s.peak;
    }

    // millis_to_samples(nSampleRate, fHold) as update_settings() takes it (:122); the conversion to an integer is defined for
    // [0, 2^32) only
    bool hold_samples(uint32_t sample_rate, float hold, uint32_t *samples)
    {
        const float m = millis_to_samples(float(sample_rate), hold);
        if (!(m >= 0.0f && m < 4294967296.0f))
            return false;
        *samples = uint32_t(m);
        return true;
    }

    float value_factor(float tau, uint32_t count)
    {
        return expf(logf(tau) * float(count));                                  // :202
    }

    // update_settings(), :116-125, in host float32
    void compute_params(const settings &s, mi_peakmeter_params_t &p)
    {
        uint32_t hold = 0;
        (void)hold_samples(s.sample_rate, s.hold, &hold);                       // the setters refused what cannot be converted
        p.hold = hold;
        p.tau = expf(logf(1.0f - float(M_SQRT1_2)) / millis_to_samples(float(s.sample_rate), s.release));
        p.factor = value_factor(p.tau, p.count);
    }
} // namespace

struct mi_peakmeter_bank : mi_bank::settings_bank<settings, mi_peakmeter_params_t, device_state>
{
    static constexpr const char *NAME = "mi_peakmeter_bank";

    std::vector<uint8_t>    zero;                   // clear() was called for the channel
    bool                    work = false;           // ... for some channel

    static settings fresh_settings() { return settings{ 0, 5.0f, 0.0f }; }     // construct(), :40-50
    static mi_peakmeter_params_t fresh_params()
    {
        mi_peakmeter_params_t p = {};
        p.tau = 1.0f, p.factor = 1.0f;
        return p;
    }
    static device_state fresh_state() { return device_state{ 0.0f, 0 }; }
    static void compute(const settings &s, mi_peakmeter_params_t &p) { compute_params(s, p); }
};

namespace
{
    // what clear() left, then update_settings() of the flagged channels
    int pm_update(mi_peakmeter_bank *b, hipStream_t st)
    {
        if (b->work)
        {
            const int r = mi::refuse_capture(mi_peakmeter_bank::NAME, st);
            if (r != MI_OK)
                return r;
            for (uint32_t ch = 0; ch < b->channels; ++ch)
                if (b->zero[ch])
                {
                    MI_HIP_CHECK(hipMemsetAsync(b->d_state + ch, 0, sizeof(device_state), st));
                    b->zero[ch] = 0;
                }
            b->work = false;
        }
        return mi_bank::update(b, st);
    }

    // the setters' common end: the times as they would be set must give a hold that can be counted
    int pm_set(mi_peakmeter_bank *b, const char *entry, uint32_t channel, const settings &s)
    {
        uint32_t hold = 0;
        MI_REQUIRE(hold_samples(s.sample_rate, s.hold, &hold), MI_EINVAL,
                   "%s: a hold of %g ms at %u Hz is not a number of samples in [0, 2^32)", entry, double(s.hold), s.sample_rate);
        b->cfg[channel] = s;
        b->update[channel] = 1;
        return MI_OK;
    }
} // namespace

extern "C" {

int mi_peakmeter_compute_params(uint32_t sample_rate, float hold, float release, mi_peakmeter_params_t *params)   // :116-125
{
    MI_REQUIRE(params != nullptr, MI_EINVAL, "mi_peakmeter_compute_params: NULL argument");
    uint32_t samples = 0;
    MI_REQUIRE(hold_samples(sample_rate, hold, &samples), MI_EINVAL,
               "mi_peakmeter_compute_params: a hold of %g ms at %u Hz is not a number of samples in [0, 2^32)", double(hold), sample_rate);
    *params = mi_peakmeter_bank::fresh_params();
    compute_params(settings{ sample_rate, hold, release }, *params);
    return MI_OK;
}

int mi_peakmeter_bank_create(mi_peakmeter_bank_t **bank, uint32_t channels)                                  // :40-50
{
    const int r = mi_bank::create(bank, "mi_peakmeter_bank_create", channels);
    if (r == MI_OK)
        (*bank)->zero.assign(channels, 0);
    return r;
}

int mi_peakmeter_bank_destroy(mi_peakmeter_bank_t *b)
{
    return mi_bank::destroy(b);
}

int mi_peakmeter_bank_set_sample_rate(mi_peakmeter_bank_t *b, uint32_t channel, uint32_t sample_rate)        // :57-63
{
    MI_BANK_SETTER("peakmeter", "set_sample_rate");
    if (c.sample_rate == sample_rate)
        return MI_OK;
    return pm_set(b, "mi_peakmeter_bank_set_sample_rate", channel, settings{ sample_rate, c.hold, c.release });
}

int mi_peakmeter_bank_set_hold_time(mi_peakmeter_bank_t *b, uint32_t channel, float hold)                    // :70-76
{
    MI_BANK_SETTER("peakmeter", "set_hold_time");
    if (c.hold == hold)
        return MI_OK;
    return pm_set(b, "mi_peakmeter_bank_set_hold_time", channel, settings{ c.sample_rate, hold, c.release });
}

int mi_peakmeter_bank_set_release_time(mi_peakmeter_bank_t *b, uint32_t channel, float release)              // :83-89
{
    MI_BANK_SETTER("peakmeter", "set_release_time");
    if (c.release == release)
        return MI_OK;
    return pm_set(b, "mi_peakmeter_bank_set_release_time", channel, settings{ c.sample_rate, c.hold, release });
}

int mi_peakmeter_bank_set_time(mi_peakmeter_bank_t *b, uint32_t channel, float hold, float release)          // :96-103
{
    MI_BANK_SETTER("peakmeter", "set_time");
    if (c.hold == hold && c.release == release)
        return MI_OK;
    return pm_set(b, "mi_peakmeter_bank_set_time", channel, settings{ c.sample_rate, hold, release });
}

int mi_peakmeter_bank_clear(mi_peakmeter_bank_t *b, uint32_t channel)                                        // :110-114
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_peakmeter_bank_clear: NULL bank");
    MI_REQUIRE(channel < b->channels || channel == UINT32_MAX, MI_EINVAL, "mi_peakmeter_bank_clear: channel %u out of range", channel);
    for (uint32_t ch = 0; ch < b->channels; ++ch)
        if (channel == UINT32_MAX || ch == channel)
            b->zero[ch] = 1;
    b->work = true;
    return MI_OK;
}

int mi_peakmeter_bank_update_settings(mi_peakmeter_bank_t *b, void *stream)                                  // :116-125
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_peakmeter_bank_update_settings: NULL bank");
    return pm_update(b, mi::as_stream(stream));
}

int mi_peakmeter_bank_get_params(const mi_peakmeter_bank_t *b, uint32_t channel, mi_peakmeter_params_t *params)
{
    const int r = mi_bank::get_checks(b, "mi_peakmeter_bank_get_params", channel, params);
    if (r != MI_OK)
        return r;
    *params = b->params[channel];
    if (b->update[channel])                                     // as update_settings() will leave them
        compute_params(b->cfg[channel], *params);
    return MI_OK;
}

int mi_peakmeter_bank_set_params(mi_peakmeter_bank_t *b, uint32_t channel, const mi_peakmeter_params_t *params)
{
    const int r = mi_bank::set_params_checks(b, "mi_peakmeter_bank_set_params", channel, params);
    if (r != MI_OK)
        return r;
    mi_peakmeter_params_t p = *params;                          // tau and hold as given; the factor is the bank's own
    p.count = b->params[channel].count;
    p.factor = value_factor(p.tau, p.count);
    return mi_bank::set_params_store(b, channel, &p);
}

int mi_peakmeter_bank_get_state(mi_peakmeter_bank_t *b, uint32_t channel, mi_peakmeter_state_t *state, void *stream)
{
    device_state s;
    int r = mi_bank::get_checks(b, "mi_peakmeter_bank_get_state", channel, state);
    if (r == MI_OK)
        r = mi::refuse_state_access(mi::as_stream(stream));
    if (r == MI_OK)
        r = pm_update(b, mi::as_stream(stream));
    if (r == MI_OK)
        r = mi_bank::get_state(b, "mi_peakmeter_bank_get_state", channel, &s, stream);
    if (r != MI_OK)
        return r;
    state->peak = s.peak, state->counter = s.counter;
    return MI_OK;
}

int mi_peakmeter_bank_set_state(mi_peakmeter_bank_t *b, uint32_t channel, const mi_peakmeter_state_t *state, void *stream)
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_peakmeter_bank_set_state: NULL bank");
    MI_REQUIRE(state != nullptr, MI_EINVAL, "mi_peakmeter_bank_set_state: NULL state");
    MI_REQUIRE(channel < b->channels, MI_EINVAL, "mi_peakmeter_bank_set_state: channel %u out of range", channel);
    hipStream_t st = mi::as_stream(stream);
    int r = mi::refuse_state_access(st);
    if (r == MI_OK)
        r = pm_update(b, st);                                   // a clear() before this call does not undo it
    if (r != MI_OK)
        return r;
    return mi_bank::set_state(b, "mi_peakmeter_bank_set_state", channel, device_state{ state->peak, state->counter }, true, st);
}

int mi_peakmeter_bank_process(mi_peakmeter_bank_t *b, float *dst, const float *src, float *peaks, size_t count, size_t dst_stride,
                              size_t src_stride, void *stream)                                               // :127-183
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_peakmeter_bank_process: NULL bank");
    hipStream_t st = mi::as_stream(stream);
    const int r = pm_update(b, st);
    if (r != MI_OK || count == 0)
        return r;
    const int k = mi_bank::check_rows("mi_peakmeter_bank_process", b->channels, count, COUNT_LIMIT,
                                      { { dst, dst_stride, count, mi_bank::OUTPUT }, { src, src_stride, count, mi_bank::REQUIRED } });
    if (k != MI_OK)
        return k;
    const uint32_t vec = (mi::aligned16(dst, dst_stride, b->channels) ? VEC_DST : 0) | (mi::aligned16(src, src_stride, b->channels) ? VEC_SRC : 0);
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    mi::take_profile_events(&ev0, &ev1);
    MI_LAUNCH(peakmeter_kernel, dim3((b->channels + GROUP - 1) / GROUP), dim3(BLOCK), 0, st, ev0, ev1, dst, src, peaks, dst_stride,
              src_stride, uint32_t(count), b->channels, b->d_params, b->d_state, vec);
    MI_HIP_CHECK(hipGetLastError());
    return MI_OK;
}

int mi_peakmeter_bank_process_value(mi_peakmeter_bank_t *b, float *peaks, const float *values, size_t count, void *stream)   // :185-205
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_peakmeter_bank_process_value: NULL bank");
    MI_REQUIRE(values != nullptr, MI_EINVAL, "mi_peakmeter_bank_process_value: NULL buffer");
    MI_REQUIRE(count <= size_t(UINT32_MAX), MI_EINVAL, "mi_peakmeter_bank_process_value: count %zu too large", count);
    hipStream_t st = mi::as_stream(stream);
    for (uint32_t ch = 0; ch < b->channels; ++ch)
        if (b->params[ch].count != uint32_t(count))
        {
            b->params[ch].count = uint32_t(count);
            b->params[ch].factor = value_factor(b->params[ch].tau, uint32_t(count));    // again in compute() where tau changes
            b->up.touch(ch);
        }
    const int r = pm_update(b, st);
    if (r != MI_OK)
        return r;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    mi::take_profile_events(&ev0, &ev1);
    MI_LAUNCH(peakmeter_value_kernel, dim3((b->channels + VALUE_BLOCK - 1) / VALUE_BLOCK), dim3(VALUE_BLOCK), 0, st, ev0, ev1, peaks,
              values, uint32_t(count), b->channels, b->d_params, b->d_state);
    MI_HIP_CHECK(hipGetLastError());
    return MI_OK;
}

} // extern "C"
