// The host side of mi_autogain_bank and mi_simple_autogain_bank (kernels: autogain.hip): update() in host float32, the
// setters with the reference's rules, the parameter tables and the entries; and lsp::dspu::AutoGain and SimpleAutoGain
// (src/main/dynamics/AutoGain.cpp, SimpleAutoGain.cpp) on banks of one channel.  The classes have no member to hang a bank
// on (their 128 and 40 bytes are the reference's), so the bank and its staging buffer live in a table keyed by the object's
// address, as for Compressor: made at the first process() call, dropped in destroy() and in construct().  Before every
// device call the bank is handed the object's own computed fields, and the state where it is not what was read back after
// the previous call (the setters of SimpleAutoGain write fCurrGain; a subclass may write any of them).
#include <lsp-plug.in/dsp-units/dynamics/AutoGain.h>
#include <lsp-plug.in/dsp-units/dynamics/SimpleAutoGain.h>

#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#include "autogain_bank.h"
#include "beside.h"

#pragma clang fp contract(off)      // update() rounds every product and every sum on its own

namespace
{
    constexpr uint32_t SWITCHES = MI_AG_QUICK_AMP | MI_AG_MAX_GAIN;
    constexpr uint32_t SURGES   = MI_AG_SURGE_UP | MI_AG_SURGE_DOWN;

    // AutoGain::calc_compressor, AutoGain.cpp:180-195; c.a goes through double as the reference's expression does
    void calc_curve(mi_autogain_curve_t &c, float x1, float x2, float y2)
    {
        c.x1 = x1;
        c.x2 = x2;
        const float dy = y2 - c.x1;
        const float dx = c.x2 - c.x1;
        const float dx1 = 1.0f / dx;
        const float dx2 = dx1 * dx1;
        c.t = y2;
        c.d = c.x1;
        c.c = 1.0f;
        c.b = 3.0f * dy * dx2 - 2.0f * dx1;
        c.a = float((1.0f - 2.0 * dy * dx1) * dx2);
    }

    // AutoGain::update, :155-173
    void compute_params(const mi_autogain_settings_t &s, mi_autogain_params_t &p)
    {
        const float ksr = float((M_LN10 / 20.0f) / double(s.sample_rate));
        p.short_kgrow = expf(s.short_grow * ksr);
        p.short_kfall = expf(-s.short_fall * ksr);
        p.long_kgrow = expf(s.long_grow * ksr);
        p.long_kfall = expf(-s.long_fall * ksr);
        const float q = sqrtf(s.deviation);
        calc_curve(p.short_comp, 1.0f / s.deviation, s.deviation, 1.0f);
        calc_curve(p.out_comp, q, s.deviation * q, s.deviation);
        p.silence = s.silence;
        p.deviation = s.deviation;
        p.max_gain = s.max_gain;
        p.flags = s.flags & SWITCHES;
    }

    mi_autogain_settings_t fresh_settings()                     // construct(), :43-66
    {
        mi_autogain_settings_t s = {};
        s.silence = float(2.5119e-4);                           // GAIN_AMP_M_72_DB
        s.deviation = float(1.99526);                           // GAIN_AMP_P_6_DB
        s.max_gain = float(3.98107);                            // GAIN_AMP_P_12_DB
        return s;
    }

    mi_autogain_params_t fresh_params()                         // ... with init_compressor, :72-81
    {
        mi_autogain_params_t p = {};
        p.short_comp.x1 = p.short_comp.x2 = p.short_comp.t = 1.0f;
        p.out_comp = p.short_comp;
        const mi_autogain_settings_t s = fresh_settings();
        p.silence = s.silence, p.deviation = s.deviation, p.max_gain = s.max_gain;
        return p;
    }

    // SimpleAutoGain::update, SimpleAutoGain.cpp:142-153
    void compute_params(const mi_simple_autogain_settings_t &s, mi_simple_autogain_params_t &p)
    {
        const float ksr = float((M_LN10 * 0.05f) / double(s.sample_rate));
        p.kgrow = expf(s.grow * ksr);
        p.kfall = expf(-s.fall * ksr);
        p.threshold = s.threshold;
        p.min_gain = s.min_gain;
        p.max_gain = s.max_gain;
    }

    mi_simple_autogain_settings_t fresh_simple_settings()       // construct(), :43-56
    {
        mi_simple_autogain_settings_t s = {};
        s.min_gain = 0.000001f;
        s.max_gain = 1.0f;
        return s;
    }

    mi_simple_autogain_params_t fresh_simple_params()
    {
        mi_simple_autogain_params_t p = {};
        p.min_gain = 0.000001f;
        p.max_gain = 1.0f;
        return p;
    }
} // namespace

struct mi_autogain_bank
{
    uint32_t                                channels = 0;
    std::vector<mi_autogain_settings_t>     cfg;            // the setters' values
    std::vector<uint8_t>                    update;         // F_UPDATE of every channel
    std::vector<mi_autogain_params_t>       params;         // what update() computed, and the values that need no update()
    mi::dirty_range                         up;             // where params differs from the device table
    mi_autogain_params_t                   *d_params = nullptr;     // [channels]
    mi::autogain_state                     *d_state = nullptr;      // [channels]
};

struct mi_simple_autogain_bank
{
    struct recorded { uint32_t channel; mi::simple_autogain_op op; };
    uint32_t                                    channels = 0;
    std::vector<mi_simple_autogain_settings_t>  cfg;
    std::vector<uint8_t>                        update;
    std::vector<mi_simple_autogain_params_t>    params;
    mi::dirty_range                             up;
    std::vector<recorded>                       ops;        // the limits' changes since the last launch, in order
    mi_simple_autogain_params_t                *d_params = nullptr;     // [channels]
    float                                      *d_gain = nullptr;       // [channels]: fCurrGain
    mi::simple_autogain_pending                *d_pending = nullptr;    // [channels]
    mi::simple_autogain_op                     *d_ops = nullptr;        // [ops_cap], a channel's side by side
    size_t                                      ops_cap = 0;
};

namespace
{
    int ag_update(mi_autogain_bank *b, hipStream_t st)
    {
        for (uint32_t ch = 0; ch < b->channels; ++ch)
        {
            if (!b->update[ch])
                continue;
            compute_params(b->cfg[ch], b->params[ch]);
            b->update[ch] = 0;
            b->up.touch(ch);
        }
        return mi::upload_dirty("mi_autogain_bank", b->d_params, b->params.data(), b->up, st);
    }

    int sag_update(mi_simple_autogain_bank *b, hipStream_t st)
    {
        for (uint32_t ch = 0; ch < b->channels; ++ch)
        {
            if (!b->update[ch])
                continue;
            compute_params(b->cfg[ch], b->params[ch]);
            b->update[ch] = 0;
            b->up.touch(ch);
        }
        return mi::upload_dirty("mi_simple_autogain_bank", b->d_params, b->params.data(), b->up, st);
    }

    // the recorded changes of the limits go to the device, every channel's side by side and in their order
    int sag_send_ops(mi_simple_autogain_bank *b, hipStream_t st)
    {
        if (b->ops.empty())
            return MI_OK;
        const int r = mi::refuse_capture("mi_simple_autogain_bank", st);
        if (r != MI_OK)
            return r;
        const size_t n = b->ops.size();
        if (n > b->ops_cap)
        {
            (void)hipFree(b->d_ops);
            b->d_ops = nullptr;
            b->ops_cap = 0;
            MI_HIP_CHECK(hipMalloc(reinterpret_cast<void **>(&b->d_ops), 2 * n * sizeof(mi::simple_autogain_op)));
            b->ops_cap = 2 * n;
        }
        std::vector<mi::simple_autogain_pending> where(b->channels, mi::simple_autogain_pending{ 0, 0 });
        for (const auto &o : b->ops)
            ++where[o.channel].count;
        uint32_t first = 0;
        for (auto &w : where)
            w.first = first, first += w.count, w.count = 0;
        std::vector<mi::simple_autogain_op> sorted(n);
        for (const auto &o : b->ops)
            sorted[where[o.channel].first + where[o.channel].count++] = o.op;
        MI_HIP_CHECK(hipMemcpyAsync(b->d_ops, sorted.data(), n * sizeof(mi::simple_autogain_op), hipMemcpyHostToDevice, st));
        MI_HIP_CHECK(hipMemcpyAsync(b->d_pending, where.data(), where.size() * sizeof(mi::simple_autogain_pending), hipMemcpyHostToDevice, st));
        MI_HIP_CHECK(hipStreamSynchronize(st));                 // the host tables go away
        b->ops.clear();
        return MI_OK;
    }

    void sag_record(mi_simple_autogain_bank *b, uint32_t channel, uint32_t kind, float lo, float hi)
    {
        b->ops.push_back({ channel, mi::simple_autogain_op{ kind, lo, hi, 0 } });
    }

    bool same_or_apart(const void *out, size_t out_stride, const void *in, size_t in_stride)
    {
        return out != in || out_stride == in_stride;
    }
} // namespace

namespace mi
{
    int autogain_bank_set_params(mi_autogain_bank_t *b, uint32_t channel, const mi_autogain_params_t *p)
    {
        MI_REQUIRE(b != nullptr && p != nullptr && channel < b->channels, MI_EINVAL, "autogain_bank_set_params: bad argument");
        if (b->update[channel] == 0 && memcmp(&b->params[channel], p, sizeof(*p)) == 0)
            return MI_OK;
        b->params[channel] = *p;
        b->update[channel] = 0;
        b->up.touch(channel);
        return MI_OK;
    }

    int autogain_bank_set_state(mi_autogain_bank_t *b, uint32_t channel, float curr_gain, float out_gain, uint32_t surge, hipStream_t st)
    {
        MI_REQUIRE(b != nullptr && channel < b->channels, MI_EINVAL, "autogain_bank_set_state: bad argument");
        return mi::write_state(b->d_state + channel, autogain_state{ curr_gain, out_gain, surge & SURGES, 0 }, st);
    }

    int simple_autogain_bank_set_params(mi_simple_autogain_bank_t *b, uint32_t channel, const mi_simple_autogain_params_t *p)
    {
        MI_REQUIRE(b != nullptr && p != nullptr && channel < b->channels, MI_EINVAL, "simple_autogain_bank_set_params: bad argument");
        if (b->update[channel] == 0 && memcmp(&b->params[channel], p, sizeof(*p)) == 0)
            return MI_OK;
        b->params[channel] = *p;
        b->update[channel] = 0;
        b->up.touch(channel);
        return MI_OK;
    }

    // ... the gain as it stands: changes of the limits recorded for the channel before are dropped
    int simple_autogain_bank_set_state(mi_simple_autogain_bank_t *b, uint32_t channel, float curr_gain, hipStream_t st)
    {
        MI_REQUIRE(b != nullptr && channel < b->channels, MI_EINVAL, "simple_autogain_bank_set_state: bad argument");
        const int r = mi::write_state(b->d_gain + channel, curr_gain, st);
        if (r != MI_OK)
            return r;
        std::vector<mi_simple_autogain_bank::recorded> kept;
        for (const auto &o : b->ops)
            if (o.channel != channel)
                kept.push_back(o);
        b->ops.swap(kept);
        return MI_OK;
    }
}

extern "C" {

/* ---- AutoGain ------------------------------------------------------------------------------------------------------- */

int mi_autogain_compute_params(const mi_autogain_settings_t *settings, mi_autogain_params_t *params)
{
    MI_REQUIRE(settings != nullptr && params != nullptr, MI_EINVAL, "mi_autogain_compute_params: NULL argument");
    *params = fresh_params();
    compute_params(*settings, *params);
    return MI_OK;
}

int mi_autogain_bank_create(mi_autogain_bank_t **bank, uint32_t channels)                // AutoGain.cpp:43-66
{
    MI_REQUIRE(bank != nullptr, MI_EINVAL, "mi_autogain_bank_create: NULL result pointer");
    *bank = nullptr;
    MI_REQUIRE(channels > 0 && channels <= (1u << 20), MI_EINVAL, "mi_autogain_bank_create: channels must be 1 .. 1048576");
    MI_REQUIRE(mi_dspu_device_count() > 0, MI_ENODEV, "no HIP device available (there is no CPU fallback)");
    mi_autogain_bank *b = new (std::nothrow) mi_autogain_bank();
    MI_REQUIRE(b != nullptr, MI_ENOMEM, "mi_autogain_bank_create: out of host memory");
    b->channels = channels;
    b->cfg.assign(channels, fresh_settings());
    b->update.assign(channels, 1);
    b->params.assign(channels, fresh_params());
    const std::vector<mi::autogain_state> ones(channels, mi::autogain_state{ 1.0f, 1.0f, 0, 0 });
    hipError_t e = hipMalloc(reinterpret_cast<void **>(&b->d_params), size_t(channels) * sizeof(mi_autogain_params_t));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&b->d_state), size_t(channels) * sizeof(mi::autogain_state));
    if (e == hipSuccess) e = hipMemcpy(b->d_params, b->params.data(), size_t(channels) * sizeof(mi_autogain_params_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(b->d_state, ones.data(), size_t(channels) * sizeof(mi::autogain_state), hipMemcpyHostToDevice);
    if (e != hipSuccess)
    {
        mi_autogain_bank_destroy(b);
        return mi::fail(MI_EHIP, "mi_autogain_bank_create: %s", hipGetErrorString(e));
    }
    *bank = b;
    return MI_OK;
}

int mi_autogain_bank_destroy(mi_autogain_bank_t *b)
{
    if (b == nullptr)
        return MI_OK;
    (void)hipFree(b->d_params); (void)hipFree(b->d_state);
    delete b;
    return MI_OK;
}

int mi_autogain_bank_set_sample_rate(mi_autogain_bank_t *b, uint32_t channel, uint32_t sample_rate)          // :100-109
{
    MI_BANK_SETTER("autogain", "set_sample_rate");
    if (c.sample_rate == sample_rate)
        return MI_OK;
    c.sample_rate = sample_rate;
    b->update[channel] = 1;
    return MI_OK;
}

int mi_autogain_bank_set_silence_threshold(mi_autogain_bank_t *b, uint32_t channel, float threshold)         // :111-115
{
    MI_BANK_SETTER("autogain", "set_silence_threshold");
    c.silence = (0.0f > threshold) ? 0.0f : threshold;
    b->params[channel].silence = c.silence;
    b->up.touch(channel);
    return MI_OK;
}

int mi_autogain_bank_set_deviation(mi_autogain_bank_t *b, uint32_t channel, float deviation)                 // :117-125
{
    MI_BANK_SETTER("autogain", "set_deviation");
    deviation = (1.0f > deviation) ? 1.0f : deviation;
    if (deviation == c.deviation)
        return MI_OK;
    c.deviation = deviation;
    b->update[channel] = 1;
    return MI_OK;
}

} // extern "C"

namespace
{
    // AutoGain::set_timing, :90-98
    void set_timing(mi_autogain_bank *b, uint32_t channel, float &slot, float value)
    {
        value = (value > 0.0f) ? value : 0.0f;
        if (slot == value)
            return;
        slot = value;
        b->update[channel] = 1;
    }

    void set_switch(mi_autogain_bank *b, uint32_t channel, uint32_t flag, int enable)
    {
        uint32_t &f = b->cfg[channel].flags;
        f = enable ? (f | flag) : (f & ~flag);
        b->params[channel].flags = f & SWITCHES;
        b->up.touch(channel);
    }
}

extern "C" {

int mi_autogain_bank_set_short_grow(mi_autogain_bank_t *b, uint32_t channel, float value)
{
    MI_BANK_SETTER("autogain", "set_short_grow");
    set_timing(b, channel, c.short_grow, value);
    return MI_OK;
}

int mi_autogain_bank_set_short_fall(mi_autogain_bank_t *b, uint32_t channel, float value)
{
    MI_BANK_SETTER("autogain", "set_short_fall");
    set_timing(b, channel, c.short_fall, value);
    return MI_OK;
}

int mi_autogain_bank_set_short_speed(mi_autogain_bank_t *b, uint32_t channel, float grow, float fall)        // :127-131
{
    MI_BANK_SETTER("autogain", "set_short_speed");
    set_timing(b, channel, c.short_grow, grow);
    set_timing(b, channel, c.short_fall, fall);
    return MI_OK;
}

int mi_autogain_bank_set_long_grow(mi_autogain_bank_t *b, uint32_t channel, float value)
{
    MI_BANK_SETTER("autogain", "set_long_grow");
    set_timing(b, channel, c.long_grow, value);
    return MI_OK;
}

int mi_autogain_bank_set_long_fall(mi_autogain_bank_t *b, uint32_t channel, float value)
{
    MI_BANK_SETTER("autogain", "set_long_fall");
    set_timing(b, channel, c.long_fall, value);
    return MI_OK;
}

int mi_autogain_bank_set_long_speed(mi_autogain_bank_t *b, uint32_t channel, float grow, float fall)         // :133-137
{
    MI_BANK_SETTER("autogain", "set_long_speed");
    set_timing(b, channel, c.long_grow, grow);
    set_timing(b, channel, c.long_fall, fall);
    return MI_OK;
}

int mi_autogain_bank_set_max_gain(mi_autogain_bank_t *b, uint32_t channel, float value)                      // :145-148
{
    MI_BANK_SETTER("autogain", "set_max_gain");
    c.max_gain = (0.0f > value) ? 0.0f : value;
    b->params[channel].max_gain = c.max_gain;
    b->up.touch(channel);
    return MI_OK;
}

int mi_autogain_bank_set_max_gain_control(mi_autogain_bank_t *b, uint32_t channel, float value, int enable)  // :139-143
{
    MI_BANK_SETTER("autogain", "set_max_gain_control");
    c.max_gain = (0.0f > value) ? 0.0f : value;
    b->params[channel].max_gain = c.max_gain;
    set_switch(b, channel, MI_AG_MAX_GAIN, enable);
    return MI_OK;
}

int mi_autogain_bank_enable_max_gain(mi_autogain_bank_t *b, uint32_t channel, int enable)                    // :150-153
{
    MI_BANK_SETTER("autogain", "enable_max_gain");
    (void)c;
    set_switch(b, channel, MI_AG_MAX_GAIN, enable);
    return MI_OK;
}

int mi_autogain_bank_enable_quick_amplifier(mi_autogain_bank_t *b, uint32_t channel, int enable)             // :175-178
{
    MI_BANK_SETTER("autogain", "enable_quick_amplifier");
    (void)c;
    set_switch(b, channel, MI_AG_QUICK_AMP, enable);
    return MI_OK;
}

int mi_autogain_bank_update_settings(mi_autogain_bank_t *b, void *stream)                                    // :155-173
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_autogain_bank_update_settings: NULL bank");
    return ag_update(b, mi::as_stream(stream));
}

int mi_autogain_bank_get_params(const mi_autogain_bank_t *b, uint32_t channel, mi_autogain_params_t *params)
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_autogain_bank_get_params: NULL bank");
    MI_REQUIRE(channel < b->channels && params != nullptr, MI_EINVAL, "mi_autogain_bank_get_params: bad argument");
    *params = b->params[channel];
    return MI_OK;
}

int mi_autogain_bank_get_state(mi_autogain_bank_t *b, uint32_t channel, float *curr_gain, float *out_gain, uint32_t *flags,
                               void *stream)
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_autogain_bank_get_state: NULL bank");
    MI_REQUIRE(channel < b->channels, MI_EINVAL, "mi_autogain_bank_get_state: channel %u out of range", channel);
    mi::autogain_state s;
    const int r = mi::read_state(&s, b->d_state + channel, mi::as_stream(stream));
    if (r != MI_OK)
        return r;
    if (curr_gain != nullptr) *curr_gain = s.gain;
    if (out_gain != nullptr) *out_gain = s.out;
    if (flags != nullptr) *flags = (b->params[channel].flags & SWITCHES) | (s.surge & SURGES);
    return MI_OK;
}

} // extern "C"

namespace
{
    // the checks and the launch of the three process entries.  level: lexp is one float per channel
    int ag_process(mi_autogain_bank *b, const char *who, float *vca, const float *audio, const float *llong, const float *lshort,
                   const float *lexp, bool level, size_t count, size_t vca_stride, size_t audio_stride, size_t long_stride,
                   size_t short_stride, size_t exp_stride, bool with_audio, hipStream_t st)
    {
        const int r = ag_update(b, st);
        if (r != MI_OK || count == 0)
            return r;
        MI_REQUIRE(vca != nullptr && llong != nullptr && lshort != nullptr && lexp != nullptr && (!with_audio || audio != nullptr),
                   MI_EINVAL, "%s: NULL buffer", who);
        MI_REQUIRE(count < (size_t(1) << 31), MI_EINVAL, "%s: count %zu too large", who, count);
        MI_REQUIRE(b->channels == 1 || (vca_stride >= count && long_stride >= count && short_stride >= count &&
                                        (level || exp_stride >= count) && (!with_audio || audio_stride >= count)),
                   MI_EINVAL, "%s: a stride is shorter than count %zu", who, count);
        MI_REQUIRE(same_or_apart(vca, vca_stride, llong, long_stride) && same_or_apart(vca, vca_stride, lshort, short_stride) &&
                   (level || same_or_apart(vca, vca_stride, lexp, exp_stride)) &&
                   (!with_audio || same_or_apart(vca, vca_stride, audio, audio_stride)),
                   MI_EINVAL, "%s: in place with different strides", who);
        MI_REQUIRE(!level || static_cast<const void *>(lexp) != static_cast<const void *>(vca), MI_EINVAL,
                   "%s: the levels are the output buffer", who);
        return mi::autogain_launch(vca, llong, lshort, lexp, level, with_audio ? audio : nullptr, vca_stride, long_stride, short_stride,
                                   level ? 0 : exp_stride, with_audio ? audio_stride : 0, uint32_t(count), b->channels, b->d_params,
                                   b->d_state, st);
    }
}

extern "C" {

int mi_autogain_bank_process(mi_autogain_bank_t *b, float *vca, const float *llong, const float *lshort, const float *lexp,
                             size_t count, size_t vca_stride, size_t long_stride, size_t short_stride, size_t exp_stride,
                             void *stream)                                                                   // :278-286
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_autogain_bank_process: NULL bank");
    return ag_process(b, "mi_autogain_bank_process", vca, nullptr, llong, lshort, lexp, false, count, vca_stride, 0, long_stride,
                      short_stride, exp_stride, false, mi::as_stream(stream));
}

int mi_autogain_bank_process_level(mi_autogain_bank_t *b, float *vca, const float *llong, const float *lshort, const float *levels,
                                   size_t count, size_t vca_stride, size_t long_stride, size_t short_stride, void *stream)   // :288-296
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_autogain_bank_process_level: NULL bank");
    return ag_process(b, "mi_autogain_bank_process_level", vca, nullptr, llong, lshort, levels, true, count, vca_stride, 0, long_stride,
                      short_stride, 0, false, mi::as_stream(stream));
}

int mi_autogain_bank_process_apply(mi_autogain_bank_t *b, float *dst, const float *audio, const float *llong, const float *lshort,
                                   const float *lexp, size_t count, size_t dst_stride, size_t audio_stride, size_t long_stride,
                                   size_t short_stride, size_t exp_stride, void *stream)
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_autogain_bank_process_apply: NULL bank");
    return ag_process(b, "mi_autogain_bank_process_apply", dst, audio, llong, lshort, lexp, false, count, dst_stride, audio_stride,
                      long_stride, short_stride, exp_stride, true, mi::as_stream(stream));
}

/* ---- SimpleAutoGain ------------------------------------------------------------------------------------------------- */

int mi_simple_autogain_compute_params(const mi_simple_autogain_settings_t *settings, mi_simple_autogain_params_t *params)
{
    MI_REQUIRE(settings != nullptr && params != nullptr, MI_EINVAL, "mi_simple_autogain_compute_params: NULL argument");
    compute_params(*settings, *params);
    return MI_OK;
}

int mi_simple_autogain_bank_create(mi_simple_autogain_bank_t **bank, uint32_t channels)   // SimpleAutoGain.cpp:43-56
{
    MI_REQUIRE(bank != nullptr, MI_EINVAL, "mi_simple_autogain_bank_create: NULL result pointer");
    *bank = nullptr;
    MI_REQUIRE(channels > 0 && channels <= (1u << 20), MI_EINVAL, "mi_simple_autogain_bank_create: channels must be 1 .. 1048576");
    MI_REQUIRE(mi_dspu_device_count() > 0, MI_ENODEV, "no HIP device available (there is no CPU fallback)");
    mi_simple_autogain_bank *b = new (std::nothrow) mi_simple_autogain_bank();
    MI_REQUIRE(b != nullptr, MI_ENOMEM, "mi_simple_autogain_bank_create: out of host memory");
    b->channels = channels;
    b->cfg.assign(channels, fresh_simple_settings());
    b->update.assign(channels, 1);
    b->params.assign(channels, fresh_simple_params());
    const std::vector<float> ones(channels, 1.0f);
    hipError_t e = hipMalloc(reinterpret_cast<void **>(&b->d_params), size_t(channels) * sizeof(mi_simple_autogain_params_t));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&b->d_gain), size_t(channels) * sizeof(float));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&b->d_pending), size_t(channels) * sizeof(mi::simple_autogain_pending));
    if (e == hipSuccess) e = hipMemcpy(b->d_params, b->params.data(), size_t(channels) * sizeof(mi_simple_autogain_params_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(b->d_gain, ones.data(), size_t(channels) * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(b->d_pending, 0, size_t(channels) * sizeof(mi::simple_autogain_pending));
    if (e == hipSuccess) e = hipDeviceSynchronize();            // the memset, whatever stream the first call comes on
    if (e != hipSuccess)
    {
        mi_simple_autogain_bank_destroy(b);
        return mi::fail(MI_EHIP, "mi_simple_autogain_bank_create: %s", hipGetErrorString(e));
    }
    *bank = b;
    return MI_OK;
}

int mi_simple_autogain_bank_destroy(mi_simple_autogain_bank_t *b)
{
    if (b == nullptr)
        return MI_OK;
    (void)hipFree(b->d_params); (void)hipFree(b->d_gain); (void)hipFree(b->d_pending); (void)hipFree(b->d_ops);
    delete b;
    return MI_OK;
}

int mi_simple_autogain_bank_set_sample_rate(mi_simple_autogain_bank_t *b, uint32_t channel, uint32_t sample_rate)     // :68-77
{
    MI_BANK_SETTER("simple_autogain", "set_sample_rate");
    if (c.sample_rate == sample_rate)
        return MI_OK;
    c.sample_rate = sample_rate;
    b->update[channel] = 1;
    return MI_OK;
}

int mi_simple_autogain_bank_set_grow(mi_simple_autogain_bank_t *b, uint32_t channel, float value)             // :79-86
{
    MI_BANK_SETTER("simple_autogain", "set_grow");
    if (c.grow == value)
        return MI_OK;
    c.grow = value;
    b->update[channel] = 1;
    return MI_OK;
}

int mi_simple_autogain_bank_set_fall(mi_simple_autogain_bank_t *b, uint32_t channel, float value)             // :88-95
{
    MI_BANK_SETTER("simple_autogain", "set_fall");
    if (c.fall == value)
        return MI_OK;
    c.fall = value;
    b->update[channel] = 1;
    return MI_OK;
}

int mi_simple_autogain_bank_set_speed(mi_simple_autogain_bank_t *b, uint32_t channel, float grow, float fall) // :97-106
{
    MI_BANK_SETTER("simple_autogain", "set_speed");
    if (c.grow == grow && c.fall == fall)
        return MI_OK;
    c.grow = grow, c.fall = fall;
    b->update[channel] = 1;
    return MI_OK;
}

int mi_simple_autogain_bank_set_max_gain(mi_simple_autogain_bank_t *b, uint32_t channel, float value)         // :108-115
{
    MI_BANK_SETTER("simple_autogain", "set_max_gain");
    if (c.max_gain == value)
        return MI_OK;
    c.max_gain = value;
    b->params[channel].max_gain = value;
    b->up.touch(channel);
    sag_record(b, channel, mi::SAG_MIN, 0.0f, value);
    return MI_OK;
}

int mi_simple_autogain_bank_set_min_gain(mi_simple_autogain_bank_t *b, uint32_t channel, float value)         // :117-124
{
    MI_BANK_SETTER("simple_autogain", "set_min_gain");
    if (c.min_gain == value)
        return MI_OK;
    c.min_gain = value;
    b->params[channel].min_gain = value;
    b->up.touch(channel);
    sag_record(b, channel, mi::SAG_MAX, value, 0.0f);
    return MI_OK;
}

int mi_simple_autogain_bank_set_gain(mi_simple_autogain_bank_t *b, uint32_t channel, float min, float max)    // :126-135
{
    MI_BANK_SETTER("simple_autogain", "set_gain");
    if (c.min_gain == min && c.max_gain == max)
        return MI_OK;
    c.min_gain = min, c.max_gain = max;
    b->params[channel].min_gain = min, b->params[channel].max_gain = max;
    b->up.touch(channel);
    sag_record(b, channel, mi::SAG_LIMIT, min, max);
    return MI_OK;
}

int mi_simple_autogain_bank_set_threshold(mi_simple_autogain_bank_t *b, uint32_t channel, float threshold)    // :137-140
{
    MI_BANK_SETTER("simple_autogain", "set_threshold");
    c.threshold = threshold;
    b->params[channel].threshold = threshold;
    b->up.touch(channel);
    return MI_OK;
}

int mi_simple_autogain_bank_update_settings(mi_simple_autogain_bank_t *b, void *stream)                       // :142-153
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_simple_autogain_bank_update_settings: NULL bank");
    return sag_update(b, mi::as_stream(stream));
}

int mi_simple_autogain_bank_get_params(const mi_simple_autogain_bank_t *b, uint32_t channel, mi_simple_autogain_params_t *params)
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_simple_autogain_bank_get_params: NULL bank");
    MI_REQUIRE(channel < b->channels && params != nullptr, MI_EINVAL, "mi_simple_autogain_bank_get_params: bad argument");
    *params = b->params[channel];
    return MI_OK;
}

int mi_simple_autogain_bank_get_state(mi_simple_autogain_bank_t *b, uint32_t channel, float *curr_gain, void *stream)
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_simple_autogain_bank_get_state: NULL bank");
    MI_REQUIRE(channel < b->channels, MI_EINVAL, "mi_simple_autogain_bank_get_state: channel %u out of range", channel);
    float g = 0.0f;
    const int r = mi::read_state(&g, b->d_gain + channel, mi::as_stream(stream));
    if (r != MI_OK)
        return r;
    for (const auto &o : b->ops)                                // what the next launch will do first
        if (o.channel == channel)
            g = mi::simple_autogain_apply(g, o.op);
    if (curr_gain != nullptr) *curr_gain = g;
    return MI_OK;
}

int mi_simple_autogain_bank_process(mi_simple_autogain_bank_t *b, float *dst, const float *src, size_t count, size_t dst_stride,
                                    size_t src_stride, void *stream)                                          // :155-175
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_simple_autogain_bank_process: NULL bank");
    hipStream_t st = mi::as_stream(stream);
    const int r = sag_update(b, st);
    if (r != MI_OK || count == 0)
        return r;
    MI_REQUIRE(dst != nullptr && src != nullptr, MI_EINVAL, "mi_simple_autogain_bank_process: NULL buffer");
    MI_REQUIRE(count < (size_t(1) << 31), MI_EINVAL, "mi_simple_autogain_bank_process: count %zu too large", count);
    MI_REQUIRE(b->channels == 1 || (dst_stride >= count && src_stride >= count), MI_EINVAL,
               "mi_simple_autogain_bank_process: strides (%zu, %zu) shorter than count %zu", dst_stride, src_stride, count);
    MI_REQUIRE(same_or_apart(dst, dst_stride, src, src_stride), MI_EINVAL, "mi_simple_autogain_bank_process: in place with different strides");
    const int s = sag_send_ops(b, st);
    if (s != MI_OK)
        return s;
    return mi::simple_autogain_launch(dst, src, dst_stride, src_stride, uint32_t(count), b->channels, b->d_params, b->d_gain,
                                      b->d_pending, b->d_ops, st);
}

} // extern "C"

/* ---- the classes ------------------------------------------------------------------------------------------------------ */

namespace lsp
{
namespace dspu
{
namespace
{
    // the state as the device holds it, beside the object (beside.h)
    struct autogain_held { float gain = 1.0f, out = 1.0f; uint32_t surge = 0; };
    struct simple_held { float gain = 1.0f; };
    typedef mi_host::registry<mi_autogain_bank_t, autogain_held, mi_autogain_bank_create, mi_autogain_bank_destroy> autogains;
    typedef mi_host::registry<mi_simple_autogain_bank_t, simple_held, mi_simple_autogain_bank_create, mi_simple_autogain_bank_destroy> simples;

    int send_autogain_state(mi_autogain_bank_t *bank, const autogain_held &s)
    {
        return mi::autogain_bank_set_state(bank, 0, s.gain, s.out, s.surge, nullptr);
    }
    int send_simple_state(mi_simple_autogain_bank_t *bank, const simple_held &s)
    {
        return mi::simple_autogain_bank_set_state(bank, 0, s.gain, nullptr);
    }
}

AutoGain::AutoGain()  { construct(); }
AutoGain::~AutoGain() { destroy(); }

void AutoGain::construct()                                      // AutoGain.cpp:43-66
{
    autogains::drop(this);                                      // whatever lived at this address before
    nSampleRate = 0;
    sShort.fGrow = sShort.fFall = sShort.fKGrow = sShort.fKFall = 0.0f;
    sLong.fGrow = sLong.fFall = sLong.fKGrow = sLong.fKFall = 0.0f;
    init_compressor(sShortComp);
    init_compressor(sOutComp);
    fSilence = float(2.5119e-4);                                // GAIN_AMP_M_72_DB
    fDeviation = float(1.99526);                                // GAIN_AMP_P_6_DB
    fCurrGain = 1.0f;
    fMaxGain = float(3.98107);                                  // GAIN_AMP_P_12_DB
    fOutGain = 1.0f;
    nFlags = F_UPDATE;
}

void AutoGain::destroy()                                        // :68-70
{
    autogains::drop(this);
}

void AutoGain::init_compressor(compressor_t &c)                 // :72-81
{
    c.x1 = 1.0f;
    c.x2 = 1.0f;
    c.t = 1.0f;
    c.a = c.b = c.c = c.d = 0.0f;
}

status_t AutoGain::init()                                       // :83-88
{
    destroy();
    return STATUS_OK;
}

void AutoGain::set_timing(float *ptr, float value)              // :90-98
{
    value = (value > 0.0f) ? value : 0.0f;
    if (*ptr == value)
        return;
    *ptr = value;
    nFlags |= F_UPDATE;
}

status_t AutoGain::set_sample_rate(size_t sample_rate)          // :100-109
{
    if (nSampleRate == sample_rate)
        return STATUS_OK;
    nSampleRate = sample_rate;
    nFlags |= F_UPDATE;
    return STATUS_OK;
}

void AutoGain::set_silence_threshold(float threshold)           // :111-115
{
    fSilence = (0.0f > threshold) ? 0.0f : threshold;
}

void AutoGain::set_deviation(float deviation)                   // :117-125
{
    deviation = (1.0f > deviation) ? 1.0f : deviation;
    if (deviation == fDeviation)
        return;
    fDeviation = deviation;
    nFlags |= F_UPDATE;
}

void AutoGain::set_short_speed(float grow, float fall)          // :127-131
{
    set_timing(&sShort.fGrow, grow);
    set_timing(&sShort.fFall, fall);
}

void AutoGain::set_long_speed(float grow, float fall)           // :133-137
{
    set_timing(&sLong.fGrow, grow);
    set_timing(&sLong.fFall, fall);
}

void AutoGain::set_max_gain(float value, bool enable)           // :139-143
{
    fMaxGain = (0.0f > value) ? 0.0f : value;
    nFlags = enable ? (nFlags | F_MAX_GAIN) : (nFlags & ~size_t(F_MAX_GAIN));
}

void AutoGain::set_max_gain(float value)                        // :145-148
{
    fMaxGain = (0.0f > value) ? 0.0f : value;
}

void AutoGain::enable_max_gain(bool enable)                     // :150-153
{
    nFlags = enable ? (nFlags | F_MAX_GAIN) : (nFlags & ~size_t(F_MAX_GAIN));
}

void AutoGain::enable_quick_amplifier(bool enable)              // :175-178
{
    nFlags = enable ? (nFlags | F_QUICK_AMP) : (nFlags & ~size_t(F_QUICK_AMP));
}

void AutoGain::update()                                         // :155-173
{
    if (!(nFlags & F_UPDATE))
        return;
    mi_autogain_settings_t s = {};
    s.sample_rate = uint32_t(nSampleRate);
    s.short_grow = sShort.fGrow, s.short_fall = sShort.fFall, s.long_grow = sLong.fGrow, s.long_fall = sLong.fFall;
    s.silence = fSilence, s.deviation = fDeviation, s.max_gain = fMaxGain;
    mi_autogain_params_t p;
    mi_autogain_compute_params(&s, &p);
    sShort.fKGrow = p.short_kgrow, sShort.fKFall = p.short_kfall;
    sLong.fKGrow = p.long_kgrow, sLong.fKFall = p.long_kfall;
    static_assert(sizeof(sShortComp) == sizeof(p.short_comp), "curve layouts");
    memcpy(&sShortComp, &p.short_comp, sizeof(sShortComp));
    memcpy(&sOutComp, &p.out_comp, sizeof(sOutComp));
    nFlags &= ~size_t(F_UPDATE);
}

// both process() overloads: the rows go to the device side by side, the gain comes back from the first of them
void AutoGain::run(float *vca, const float *llong, const float *lshort, const float *lexp, float level, size_t count)
{
    update();
    autogains::entry *p = autogains::of(this);
    if (p == nullptr || count == 0 || !p->reserve(count, 3))
        return;
    mi_autogain_params_t q;
    q.short_kgrow = sShort.fKGrow, q.short_kfall = sShort.fKFall, q.long_kgrow = sLong.fKGrow, q.long_kfall = sLong.fKFall;
    memcpy(&q.short_comp, &sShortComp, sizeof(q.short_comp));
    memcpy(&q.out_comp, &sOutComp, sizeof(q.out_comp));
    q.silence = fSilence, q.deviation = fDeviation, q.max_gain = fMaxGain;
    q.flags = uint32_t(nFlags) & (MI_AG_QUICK_AMP | MI_AG_MAX_GAIN);
    if (mi::autogain_bank_set_params(p->bank, 0, &q) != MI_OK)
        return;
    const uint32_t surge = uint32_t(nFlags) & (MI_AG_SURGE_UP | MI_AG_SURGE_DOWN);
    if (!p->hand_over_state({ fCurrGain, fOutGain, surge }, send_autogain_state))
        return;
    float *d_long = p->d_buf, *d_short = d_long + p->cap, *d_exp = d_short + p->cap;
    const size_t bytes = count * sizeof(float);
    if (mi_dspu_copy_h2d(d_long, llong, bytes, nullptr) != MI_OK || mi_dspu_copy_h2d(d_short, lshort, bytes, nullptr) != MI_OK)
        return;
    if (lexp != nullptr)
    {
        if (mi_dspu_copy_h2d(d_exp, lexp, bytes, nullptr) != MI_OK ||
            mi_autogain_bank_process(p->bank, d_long, d_long, d_short, d_exp, count, count, count, count, count, nullptr) != MI_OK)
            return;
    }
    else if (mi_dspu_copy_h2d(d_exp, &level, sizeof(float), nullptr) != MI_OK ||
             mi_autogain_bank_process_level(p->bank, d_long, d_long, d_short, d_exp, count, count, count, count, nullptr) != MI_OK)
        return;
    if (mi_dspu_copy_d2h(vca, d_long, bytes, nullptr) != MI_OK)
        return;
    uint32_t flags = 0;
    if (mi_autogain_bank_get_state(p->bank, 0, &p->held.gain, &p->held.out, &flags, nullptr) != MI_OK)
        return;
    p->held.surge = flags & (MI_AG_SURGE_UP | MI_AG_SURGE_DOWN);
    fCurrGain = p->held.gain, fOutGain = p->held.out;
    nFlags = (nFlags & ~size_t(F_SURGE_UP | F_SURGE_DOWN)) | p->held.surge;
}

void AutoGain::process(float *vca, const float *llong, const float *lshort, const float *lexp, size_t count)   // :278-286
{
    run(vca, llong, lshort, lexp, 0.0f, count);
}

void AutoGain::process(float *vca, const float *llong, const float *lshort, float lexp, size_t count)          // :288-296
{
    run(vca, llong, lshort, nullptr, lexp, count);
}

void AutoGain::dump(const char *id, const timing_t *t, IStateDumper *v)         // :298-308
{
    v->begin_object(id, t, sizeof(timing_t));
    v->write("fGrow", t->fGrow);
    v->write("fFall", t->fFall);
    v->write("fKGrow", t->fKGrow);
    v->write("fKFall", t->fKFall);
    v->end_object();
}

void AutoGain::dump(const char *id, const compressor_t *c, IStateDumper *v)     // :310-323
{
    v->begin_object(id, c, sizeof(compressor_t));
    v->write("x1", c->x1);
    v->write("x2", c->x2);
    v->write("t", c->t);
    v->write("a", c->a);
    v->write("b", c->b);
    v->write("c", c->c);
    v->write("d", c->d);
    v->end_object();
}

void AutoGain::dump(IStateDumper *v) const                      // :325-339 (fMaxGain is not written there either)
{
    v->write("nSampleRate", nSampleRate);
    v->write("nFlags", nFlags);
    dump("sShort", &sShort, v);
    dump("sLong", &sLong, v);
    dump("sShortComp", &sShortComp, v);
    dump("sOutComp", &sOutComp, v);
    v->write("fSilence", fSilence);
    v->write("fDeviation", fDeviation);
    v->write("fCurrGain", fCurrGain);
    v->write("fOutGain", fOutGain);
}

SimpleAutoGain::SimpleAutoGain()  { construct(); }
SimpleAutoGain::~SimpleAutoGain() { destroy(); }

void SimpleAutoGain::construct()                                // SimpleAutoGain.cpp:43-56
{
    simples::drop(this);
    nSampleRate = 0;
    nFlags = F_UPDATE;
    fKGrow = 0.0f;
    fKFall = 0.0f;
    fGrow = 0.0f;
    fFall = 0.0f;
    fThreshold = 0.0f;
    fCurrGain = 1.0f;
    fMinGain = 0.000001f;
    fMaxGain = 1.0f;
}

void SimpleAutoGain::destroy()                                  // :58-60
{
    simples::drop(this);
}

status_t SimpleAutoGain::init()                                 // :62-66
{
    destroy();
    return STATUS_OK;
}

status_t SimpleAutoGain::set_sample_rate(size_t sample_rate)    // :68-77
{
    if (nSampleRate == sample_rate)
        return STATUS_OK;
    nSampleRate = uint32_t(sample_rate);
    nFlags |= F_UPDATE;
    return STATUS_OK;
}

void SimpleAutoGain::set_grow(float value)                      // :79-86
{
    if (fGrow == value)
        return;
    fGrow = value;
    nFlags |= F_UPDATE;
}

void SimpleAutoGain::set_fall(float value)                      // :88-95
{
    if (fFall == value)
        return;
    fFall = value;
    nFlags |= F_UPDATE;
}

void SimpleAutoGain::set_speed(float grow, float fall)          // :97-106
{
    if ((fGrow == grow) && (fFall == fall))
        return;
    fGrow = grow;
    fFall = fall;
    nFlags |= F_UPDATE;
}

void SimpleAutoGain::set_max_gain(float value)                  // :108-115
{
    if (fMaxGain == value)
        return;
    fMaxGain = value;
    fCurrGain = (fCurrGain < fMaxGain) ? fCurrGain : fMaxGain;           // lsp_min
}

void SimpleAutoGain::set_min_gain(float value)                  // :117-124
{
    if (fMinGain == value)
        return;
    fMinGain = value;
    fCurrGain = (fCurrGain > fMinGain) ? fCurrGain : fMinGain;           // lsp_max
}

void SimpleAutoGain::set_gain(float min, float max)             // :126-135
{
    if ((fMinGain == min) && (fMaxGain == max))
        return;
    fMinGain = min;
    fMaxGain = max;
    fCurrGain = gain();                                         // lsp_limit
}

void SimpleAutoGain::set_threshold(float threshold)             // :137-140
{
    fThreshold = threshold;
}

void SimpleAutoGain::update()                                   // :142-153
{
    if (!(nFlags & F_UPDATE))
        return;
    mi_simple_autogain_settings_t s = { nSampleRate, fGrow, fFall, fThreshold, fMinGain, fMaxGain };
    mi_simple_autogain_params_t p;
    mi_simple_autogain_compute_params(&s, &p);
    fKGrow = p.kgrow;
    fKFall = p.kfall;
    nFlags &= ~uint32_t(F_UPDATE);
}

void SimpleAutoGain::process(float *dst, const float *src, size_t count)        // :155-175
{
    update();
    simples::entry *p = simples::of(this);
    if (p == nullptr || count == 0 || !p->reserve(count, 1))
        return;
    const mi_simple_autogain_params_t q = { fKGrow, fKFall, fThreshold, fMinGain, fMaxGain };
    if (mi::simple_autogain_bank_set_params(p->bank, 0, &q) != MI_OK)
        return;
    if (!p->hand_over_state({ fCurrGain }, send_simple_state))
        return;
    if (mi_dspu_copy_h2d(p->d_buf, src, count * sizeof(float), nullptr) != MI_OK ||
        mi_simple_autogain_bank_process(p->bank, p->d_buf, p->d_buf, count, count, count, nullptr) != MI_OK ||
        mi_dspu_copy_d2h(dst, p->d_buf, count * sizeof(float), nullptr) != MI_OK ||
        mi_simple_autogain_bank_get_state(p->bank, 0, &p->held.gain, nullptr) != MI_OK)
        return;
    fCurrGain = p->held.gain;
}

float SimpleAutoGain::process(float src)                        // :177-194: one sample on the device
{
    float out = 0.0f;
    process(&out, &src, 1);
    return out;
}

void SimpleAutoGain::dump(IStateDumper *v) const                // :196-209
{
    v->write("nSampleRate", nSampleRate);
    v->write("nFlags", nFlags);
    v->write("fKGrow", fKGrow);
    v->write("fKFall", fKFall);
    v->write("fGrow", fGrow);
    v->write("fFall", fFall);
    v->write("fThreshold", fThreshold);
    v->write("fCurrGain", fCurrGain);
    v->write("fMinGain", fMinGain);
    v->write("fMaxGain", fMaxGain);
}

} // namespace dspu
} // namespace lsp
