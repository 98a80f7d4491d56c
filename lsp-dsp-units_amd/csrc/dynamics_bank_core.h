// The host side that the Compressor, Expander, Gate and DynamicProcessor banks share: the fields, update_settings over the
// dirty channels, the parameter and state hand-overs, create / destroy / clear, the argument checks of process(),
// process_apply() and curve(), and the launch of the bank's kernel.  Every error text starts with the name of the C entry that
// reports it, so the entries pass their names in.
//
// A bank is  struct mi_<x>_bank : mi_dynamics::bank<settings, params, device state>  with, as static members, what is its own:
//     NAME                                 "mi_<x>_bank", as upload_dirty's messages have it
//     fresh_settings(), fresh_params()     a channel as construct() leaves it
//     compute(settings, params)            update_settings of one channel
//     launch(grid, st, ev0, ev1, args...)  MI_LAUNCH of its kernel, follow_kernel's arguments
#pragma once
#include "dynamics_device.h"

#include <new>
#include <vector>

namespace mi_dynamics
{
    template <class Settings, class Params, class State> struct bank
    {
        uint32_t                channels = 0;
        std::vector<Settings>   cfg;                    // the setters' values
        std::vector<uint8_t>    update;                 // bUpdate of every channel
        std::vector<Params>     params;                 // what update_settings computed
        mi::dirty_range         up;                     // where params differs from the device table
        Params                 *d_params = nullptr;     // [channels]
        State                  *d_state = nullptr;      // [channels]
    };

    // update_settings of every channel whose bUpdate is set; the changed stretch of the table goes to the device
    template <class Bank> int update(Bank *b, hipStream_t st)
    {
        for (uint32_t ch = 0; ch < b->channels; ++ch)
        {
            if (!b->update[ch])
                continue;
            Bank::compute(b->cfg[ch], b->params[ch]);
            b->update[ch] = 0;
            b->up.touch(ch);
        }
        return mi::upload_dirty(Bank::NAME, b->d_params, b->params.data(), b->up, st);
    }

    template <class Bank> int update_settings(Bank *b, const char *entry, void *stream)
    {
        MI_REQUIRE(b != nullptr, MI_ESTATE, "%s: NULL bank", entry);
        return update(b, mi::as_stream(stream));
    }

    // The computed parameters of one channel, set as they stand.  In two halves, so that a bank can check more of *p between them.
    template <class Bank, class Params> int set_params_checks(Bank *b, const char *entry, uint32_t channel, const Params *p)
    {
        MI_REQUIRE(b != nullptr && p != nullptr && channel < b->channels, MI_EINVAL, "%s: bad argument", entry);
        return MI_OK;
    }
    template <class Bank, class Params> int set_params_store(Bank *b, uint32_t channel, const Params *p)
    {
        if (b->update[channel] == 0 && memcmp(&b->params[channel], p, sizeof(*p)) == 0)
            return MI_OK;
        b->params[channel] = *p;
        b->update[channel] = 0;
        b->up.touch(channel);
        return MI_OK;
    }
    template <class Bank, class Params> int set_params(Bank *b, const char *entry, uint32_t channel, const Params *p)
    {
        const int r = set_params_checks(b, entry, channel, p);
        return (r != MI_OK) ? r : set_params_store(b, channel, p);
    }

    template <class Bank, class Params> int get_params(const Bank *b, const char *entry, uint32_t channel, Params *params)
    {
        MI_REQUIRE(b != nullptr, MI_ESTATE, "%s: NULL bank", entry);
        MI_REQUIRE(channel < b->channels && params != nullptr, MI_EINVAL, "%s: bad argument", entry);
        *params = b->params[channel];
        return MI_OK;
    }

    // one channel's device state, from and to the host (`valid`: what the bank asks of the values it is given)
    template <class Bank, class State> int get_state(Bank *b, const char *entry, uint32_t channel, State *s, void *stream)
    {
        MI_REQUIRE(b != nullptr, MI_ESTATE, "%s: NULL bank", entry);
        MI_REQUIRE(channel < b->channels, MI_EINVAL, "%s: channel %u out of range", entry, channel);
        return mi::read_state(s, b->d_state + channel, mi::as_stream(stream));
    }
    template <class Bank, class State> int set_state(Bank *b, const char *entry, uint32_t channel, const State &s, bool valid, hipStream_t st)
    {
        MI_REQUIRE(b != nullptr && channel < b->channels && valid, MI_EINVAL, "%s: bad argument", entry);
        return mi::write_state(b->d_state + channel, s, st);
    }
    // ... of a bank with the Compressor's follower: fEnvelope, fPeak, nHoldCounter, each wanted or not
    template <class Bank> int get_follow_state(Bank *b, const char *entry, uint32_t channel, float *envelope, float *peak,
                                               uint32_t *hold, void *stream)
    {
        device_state s;
        const int r = get_state(b, entry, channel, &s, stream);
        if (r != MI_OK)
            return r;
        if (envelope != nullptr) *envelope = s.e;
        if (peak != nullptr) *peak = s.peak;
        if (hold != nullptr) *hold = s.hold;
        return MI_OK;
    }

    template <class Bank> int destroy(Bank *b)
    {
        if (b == nullptr)
            return MI_OK;
        (void)hipFree(b->d_params); (void)hipFree(b->d_state);
        delete b;
        return MI_OK;
    }

    template <class Bank> int create(Bank **bank, const char *entry, uint32_t channels)
    {
        MI_REQUIRE(bank != nullptr, MI_EINVAL, "%s: NULL result pointer", entry);
        *bank = nullptr;
        MI_REQUIRE(channels > 0 && channels <= (1u << 20), MI_EINVAL, "%s: channels must be 1 .. 1048576", entry);
        MI_REQUIRE(mi_dspu_device_count() > 0, MI_ENODEV, "no HIP device available (there is no CPU fallback)");
        Bank *b = new (std::nothrow) Bank();
        MI_REQUIRE(b != nullptr, MI_ENOMEM, "%s: out of host memory", entry);
        b->channels = channels;
        b->cfg.assign(channels, Bank::fresh_settings());
        b->update.assign(channels, 1);
        b->params.assign(channels, Bank::fresh_params());
        const size_t params_bytes = size_t(channels) * sizeof(*b->d_params), state_bytes = size_t(channels) * sizeof(*b->d_state);
        hipError_t e = hipMalloc(reinterpret_cast<void **>(&b->d_params), params_bytes);
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&b->d_state), state_bytes);
        if (e == hipSuccess) e = hipMemcpy(b->d_params, b->params.data(), params_bytes, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemset(b->d_state, 0, state_bytes);
        if (e != hipSuccess)
        {
            destroy(b);
            return mi::fail(MI_EHIP, "%s: %s", entry, hipGetErrorString(e));
        }
        *bank = b;
        return MI_OK;
    }

    template <class Bank> int clear(Bank *b, const char *entry, void *stream)
    {
        MI_REQUIRE(b != nullptr, MI_ESTATE, "%s: NULL bank", entry);
        MI_HIP_CHECK(hipMemsetAsync(b->d_state, 0, size_t(b->channels) * sizeof(*b->d_state), mi::as_stream(stream)));
        return MI_OK;
    }

    template <class Bank> int launch(Bank *b, float *gain, float *env, const float *in, const float *audio, size_t count,
                                     size_t gain_stride, size_t env_stride, size_t in_stride, size_t audio_stride, hipStream_t st)
    {
        const uint32_t vec = (mi::aligned16(in, in_stride, b->channels) ? VEC_IN : 0) | (mi::aligned16(gain, gain_stride, b->channels) ? VEC_GAIN : 0) |
                             (mi::aligned16(env, env_stride, b->channels) ? VEC_ENV : 0) | (mi::aligned16(audio, audio_stride, b->channels) ? VEC_AUDIO : 0);
        hipEvent_t ev0 = nullptr, ev1 = nullptr;
        mi::take_profile_events(&ev0, &ev1);
        Bank::launch(dim3((b->channels + GROUP - 1) / GROUP), st, ev0, ev1, gain, env, in, audio, gain_stride, env_stride, in_stride,
                     audio_stride, uint32_t(count), b->channels, b->d_params, b->d_state, vec);
        MI_HIP_CHECK(hipGetLastError());
        return MI_OK;
    }

    template <class Bank> int process(Bank *b, const char *entry, float *gain, float *env, const float *in, size_t count,
                                      size_t gain_stride, size_t env_stride, size_t in_stride, void *stream)
    {
        MI_REQUIRE(b != nullptr, MI_ESTATE, "%s: NULL bank", entry);
        hipStream_t st = mi::as_stream(stream);
        const int r = update(b, st);
        if (r != MI_OK || count == 0)
            return r;
        MI_REQUIRE(gain != nullptr && in != nullptr, MI_EINVAL, "%s: NULL buffer", entry);
        MI_REQUIRE(count < (size_t(1) << 31), MI_EINVAL, "%s: count %zu too large", entry, count);
        MI_REQUIRE(b->channels == 1 || (gain_stride >= count && in_stride >= count && (env == nullptr || env_stride >= count)), MI_EINVAL,
                   "%s: strides (%zu, %zu, %zu) shorter than count %zu", entry, gain_stride, env_stride, in_stride, count);
        MI_REQUIRE(gain != env, MI_EINVAL, "%s: gain and env are the same buffer", entry);
        MI_REQUIRE((gain != in || gain_stride == in_stride) && (env != in || env_stride == in_stride), MI_EINVAL,
                   "%s: in place with different strides", entry);
        return launch(b, gain, env, in, nullptr, count, gain_stride, env_stride, in_stride, 0, st);
    }

    template <class Bank> int process_apply(Bank *b, const char *entry, float *dst, const float *audio, const float *sc, size_t count,
                                            size_t dst_stride, size_t audio_stride, size_t sc_stride, void *stream)
    {
        MI_REQUIRE(b != nullptr, MI_ESTATE, "%s: NULL bank", entry);
        hipStream_t st = mi::as_stream(stream);
        const int r = update(b, st);
        if (r != MI_OK || count == 0)
            return r;
        MI_REQUIRE(dst != nullptr && audio != nullptr && sc != nullptr, MI_EINVAL, "%s: NULL buffer", entry);
        MI_REQUIRE(count < (size_t(1) << 31), MI_EINVAL, "%s: count %zu too large", entry, count);
        MI_REQUIRE(b->channels == 1 || (dst_stride >= count && audio_stride >= count && sc_stride >= count), MI_EINVAL,
                   "%s: strides (%zu, %zu, %zu) shorter than count %zu", entry, dst_stride, audio_stride, sc_stride, count);
        MI_REQUIRE((dst != audio || dst_stride == audio_stride) && (dst != sc || dst_stride == sc_stride), MI_EINVAL,
                   "%s: in place with different strides", entry);
        return launch(b, dst, nullptr, sc, audio, count, dst_stride, 0, sc_stride, audio_stride, st);
    }

    // curve() and its kin over rows of `dots`: run(grid, st, ev0, ev1) is the MI_LAUNCH of the bank's curve kernel, blocks of
    // CURVE_BLOCK dots by channels
    template <class Bank, class Run> int curve(Bank *b, const char *entry, float *out, const float *in, size_t dots, size_t out_stride,
                                               size_t in_stride, void *stream, Run run)
    {
        MI_REQUIRE(b != nullptr, MI_ESTATE, "%s: NULL bank", entry);
        hipStream_t st = mi::as_stream(stream);
        const int r = update(b, st);
        if (r != MI_OK || dots == 0)
            return r;
        MI_REQUIRE(out != nullptr && in != nullptr, MI_EINVAL, "%s: NULL buffer", entry);
        MI_REQUIRE(dots < (size_t(1) << 31), MI_EINVAL, "%s: %zu dots are too many", entry, dots);
        MI_REQUIRE(b->channels <= 65535u, MI_EINVAL, "%s: more than 65535 channels", entry);
        MI_REQUIRE(b->channels == 1 || (out_stride >= dots && in_stride >= dots), MI_EINVAL,
                   "%s: strides (%zu, %zu) shorter than %zu dots", entry, out_stride, in_stride, dots);
        MI_REQUIRE(out != in || out_stride == in_stride, MI_EINVAL, "%s: in place with different strides", entry);
        hipEvent_t ev0 = nullptr, ev1 = nullptr;
        mi::take_profile_events(&ev0, &ev1);
        run(dim3(uint32_t((dots + CURVE_BLOCK - 1) / CURVE_BLOCK), b->channels), st, ev0, ev1);
        MI_HIP_CHECK(hipGetLastError());
        return MI_OK;
    }
} // namespace mi_dynamics
