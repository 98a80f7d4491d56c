// What is specific to the follower family -- the Compressor, Expander, Gate and DynamicProcessor banks -- on the host: the launch
// of the bank's kernel, process(), process_apply() and curve() around it, and the follower's state.  The banks themselves are
// mi_bank::settings_bank (bank_core.h), which has the fields, update_settings, the hand-overs and create / destroy / clear;
// beside its static members a bank of this family supplies
//     launch(grid, st, ev0, ev1, args...)  MI_LAUNCH of its kernel, follow_kernel's arguments
#pragma once
#include "bank_core.h"
#include "dynamics_device.h"

namespace mi_dynamics
{
    using mi_bank::update;
    constexpr size_t COUNT_LIMIT = size_t(1) << 31;     // the kernels count samples and dots in 32 bits

    // the state of a bank with the Compressor's follower: fEnvelope, fPeak, nHoldCounter, each wanted or not
    template <class Bank> int get_follow_state(Bank *b, const char *entry, uint32_t channel, float *envelope, float *peak,
                                               uint32_t *hold, void *stream)
    {
        device_state s;
        const int r = mi_bank::get_state(b, entry, channel, &s, stream);
        if (r != MI_OK)
            return r;
        if (envelope != nullptr) *envelope = s.e;
        if (peak != nullptr) *peak = s.peak;
        if (hold != nullptr) *hold = s.hold;
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
        const int k = mi_bank::check_rows(entry, b->channels, count, COUNT_LIMIT,
                                          { { gain, gain_stride, count, mi_bank::REQUIRED | mi_bank::OUTPUT },
                                            { env, env_stride, count, mi_bank::OUTPUT }, { in, in_stride, count, mi_bank::REQUIRED } });
        if (k != MI_OK)
            return k;
        MI_REQUIRE(gain != env, MI_EINVAL, "%s: gain and env are the same buffer", entry);
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
        const int k = mi_bank::check_rows(entry, b->channels, count, COUNT_LIMIT,
                                          { { dst, dst_stride, count, mi_bank::REQUIRED | mi_bank::OUTPUT },
                                            { audio, audio_stride, count, mi_bank::REQUIRED }, { sc, sc_stride, count, mi_bank::REQUIRED } });
        if (k != MI_OK)
            return k;
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
        const int k = mi_bank::check_rows(entry, b->channels, dots, COUNT_LIMIT,
                                          { { out, out_stride, dots, mi_bank::REQUIRED | mi_bank::OUTPUT },
                                            { in, in_stride, dots, mi_bank::REQUIRED } });
        if (k != MI_OK)
            return k;
        MI_REQUIRE(b->channels <= 65535u, MI_EINVAL, "%s: more than 65535 channels", entry);
        hipEvent_t ev0 = nullptr, ev1 = nullptr;
        mi::take_profile_events(&ev0, &ev1);
        run(dim3(uint32_t((dots + CURVE_BLOCK - 1) / CURVE_BLOCK), b->channels), st, ev0, ev1);
        MI_HIP_CHECK(hipGetLastError());
        return MI_OK;
    }
} // namespace mi_dynamics
