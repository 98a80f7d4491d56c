// lsp::dspu::ADSREnvelope's arithmetic, shared by the bank (adsr.hip), the designer (host/adsr.cpp) and the class
// (host/adsr_class.cpp): the record that the kernel reads, the stage rule, the five generators (src/main/util/ADSREnvelope.cpp
// :350-383) and do_process (:295-326), written once for the host and the device.  Float arithmetic in the reference's order; every
// file that includes this switches contraction off.  expf is the float64 exp of the float32 argument rounded once on both sides.
#pragma once
#include "mi_dspu.h"

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MI_ADSR_HD __host__ __device__ __forceinline__
#else
#define MI_ADSR_HD inline
#endif

#pragma clang fp contract(off)                                  // from here to the end of the including file

namespace mi_adsr
{
    // the stages that generate()'s loops walk through, in their order (:392-432)
    enum { BEFORE, ATTACK, HOLD, DECAY, SLOPE, SUSTAIN, RELEASE, AFTER };

    // what the kernel needs of one channel: the segment ends (hold is the attack's end where F_USE_HOLD is off, so that the
    // hold compare never holds), the sustain level, the flags, the row switch, and the four designed curves
    struct record
    {
        float    t_attack, t_hold, t_decay, t_slope, t_release, sustain;
        uint32_t flags, enabled;
        uint32_t fn[MI_ADSR_PARTS];
        float    p[MI_ADSR_PARTS][6];
    };

    MI_ADSR_HD record record_of(const mi_adsr_settings_t &s, uint32_t enabled)
    {
        record r;
        r.t_attack = s.curve[MI_ADSR_ATTACK].time;
        r.t_hold = (s.flags & MI_ADSR_USE_HOLD) ? s.hold_time : s.curve[MI_ADSR_ATTACK].time;      // :304
        r.t_decay = s.curve[MI_ADSR_DECAY].time;
        r.t_slope = s.curve[MI_ADSR_SLOPE].time;
        r.t_release = s.curve[MI_ADSR_RELEASE].time;
        r.sustain = s.sustain_level;
        r.flags = s.flags & (MI_ADSR_USE_HOLD | MI_ADSR_USE_BREAK);
        r.enabled = enabled;
        for (int k = 0; k < MI_ADSR_PARTS; ++k)
        {
            r.fn[k] = s.curve[k].function;
            for (int j = 0; j < 6; ++j)
                r.p[k][j] = s.curve[k].params[j];
        }
        return r;
    }

    // The first loop condition of generate() that t meets (:393-427), which is do_process's chain of compares (:297-325) too.
    // A NaN meets none: generate() falls through to "after" (nan_stage = AFTER), do_process reaches the release generator
    // (nan_stage = RELEASE).
    MI_ADSR_HD int stage_of(const record &r, float t, int nan_stage)
    {
        if (t != t)
            return nan_stage;
        if (t <= 0.0f)
            return BEFORE;
        if (t >= 1.0f)
            return AFTER;
        if (t < r.t_attack)
            return ATTACK;
        if (t < r.t_hold)
            return HOLD;
        if (t < r.t_decay)
            return DECAY;
        if ((r.flags & MI_ADSR_USE_BREAK) && (t < r.t_slope))
            return SLOPE;
        if (t < r.t_release)
            return SUSTAIN;
        return RELEASE;
    }

    MI_ADSR_HD float exp_star(float x) { return float(exp(double(x))); }

    // pGenerator of curve PART at t; a function outside the enum is the default: label of configure_curve, none_generator
    template <int PART> MI_ADSR_HD float curve(const record &r, float t)
    {
        const float *p = r.p[PART];
        switch (r.fn[PART])
        {
            case MI_ADSR_LINE: case MI_ADSR_LINE2:              // :356-362
                return (t < p[0]) ? t * p[1] + p[2] : t * p[3] + p[4];
            case MI_ADSR_CUBIC:                                 // :364-369
            {
                const float u = t - p[0];
                return ((p[1] * u + p[2]) * u + p[3]) * u + p[4];
            }
            case MI_ADSR_QUADRO:                                // :371-376
            {
                const float u = t - p[0];
                return (((p[1] * u + p[2]) * u + p[3]) * u + p[4]) * u + p[5];
            }
            case MI_ADSR_EXP:                                   // :378-383
            {
                const float u = (t - p[0]) * p[4] + p[5];
                return p[2] + p[3] * u * exp_star(u * p[1]);
            }
            default:                                            // :350-354
                return (t - p[0]) * p[1] + p[2];
        }
    }

    // the envelope at t once its stage is known (hold is 1.0f, :308; stages 0 and 7 are +0, :298)
    MI_ADSR_HD float value_at(const record &r, int stage, float t)
    {
        switch (stage)
        {
            case ATTACK:    return curve<MI_ADSR_ATTACK>(r, t);
            case HOLD:      return 1.0f;
            case DECAY:     return curve<MI_ADSR_DECAY>(r, t);
            case SLOPE:     return curve<MI_ADSR_SLOPE>(r, t);
            case SUSTAIN:   return r.sustain;
            case RELEASE:   return curve<MI_ADSR_RELEASE>(r, t);
            default:        return 0.0f;
        }
    }

    MI_ADSR_HD float do_process(const record &r, float t) { return value_at(r, stage_of(r, t, RELEASE), t); }
} // namespace mi_adsr
