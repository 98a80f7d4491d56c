// The settings arithmetic of lsp::dspu::Oscillator (src/main/util/Oscillator.cpp): construct(), the setters and update_settings()
// on a mi_oscillator_settings_t, shared by the bank (csrc/oscillator.hip) and by whoever wants the words without a device.
// Every expression keeps the reference's types: where it mixes double and float, so does this (nPhaseAccMask + 1.0 is a double,
// nPhaseAccMask + 1.0f is float 2^32 for a 32-bit accumulator, M_SQRT1_2 is a double stored to a float).
#include "mi_common.h"

#include <cmath>
#include <cstdint>

#pragma clang fp contract(off)

namespace
{
    // floating point -> uint32_t as the bank defines it: through int64_t, the low 32 bits; NaN and beyond int64_t: 0
    inline uint32_t to_u32(double x)
    {
        if (!(std::fabs(x) < 9223372036854775808.0))
            return 0;
        return uint32_t(uint64_t(int64_t(x)));
    }

    inline float clamp01(float v) { return (v < 0.0f) ? 0.0f : (v > 1.0f) ? 1.0f : v; }

    constexpr double PI = 3.14159265358979323846, ONE_OVER_PI = 0.31830988618379067154, SQRT1_2 = 0.70710678118654752440;
    constexpr uint32_t MAX_BITS = 32;                       // sizeof(phacc_t) * 8, :54-55

    static_assert(sizeof(mi_oscillator_settings_t) == 248, "mi_oscillator_settings_t: the Python binding mirrors this layout");
}

extern "C" {

int mi_oscillator_settings_init(mi_oscillator_settings_t *s)                            // construct(), :42-117
{
    MI_REQUIRE(s != nullptr, MI_EINVAL, "mi_oscillator_settings_init: NULL settings");
    *s = mi_oscillator_settings_t();
    s->function = MI_FG_SINE;
    s->amplitude = 1.0f;
    s->dc_reference = MI_DC_WAVEDC;
    s->sample_rate = UINT64_MAX;                            // size_t(-1)
    s->bits = MAX_BITS;
    s->duty = 0.5f;
    s->width = 1.0f;
    s->raise_ratio = 0.25f, s->fall_ratio = 0.25f;
    s->par_amplitude = 1.0f;
    s->over_mode = MI_OM_NONE;
    s->sync = 1;
    s->phase_known = 1, s->phase = 0;                       // nPhaseAcc = 0
    return MI_OK;
}

int mi_oscillator_settings_set(mi_oscillator_settings_t *s, uint32_t setter, double a, double b)
{
    MI_REQUIRE(s != nullptr, MI_EINVAL, "mi_oscillator_settings_set: NULL settings");
    const float fa = float(a), fb = float(b);
    switch (setter)
    {
        case MI_OSC_SET_FUNCTION:                           // .h:240-244: no comparison with the old value
            MI_REQUIRE(a >= 0 && a <= MI_FG_BL_PARABOLIC && a == std::floor(a), MI_EINVAL, "mi_oscillator_bank_set_function: no function %g", a);
            s->function = uint32_t(a), s->sync = 1;
            break;
        case MI_OSC_SET_FREQUENCY:                          // .h:250-257
            if (s->frequency == fa)
                break;
            s->frequency = fa, s->sync = 1;
            break;
        case MI_OSC_SET_SAMPLE_RATE:                        // .h:221-229
        {
            MI_REQUIRE(a >= 0 && a < 18446744073709551616.0, MI_EINVAL, "mi_oscillator_bank_set_sample_rate: bad rate %g", a);
            const uint64_t sr = uint64_t(a);
            if (s->sample_rate == sr)
                break;
            s->sample_rate = sr, s->phase_known = 1, s->phase = 0, s->sync = 1;
            break;
        }
        case MI_OSC_SET_PHASE:                              // :749-757
            if (s->init_phase == fa)
                break;
            s->init_phase = fa, s->sync = 1;
            break;
        case MI_OSC_SET_PHASE_ACCUMULATOR_BITS:             // .h:207-215: the argument is a uint8_t
        {
            MI_REQUIRE(a >= 0 && a <= 255 && a == std::floor(a), MI_EINVAL, "mi_oscillator_bank_set_phase_accumulator_bits: bad width %g", a);
            const uint32_t bits = uint32_t(a);
            if (s->bits == bits || bits > MAX_BITS)
                break;
            s->bits = bits, s->phase_known = 1, s->phase = 0, s->sync = 1;
            break;
        }
        case MI_OSC_SET_DC_OFFSET:                          // :765-771: bSync stays
            if (s->dc_offset == fa)
                break;
            s->dc_offset = fa;
            break;
        case MI_OSC_SET_DC_REFERENCE:                       // :773-777
            MI_REQUIRE(a == MI_DC_WAVEDC || a == MI_DC_ZERO, MI_EINVAL, "mi_oscillator_bank_set_dc_reference: no reference %g", a);
            s->dc_reference = uint32_t(a), s->sync = 1;
            break;
        case MI_OSC_SET_AMPLITUDE:                          // :883-890
            if (s->amplitude == fa)
                break;
            s->amplitude = fa, s->sync = 1;
            break;
        case MI_OSC_SET_DUTY_RATIO:                         // :797-804
            if ((s->duty == fa) || (fa < 0.0f) || (fa > 1.0f) || std::isnan(fa))    // a NaN would be stored by :799; refused here
                break;
            s->duty = fa, s->sync = 1;
            break;
        case MI_OSC_SET_WIDTH:                              // :806-817
        {
            const float w = clamp01(fa);
            if (s->width == w)
                break;
            s->width = w, s->sync = 1;
            break;
        }
        case MI_OSC_SET_TRAPEZOID_RATIOS:                   // :819-838
        {
            const float raise = clamp01(fa);
            float fall = fb;
            if (fall < 0.0f)
                fall = 0.0f;
            else if (fall > 1 - raise)
                fall = 1 - raise;
            if ((raise == s->raise_ratio) && (fall == s->fall_ratio))
                break;
            s->raise_ratio = raise, s->fall_ratio = fall, s->sync = 1;
            break;
        }
        case MI_OSC_SET_PULSETRAIN_RATIOS:                  // :840-858
        {
            const float pos = clamp01(fa), neg = clamp01(fb);
            if ((pos == s->pos_ratio) && (neg == s->neg_ratio))
                break;
            s->pos_ratio = pos, s->neg_ratio = neg, s->sync = 1;
            break;
        }
        case MI_OSC_SET_PARABOLIC_WIDTH:                    // :860-872
        {
            const float w = clamp01(fa);
            if (s->par_width == w)
                break;
            s->par_width = w, s->sync = 1;
            break;
        }
        case MI_OSC_SET_SQUARED_SINUSOID_INVERSION:         // :779-786
            if (s->sq_invert == uint32_t(a != 0))
                break;
            s->sq_invert = a != 0, s->sync = 1;
            break;
        case MI_OSC_SET_PARABOLIC_INVERSION:                // :788-795
            if (s->par_invert == uint32_t(a != 0))
                break;
            s->par_invert = a != 0, s->sync = 1;
            break;
        case MI_OSC_SET_OVERSAMPLER_MODE:                   // :874-881
            MI_REQUIRE(a >= 0 && a <= MI_OM_LANCZOS_8X24BIT && a == std::floor(a), MI_EINVAL, "mi_oscillator_bank_set_oversampler_mode: no mode %g", a);
            if (uint32_t(a) == s->over_mode)
                break;
            s->over_mode = uint32_t(a), s->sync = 1;
            break;
        case MI_OSC_RESET_PHASE_ACCUMULATOR:                // .h:234
            s->phase_known = 1, s->phase = 0;
            break;
        default:
            return mi::fail(MI_EINVAL, "mi_oscillator_settings_set: no setter %u", setter);
    }
    return MI_OK;
}

int mi_oscillator_settings_update(mi_oscillator_settings_t *s)                          // update_settings(), :151-357
{
    MI_REQUIRE(s != nullptr, MI_EINVAL, "mi_oscillator_settings_update: NULL settings");
    if (!s->sync)                                                                       // :153
        return MI_OK;
    const uint32_t old_mask = s->mask;
    s->mask = (s->bits == MAX_BITS) ? uint32_t(-1) : (uint32_t(1) << s->bits) - uint32_t(1);    // :156-159
    const double m1 = s->mask + 1.0;
    s->acc2phase = 2.0 * PI * (1.0 / m1);                                               // :161
    s->freq_word = to_u32((m1 * s->frequency) / double(s->sample_rate));                // :162

    // :164-166.  With the phase known the two masked steps are taken here; otherwise the phase is the device's plus what is
    // kept in s->phase, and the mask has not changed (a change of the width makes the phase known): the two steps add up
    const uint32_t old_word = s->init_word;
    s->init_word = to_u32(m1 * 0.5 * ONE_OVER_PI * (s->init_phase - 2.0 * PI * std::floor(s->init_phase * 0.5 * ONE_OVER_PI)));
    if (s->phase_known || old_mask != s->mask)
    {
        s->phase_known = 1;                                                             // (a mask change without a reset cannot happen)
        s->phase = (s->phase - old_word) & s->mask;
        s->phase = (s->phase + s->init_word) & s->mask;
    }
    else
        s->phase = s->phase - old_word + s->init_word;

    const float fm1 = s->mask + 1.0f, A = s->amplitude;                                 // float(mask) + 1.0f
    switch (s->function)
    {
        case MI_FG_SINE: case MI_FG_COSINE:                                             // :170-173
            s->referenced_dc = s->dc_offset;
            break;
        case MI_FG_SQUARED_SINE: case MI_FG_SQUARED_COSINE:                             // :174-195
            s->sq_amplitude = s->sq_invert ? -A : A;
            s->sq_wave_dc = 0.5f * s->sq_amplitude;
            s->referenced_dc = (s->dc_reference == MI_DC_ZERO) ? s->dc_offset - s->sq_wave_dc : s->dc_offset;
            break;
        case MI_FG_RECTANGULAR: case MI_FG_BL_RECTANGULAR:                              // :197-220
            s->duty_word = (s->duty == 1.0f) ? s->mask : to_u32(s->duty * fm1);
            s->rect_wave_dc = A * (2.0f * s->duty - 1.0f);
            s->referenced_dc = (s->dc_reference == MI_DC_ZERO) ? s->dc_offset - s->rect_wave_dc : s->dc_offset;
            s->rect_atten = 0.6f;
            break;
        case MI_FG_SAWTOOTH: case MI_FG_BL_SAWTOOTH:                                    // :222-247
        {
            s->width_word = (s->width == 1.0f) ? s->mask : to_u32(s->width * fm1);
            const float ww = float(s->width_word);
            s->saw_coeffs[0] = 2.0f * A / ww;
            s->saw_coeffs[1] = -A;
            s->saw_coeffs[2] = (-2.0f * A) / (fm1 - ww);
            s->saw_coeffs[3] = A * (fm1 + ww) / (fm1 - ww);
            s->saw_wave_dc = 0.0f;
            s->referenced_dc = s->dc_offset;
            if (s->width > 0.60f)
                s->saw_atten = 0.64f / 0.4f - s->width;
            else if (s->width < 0.40f)
                s->saw_atten = s->width + 0.6f;
            else
                s->saw_atten = 1.0f;
            break;
        }
        case MI_FG_TRAPEZOID: case MI_FG_BL_TRAPEZOID:                                  // :249-279
        {
            s->points[0] = to_u32(s->raise_ratio * 0.5f * fm1);
            s->points[1] = to_u32((1.0f - s->fall_ratio) * 0.5f * fm1);
            s->points[2] = (s->fall_ratio < 1.0f) ? to_u32((1.0f + s->fall_ratio) * 0.5f * fm1) : s->mask;
            s->points[3] = (s->raise_ratio > 0.0f) ? to_u32((2.0f - s->raise_ratio) * 0.5f * fm1) : s->mask;
            s->trap_coeffs[0] = A / float(s->points[0]);
            s->trap_coeffs[1] = -2.0f * A / float(uint32_t(s->points[2] - s->points[1]));
            s->trap_coeffs[2] = A / s->fall_ratio;
            s->trap_coeffs[3] = -2.0f * A / s->raise_ratio;
            s->trap_wave_dc = 0.0f;
            s->referenced_dc = s->dc_offset;
            const float low = (s->raise_ratio < s->fall_ratio) ? s->raise_ratio : s->fall_ratio;
            s->trap_atten = (low < 0.4f) ? low + 0.6f : 1.0f;
            break;
        }
        case MI_FG_PULSETRAIN: case MI_FG_BL_PULSETRAIN:                                // :281-308
        {
            s->train[0] = to_u32(s->pos_ratio * 0.5f * fm1);
            s->train[1] = to_u32(0.5f * fm1);
            s->train[2] = (s->neg_ratio == 1.0f) ? s->mask : to_u32((1.0f + s->neg_ratio) * 0.5f * fm1);
            s->pulse_wave_dc = 0.5f * A * (s->pos_ratio - s->neg_ratio);
            s->referenced_dc = (s->dc_reference == MI_DC_ZERO) ? s->dc_offset - s->pulse_wave_dc : s->dc_offset;
            const float high = (s->neg_ratio > s->pos_ratio) ? s->neg_ratio : s->pos_ratio;
            s->pulse_atten = (high > 0.5f) ? 0.6f : SQRT1_2;
            break;
        }
        case MI_FG_PARABOLIC: case MI_FG_BL_PARABOLIC:                                  // :310-338
            s->par_amplitude = s->par_invert ? -A : A;
            s->par_word = (s->par_width == 1) ? s->mask : to_u32(s->par_width * fm1);
            s->par_wave_dc = 2.0f * s->par_amplitude * s->par_width / 3.0f;
            s->referenced_dc = (s->dc_reference == MI_DC_ZERO) ? s->dc_offset - s->par_wave_dc : s->dc_offset;
            s->par_atten = 1.0f;
            break;
        default:
            break;
    }
    uint32_t times = 1;                                                                 // :353, Oversampler.cpp:146-195
    if (s->over_mode >= MI_OM_LANCZOS_2X2 && s->over_mode <= MI_OM_LANCZOS_8X24BIT)
    {
        static const uint32_t TIMES[5] = { 2, 3, 4, 6, 8 };
        times = TIMES[(s->over_mode - MI_OM_LANCZOS_2X2) / 6];
    }
    s->oversampling = times;
    s->freq_word_over = s->freq_word / times;                                           // :354
    s->sync = 0;
    return MI_OK;
}

} // extern "C"
