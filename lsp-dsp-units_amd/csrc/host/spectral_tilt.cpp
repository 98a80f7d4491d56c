// The designer of lsp::dspu::SpectralTilt (reference: src/main/filters/SpectralTilt.cpp) on a mi_spectral_tilt_settings_t, host only:
// construct(), the setters, update_settings() line for line -- every expression has the reference's operand types, so what the
// reference evaluates in double and rounds to float is evaluated in double and rounded to float here --, and complex_transfer_calc.
// size_t is the reference's LP64 one: uint64_t.  dsp::bilinear_transform_x1 is lsp-dsp-lib's; what stands here are the formulas of
// Filter::bilinear_transform (Filter.cpp:2225-2262) in float, the reading that csrc/dynfilter.hip has of it.
#include "mi_common.h"

#include <cmath>
#include <cstdint>
#include <utility>

#pragma clang fp contract(off)

namespace
{
    constexpr uint64_t MAX_ORDER = 128u;                        // SpectralTilt.cpp:29-35
    constexpr float DFL_LOWER_FREQUENCY = 0.1f, DFL_UPPER_FREQUENCY = 20.0e3f;
    constexpr float DB_PER_OCTAVE_FALLOFF = 0.16609640419483184814453125f, DB_PER_DECADE_FALLOFF = 0.05f;

    float bilinear_coefficient(float angularFrequency, float samplerate)    // :150-153
    {
        return angularFrequency / tanf(0.5f * angularFrequency / samplerate);
    }

    float digital_biquad_gain(const mi_spectral_tilt_settings_t &s, const mi_biquad_x1_t *digitalbq, float frequency)   // :180-203
    {
        double w = 2 * M_PI * frequency / s.sample_rate;
        w = fmod(w + M_PI, 2.0 * M_PI);
        w = (w >= 0.0) ? w - M_PI : w + M_PI;

        double cw   = cos(w);
        double sw   = sin(w);
        double c2w  = cw*cw - sw*sw;
        double s2w  = 2.0f * cw * sw;

        double num_re = digitalbq->b0 + digitalbq->b1 * cw + digitalbq->b2 * c2w;
        double num_im = -digitalbq->b1 * sw - digitalbq->b2 * s2w;

        double den_re = 1.0 - digitalbq->a1 * cw - digitalbq->a2 * c2w;
        double den_im = digitalbq->a1 * sw + digitalbq->a2 * s2w;
        double den_sq_mag = den_re * den_re + den_im * den_im;

        double gain_re = (num_re * den_re + num_im * den_im) / den_sq_mag;
        double gain_im = (num_im * den_re - num_re * den_im) / den_sq_mag;

        return sqrt(gain_re * gain_re + gain_im * gain_im);
    }

    void normalise_digital_biquad(const mi_spectral_tilt_settings_t &s, mi_biquad_x1_t *digitalbq)     // :205-252
    {
        const uint64_t nSampleRate = s.sample_rate;
        float gain;
        switch (s.norm)
        {
            case MI_STLT_NORM_AT_DC:        gain = 1.0f / digital_biquad_gain(s, digitalbq, 0.0f); break;
            case MI_STLT_NORM_AT_20_HZ:     gain = 1.0f / digital_biquad_gain(s, digitalbq, 20.0f); break;
            case MI_STLT_NORM_AT_1_KHZ:     gain = 1.0f / digital_biquad_gain(s, digitalbq, 1000.0f); break;
            case MI_STLT_NORM_AT_20_KHZ:    gain = 1.0f / digital_biquad_gain(s, digitalbq, 20000.0f); break;
            case MI_STLT_NORM_AT_NYQUIST:   gain = 1.0f / digital_biquad_gain(s, digitalbq, 0.5f * nSampleRate); break;
            case MI_STLT_NORM_AUTO:
                if (s.slope_nep_nep <= 0)
                    gain = (0.5f * nSampleRate > 20.0f) ? 1.0f / digital_biquad_gain(s, digitalbq, 20.0f) : 1.0f / digital_biquad_gain(s, digitalbq, 0.0f);
                else
                    gain = (0.5f * nSampleRate > 20000.0f) ? 1.0f / digital_biquad_gain(s, digitalbq, 20000.0f) : 1.0f / digital_biquad_gain(s, digitalbq, 0.5f * nSampleRate);
                break;
            default:
            case MI_STLT_NORM_NONE:         gain = 1.0f; break;
        }
        digitalbq->b0 *= gain;
        digitalbq->b1 *= gain;
        digitalbq->b2 *= gain;
    }

    // dsp::bilinear_transform_x1(bf, bc, kf, 1): Filter.cpp:2225-2262 in float
    void bilinear_transform_x1(mi_biquad_x1_t *f, const float *t, const float *b, float kf)
    {
        const float kf2 = kf * kf;
        const float T0 = t[0], T1 = t[1] * kf, T2 = t[2] * kf2;
        const float B0 = b[0], B1 = b[1] * kf, B2 = b[2] * kf2;
        const float N = 1.0f / (B0 + B1 + B2);
        f->b0 = (T0 + T1 + T2) * N;
        f->b1 = 2.0f * (T0 - T2) * N;
        f->b2 = (T0 - T1 + T2) * N;
        f->a1 = 2.0f * (B2 - B0) * N;                           // sign negated
        f->a2 = (B1 - B2 - B0) * N;                             // sign negated
        f->p0 = f->p1 = f->p2 = 0.0f;
    }

    void complex_transfer_calc(const mi_spectral_tilt_settings_t &s, float *re, float *im, float f)     // :453-503
    {
        float kf    = f / float(s.sample_rate);
        float w     = 2.0f * M_PI * kf;
        w           = fmodf(w + M_PI, 2.0 * M_PI);
        w           = w >= 0.0f ? (w - M_PI) : (w + M_PI);

        float cw    = cosf(w);
        float sw    = sinf(w);
        float c2w   = cw * cw - sw * sw;
        float s2w   = 2.0 * sw * cw;

        float r_re  = 1.0f, r_im = 0.0f;
        float b_re, b_im;

        for (uint32_t i = 0; i < s.n_sections; ++i)
        {
            const mi_biquad_x1_t *bq = &s.sections[i];

            float num_re = bq->b0 + bq->b1 * cw + bq->b2 * c2w;
            float num_im = -bq->b1 * sw - bq->b2 * s2w;

            float den_re = 1.0 - bq->a1 * cw - bq->a2 * c2w;
            float den_im = bq->a1 * sw + bq->a2 * s2w;

            float den_sq_mag = den_re * den_re + den_im * den_im;

            float w_re = (num_re * den_re + num_im * den_im) / den_sq_mag;
            float w_im = (den_re * num_im - num_re * den_im) / den_sq_mag;

            b_re            = r_re*w_re - r_im*w_im;
            b_im            = r_re*w_im + r_im*w_re;

            r_re            = b_re;
            r_im            = b_im;
        }

        *re     = r_re;
        *im     = r_im;
    }
} // namespace

extern "C" {

int mi_spectral_tilt_settings_init(mi_spectral_tilt_settings_t *s)                          // construct(), :52-71
{
    MI_REQUIRE(s != nullptr, MI_EINVAL, "mi_spectral_tilt_settings_init: NULL settings");
    *s = mi_spectral_tilt_settings_t();
    s->order = 1;
    s->slope_unit = MI_STLT_SLOPE_UNIT_NEPER_PER_NEPER;
    s->norm = MI_STLT_NORM_AUTO;
    s->slope_val = 0.5f;
    s->slope_nep_nep = 0.5f;
    s->lower_frequency = DFL_LOWER_FREQUENCY;
    s->upper_frequency = DFL_UPPER_FREQUENCY;
    s->sample_rate = ~uint64_t(0);                              // nSampleRate = -1
    s->bypass = 0;
    s->sync = 1;
    return MI_OK;
}

#define TILT_SETTINGS(name) MI_REQUIRE(s != nullptr, MI_EINVAL, "mi_spectral_tilt_settings_" name ": NULL settings")

int mi_spectral_tilt_settings_set_order(mi_spectral_tilt_settings_t *s, uint64_t order)     // :139-146
{
    TILT_SETTINGS("set_order");
    if (order == s->order)
        return MI_OK;
    s->order = order;
    s->sync = 1;
    return MI_OK;
}

int mi_spectral_tilt_settings_set_slope(mi_spectral_tilt_settings_t *s, float slope, uint32_t unit)    // :129-137
{
    TILT_SETTINGS("set_slope");
    if ((slope == s->slope_val) && (unit == s->slope_unit))
        return MI_OK;
    s->slope_val = slope;
    s->slope_unit = unit;
    s->sync = 1;
    return MI_OK;
}

int mi_spectral_tilt_settings_set_norm(mi_spectral_tilt_settings_t *s, uint32_t norm)       // :123-127
{
    TILT_SETTINGS("set_norm");
    s->norm = norm;
    s->sync = 1;
    return MI_OK;
}

int mi_spectral_tilt_settings_set_lower_frequency(mi_spectral_tilt_settings_t *s, float lower)     // :101-108
{
    TILT_SETTINGS("set_lower_frequency");
    if (lower == s->lower_frequency)
        return MI_OK;
    s->lower_frequency = lower;
    s->sync = 1;
    return MI_OK;
}

int mi_spectral_tilt_settings_set_upper_frequency(mi_spectral_tilt_settings_t *s, float upper)     // :92-99
{
    TILT_SETTINGS("set_upper_frequency");
    if (upper == s->upper_frequency)
        return MI_OK;
    s->upper_frequency = upper;
    s->sync = 1;
    return MI_OK;
}

int mi_spectral_tilt_settings_set_frequency_range(mi_spectral_tilt_settings_t *s, float lower, float upper)    // :110-121
{
    TILT_SETTINGS("set_frequency_range");
    if (upper > lower)                                          // the wrong way round, as the reference has it
        std::swap(upper, lower);
    if ((lower == s->lower_frequency) && (upper == s->upper_frequency))
        return MI_OK;
    s->lower_frequency = lower;
    s->upper_frequency = upper;
    s->sync = 1;
    return MI_OK;
}

int mi_spectral_tilt_settings_set_sample_rate(mi_spectral_tilt_settings_t *s, uint64_t sr)  // :83-90
{
    TILT_SETTINGS("set_sample_rate");
    if (s->sample_rate == sr)
        return MI_OK;
    s->sample_rate = sr;
    s->sync = 1;
    return MI_OK;
}

// update_settings(), :254-375.  *designed (may be NULL): the sections were made anew, which is sFilter.begin() ... end(true):
// whoever runs them clears the filter memory.
int mi_spectral_tilt_settings_update(mi_spectral_tilt_settings_t *s, int *designed)
{
    TILT_SETTINGS("update");
    if (designed != nullptr)
        *designed = 0;
    if (!s->sync)
        return MI_OK;

    uint64_t nOrder = s->order;
    const uint64_t nSampleRate = s->sample_rate;
    nOrder = (nOrder % 2 == 0) ? nOrder : nOrder + 1;
    nOrder = (nOrder < MAX_ORDER) ? nOrder : MAX_ORDER;
    s->order = nOrder;

    switch (s->slope_unit)
    {
        case MI_STLT_SLOPE_UNIT_DB_PER_OCTAVE:  s->slope_nep_nep = s->slope_val * DB_PER_OCTAVE_FALLOFF; break;
        case MI_STLT_SLOPE_UNIT_DB_PER_DECADE:  s->slope_nep_nep = s->slope_val * DB_PER_DECADE_FALLOFF; break;
        default:
        case MI_STLT_SLOPE_UNIT_NEPER_PER_NEPER: s->slope_nep_nep = s->slope_val; break;
    }

    if (s->lower_frequency >= 0.5f * nSampleRate)
        s->lower_frequency = DFL_LOWER_FREQUENCY;
    if (s->upper_frequency >= 0.5f * nSampleRate)
        s->upper_frequency = DFL_UPPER_FREQUENCY;
    if (s->lower_frequency >= s->upper_frequency)
    {
        s->lower_frequency = DFL_LOWER_FREQUENCY;
        s->upper_frequency = DFL_UPPER_FREQUENCY;
    }

    if ((s->slope_unit == MI_STLT_SLOPE_UNIT_NONE) || (s->slope_nep_nep == 0.0f))
    {
        s->bypass = 1;                                          // the sections stay as the last design left them
        s->sync = 0;
        return MI_OK;
    }
    else
        s->bypass = 0;

    float l_angf = 2.0f * M_PI * s->lower_frequency;
    float u_angf = 2.0f * M_PI * s->upper_frequency;

    float r = powf(u_angf / l_angf, 1.0f / (nOrder - 1));       // nOrder 0: 1 / float(2^64 - 1)
    float c_fn = bilinear_coefficient(1.0f, nSampleRate);
    float negZero = l_angf * powf(r, -s->slope_nep_nep);
    float negPole = l_angf;

    s->n_sections = 0;                                          // sFilter.begin()
    for (uint64_t n = 0; n < nOrder; n += 2)
    {
        const float now_b0 = negZero, now_b1 = 1.0f, now_a0 = negPole, now_a1 = 1.0f;      // compute_bilinear_element(), :156-178
        negZero *= r;
        negPole *= r;
        const float nxt_b0 = negZero, nxt_b1 = 1.0f, nxt_a0 = negPole, nxt_a1 = 1.0f;
        negZero *= r;
        negPole *= r;

        mi_biquad_x1_t *digitalbq = &s->sections[s->n_sections++];     // add_chain(): 64 of FilterBank::init(128)'s places at most

        float t[3], b[3];
        t[0] = now_b0 * nxt_b0;
        t[1] = now_b0 * nxt_b1 + now_b1 * nxt_b0;
        t[2] = now_b1 * nxt_b1;
        b[0] = now_a0 * nxt_a0;
        b[1] = now_a0 * nxt_a1 + now_a1 * nxt_a0;
        b[2] = now_a1 * nxt_a1;

        bilinear_transform_x1(digitalbq, t, b, c_fn);
        normalise_digital_biquad(*s, digitalbq);
    }
    if (designed != nullptr)                                    // sFilter.end(true)
        *designed = 1;

    s->sync = 0;
    return MI_OK;
}

// digital_biquad_gain() and normalise_digital_biquad() of one section, :180-252, with the members of *s (the class's protected entries)
int mi_spectral_tilt_settings_section_gain(const mi_spectral_tilt_settings_t *s, const mi_biquad_x1_t *section, float frequency, float *gain)
{
    TILT_SETTINGS("section_gain");
    MI_REQUIRE(section != nullptr && gain != nullptr, MI_EINVAL, "mi_spectral_tilt_settings_section_gain: NULL argument");
    *gain = digital_biquad_gain(*s, section, frequency);
    return MI_OK;
}

int mi_spectral_tilt_settings_normalise_section(const mi_spectral_tilt_settings_t *s, mi_biquad_x1_t *section)
{
    TILT_SETTINGS("normalise_section");
    MI_REQUIRE(section != nullptr, MI_EINVAL, "mi_spectral_tilt_settings_normalise_section: NULL section");
    normalise_digital_biquad(*s, section);
    return MI_OK;
}

// freq_chart() behind its update_settings(), :505-523: both forms, by the pointers given (c: re and im interleaved)
int mi_spectral_tilt_settings_freq_chart(const mi_spectral_tilt_settings_t *s, float *re, float *im, float *c, const float *f, size_t count)
{
    TILT_SETTINGS("freq_chart");
    MI_REQUIRE(count == 0 || (f != nullptr && ((re != nullptr && im != nullptr) || c != nullptr)), MI_EINVAL,
               "mi_spectral_tilt_settings_freq_chart: NULL buffer");
    for (size_t i = 0; i < count; ++i)
    {
        float r_re, r_im;
        complex_transfer_calc(*s, &r_re, &r_im, f[i]);
        if (c != nullptr)
            c[2 * i] = r_re, c[2 * i + 1] = r_im;
        if (re != nullptr && im != nullptr)
            re[i] = r_re, im[i] = r_im;
    }
    return MI_OK;
}

} // extern "C"
