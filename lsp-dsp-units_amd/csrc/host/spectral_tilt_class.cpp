// lsp::dspu::SpectralTilt (src/main/filters/SpectralTilt.cpp).  The class keeps the reference's members; update_settings() copies them
// into a mi_spectral_tilt_settings_t, runs the library's host designer (csrc/host/spectral_tilt.cpp) and copies them back, and a new
// design goes to sFilter -- this library's FilterBank, whose rows run on the device -- with end(true).
#include <lsp-plug.in/dsp-units/filters/SpectralTilt.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "mi_dspu.h"

#pragma clang fp contract(off)

namespace lsp
{
namespace dspu
{
namespace
{
    constexpr size_t MAX_ORDER = 128;

    // the members as the designer reads them; the sections are sFilter's
    mi_spectral_tilt_settings_t settings_of(size_t order, stlt_slope_unit_t unit, stlt_norm_t norm, float slope, float nepnep, float lower, float upper,
                                            size_t rate, bool bypass, bool sync)
    {
        mi_spectral_tilt_settings_t s = mi_spectral_tilt_settings_t();
        s.order = order, s.sample_rate = rate, s.slope_unit = uint32_t(unit), s.norm = uint32_t(norm);
        s.slope_val = slope, s.slope_nep_nep = nepnep, s.lower_frequency = lower, s.upper_frequency = upper;
        s.bypass = bypass, s.sync = sync;
        return s;
    }
}

#define TILT_SETTINGS() settings_of(nOrder, enSlopeUnit, enNorm, fSlopeVal, fSlopeNepNep, fLowerFrequency, fUpperFrequency, nSampleRate, bBypass, bSync)

SpectralTilt::SpectralTilt()    { construct(); }
SpectralTilt::~SpectralTilt()   { destroy(); }

void SpectralTilt::construct()                                  // :52-71
{
    mi_spectral_tilt_settings_t s;
    mi_spectral_tilt_settings_init(&s);
    nOrder = s.order;
    enSlopeUnit = stlt_slope_unit_t(s.slope_unit), enNorm = stlt_norm_t(s.norm);
    fSlopeVal = s.slope_val, fSlopeNepNep = s.slope_nep_nep;
    fLowerFrequency = s.lower_frequency, fUpperFrequency = s.upper_frequency;
    nSampleRate = size_t(s.sample_rate);
    bBypass = s.bypass != 0, bSync = s.sync != 0;
    sFilter.construct();
}

void SpectralTilt::init()       { sFilter.init(MAX_ORDER); }
void SpectralTilt::destroy()    { sFilter.destroy(); }

void SpectralTilt::set_sample_rate(size_t sr)                   // :83-90
{
    if (nSampleRate == sr)
        return;
    nSampleRate = sr, bSync = true;
}

void SpectralTilt::set_upper_frequency(float upperFrequency)
{
    if (upperFrequency == fUpperFrequency)
        return;
    fUpperFrequency = upperFrequency, bSync = true;
}

void SpectralTilt::set_lower_frequency(float lowerFrequency)
{
    if (lowerFrequency == fLowerFrequency)
        return;
    fLowerFrequency = lowerFrequency, bSync = true;
}

void SpectralTilt::set_frequency_range(float lower, float upper)   // :110-121: swapped the wrong way round, as there
{
    mi_spectral_tilt_settings_t s = TILT_SETTINGS();
    mi_spectral_tilt_settings_set_frequency_range(&s, lower, upper);
    fLowerFrequency = s.lower_frequency, fUpperFrequency = s.upper_frequency, bSync = s.sync != 0;
}

void SpectralTilt::set_norm(stlt_norm_t norm)   { enNorm = norm, bSync = true; }

void SpectralTilt::set_slope(float slope, stlt_slope_unit_t slopeType)
{
    if ((slope == fSlopeVal) && (slopeType == enSlopeUnit))
        return;
    fSlopeVal = slope, enSlopeUnit = slopeType, bSync = true;
}

void SpectralTilt::set_order(size_t order)
{
    if (order == nOrder)
        return;
    nOrder = order, bSync = true;
}

float SpectralTilt::bilinear_coefficient(float angularFrequency, float samplerate)      // :150-153
{
    return angularFrequency / tanf(0.5f * angularFrequency / samplerate);
}

SpectralTilt::bilinear_spec_t SpectralTilt::compute_bilinear_element(float negZero, float negPole)  // :156-178
{
    bilinear_spec_t spec;
    spec.b0 = negZero, spec.b1 = 1.0f;
    spec.a0 = negPole, spec.a1 = 1.0f;
    return spec;
}

float SpectralTilt::digital_biquad_gain(dsp::biquad_x1_t *digitalbq, float frequency)
{
    const mi_spectral_tilt_settings_t s = TILT_SETTINGS();
    float gain = 0.0f;
    mi_spectral_tilt_settings_section_gain(&s, reinterpret_cast<const mi_biquad_x1_t *>(digitalbq), frequency, &gain);
    return gain;
}

void SpectralTilt::normalise_digital_biquad(dsp::biquad_x1_t *digitalbq)
{
    const mi_spectral_tilt_settings_t s = TILT_SETTINGS();
    mi_spectral_tilt_settings_normalise_section(&s, reinterpret_cast<mi_biquad_x1_t *>(digitalbq));
}

void SpectralTilt::update_settings()                            // :254-375
{
    if (!bSync)
        return;
    mi_spectral_tilt_settings_t s = TILT_SETTINGS();
    int designed = 0;
    if (mi_spectral_tilt_settings_update(&s, &designed) != MI_OK)
        return;
    nOrder = size_t(s.order);
    fSlopeNepNep = s.slope_nep_nep;
    fLowerFrequency = s.lower_frequency, fUpperFrequency = s.upper_frequency;
    bBypass = s.bypass != 0, bSync = s.sync != 0;
    if (!designed)
        return;
    sFilter.begin();
    for (uint32_t i = 0; i < s.n_sections; ++i)
    {
        dsp::biquad_x1_t *q = sFilter.add_chain();
        if (q == NULL)
            return;
        memcpy(q, &s.sections[i], sizeof(*q));
    }
    sFilter.end(true);
}

void SpectralTilt::process_add(float *dst, const float *src, size_t count)     // :377-407
{
    update_settings();
    if (src == NULL)
        return;
    if (bBypass)
    {
        for (size_t i = 0; i < count; ++i)
            dst[i] = dst[i] + src[i];
        return;
    }
    std::vector<float> tmp(count);                              // (the reference's chunks of 256 are one stream to the filter)
    sFilter.process(tmp.data(), src, count);
    for (size_t i = 0; i < count; ++i)
        dst[i] = dst[i] + tmp[i];
}

void SpectralTilt::process_mul(float *dst, const float *src, size_t count)     // :409-439
{
    update_settings();
    if (src == NULL)
    {
        for (size_t i = 0; i < count; ++i)
            dst[i] = 0.0f;
        return;
    }
    if (bBypass)
    {
        for (size_t i = 0; i < count; ++i)
            dst[i] = dst[i] * src[i];
        return;
    }
    std::vector<float> tmp(count);
    sFilter.process(tmp.data(), src, count);
    for (size_t i = 0; i < count; ++i)
        dst[i] = dst[i] * tmp[i];
}

void SpectralTilt::process_overwrite(float *dst, const float *src, size_t count)   // :441-451
{
    update_settings();
    if (src == NULL)
    {
        for (size_t i = 0; i < count; ++i)
            dst[i] = 0.0f;
    }
    else if (bBypass)
    {
        if (dst != src)
            memmove(dst, src, count * sizeof(float));
    }
    else
        sFilter.process(dst, src, count);
}

void SpectralTilt::complex_transfer_calc(float *re, float *im, float f)         // :453-503
{
    mi_spectral_tilt_settings_t s = TILT_SETTINGS();
    for (size_t i = 0, n = sFilter.size(); i < n && i < MI_STLT_MAX_SECTIONS; ++i)
    {
        const dsp::biquad_x1_t *q = sFilter.chain(i);
        if (q != NULL)
            memcpy(&s.sections[s.n_sections++], q, sizeof(*q));
    }
    mi_spectral_tilt_settings_freq_chart(&s, re, im, NULL, &f, 1);
}

void SpectralTilt::freq_chart(float *re, float *im, const float *f, size_t count)
{
    update_settings();
    for (size_t i = 0; i < count; ++i)
        complex_transfer_calc(&re[i], &im[i], f[i]);
}

void SpectralTilt::freq_chart(float *c, const float *f, size_t count)
{
    update_settings();
    for (size_t i = 0; i < count; ++i)
        complex_transfer_calc(&c[2 * i], &c[2 * i + 1], f[i]);
}

void SpectralTilt::dump(IStateDumper *v) const                  // :525-543
{
    v->write("nOrder", nOrder);
    v->write("enSlopeType", enSlopeUnit);
    v->write("enNorm", enNorm);
    v->write("fSlopeVal", fSlopeVal);
    v->write("fSlopeNepNep", fSlopeNepNep);
    v->write("fLowerFrequency", fLowerFrequency);
    v->write("fUpperFrequency", fUpperFrequency);
    v->write("nSampleRate", nSampleRate);
    v->write_object("sFilter", &sFilter);
    v->write("bBypass", bBypass);
    v->write("bSync", bSync);
}

} // namespace dspu
} // namespace lsp
