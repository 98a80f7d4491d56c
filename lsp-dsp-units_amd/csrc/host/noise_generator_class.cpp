// lsp::dspu::NoiseGenerator (src/main/noise/Generator.cpp).  The object holds this library's MLS, LCG, Velvet and SpectralTilt by value;
// what is here is which setter raises which UPD_* bit, what update_settings() tells the four units, and the composition of a call:
// the unit that enGenerator names draws the row (on its one-channel bank of the calling thread), sColorFilter colours it in place,
// and with a source the call is cut into chunks of BUF_LIM_SIZE that are added to or multiplied with the source on the host.
#include <lsp-plug.in/dsp-units/noise/Generator.h>
#include <lsp-plug.in/dsp-units/units.h>

#pragma clang fp contract(off)

namespace lsp
{
namespace dspu
{
namespace
{
    constexpr size_t BUF_LIM_SIZE = 256;

    inline bool coloured(ng_color_t color)                      // do_process()'s and freq_chart()'s switch: default: is white
    {
        switch (color)
        {
            case NG_COLOR_PINK: case NG_COLOR_RED: case NG_COLOR_BLUE: case NG_COLOR_VIOLET: case NG_COLOR_ARBITRARY: return true;
            default: return false;
        }
    }
}

NoiseGenerator::NoiseGenerator()    { construct(); }
NoiseGenerator::~NoiseGenerator()   { destroy(); }

void NoiseGenerator::construct()                                // :44-78
{
    sMLS.construct();
    sLCG.construct();
    sVelvetNoise.construct();
    sColorFilter.construct();
    sMLSParams.nBits = 0, sMLSParams.nSeed = 0;
    sLCGParams.nSeed = 0, sLCGParams.enDistribution = LCG_UNIFORM;
    sVelvetParams.nRandSeed = 0, sVelvetParams.nMLSnBits = 0, sVelvetParams.nMLSseed = 0;
    sVelvetParams.enCore = VN_CORE_LCG, sVelvetParams.enVelvetType = VN_VELVET_OVN;
    sVelvetParams.fWindowWidth_s = 0.1f, sVelvetParams.fARNdelta = 0.5f, sVelvetParams.bCrush = false, sVelvetParams.fCrushProb = 0.5f;
    sColorParams.enColor = NG_COLOR_WHITE, sColorParams.nOrder = 50, sColorParams.fSlope = 0.0f;
    sColorParams.enSlopeUnit = STLT_SLOPE_UNIT_NEPER_PER_NEPER;
    nSampleRate = 0;
    enGenerator = NG_GEN_LCG;
    fAmplitude = 1.0f, fOffset = 0.0f;
    nUpdate = UPD_ALL;
}

void NoiseGenerator::destroy()
{
    sMLS.destroy();
    sLCG.destroy();
    sVelvetNoise.destroy();
    sColorFilter.destroy();
}

void NoiseGenerator::init(uint8_t mls_n_bits, MLS::mls_t mls_seed, uint32_t lcg_seed,
                          uint32_t velvet_rand_seed, uint8_t velvet_mls_n_bits, MLS::mls_t velvet_mls_seed)    // :88-108
{
    sMLSParams.nBits = mls_n_bits, sMLSParams.nSeed = mls_seed;
    sLCGParams.nSeed = lcg_seed;
    sLCG.init(lcg_seed);
    sVelvetParams.nRandSeed = velvet_rand_seed, sVelvetParams.nMLSnBits = velvet_mls_n_bits, sVelvetParams.nMLSseed = velvet_mls_seed;
    sVelvetNoise.init(velvet_rand_seed, velvet_mls_n_bits, velvet_mls_seed);
    sColorFilter.init();
    sColorFilter.set_norm(STLT_NORM_AUTO);
    nUpdate = UPD_ALL;
}

void NoiseGenerator::init()                                     // :110-122
{
    sMLSParams.nBits = uint8_t(sMLS.maximum_number_of_bits());
    sMLSParams.nSeed = 0;                                       // the MLS makes its default seed of it
    sLCG.init();
    sVelvetNoise.init();
    sColorFilter.init();
    sColorFilter.set_norm(STLT_NORM_AUTO);
    nUpdate = UPD_ALL;
}

// a setter: nothing happens if the member has the value, otherwise it is set and `bits` are raised
#define NG_SET(member, value, bits) do { if ((value) == (member)) return; (member) = (value); nUpdate |= (bits); } while (0)

void NoiseGenerator::set_sample_rate(size_t sr)                         { NG_SET(nSampleRate, sr, UPD_COLOR | UPD_VELVET); }
void NoiseGenerator::set_mls_n_bits(uint8_t nbits)                      { NG_SET(sMLSParams.nBits, nbits, UPD_MLS); }
void NoiseGenerator::set_mls_seed(MLS::mls_t seed)                      { NG_SET(sMLSParams.nSeed, seed, UPD_MLS); }
void NoiseGenerator::set_lcg_distribution(lcg_dist_t dist)              { NG_SET(sLCGParams.enDistribution, dist, UPD_LCG); }
void NoiseGenerator::set_velvet_type(vn_velvet_type_t type)             { NG_SET(sVelvetParams.enVelvetType, type, UPD_VELVET); }
void NoiseGenerator::set_velvet_window_width(float width)               { NG_SET(sVelvetParams.fWindowWidth_s, width, UPD_VELVET); }
void NoiseGenerator::set_velvet_arn_delta(float delta)                  { NG_SET(sVelvetParams.fARNdelta, delta, UPD_VELVET); }
void NoiseGenerator::set_velvet_crush(bool crush)                       { NG_SET(sVelvetParams.bCrush, crush, UPD_VELVET); }
void NoiseGenerator::set_velvet_crushing_probability(float prob)        { NG_SET(sVelvetParams.fCrushProb, prob, UPD_VELVET); }
void NoiseGenerator::set_noise_color(ng_color_t color)                  { NG_SET(sColorParams.enColor, color, UPD_COLOR); }
void NoiseGenerator::set_coloring_order(size_t order)                   { NG_SET(sColorParams.nOrder, order, UPD_COLOR); }
void NoiseGenerator::set_amplitude(float amplitude)                     { NG_SET(fAmplitude, amplitude, UPD_OTHER); }
void NoiseGenerator::set_offset(float offset)                           { NG_SET(fOffset, offset, UPD_OTHER); }

void NoiseGenerator::set_generator(ng_generator_t core)         { enGenerator = core; }     // raises nothing, :205-211

void NoiseGenerator::set_color_slope(float slope, stlt_slope_unit_t unit)
{
    if ((slope == sColorParams.fSlope) && (unit == sColorParams.enSlopeUnit))
        return;
    sColorParams.fSlope = slope, sColorParams.enSlopeUnit = unit;
    nUpdate |= UPD_COLOR;
}

void NoiseGenerator::update_settings()                          // :259-345
{
    if (!nUpdate)
        return;
    sMLS.set_amplitude(fAmplitude);
    sMLS.set_offset(fOffset);
    if (nUpdate & UPD_MLS)
    {
        sMLS.set_n_bits(sMLSParams.nBits);
        sMLS.set_state(sMLSParams.nSeed);
    }
    sLCG.set_amplitude(fAmplitude);
    sLCG.set_offset(fOffset);
    if (nUpdate & UPD_LCG)
        sLCG.set_distribution(sLCGParams.enDistribution);
    sVelvetNoise.set_amplitude(fAmplitude);
    sVelvetNoise.set_offset(fOffset);
    if (nUpdate & UPD_VELVET)
    {
        sVelvetNoise.set_core_type(sVelvetParams.enCore);
        sVelvetNoise.set_velvet_type(sVelvetParams.enVelvetType);
        sVelvetNoise.set_velvet_window_width(seconds_to_samples(nSampleRate, sVelvetParams.fWindowWidth_s));
        sVelvetNoise.set_delta_value(sVelvetParams.fARNdelta);
        sVelvetNoise.set_crush(sVelvetParams.bCrush);
        sVelvetNoise.set_crush_probability(sVelvetParams.fCrushProb);
    }
    if (nUpdate & UPD_COLOR)
    {
        sColorFilter.set_sample_rate(nSampleRate);
        float slope = 0.0f;
        stlt_slope_unit_t unit = STLT_SLOPE_UNIT_NEPER_PER_NEPER;
        switch (sColorParams.enColor)
        {
            case NG_COLOR_PINK:         slope = -0.5f; break;
            case NG_COLOR_RED:          slope = -1.0f; break;
            case NG_COLOR_BLUE:         slope = 0.5f; break;
            case NG_COLOR_VIOLET:       slope = 1.0f; break;
            case NG_COLOR_ARBITRARY:    slope = sColorParams.fSlope, unit = sColorParams.enSlopeUnit; break;
            default:                    break;
        }
        sColorFilter.set_order(sColorParams.nOrder);
        sColorFilter.set_slope(slope, unit);
        sColorFilter.set_lower_frequency(10.0f);
        sColorFilter.set_upper_frequency(0.9f * 0.5f * nSampleRate);
    }
    nUpdate = 0;
}

void NoiseGenerator::do_process(float *dst, size_t count)       // :347-379
{
    switch (enGenerator)
    {
        case NG_GEN_MLS:    sMLS.process_overwrite(dst, count); break;
        case NG_GEN_VELVET: sVelvetNoise.process_overwrite(dst, count); break;
        default:            sLCG.process_overwrite(dst, count); break;
    }
    if (coloured(sColorParams.enColor))
        sColorFilter.process_overwrite(dst, dst, count);
}

void NoiseGenerator::process_add(float *dst, const float *src, size_t count)   // :381-405
{
    update_settings();
    if (src == NULL)
    {
        do_process(dst, count);
        return;
    }
    float tmp[BUF_LIM_SIZE];
    for (size_t at = 0; at < count; )
    {
        const size_t n = (count - at < BUF_LIM_SIZE) ? count - at : BUF_LIM_SIZE;
        do_process(tmp, n);
        for (size_t i = 0; i < n; ++i)
            dst[at + i] = tmp[i] + src[at + i];
        at += n;
    }
}

void NoiseGenerator::process_mul(float *dst, const float *src, size_t count)   // :407-431
{
    update_settings();
    if (src == NULL)
    {
        for (size_t i = 0; i < count; ++i)
            dst[i] = 0.0f;
        return;
    }
    float tmp[BUF_LIM_SIZE];
    for (size_t at = 0; at < count; )
    {
        const size_t n = (count - at < BUF_LIM_SIZE) ? count - at : BUF_LIM_SIZE;
        do_process(tmp, n);
        for (size_t i = 0; i < n; ++i)
            dst[at + i] = tmp[i] * src[at + i];
        at += n;
    }
}

void NoiseGenerator::process_overwrite(float *dst, size_t count)
{
    update_settings();
    do_process(dst, count);
}

void NoiseGenerator::freq_chart(float *re, float *im, const float *f, size_t count)    // :440-458
{
    if (coloured(sColorParams.enColor))
    {
        sColorFilter.freq_chart(re, im, f, count);
        return;
    }
    for (size_t i = 0; i < count; ++i)
        re[i] = 1.0f, im[i] = 0.0f;
}

void NoiseGenerator::freq_chart(float *c, const float *f, size_t count)        // :460-477
{
    if (coloured(sColorParams.enColor))
    {
        sColorFilter.freq_chart(c, f, count);
        return;
    }
    for (size_t i = 0; i < count; ++i)
        c[2 * i] = 1.0f, c[2 * i + 1] = 0.0f;
}

void NoiseGenerator::dump(IStateDumper *v) const                // :479-528
{
    v->write("nSampleRate", nSampleRate);
    v->write_object("sMLS", &sMLS);
    v->write_object("sLCG", &sLCG);
    v->write_object("sVelvetNoise", &sVelvetNoise);
    v->begin_object("sMLSParams", &sMLSParams, sizeof(sMLSParams));
    {
        v->write("nBits", sMLSParams.nBits);
        v->write("nSeed", sMLSParams.nSeed);
    }
    v->end_object();
    v->begin_object("sLCGParams", &sLCGParams, sizeof(sLCGParams));
    {
        v->write("nSeed", sLCGParams.nSeed);
        v->write("enDistribution", sLCGParams.enDistribution);
    }
    v->end_object();
    v->begin_object("sVelvetParams", &sVelvetParams, sizeof(sVelvetParams));
    {
        v->write("nRandSeed", sVelvetParams.nRandSeed);
        v->write("nMLSnBits", sVelvetParams.nMLSnBits);
        v->write("nMLSseed", sVelvetParams.nMLSseed);
        v->write("enCore", sVelvetParams.enCore);
        v->write("enVelvetType", sVelvetParams.enVelvetType);
        v->write("fWindowWidth_s", sVelvetParams.fWindowWidth_s);
        v->write("fARNdelta", sVelvetParams.fARNdelta);
        v->write("bCrush", sVelvetParams.bCrush);
        v->write("fCrushProb", sVelvetParams.fCrushProb);
    }
    v->end_object();
    v->begin_object("sColorParams", &sColorParams, sizeof(sColorParams));
    {
        v->write("enColor", sColorParams.enColor);
        v->write("nOrder", sColorParams.nOrder);
        v->write("fSlope", sColorParams.fSlope);
        v->write("enSlopeUnit", sColorParams.enSlopeUnit);
    }
    v->end_object();
    v->write("enGenerator", enGenerator);
    v->write("fAmplitude", fAmplitude);
    v->write("fOffset", fOffset);
}

} // namespace dspu
} // namespace lsp
