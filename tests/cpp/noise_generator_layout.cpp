// sizeof and offsetof of lsp::dspu::SpectralTilt and lsp::dspu::NoiseGenerator, and what the host side of the two classes does with no
// device: compiled against this library's headers (and, where the reference tree exists, against the reference's: the same lines
// come out; tests/golden/make_noise_generator_vectors.py records them from there).
//   noise_generator_layout            sizeof and offsets of both classes and of NoiseGenerator's four parameter structs
//   noise_generator_layout behaviour  fresh objects, the setters and the UPD_* bits they raise, init(), the dump keys of fresh objects
#define private public
#define protected public
#include <lsp-plug.in/dsp-units/noise/Generator.h>
#undef private
#undef protected
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <string>

using namespace lsp;
using namespace lsp::dspu;

struct keys: public IStateDumper
{
    std::string seen;
    int depth = 0;
    void note(const char *n) { seen += " "; seen += std::to_string(depth); seen += ":"; seen += n; }
    void begin_object(const char *n, const void *, size_t) override { note(n); ++depth; }
    void begin_object(const void *, size_t) override    { ++depth; }
    void end_object() override                          { --depth; }
    void begin_array(const char *n, const void *, size_t) override { note(n); ++depth; }
    void begin_array(const void *, size_t) override     { ++depth; }
    void end_array() override                           { --depth; }
    void write(const char *n, const void *) override    { note(n); }
    void write(const char *n, bool) override            { note(n); }
    void write(const char *n, unsigned char) override   { note(n); }
    void write(const char *n, signed int) override      { note(n); }
    void write(const char *n, unsigned int) override    { note(n); }
    void write(const char *n, unsigned long) override   { note(n); }
    void write(const char *n, unsigned long long) override { note(n); }
    void write(const char *n, float) override           { note(n); }
};

static unsigned fb(float f) { unsigned u; memcpy(&u, &f, 4); return u; }

static void tilt(const char *name, const SpectralTilt &t)
{
    printf("%s %zu %d %d %u %u %u %u %zu %d %d\n", name, t.nOrder, int(t.enSlopeUnit), int(t.enNorm), fb(t.fSlopeVal), fb(t.fSlopeNepNep),
           fb(t.fLowerFrequency), fb(t.fUpperFrequency), t.nSampleRate, int(t.bBypass), int(t.bSync));
}

static void generator(const char *name, const NoiseGenerator &g)
{
    printf("%s %d %llu %u %d %u %d %llu %d %d %u %u %d %u %d %zu %u %d %zu %d %u %u %zu\n", name, int(g.sMLSParams.nBits), (unsigned long long)g.sMLSParams.nSeed,
           g.sLCGParams.nSeed, int(g.sLCGParams.enDistribution), g.sVelvetParams.nRandSeed, int(g.sVelvetParams.nMLSnBits),
           (unsigned long long)g.sVelvetParams.nMLSseed, int(g.sVelvetParams.enCore), int(g.sVelvetParams.enVelvetType), fb(g.sVelvetParams.fWindowWidth_s),
           fb(g.sVelvetParams.fARNdelta), int(g.sVelvetParams.bCrush), fb(g.sVelvetParams.fCrushProb), int(g.sColorParams.enColor), g.sColorParams.nOrder,
           fb(g.sColorParams.fSlope), int(g.sColorParams.enSlopeUnit), g.nSampleRate, int(g.enGenerator), fb(g.fAmplitude), fb(g.fOffset), g.nUpdate);
}

int main(int argc, char **argv)
{
    if (argc == 1)
    {
        typedef NoiseGenerator N;
        printf("sizeof %zu %zu %zu %zu %zu %zu %zu\n", sizeof(SpectralTilt), sizeof(N), sizeof(N::mls_params_t), sizeof(N::lcg_params_t),
               sizeof(N::velvet_params_t), sizeof(N::color_params_t), sizeof(SpectralTilt::bilinear_spec_t));
        printf("offsetof_tilt %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", offsetof(SpectralTilt, nOrder), offsetof(SpectralTilt, enSlopeUnit),
               offsetof(SpectralTilt, enNorm), offsetof(SpectralTilt, fSlopeVal), offsetof(SpectralTilt, fSlopeNepNep), offsetof(SpectralTilt, fLowerFrequency),
               offsetof(SpectralTilt, fUpperFrequency), offsetof(SpectralTilt, nSampleRate), offsetof(SpectralTilt, bBypass), offsetof(SpectralTilt, bSync),
               offsetof(SpectralTilt, sFilter));
        printf("offsetof_generator %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", offsetof(N, sMLS), offsetof(N, sLCG), offsetof(N, sVelvetNoise),
               offsetof(N, sColorFilter), offsetof(N, sMLSParams), offsetof(N, sLCGParams), offsetof(N, sVelvetParams), offsetof(N, sColorParams),
               offsetof(N, nSampleRate), offsetof(N, enGenerator), offsetof(N, fAmplitude), offsetof(N, fOffset), offsetof(N, nUpdate));
        printf("offsetof_params %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", offsetof(N::mls_params_t, nBits), offsetof(N::mls_params_t, nSeed),
               offsetof(N::lcg_params_t, nSeed), offsetof(N::lcg_params_t, enDistribution), offsetof(N::velvet_params_t, nRandSeed),
               offsetof(N::velvet_params_t, nMLSnBits), offsetof(N::velvet_params_t, nMLSseed), offsetof(N::velvet_params_t, enCore),
               offsetof(N::velvet_params_t, enVelvetType), offsetof(N::velvet_params_t, fWindowWidth_s), offsetof(N::velvet_params_t, fARNdelta),
               offsetof(N::velvet_params_t, bCrush), offsetof(N::velvet_params_t, fCrushProb), offsetof(N::color_params_t, enColor),
               offsetof(N::color_params_t, nOrder), offsetof(N::color_params_t, fSlope), offsetof(N::color_params_t, enSlopeUnit));
        return 0;
    }
    // ---- behaviour with no device (neither object is init()ed: sFilter has no bank)
    SpectralTilt t;
    tilt("tilt_fresh", t);
    t.bSync = false;
    t.set_order(1), t.set_slope(0.5f, STLT_SLOPE_UNIT_NEPER_PER_NEPER), t.set_lower_frequency(0.1f), t.set_upper_frequency(20.0e3f), t.set_sample_rate(size_t(-1));
    tilt("tilt_same", t);                                   // the values it has: bSync stays clear
    t.set_norm(STLT_NORM_AUTO);
    tilt("tilt_norm", t);                                   // set_norm does not compare
    t.bSync = false;
    t.set_frequency_range(20.0f, 18000.0f);
    tilt("tilt_range", t);                                  // swapped the wrong way round
    t.bSync = false;
    t.set_frequency_range(18000.0f, 20.0f);
    tilt("tilt_range_again", t);                            // equal to the members: nothing
    t.set_order(7), t.set_slope(-3.0f, STLT_SLOPE_UNIT_DB_PER_OCTAVE), t.set_sample_rate(48000);
    tilt("tilt_set", t);
    keys kt;
    t.dump(&kt);
    printf("SpectralTilt%s\n", kt.seen.c_str());

    NoiseGenerator g;
    generator("generator_fresh", g);
    g.nUpdate = 0;
    g.set_sample_rate(0), g.set_mls_n_bits(0), g.set_mls_seed(0), g.set_lcg_distribution(LCG_UNIFORM), g.set_velvet_type(VN_VELVET_OVN);
    g.set_velvet_window_width(0.1f), g.set_velvet_arn_delta(0.5f), g.set_velvet_crush(false), g.set_velvet_crushing_probability(0.5f);
    g.set_noise_color(NG_COLOR_WHITE), g.set_coloring_order(50), g.set_color_slope(0.0f, STLT_SLOPE_UNIT_NEPER_PER_NEPER), g.set_amplitude(1.0f), g.set_offset(0.0f);
    g.set_generator(NG_GEN_VELVET);
    generator("generator_same", g);                         // the values it has: nUpdate stays 0; set_generator raises nothing
    printf("raised");
    #define RAISED(call) g.nUpdate = 0; call; printf(" %zu", g.nUpdate)
    RAISED(g.set_sample_rate(44100)); RAISED(g.set_mls_n_bits(9)); RAISED(g.set_mls_seed(5)); RAISED(g.set_lcg_distribution(LCG_GAUSSIAN));
    RAISED(g.set_velvet_type(VN_VELVET_ARN)); RAISED(g.set_velvet_window_width(0.01f)); RAISED(g.set_velvet_arn_delta(0.25f)); RAISED(g.set_velvet_crush(true));
    RAISED(g.set_velvet_crushing_probability(0.3f)); RAISED(g.set_noise_color(NG_COLOR_PINK)); RAISED(g.set_coloring_order(12));
    RAISED(g.set_color_slope(-3.0f, STLT_SLOPE_UNIT_DB_PER_OCTAVE)); RAISED(g.set_amplitude(-2.0f)); RAISED(g.set_offset(-0.0f)); RAISED(g.set_generator(NG_GEN_MLS));
    printf("\n");
    generator("generator_set", g);
    keys kg;
    g.dump(&kg);
    printf("NoiseGenerator%s\n", kg.seen.c_str());
    return 0;
}
