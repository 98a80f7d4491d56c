// lsp::dspu::NoiseGenerator on the GPU library (one generator, host pointers; the device-resident form for many channels is
// mi_noise_generator_bank_*).  The object holds this library's MLS, LCG, Velvet and SpectralTilt by value, as the reference holds
// its own: update_settings() tells them what the UPD_* bits say, and a call draws from the one that enGenerator names -- whose
// rows run on its one-channel bank of the calling thread, state in before the row and back after it -- and colours the row with
// sColorFilter.  With a source the call is cut into the reference's chunks of 256, which only Velvet can tell from one call.
// Where the reference's behaviour is undefined: before init() the rows of the LCG and of Velvet stay untouched (Randomizer.h).
#ifndef MI_LSP_PLUG_IN_DSP_UNITS_NOISE_GENERATOR_H_
#define MI_LSP_PLUG_IN_DSP_UNITS_NOISE_GENERATOR_H_

#include <lsp-plug.in/dsp-units/version.h>
#include <lsp-plug.in/dsp-units/filters/SpectralTilt.h>
#include <lsp-plug.in/dsp-units/iface/IStateDumper.h>
#include <lsp-plug.in/dsp-units/noise/LCG.h>
#include <lsp-plug.in/dsp-units/noise/MLS.h>
#include <lsp-plug.in/dsp-units/noise/Velvet.h>

namespace lsp
{
    namespace dspu
    {
        enum ng_generator_t
        {
            NG_GEN_MLS,
            NG_GEN_LCG,
            NG_GEN_VELVET
        };

        enum ng_color_t
        {
            NG_COLOR_WHITE,
            NG_COLOR_PINK,
            NG_COLOR_RED,
            NG_COLOR_BLUE,
            NG_COLOR_VIOLET,
            NG_COLOR_ARBITRARY,         // the slope of set_color_slope()

            NG_COLOR_BROWN = NG_COLOR_RED,
            NG_COLOR_BROWNIAN = NG_COLOR_RED
        };

        class LSP_DSP_UNITS_PUBLIC NoiseGenerator
        {
            protected:
                enum update_t
                {
                    UPD_MLS     = 1 << 0,
                    UPD_LCG     = 1 << 1,
                    UPD_VELVET  = 1 << 2,
                    UPD_COLOR   = 1 << 3,
                    UPD_OTHER   = 1 << 4,

                    UPD_ALL     = UPD_MLS | UPD_LCG | UPD_VELVET | UPD_COLOR | UPD_OTHER
                };

                typedef struct mls_params_t
                {
                    uint8_t             nBits;
                    MLS::mls_t          nSeed;
                } mls_params_t;

                typedef struct lcg_params_t
                {
                    uint32_t            nSeed;
                    lcg_dist_t          enDistribution;
                } lcg_params_t;

                typedef struct velvet_params_t
                {
                    uint32_t            nRandSeed;
                    uint8_t             nMLSnBits;
                    MLS::mls_t          nMLSseed;
                    vn_core_t           enCore;
                    vn_velvet_type_t    enVelvetType;
                    float               fWindowWidth_s;
                    float               fARNdelta;
                    bool                bCrush;
                    float               fCrushProb;
                } velvet_params_t;

                typedef struct color_params_t
                {
                    ng_color_t          enColor;
                    size_t              nOrder;
                    float               fSlope;
                    stlt_slope_unit_t   enSlopeUnit;
                } color_params_t;

            // Binary layout: data members and their order as in the reference class (tests/cpp/noise_generator_layout.cpp).
            private:
                MLS                 sMLS;
                LCG                 sLCG;
                Velvet              sVelvetNoise;
                SpectralTilt        sColorFilter;

                mls_params_t        sMLSParams;
                lcg_params_t        sLCGParams;
                velvet_params_t     sVelvetParams;
                color_params_t      sColorParams;

                size_t              nSampleRate;
                ng_generator_t      enGenerator;

                float               fAmplitude;
                float               fOffset;

                size_t              nUpdate;

            public:
                explicit NoiseGenerator();
                NoiseGenerator(const NoiseGenerator &) = delete;
                NoiseGenerator(NoiseGenerator &&) = delete;
                ~NoiseGenerator();

                NoiseGenerator & operator = (const NoiseGenerator &) = delete;
                NoiseGenerator & operator = (NoiseGenerator &&) = delete;

                void construct();
                void destroy();

            protected:
                void do_process(float *dst, size_t count);
                void update_settings();

            public:
                void init(
                    uint8_t mls_n_bits, MLS::mls_t mls_seed,
                    uint32_t lcg_seed,
                    uint32_t velvet_rand_seed, uint8_t velvet_mls_n_bits, MLS::mls_t velvet_mls_seed);
                void init();                                    // time seeds, an MLS of 64 bits with the default seed

                void set_sample_rate(size_t sr);
                void set_mls_n_bits(uint8_t nbits);
                void set_mls_seed(MLS::mls_t seed);
                void set_lcg_distribution(lcg_dist_t dist);
                void set_velvet_type(vn_velvet_type_t type);
                void set_velvet_window_width(float width);      // seconds
                void set_velvet_arn_delta(float delta);
                void set_velvet_crush(bool crush);
                void set_velvet_crushing_probability(float prob);
                void set_generator(ng_generator_t core);
                void set_noise_color(ng_color_t color);
                void set_coloring_order(size_t order);
                void set_color_slope(float slope, stlt_slope_unit_t unit);
                void set_amplitude(float amplitude);
                void set_offset(float offset);

                void process_add(float *dst, const float *src, size_t count);  // dst = src + noise; NULL src: as process_overwrite
                void process_mul(float *dst, const float *src, size_t count);  // dst = src * noise; NULL src: zero fill
                void process_overwrite(float *dst, size_t count);

                void freq_chart(float *re, float *im, const float *f, size_t count);
                void freq_chart(float *c, const float *f, size_t count);

                void dump(IStateDumper *v) const;
        };
    }
}

#endif
