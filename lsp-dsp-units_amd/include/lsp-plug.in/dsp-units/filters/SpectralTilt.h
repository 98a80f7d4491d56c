// lsp::dspu::SpectralTilt on the GPU library (one filter, host pointers; the device-resident form for many channels is
// mi_spectral_tilt_bank_*).  update_settings() is the library's host designer (mi_spectral_tilt_settings_update: the reference's
// update_settings() line for line, quirks included), whose sections go to sFilter -- this library's FilterBank, a one-channel
// biquad bank on the device, exact or fast by the process-wide default (mi_dspu_set_exact_iir_default) -- with end(true).  The
// three process entries are the reference's: the second operand is dst itself.
#ifndef MI_LSP_PLUG_IN_DSP_UNITS_FILTERS_SPECTRALTILT_H_
#define MI_LSP_PLUG_IN_DSP_UNITS_FILTERS_SPECTRALTILT_H_

#include <lsp-plug.in/dsp-units/version.h>
#include <lsp-plug.in/dsp-units/filters/FilterBank.h>
#include <lsp-plug.in/dsp-units/iface/IStateDumper.h>

namespace lsp
{
    namespace dspu
    {
        enum stlt_slope_unit_t
        {
            STLT_SLOPE_UNIT_NEPER_PER_NEPER,
            STLT_SLOPE_UNIT_DB_PER_OCTAVE,
            STLT_SLOPE_UNIT_DB_PER_DECADE,
            STLT_SLOPE_UNIT_NONE,       // bypass
            STLT_SLOPE_UNIT_MAX
        };

        enum stlt_norm_t
        {
            STLT_NORM_AT_DC,
            STLT_NORM_AT_20_HZ,
            STLT_NORM_AT_1_KHZ,
            STLT_NORM_AT_20_KHZ,
            STLT_NORM_AT_NYQUIST,
            STLT_NORM_AUTO,             // at 20 Hz for a falling slope, at 20 kHz for a rising one
            STLT_NORM_NONE,
            STLT_NORM_MAX
        };

        class LSP_DSP_UNITS_PUBLIC SpectralTilt
        {
            protected:
                typedef struct bilinear_spec_t
                {
                    float b0;
                    float b1;

                    float a0;
                    float a1;
                } bq_spec_t;

            // Binary layout: data members and their order as in the reference class (tests/cpp/noise_generator_layout.cpp).
            private:
                size_t              nOrder;

                stlt_slope_unit_t   enSlopeUnit;
                stlt_norm_t         enNorm;
                float               fSlopeVal;
                float               fSlopeNepNep;

                float               fLowerFrequency;
                float               fUpperFrequency;

                size_t              nSampleRate;

                bool                bBypass;
                bool                bSync;

                dspu::FilterBank    sFilter;

            public:
                explicit SpectralTilt();
                SpectralTilt(const SpectralTilt &) = delete;
                SpectralTilt(SpectralTilt &&) = delete;
                ~SpectralTilt();

                SpectralTilt & operator = (const SpectralTilt &) = delete;
                SpectralTilt & operator = (SpectralTilt &&) = delete;

                void construct();
                void destroy();

                void init();                                    // sFilter.init(128)

            protected:
                float               bilinear_coefficient(float angularFrequency, float samplerate);
                bilinear_spec_t     compute_bilinear_element(float negZero, float negPole);
                float               digital_biquad_gain(dsp::biquad_x1_t *digitalbq, float frequency);
                void                normalise_digital_biquad(dsp::biquad_x1_t *digitalbq);
                void                complex_transfer_calc(float *re, float *im, float f);
                void                update_settings();

            public:
                void set_order(size_t order);                   // raised to even, clamped to 128 at the update
                void set_slope(float slope, stlt_slope_unit_t slopeType);
                void set_norm(stlt_norm_t norm);
                void set_lower_frequency(float lowerFrequency);
                void set_upper_frequency(float upperFrequency);
                void set_frequency_range(float lower, float upper);
                void set_sample_rate(size_t sr);

                void process_add(float *dst, const float *src, size_t count);          // dst += filter(src); NULL src: nothing
                void process_mul(float *dst, const float *src, size_t count);          // dst *= filter(src); NULL src: zero fill
                void process_overwrite(float *dst, const float *src, size_t count);    // dst = filter(src); NULL src: zero fill

                void freq_chart(float *re, float *im, const float *f, size_t count);
                void freq_chart(float *c, const float *f, size_t count);

                void dump(IStateDumper *v) const;
        };
    }
}

#endif
