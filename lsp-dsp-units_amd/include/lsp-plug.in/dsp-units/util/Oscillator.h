// lsp::dspu::Oscillator on the GPU library (one oscillator, host pointers; the device-resident form for many channels is
// mi_oscillator_bank_*).  init() makes a bank of one channel; the setters and update_settings() work on the members, with the
// arithmetic of mi_oscillator_settings_update (the reference's, its mix of double and float kept); process_*() hand the members
// to the bank where they changed, stage the caller's rows on the device and run the bank's kernel.  nPhaseAcc is the
// reference's: it moves on the host by the call's samples as on the device, and a value that differs from what the device holds
// reaches it before the next call.  vProcessBuffer and vSynthBuffer stay NULL (the rows are on the device); pData is the
// handle.  The band-limited functions run through the bank's own oversampler; sOver and sOverGetPeriods carry the rate and
// the mode as in the reference.
// Where the reference's behaviour is undefined the bank's holds (mi_dspu.h): a trapezoid sample takes the first branch that
// holds, a word that does not fit uint32_t converts through int64_t.  A sample rate that was never set is size_t(-1) in the
// arithmetic, as in the reference.  get_periods() is the bank's: a call behind skipped periods that fits one buffer has the
// reference's values; where the reference's read position runs in front of its buffer (every call that refills) a position
// there reads 0.0f, and a period that is not positive and finite writes nothing (mi_dspu.h).
#ifndef MI_LSP_PLUG_IN_DSP_UNITS_UTIL_OSCILLATOR_H_
#define MI_LSP_PLUG_IN_DSP_UNITS_UTIL_OSCILLATOR_H_

#include <lsp-plug.in/dsp-units/version.h>
#include <lsp-plug.in/dsp-units/iface/IStateDumper.h>
#include <lsp-plug.in/dsp-units/util/Oversampler.h>

namespace lsp
{
    namespace dspu
    {
        enum fg_function_t
        {
            FG_SINE, FG_COSINE, FG_SQUARED_SINE, FG_SQUARED_COSINE, FG_RECTANGULAR, FG_SAWTOOTH, FG_TRAPEZOID, FG_PULSETRAIN,
            FG_PARABOLIC, FG_BL_RECTANGULAR, FG_BL_SAWTOOTH, FG_BL_TRAPEZOID, FG_BL_PULSETRAIN, FG_BL_PARABOLIC
        };

        enum dc_reference_t
        {
            DC_WAVEDC,          // the DC offset counts from the wave's own DC
            DC_ZERO             // the DC offset counts from 0
        };

        class LSP_DSP_UNITS_PUBLIC Oscillator
        {
            // Binary layout: data members and their order as in the reference class (util/Oscillator.h of lsp-dsp-units), 608
            // bytes on LP64 with the two Oversampler objects embedded by value (host/oscillator_class.cpp asserts the size).
            protected:
                typedef uint32_t phacc_t;

                typedef struct squared_sinusoid_t { bool bInvert; float fAmplitude; float fWaveDC; } squared_sinusoid_t;
                typedef struct rectangular_t { float fDutyRatio; phacc_t nDutyWord; float fWaveDC; float fBLPeakAtten; } rectangular_t;
                typedef struct sawtooth_t { float fWidth; phacc_t nWidthWord; float fCoeffs[4]; float fWaveDC; float fBLPeakAtten; } sawtooth_t;
                typedef struct trapezoid_t
                {
                    float fRaiseRatio; float fFallRatio; phacc_t nPoints[4]; float fCoeffs[4]; float fWaveDC; float fBLPeakAtten;
                } trapezoid_t;
                typedef struct pulse_t { float fPosWidthRatio; float fNegWidthRatio; phacc_t nTrainPoints[3]; float fWaveDC; float fBLPeakAtten; } pulse_t;
                typedef struct parabolic_t
                {
                    bool bInvert; float fAmplitude; float fWidth; phacc_t nWidthWord; float fWaveDC; float fBLPeakAtten;
                } parabolic_t;

            private:
                fg_function_t       enFunction;
                float               fAmplitude;
                float               fFrequency;
                float               fDCOffset;
                dc_reference_t      enDCReference;
                float               fReferencedDC;
                float               fInitPhase;

                size_t              nSampleRate;
                phacc_t             nPhaseAcc;
                uint8_t             nPhaseAccBits;
                uint8_t             nPhaseAccMaxBits;
                phacc_t             nPhaseAccMask;
                float               fAcc2Phase;

                phacc_t             nFreqCtrlWord;
                phacc_t             nInitPhaseWord;

                squared_sinusoid_t  sSquaredSinusoid;
                rectangular_t       sRectangular;
                sawtooth_t          sSawtooth;
                trapezoid_t         sTrapezoid;
                pulse_t             sPulse;
                parabolic_t         sParabolic;

                float              *vProcessBuffer;         // NULL: the rows are on the device
                float              *vSynthBuffer;           // NULL
                uint8_t            *pData;                  // the bank of one channel and its staging rows

                Oversampler         sOver;
                Oversampler         sOverGetPeriods;
                size_t              nOversampling;
                over_mode_t         enOverMode;
                phacc_t             nFreqCtrlWord_Over;

                bool                bSync;

            protected:
                void do_process(Oversampler *os, float *dst, size_t count);

            public:
                explicit Oscillator();
                Oscillator(const Oscillator &) = delete;
                Oscillator(Oscillator &&) = delete;
                ~Oscillator();

                Oscillator & operator = (const Oscillator &) = delete;
                Oscillator & operator = (Oscillator &&) = delete;

                void construct();           // valid on raw (e.g. zeroed) memory
                bool init();
                void destroy();

            public:
                inline bool needs_update() const
                {
                    return bSync;
                }

                void update_settings();

                inline void set_phase_accumulator_bits(uint8_t nBits)
                {
                    if ((nPhaseAccBits == nBits) || (nBits > nPhaseAccMaxBits))
                        return;

                    nPhaseAccBits   = nBits;
                    nPhaseAcc       = 0;
                    bSync           = true;
                }

                inline void set_sample_rate(size_t sr)
                {
                    if (nSampleRate == sr)
                        return;

                    nSampleRate = sr;
                    nPhaseAcc   = 0;
                    bSync       = true;
                }

                inline void reset_phase_accumulator() { nPhaseAcc = 0; }

                inline void set_function(fg_function_t function)
                {
                    enFunction  = function;
                    bSync       = true;
                }

                inline void set_frequency(float frequency)
                {
                    if (fFrequency == frequency)
                        return;

                    fFrequency      = frequency;
                    bSync           = true;
                }

                inline float get_exact_frequency() const
                {
                    return nSampleRate * nFreqCtrlWord * (1.0f / (nPhaseAccMask + 1.0f));
                }

                void set_phase(float phase);
                float get_exact_phase() const;
                void set_dc_offset(float dcOffset);
                void set_dc_reference(dc_reference_t dcReference);
                void set_squared_sinusoid_inversion(bool invert);
                void set_parabolic_inversion(bool invert);
                void set_duty_ratio(float dutyRatio);
                void set_width(float width);
                void set_trapezoid_ratios(float raise, float fall);
                void set_pulsetrain_ratios(float posWidthRatio, float negWidthRatio);
                void set_parabolic_width(float width);
                void set_oversampler_mode(over_mode_t mode);
                void set_amplitude(float amplitude);

                // `samples` values out of `periods` periods of the wave behind `periodsSkip` skipped ones, from the initial phase
                void get_periods(float *dst, size_t periods, size_t periodsSkip, size_t samples);

                // dst, src: host pointers to `count` floats; src may be NULL or dst
                void process_add(float *dst, const float *src, size_t count);
                void process_mul(float *dst, const float *src, size_t count);
                void process_overwrite(float *dst, size_t count);

                void dump(IStateDumper *v) const;
        };
    }
}

#endif
