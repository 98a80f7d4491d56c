// lsp::dspu::Sidechain on the GPU library (one sidechain, host pointers; the device-resident form for many channels is
// mi_sidechain_bank_*).  The setters and update_settings() are host arithmetic; both process() overloads run on the device
// through a bank of one channel that the object makes at its first such call.  With a pre-equalizer set, the block process()
// is mi_sidechain_bank_premix, pPreEq->process() on the signed source, mi_sidechain_bank_process_premixed: the equalizer
// sits where the reference's block overload has it (Sidechain.cpp:183-333: every source of both stereo modes and the single
// input; not for in == NULL).  Inputs are finite: NaN is out of scope.
//
// The single-sample process(const float *) is a call of ONE sample through the block path.  The reference's own text for it
// (Sidechain.cpp:556-624) differs from its block overload in four places, and these are NOT reproduced:
//   * it counts the sample before it looks at nRefresh (++nRefresh >= REFRESH_RATE), so its refresh comes one sample earlier;
//   * it divides by float(nReactivity) (rms / float(nReactivity)) where the block overload multiplies by 1.0f / nReactivity;
//   * it sums from the left, (fRmsValue + new) - last (:600, :613), where the block overload adds the difference,
//     rms += new - last (:499, :528);
//   * in stereo mode it has no equalizer for LEFT and RIGHT (:388-393).
//
// The magnitude of a negative zero is +0 here (fabsf); the reference's scalar text, (s < 0.0f) ? -s : s (Sidechain.cpp:435),
// keeps -0, which in PEAK mode reaches the output's sign bit.  What lsp-dsp-lib's abs1 / abs2 give in the block overload is
// not in the reference tree, so this is unpinned, and it is a deviation from the scalar text.
//
// As the reference: set_mode() zeroes fRmsValue without a refresh, so until the next refresh (at most 0x2000 samples) the
// running sum of the RMS and UNIFORM detectors may be negative and the output sits on the clamp; clear() and
// set_stereo_mode() leave the ring's position where it is.
#ifndef MI_LSP_PLUG_IN_DSP_UNITS_UTIL_SIDECHAIN_H_
#define MI_LSP_PLUG_IN_DSP_UNITS_UTIL_SIDECHAIN_H_

#include <lsp-plug.in/dsp-units/version.h>
#include <lsp-plug.in/dsp-units/iface/IStateDumper.h>
#include <lsp-plug.in/dsp-units/util/RawRingBuffer.h>
#include <lsp-plug.in/dsp-units/filters/Equalizer.h>

namespace lsp
{
    namespace dspu
    {
        enum sidechain_source_t
        {
            SCS_MIDDLE,
            SCS_SIDE,
            SCS_LEFT,
            SCS_RIGHT,
            SCS_AMIN,
            SCS_AMAX
        };

        enum sidechain_mode_t
        {
            SCM_PEAK,
            SCM_RMS,
            SCM_LPF,
            SCM_UNIFORM
        };

        enum sidechain_stereo_mode_t
        {
            SCSM_STEREO,
            SCSM_MIDSIDE
        };

        class LSP_DSP_UNITS_PUBLIC Sidechain
        {
            // Binary layout: data members and their order as in the reference class (util/Sidechain.h:69-83 of lsp-dsp-units),
            // 80 bytes on LP64 (host/sidechain.cpp asserts the size and every offset).  There is no spare member: the GPU bank
            // is kept beside the object, keyed by its address, and goes away in destroy().
            protected:
                enum flags_t
                {
                    SCF_MIDSIDE     = 1 << 0,
                    SCF_UPDATE      = 1 << 1,
                    SCF_CLEAR       = 1 << 2
                };

            protected:
                RawRingBuffer   sBuffer;                // capacity and position of the ring; the samples are on the device
                size_t          nReactivity;
                size_t          nSampleRate;
                Equalizer      *pPreEq;
                float           fReactivity;
                float           fTau;
                float           fRmsValue;
                float           fMaxReactivity;
                float           fGain;
                uint32_t        nRefresh;
                uint8_t         nSource;
                uint8_t         nMode;
                uint8_t         nChannels;
                uint8_t         nFlags;

            protected:
                // (the reference's refresh_processing() and preprocess() have no host form: they are parts of the device's kernel)
                void            update_settings();

            public:
                explicit Sidechain();
                Sidechain(const Sidechain &) = delete;
                Sidechain(Sidechain &&) = delete;
                ~Sidechain();

                Sidechain & operator = (const Sidechain &) = delete;
                Sidechain & operator = (Sidechain &&) = delete;

                void            construct();            // valid on raw (e.g. zeroed) memory
                bool            init(size_t channels, float max_reactivity);        // channels: 1 or 2
                void            destroy();

            public:
                inline void     set_pre_equalizer(Equalizer *eq)    { pPreEq = eq; }
                void            set_sample_rate(size_t sr);
                void            set_reactivity(float reactivity);   // ms; ignored outside [0, max_reactivity]
                void            set_stereo_mode(sidechain_stereo_mode_t mode);
                inline void     set_source(size_t source)           { nSource = uint8_t(source); }
                void            clear();
                inline void     set_mode(size_t mode)
                {
                    if (nMode == mode)
                        return;
                    fRmsValue       = 0.0f;
                    nMode           = uint8_t(mode);
                }
                inline void     set_gain(float gain)                { fGain = gain; }
                inline float    get_gain() const                    { return fGain; }

                // in: nChannels host pointers, or NULL for silence
                void            process(float *out, const float **in, size_t samples);
                // in: one sample per input
                float           process(const float *in);

                void            dump(IStateDumper *v) const;
        };
    }
}

#endif
