// lsp::dspu::Compressor on the GPU library (one compressor, host pointers; the device-resident form for many channels is
// mi_compressor_bank_*).  update_settings(), the scalar curve() and reduction() are host arithmetic on sComp; the array
// forms and both process() overloads run on the device through a bank of one channel that the object makes at its first
// such call (the scalar process() is a call of one sample).  Inputs are finite: NaN is out of scope.
//
// As the reference: the array reduction(out, in, dots) is the curve, not the gain (the scalar reduction() is the gain),
// and dump() closes the sComp object with end_array().
#ifndef MI_LSP_PLUG_IN_DSP_UNITS_DYNAMICS_COMPRESSOR_H_
#define MI_LSP_PLUG_IN_DSP_UNITS_DYNAMICS_COMPRESSOR_H_

#include <lsp-plug.in/dsp-units/version.h>
#include <lsp-plug.in/dsp-units/iface/IStateDumper.h>
#include <lsp-plug.in/dsp/dsp.h>

namespace lsp
{
    namespace dspu
    {
        enum compressor_mode_t
        {
            CM_DOWNWARD,
            CM_UPWARD,
            CM_BOOSTING
        };

        class LSP_DSP_UNITS_PUBLIC Compressor
        {
            // Binary layout: data members and their order as in the reference class
            // (include/lsp-plug.in/dsp-units/dynamics/Compressor.h:46-72 of lsp-dsp-units), 132 bytes.  There is no spare
            // member: the GPU bank is kept beside the object, keyed by its address, and goes away in destroy().
            protected:
                typedef dsp::compressor_x2_t comp_t;

            protected:
                float       fAttackThresh;
                float       fReleaseThresh;
                float       fBoostThresh;
                float       fAttack;
                float       fRelease;
                float       fKnee;
                float       fRatio;
                float       fHold;
                float       fEnvelope;
                float       fPeak;

                float       fTauAttack;
                float       fTauRelease;
                comp_t      sComp;

                uint32_t    nHold;
                uint32_t    nHoldCounter;
                uint32_t    nSampleRate;
                uint32_t    nMode;
                bool        bUpdate;

            public:
                explicit Compressor();
                Compressor(const Compressor &) = delete;
                Compressor(Compressor &&) = delete;
                ~Compressor();

                Compressor & operator = (const Compressor &) = delete;
                Compressor & operator = (Compressor &&) = delete;

                void        construct();            // valid on raw (e.g. zeroed) memory
                void        destroy();

            public:
                inline bool     modified() const            { return bUpdate; }
                void            update_settings();

                inline float    attack_threshold() const    { return fAttackThresh; }
                void            set_attack_threshold(float threshold);
                inline float    release_threshold() const   { return fReleaseThresh; }
                void            set_release_threshold(float threshold);
                void            set_threshold(float attack, float release);
                inline float    boost_threshold() const     { return fBoostThresh; }
                void            set_boost_threshold(float boost);

                void            set_timings(float attack, float release);       // ms
                inline float    attack() const              { return fAttack; }
                void            set_attack(float attack);
                inline float    release() const             { return fRelease; }
                void            set_release(float release);

                inline size_t   sample_rate() const         { return nSampleRate; }
                void            set_sample_rate(size_t sr);
                inline float    knee() const                { return fKnee; }
                void            set_knee(float knee);
                inline float    ratio() const               { return fRatio; }
                void            set_ratio(float ratio);
                void            set_mode(size_t mode);
                inline size_t   mode() const                { return nMode; }
                float           hold() const                { return fHold; }
                void            set_hold(float hold);       // ms

                // out: the gain for the VCA, env (may be NULL): the envelope, in: the sidechain signal
                void            process(float *out, float *env, const float *in, size_t samples);
                float           process(float *env, float in);

                void            curve(float *out, const float *in, size_t dots);
                float           curve(float in);
                void            reduction(float *out, const float *in, size_t dots);
                float           reduction(float in);

                void            dump(IStateDumper *v) const;
        };
    }
}

#endif
