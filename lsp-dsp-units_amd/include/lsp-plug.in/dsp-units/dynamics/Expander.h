// lsp::dspu::Expander on the GPU library (one expander, host pointers; the device-resident form for many channels is
// mi_expander_bank_*).  update_settings(), the scalar curve() and both amplification() forms are host arithmetic on sExp
// (the array amplification() is the scalar one dot by dot: the bank has no gain-only entry); the array curve() and both
// process() overloads run on the device through a bank of one channel that the object makes at its first such call (the
// scalar process() is a call of one sample).  Inputs are finite: NaN is out of scope.
//
// As the reference: a fresh object is UPWARD, set_knee() limits nothing, and upward the curve() of a level above the
// threshold is that of the threshold.
#ifndef MI_LSP_PLUG_IN_DSP_UNITS_DYNAMICS_EXPANDER_H_
#define MI_LSP_PLUG_IN_DSP_UNITS_DYNAMICS_EXPANDER_H_

#include <lsp-plug.in/dsp-units/version.h>
#include <lsp-plug.in/dsp-units/iface/IStateDumper.h>
#include <lsp-plug.in/dsp/dsp.h>

namespace lsp
{
    namespace dspu
    {
        enum expander_mode_t
        {
            EM_DOWNWARD,
            EM_UPWARD
        };

        class LSP_DSP_UNITS_PUBLIC Expander
        {
            // Binary layout: data members and their order as in the reference class
            // (include/lsp-plug.in/dsp-units/dynamics/Expander.h:42-64 of lsp-dsp-units), 92 bytes.  There is no spare member:
            // the GPU bank is kept beside the object, keyed by its address, and goes away in destroy().
            protected:
                float       fAttackThresh;
                float       fReleaseThresh;
                float       fAttack;
                float       fRelease;
                float       fKnee;
                float       fRatio;
                float       fEnvelope;
                float       fHold;
                float       fPeak;

                float       fTauAttack;
                float       fTauRelease;
                dsp::expander_knee_t sExp;

                uint32_t    nHold;
                uint32_t    nHoldCounter;
                uint32_t    nSampleRate;
                bool        bUpdate;
                bool        bUpward;

            public:
                explicit Expander();
                Expander(const Expander &) = delete;
                Expander(Expander &&) = delete;
                ~Expander();

                Expander & operator = (const Expander &) = delete;
                Expander & operator = (Expander &&) = delete;

                void        construct();            // valid on raw (e.g. zeroed) memory
                void        destroy();

            public:
                inline bool     modified() const            { return bUpdate; }
                inline bool     is_upward() const           { return bUpward; }
                inline bool     is_downward() const         { return !bUpward; }
                void            update_settings();

                void            set_attack_threshold(float threshold);
                inline float    attack_threshold() const    { return fAttackThresh; }
                void            set_release_threshold(float threshold);
                inline float    release_threshold() const   { return fReleaseThresh; }
                void            set_threshold(float attack, float release);

                void            set_timings(float attack, float release);       // ms
                void            set_attack(float attack);
                inline float    attack() const              { return fAttack; }
                void            set_release(float release);
                inline float    release() const             { return fRelease; }

                void            set_sample_rate(size_t sr);
                inline size_t   sample_rate() const         { return nSampleRate; }
                void            set_knee(float knee);
                inline float    knee() const                { return fKnee; }
                void            set_ratio(float ratio);
                inline float    ratio() const               { return fRatio; }
                void            set_mode(size_t mode);
                inline size_t   mode() const                { return (bUpward) ? EM_UPWARD : EM_DOWNWARD; }
                float           hold() const                { return fHold; }
                void            set_hold(float hold);       // ms

                // out: the gain for the VCA, env (may be NULL): the envelope, in: the sidechain signal
                void            process(float *out, float *env, const float *in, size_t samples);
                float           process(float *env, float s);

                void            curve(float *out, const float *in, size_t dots);
                float           curve(float in);
                void            amplification(float *out, const float *in, size_t dots);
                float           amplification(float in);

                void            dump(IStateDumper *v) const;
        };
    }
}

#endif
