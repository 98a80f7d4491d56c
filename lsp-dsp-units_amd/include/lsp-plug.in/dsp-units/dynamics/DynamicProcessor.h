// lsp::dspu::DynamicProcessor on the GPU library (one processor, host pointers; the device-resident form for many channels
// is mi_dynproc_bank_*).  update_settings() and the scalar overloads process(float *, float), curve(float), model(float) and
// reduction(float) are host arithmetic on the object's own tables; the array overloads process(), curve() and model() run on
// the device through a bank of one channel that the object makes at its first such call.  The array reduction() is the
// reference's loop on the host (the bank has no gain-only entry).  Inputs are finite: NaN is out of scope.  An array overload
// that the device refuses returns without writing `out`; that includes an object whose update_settings() never ran (all
// counts 0), where the reference would run on whatever vAttack[0] holds.
//
// As the reference: process() and the array reduction() limit the level below at GAIN_AMP_MIN (1e-6), the scalar
// reduction(float), curve and model at FLOAT_SAT_M_INF (1e-10); a fresh object has all four dots ON at (0, 0, 0), which
// update_settings() cannot evaluate to finite numbers -- set every dot (set_dot(id, NULL) switches one off) before use.
#ifndef MI_LSP_PLUG_IN_DSP_UNITS_DYNAMICS_DYNAMICPROCESSOR_H_
#define MI_LSP_PLUG_IN_DSP_UNITS_DYNAMICS_DYNAMICPROCESSOR_H_

#include <lsp-plug.in/dsp-units/version.h>
#include <lsp-plug.in/dsp-units/iface/IStateDumper.h>

#define DYNAMIC_PROCESSOR_DOTS      4
#define DYNAMIC_PROCESSOR_RANGES    (DYNAMIC_PROCESSOR_DOTS + 1)

namespace lsp
{
    namespace dspu
    {
        typedef struct dyndot_t
        {
            float   fInput;         // a negative value means off
            float   fOutput;        // a negative value means off
            float   fKnee;          // a negative value means off
        } dyndot_t;

        class LSP_DSP_UNITS_PUBLIC DynamicProcessor
        {
            // Binary layout: data members and their order as in the reference class
            // (include/lsp-plug.in/dsp-units/dynamics/DynamicProcessor.h:75-100 of lsp-dsp-units), 400 bytes.  There is no
            // spare member: the GPU bank is kept beside the object, keyed by its address, and goes away in destroy().
            protected:
                typedef struct spline_t
                {
                    float       fPreRatio;
                    float       fPostRatio;
                    float       fKneeStart;
                    float       fKneeStop;
                    float       fThresh;        // logarithmic
                    float       fMakeup;
                    float       vHermite[4];
                } spline_t;

                typedef struct reaction_t
                {
                    float       fLevel;
                    float       fTau;
                } reaction_t;

                enum counters_t
                {
                    CT_SPLINES,
                    CT_ATTACK,
                    CT_RELEASE,

                    CT_TOTAL
                };

            protected:
                dyndot_t    vDots[DYNAMIC_PROCESSOR_DOTS];
                float       vAttackLvl[DYNAMIC_PROCESSOR_DOTS];
                float       vReleaseLvl[DYNAMIC_PROCESSOR_DOTS];
                float       vAttackTime[DYNAMIC_PROCESSOR_RANGES];
                float       vReleaseTime[DYNAMIC_PROCESSOR_RANGES];
                float       fInRatio;
                float       fOutRatio;

                spline_t    vSplines[DYNAMIC_PROCESSOR_DOTS];
                reaction_t  vAttack[DYNAMIC_PROCESSOR_RANGES];
                reaction_t  vRelease[DYNAMIC_PROCESSOR_RANGES];
                uint8_t     fCount[CT_TOTAL];

                float       fEnvelope;
                float       fHold;
                float       fPeak;

                uint32_t    nHold;
                uint32_t    nHoldCounter;
                uint32_t    nSampleRate;
                bool        bUpdate;

            protected:
                static float    spline_amp(const spline_t *s, float x);
                static float    spline_model(const spline_t *s, float x);
                static float    solve_reaction(const reaction_t *s, float x, size_t count);

            public:
                explicit DynamicProcessor();
                DynamicProcessor(const DynamicProcessor &) = delete;
                DynamicProcessor(DynamicProcessor &&) = delete;
                ~DynamicProcessor();

                DynamicProcessor & operator = (const DynamicProcessor &) = delete;
                DynamicProcessor & operator = (DynamicProcessor &&) = delete;

                void        construct();            // valid on raw (e.g. zeroed) memory
                void        destroy();

            public:
                inline bool     modified() const            { return bUpdate; }
                void            update_settings();

                inline size_t   sample_rate() const         { return nSampleRate; }
                void            set_sample_rate(size_t sr);
                inline float    in_ratio() const            { return fInRatio; }
                void            set_in_ratio(float ratio);
                inline float    out_ratio() const           { return fOutRatio; }
                void            set_out_ratio(float ratio);

                bool            get_dot(size_t id, dyndot_t *dst) const;
                bool            set_dot(size_t id, const dyndot_t *src);           // NULL: off
                bool            set_dot(size_t id, float in, float out, float knee);

                float           attack_level(size_t id) const;                      // -1 for an id out of range
                void            set_attack_level(size_t id, float value);
                float           release_level(size_t id) const;
                void            set_release_level(size_t id, float value);
                float           attack_time(size_t id) const;                       // ms
                void            set_attack_time(size_t id, float value);
                float           release_time(size_t id) const;
                void            set_release_time(size_t id, float value);
                float           hold() const                { return fHold; }
                void            set_hold(float hold);       // ms

                // out: the gain for the VCA, env (may be NULL): the envelope, in: the sidechain signal
                void            process(float *out, float *env, const float *in, size_t samples);
                float           process(float *env, float s);

                void            curve(float *out, const float *in, size_t dots);
                float           curve(float in);
                void            model(float *out, const float *in, size_t dots);
                float           model(float in);
                void            reduction(float *out, const float *in, size_t dots);
                float           reduction(float in);

                void            dump(IStateDumper *v) const;
        };
    }
}

#endif
