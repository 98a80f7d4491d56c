// lsp::dspu::Gate on the GPU library (one gate, host pointers; the device-resident form for many channels is
// mi_gate_bank_*).  update_settings(), the scalar curve(), the amplification() forms (the array one is the scalar one dot
// by dot) and the scalar process() are host arithmetic on the object's fields: the scalar process() is the reference's own
// one-step rule (Gate.cpp:369-407), which is not the block overload's.  The block process() and the array curve() run on the
// device through a bank of one channel that the object makes at its first such call.  Inputs are finite: NaN is out of scope.
//
// As the reference: process() does not call update_settings(), and update_settings() computes whether or not bUpdate is
// set.  Unlike it: the block process() steps a sample a second time at most once (see mi_gate_bank in mi_dspu.h), and it
// does not read back its own output where out == in: the arithmetic is the out-of-place call's.
#ifndef MI_LSP_PLUG_IN_DSP_UNITS_DYNAMICS_GATE_H_
#define MI_LSP_PLUG_IN_DSP_UNITS_DYNAMICS_GATE_H_

#include <lsp-plug.in/dsp-units/version.h>
#include <lsp-plug.in/dsp-units/iface/IStateDumper.h>
#include <lsp-plug.in/dsp/dsp.h>

namespace lsp
{
    namespace dspu
    {
        class LSP_DSP_UNITS_PUBLIC Gate
        {
            // Binary layout: data members and their order as in the reference class
            // (include/lsp-plug.in/dsp-units/dynamics/Gate.h:36-61 of lsp-dsp-units), 128 bytes.  There is no spare member:
            // the GPU bank is kept beside the object, keyed by its address, and goes away in destroy().
            protected:
                typedef struct curve_t
                {
                    float               fThreshold;
                    float               fZone;
                    dsp::gate_knee_t    sKnee;
                } curve_t;

            protected:
                curve_t     sCurves[2];
                float       fAttack;
                float       fRelease;
                float       fTauAttack;
                float       fTauRelease;
                float       fReduction;
                float       fEnvelope;
                float       fHold;
                float       fPeak;

                uint32_t    nHold;
                uint32_t    nHoldCounter;
                uint32_t    nSampleRate;
                uint8_t     nCurve;
                bool        bUpdate;

            public:
                explicit Gate();
                Gate(const Gate &) = delete;
                Gate(Gate &&) = delete;
                ~Gate();

                Gate & operator = (const Gate &) = delete;
                Gate & operator = (Gate &&) = delete;

                void        construct();            // valid on raw (e.g. zeroed) memory
                void        destroy();

            public:
                inline bool     modified() const            { return bUpdate; }
                void            update_settings();

                void            set_threshold(float topen, float tclose);
                inline float    open_threshold() const      { return sCurves[0].fThreshold; }
                void            set_open_threshold(float threshold);
                inline float    close_threshold() const     { return sCurves[1].fThreshold; }
                void            set_close_threshold(float threshold);
                void            set_reduction(float reduction);
                inline float    reduction() const           { return fReduction; }

                void            set_timings(float attack, float release);       // ms
                void            set_attack(float attack);
                inline float    attack() const              { return fAttack; }
                void            set_release(float release);
                inline float    release() const             { return fRelease; }

                void            set_sample_rate(size_t sr);
                inline size_t   sample_rate() const         { return nSampleRate; }
                void            set_zone(float open, float close);
                void            set_open_zone(float zone);
                inline float    open_zone() const           { return sCurves[0].fZone; }
                void            set_close_zone(float zone);
                inline float    close_zone() const          { return sCurves[1].fZone; }
                void            set_hold(float hold);       // ms
                float           hold() const                { return fHold; }

                // out: the gain for the VCA, env (may be NULL): the envelope, in: the sidechain signal
                void            process(float *out, float *env, const float *in, size_t samples);
                float           process(float *env, float s);

                void            curve(float *out, const float *in, size_t dots, bool hyst) const;
                float           curve(float in, bool hyst) const;
                void            amplification(float *out, const float *in, size_t dots, bool hyst) const;
                float           amplification(float in) const;
                float           amplification(float in, bool hyst) const;

                void            dump(IStateDumper *v) const;
        };
    }
}

#endif
