// lsp::dspu::Bypass on the GPU library (one channel, host pointers; the device-resident form for many channels is
// mi_bypass_bank_*).  init(), set_bypass() and bypassing() are host code on the object's fields; the three process calls run on
// the device through a bank of one channel that the object makes at its first such call, hand it the fields where they are
// not what the previous call read back, and read nState, fDelta and fGain back afterwards, so on(), off(), active(), dump()
// and a later call see the reference's values.
#ifndef MI_LSP_PLUG_IN_DSP_UNITS_CTL_BYPASS_H_
#define MI_LSP_PLUG_IN_DSP_UNITS_CTL_BYPASS_H_

#include <lsp-plug.in/dsp-units/version.h>
#include <lsp-plug.in/dsp-units/iface/IStateDumper.h>

namespace lsp
{
    namespace dspu
    {
        class LSP_DSP_UNITS_PUBLIC Bypass
        {
            // Binary layout: data members and their order as in the reference class (ctl/Bypass.h of lsp-dsp-units), 12 bytes
            // (host/bypass.cpp asserts the size).  The GPU bank is kept beside the object, keyed by its address, and goes away
            // in destroy().
            private:
                enum state_t
                {
                    S_ON,               // the dry signal passes
                    S_ACTIVE,           // on the way
                    S_OFF               // the wet signal passes
                };

                state_t nState;
                float   fDelta;         // the gain's step per sample; its sign is the direction
                float   fGain;          // 0: dry, 1: wet

            public:
                explicit Bypass();
                Bypass(const Bypass &) = delete;
                Bypass(Bypass &&) = delete;
                ~Bypass();

                Bypass & operator = (const Bypass &) = delete;
                Bypass & operator = (Bypass &&) = delete;

                void        construct();            // valid on raw (e.g. zeroed) memory
                void        destroy();

            public:
                // off, with a switch time of `time` seconds
                void        init(int sample_rate, float time = 0.005f);

                // dst, dry, wet: host pointers; dry may be NULL
                void        process(float *dst, const float *dry, const float *wet, size_t count);
                void        process_wet(float *dst, const float *dry, const float *wet, float wet_gain, size_t count);
                void        process_drywet(float *dst, const float *dry, const float *wet, float dry_gain, float wet_gain, size_t count);

                // true if the direction changed
                bool        set_bypass(bool bypass);
                inline bool set_bypass(float bypass) { return set_bypass(bypass >= 0.5f); };

                inline bool on() const      { return nState == S_ON; };
                inline bool off() const     { return nState == S_OFF; };
                inline bool active() const  { return nState == S_ACTIVE; };

                // on, or on the way there
                bool        bypassing() const;

                void        dump(IStateDumper *v) const;
        };
    }
}

#endif
