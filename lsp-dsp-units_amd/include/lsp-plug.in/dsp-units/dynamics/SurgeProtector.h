// lsp::dspu::SurgeProtector on the GPU library (one protector, host pointers; the device-resident form for many channels is
// mi_surge_bank_*).  The setters and reset() are host arithmetic on the object's fields, which are what counts; the process()
// overloads run on the device through a bank of one channel that the object makes at its first such call, and read fGain, both
// counters and bOn back afterwards.  The reference's times are size_t; the device counts in 32 bits, so a time above 2^32 - 1
// samples is taken as 2^32 - 1 there.
#ifndef MI_LSP_PLUG_IN_DSP_UNITS_DYNAMICS_SURGEPROTECTOR_H_
#define MI_LSP_PLUG_IN_DSP_UNITS_DYNAMICS_SURGEPROTECTOR_H_

#include <lsp-plug.in/dsp-units/version.h>
#include <lsp-plug.in/dsp-units/iface/IStateDumper.h>

namespace lsp
{
    namespace dspu
    {
        class LSP_DSP_UNITS_PUBLIC SurgeProtector
        {
            private:
                SurgeProtector(const SurgeProtector &) = delete;
                SurgeProtector(const SurgeProtector &&) = delete;
                SurgeProtector & operator = (const SurgeProtector &) = delete;
                SurgeProtector & operator = (const SurgeProtector &&) = delete;

            // Binary layout: data members and their order as in the reference class (dynamics/SurgeProtector.h of lsp-dsp-units),
            // 56 bytes on LP64 (host/surge_protector.cpp asserts the size).  There is no spare member: the GPU bank is kept
            // beside the object, keyed by its address, and goes away in destroy().
            protected:
                float       fGain;              // the last gain
                size_t      nTransitionTime;    // where the fade stands, samples
                size_t      nTransitionMax;     // length of a fade, samples
                size_t      nShutdownTime;      // samples below fOffThreshold in a row
                size_t      nShutdownMax;       // ... after which it goes off
                float       fOnThreshold;       // >= : on
                float       fOffThreshold;      // >= : stays on
                bool        bOn;                // fading in or open

            public:
                explicit SurgeProtector();
                ~SurgeProtector();

                void        construct();        // valid on raw (e.g. zeroed) memory
                void        destroy();

            public:
                void        reset();                                // bOn and nTransitionTime cleared, nothing else
                void        set_transition_time(size_t time);       // samples; clamps the live counter at once
                void        set_shutdown_time(size_t time);         // samples; clamps the live counter at once
                void        set_on_threshold(float threshold);
                void        set_off_threshold(float threshold);
                void        set_threshold(float on, float off);

                // one sample on the device; the return value is the gain
                float       process(float in);
                // in, out: host pointers; out NULL moves the state only
                void        process(const float *in, size_t samples);
                void        process(float *out, const float *in, size_t samples);
                void        process_mul(float *out, const float *in, size_t samples);      // out[i] *= gain

                void        dump(IStateDumper *v) const;
        };
    }
}

#endif
