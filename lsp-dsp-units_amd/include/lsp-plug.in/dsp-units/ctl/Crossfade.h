// lsp::dspu::Crossfade on the GPU library (one channel, host pointers; the device-resident form for many channels is
// mi_crossfade_bank_*).  init(), toggle() and reset() are host code on the object's fields; process() runs on the device through
// a bank of one channel that the object makes at its first such call, hands it nCounter, fDelta and fGain where they are not
// what the previous call read back, and reads them back afterwards, so remaining(), active(), dump() and a later call see the
// reference's values.  The bank counts in 32 bits: a fade of 2^32 samples and more is clamped to 2^32 - 1, and a NaN length
// (undefined in the reference) to 1.
#ifndef MI_LSP_PLUG_IN_DSP_UNITS_CTL_CROSSFADE_H_
#define MI_LSP_PLUG_IN_DSP_UNITS_CTL_CROSSFADE_H_

#include <lsp-plug.in/dsp-units/version.h>
#include <lsp-plug.in/dsp-units/iface/IStateDumper.h>

namespace lsp
{
    namespace dspu
    {
        class LSP_DSP_UNITS_PUBLIC Crossfade
        {
            // Binary layout: data members and their order as in the reference class (ctl/Crossfade.h of lsp-dsp-units), 24 bytes
            // (host/crossfade.cpp asserts the size).  The GPU bank is kept beside the object, keyed by its address, and goes
            // away in destroy().
            protected:
                size_t      nSamples;   // the length of a fade
                size_t      nCounter;   // samples of the running fade that are left
                float       fDelta;     // the gain's step per sample
                float       fGain;      // 0: fade_out, 1: fade_in

            public:
                explicit Crossfade();

                Crossfade(const Crossfade &) = delete;
                Crossfade(Crossfade &&) = delete;
                ~Crossfade();

                Crossfade & operator = (const Crossfade &) = delete;
                Crossfade & operator = (Crossfade &&) = delete;

                void            construct();            // valid on raw (e.g. zeroed) memory
                void            destroy();

            public:
                void            init(int sample_rate, float time = 0.005f);

                // dst, fade_out, fade_in: host pointers; either input may be NULL, or both
                void            process(float *dst, const float *fade_out, const float *fade_in, size_t count);

                inline size_t   remaining() const { return nCounter; }
                inline bool     active() const { return nCounter > 0; }

                // stops the fade where it is, on the fade_out side
                void            reset();

                // starts a fade unless one is running; true if it did
                bool            toggle();

                void            dump(IStateDumper *v) const;
        };
    }
}

#endif
