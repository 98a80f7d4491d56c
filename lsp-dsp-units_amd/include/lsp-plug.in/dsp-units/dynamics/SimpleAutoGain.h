// lsp::dspu::SimpleAutoGain on the GPU library (one unit, host pointers; the device-resident form for many channels is
// mi_simple_autogain_bank_*).  The setters, update() and dump() are host arithmetic on the object's fields (set_max_gain,
// set_min_gain and set_gain act on fCurrGain at once, as in the reference); process() runs on the device through a bank of
// one channel that the object makes at its first such call and reads fCurrGain back afterwards; process(float) is a call of
// one sample.  Inputs are finite: NaN is out of scope.
//
// As the reference: max_gain() and min_gain() return bool.
#ifndef MI_LSP_PLUG_IN_DSP_UNITS_DYNAMICS_SIMPLEAUTOGAIN_H_
#define MI_LSP_PLUG_IN_DSP_UNITS_DYNAMICS_SIMPLEAUTOGAIN_H_

#include <lsp-plug.in/dsp-units/version.h>
#include <lsp-plug.in/dsp-units/iface/IStateDumper.h>
#include <lsp-plug.in/dsp/dsp.h>

namespace lsp
{
    namespace dspu
    {
        class LSP_DSP_UNITS_PUBLIC SimpleAutoGain
        {
            // Binary layout: data members and their order as in the reference class
            // (include/lsp-plug.in/dsp-units/dynamics/SimpleAutoGain.h:50-60 of lsp-dsp-units), 40 bytes.  The GPU bank is
            // kept beside the object, keyed by its address, and goes away in destroy().
            protected:
                enum flags_t
                {
                    F_UPDATE        = 1 << 0
                };

            protected:
                uint32_t        nSampleRate;
                uint32_t        nFlags;

                float           fKGrow;
                float           fKFall;
                float           fGrow;          // dB/s
                float           fFall;
                float           fThreshold;
                float           fCurrGain;
                float           fMinGain;
                float           fMaxGain;

            public:
                explicit SimpleAutoGain();
                SimpleAutoGain(const SimpleAutoGain &) = delete;
                SimpleAutoGain(SimpleAutoGain &&) = delete;
                ~SimpleAutoGain();

                SimpleAutoGain & operator = (const SimpleAutoGain &) = delete;
                SimpleAutoGain & operator = (SimpleAutoGain &&) = delete;

                void            construct();            // valid on raw (e.g. zeroed) memory
                void            destroy();
                status_t        init();

            public:
                status_t        set_sample_rate(size_t sample_rate);
                inline size_t   sample_rate() const             { return nSampleRate;   }

                void            set_grow(float value);
                inline float    grow() const                    { return fGrow;         }
                void            set_fall(float value);
                float           fall() const                    { return fFall;         }
                void            set_speed(float grow, float fall);

                void            set_max_gain(float value);
                inline bool     max_gain() const                { return fMaxGain;      }
                void            set_min_gain(float value);
                bool            min_gain() const                { return fMinGain;      }
                void            set_gain(float min, float max);
                // lsp_limit(fCurrGain, fMinGain, fMaxGain)
                inline float    gain() const
                    { return (fCurrGain < fMinGain) ? fMinGain : ((fCurrGain > fMaxGain) ? fMaxGain : fCurrGain); }

                inline bool     needs_update() const            { return nFlags & F_UPDATE; }
                void            update();

                inline float    threshold() const               { return fThreshold; }
                void            set_threshold(float threshold);

                // dst: the gain adjustment; src: the measured gain
                void            process(float *dst, const float *src, size_t count);
                float           process(float src);

                void            dump(IStateDumper *v) const;
        };
    }
}

#endif
