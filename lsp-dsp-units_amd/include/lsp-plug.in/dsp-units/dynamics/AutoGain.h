// lsp::dspu::AutoGain on the GPU library (one unit, host pointers; the device-resident form for many channels is
// mi_autogain_bank_*).  The setters, update() and dump() are host arithmetic on the object's fields; both process()
// overloads run on the device through a bank of one channel that the object makes at its first such call, and read
// fCurrGain, fOutGain and the surge flags back afterwards.  lexp > 0 and inputs are finite: NaN is out of scope.
//
// As the reference: max_gain() returns bool, dump() does not write fMaxGain, and set_silence_threshold, set_max_gain,
// enable_max_gain and enable_quick_amplifier do not ask for an update().
#ifndef MI_LSP_PLUG_IN_DSP_UNITS_DYNAMICS_AUTOGAIN_H_
#define MI_LSP_PLUG_IN_DSP_UNITS_DYNAMICS_AUTOGAIN_H_

#include <lsp-plug.in/dsp-units/version.h>
#include <lsp-plug.in/dsp-units/iface/IStateDumper.h>
#include <lsp-plug.in/dsp/dsp.h>

namespace lsp
{
    namespace dspu
    {
        class LSP_DSP_UNITS_PUBLIC AutoGain
        {
            // Binary layout: data members and their order as in the reference class
            // (include/lsp-plug.in/dsp-units/dynamics/AutoGain.h:45-81 of lsp-dsp-units), 128 bytes.  There is no spare
            // member: the GPU bank is kept beside the object, keyed by its address, and goes away in destroy().
            protected:
                typedef struct timing_t
                {
                    float           fGrow;          // dB/s
                    float           fFall;
                    float           fKGrow;         // per sample
                    float           fKFall;
                } timing_t;

                typedef struct
                {
                    float           x1, x2;
                    float           t;
                    float           a, b, c, d;
                } compressor_t;

                enum flags_t
                {
                    F_UPDATE        = 1 << 0,
                    F_QUICK_AMP     = 1 << 1,
                    F_MAX_GAIN      = 1 << 2,
                    F_SURGE_UP      = 1 << 3,
                    F_SURGE_DOWN    = 1 << 4
                };

            protected:
                size_t          nSampleRate;
                size_t          nFlags;

                timing_t        sShort;
                timing_t        sLong;
                compressor_t    sShortComp;
                compressor_t    sOutComp;
                float           fSilence;
                float           fDeviation;
                float           fCurrGain;
                float           fMaxGain;
                float           fOutGain;

            protected:
                static void     init_compressor(compressor_t &c);
                static void     dump(const char *id, const timing_t *t, IStateDumper *v);
                static void     dump(const char *id, const compressor_t *c, IStateDumper *v);

            protected:
                void            set_timing(float *ptr, float value);
                void            run(float *vca, const float *llong, const float *lshort, const float *lexp, float level, size_t count);

            public:
                explicit AutoGain();
                AutoGain(const AutoGain &) = delete;
                AutoGain(AutoGain &&) = delete;
                ~AutoGain();

                AutoGain & operator = (const AutoGain &) = delete;
                AutoGain & operator = (AutoGain &&) = delete;

                void            construct();            // valid on raw (e.g. zeroed) memory
                void            destroy();
                status_t        init();

            public:
                status_t        set_sample_rate(size_t sample_rate);
                inline size_t   sample_rate() const             { return nSampleRate;   }

                void            set_silence_threshold(float threshold);
                inline float    silence_threshold() const       { return fSilence;      }

                void            set_deviation(float deviation);
                inline float    deviation() const               { return fDeviation;    }

                inline void     set_short_grow(float value)     { set_timing(&sShort.fGrow, value);     }
                inline float    short_grow() const              { return sShort.fGrow;                  }
                inline void     set_short_fall(float value)     { set_timing(&sShort.fFall, value);     }
                inline float    short_fall() const              { return sShort.fFall;                  }
                void            set_short_speed(float grow, float fall);

                inline void     set_long_grow(float value)      { set_timing(&sLong.fGrow, value);      }
                inline float    long_grow() const               { return sLong.fGrow;                   }
                inline void     set_long_fall(float value)      { set_timing(&sLong.fFall, value);      }
                inline float    long_fall() const               { return sLong.fFall;                   }
                void            set_long_speed(float grow, float fall);

                void            set_max_gain(float value, bool enable);
                void            set_max_gain(float value);
                void            enable_max_gain(bool enable);
                inline bool     max_gain() const                { return fMaxGain;                      }
                inline bool     max_gain_enabled() const        { return nFlags & F_MAX_GAIN;           }

                void            enable_quick_amplifier(bool enable);
                inline bool     quick_amplifier() const         { return nFlags & F_QUICK_AMP;          }

                inline bool     needs_update() const            { return nFlags & F_UPDATE;             }
                void            update();

                // vca: the gain for the VCA; llong, lshort: the long- and short-period loudness; lexp: the expected level
                void            process(float *vca, const float *llong, const float *lshort, const float *lexp, size_t count);
                void            process(float *vca, const float *llong, const float *lshort, float lexp, size_t count);

                void            dump(IStateDumper *v) const;
        };
    }
}

#endif
