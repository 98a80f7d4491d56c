// lsp::dspu::Depopper on the GPU library (one depopper, host pointers; the device-resident form for many channels is
// mi_depopper_bank_*).  init(), the setters and reconfigure() are host work on the object's fields and buffers, which are what
// counts; process() runs on the device through a bank of one channel that the object makes at its first such call: the fields
// go over where they differ from what the previous call left there, and the state words and the contents of both buffers come
// back afterwards.  Where the bank refuses the settings (no init(), an RMS length of less than a sample, a fade-out time outside
// [0, max_fade], times that are no numbers) process() leaves env and gain untouched.
#ifndef MI_LSP_PLUG_IN_DSP_UNITS_UTIL_DEPOPPER_H_
#define MI_LSP_PLUG_IN_DSP_UNITS_UTIL_DEPOPPER_H_

#include <stddef.h>
#include <stdint.h>
#include <sys/types.h>      // ssize_t

#include <lsp-plug.in/dsp-units/version.h>
#include <lsp-plug.in/dsp-units/iface/IStateDumper.h>

namespace lsp
{
    namespace dspu
    {
        enum depopper_mode_t
        {
            DPM_LINEAR,
            DPM_CUBIC,
            DPM_SINE,
            DPM_GAUSSIAN,
            DPM_PARABOLIC
        };

        class LSP_DSP_UNITS_PUBLIC Depopper
        {
            private:
                Depopper & operator = (const Depopper &);
                Depopper(const Depopper &);

            protected:
                enum state_t
                {
                    ST_CLOSED,      // the gain is 0, waiting for the envelope to reach the fade-in threshold
                    ST_FADE,        // fading in
                    ST_OPENED,      // the gain is 1, waiting for the envelope to fall below the fade-out threshold
                    ST_WAIT         // the gain is 0 for nDelay more samples
                };

            // Binary layout: data members and their order as in the reference class (util/Depopper.h of lsp-dsp-units), 248 bytes
            // on LP64 with a fade_t of 48 (host/depopper_class.cpp asserts both).  There is no spare member: the GPU bank is kept
            // beside the object, keyed by its address, and goes away in destroy().
            protected:
                typedef struct fade_t
                {
                    depopper_mode_t enMode;         // curve
                    float           fThresh;        // threshold of the envelope
                    float           fTime;          // length, ms
                    float           fDelay;         // delay, ms
                    ssize_t         nSamples;       // length, samples
                    ssize_t         nDelay;         // delay, samples
                    float           fPoly[4];       // the curve's coefficients
                } fade_t;

            protected:
                size_t          nSampleRate;
                state_t         nState;

                float           fLookMax;           // the longest fade-out, ms
                ssize_t         nLookMin;           // the gain buffer keeps this many entries
                ssize_t         nLookMax;           // ... and is shifted at this offset
                ssize_t         nLookOff;           // where the next gain goes
                ssize_t         nLookCount;         // how late the gain leaves

                float           fRmsMax;            // the longest RMS window, ms
                float           fRmsLength;         // the RMS window, ms
                ssize_t         nRmsMin;            // the buffer of squares keeps this many entries
                ssize_t         nRmsMax;            // ... and is shifted at this offset
                ssize_t         nRmsOff;            // where the next square goes
                ssize_t         nRmsLen;            // the RMS window, samples
                float           fRmsNorm;           // 1 / nRmsLen

                ssize_t         nCounter;           // samples of the fade-in done
                ssize_t         nDelay;             // samples of the delay left
                float           fRms;               // the running sum of squares

                fade_t          sFadeIn;
                fade_t          sFadeOut;

                float          *pGainBuf;           // nLookMax gains (host memory)
                float          *pRmsBuf;            // nRmsMax squares (host memory)
                uint8_t        *pData;

                bool            bReconfigure;

            public:
                explicit        Depopper();
                ~Depopper();

                void            construct();        // valid on raw (e.g. zeroed) memory
                void            destroy();

            public:
                // srate in Hz, max_fade and max_rms in milliseconds; nothing happens where the three are what they were
                bool            init(size_t srate, float max_fade, float max_rms);

                inline bool     needs_reconfiguration() const       { return bReconfigure;          }
                // the designed values of both fades, nRmsLen, nLookCount, fRmsNorm, and fRms summed again over the window
                void            reconfigure();

                // Times in milliseconds.  Each setter returns the previous value as the reference does (clamped) and stores the
                // new one as it is given.
                inline float    get_fade_in_time() const            { return sFadeIn.fTime;         }
                float           set_fade_in_time(float time);
                inline float    get_fade_out_time() const           { return sFadeOut.fTime;        }
                float           set_fade_out_time(float time);
                inline float    get_fade_in_delay() const           { return sFadeIn.fDelay;        }
                float           set_fade_in_delay(float delay);
                inline float    get_fade_out_delay() const          { return sFadeOut.fDelay;       }
                float           set_fade_out_delay(float delay);
                inline float    get_fade_in_threshold() const       { return sFadeIn.fThresh;       }
                float           set_fade_in_threshold(float thresh);
                inline float    get_fade_out_threshold() const      { return sFadeOut.fThresh;      }
                float           set_fade_out_threshold(float thresh);
                inline float    rms_length() const                  { return fRmsLength;            }
                float           set_rms_length(float length);
                depopper_mode_t get_fade_in_mode() const            { return sFadeIn.enMode;        }
                depopper_mode_t set_fade_in_mode(depopper_mode_t mode);
                depopper_mode_t get_fade_out_mode() const           { return sFadeOut.enMode;       }
                depopper_mode_t set_fade_out_mode(depopper_mode_t mode);

                // declared by the reference and defined nowhere in it; not defined here either
                float           set_release(float release);

                // env, gain, src: host pointers to count floats; env may be NULL.  The gain belongs to the sample latency() back.
                void            process(float *env, float *gain, const float *src, size_t count);

                void            dump(IStateDumper *v) const;

                inline size_t   latency() const                 { return sFadeOut.nSamples; }
        };

    } /* namespace dspu */
} /* namespace lsp */

#endif
