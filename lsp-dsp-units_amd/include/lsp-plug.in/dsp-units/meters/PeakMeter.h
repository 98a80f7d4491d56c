// lsp::dspu::PeakMeter on the GPU library (one meter, host pointers; the device-resident form for many channels is
// mi_peakmeter_bank_*).  The setters are host arithmetic on the object's fields; the three process() overloads run on the device
// through a bank of one channel that the object makes at its first such call, and read fPeak and nCounter back afterwards, so
// value(), dump() and a later call see the reference's values.  A hold time whose sample count is negative, NaN or 2^32 and
// more is undefined in the reference (uint32_t of such a float); here it is clamped into [0, 2^32 - 1], NaN to 0.
#ifndef MI_LSP_PLUG_IN_DSP_UNITS_METERS_PEAKMETER_H_
#define MI_LSP_PLUG_IN_DSP_UNITS_METERS_PEAKMETER_H_

#include <lsp-plug.in/dsp-units/version.h>
#include <lsp-plug.in/dsp-units/iface/IStateDumper.h>

namespace lsp
{
    namespace dspu
    {
        class LSP_DSP_UNITS_PUBLIC PeakMeter
        {
            // Binary layout: data members and their order as in the reference class (meters/PeakMeter.h of lsp-dsp-units), 32
            // bytes (host/peakmeter.cpp asserts the size).  There is no spare member: the GPU bank is kept beside the object,
            // keyed by its address, and goes away in destroy().
            protected:
                float       fPeak;      // the peak as it stands
                float       fTau;       // decay per sample once the hold has run out
                float       fHold;      // ms
                float       fRelease;   // ms
                uint32_t    nHold;      // fHold in samples
                uint32_t    nCounter;   // samples of hold left
                uint32_t    nSampleRate;// Hz
                bool        bUpdate;    // fTau and nHold are stale

            protected:
                void        update_settings();

            public:
                explicit PeakMeter();
                PeakMeter(const PeakMeter &) = delete;
                PeakMeter(PeakMeter &&) = delete;
                ~PeakMeter();
                PeakMeter & operator = (const PeakMeter &) = delete;
                PeakMeter & operator = (PeakMeter &&) = delete;

                void            construct();            // valid on raw (e.g. zeroed) memory
                void            destroy();

            public:
                void            set_sample_rate(size_t sample_rate);
                size_t          sample_rate() const;

                // data, dst, src: host pointers; the return value is the peak after the last sample
                float           process(const float *data, size_t count);
                float           process(float *dst, const float *src, size_t count);
                // one block-rate step on the device
                float           process(float value, size_t count);

                void            set_hold_time(float value);     // milliseconds
                float           hold_time() const;
                void            set_release_time(float value);  // milliseconds
                float           release_time() const;
                void            set_time(float hold, float release);

                float           value() const;
                void            clear();

                void            dump(IStateDumper *v) const;
        };
    }
}

#endif
