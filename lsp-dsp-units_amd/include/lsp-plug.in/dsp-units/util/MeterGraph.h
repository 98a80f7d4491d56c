// lsp::dspu::MeterGraph on the GPU library (one graph, host pointers; the device-resident form for many channels is
// mi_metergraph_bank_*).  The object's bytes are the reference's: a RingBuffer of frames, fCurrent, fDefault, nCount, nPeriod and
// enMethod.  The inline members are the reference's over this library's RingBuffer; process(float) is control-rate host work on
// the object's fields; the two array forms stage the caller's row on the device and run the bank's kernel through a bank of one
// channel that the object makes at its first such call, then append the frames the call produced to sBuffer.
#ifndef MI_LSP_PLUG_IN_DSP_UNITS_UTIL_METERGRAPH_H_
#define MI_LSP_PLUG_IN_DSP_UNITS_UTIL_METERGRAPH_H_

#include <stddef.h>
#include <stdint.h>

#include <lsp-plug.in/dsp-units/version.h>
#include <lsp-plug.in/dsp-units/iface/IStateDumper.h>
#include <lsp-plug.in/dsp-units/util/RingBuffer.h>

namespace lsp
{
    namespace dspu
    {
        enum meter_method_t
        {
            MM_ABS_MAXIMUM,         // the largest fabsf of the frame
            MM_ABS_MINIMUM,         // the smallest fabsf of the frame
            MM_SIGN_MAXIMUM,        // the sample of the largest magnitude, with its sign
            MM_SIGN_MINIMUM,        // the sample of the smallest magnitude, with its sign
            MM_PEAK                 // the frame's first sample
        };

        class LSP_DSP_UNITS_PUBLIC MeterGraph
        {
            protected:
                RingBuffer          sBuffer;
                float               fCurrent;
                float               fDefault;
                uint32_t            nCount;
                uint32_t            nPeriod;
                meter_method_t      enMethod;

            public:
                explicit MeterGraph();
                MeterGraph(const MeterGraph &) = delete;
                MeterGraph(MeterGraph &&) = delete;
                ~MeterGraph();

                MeterGraph & operator = (const MeterGraph &) = delete;
                MeterGraph & operator = (MeterGraph &&) = delete;

                void        construct();
                // frames of the graph, samples per frame (0 is refused), what clear() and a long read() fill with
                bool        init(size_t frames, size_t period, float default_value = 0.0f);
                void        destroy();

            public:
                inline size_t get_frames() const            { return sBuffer.size(); }
                inline float default_value() const          { return fDefault; }
                // the ring keeps its contents
                inline void set_default_value(float value)  { fDefault = value; }
                inline void set_method(meter_method_t m)    { enMethod = m; }
                // the newest `count` frames, oldest first; fDefault ahead of them where count exceeds get_frames()
                void read(float *dst, size_t count) const;
                inline void set_period(size_t period)       { nPeriod = uint32_t(period); }
                inline float period() const                 { return nPeriod; }
                void process(float sample);
                void process(const float *s, size_t n);
                // every frame's value times gain
                void process(const float *s, float gain, size_t n);
                inline float level() const                  { return sBuffer.get(0); }
                inline void fill(float level)               { sBuffer.fill(level); }
                inline void clear()                         { sBuffer.fill(fDefault); }
                void dump(IStateDumper *v) const;
        };
    } /* namespace dspu */
} /* namespace lsp */

#endif
