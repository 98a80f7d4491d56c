// lsp::dspu::DynamicDelay on the GPU library (one line, host pointers; the device-resident form for many channels is
// mi_dyndelay_bank_*).  init() makes a bank of one channel; process() stages its five rows on the device and runs the bank's
// kernel; copy() runs the bank's copy kernel between the two objects' lines; swap() exchanges the handles.  The line lives on
// the device only: vDelay stays NULL, and pData is the handle of the bank and its staging buffer.  nHead is the reference's:
// it moves by the number of samples of every call, and a value written into it reaches the device before the next call.
// Where the reference's behaviour is undefined -- a NaN delay, a delay beyond the range of ssize_t, a NaN fdelay -- the bank's
// holds (mi_dspu.h): the delay converts with saturation and NaN as 0, a NaN fdelay counts as 0.
#ifndef MI_LSP_PLUG_IN_DSP_UNITS_UTIL_DYNAMICDELAY_H_
#define MI_LSP_PLUG_IN_DSP_UNITS_UTIL_DYNAMICDELAY_H_

#include <lsp-plug.in/dsp-units/version.h>
#include <lsp-plug.in/dsp/dsp.h>
#include <lsp-plug.in/dsp-units/iface/IStateDumper.h>

namespace lsp
{
    namespace dspu
    {
        class DynamicDelay;

        // `count` floats of d's line from position `offset` on -- the reference's vDelay[offset .. offset + count) -- read from
        // the device; false where d has no line or the stretch does not fit it.  Not part of the reference's interface.
        LSP_DSP_UNITS_PUBLIC bool dynamic_delay_read_line(const DynamicDelay *d, float *dst, size_t offset, size_t count);

        class LSP_DSP_UNITS_PUBLIC DynamicDelay
        {
            // Binary layout: data members and their order as in the reference class (util/DynamicDelay.h of lsp-dsp-units),
            // 32 bytes on LP64 (host/dynamic_delay.cpp asserts the size).
            protected:
                float      *vDelay;             // NULL: the line is on the device
                uint32_t    nHead;
                uint32_t    nCapacity;
                int32_t     nMaxDelay;
                uint8_t    *pData;              // the bank of one channel and its staging buffer

                friend bool dynamic_delay_read_line(const DynamicDelay *d, float *dst, size_t offset, size_t count);

            public:
                explicit DynamicDelay();
                DynamicDelay(const DynamicDelay &) = delete;
                DynamicDelay(DynamicDelay &&) = delete;
                ~DynamicDelay();

                DynamicDelay & operator = (const DynamicDelay &) = delete;
                DynamicDelay & operator = (DynamicDelay &&) = delete;

                void        construct();            // valid on raw (e.g. zeroed) memory
                void        destroy();

            public:
                inline size_t max_delay() const     { return nMaxDelay;     }
                inline size_t capacity() const      { return nCapacity;     }

                // a line for delays of up to max_size samples, zeroed; STATUS_NO_MEM where the bank cannot be made (a line
                // longer than 2^24 floats among the reasons: its feed index would not be exact in float32)
                status_t    init(size_t max_size);

                // out, in, delay, fgain, fdelay: host pointers to `samples` floats; out may be any of the inputs
                void        process(float *out, const float *in,
                                    const float *delay, const float *fgain, const float *fdelay,
                                    size_t samples);

                void        clear();

                // the newest samples of s to the end of this line, on the device
                void        copy(DynamicDelay *s);

                void        swap(DynamicDelay *d);

                void        dump(IStateDumper *v) const;
        };
    }
}

#endif
