// lsp::dspu::Panometer on the GPU library (one panometer, host pointers; the device-resident form for many channels is
// mi_panometer_bank_*).  The setters are host arithmetic on the object's fields; process() runs on the device through a bank of
// one channel that the object makes at its first such call, and reads fValueA, fValueB, nHead and nWindow back afterwards, so
// dump() and a later call see the reference's values.  The two rings (of squares) live on the device only: vInA, vInB and
// pData stay NULL.  A period of 0 makes the reference's process() loop forever; here it returns without writing dst.
// Inputs are finite: NaN is out of scope.
#ifndef MI_LSP_PLUG_IN_DSP_UNITS_METERS_PANOMETER_H_
#define MI_LSP_PLUG_IN_DSP_UNITS_METERS_PANOMETER_H_

#include <lsp-plug.in/dsp-units/version.h>
#include <lsp-plug.in/dsp/dsp.h>
#include <lsp-plug.in/dsp-units/iface/IStateDumper.h>

namespace lsp
{
    namespace dspu
    {
        enum pan_law_t
        {
            PAN_LAW_LINEAR,
            PAN_LAW_EQUAL_POWER
        };

        class LSP_DSP_UNITS_PUBLIC Panometer
        {
            // Binary layout: data members and their order as in the reference class (meters/Panometer.h of lsp-dsp-units),
            // 64 bytes on LP64 (host/panometer.cpp asserts the size).  There is no spare member: the GPU bank is kept beside the
            // object, keyed by its address, and goes away in destroy().
            private:
                float              *vInA;               // NULL: the ring is on the device
                float              *vInB;               // NULL
                pan_law_t           enPanLaw;
                float               fValueA;
                float               fValueB;
                float               fNorm;
                float               fDefault;
                uint32_t            nCapacity;
                uint32_t            nHead;
                uint32_t            nMaxPeriod;
                uint32_t            nPeriod;
                uint32_t            nWindow;

                uint8_t            *pData;              // NULL

            public:
                Panometer();
                Panometer(const Panometer &) = delete;
                Panometer(Panometer &&) = delete;
                ~Panometer();

                Panometer & operator = (const Panometer &) = delete;
                Panometer && operator = (Panometer &&) = delete;

                void            construct();            // valid on raw (e.g. zeroed) memory
                void            destroy();
                status_t        init(size_t max_period);        // in samples

            public:
                void            set_pan_law(pan_law_t law);
                inline pan_law_t pan_law() const            { return enPanLaw; }
                void            set_default_pan(float dfl);     // the output where both sums are (next to) nothing
                inline float    default_pan() const         { return fDefault; }
                void            set_period(size_t period);      // clamped; a changed value zeroes both sums at once
                inline size_t   period() const              { return nPeriod; }
                void            clear();                        // rings zero, nHead = nPeriod; the sums stay

                // dst, a, b: host pointers
                void            process(float *dst, const float *a, const float *b, size_t count);

                void            dump(IStateDumper *v) const;
        };
    }
}

#endif
