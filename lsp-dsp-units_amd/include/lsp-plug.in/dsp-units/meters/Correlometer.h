// lsp::dspu::Correlometer on the GPU library (one correlometer, host pointers; the device-resident form for many channels is
// mi_correlometer_bank_*).  The setters are host arithmetic on the object's fields; process() runs on the device through a bank
// of one channel that the object makes at its first such call, and reads sCorr, nHead and nWindow back afterwards, so dump()
// and a later call see the reference's values.  The two rings live on the device only: vInA, vInB and pData stay NULL.
// A period of 0 makes the reference's process() loop forever; here it returns without writing dst.
// Inputs are finite: NaN is out of scope.
#ifndef MI_LSP_PLUG_IN_DSP_UNITS_METERS_CORRELOMETER_H_
#define MI_LSP_PLUG_IN_DSP_UNITS_METERS_CORRELOMETER_H_

#include <lsp-plug.in/dsp-units/version.h>
#include <lsp-plug.in/dsp/dsp.h>
#include <lsp-plug.in/dsp-units/iface/IStateDumper.h>

namespace lsp
{
    namespace dspu
    {
        class LSP_DSP_UNITS_PUBLIC Correlometer
        {
            // Binary layout: data members and their order as in the reference class (meters/Correlometer.h of lsp-dsp-units),
            // 64 bytes on LP64 (host/correlometer.cpp asserts the size).  There is no spare member: the GPU bank is kept beside
            // the object, keyed by its address, and goes away in destroy().
            private:
                enum flags_t
                {
                    CF_UPDATE       = 1 << 0
                };

            private:
                dsp::correlation_t  sCorr;
                float              *vInA;               // NULL: the ring is on the device
                float              *vInB;               // NULL
                uint32_t            nCapacity;
                uint32_t            nHead;
                uint32_t            nMaxPeriod;
                uint32_t            nPeriod;
                uint32_t            nWindow;
                uint32_t            nFlags;

                uint8_t            *pData;              // NULL

            public:
                Correlometer();
                Correlometer(const Correlometer &) = delete;
                Correlometer(Correlometer &&) = delete;
                ~Correlometer();

                Correlometer & operator = (const Correlometer &) = delete;
                Correlometer && operator = (Correlometer &&) = delete;

                void            construct();            // valid on raw (e.g. zeroed) memory
                void            destroy();
                status_t        init(size_t max_period);        // in samples

            public:
                void            set_period(size_t period);      // clamped to max_period; an unchanged value is ignored
                inline size_t   period() const              { return nPeriod; }
                inline bool     needs_update() const        { return nFlags != 0; }
                void            update_settings();
                void            clear();                        // rings and sums zero, nHead = nPeriod

                // dst, a, b: host pointers
                void            process(float *dst, const float *a, const float *b, size_t count);

                void            dump(IStateDumper *v) const;
        };
    }
}

#endif
