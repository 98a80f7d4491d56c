// lsp::dspu::QuantizedCounter on the GPU library (one counter, host pointers; the device-resident form for many channels is
// mi_qcounter_bank_*): the histogram of the last period() samples over levels() quantisation levels of [min, max), with one
// counter for what lies below the range and one for above.  The object's bytes are the reference's.  The setters are host work
// on the object's fields.  process() stages the caller's row on the device and runs the bank's kernel through a bank of one
// channel that the object makes at its first such call; vHistory and vCounters are the host's copies of the ring and of the
// counters, read back from the device after every call that changes them, so counters(), below(), above() and count() are the
// reference's inline members.
//   - where C++ leaves the reference's float-to-int conversion undefined (a NaN, a scaled sample outside int32_t) the sample
//     counts as the reference's compiled class has it on x86-64: below for a NaN or a product >= 2^31, above from levels() on;
//   - process() leaves the window of the last min(period(), samples seen) samples for any count.  A single call of the
//     reference's with more than nCapacity - nPeriod samples corrupts its window; here the result is that of the same row fed
//     in pieces;
//   - process() before init(), before set_period() or before the levels were ever set does nothing (the reference divides by
//     zero into a meaningless state); so does a call of 2^31 samples or more.
#ifndef MI_LSP_PLUG_IN_DSP_UNITS_STAT_QUANTIZEDCOUNTER_H_
#define MI_LSP_PLUG_IN_DSP_UNITS_STAT_QUANTIZEDCOUNTER_H_

#include <stddef.h>
#include <stdint.h>

#include <lsp-plug.in/dsp-units/version.h>
#include <lsp-plug.in/dsp/dsp.h>
#include <lsp-plug.in/dsp-units/iface/IStateDumper.h>

namespace lsp
{
    namespace dspu
    {
        class LSP_DSP_UNITS_PUBLIC QuantizedCounter
        {
            // Binary layout: data members and their order as in the reference class, 72 bytes on LP64
            // (host/quantized_counter_class.cpp asserts the size).  The GPU bank is kept beside the object, keyed by its
            // address, and goes away in destroy().
            private:
                uint32_t        nPeriod;        // the window in samples
                uint32_t        nLevels;        // quantisation levels
                uint32_t        nHead;          // where the next sample goes in the ring
                uint32_t        nCapacity;      // the ring in samples
                uint32_t        nCount;         // samples in the window
                uint32_t        nMaxPeriod;
                uint32_t        nMaxLevels;
                float           fMinValue;
                float           fMaxValue;
                float           fRStep;         // levels per unit, as of the last update
                bool            bUpdate;        // levels, min or max changed since

                float          *vHistory;       // the host's copy of the ring
                uint32_t       *vCounters;      // the host's copy of the nMaxLevels + 2 counters

                uint8_t        *pData;

            public:
                QuantizedCounter();
                QuantizedCounter(const QuantizedCounter &) = delete;
                QuantizedCounter(QuantizedCounter &&) = delete;
                ~QuantizedCounter();

                QuantizedCounter & operator = (const QuantizedCounter &) = delete;
                QuantizedCounter & operator = (QuantizedCounter &&) = delete;

                void            construct();
                void            destroy();

            public:
                // max_period in samples (1 .. 2^32 - 2049), max_levels 1 .. 2^24
                status_t        init(size_t max_period, size_t max_levels);

            public:
                // limited to 1 .. max_period(); takes effect at the next process(): until then count() may exceed period()
                void            set_period(size_t period);
                inline size_t   period() const          { return nPeriod;       }
                inline size_t   max_period() const      { return nMaxPeriod;    }

                // limited to 1 .. max_levels
                void            set_levels(size_t levels);
                inline size_t   levels() const          { return nLevels;       }

                void            set_min_value(float min);
                void            set_max_value(float max);
                void            set_value_range(float min, float max);
                void            set_range(float min, float max, size_t levels);

                inline bool     needs_update() const        { return bUpdate; }
                // the counters counted anew over the count() samples held, under the new step
                void            update_settings();

                void            process(const float *data, size_t count);

                // counters and count; the ring's words stay
                void            clear();

                inline const uint32_t *counters() const     { return vCounters;     }
                inline uint32_t below() const               { return vCounters[nMaxLevels];         }
                inline uint32_t above() const               { return vCounters[nMaxLevels + 1];     }
                inline size_t   count() const               { return nCount;        }

                void            dump(IStateDumper *v) const;
        };

    } /* namespace dspu */
} /* namespace lsp */

#endif
