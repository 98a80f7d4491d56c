// lsp::dspu::ScaledMeterGraph on the GPU library (one graph, host pointers; the device-resident form for many channels is
// mi_scaled_metergraph_bank_*).  The object's bytes are the reference's: two samplers -- a RawRingBuffer, fCurrent, nCount, nPeriod
// and nFrames each, the history of sub-samples and the display frames -- then the target nPeriod, nMaxPeriod and enMethod.  The
// inline members are the reference's; process(float) and the setters are control-rate host work on the object's fields; the two
// array forms stage the caller's row on the device and run the bank's kernel through a bank of one channel that the object makes
// at its first such call, then bring both rings and every state word back.
#ifndef MI_LSP_PLUG_IN_DSP_UNITS_UTIL_SCALEDMETERGRAPH_H_
#define MI_LSP_PLUG_IN_DSP_UNITS_UTIL_SCALEDMETERGRAPH_H_

#include <stddef.h>
#include <stdint.h>

#include <lsp-plug.in/dsp-units/version.h>
#include <lsp-plug.in/dsp-units/iface/IStateDumper.h>
#include <lsp-plug.in/dsp-units/util/RawRingBuffer.h>
#include <lsp-plug.in/dsp-units/util/MeterGraph.h>

namespace lsp
{
    namespace dspu
    {
        class LSP_DSP_UNITS_PUBLIC ScaledMeterGraph
        {
            protected:
                typedef struct sampler_t
                {
                    RawRingBuffer       sBuffer;        // what the sampler has produced
                    float               fCurrent;       // the open frame's value
                    uint32_t            nCount;         // samples in the open frame
                    uint32_t            nPeriod;        // samples per frame
                    uint32_t            nFrames;        // frames that are read of the ring (it holds 16 more)
                } sampler_t;

            protected:
                sampler_t           sHistory;           // sub-samples of `subsampling` samples
                sampler_t           sFrames;            // display frames of the period last taken over
                uint32_t            nPeriod;            // the period that the next process() takes over
                uint32_t            nMaxPeriod;
                meter_method_t      enMethod;

            private:
                bool                update_period();
                void                process_sampler(sampler_t *sampler, float sample);
                void                process_block(const float *s, const float *gain, size_t count);

            public:
                explicit ScaledMeterGraph();
                ScaledMeterGraph(const ScaledMeterGraph &) = delete;
                ScaledMeterGraph(ScaledMeterGraph &&) = delete;
                ~ScaledMeterGraph();

                ScaledMeterGraph & operator = (const ScaledMeterGraph &) = delete;
                ScaledMeterGraph & operator = (ScaledMeterGraph &&) = delete;

                void        construct();
                // frames of the graph, samples per sub-sample, the longest period.  false where the reference is undefined:
                // no frames, a subsampling of 0, max_period < subsampling, frames * max_period from 2^31 on
                bool        init(size_t frames, size_t subsampling, size_t max_period);
                void        destroy();

            public:
                inline size_t subsampling() const           { return sHistory.nPeriod; }
                inline size_t frames() const                { return sFrames.nFrames; }
                void set_method(meter_method_t m);
                inline meter_method_t method() const        { return enMethod; }
                // limited to subsampling() .. max_period; the next process() re-decimates the history where it differs
                void        set_period(size_t period);
                inline float period() const                 { return nPeriod; }
                // the newest min(count, frames()) frames, oldest first
                void        read(float *dst, size_t count);
                void        process(float sample);
                void        process(const float *s, size_t count);
                // every frame's value times gain
                void        process(const float *s, float gain, size_t count);
                float       level() const;
                void        fill(float level);
                void        dump(IStateDumper *v) const;
        };
    } /* namespace dspu */
} /* namespace lsp */

#endif
