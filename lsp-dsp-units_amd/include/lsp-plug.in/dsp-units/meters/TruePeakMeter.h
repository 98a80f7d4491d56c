// lsp::dspu::TruePeakMeter on the GPU library (one meter, host pointers; the device-resident form for many meters is
// mi_truepeak_bank_*).  ITU-R BS.1770-4 Annex 2 true peak: the input upsampled N times (N from the sample rate) by a
// Lanczos kernel, every output the largest magnitude of its N oversampled values.
//
// process_max() returns the largest value process() would have written for the block, as this header documents.  The
// reference's (src/main/meters/TruePeakMeter.cpp:238-272) returns 0.0f and looks at only part of the oversampled block;
// both differences are deliberate.
#ifndef MI_LSP_PLUG_IN_DSP_UNITS_METERS_TRUEPEAKMETER_H_
#define MI_LSP_PLUG_IN_DSP_UNITS_METERS_TRUEPEAKMETER_H_

#include <lsp-plug.in/dsp-units/version.h>
#include <lsp-plug.in/dsp-units/iface/IStateDumper.h>
#include <lsp-plug.in/dsp/dsp.h>

namespace lsp
{
    namespace dspu
    {
        class LSP_DSP_UNITS_PUBLIC TruePeakMeter
        {
            // Binary layout: data members and their order as in the reference class
            // (include/lsp-plug.in/dsp-units/meters/TruePeakMeter.h:40-60 of lsp-dsp-units); pData owns the GPU bank of one
            // channel and its staging buffers, vBuffer and pFunc stay NULL (the oversampled block exists only in registers).
            private:
                typedef void (*reduce_t)(float *dst, const float *src, size_t count);

            private:
                uint32_t            nSampleRate;
                uint32_t            nHead;
                uint8_t             nTimes;
                bool                bUpdate;

                dsp::resampling_function_t pFunc;
                reduce_t            pReduce;
                float              *vBuffer;
                uint8_t            *pData;

            protected:
                static uint8_t      calc_oversampling_multiplier(size_t sample_rate);
                static void         reduce_2x(float *dst, const float *src, size_t count);
                static void         reduce_3x(float *dst, const float *src, size_t count);
                static void         reduce_4x(float *dst, const float *src, size_t count);
                static void         reduce_6x(float *dst, const float *src, size_t count);
                static void         reduce_8x(float *dst, const float *src, size_t count);

            public:
                TruePeakMeter();
                TruePeakMeter(const TruePeakMeter &) = delete;
                TruePeakMeter(TruePeakMeter &&) = delete;
                ~TruePeakMeter();

                TruePeakMeter & operator = (const TruePeakMeter &) = delete;
                TruePeakMeter && operator = (TruePeakMeter &&) = delete;

                void            construct();            // valid on raw (e.g. zeroed) memory
                void            destroy();
                bool            init();

            public:
                void            update_settings();
                void            set_sample_rate(uint32_t sr);
                size_t          sample_rate() const;
                void            clear();
                void            process(float *dst, const float *src, size_t count);
                void            process(float *buf, size_t count);
                float           process_max(const float *src, size_t count);
                size_t          latency() const;
                void            dump(IStateDumper *v) const;
        };
    }
}

#endif
