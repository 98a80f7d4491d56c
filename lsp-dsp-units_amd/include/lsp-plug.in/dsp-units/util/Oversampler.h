// lsp::dspu::Oversampler on the GPU library (one oversampler, host pointers; the device-resident form for many channels
// is mi_oversampler_bank_*).  Lanczos upsampling N times, the caller's work on the oversampled block, the anti-alias
// low-pass and the decimation back.
//
// The callbacks run on the HOST on a staged copy of the oversampled block, with the reference's signatures.  The taps
// are inferred (L(x) = sinc(x) sinc(x / a), a = latency()); the *12BIT modes use the *X4 table.
#ifndef MI_LSP_PLUG_IN_DSP_UNITS_UTIL_OVERSAMPLER_H_
#define MI_LSP_PLUG_IN_DSP_UNITS_UTIL_OVERSAMPLER_H_

#include <lsp-plug.in/dsp-units/version.h>
#include <lsp-plug.in/dsp-units/iface/IStateDumper.h>
#include <lsp-plug.in/dsp-units/filters/Filter.h>

namespace lsp
{
    namespace dspu
    {
        // Work on the oversampled block between upsampling and downsampling; the default copies in to out.
        class LSP_DSP_UNITS_PUBLIC IOversamplerCallback
        {
            public:
                virtual ~IOversamplerCallback();
                virtual void process(float *out, const float *in, size_t samples);
        };

        // The same as a plain function: `samples` oversampled samples, `arg` as given to process().
        typedef void (*oversampler_callback_t)(float *out, const float *in, size_t samples, void *arg);

        enum over_mode_t
        {
            OM_NONE,

            OM_LANCZOS_2X2, OM_LANCZOS_2X3, OM_LANCZOS_2X4, OM_LANCZOS_2X12BIT, OM_LANCZOS_2X16BIT, OM_LANCZOS_2X24BIT,
            OM_LANCZOS_3X2, OM_LANCZOS_3X3, OM_LANCZOS_3X4, OM_LANCZOS_3X12BIT, OM_LANCZOS_3X16BIT, OM_LANCZOS_3X24BIT,
            OM_LANCZOS_4X2, OM_LANCZOS_4X3, OM_LANCZOS_4X4, OM_LANCZOS_4X12BIT, OM_LANCZOS_4X16BIT, OM_LANCZOS_4X24BIT,
            OM_LANCZOS_6X2, OM_LANCZOS_6X3, OM_LANCZOS_6X4, OM_LANCZOS_6X12BIT, OM_LANCZOS_6X16BIT, OM_LANCZOS_6X24BIT,
            OM_LANCZOS_8X2, OM_LANCZOS_8X3, OM_LANCZOS_8X4, OM_LANCZOS_8X12BIT, OM_LANCZOS_8X16BIT, OM_LANCZOS_8X24BIT
        };

        constexpr size_t OVERSAMPLER_MAX_LATENCY        = 62;

        class LSP_DSP_UNITS_PUBLIC Oversampler
        {
            // Binary layout: data members and their order as in the reference class
            // (include/lsp-plug.in/dsp-units/util/Oversampler.h:109-133 of lsp-dsp-units).  bData owns the GPU bank of one
            // channel and its staging buffers; fUpBuffer, fDownBuffer and pFunc stay NULL and nUpHead 0 (the pending sums
            // they hold in the reference do not exist here: the bank keeps the last 2a inputs on the device).  sFilter
            // carries the anti-alias parameters and rate as in the reference; the sections run inside the bank.
            protected:
                typedef void (*resample_func_t)(float *dst, const float *src, size_t count);

            protected:
                enum update_t
                {
                    UP_MODE         = 1 << 0,
                    UP_SAMPLE_RATE  = 1 << 2,
                    UP_OTHER        = 1 << 3,

                    UP_ALL          = UP_MODE | UP_OTHER | UP_SAMPLE_RATE
                };

            protected:
                IOversamplerCallback   *pCallback;
                float                  *fUpBuffer;
                float                  *fDownBuffer;
                resample_func_t         pFunc;
                size_t                  nUpHead;
                size_t                  nMode;
                size_t                  nSampleRate;
                size_t                  nUpdate;
                Filter                  sFilter;
                uint8_t                *bData;
                bool                    bFilter;

            protected:
                static resample_func_t  get_function(size_t mode);      // always NULL here: the kernels live in the bank

            public:
                explicit Oversampler();
                Oversampler(const Oversampler &) = delete;
                Oversampler(Oversampler &&) = delete;
                ~Oversampler();

                Oversampler & operator = (const Oversampler &) = delete;
                Oversampler & operator = (Oversampler &&) = delete;

                void            construct();            // valid on raw (e.g. zeroed) memory

            public:
                bool            init();
                void            destroy();
                void            set_sample_rate(size_t sr);

                inline void     set_callback(IOversamplerCallback *callback)
                {
                    pCallback       = callback;
                }

                void            set_mode(over_mode_t mode);
                over_mode_t     mode() const;

                inline void     set_filtering(bool filter)      // the bank learns of it at the next call
                {
                    if (bFilter == filter)
                        return;
                    bFilter     = filter;
                    nUpdate   |= UP_MODE;
                }

                bool            filtering() const;

                inline bool     modified() const
                {
                    return nUpdate;
                }

                size_t          get_oversampling() const;
                void            update_settings();

                // dst of samples * get_oversampling(), src of samples
                void            upsample(float *dst, const float *src, size_t samples);
                // dst of samples, src of samples * get_oversampling()
                void            downsample(float *dst, const float *src, size_t samples);
                void            process(float *dst, const float *src, size_t samples, IOversamplerCallback *callback);
                void            process(float *dst, const float *src, size_t samples, oversampler_callback_t callback, void *arg);

                inline void     process(float *dst, const float *src, size_t samples)
                {
                    process(dst, src, samples, pCallback);
                }

                size_t          latency() const;
                inline size_t   max_latency() const       { return OVERSAMPLER_MAX_LATENCY; }

                void            dump(IStateDumper *v) const;
        };
    }
}

#endif
