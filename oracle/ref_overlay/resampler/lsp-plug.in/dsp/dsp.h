// Ahead of oracle/ref_shim's <lsp-plug.in/dsp/dsp.h> for oracle/_ref/truepeak_ref only: what TruePeakMeter.cpp takes from
// lsp-dsp-lib beside copy, fill_zero and abs2.  These are this project's text, NOT lsp-dsp-lib's.
//
// lanczos_resample_Nx16bit: one scatter loop, dst[N i + j] += h[j] * src[i], every product and every sum rounded on its own.
// The taps h are UNPINNED: the driver hands them over from its case file, where the generator put mi_truepeak_coefficients'
// table (phase k, tap t at h[N t + k]; 20 N taps).  What the recordings pin is everything the class does around them.
// A call's pending sums reach 19 N values past its last input's block, inside the class's own tail of 20 N
// (TRUE_PEAK_LATENCY * 2 * nTimes); lsp-dsp-lib's LSP_DSP_RESAMPLING_RSV_SAMPLES is not used by this class.
#ifndef ORACLE_REF_OVERLAY_RESAMPLER_DSP_H_
#define ORACLE_REF_OVERLAY_RESAMPLER_DSP_H_

// ref_shim's abs2 is the Sidechain's scalar text, (s < 0.0f) ? -s : s, which keeps -0; this class states its magnitudes with
// fabsf (reduce_Nx, :115-147), so here abs2 is fabsf (UNPINNED like the rest) and ref_shim's goes by another name
#define abs2 shim_sidechain_abs2
#include_next <lsp-plug.in/dsp/dsp.h>
#undef abs2

namespace lsp
{
    namespace dsp
    {
        typedef void (*resampling_function_t)(float *dst, const float *src, size_t count);

        // set by the driver: shim_taps[N] holds shim_ntaps[N] taps
        extern const float *shim_taps[9];
        extern size_t       shim_ntaps[9];

        inline void shim_scatter(float *dst, const float *src, size_t count, size_t times)
        {
            const float *h = shim_taps[times];
            const size_t taps = shim_ntaps[times];
            for (size_t i = 0; i < count; ++i)
                for (size_t j = 0; j < taps; ++j)
                    dst[times * i + j] += h[j] * src[i];
        }

        inline void lanczos_resample_2x16bit(float *dst, const float *src, size_t count)   { shim_scatter(dst, src, count, 2); }
        inline void lanczos_resample_3x16bit(float *dst, const float *src, size_t count)   { shim_scatter(dst, src, count, 3); }
        inline void lanczos_resample_4x16bit(float *dst, const float *src, size_t count)   { shim_scatter(dst, src, count, 4); }
        inline void lanczos_resample_6x16bit(float *dst, const float *src, size_t count)   { shim_scatter(dst, src, count, 6); }
        inline void lanczos_resample_8x16bit(float *dst, const float *src, size_t count)   { shim_scatter(dst, src, count, 8); }

        inline void abs2(float *dst, const float *src, size_t count)                       // :204, no oversampling
        {
            for (size_t i = 0; i < count; ++i)
                dst[i] = fabsf(src[i]);
        }

        // TruePeakMeter.cpp:244, :264: the largest magnitude, 0 for no samples
        inline float abs_max(const float *src, size_t count)
        {
            float m = 0.0f;
            for (size_t i = 0; i < count; ++i)
                if (fabsf(src[i]) > m)
                    m = fabsf(src[i]);
            return m;
        }
    }
}

#endif
