// Ahead of oracle/ref_shim's <lsp-plug.in/dsp/dsp.h> for oracle/_ref/oversampler_ref only: what Oversampler.cpp takes from
// lsp-dsp-lib beside copy, move and fill_zero.  These are this project's text, NOT lsp-dsp-lib's.
//
// lanczos_resample_NxK (30 functions): one scatter loop, dst[N i + j] += h[j] * src[i], every product and every sum rounded on
// its own.  The taps h are UNPINNED: the driver hands them over from its case file, where the generator put
// mi_oversampler_coefficients' table of the mode (phase k, tap t at h[N t + k]; 2 a N taps).  What the recordings pin is
// everything the class does around them.  downsample_Nx (5): dst[i] = src[N i].
//
// LSP_DSP_RESAMPLING_RSV_SAMPLES is lsp-dsp-lib's and not in the reference tree: it is how many pending sums the class carries
// over a compaction of its buffer (Oversampler.cpp:213).  UNPINNED; here 1024, no less than the longest pending tail of any
// mode (8 x 2 x 62 = 992 taps), so no sum is lost; the generator asserts that of every recorded mode.
#ifndef ORACLE_REF_OVERLAY_OVERSAMPLER_DSP_H_
#define ORACLE_REF_OVERLAY_OVERSAMPLER_DSP_H_

#include_next <lsp-plug.in/dsp/dsp.h>

#define LSP_DSP_RESAMPLING_RSV_SAMPLES      1024

namespace lsp
{
    namespace dsp
    {
        // set by the driver: shim_taps[mode] holds shim_ntaps[mode] taps (mode: over_mode_t, 1 .. 30)
        extern const float *shim_taps[31];
        extern size_t       shim_ntaps[31];

        inline void shim_scatter(float *dst, const float *src, size_t count, size_t times, size_t mode)
        {
            const float *h = shim_taps[mode];
            const size_t taps = shim_ntaps[mode];
            for (size_t i = 0; i < count; ++i)
                for (size_t j = 0; j < taps; ++j)
                    dst[times * i + j] += h[j] * src[i];
        }

        inline void shim_decimate(float *dst, const float *src, size_t count, size_t times)
        {
            for (size_t i = 0; i < count; ++i)
                dst[i] = src[times * i];
        }

        inline void lanczos_resample_2x2(float *dst, const float *src, size_t count)       { shim_scatter(dst, src, count, 2, 1); }
        inline void lanczos_resample_2x3(float *dst, const float *src, size_t count)       { shim_scatter(dst, src, count, 2, 2); }
        inline void lanczos_resample_2x4(float *dst, const float *src, size_t count)       { shim_scatter(dst, src, count, 2, 3); }
        inline void lanczos_resample_2x12bit(float *dst, const float *src, size_t count)   { shim_scatter(dst, src, count, 2, 4); }
        inline void lanczos_resample_2x16bit(float *dst, const float *src, size_t count)   { shim_scatter(dst, src, count, 2, 5); }
        inline void lanczos_resample_2x24bit(float *dst, const float *src, size_t count)   { shim_scatter(dst, src, count, 2, 6); }
        inline void lanczos_resample_3x2(float *dst, const float *src, size_t count)       { shim_scatter(dst, src, count, 3, 7); }
        inline void lanczos_resample_3x3(float *dst, const float *src, size_t count)       { shim_scatter(dst, src, count, 3, 8); }
        inline void lanczos_resample_3x4(float *dst, const float *src, size_t count)       { shim_scatter(dst, src, count, 3, 9); }
        inline void lanczos_resample_3x12bit(float *dst, const float *src, size_t count)   { shim_scatter(dst, src, count, 3, 10); }
        inline void lanczos_resample_3x16bit(float *dst, const float *src, size_t count)   { shim_scatter(dst, src, count, 3, 11); }
        inline void lanczos_resample_3x24bit(float *dst, const float *src, size_t count)   { shim_scatter(dst, src, count, 3, 12); }
        inline void lanczos_resample_4x2(float *dst, const float *src, size_t count)       { shim_scatter(dst, src, count, 4, 13); }
        inline void lanczos_resample_4x3(float *dst, const float *src, size_t count)       { shim_scatter(dst, src, count, 4, 14); }
        inline void lanczos_resample_4x4(float *dst, const float *src, size_t count)       { shim_scatter(dst, src, count, 4, 15); }
        inline void lanczos_resample_4x12bit(float *dst, const float *src, size_t count)   { shim_scatter(dst, src, count, 4, 16); }
        inline void lanczos_resample_4x16bit(float *dst, const float *src, size_t count)   { shim_scatter(dst, src, count, 4, 17); }
        inline void lanczos_resample_4x24bit(float *dst, const float *src, size_t count)   { shim_scatter(dst, src, count, 4, 18); }
        inline void lanczos_resample_6x2(float *dst, const float *src, size_t count)       { shim_scatter(dst, src, count, 6, 19); }
        inline void lanczos_resample_6x3(float *dst, const float *src, size_t count)       { shim_scatter(dst, src, count, 6, 20); }
        inline void lanczos_resample_6x4(float *dst, const float *src, size_t count)       { shim_scatter(dst, src, count, 6, 21); }
        inline void lanczos_resample_6x12bit(float *dst, const float *src, size_t count)   { shim_scatter(dst, src, count, 6, 22); }
        inline void lanczos_resample_6x16bit(float *dst, const float *src, size_t count)   { shim_scatter(dst, src, count, 6, 23); }
        inline void lanczos_resample_6x24bit(float *dst, const float *src, size_t count)   { shim_scatter(dst, src, count, 6, 24); }
        inline void lanczos_resample_8x2(float *dst, const float *src, size_t count)       { shim_scatter(dst, src, count, 8, 25); }
        inline void lanczos_resample_8x3(float *dst, const float *src, size_t count)       { shim_scatter(dst, src, count, 8, 26); }
        inline void lanczos_resample_8x4(float *dst, const float *src, size_t count)       { shim_scatter(dst, src, count, 8, 27); }
        inline void lanczos_resample_8x12bit(float *dst, const float *src, size_t count)   { shim_scatter(dst, src, count, 8, 28); }
        inline void lanczos_resample_8x16bit(float *dst, const float *src, size_t count)   { shim_scatter(dst, src, count, 8, 29); }
        inline void lanczos_resample_8x24bit(float *dst, const float *src, size_t count)   { shim_scatter(dst, src, count, 8, 30); }

        inline void downsample_2x(float *dst, const float *src, size_t count)     { shim_decimate(dst, src, count, 2); }
        inline void downsample_3x(float *dst, const float *src, size_t count)     { shim_decimate(dst, src, count, 3); }
        inline void downsample_4x(float *dst, const float *src, size_t count)     { shim_decimate(dst, src, count, 4); }
        inline void downsample_6x(float *dst, const float *src, size_t count)     { shim_decimate(dst, src, count, 6); }
        inline void downsample_8x(float *dst, const float *src, size_t count)     { shim_decimate(dst, src, count, 8); }
    }
}

#endif
