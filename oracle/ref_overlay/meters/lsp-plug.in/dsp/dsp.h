// Ahead of oracle/ref_overlay/filters' and oracle/ref_shim's <lsp-plug.in/dsp/dsp.h> for oracle/_ref/loudness_ref only: what
// LoudnessMeter.cpp takes from lsp-dsp-lib beside those (ILUFSMeter.cpp needs nothing more).  All of it is OURS: plain loops
// written from the call sites, NOT lsp-dsp-lib's code, and they pin none of its SIMD variants.
#ifndef ORACLE_REF_OVERLAY_METERS_DSP_H_
#define ORACLE_REF_OVERLAY_METERS_DSP_H_

#include_next <lsp-plug.in/dsp/dsp.h>

namespace lsp
{
    namespace dsp
    {
        // UNPINNED, a stand-in by this project's reading.  LoudnessMeter.cpp:393, :403-404 h_sum(src, count): a serial float32 sum
        // from 0, oldest cell first, each partial sum rounded on its own (as h_sqr_sum / h_abs_sum of oracle/ref_shim).
        // lsp-dsp-lib's SIMD variants add in another order; nothing in the reference tree pins which.
        inline float h_sum(const float *src, size_t count)
        {
            float sum = 0.0f;
            for (size_t i = 0; i < count; ++i)
                sum += src[i];
            return sum;
        }

        // :434-438 sqr2(dst, src, count): "put the squared input data to the buffer"
        inline void sqr2(float *dst, const float *src, size_t count)
        {
            for (size_t i = 0; i < count; ++i)
                dst[i] = src[i] * src[i];
        }

        // :455 fmadd_k3(vBuffer, c->vMS, c->fWeight, samples): "add mean square values to the loudness estimation buffer",
        // beside mul_k3 for the first channel: dst += src * k, the product rounded before the sum (no contraction)
        inline void fmadd_k3(float *dst, const float *src, float k, size_t count)
        {
            for (size_t i = 0; i < count; ++i)
                dst[i] = dst[i] + src[i] * k;
        }

        // :503, :553 mix_copy2(dst, a, b, ka, kb, count): the linked channel output, dst = a * ka + b * kb
        inline void mix_copy2(float *dst, const float *a, const float *b, float ka, float kb, size_t count)
        {
            for (size_t i = 0; i < count; ++i)
                dst[i] = a[i] * ka + b[i] * kb;
        }
    }
}

#endif
