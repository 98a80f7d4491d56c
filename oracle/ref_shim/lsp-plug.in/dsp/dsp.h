// STAND-IN for lsp-dsp-lib's <lsp-plug.in/dsp/dsp.h>, which the reference tree does not carry.  Only what Compressor,
// Expander, Gate, DynamicProcessor and Limiter take from it: dsp::copy, the knee structs, the eight array gain primitives, and
// Limiter.cpp's buffer primitives (AutoGain and SimpleAutoGain take nothing), and what Sidechain.cpp and RawRingBuffer.cpp take
// (at the end of this file).
//
// The primitives are plain loops of the formula that each class states in full in its own scalar overload
// (Compressor::reduction(float) / curve(float), Expander::amplification(float) / curve(float), Gate::amplification(float, bool)
// / curve(float, bool)).  They are NOT lsp-dsp-lib's code and pin none of its SIMD variants; the vector generator asserts, on
// every level and envelope sample it records, that each loop returns the bits of the class's scalar overload, so what is
// recorded as the reference's gain is what the reference's own text computes.  No follower, settings or hysteresis
// arithmetic lives here.
#ifndef ORACLE_REF_SHIM_DSP_DSP_H_
#define ORACLE_REF_SHIM_DSP_DSP_H_

#include <cmath>
#include <cstring>
#include <lsp-plug.in/common/types.h>

namespace lsp
{
    namespace dsp
    {
        struct compressor_knee_t    { float start, end, gain, herm[3], tilt[2]; };
        struct compressor_x2_t      { compressor_knee_t k[2]; };
        struct expander_knee_t      { float start, end, threshold, herm[3], tilt[2]; };
        struct gate_knee_t          { float start, end, gain_start, gain_end, herm[4]; };

        inline void copy(float *dst, const float *src, size_t count)
        {
            if (dst != src)
                memmove(dst, src, count * sizeof(float));
        }

        // ---- compressor: two knees, their gains multiplied ------------------------------------------------------------
        inline float shim_compressor_gain(const compressor_x2_t *c, float x)
        {
            if ((x <= c->k[0].start) && (x <= c->k[1].start))
                return c->k[0].gain * c->k[1].gain;
            float lx = logf(x), g[2];
            for (size_t j = 0; j < 2; ++j)
            {
                const compressor_knee_t *k = &c->k[j];
                g[j] = (x <= k->start) ? k->gain :
                       (x >= k->end) ? expf(lx * k->tilt[0] + k->tilt[1]) :
                       expf((k->herm[0] * lx + k->herm[1]) * lx + k->herm[2]);
            }
            return g[0] * g[1];
        }

        inline void compressor_x2_gain(float *dst, const float *src, const compressor_x2_t *c, size_t count)
        {
            for (size_t i = 0; i < count; ++i)
                dst[i] = shim_compressor_gain(c, fabsf(src[i]));
        }

        inline void compressor_x2_curve(float *dst, const float *src, const compressor_x2_t *c, size_t count)
        {
            for (size_t i = 0; i < count; ++i)
            {
                float x = fabsf(src[i]);
                // the scalar overload's two returns: (gain0 * gain1) * x below both knees, (g1 * g2) * x elsewhere
                dst[i] = shim_compressor_gain(c, x) * x;
            }
        }

        // ---- gate: one knee, a cubic in ln x ----------------------------------------------------------------------------
        inline float shim_gate_gain(const gate_knee_t *c, float x)
        {
            if (x <= c->start)
                return c->gain_start;
            if (x >= c->end)
                return c->gain_end;
            float lx = logf(x);
            return expf(((c->herm[0] * lx + c->herm[1]) * lx + c->herm[2]) * lx + c->herm[3]);
        }

        inline void gate_x1_gain(float *dst, const float *src, const gate_knee_t *c, size_t count)
        {
            for (size_t i = 0; i < count; ++i)
                dst[i] = shim_gate_gain(c, fabsf(src[i]));
        }

        inline void gate_x1_curve(float *dst, const float *src, const gate_knee_t *c, size_t count)
        {
            for (size_t i = 0; i < count; ++i)
            {
                float x = fabsf(src[i]);
                dst[i] = x * shim_gate_gain(c, x);
            }
        }

        // ---- expander, upward: the level limited to the threshold ------------------------------------------------------
        inline float shim_uexpander_gain(const expander_knee_t *c, float *x)
        {
            if (*x > c->threshold)
                *x = c->threshold;
            if (*x > c->start)
            {
                float lx = logf(*x);
                return (*x >= c->end) ? expf(c->tilt[0] * lx + c->tilt[1]) :
                                        expf((c->herm[0] * lx + c->herm[1]) * lx + c->herm[2]);
            }
            return 1.0f;
        }

        inline void uexpander_x1_gain(float *dst, const float *src, const expander_knee_t *c, size_t count)
        {
            for (size_t i = 0; i < count; ++i)
            {
                float x = fabsf(src[i]);
                dst[i] = shim_uexpander_gain(c, &x);
            }
        }

        inline void uexpander_x1_curve(float *dst, const float *src, const expander_knee_t *c, size_t count)
        {
            for (size_t i = 0; i < count; ++i)
            {
                float x = fabsf(src[i]);
                float g = shim_uexpander_gain(c, &x);
                dst[i] = (x > c->start) ? x * g : x;
            }
        }

        // ---- expander, downward: nothing below the threshold ------------------------------------------------------------
        inline void dexpander_x1_gain(float *dst, const float *src, const expander_knee_t *c, size_t count)
        {
            for (size_t i = 0; i < count; ++i)
            {
                float x = fabsf(src[i]);
                if (x < c->threshold)
                    dst[i] = 0.0f;
                else if (x < c->end)
                {
                    float lx = logf(x);
                    dst[i] = (x <= c->start) ? expf(c->tilt[0] * lx + c->tilt[1]) :
                                               expf((c->herm[0] * lx + c->herm[1]) * lx + c->herm[2]);
                }
                else
                    dst[i] = 1.0f;
            }
        }

        inline void dexpander_x1_curve(float *dst, const float *src, const expander_knee_t *c, size_t count)
        {
            for (size_t i = 0; i < count; ++i)
            {
                float x = fabsf(src[i]);
                if (x < c->threshold)
                    dst[i] = 0.0f;
                else if (x < c->end)
                {
                    float lx = logf(x);
                    dst[i] = (x <= c->start) ? x * expf(c->tilt[0] * lx + c->tilt[1]) :
                                               x * expf((c->herm[0] * lx + c->herm[1]) * lx + c->herm[2]);
                }
                else
                    dst[i] = x;
            }
        }

        // ---- Limiter.cpp's buffer primitives, each written from its call sites ---------------------------------------------
        // :775 move(vGainBuf, &vGainBuf[nHead], 4 ML): the ranges overlap where nHead < 4 ML
        inline void move(float *dst, const float *src, size_t count)
        {
            memmove(dst, src, count * sizeof(float));
        }

        // :103, :404, :707 (the comments say "fill gain buffer"; construct() starts from a gain of one) and :104
        inline void fill_one(float *dst, size_t count)
        {
            for (size_t i = 0; i < count; ++i)
                dst[i] = 1.0f;
        }

        inline void fill_zero(float *dst, size_t count)
        {
            for (size_t i = 0; i < count; ++i)
                dst[i] = 0.0f;
        }

        // :415 mul_k2(gbuf, gnorm, nMaxLookahead): "lower gain since threshold has been lowered"
        inline void mul_k2(float *dst, float k, size_t count)
        {
            for (size_t i = 0; i < count; ++i)
                dst[i] *= k;
        }

        // UNPINNED, a stand-in by this project's reading.  :708, :712, :763 abs_mul3(vTmpBuf, gbuf, sc, to_do): "apply gain
        // to sidechain", the result compared with the threshold as a level: a[i] * |b[i]|.  The reference tree does not carry
        // lsp-dsp-lib, so neither the operand that loses its sign nor the order of the product is pinned by anything here.
        inline void abs_mul3(float *dst, const float *a, const float *b, size_t count)
        {
            for (size_t i = 0; i < count; ++i)
                dst[i] = a[i] * fabsf(b[i]);
        }

        // UNPINNED, a stand-in by this project's reading.  :721 max_index(vTmpBuf, to_do): "find peak": the FIRST index of
        // the maximum.  Which of two equal maxima lsp-dsp-lib returns (and what its SIMD variants return) is not pinned by
        // anything here; the vectors hold a case with two exactly equal peaks so that whoever pins it later sees it move.
        inline size_t max_index(const float *src, size_t count)
        {
            size_t idx = 0;
            for (size_t i = 1; i < count; ++i)
                if (src[i] > src[idx])
                    idx = i;
            return idx;
        }

        // ---- Sidechain.cpp's and RawRingBuffer.cpp's primitives ---------------------------------------------------------------
        // Each is the plain loop of what the class's scalar preprocess(float *, const float *) states (Sidechain.cpp:335-437);
        // tests/golden/make_sidechain_vectors.py asserts, on every recorded sample, that the array path returns the bits of
        // that scalar overload.
        inline void fill(float *dst, float value, size_t count)
        {
            for (size_t i = 0; i < count; ++i)
                dst[i] = value;
        }

        inline void abs1(float *dst, size_t count)                                  // :435 (s < 0.0f) ? -s : s
        {
            for (size_t i = 0; i < count; ++i)
                dst[i] = (dst[i] < 0.0f) ? -dst[i] : dst[i];
        }

        inline void abs2(float *dst, const float *src, size_t count)
        {
            for (size_t i = 0; i < count; ++i)
                dst[i] = (src[i] < 0.0f) ? -src[i] : src[i];
        }

        inline void lr_to_mid(float *m, const float *l, const float *r, size_t count)      // :395
        {
            for (size_t i = 0; i < count; ++i)
                m[i] = (l[i] + r[i]) * 0.5f;
        }

        inline void lr_to_side(float *s, const float *l, const float *r, size_t count)     // :400
        {
            for (size_t i = 0; i < count; ++i)
                s[i] = (l[i] - r[i]) * 0.5f;
        }

        inline void ms_to_left(float *l, const float *m, const float *s, size_t count)     // :346
        {
            for (size_t i = 0; i < count; ++i)
                l[i] = m[i] + s[i];
        }

        inline void ms_to_right(float *r, const float *m, const float *s, size_t count)    // :351
        {
            for (size_t i = 0; i < count; ++i)
                r[i] = m[i] - s[i];
        }

        inline float shim_smin(float a, float b)    { return (fabsf(a) < fabsf(b)) ? a : b; }      // :405, :368
        inline float shim_smax(float a, float b)    { return (fabsf(b) < fabsf(a)) ? a : b; }      // :410, :375
        inline float shim_abs(float s)              { return (s < 0.0f) ? -s : s; }                // :435

        inline void psmin3(float *dst, const float *a, const float *b, size_t count)
        {
            for (size_t i = 0; i < count; ++i)
                dst[i] = shim_smin(a[i], b[i]);
        }

        inline void psmax3(float *dst, const float *a, const float *b, size_t count)
        {
            for (size_t i = 0; i < count; ++i)
                dst[i] = shim_smax(a[i], b[i]);
        }

        inline void pamin3(float *dst, const float *a, const float *b, size_t count)
        {
            for (size_t i = 0; i < count; ++i)
                dst[i] = shim_abs(shim_smin(a[i], b[i]));
        }

        inline void pamax3(float *dst, const float *a, const float *b, size_t count)
        {
            for (size_t i = 0; i < count; ++i)
                dst[i] = shim_abs(shim_smax(a[i], b[i]));
        }

        inline void ms_pamin3(float *dst, const float *m, const float *s, size_t count)    // :366-368
        {
            for (size_t i = 0; i < count; ++i)
                dst[i] = shim_abs(shim_smin(m[i] + s[i], m[i] - s[i]));
        }

        inline void ms_pamax3(float *dst, const float *m, const float *s, size_t count)    // :373-375
        {
            for (size_t i = 0; i < count; ++i)
                dst[i] = shim_abs(shim_smax(m[i] + s[i], m[i] - s[i]));
        }

        // Sidechain.cpp:231, :241 call these on the mid and side rows, ahead of a pre-equalizer only.  No recorded case has a
        // pre-equalizer, so they are never run; they are here for the class to compile and link.
        inline void lr_psmin3(float *dst, const float *l, const float *r, size_t count)
        {
            for (size_t i = 0; i < count; ++i)
                dst[i] = shim_smin((l[i] + r[i]) * 0.5f, (l[i] - r[i]) * 0.5f);
        }

        inline void lr_psmax3(float *dst, const float *l, const float *r, size_t count)
        {
            for (size_t i = 0; i < count; ++i)
                dst[i] = shim_smax((l[i] + r[i]) * 0.5f, (l[i] - r[i]) * 0.5f);
        }

        // UNPINNED, a stand-in by this project's reading.  :158-161, :171-174 h_abs_sum / h_sqr_sum(src, count): a serial
        // float32 sum from 0, oldest sample first, each term and each partial sum rounded on its own.  lsp-dsp-lib's SIMD
        // variants add in another order; nothing here pins which.  The stereo meters' and the Depopper's vectors use the same.
        inline float h_abs_sum(const float *src, size_t count)
        {
            float sum = 0.0f;
            for (size_t i = 0; i < count; ++i)
                sum += fabsf(src[i]);
            return sum;
        }

        inline float h_sqr_sum(const float *src, size_t count)
        {
            float sum = 0.0f;
            for (size_t i = 0; i < count; ++i)
                sum += src[i] * src[i];
            return sum;
        }

        // UNPINNED, a stand-in by this project's reading.  :539 ssqrt1(out, to_do), "saturated" square root: sqrtf of the
        // value clamped at 0, as the single-sample overload states it (:614, (rms < 0.0f) ? 0.0f : sqrtf(...)).
        inline void ssqrt1(float *dst, size_t count)
        {
            for (size_t i = 0; i < count; ++i)
                dst[i] = (dst[i] > 0.0f) ? sqrtf(dst[i]) : 0.0f;
        }
    }
}

#endif
