// Minimal stand-in for the lsp-dsp-lib types that appear in the lsp::dspu class API
// (FilterBank::add_chain() hands out dsp::biquad_x1_t, Filter keeps dsp::f_cascade_t).
// Only the two plain structs are provided; the arithmetic of lsp-dsp-lib is replaced by the GPU library.
#ifndef MI_LSP_PLUG_IN_DSP_DSP_H_
#define MI_LSP_PLUG_IN_DSP_DSP_H_

#include <cstddef>
#include <cstdint>
#include <sys/types.h>

namespace lsp
{
    // status codes used by the few hot-path APIs that return one
    typedef int status_t;
    // (lsp-common-lib's status.h is not part of the reference tree: callers compare these symbolically)
    enum { STATUS_OK = 0, STATUS_NO_MEM = 5, STATUS_BAD_STATE = 12, STATUS_OVERFLOW = 18, STATUS_INVALID_VALUE = 27,
           STATUS_NOT_BOUND = 50 };

    namespace dsp
    {
        // one digital section: y = b0 x + b1 x[-1] + b2 x[-2] + a1 y[-1] + a2 y[-2]; p* pad to 32 bytes
        struct biquad_x1_t
        {
            float b0, b1, b2;
            float a1, a2;
            float p0, p1, p2;
        };

        // lsp-dsp-lib's packed banks, kept for layout only (FilterBank holds a pointer of this type; field use as in
        // src/main/filters/FilterBank.cpp:112-230 of the reference): 16 delay values, then the coefficients of one
        // x1 / x2 / x4 / x8 group, 256 bytes, 64-byte aligned.  Nothing in this library computes with it.
        struct biquad_x2_t { float b0[2], b1[2], b2[2], a1[2], a2[2], p[2]; };
        struct biquad_x4_t { float b0[4], b1[4], b2[4], a1[4], a2[4]; };
        struct biquad_x8_t { float b0[8], b1[8], b2[8], a1[8], a2[8]; };
        struct alignas(64) biquad_t
        {
            float d[16];
            union
            {
                biquad_x1_t x1;
                biquad_x2_t x2;
                biquad_x4_t x4;
                biquad_x8_t x8;
            };
            float __pad[8];
        };
        static_assert(sizeof(biquad_x1_t) == 32 && sizeof(biquad_x8_t) == 160 && sizeof(biquad_t) == 256, "lsp-dsp-lib layouts");

        // numerator t[] / denominator b[] of an analog second-order cascade
        struct f_cascade_t
        {
            float t[4];
            float b[4];
        };

        // lsp-dsp-lib's resampling function type (TruePeakMeter keeps one): dst receives the oversampled src
        typedef void (*resampling_function_t)(float *dst, const float *src, size_t count);

        // lsp-dsp-lib's compressor curve (Compressor keeps one): below start the constant gain, above end
        // exp(tilt[0] ln x + tilt[1]), between them exp((herm[0] ln x + herm[1]) ln x + herm[2]); two knees multiply
        struct compressor_knee_t
        {
            float start;
            float end;
            float gain;
            float herm[3];
            float tilt[2];
        };
        struct compressor_x2_t { compressor_knee_t k[2]; };
        static_assert(sizeof(compressor_knee_t) == 32 && sizeof(compressor_x2_t) == 64, "lsp-dsp-lib layouts");

        // lsp-dsp-lib's expander curve (Expander keeps one): a tilt line exp(tilt[0] ln x + tilt[1]) and a knee
        // exp((herm[0] ln x + herm[1]) ln x + herm[2]) between start and end; threshold is the ceiling of the level (upward)
        // or the level below which the gain is 0 (downward)
        struct expander_knee_t
        {
            float start;
            float end;
            float threshold;
            float herm[3];
            float tilt[2];
        };
        // lsp-dsp-lib's gate curve (Gate keeps two): gain_start up to start, gain_end from end on, between them
        // exp(((herm[0] ln x + herm[1]) ln x + herm[2]) ln x + herm[3])
        struct gate_knee_t
        {
            float start;
            float end;
            float gain_start;
            float gain_end;
            float herm[4];
        };
        static_assert(sizeof(expander_knee_t) == 32 && sizeof(gate_knee_t) == 32, "lsp-dsp-lib layouts");

        // lsp-dsp-lib's correlation state (Correlometer keeps one): the window sums of a*b, a*a and b*b
        struct correlation_t
        {
            float v;
            float a;
            float b;
        };
        static_assert(sizeof(correlation_t) == 12, "lsp-dsp-lib layouts");

        // lsp-dsp-lib's per-thread context / init are no-ops here: there is no SIMD dispatch to select
        struct context_t { uint32_t top; uint32_t data[15]; };
        inline void init() {}
        inline void start(context_t *) {}
        inline void finish(context_t *) {}
    }
}

#endif
