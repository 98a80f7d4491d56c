// Ahead of oracle/ref_shim's <lsp-plug.in/dsp/dsp.h> for oracle/_ref/filter_ref (Filter.cpp and FilterBank.cpp compiled
// UNMODIFIED) and oracle/_ref/dynfilter_ref (DynamicFilters.cpp likewise) only: what the three take from lsp-dsp-lib beside
// dsp::copy / fill / fill_zero / fill_one.  All of it is OURS.
//
// The structs have the fields that FilterBank.cpp:112-230 and Filter.cpp name.  UNPINNED: the arithmetic.  biquad_process_x1 /
// x2 / x4 / x8 are the serial recurrence of oracle/biquad_oracle.c (orc_biquad_cascade), section by section in chain order, NOT
// lsp-dsp-lib's code; with them filter_ref pins what the reference's own text decides -- which sections a design has, how
// FilterBank::end packs them into x8 / x4 / x2 / x1 groups, when the delays are cleared and when they are kept, and
// impulse_response()'s backup of d[] -- and nothing of the rounding inside a section.  tests/golden/make_filter_vectors.py
// asserts that every recorded output is orc_biquad_cascade on the recorded sections bit for bit, so the packing has no arithmetic
// effect under this stand-in.  filter_transfer_* (freq_chart of the bilinear and matched designs) end the program: no recorded case
// may depend on them.
#ifndef ORACLE_REF_OVERLAY_FILTERS_DSP_H_
#define ORACLE_REF_OVERLAY_FILTERS_DSP_H_

#include <cstdio>
#include <cstdlib>
#include <lsp-plug.in/common/types.h>
#include_next <lsp-plug.in/dsp/dsp.h>

#define LSP_DSP_BIQUAD_ALIGN        0x40
#define LSP_DSP_BIQUAD_D_ITEMS      16

namespace lsp
{
    namespace dsp
    {
        struct biquad_x1_t { float b0, b1, b2, a1, a2, p0, p1, p2; };
        struct biquad_x2_t { float b0[2], b1[2], b2[2], a1[2], a2[2], p[2]; };
        struct biquad_x4_t { float b0[4], b1[4], b2[4], a1[4], a2[4]; };
        struct biquad_x8_t { float b0[8], b1[8], b2[8], a1[8], a2[8]; };

        // d[]: this stand-in keeps section j's d0 at d[j] and its d1 at d[N + j] in a group of N; FilterBank only zeroes, saves
        // and restores the sixteen values as a whole
        struct __attribute__((aligned(LSP_DSP_BIQUAD_ALIGN))) biquad_t
        {
            float d[LSP_DSP_BIQUAD_D_ITEMS];
            union
            {
                biquad_x1_t x1;
                biquad_x2_t x2;
                biquad_x4_t x4;
                biquad_x8_t x8;
            };
            float __pad[8];
        };

        struct f_cascade_t { float t[4], b[4]; };

        // one section over the whole block: y = b0 x + d0, d0' = d1 + (b1 x + a1 y), d1' = b2 x + a2 y
        inline void shim_biquad_section(float *dst, const float *src, size_t count, float b0, float b1, float b2, float a1, float a2,
                                        float *d0p, float *d1p)
        {
            float d0 = *d0p, d1 = *d1p;
            for (size_t i = 0; i < count; ++i)
            {
                const float x  = src[i];
                const float y  = b0 * x + d0;
                const float p1 = b1 * x + a1 * y;
                const float p2 = b2 * x + a2 * y;
                d0      = d1 + p1;
                d1      = p2;
                dst[i]  = y;
            }
            *d0p = d0;
            *d1p = d1;
        }

        inline void biquad_process_x1(float *dst, const float *src, size_t count, biquad_t *f)
        {
            const biquad_x1_t *c = &f->x1;
            shim_biquad_section(dst, src, count, c->b0, c->b1, c->b2, c->a1, c->a2, &f->d[0], &f->d[1]);
        }

        inline void biquad_process_x2(float *dst, const float *src, size_t count, biquad_t *f)
        {
            const biquad_x2_t *c = &f->x2;
            for (size_t j = 0; j < 2; ++j)
                shim_biquad_section(dst, (j == 0) ? src : dst, count, c->b0[j], c->b1[j], c->b2[j], c->a1[j], c->a2[j], &f->d[j], &f->d[2 + j]);
        }

        inline void biquad_process_x4(float *dst, const float *src, size_t count, biquad_t *f)
        {
            const biquad_x4_t *c = &f->x4;
            for (size_t j = 0; j < 4; ++j)
                shim_biquad_section(dst, (j == 0) ? src : dst, count, c->b0[j], c->b1[j], c->b2[j], c->a1[j], c->a2[j], &f->d[j], &f->d[4 + j]);
        }

        inline void biquad_process_x8(float *dst, const float *src, size_t count, biquad_t *f)
        {
            const biquad_x8_t *c = &f->x8;
            for (size_t j = 0; j < 8; ++j)
                shim_biquad_section(dst, (j == 0) ? src : dst, count, c->b0[j], c->b1[j], c->b2[j], c->a1[j], c->a2[j], &f->d[j], &f->d[8 + j]);
        }

        // Filter.cpp:547, :647 mul_k3(freqs, f, kf, to_do): dst = src * k.  Reached only on the way to filter_transfer_*.
        inline void mul_k3(float *dst, const float *src, float k, size_t count)
        {
            for (size_t i = 0; i < count; ++i)
                dst[i] = src[i] * k;
        }

        // Filter.cpp:693 pcomplex_fill_ri(c, 1.0f, 0.0f, count): `count` packed complex numbers re, im
        inline void pcomplex_fill_ri(float *dst, float re, float im, size_t count)
        {
            for (size_t i = 0; i < count; ++i)
            {
                dst[2 * i]      = re;
                dst[2 * i + 1]  = im;
            }
        }

        inline void shim_not_pinned(const char *what)
        {
            fprintf(stderr, "%s reached: no recorded case may depend on it\n", what);
            abort();
        }

        // ---- DynamicFilters.cpp (oracle/_ref/dynfilter_ref) -------------------------------------------------------------------
        // UNPINNED, all of it.  DynamicFilters.cpp:340, :529 irootf(x, n): the n-th root, here expf(logf(x) / n) in float as
        // oracle/dynamic_filters.py restates it; lsp-dsp-lib's own method is not in the reference tree.
        inline float irootf(float x, uint32_t n)
        {
            return expf(logf(x) / float(n));
        }

        // A recording stand-in (as the Oversampler's overlay has for dspu::Filter): every transform hands the cascade array it was
        // given, and the sections it made of it (5 floats per cascade, in the array's order), to the driver's hook: `lanes` cascades
        // per row, `rows` rows, in the diagonal layout of DynamicFilters.cpp
        // (the values of sample n for lane j stand in row n + j).  That array is the reference's own text at work: which cascades
        // a type has, their grouping into 8 / 4 / 2 / 1, and every t[] and b[].
        typedef void (*shim_cascade_hook_t)(const f_cascade_t *bc, const float *sections, size_t lanes, size_t rows, float kf, float f, bool matched);
        inline shim_cascade_hook_t &shim_cascade_hook()
        {
            static shim_cascade_hook_t hook = NULL;
            return hook;
        }

        // Filter::bilinear_transform (Filter.cpp:2225-2262) on one cascade, in float as oracle/dynamic_filters.py::bilinear
        inline void shim_bilinear(float *q, const f_cascade_t *c, float kf)
        {
            const float kf2 = kf * kf;
            const float T0 = c->t[0], T1 = c->t[1] * kf, T2 = c->t[2] * kf2;
            const float B0 = c->b[0], B1 = c->b[1] * kf, B2 = c->b[2] * kf2;
            const float N  = 1.0f / (B0 + B1 + B2);
            q[0] = (T0 + T1 + T2) * N;
            q[1] = 2.0f * (T0 - T2) * N;
            q[2] = (T0 - T1 + T2) * N;
            q[3] = 2.0f * (B2 - B0) * N;
            q[4] = (B1 - B2 - B0) * N;
        }

        // The matched Z transform of one cascade, in the shape of this project's own restatement (csrc/dynfilter.hip: matched_poly,
        // matched_one, matched) of what Filter::matched_transform (Filter.cpp:2291-2416) computes: the digital image of each
        // polynomial in float, the amplitude match in double, td = 2 pi / sample rate handed in, the match point w = 0.1 f td.
        inline void shim_matched_poly(const float *p, float f, float td, float *Qo)
        {
            Qo[0] = Qo[1] = Qo[2] = 0.0f;
            if (p[2] == 0.0f)
            {
                if (p[1] == 0.0f)
                    Qo[0] = p[0];
                else
                {
                    const float k = p[1] / f, R = -p[0] / k;
                    Qo[0] = k;
                    Qo[1] = -k * expf(R * td);
                }
                return;
            }
            const float k = p[2], qa = 1.0f / (f * f), qb = p[1] / (f * p[2]), qc = p[0] / p[2];
            float D = qb * qb - 4.0f * qa * qc;
            if (D >= 0)
            {
                D = sqrtf(D);
                const float R0 = (-qb - D) / (2.0f * qa), R1 = (-qb + D) / (2.0f * qa);
                Qo[0] = k;
                Qo[1] = -k * (expf(R0 * td) + expf(R1 * td));
                Qo[2] = k * expf((R0 + R1) * td);
            }
            else
            {
                D = sqrtf(-D);
                const float R = -qb / (2.0f * qa), K = D / (2.0f * qa);
                Qo[0] = k;
                Qo[1] = -2.0f * k * expf(R * td) * cosf(K * td);
                Qo[2] = k * expf(2.0f * R * td);
            }
        }

        struct shim_matched_side { float P[3]; double A, I; };     // a polynomial's digital image, |digital| and |analog| at the match point

        inline shim_matched_side shim_matched_one(const float *p, float f, float td, double w)
        {
            shim_matched_side r;
            shim_matched_poly(p, f, td, r.P);
            double re = r.P[0] * cos(2.0 * w) + r.P[1] * cos(w) + r.P[2];
            double im = r.P[0] * sin(2.0 * w) + r.P[1] * sin(w);
            r.A = sqrt(re * re + im * im);
            re = p[0] - p[2] * 0.01;
            im = p[1] * 0.1;
            r.I = sqrt(re * re + im * im);
            return r;
        }

        inline void shim_matched(float *q, const f_cascade_t *c, float f, float td)
        {
            const double w = 0.1 * double(f) * double(td);
            const shim_matched_side n = shim_matched_one(c->t, f, td, w), d = shim_matched_one(c->b, f, td, w);
            const double AN = (d.A * n.I) / (n.A * d.I), N = 1.0 / d.P[0];
            q[0] = float(n.P[0] * N * AN); q[1] = float(n.P[1] * N * AN); q[2] = float(n.P[2] * N * AN);
            q[3] = float(-d.P[1] * N); q[4] = float(-d.P[2] * N);
        }

        // -> the sections of a whole cascade array, 5 floats each in the array's order (the caller frees them)
        inline float *shim_sections(const f_cascade_t *bc, size_t count, float kf, float f, bool matched)
        {
            float *q = new float[5 * count + 1];
            for (size_t i = 0; i < count; ++i)
            {
                if (matched)
                    shim_matched(&q[5 * i], &bc[i], f, kf);
                else
                    shim_bilinear(&q[5 * i], &bc[i], kf);
            }
            return q;
        }

        template <class BQ>
        inline void shim_transform(BQ *bf, const f_cascade_t *bc, size_t lanes, size_t rows, float kf, float f, bool matched)
        {
            float *q = shim_sections(bc, lanes * rows, kf, f, matched);
            if (shim_cascade_hook() != NULL)
                shim_cascade_hook()(bc, q, lanes, rows, kf, f, matched);
            for (size_t r = 0; r < rows; ++r)
                for (size_t j = 0; j < lanes; ++j)
                {
                    const float *v = &q[5 * (r * lanes + j)];
                    bf[r].b0[j] = v[0]; bf[r].b1[j] = v[1]; bf[r].b2[j] = v[2]; bf[r].a1[j] = v[3]; bf[r].a2[j] = v[4];
                }
            delete [] q;
        }

        // one cascade per row: biquad_x1_t has scalars for the arrays of the wider ones
        inline void shim_transform_x1(biquad_x1_t *bf, const f_cascade_t *bc, size_t count, float kf, float f, bool matched)
        {
            float *q = shim_sections(bc, count, kf, f, matched);
            if (shim_cascade_hook() != NULL)
                shim_cascade_hook()(bc, q, 1, count, kf, f, matched);
            for (size_t r = 0; r < count; ++r)
            {
                const float *v = &q[5 * r];
                bf[r].b0 = v[0]; bf[r].b1 = v[1]; bf[r].b2 = v[2]; bf[r].a1 = v[3]; bf[r].a2 = v[4];
                bf[r].p0 = bf[r].p1 = bf[r].p2 = 0.0f;
            }
            delete [] q;
        }

        inline void bilinear_transform_x1(biquad_x1_t *bf, const f_cascade_t *bc, float kf, size_t count)               { shim_transform_x1(bf, bc, count, kf, 0.0f, false); }
        inline void matched_transform_x1(biquad_x1_t *bf, const f_cascade_t *bc, float f, float td, size_t count)       { shim_transform_x1(bf, bc, count, td, f, true); }
        inline void bilinear_transform_x2(biquad_x2_t *bf, const f_cascade_t *bc, float kf, size_t count)   { shim_transform(bf, bc, 2, count, kf, 0.0f, false); }
        inline void bilinear_transform_x4(biquad_x4_t *bf, const f_cascade_t *bc, float kf, size_t count)   { shim_transform(bf, bc, 4, count, kf, 0.0f, false); }
        inline void bilinear_transform_x8(biquad_x8_t *bf, const f_cascade_t *bc, float kf, size_t count)   { shim_transform(bf, bc, 8, count, kf, 0.0f, false); }
        inline void matched_transform_x2(biquad_x2_t *bf, const f_cascade_t *bc, float f, float td, size_t count)   { shim_transform(bf, bc, 2, count, td, f, true); }
        inline void matched_transform_x4(biquad_x4_t *bf, const f_cascade_t *bc, float f, float td, size_t count)   { shim_transform(bf, bc, 4, count, td, f, true); }
        inline void matched_transform_x8(biquad_x8_t *bf, const f_cascade_t *bc, float f, float td, size_t count)   { shim_transform(bf, bc, 8, count, td, f, true); }

        // dyn_biquad_process_x*: orc_dyn_biquad_cascade's recurrence (oracle/biquad_oracle.c), section by section; section j takes
        // its coefficients for sample n from row n + j.  d[]: section j's d0 at d[2 j], its d1 at d[2 j + 1].
        template <class BQ>
        inline void shim_dyn_process(float *dst, const float *src, float *d, size_t count, const BQ *bf, size_t lanes)
        {
            for (size_t j = 0; j < lanes; ++j)
            {
                float d0 = d[2 * j], d1 = d[2 * j + 1];
                const float *in = (j == 0) ? src : dst;
                for (size_t i = 0; i < count; ++i)
                {
                    const BQ *q    = &bf[i + j];
                    const float x  = in[i];
                    const float y  = q->b0[j] * x + d0;
                    const float p1 = q->b1[j] * x + q->a1[j] * y;
                    const float p2 = q->b2[j] * x + q->a2[j] * y;
                    d0      = d1 + p1;
                    d1      = p2;
                    dst[i]  = y;
                }
                d[2 * j] = d0;
                d[2 * j + 1] = d1;
            }
        }

        inline void dyn_biquad_process_x1(float *dst, const float *src, float *d, size_t count, const biquad_x1_t *bf)
        {
            float d0 = d[0], d1 = d[1];
            for (size_t i = 0; i < count; ++i)
            {
                const biquad_x1_t *q = &bf[i];
                const float x  = src[i];
                const float y  = q->b0 * x + d0;
                const float p1 = q->b1 * x + q->a1 * y;
                const float p2 = q->b2 * x + q->a2 * y;
                d0      = d1 + p1;
                d1      = p2;
                dst[i]  = y;
            }
            d[0] = d0;
            d[1] = d1;
        }
        inline void dyn_biquad_process_x2(float *dst, const float *src, float *d, size_t count, const biquad_x2_t *bf)  { shim_dyn_process(dst, src, d, count, bf, 2); }
        inline void dyn_biquad_process_x4(float *dst, const float *src, float *d, size_t count, const biquad_x4_t *bf)  { shim_dyn_process(dst, src, d, count, bf, 4); }
        inline void dyn_biquad_process_x8(float *dst, const float *src, float *d, size_t count, const biquad_x8_t *bf)  { shim_dyn_process(dst, src, d, count, bf, 8); }

        inline void filter_transfer_calc_ri(float *, float *, const f_cascade_t *, const float *, size_t)   { shim_not_pinned("filter_transfer_calc_ri"); }
        inline void filter_transfer_apply_ri(float *, float *, const f_cascade_t *, const float *, size_t)  { shim_not_pinned("filter_transfer_apply_ri"); }
        inline void filter_transfer_calc_pc(float *, const f_cascade_t *, const float *, size_t)            { shim_not_pinned("filter_transfer_calc_pc"); }
        inline void filter_transfer_apply_pc(float *, const f_cascade_t *, const float *, size_t)           { shim_not_pinned("filter_transfer_apply_pc"); }
    }
}

#endif
