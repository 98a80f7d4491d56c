"""Writes tests/golden/oscillator_ref_vectors.npz: what the reference's own Oscillator class computes on a list of cases, and next to
it oscillator_public_names.json and oscillator_dump_keys.json.  Data only: operation lists, one source row, the reference's
output, the rows that get_periods returned (calls behind skipped periods that fit one buffer: the defined ones) and the settings
words each case ends with; names of public members; dump keys.  Run
where the reference tree exists:

    python tests/golden/make_oscillator_vectors.py [reference tree]

util/Oscillator.cpp, util/Oversampler.cpp, filters/Filter.cpp, filters/FilterBank.cpp and iface/IStateDumper.cpp are compiled
unmodified into a temporary directory (-O2 -ffp-contract=off -msse2 -mfpmath=sse) against oracle/ref_shim plus an overlay, written
here, of what that shim lacks: the biquad structs and constants of lsp-dsp-lib, and the dsp:: primitives that Oversampler and
FilterBank call as plain scalar C++ (a section is y = b0 x + d0, d0' = d1 + (b1 x + a1 y), d1' = b2 x + a2 y; the x2, x4 and x8 banks
are that section 2, 4 and 8 times in series; downsample_Nx keeps every N-th value; the Lanczos tables are what
mi_oversampler_coefficients documents; the oscillator never upsamples).  The program -- a stand-alone one with its own main -- is
built a first time with -fsanitize=address,undefined and run over every case before anything is recorded.

Every case is an operation list ops [k, 4] of (what, a, b, c) -- tests/oscillator_ref.py names them -- on a fresh object after init(),
and a source row src [N] that the add and mul operations read.  The process operations fill out [N] in order; GET_PERIODS operations
append to the case's periods.  No recorded trapezoid phase satisfies two branches of :430-443 (checked here with the restatement;
the sanitized run is the guard)."""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import oscillator_ref as R  # noqa: E402
from make_bypass_crossfade_vectors import npz_bytes, public_names  # noqa: E402

OUT = os.path.join(HERE, "oscillator_ref_vectors.npz")
f32 = np.float32

N = 1100
PIECES = (N, 1, 7, 256, 1023)
BL_MODES = {2: 1, 3: 8, 4: 15, 6: 22, 8: 29}            # 2X2, 3X3, 4X4, 6X12BIT, 8X16BIT

OVERLAY_VERSION = r'''
#ifndef OSC_OVERLAY_VERSION_H_
#define OSC_OVERLAY_VERSION_H_
#include <lsp-plug.in/common/types.h>
#ifndef LSP_DSP_UNITS_PUBLIC
#define LSP_DSP_UNITS_PUBLIC
#endif
#endif
'''

# the shim's types.h, and what Filter.cpp takes from lsp-common-lib besides: the alignment attribute and lsp_min / lsp_max of two types
OVERLAY_TYPES = r'''
#ifndef OSC_OVERLAY_TYPES_H_
#define OSC_OVERLAY_TYPES_H_
#include_next <lsp-plug.in/common/types.h>
#define __lsp_aligned32 __attribute__((aligned(32)))
namespace lsp
{
    template <class A, class B> inline A lsp_min(A a, B b) { return (a < A(b)) ? a : A(b); }
    template <class A, class B> inline A lsp_max(A a, B b) { return (a > A(b)) ? a : A(b); }
}
#endif
'''

OVERLAY_ALLOC = r'''
#ifndef OSC_OVERLAY_ALLOC_H_
#define OSC_OVERLAY_ALLOC_H_
#include_next <lsp-plug.in/common/alloc.h>
namespace lsp
{
    inline size_t align_size(size_t size, size_t align)     { return (size + align - 1) / align * align; }
    template <class T> inline T *align_ptr(T *ptr, size_t align = DEFAULT_ALIGN)
    {
        uintptr_t x = uintptr_t(ptr);
        return reinterpret_cast<T *>((x + align - 1) / align * align);
    }
}
#endif
'''

OVERLAY_DSP = r'''
#ifndef OSC_OVERLAY_DSP_H_
#define OSC_OVERLAY_DSP_H_
#include_next <lsp-plug.in/dsp/dsp.h>
#define LSP_DSP_BIQUAD_ALIGN            0x40
#define LSP_DSP_BIQUAD_D_ITEMS          16
#define LSP_DSP_RESAMPLING_RSV_SAMPLES  1024
namespace lsp
{
    namespace dsp
    {
        struct biquad_x1_t { float b0, b1, b2, a1, a2, p0, p1, p2; };
        struct biquad_x2_t { float b0[2], b1[2], b2[2], a1[2], a2[2], p[2]; };
        struct biquad_x4_t { float b0[4], b1[4], b2[4], a1[4], a2[4]; };
        struct biquad_x8_t { float b0[8], b1[8], b2[8], a1[8], a2[8]; };
        struct alignas(64) biquad_t
        {
            float d[16];
            union { biquad_x1_t x1; biquad_x2_t x2; biquad_x4_t x4; biquad_x8_t x8; };
            float __pad[8];
        };
        struct f_cascade_t { float t[4]; float b[4]; };

        inline void add2(float *dst, const float *src, size_t n)        { for (size_t i = 0; i < n; ++i) dst[i] = dst[i] + src[i]; }
        inline void mul2(float *dst, const float *src, size_t n)        { for (size_t i = 0; i < n; ++i) dst[i] = dst[i] * src[i]; }
        inline void mul_k3(float *dst, const float *src, float k, size_t n) { for (size_t i = 0; i < n; ++i) dst[i] = src[i] * k; }
        inline void pcomplex_fill_ri(float *dst, float re, float im, size_t n) { for (size_t i = 0; i < n; ++i) { dst[2 * i] = re; dst[2 * i + 1] = im; } }

        // H(jf) of one analog cascade: (t0 + t1 s + t2 s^2) / (b0 + b1 s + b2 s^2) at s = j f
        inline void osc_overlay_h(const f_cascade_t *c, float f, float *re, float *im)
        {
            float nr = c->t[0] - c->t[2] * f * f, ni = c->t[1] * f, dr = c->b[0] - c->b[2] * f * f, di = c->b[1] * f;
            float n = 1.0f / (dr * dr + di * di);
            *re = (nr * dr + ni * di) * n, *im = (ni * dr - nr * di) * n;
        }
        inline void filter_transfer_calc_ri(float *re, float *im, const f_cascade_t *c, const float *freq, size_t n)
        {
            for (size_t i = 0; i < n; ++i) osc_overlay_h(c, freq[i], &re[i], &im[i]);
        }
        inline void filter_transfer_apply_ri(float *re, float *im, const f_cascade_t *c, const float *freq, size_t n)
        {
            for (size_t i = 0; i < n; ++i)
            {
                float r, m; osc_overlay_h(c, freq[i], &r, &m);
                float a = re[i] * r - im[i] * m, b = re[i] * m + im[i] * r;
                re[i] = a, im[i] = b;
            }
        }
        inline void filter_transfer_calc_pc(float *dst, const f_cascade_t *c, const float *freq, size_t n)
        {
            for (size_t i = 0; i < n; ++i) osc_overlay_h(c, freq[i], &dst[2 * i], &dst[2 * i + 1]);
        }
        inline void filter_transfer_apply_pc(float *dst, const f_cascade_t *c, const float *freq, size_t n)
        {
            for (size_t i = 0; i < n; ++i)
            {
                float r, m; osc_overlay_h(c, freq[i], &r, &m);
                float a = dst[2 * i] * r - dst[2 * i + 1] * m, b = dst[2 * i] * m + dst[2 * i + 1] * r;
                dst[2 * i] = a, dst[2 * i + 1] = b;
            }
        }

        // `sections` sections in series; section j keeps its two delays in d[j] and d[j + sections]
        inline void osc_overlay_biquad(float *dst, const float *src, size_t n, float *d, size_t sections, const float *b0, const float *b1,
                                       const float *b2, const float *a1, const float *a2)
        {
            for (size_t i = 0; i < n; ++i)
            {
                float x = src[i];
                for (size_t j = 0; j < sections; ++j)
                {
                    float y  = b0[j] * x + d[j];
                    float p1 = b1[j] * x + a1[j] * y;
                    float p2 = b2[j] * x + a2[j] * y;
                    d[j] = d[j + sections] + p1;
                    d[j + sections] = p2;
                    x = y;
                }
                dst[i] = x;
            }
        }
        inline void biquad_process_x1(float *dst, const float *src, size_t n, biquad_t *f)
        {
            osc_overlay_biquad(dst, src, n, f->d, 1, &f->x1.b0, &f->x1.b1, &f->x1.b2, &f->x1.a1, &f->x1.a2);
        }
        inline void biquad_process_x2(float *dst, const float *src, size_t n, biquad_t *f)
        {
            osc_overlay_biquad(dst, src, n, f->d, 2, f->x2.b0, f->x2.b1, f->x2.b2, f->x2.a1, f->x2.a2);
        }
        inline void biquad_process_x4(float *dst, const float *src, size_t n, biquad_t *f)
        {
            osc_overlay_biquad(dst, src, n, f->d, 4, f->x4.b0, f->x4.b1, f->x4.b2, f->x4.a1, f->x4.a2);
        }
        inline void biquad_process_x8(float *dst, const float *src, size_t n, biquad_t *f)
        {
            osc_overlay_biquad(dst, src, n, f->d, 8, f->x8.b0, f->x8.b1, f->x8.b2, f->x8.a1, f->x8.a2);
        }

        template <size_t T> inline void osc_overlay_down(float *dst, const float *src, size_t n) { for (size_t i = 0; i < n; ++i) dst[i] = src[i * T]; }
        inline void downsample_2x(float *dst, const float *src, size_t n)   { osc_overlay_down<2>(dst, src, n); }
        inline void downsample_3x(float *dst, const float *src, size_t n)   { osc_overlay_down<3>(dst, src, n); }
        inline void downsample_4x(float *dst, const float *src, size_t n)   { osc_overlay_down<4>(dst, src, n); }
        inline void downsample_6x(float *dst, const float *src, size_t n)   { osc_overlay_down<6>(dst, src, n); }
        inline void downsample_8x(float *dst, const float *src, size_t n)   { osc_overlay_down<8>(dst, src, n); }

        // every input adds its T x 2a taps onto the pending sums: h_k[t] = float(L(t - a + k / T)), L(x) = sinc(x) sinc(x / a) in double
        template <size_t T, size_t A> inline void osc_overlay_lanczos(float *dst, const float *src, size_t n)
        {
            for (size_t i = 0; i < n; ++i)
                for (size_t t = 0; t < 2 * A; ++t)
                    for (size_t k = 0; k < T; ++k)
                    {
                        double x = double(t) - double(A) + double(k) / double(T), px = M_PI * x;
                        double l = (x == 0.0) ? 1.0 : (sin(px) / px) * (sin(px / double(A)) / (px / double(A)));
                        if (k == 0) l = (t == A) ? 1.0 : 0.0;
                        dst[(i + t) * T + k] += float(l) * src[i];
                    }
        }
        #define OSC_OVERLAY_LANCZOS(T) \
            inline void lanczos_resample_##T##x2(float *d, const float *s, size_t n)     { osc_overlay_lanczos<T, 2>(d, s, n); } \
            inline void lanczos_resample_##T##x3(float *d, const float *s, size_t n)     { osc_overlay_lanczos<T, 3>(d, s, n); } \
            inline void lanczos_resample_##T##x4(float *d, const float *s, size_t n)     { osc_overlay_lanczos<T, 4>(d, s, n); } \
            inline void lanczos_resample_##T##x12bit(float *d, const float *s, size_t n) { osc_overlay_lanczos<T, 4>(d, s, n); } \
            inline void lanczos_resample_##T##x16bit(float *d, const float *s, size_t n) { osc_overlay_lanczos<T, 10>(d, s, n); } \
            inline void lanczos_resample_##T##x24bit(float *d, const float *s, size_t n) { osc_overlay_lanczos<T, 62>(d, s, n); }
        OSC_OVERLAY_LANCZOS(2) OSC_OVERLAY_LANCZOS(3) OSC_OVERLAY_LANCZOS(4) OSC_OVERLAY_LANCZOS(6) OSC_OVERLAY_LANCZOS(8)
    }
}
#endif
'''

# reads the cases, runs the class, writes out[n], the settings words and the periods of every case; with "keys" as its only
# argument it prints the object's size, what the float overload question of :372 answers and what dump() writes
DRIVER = r'''
#define private public
#define protected public
#include <lsp-plug.in/dsp-units/util/Oscillator.h>
#undef private
#undef protected
#include <cmath>
#include <math.h>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
using namespace lsp;
struct keys: public dspu::IStateDumper
{
    std::string seen, closes;
    int depth = 0;
    void note(const char *n) { if (depth == 0) { seen += " "; seen += n; } }
    void begin_object(const char *n, const void *, size_t) override { note(n); ++depth; }
    void begin_object(const void *, size_t) override    { ++depth; }
    void end_object() override                          { --depth; }
    void begin_array(const char *n, const void *, size_t) override { note(n); ++depth; }
    void begin_array(const void *, size_t) override     { ++depth; }
    void end_array() override                           { --depth; }
    void write(const char *n, const void *) override    { note(n); }
    void write(const char *n, bool) override            { note(n); }
    void write(const char *n, unsigned char) override   { note(n); }
    void write(const char *n, signed int) override      { note(n); }
    void write(const char *n, unsigned int) override    { note(n); }
    void write(const char *n, unsigned long) override   { note(n); }
    void write(const char *n, float) override           { note(n); }
    void writev(const char *n, const float *, size_t) override          { note(n); }
    void writev(const char *n, const unsigned int *, size_t) override   { note(n); }
};
static uint32_t fb(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
#ifdef EXACT_FILTERS
extern "C" int mi_dspu_set_exact_iir_default(int on);           // the same program on a class whose filters have a fast mode
#endif
int main(int argc, char **argv)
{
#ifdef EXACT_FILTERS
    mi_dspu_set_exact_iir_default(1);
#endif
    if (argc == 2 && strcmp(argv[1], "keys") == 0)
    {
        dspu::Oscillator o;
        if (!o.init()) return 2;
        keys k;
        o.dump(&k);
        float a2p = 1.0f; uint32_t acc = 3;
        printf("sizeof %zu %zu\nsinsize %zu\noscillator%s\n", sizeof(o), sizeof(dspu::Oversampler), sizeof(sin(a2p * acc)), k.seen.c_str());
        return 0;
    }
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb"), *g = fopen(argv[2], "wb");
    if (!f || !g) return 2;
    uint32_t hdr[2];
    if (fread(hdr, 4, 2, f) != 2) return 3;
    const uint32_t cases = hdr[0], n = hdr[1];
    std::vector<float> src(n), out(n), per;
    for (uint32_t c = 0; c < cases; ++c)
    {
        uint32_t k;
        if (fread(&k, 4, 1, f) != 1) return 3;
        std::vector<double> ops(4 * size_t(k));
        if (fread(ops.data(), 8, ops.size(), f) != ops.size()) return 3;
        if (fread(src.data(), 4, n, f) != n) return 3;
        std::fill(out.begin(), out.end(), 0.0f);
        per.clear();
        dspu::Oscillator o;
        if (!o.init()) return 4;
        size_t at = 0;
        for (uint32_t j = 0; j < k; ++j)
        {
            const int what = int(ops[4 * j]);
            const double a = ops[4 * j + 1], b = ops[4 * j + 2], cc = ops[4 * j + 3];
            const size_t cnt = (what <= 6) ? size_t(a) : 0;
            if (at + cnt > n) return 5;
            switch (what)
            {
                case 0: o.process_overwrite(&out[at], cnt); break;
                case 1: o.process_add(&out[at], &src[at], cnt); break;
                case 2: o.process_add(&out[at], NULL, cnt); break;
                case 3: memcpy(&out[at], &src[at], 4 * cnt); o.process_add(&out[at], &out[at], cnt); break;
                case 4: o.process_mul(&out[at], &src[at], cnt); break;
                case 5: o.process_mul(&out[at], NULL, cnt); break;
                case 6: memcpy(&out[at], &src[at], 4 * cnt); o.process_mul(&out[at], &out[at], cnt); break;
                case 7: o.set_function(dspu::fg_function_t(int(a))); break;
                case 8: o.set_frequency(float(a)); break;
                case 9: o.set_sample_rate(size_t(a)); break;
                case 10: o.set_phase(float(a)); break;
                case 11: o.set_phase_accumulator_bits(uint8_t(a)); break;
                case 12: o.set_dc_offset(float(a)); break;
                case 13: o.set_dc_reference(dspu::dc_reference_t(int(a))); break;
                case 14: o.set_amplitude(float(a)); break;
                case 15: o.set_duty_ratio(float(a)); break;
                case 16: o.set_width(float(a)); break;
                case 17: o.set_trapezoid_ratios(float(a), float(b)); break;
                case 18: o.set_pulsetrain_ratios(float(a), float(b)); break;
                case 19: o.set_parabolic_width(float(a)); break;
                case 20: o.set_squared_sinusoid_inversion(a != 0.0); break;
                case 21: o.set_parabolic_inversion(a != 0.0); break;
                case 22: o.set_oversampler_mode(dspu::over_mode_t(int(a))); break;
                case 23: o.reset_phase_accumulator(); break;
                case 24: o.update_settings(); break;
                case 25:
                {
                    const size_t was = per.size();
                    per.resize(was + size_t(cc));
                    o.get_periods(&per[was], size_t(a), size_t(b), size_t(cc));
                    break;
                }
                default: return 6;
            }
            at += cnt;
        }
        if (at != n) return 7;
        fwrite(out.data(), 4, n, g);
        const uint32_t w[38] = { o.nPhaseAcc, o.nPhaseAccMask, fb(o.fAcc2Phase), o.nFreqCtrlWord, o.nInitPhaseWord, fb(o.fReferencedDC),
            fb(o.sSquaredSinusoid.fAmplitude), fb(o.sSquaredSinusoid.fWaveDC), o.sRectangular.nDutyWord, fb(o.sRectangular.fWaveDC),
            fb(o.sRectangular.fBLPeakAtten), o.sSawtooth.nWidthWord, fb(o.sSawtooth.fCoeffs[0]), fb(o.sSawtooth.fCoeffs[1]),
            fb(o.sSawtooth.fCoeffs[2]), fb(o.sSawtooth.fCoeffs[3]), fb(o.sSawtooth.fBLPeakAtten), o.sTrapezoid.nPoints[0],
            o.sTrapezoid.nPoints[1], o.sTrapezoid.nPoints[2], o.sTrapezoid.nPoints[3], fb(o.sTrapezoid.fCoeffs[0]),
            fb(o.sTrapezoid.fCoeffs[1]), fb(o.sTrapezoid.fCoeffs[2]), fb(o.sTrapezoid.fCoeffs[3]), fb(o.sTrapezoid.fBLPeakAtten),
            o.sPulse.nTrainPoints[0], o.sPulse.nTrainPoints[1], o.sPulse.nTrainPoints[2], fb(o.sPulse.fWaveDC), fb(o.sPulse.fBLPeakAtten),
            fb(o.sParabolic.fAmplitude), o.sParabolic.nWidthWord, fb(o.sParabolic.fWaveDC), fb(o.sParabolic.fBLPeakAtten),
            uint32_t(o.nOversampling), o.nFreqCtrlWord_Over, uint32_t(per.size()) };
        fwrite(w, 4, 38, g);
        if (!per.empty())
            fwrite(per.data(), 4, per.size(), g);
    }
    fclose(f);
    return fclose(g) == 0 ? 0 : 8;
}
'''

FLAGS = ["-std=c++11", "-O2", "-ffp-contract=off", "-msse2", "-mfpmath=sse", "-DLSP_DSP_UNITS_BUILTIN", "-Wall"]
SAN_FLAGS = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
REF_SOURCES = ("util/Oscillator.cpp", "util/Oversampler.cpp", "filters/Filter.cpp", "filters/FilterBank.cpp", "iface/IStateDumper.cpp")


def source_row():
    """What add and mul read: noise with +0, -0, Inf, NaN and subnormals in it."""
    rng = np.random.default_rng(97531)
    s = (rng.standard_normal(N) * 0.5).astype(f32)
    s[::50] = 0.0
    s[25::50] = -0.0
    for at in (3, 301, 777):
        s[at] = np.inf if at % 2 else -np.inf
    s[3] = np.inf
    s[302] = -np.inf
    for at in (11, 500, 1001):
        s[at] = np.nan
    s[40], s[41] = 1e-40, -1e-42
    return s


def pieces(call, what=R.P_OVERWRITE, n=N):
    ops, at = [], 0
    while at < n:
        k = min(call, n - at)
        ops.append((what, k, 0, 0))
        at += k
    return ops


def split(ops_at, call=N, what=R.P_OVERWRITE):
    """Process operations in calls of `call` samples, with ops_at = {sample: [operations]} put between them."""
    ops, at = [], 0
    marks = sorted(ops_at) + [N]
    for m in marks:
        ops += pieces(call, what, m - at)
        at = m
        ops += ops_at.get(m, [])
    return ops


def cases():
    out = []
    base = [(R.SET_SAMPLE_RATE, 48000, 0, 0), (R.SET_FREQUENCY, 1000.5, 0, 0)]
    shaped = base + [(R.SET_AMPLITUDE, 0.8, 0, 0), (R.SET_DC_OFFSET, 0.1, 0, 0), (R.SET_PHASE, 0.3, 0, 0)]

    def add(name, setup, body):
        ops = np.array([tuple(float(v) for v in (list(o) + [0, 0, 0])[:4]) for o in list(setup) + list(body)], np.float64).reshape(-1, 4)
        out.append(dict(name=name, ops=ops))

    i = 0

    def call():
        nonlocal i
        i += 1
        return PIECES[i % len(PIECES)]

    # all fourteen functions, amplitude and DC offset not 1 and 0, a phase; the BL ones at one mode per N and at OM_NONE
    for fn in range(9):
        add("%s shaped" % R.FUNCTIONS[fn], shaped + [(R.SET_FUNCTION, fn)], pieces(call()))
    for fn, times in zip(range(9, 14), (2, 3, 4, 6, 8)):
        add("%s at %dx" % (R.FUNCTIONS[fn], times), shaped + [(R.SET_FUNCTION, fn), (R.SET_OVER_MODE, BL_MODES[times])], pieces(call()))
        add("%s at OM_NONE" % R.FUNCTIONS[fn], shaped + [(R.SET_FUNCTION, fn)], pieces(call()))
    # amplitude 1, DC 0: the sinusoids alone
    for fn in R.SINUSOIDS:
        add("%s plain" % R.FUNCTIONS[fn], base + [(R.SET_FUNCTION, fn)], pieces(call()))
    # both DC references, both inversions
    for fn in (R.FG_SQUARED_SINE, R.FG_SQUARED_COSINE, R.FG_RECTANGULAR, R.FG_PULSETRAIN, R.FG_PARABOLIC):
        extra = [(R.SET_DUTY, 0.3), (R.SET_PULSETRAIN, 0.7, 0.2), (R.SET_PARABOLIC_WIDTH, 0.6)]
        for ref in (R.DC_WAVEDC, R.DC_ZERO):
            add("%s DC reference %d" % (R.FUNCTIONS[fn], ref), shaped + extra + [(R.SET_FUNCTION, fn), (R.SET_DC_REFERENCE, ref)], pieces(call()))
    add("squared sine inverted, DC_ZERO", shaped + [(R.SET_FUNCTION, R.FG_SQUARED_SINE), (R.SET_SQUARED_INVERSION, 1), (R.SET_DC_REFERENCE, R.DC_ZERO)],
        pieces(call()))
    add("squared cosine inverted", shaped + [(R.SET_FUNCTION, R.FG_SQUARED_COSINE), (R.SET_SQUARED_INVERSION, 1)], pieces(call()))
    add("parabolic inverted, DC_ZERO", shaped + [(R.SET_FUNCTION, R.FG_PARABOLIC), (R.SET_PARABOLIC_WIDTH, 0.8), (R.SET_PARABOLIC_INVERSION, 1),
                                                  (R.SET_DC_REFERENCE, R.DC_ZERO)], pieces(call()))
    add("BL parabolic inverted at 2x", shaped + [(R.SET_FUNCTION, R.FG_BL_PARABOLIC), (R.SET_PARABOLIC_WIDTH, 0.8), (R.SET_PARABOLIC_INVERSION, 1),
                                                  (R.SET_OVER_MODE, BL_MODES[2])], pieces(call()))
    # accumulator widths 24 and 8 (the 8-bit one wraps within a few samples: 1000.5 Hz is a word of 5)
    for bits in (24, 8):
        for fn in (R.FG_SINE, R.FG_SQUARED_COSINE, R.FG_RECTANGULAR, R.FG_SAWTOOTH, R.FG_TRAPEZOID, R.FG_PULSETRAIN, R.FG_PARABOLIC):
            extra = [(R.SET_WIDTH, 0.7), (R.SET_PULSETRAIN, 0.4, 0.5), (R.SET_PARABOLIC_WIDTH, 0.5), (R.SET_TRAPEZOID, 0.3, 0.2)]
            freq = [(R.SET_FREQUENCY, 9000.25)] if bits == 8 else []
            add("%s, %d bits" % (R.FUNCTIONS[fn], bits), shaped + extra + freq + [(R.SET_FUNCTION, fn), (R.SET_BITS, bits)], pieces(call()))
    add("BL sawtooth, 24 bits at 3x", shaped + [(R.SET_FUNCTION, R.FG_BL_SAWTOOTH), (R.SET_BITS, 24), (R.SET_WIDTH, 0.5), (R.SET_OVER_MODE, BL_MODES[3])],
        pieces(call()))
    # a word that wraps the 32-bit accumulator every other sample; frequency 0
    for fn in (R.FG_SINE, R.FG_SAWTOOTH, R.FG_TRAPEZOID):
        add("%s wraps 32 bits" % R.FUNCTIONS[fn], shaped + [(R.SET_FREQUENCY, 30000.0), (R.SET_FUNCTION, fn)], pieces(call()))
        add("%s frequency 0" % R.FUNCTIONS[fn], shaped + [(R.SET_FREQUENCY, 0.0), (R.SET_FUNCTION, fn)], pieces(call()))
    # duty, width and ratios at 0, 1 and inside
    for d in (0.0, 1.0, 0.25):
        add("rectangular duty %g" % d, shaped + [(R.SET_FUNCTION, R.FG_RECTANGULAR), (R.SET_DUTY, d)], pieces(call()))
    add("BL rectangular duty 1 at 4x", shaped + [(R.SET_FUNCTION, R.FG_BL_RECTANGULAR), (R.SET_DUTY, 1.0), (R.SET_OVER_MODE, BL_MODES[4])], pieces(call()))
    for w in (0.0, 1.0, 0.3, 0.5):
        add("sawtooth width %g" % w, shaped + [(R.SET_FUNCTION, R.FG_SAWTOOTH), (R.SET_WIDTH, w)], pieces(call()))
    for w in (0.2, 0.9):
        add("BL sawtooth width %g at 2x" % w, shaped + [(R.SET_FUNCTION, R.FG_BL_SAWTOOTH), (R.SET_WIDTH, w), (R.SET_OVER_MODE, BL_MODES[2])], pieces(call()))
    # width 1.0 on 32 bits: the falling branch's coefficients are -Inf and +Inf; a phase of -1e-9 rad is the word `mask`, and with
    # frequency 0 every sample stays there: NaN.  Then a frequency: the rising branch
    add("sawtooth width 1 at phase == mask", base + [(R.SET_FUNCTION, R.FG_SAWTOOTH), (R.SET_WIDTH, 1.0), (R.SET_FREQUENCY, 0.0), (R.SET_PHASE, -1e-9)],
        split({300: [(R.SET_FREQUENCY, 1000.5)]}, 256))
    for r, fa in ((0.0, 0.5), (1.0, 0.0), (0.3, 0.0), (0.0, 1.0), (0.5, 0.5), (0.0, 0.0), (0.1, 0.6)):
        add("trapezoid ratios %g %g" % (r, fa), shaped + [(R.SET_FUNCTION, R.FG_TRAPEZOID), (R.SET_TRAPEZOID, r, fa)], pieces(call()))
    add("BL trapezoid ratios 0.1 0.2 at 8x", shaped + [(R.SET_FUNCTION, R.FG_BL_TRAPEZOID), (R.SET_TRAPEZOID, 0.1, 0.2), (R.SET_OVER_MODE, BL_MODES[8])],
        pieces(call()))
    for p, q in ((0.0, 0.0), (1.0, 1.0), (0.3, 0.6), (0.7, 1.0), (1.0, 0.0)):
        add("pulsetrain ratios %g %g" % (p, q), shaped + [(R.SET_FUNCTION, R.FG_PULSETRAIN), (R.SET_PULSETRAIN, p, q)], pieces(call()))
    add("BL pulsetrain ratios 0.3 0.4 at 3x", shaped + [(R.SET_FUNCTION, R.FG_BL_PULSETRAIN), (R.SET_PULSETRAIN, 0.3, 0.4), (R.SET_OVER_MODE, BL_MODES[3])],
        pieces(call()))
    for w in (0.0, 1.0, 0.6):
        add("parabolic width %g" % w, shaped + [(R.SET_FUNCTION, R.FG_PARABOLIC), (R.SET_PARABOLIC_WIDTH, w)], pieces(call()))
    # changes between pieces: phase, frequency, function, amplitude, bits, the phase reset
    changes = {300: [(R.SET_PHASE, 2.5)], 500: [(R.SET_FREQUENCY, 3333.25)], 700: [(R.SET_FUNCTION, R.FG_TRAPEZOID)], 900: [(R.SET_AMPLITUDE, -1.5)]}
    for fn in (R.FG_SAWTOOTH, R.FG_SINE, R.FG_RECTANGULAR):
        for c in (N, 7, 256):
            add("%s changed on the way, calls of %d" % (R.FUNCTIONS[fn], c), shaped + [(R.SET_FUNCTION, fn)], split(changes, c))
    add("BL sawtooth changed on the way at 4x", shaped + [(R.SET_FUNCTION, R.FG_BL_SAWTOOTH), (R.SET_WIDTH, 0.5), (R.SET_OVER_MODE, BL_MODES[4])],
        split({300: [(R.SET_PHASE, 2.5)], 500: [(R.SET_FREQUENCY, 3333.25)], 900: [(R.SET_AMPLITUDE, -1.5)]}, 256))
    add("phase beyond a turn and negative", shaped + [(R.SET_FUNCTION, R.FG_SAWTOOTH), (R.SET_PHASE, 7.5)],
        split({400: [(R.SET_PHASE, -3.25)], 800: [(R.SET_PHASE, 0.0)]}))
    add("reset_phase_accumulator on the way", shaped + [(R.SET_FUNCTION, R.FG_SAWTOOTH)], split({333: [(R.RESET_PHASE,)], 801: [(R.RESET_PHASE,), (R.SET_PHASE, 1.0)]}, 256))
    add("bits changed on the way", shaped + [(R.SET_FUNCTION, R.FG_PARABOLIC), (R.SET_PARABOLIC_WIDTH, 0.7)],
        split({400: [(R.SET_BITS, 12)], 800: [(R.SET_BITS, 32)]}, 256))
    add("sample rate changed on the way", shaped + [(R.SET_FUNCTION, R.FG_COSINE)], split({600: [(R.SET_SAMPLE_RATE, 44100)]}))
    add("oversampler mode changed on the way", shaped + [(R.SET_FUNCTION, R.FG_BL_RECTANGULAR), (R.SET_OVER_MODE, BL_MODES[2])],
        split({600: [(R.SET_OVER_MODE, BL_MODES[6])]}, 256))
    # add and mul: with a source, without, in place
    for fn in (R.FG_SAWTOOTH, R.FG_SINE, R.FG_BL_PULSETRAIN):
        setup = shaped + [(R.SET_FUNCTION, fn), (R.SET_PULSETRAIN, 0.3, 0.4), (R.SET_OVER_MODE, BL_MODES[2] if fn >= 9 else 0)]
        for what, label in ((R.P_ADD, "add"), (R.P_ADD_NULL, "add without a source"), (R.P_ADD_INPLACE, "add in place"), (R.P_MUL, "mul"),
                            (R.P_MUL_NULL, "mul without a source"), (R.P_MUL_INPLACE, "mul in place")):
            add("%s %s" % (R.FUNCTIONS[fn], label), setup, pieces(call(), what))
    add("rectangular amplitude 0 mul without a source", base + [(R.SET_FUNCTION, R.FG_RECTANGULAR), (R.SET_AMPLITUDE, 0.0), (R.SET_DC_OFFSET, -2.0)],
        pieces(256, R.P_MUL_NULL))
    add("add, mul and overwrite mixed", shaped + [(R.SET_FUNCTION, R.FG_TRAPEZOID)],
        [(R.P_ADD, 100), (R.P_MUL, 200), (R.P_OVERWRITE, 300), (R.P_MUL_INPLACE, 250), (R.P_ADD_NULL, 250)])
    # get_periods with skipped periods that fit one buffer: one fill (:649-660), every pick inside what it wrote, no refill.  (A call
    # that refills -- every call without skipped periods -- reads in front of vSynthBuffer: undefined, not recorded.)  The streaming
    # phase and the streaming oversampler go on behind it
    for fn, mode in ((R.FG_SAWTOOTH, 0), (R.FG_TRAPEZOID, 0), (R.FG_BL_SAWTOOTH, BL_MODES[2]), (R.FG_BL_PULSETRAIN, BL_MODES[4])):
        setup = shaped + [(R.SET_FUNCTION, fn), (R.SET_WIDTH, 0.5), (R.SET_PULSETRAIN, 0.3, 0.4), (R.SET_OVER_MODE, mode)]
        add("%s get_periods behind skipped periods" % R.FUNCTIONS[fn], setup,
            [(R.P_OVERWRITE, 400), (R.GET_PERIODS, 3, 5, 64), (R.P_OVERWRITE, 300), (R.GET_PERIODS, 2, 4, 50), (R.GET_PERIODS, 1, 1, 17), (R.P_OVERWRITE, 400)])
    return out


def single_fill(duration, periods, skip, samples):
    """The picks of get_periods(periods, skip, samples) all lie inside the one fill of :649-660."""
    out, sk = f32(f32(duration) * f32(periods)), f32(f32(duration) * f32(skip))
    step = f32(out / f32(samples))
    to_do = R.limited(f32(f32(out + sk) + step))
    first = f32(f32(to_do) + f32(sk - f32(to_do)))
    return sk > 0 and to_do < R.PROCESS_BUF_LIMIT_SIZE and 0 <= first and float(first) + float(step) * samples < to_do


def write_cases(path, cs, src):
    with open(path, "wb") as f:
        f.write(np.array([len(cs), N], np.uint32).tobytes())
        for c in cs:
            f.write(np.array([len(c["ops"])], np.uint32).tobytes() + c["ops"].tobytes() + src.tobytes())


def read_results(path, cs):
    got = []
    with open(path, "rb") as f:
        for c in cs:
            out = np.frombuffer(f.read(4 * N), f32)
            w = np.frombuffer(f.read(4 * 38), np.uint32)
            per = np.frombuffer(f.read(4 * int(w[37])), f32)
            got.append(dict(out=out, words=w[:37].copy(), periods=per))
        assert f.read(1) == b""
    return got


def run(exe, cs, src, cwd):
    a, b = os.path.join(cwd, "cases.bin"), os.path.join(cwd, "results.bin")
    write_cases(a, cs, src)
    subprocess.run([exe, a, b], check=True, timeout=900)
    return read_results(b, cs)


def run_reference(reference):
    cs, src = cases(), source_row()
    with tempfile.TemporaryDirectory() as d:
        for rel, text in (("lsp-plug.in/dsp-units/version.h", OVERLAY_VERSION), ("lsp-plug.in/common/alloc.h", OVERLAY_ALLOC),
                          ("lsp-plug.in/dsp/dsp.h", OVERLAY_DSP), ("lsp-plug.in/common/types.h", OVERLAY_TYPES)):
            os.makedirs(os.path.dirname(os.path.join(d, "overlay", rel)), exist_ok=True)
            with open(os.path.join(d, "overlay", rel), "w") as f:
                f.write(text)
        with open(os.path.join(d, "driver.cpp"), "w") as f:
            f.write(DRIVER)
        srcs = [os.path.join(d, "driver.cpp")] + [os.path.join(reference, "src", "main", n) for n in REF_SOURCES]
        inc = ["-I" + os.path.join(d, "overlay"), "-I" + os.path.join(ROOT, "oracle", "ref_shim"), "-I" + os.path.join(reference, "include")]
        for exe, extra in (("ref_san", SAN_FLAGS), ("ref", [])):
            subprocess.check_call(["g++"] + FLAGS + extra + inc + ["-o", os.path.join(d, exe)] + srcs + ["-lm"])
        san = run(os.path.join(d, "ref_san"), cs, src, d)            # stand-alone, before anything is recorded
        got = run(os.path.join(d, "ref"), cs, src, d)
        keys = {l.split()[0]: l.split()[1:] for l in subprocess.check_output([os.path.join(d, "ref_san"), "keys"]).decode().splitlines()}
    for c, a, b in zip(cs, san, got):
        for k in a:
            # the two builds may round a NaN's sign differently; everything else is the same bits
            assert R.same(a[k].view(f32), b[k].view(f32)) if a[k].dtype == f32 else np.array_equal(a[k], b[k]), (c["name"], k)
    assert keys["sinsize"] == ["4"], keys["sinsize"]                # sin(fAcc2Phase * nPhaseAcc) is the float overload
    names = {"util/Oscillator.h": public_names(os.path.join(reference, "include", "lsp-plug.in", "dsp-units", "util", "Oscillator.h"), "Oscillator")}
    return cs, src, got, keys, names


def oversampler():
    from oversampler_ref import OversamplerRef
    return OversamplerRef(1, None)


def check_branches(cs, src, got):
    """What the cases are there for has happened in them, and no trapezoid phase satisfies two branches."""
    by = {c["name"]: (c, g) for c, g in zip(cs, got)}
    for c in cs:
        _, _, osc, _ = R.run_case(dict(ops=c["ops"], src=src), oversampler=oversampler)
        assert osc.double_writes == 0, "%s: %d phases satisfy two trapezoid branches" % (c["name"], osc.double_writes)
    c, g = by["sawtooth width 1 at phase == mask"]
    assert np.isnan(g["out"][:301]).all() and np.isfinite(g["out"][301:]).all()     # the sample at 300 is still at the mask
    c, g = by["sine wraps 32 bits"]
    assert int(g["words"][3]) * 2 > 1 << 32
    c, g = by["sawtooth, 8 bits"]
    assert g["words"][1] == 255 and g["words"][3] * 10 > 256
    for c, g in zip(cs, got):                               # every recorded get_periods call is a defined one
        for op in c["ops"]:
            if int(op[0]) == R.GET_PERIODS:
                assert single_fill(48000.0 / 1000.5, int(op[1]), int(op[2]), int(op[3])), c["name"]
    c, g = by["BL sawtooth get_periods behind skipped periods"]
    assert g["periods"].size == 131 and np.count_nonzero(g["periods"] != g["periods"][0]) > 100
    c, g = by["rectangular amplitude 0 mul without a source"]
    assert np.signbit(g["out"]).all() and (g["out"] == 0).all()
    return len(cs)


def build(reference):
    cs, src, got, keys, names = run_reference(reference)
    check_branches(cs, src, got)
    arrs = {"src": src, "names": np.array([c["name"] for c in cs]), "ops_n": np.array([len(c["ops"]) for c in cs], np.uint32),
            "ops": np.concatenate([c["ops"] for c in cs]), "out": np.array([g["out"] for g in got]),
            "words": np.array([g["words"] for g in got]), "periods_n": np.array([g["periods"].size for g in got], np.uint32),
            "periods": np.concatenate([g["periods"] for g in got])}
    return npz_bytes(arrs), keys, names


def load(path=OUT):
    """The stored file as a list of cases: dicts of name, ops [k, 4], src [N], out [N], words [37], periods."""
    z = np.load(path)
    off = np.concatenate([[0], np.cumsum(z["ops_n"].astype(np.int64))])
    poff = np.concatenate([[0], np.cumsum(z["periods_n"].astype(np.int64))])
    return [dict(name=str(z["names"][i]), ops=z["ops"][off[i]:off[i + 1]], src=z["src"], out=z["out"][i], words=z["words"][i],
                 periods=z["periods"][poff[i]:poff[i + 1]]) for i in range(len(z["names"]))]


if __name__ == "__main__":
    data, keys, names = build(sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(ROOT), "reference"))
    assert len(data) < (1 << 20), len(data)
    with open(OUT, "wb") as f:
        f.write(data)
    with open(os.path.join(HERE, "oscillator_dump_keys.json"), "w") as f:
        json.dump({"keys": keys["oscillator"], "sizeof": int(keys["sizeof"][0]), "closes": []}, f, indent=1)
        f.write("\n")
    with open(os.path.join(HERE, "oscillator_public_names.json"), "w") as f:
        json.dump(names, f, indent=1)
        f.write("\n")
    print("%d cases, %d bytes" % (len(load()), len(data)))
