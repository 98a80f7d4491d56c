"""Writes tests/golden/noise_generator_ref_vectors.npz: what the reference's own SpectralTilt and NoiseGenerator classes compute on a
list of cases.  Data only: operation lists, one source row, the reference's output, the state words and the designed sections each
case ends with, one frequency chart per case.  Run where the reference tree exists:

    python tests/golden/make_noise_generator_vectors.py [reference tree]

filters/SpectralTilt.cpp, filters/FilterBank.cpp, noise/Generator.cpp, noise/Velvet.cpp, noise/LCG.cpp, noise/MLS.cpp,
util/Randomizer.cpp and iface/IStateDumper.cpp are compiled unmodified into a temporary directory (the flags of
make_noise_vectors.py) against oracle/ref_shim, the overlays of make_noise_vectors.py and a stand-in for the lsp-dsp-lib calls they
make: one float operation per sample for add2 / add3 / mul2 / mul3 / mul_k2 / add_k2 / copy / fill / fill_zero / pcomplex_fill_ri,
the formulas of Filter::bilinear_transform in float for bilinear_transform_x1, and for biquad_process_x1 / x2 / x4 / x8 the
arithmetic of oracle/biquad_oracle.c: the sections of a group one after the other, y = b0 x + d0, d0 = d1 + (b1 x + a1 y),
d1 = b2 x + a2 y.  The program -- a stand-alone one with its own main -- is built a first time with -fsanitize=address,undefined
and run over every case before anything is recorded.

tests/noise_generator_ref.py names the operations; a process operation fills the next samples of out, and only the filled part of
out is stored."""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)
import noise_ref as R  # noqa: E402
import velvet_ref as V  # noqa: E402
import noise_generator_ref as G  # noqa: E402
import make_noise_vectors as noise  # noqa: E402
from make_bypass_crossfade_vectors import npz_bytes, public_names  # noqa: E402

OUT = os.path.join(HERE, "noise_generator_ref_vectors.npz")
LAYOUT = os.path.join(ROOT, "tests", "cpp", "noise_generator_layout.cpp")      # sizeof, offsetof and dump keys: the same program for both trees
HEADERS = {"filters/SpectralTilt.h": "SpectralTilt", "noise/Generator.h": "NoiseGenerator"}
f32, u32, u64 = np.float32, np.uint32, np.uint64
N = noise.N
F = G.CHART_F.size

OVERLAY_DSP = r'''
#ifndef NG_OVERLAY_DSP_H_
#define NG_OVERLAY_DSP_H_
#include <lsp-plug.in/common/types.h>
#include <string.h>
#define LSP_DSP_BIQUAD_ALIGN    0x40
#define LSP_DSP_BIQUAD_D_ITEMS  16
namespace lsp
{
    // lsp-common-lib's, as SpectralTilt.cpp and FilterBank.cpp use them
    template <class T> inline void swap(T &a, T &b) { T t = a; a = b; b = t; }
    inline size_t align_size(size_t size, size_t align) { const size_t off = size % align; return off ? size + align - off : size; }

    namespace dsp
    {
        struct biquad_x1_t { float b0, b1, b2, a1, a2, p0, p1, p2; };
        struct biquad_x2_t { float b0[2], b1[2], b2[2], a1[2], a2[2], p[2]; };
        struct biquad_x4_t { float b0[4], b1[4], b2[4], a1[4], a2[4]; };
        struct biquad_x8_t { float b0[8], b1[8], b2[8], a1[8], a2[8]; };
        struct biquad_t
        {
            float d[LSP_DSP_BIQUAD_D_ITEMS];
            union { biquad_x1_t x1; biquad_x2_t x2; biquad_x4_t x4; biquad_x8_t x8; };
            float pad[8];
        } __attribute__((aligned(LSP_DSP_BIQUAD_ALIGN)));
        struct f_cascade_t { float t[4], b[4]; };

        inline void copy(float *dst, const float *src, size_t n)    { if (dst != src) memmove(dst, src, n * sizeof(float)); }
        inline void fill(float *dst, float v, size_t n)             { for (size_t i = 0; i < n; ++i) dst[i] = v; }
        inline void fill_zero(float *dst, size_t n)                 { for (size_t i = 0; i < n; ++i) dst[i] = 0.0f; }
        inline void pcomplex_fill_ri(float *dst, float re, float im, size_t n) { for (size_t i = 0; i < n; ++i) dst[2 * i] = re, dst[2 * i + 1] = im; }
        inline void mul_k2(float *dst, float k, size_t n)           { for (size_t i = 0; i < n; ++i) dst[i] = dst[i] * k; }
        inline void add_k2(float *dst, float k, size_t n)           { for (size_t i = 0; i < n; ++i) dst[i] = dst[i] + k; }
        inline void add2(float *dst, const float *src, size_t n)    { for (size_t i = 0; i < n; ++i) dst[i] = dst[i] + src[i]; }
        inline void mul2(float *dst, const float *src, size_t n)    { for (size_t i = 0; i < n; ++i) dst[i] = dst[i] * src[i]; }
        inline void add3(float *dst, const float *a, const float *b, size_t n) { for (size_t i = 0; i < n; ++i) dst[i] = a[i] + b[i]; }
        inline void mul3(float *dst, const float *a, const float *b, size_t n) { for (size_t i = 0; i < n; ++i) dst[i] = a[i] * b[i]; }

        // the formulas of Filter::bilinear_transform (Filter.cpp:2225-2262) in float
        inline void bilinear_transform_x1(biquad_x1_t *bf, const f_cascade_t *bc, float kf, size_t count)
        {
            const float kf2 = kf * kf;
            for (size_t i = 0; i < count; ++i, ++bf, ++bc)
            {
                const float T0 = bc->t[0], T1 = bc->t[1] * kf, T2 = bc->t[2] * kf2;
                const float B0 = bc->b[0], B1 = bc->b[1] * kf, B2 = bc->b[2] * kf2;
                const float N = 1.0f / (B0 + B1 + B2);
                bf->b0 = (T0 + T1 + T2) * N;
                bf->b1 = 2.0f * (T0 - T2) * N;
                bf->b2 = (T0 - T1 + T2) * N;
                bf->a1 = 2.0f * (B2 - B0) * N;
                bf->a2 = (B1 - B2 - B0) * N;
                bf->p0 = bf->p1 = bf->p2 = 0.0f;
            }
        }

        // one section over a row, oracle/biquad_oracle.c; d0 and d1 of section k of a group are d[k] and d[8 + k]
        inline void ng_section(float *dst, const float *src, size_t n, float b0, float b1, float b2, float a1, float a2, float *pd0, float *pd1)
        {
            float d0 = *pd0, d1 = *pd1;
            for (size_t i = 0; i < n; ++i)
            {
                const float x = src[i];
                const float y = b0 * x + d0;
                const float p1 = b1 * x + a1 * y;
                const float p2 = b2 * x + a2 * y;
                d0 = d1 + p1;
                d1 = p2;
                dst[i] = y;
            }
            *pd0 = d0, *pd1 = d1;
        }
        inline void biquad_process_x1(float *dst, const float *src, size_t n, biquad_t *f)
        {
            ng_section(dst, src, n, f->x1.b0, f->x1.b1, f->x1.b2, f->x1.a1, f->x1.a2, &f->d[0], &f->d[8]);
        }
        #define NG_GROUP(name, member, lanes) \
            inline void name(float *dst, const float *src, size_t n, biquad_t *f) \
            { \
                for (size_t k = 0; k < lanes; ++k) \
                    ng_section(dst, k ? dst : src, n, f->member.b0[k], f->member.b1[k], f->member.b2[k], f->member.a1[k], f->member.a2[k], &f->d[k], &f->d[8 + k]); \
            }
        NG_GROUP(biquad_process_x2, x2, 2)
        NG_GROUP(biquad_process_x4, x4, 4)
        NG_GROUP(biquad_process_x8, x8, 8)
        #undef NG_GROUP
    }
}
#endif
'''

OVERLAY_TRANSFORM = r'''
#include <lsp-plug.in/dsp/dsp.h>
'''

# reads the cases and runs the classes; per case it writes the samples filled, out[n], the words, the number of sections and
# sections[64][5], and chart[2 F]
DRIVER = r'''
#define private public
#define protected public
#include <lsp-plug.in/dsp-units/noise/Generator.h>
#undef private
#undef protected
#include <cstdio>
#include <cstring>
#include <vector>
using namespace lsp;
static uint64_t fbits(float v) { uint32_t w; memcpy(&w, &v, 4); return w; }
static void tilt_words(uint64_t *w, const dspu::SpectralTilt &t)
{
    const uint64_t v[11] = { t.nOrder, uint64_t(t.enSlopeUnit), uint64_t(t.enNorm), fbits(t.fSlopeVal), fbits(t.fSlopeNepNep), fbits(t.fLowerFrequency),
                             fbits(t.fUpperFrequency), t.nSampleRate, t.bBypass, t.bSync, t.sFilter.size() };
    memcpy(w, v, sizeof(v));
}
int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb"), *g = fopen(argv[2], "wb");
    if (!f || !g) return 2;
    uint32_t hdr[3];
    if (fread(hdr, 4, 3, f) != 3) return 3;
    const uint32_t cases = hdr[0], n = hdr[1], nf = hdr[2];
    std::vector<float> src(n), out(n), dst0(n), freqs(nf), chart(2 * nf);
    if (fread(freqs.data(), 4, nf, f) != nf) return 3;
    for (uint32_t c = 0; c < cases; ++c)
    {
        uint32_t k;
        if (fread(&k, 4, 1, f) != 1) return 3;
        std::vector<double> ops(4 * size_t(k));
        if (fread(ops.data(), 8, ops.size(), f) != ops.size()) return 3;
        if (fread(src.data(), 4, n, f) != n) return 3;
        for (uint32_t i = 0; i < n; ++i)
            dst0[i] = src[n - 1 - i] * 0.75f;
        std::fill(out.begin(), out.end(), 0.0f);
        std::fill(chart.begin(), chart.end(), 0.0f);
        dspu::SpectralTilt t;
        dspu::NoiseGenerator ng;
        t.init();
        const bool tilt_case = int(ops[0]) < 30;
        uint32_t vs = 0, vb = 0; uint64_t vm = 0;
        size_t at = 0;
        for (uint32_t j = 0; j < k; ++j)
        {
            const int what = int(ops[4 * j]);
            const double a = ops[4 * j + 1], b = ops[4 * j + 2], d = ops[4 * j + 3];
            const bool runs = what <= 8 || (what >= 30 && what <= 36);
            const size_t cnt = runs ? size_t(a) : 0;
            if (at + cnt > n) return 5;
            if (what >= 30 && what <= 36 && (ng.sLCG.sRand.nBufID > 3 || ng.sVelvetNoise.sRandomizer.nBufID > 3)) return 9;
            float *o = out.data() + at;
            const float *s = src.data() + at;
            switch (what)
            {
                case 0: t.process_overwrite(o, s, cnt); break;
                case 1: memcpy(o, dst0.data() + at, 4 * cnt); t.process_add(o, s, cnt); break;
                case 2: memcpy(o, dst0.data() + at, 4 * cnt); t.process_mul(o, s, cnt); break;
                case 3: memcpy(o, s, 4 * cnt); t.process_overwrite(o, o, cnt); break;
                case 4: memcpy(o, s, 4 * cnt); t.process_add(o, o, cnt); break;
                case 5: memcpy(o, s, 4 * cnt); t.process_mul(o, o, cnt); break;
                case 6: memcpy(o, dst0.data() + at, 4 * cnt); t.process_overwrite(o, NULL, cnt); break;
                case 7: memcpy(o, dst0.data() + at, 4 * cnt); t.process_add(o, NULL, cnt); break;
                case 8: memcpy(o, dst0.data() + at, 4 * cnt); t.process_mul(o, NULL, cnt); break;
                case 10: t.set_order(size_t(a)); break;
                case 11: t.set_slope(float(a), dspu::stlt_slope_unit_t(int(b))); break;
                case 12: t.set_norm(dspu::stlt_norm_t(int(a))); break;
                case 13: t.set_lower_frequency(float(a)); break;
                case 14: t.set_upper_frequency(float(a)); break;
                case 15: t.set_frequency_range(float(a), float(b)); break;
                case 16: t.set_sample_rate(size_t(a)); break;
                case 17: if (a != 0) t.freq_chart(chart.data(), freqs.data(), nf);
                         else { std::vector<float> re(nf), im(nf); t.freq_chart(re.data(), im.data(), freqs.data(), nf);
                                for (uint32_t i = 0; i < nf; ++i) chart[2 * i] = re[i], chart[2 * i + 1] = im[i]; }
                         break;
                case 30: ng.process_overwrite(o, cnt); break;
                case 31: ng.process_add(o, s, cnt); break;
                case 32: memcpy(o, s, 4 * cnt); ng.process_add(o, o, cnt); break;
                case 33: ng.process_mul(o, s, cnt); break;
                case 34: memcpy(o, s, 4 * cnt); ng.process_mul(o, o, cnt); break;
                case 35: memcpy(o, s, 4 * cnt); ng.process_add(o, NULL, cnt); break;
                case 36: memcpy(o, s, 4 * cnt); ng.process_mul(o, NULL, cnt); break;
                case 40: vs = uint32_t(a), vb = uint32_t(b), vm = uint64_t(d); break;
                case 41: ng.init(uint8_t(a), uint64_t(b), uint32_t(d), vs, uint8_t(vb), vm); break;
                case 42: ng.set_sample_rate(size_t(a)); break;
                case 43: ng.set_mls_n_bits(uint8_t(a)); break;
                case 44: ng.set_mls_seed(uint64_t(a)); break;
                case 45: ng.set_lcg_distribution(dspu::lcg_dist_t(int(a))); break;
                case 46: ng.set_velvet_type(dspu::vn_velvet_type_t(int(a))); break;
                case 47: ng.set_velvet_window_width(float(a)); break;
                case 48: ng.set_velvet_arn_delta(float(a)); break;
                case 49: ng.set_velvet_crush(a != 0); break;
                case 50: ng.set_velvet_crushing_probability(float(a)); break;
                case 51: ng.set_generator(dspu::ng_generator_t(int(a))); break;
                case 52: ng.set_noise_color(dspu::ng_color_t(int(a))); break;
                case 53: ng.set_coloring_order(size_t(a)); break;
                case 54: ng.set_color_slope(float(a), dspu::stlt_slope_unit_t(int(b))); break;
                case 55: ng.set_amplitude(float(a)); break;
                case 56: ng.set_offset(float(a)); break;
                case 57: if (a != 0) ng.freq_chart(chart.data(), freqs.data(), nf);
                         else { std::vector<float> re(nf), im(nf); ng.freq_chart(re.data(), im.data(), freqs.data(), nf);
                                for (uint32_t i = 0; i < nf; ++i) chart[2 * i] = re[i], chart[2 * i + 1] = im[i]; }
                         break;
                default: return 6;
            }
            at += cnt;
        }
        uint64_t w[64] = { 0 };
        if (!tilt_case)
        {
            const dspu::Randomizer &r = ng.sLCG.sRand;
            for (int i = 0; i < 4; ++i)
                w[i] = r.vRandom[i].vLast, w[4 + i] = r.vRandom[i].vMul1, w[8 + i] = r.vRandom[i].vMul2, w[12 + i] = r.vRandom[i].vAdd;
            w[16] = r.nBufID;
            const dspu::MLS &m = ng.sMLS;
            const uint64_t mw[8] = { m.nBits, m.nFeedbackBit, m.nFeedbackMask, m.nActiveMask, m.nTapsMask, m.nOutputMask, m.nState, m.bSync };
            memcpy(w + 17, mw, sizeof(mw));
            const dspu::Randomizer &vr = ng.sVelvetNoise.sRandomizer;
            for (int i = 0; i < 4; ++i)
                w[25 + i] = vr.vRandom[i].vLast, w[29 + i] = vr.vRandom[i].vMul1, w[33 + i] = vr.vRandom[i].vMul2, w[37 + i] = vr.vRandom[i].vAdd;
            w[41] = vr.nBufID;
            const dspu::MLS &vm2 = ng.sVelvetNoise.sMLS;
            const uint64_t vw[8] = { vm2.nBits, vm2.nFeedbackBit, vm2.nFeedbackMask, vm2.nActiveMask, vm2.nTapsMask, vm2.nOutputMask, vm2.nState, vm2.bSync };
            memcpy(w + 42, vw, sizeof(vw));
            w[61] = ng.nUpdate;
        }
        dspu::SpectralTilt &tt = tilt_case ? t : ng.sColorFilter;
        tilt_words(w + 50, tt);
        const uint32_t filled = uint32_t(at), ns = uint32_t(tt.sFilter.size());
        float sec[64 * 5] = { 0 };
        for (uint32_t i = 0; i < ns && i < 64; ++i)
        {
            const dsp::biquad_x1_t *q = tt.sFilter.chain(i);
            const float v[5] = { q->b0, q->b1, q->b2, q->a1, q->a2 };
            memcpy(sec + 5 * i, v, sizeof(v));
        }
        fwrite(&filled, 4, 1, g);
        fwrite(out.data(), 4, n, g);
        fwrite(w, 8, 64, g);
        fwrite(&ns, 4, 1, g);
        fwrite(sec, 4, 64 * 5, g);
        fwrite(chart.data(), 4, 2 * nf, g);
    }
    fclose(f);
    return fclose(g) == 0 ? 0 : 8;
}
'''

FLAGS = noise.FLAGS
SAN_FLAGS = noise.SAN_FLAGS
REF_SOURCES = ("filters/SpectralTilt.cpp", "filters/FilterBank.cpp", "noise/Generator.cpp", "noise/Velvet.cpp", "noise/LCG.cpp", "noise/MLS.cpp",
               "util/Randomizer.cpp", "iface/IStateDumper.cpp")
OVERLAYS = (("lsp-plug.in/dsp-units/version.h", noise.OVERLAY_VERSION), ("lsp-plug.in/common/types.h", noise.OVERLAY_TYPES),
            ("lsp-plug.in/runtime/system.h", noise.OVERLAY_SYSTEM), ("lsp-plug.in/dsp/dsp.h", OVERLAY_DSP),
            ("lsp-plug.in/dsp/common/filters/transform.h", OVERLAY_TRANSFORM))

source_row = noise.source_row


def finite_row():
    """The source row of the tilt's cases: a filter never recovers from an Inf or a NaN, so they are taken out; zeros of both signs and
    subnormals stay."""
    s = source_row()
    s[np.isnan(s)] = f32(0.125)
    return np.clip(s, f32(-1.5), f32(1.5))
COUNTS = (1, 255, 256, 257, 1100)


def as_ops(ops):
    return np.array([tuple(float(v) for v in (list(o) + [0, 0, 0])[:4]) for o in ops], np.float64).reshape(-1, 4)


def tilt(order=8, slope=-0.5, unit=G.NEPER, norm=None, rate=48000, lower=None, upper=None):
    ops = [(G.T_RATE, rate), (G.T_ORDER, order), (G.T_SLOPE, slope, unit)]
    if norm is not None:
        ops.append((G.T_NORM, norm))
    if lower is not None:
        ops.append((G.T_LOWER, lower))
    if upper is not None:
        ops.append((G.T_UPPER, upper))
    return ops


def gen(generator=G.GEN_LCG, color=G.WHITE, rate=48000, order=None, seed=1, dist=None):
    ops = [(G.G_INIT_VELVET, 0x4000 + seed, 23, 0x2F), (G.G_INIT, 17 + seed % 5, 0x1D + seed, 0x1234 + 77 * seed), (G.G_RATE, rate), (G.G_GEN, generator), (G.G_COLOR, color),
           (G.G_VWIDTH, 0.0005)]                            # windows of 24 samples at 48 kHz
    if order is not None:
        ops.append((G.G_ORDER, order))
    if dist is not None:
        ops.append((G.G_DIST, dist))
    return ops


def cases():
    out = []

    def add(name, ops):
        out.append(dict(name=name, ops=as_ops(ops), finite=int(ops[0][0]) < G.G_OVER and "non-finite" not in name))

    # ---- the tilt alone
    add("tilt with a non-finite source", tilt(order=4) + [(G.T_OVER, 100), (G.T_ADD, 100)])
    for order in (0, 1, 2, 7, 50, 128, 200):
        add("tilt order %d" % order, tilt(order=order) + [(G.T_OVER, 600), (G.T_CHART, 0), (G.T_ADD, 500)])
    for slope, unit in ((0.5, G.NEPER), (-0.5, G.NEPER), (1.0, G.NEPER), (-1.0, G.NEPER), (0.0, G.NEPER), (-3.0, G.DB_OCT), (10.0, G.DB_DEC), (-0.5, G.UNIT_NONE)):
        add("tilt slope %g unit %d" % (slope, unit), tilt(order=10, slope=slope, unit=unit) + [(G.T_OVER, 400), (G.T_MUL, 300), (G.T_CHART, 1), (G.T_ADD_IN, 400)])
    for rate in (44100, 48000, 30000):
        for norm in range(7):
            add("tilt norm %d at %d Hz" % (norm, rate), tilt(order=6, slope=(-0.5, 0.75)[norm % 2], norm=norm, rate=rate) + [(G.T_OVER, 300), (G.T_CHART, norm % 2)])
        add("tilt auto norm, slope up, at %d Hz" % rate, tilt(order=6, slope=0.5, norm=G.NORM_AUTO, rate=rate) + [(G.T_OVER, 300)])
        add("tilt auto norm, slope down, at %d Hz" % rate, tilt(order=6, slope=-0.5, norm=G.NORM_AUTO, rate=rate) + [(G.T_OVER, 300)])
    add("tilt auto norm at 30 Hz: the DC and Nyquist fallbacks", tilt(order=4, slope=-0.5, rate=30, lower=1.0, upper=10.0) + [(G.T_OVER, 200), (G.T_SLOPE, 0.5, G.NEPER), (G.T_OVER, 200)])
    # the range quirks: set_frequency_range swaps the wrong way round, so either way lower >= upper and update_settings() takes the defaults; a frequency at or above Nyquist; lower >= upper
    add("tilt range the right way round", tilt() + [(G.T_RANGE, 20.0, 18000.0), (G.T_OVER, 300), (G.T_CHART, 0)])
    add("tilt range given backwards", tilt() + [(G.T_RANGE, 18000.0, 20.0), (G.T_OVER, 300), (G.T_CHART, 0)])
    add("tilt range equal to the members", tilt(lower=18000.0, upper=20.0) + [(G.T_OVER, 100), (G.T_RANGE, 20.0, 18000.0), (G.T_OVER, 200)])
    add("tilt upper at Nyquist", tilt(upper=24000.0) + [(G.T_OVER, 300)])
    add("tilt lower above Nyquist", tilt(lower=30000.0, rate=44100) + [(G.T_OVER, 300)])
    add("tilt lower above upper", tilt(lower=5000.0, upper=100.0) + [(G.T_OVER, 300)])
    add("tilt as constructed", [(G.T_OVER, 300), (G.T_CHART, 1)])
    # the operations with NULL, bypassed and in place
    for name, pre in (("filtering", tilt(order=4)), ("bypassed", tilt(order=4, slope=0.0))):
        add("tilt %s: every operation" % name, pre + [(w, 120) for w in G.T_PROCESS] + [(G.T_CHART, 0)])
    add("tilt counts", tilt(order=12) + [(G.T_ADD, 1), (G.T_MUL, 255), (G.T_ADD, 256), (G.T_MUL_IN, 257), (G.T_OVER_IN, 331)])
    add("tilt add of 1100", tilt(order=50) + [(G.T_ADD, N)])
    add("tilt mul of 1100 in place", tilt(order=128, slope=1.0) + [(G.T_MUL_IN, N)])
    # a new design in mid-stream clears the memory; a setter that changes nothing does not; bypass keeps sections and memory
    add("tilt re-design in mid-stream", tilt(order=8) + [(G.T_OVER, 300), (G.T_ORDER, 10), (G.T_OVER, 300), (G.T_ORDER, 10), (G.T_OVER, 200), (G.T_NORM, G.NORM_AUTO), (G.T_OVER, 300)])
    add("tilt bypass keeps the stale cascade", tilt(order=8) + [(G.T_OVER, 300), (G.T_SLOPE, 0.0, G.NEPER), (G.T_OVER, 200), (G.T_CHART, 0), (G.T_ADD, 200)])
    add("tilt bypass and back", tilt(order=8) + [(G.T_OVER, 300), (G.T_SLOPE, -0.5, G.UNIT_NONE), (G.T_OVER, 200), (G.T_SLOPE, -0.5, G.NEPER), (G.T_OVER, 300), (G.T_CHART, 1)])
    add("tilt chart before any call", tilt(order=50, slope=-0.5) + [(G.T_CHART, 0)])
    # ---- the generator: every generator x every colour
    k = 0
    for g in (G.GEN_MLS, G.GEN_LCG, G.GEN_VELVET):
        for color in range(6):
            k += 1
            pre = gen(g, color, seed=k, order=(None, 8, 50, 2)[k % 4], dist=(None, R.LCG_TRIANGULAR)[k % 2]) + ([(G.G_SLOPE, -3.0, G.DB_OCT)] if color == G.ARBITRARY else [])
            add("generator %d colour %d" % (g, color), pre + [(G.G_OVER, 500), (G.G_CHART, k % 2), (G.G_ADD, 300), (G.G_MUL_IN, 300)])
    # counts for each operation, Velvet and LCG, pink
    for g in (G.GEN_LCG, G.GEN_VELVET, G.GEN_MLS):
        for what in (G.G_OVER, G.G_ADD, G.G_MUL, G.G_ADD_IN, G.G_ADD_NULL):
            k += 1
            add("generator %d op %d counts" % (g, what), gen(g, (G.PINK, G.WHITE)[k % 2], seed=k, order=6) + [(what, 1), (what, 255), (what, 256), (what, 257), (what, 331)])
        k += 1
        add("generator %d add of 1100" % g, gen(g, G.PINK, seed=k, order=10) + [(G.G_ADD, N)])
        add("generator %d add of 1100 with NULL" % g, gen(g, G.PINK, seed=k, order=10) + [(G.G_ADD_NULL, N)])
        add("generator %d mul of 1100" % g, gen(g, G.WHITE, seed=k) + [(G.G_MUL, N)])
        add("generator %d overwrite of 1100" % g, gen(g, G.RED, seed=k, order=50) + [(G.G_OVER, N)])
    add("mul with NULL between two calls", gen(G.GEN_LCG, G.PINK, order=6) + [(G.G_OVER, 300), (G.G_MUL_NULL, 300), (G.G_AMP, 0.5), (G.G_MUL_NULL, 100), (G.G_OVER, 300)])
    # the idle sources keep their state: the third call goes on where the first stopped
    add("LCG, MLS, LCG", gen(G.GEN_LCG) + [(G.G_OVER, 300), (G.G_GEN, G.GEN_MLS), (G.G_OVER, 300), (G.G_GEN, G.GEN_LCG), (G.G_OVER, 300)])
    add("LCG alone", gen(G.GEN_LCG) + [(G.G_OVER, 300), (G.G_OVER, 300)])
    add("Velvet, LCG, Velvet, coloured", gen(G.GEN_VELVET, G.BLUE, order=8) + [(G.G_OVER, 300), (G.G_GEN, G.GEN_LCG), (G.G_ADD, 300), (G.G_GEN, G.GEN_VELVET), (G.G_ADD, 300)])
    # (a generator or a colour outside its enum is an invalid enum load in the reference's build: not recorded; the device tests hold the
    # bank to the restatement there, which takes the switches' default: branches)
    # each setter between calls: with its UPD_* effect, and with the value it already has
    setters = ((G.G_RATE, 44100), (G.G_MLS_BITS, 9), (G.G_MLS_SEED, 0x155), (G.G_DIST, R.LCG_TRIANGULAR), (G.G_VTYPE, V.ARN), (G.G_VWIDTH, 0.001),
               (G.G_VDELTA, 0.25), (G.G_VCRUSH, 1), (G.G_VPROB, 0.3), (G.G_COLOR, G.VIOLET), (G.G_ORDER, 12), (G.G_SLOPE, 0.25, G.NEPER), (G.G_AMP, 0.5), (G.G_OFF, 0.25))
    concerned = {G.G_MLS_BITS: G.GEN_MLS, G.G_MLS_SEED: G.GEN_MLS, G.G_VTYPE: G.GEN_VELVET, G.G_VWIDTH: G.GEN_VELVET, G.G_VDELTA: G.GEN_VELVET,
                 G.G_VCRUSH: G.GEN_VELVET, G.G_VPROB: G.GEN_VELVET, G.G_RATE: G.GEN_VELVET, G.G_AMP: G.GEN_MLS}
    for s in setters:                                       # on the generator that the setter concerns (the LCG where it concerns all)
        for g in (concerned.get(s[0], G.GEN_LCG),):
            k += 1
            color = G.ARBITRARY if s[0] == G.G_SLOPE else G.PINK
            pre = gen(g, color, seed=k, order=6) + ([(G.G_SLOPE, -0.75, G.NEPER)] if color == G.ARBITRARY else [])
            add("generator %d setter %d" % (g, s[0]), pre + [(G.G_OVER, 200), s, (G.G_OVER, 200), s, (G.G_ADD, 200)])
    add("MLS seed set to the running state's seed again", gen(G.GEN_MLS) + [(G.G_OVER, 100), (G.G_MLS_SEED, 0x99), (G.G_OVER, 100), (G.G_MLS_BITS, 30), (G.G_MLS_BITS, 17 + 1), (G.G_OVER, 100)])
    add("init again in mid-stream", gen(G.GEN_VELVET, G.PINK, order=4) + [(G.G_OVER, 300)] + gen(G.GEN_VELVET, G.PINK, order=4, seed=2) + [(G.G_OVER, 300)])
    add("colour white keeps the filter's update pending", gen(G.GEN_LCG, G.WHITE) + [(G.G_OVER, 100), (G.G_COLOR, G.PINK), (G.G_COLOR, G.WHITE), (G.G_OVER, 100), (G.G_CHART, 0)])
    add("sample rate 30000: the 20 kHz fallback of the auto norm", gen(G.GEN_LCG, G.BLUE, rate=30000, order=8) + [(G.G_OVER, 300), (G.G_CHART, 1)])
    # special levels
    for A, off in ((0.0, 0.0), (-0.0, -0.0), (-2.0, 0.5), (np.inf, 0.0), (1.0, -0.0), (0.0, -0.0)):
        for g in (G.GEN_MLS, G.GEN_LCG, G.GEN_VELVET):
            k += 1
            add("generator %d amplitude %g offset %g" % (g, A, off), gen(g, (G.WHITE, G.PINK)[k % 2], seed=k, order=4) + [(G.G_AMP, A), (G.G_OFF, off), (G.G_OVER, 150), (G.G_ADD, 150), (G.G_MUL, 150)])
    # the transcendental distributions, white (the interval rule of noise_ref.py holds them)
    for dist in (R.LCG_EXPONENTIAL, R.LCG_GAUSSIAN):
        add("LCG distribution %d, white" % dist, gen(G.GEN_LCG, G.WHITE, dist=dist) + [(G.G_OVER, 300), (G.G_ADD, 300)])
    return out


def write_cases(path, cs, src):
    with open(path, "wb") as f:
        f.write(np.array([len(cs), N, F], u32).tobytes() + G.CHART_F.tobytes())
        for c in cs:
            f.write(np.array([len(c["ops"])], u32).tobytes() + c["ops"].tobytes() + (finite_row() if c["finite"] else src).tobytes())


def read_results(path, cs):
    got = []
    with open(path, "rb") as f:
        for _ in cs:
            filled = int(np.frombuffer(f.read(4), u32)[0])
            out = np.frombuffer(f.read(4 * N), f32)[:filled].copy()
            words = np.frombuffer(f.read(8 * G.WORDS), u64).copy()
            ns = int(np.frombuffer(f.read(4), u32)[0])
            sec = np.frombuffer(f.read(4 * 64 * 5), f32).reshape(64, 5)[:ns].copy()
            chart = np.frombuffer(f.read(8 * F), f32).copy()
            got.append(dict(out=out, words=words, chains=sec, chart=chart))
        assert f.read(1) == b""
    return got


def run(exe, cs, src, cwd):
    a, b = os.path.join(cwd, "cases.bin"), os.path.join(cwd, "results.bin")
    write_cases(a, cs, src)
    subprocess.run([exe, a, b], check=True, timeout=900)
    return read_results(b, cs)


def compile_driver(reference, d, source, exe, extra=()):
    """`source` against the reference's unmodified sources and the overlays, in directory d."""
    for rel, text in OVERLAYS:
        os.makedirs(os.path.dirname(os.path.join(d, "overlay", rel)), exist_ok=True)
        with open(os.path.join(d, "overlay", rel), "w") as f:
            f.write(text)
    srcs = [source] + [os.path.join(reference, "src", "main", n) for n in REF_SOURCES]
    inc = ["-I" + os.path.join(d, "overlay"), "-I" + os.path.join(ROOT, "oracle", "ref_shim"), "-I" + os.path.join(reference, "include")]
    subprocess.check_call(["g++"] + FLAGS + list(extra) + inc + ["-o", exe] + srcs + ["-lm"])
    return exe


def run_reference(reference, sanitized=True):
    cs, src = cases(), source_row()
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "driver.cpp"), "w") as f:
            f.write(DRIVER)
        exe = compile_driver(reference, d, os.path.join(d, "driver.cpp"), os.path.join(d, "ref"))
        if sanitized:                                       # stand-alone, before anything is recorded
            san = run(compile_driver(reference, d, os.path.join(d, "driver.cpp"), os.path.join(d, "ref_san"), SAN_FLAGS), cs, src, d)
        got = run(exe, cs, src, d)
    for c, a, b in zip(cs, san if sanitized else got, got):
        assert R.same(a["out"], b["out"]).all() and np.array_equal(a["words"], b["words"]), c["name"]
    return cs, src, got


def build(reference, sanitized=True):
    cs, src, got = run_reference(reference, sanitized)
    arrs = {"src": src, "finite": np.array([c["finite"] for c in cs], np.uint8), "names": np.array([c["name"] for c in cs]), "ops_n": np.array([len(c["ops"]) for c in cs], u32),
            "ops": np.concatenate([c["ops"] for c in cs]), "out_n": np.array([g["out"].size for g in got], u32),
            "out": np.concatenate([g["out"] for g in got]), "words": np.array([g["words"] for g in got]),
            "chains_n": np.array([g["chains"].shape[0] for g in got], u32), "chains": np.concatenate([g["chains"] for g in got]),
            "chart": np.array([g["chart"] for g in got])}
    return npz_bytes(arrs)


def load(path=OUT):
    """The stored file as a list of cases: dicts of name, ops [k, 4], src [N], out [filled], words [64], chains [n, 5], chart [2 F]."""
    z = np.load(path)
    off = np.concatenate([[0], np.cumsum(z["ops_n"].astype(np.int64))])
    oo = np.concatenate([[0], np.cumsum(z["out_n"].astype(np.int64))])
    co = np.concatenate([[0], np.cumsum(z["chains_n"].astype(np.int64))])
    fin = finite_row()
    assert np.array_equal(fin[np.isfinite(z["src"])], z["src"][np.isfinite(z["src"])].clip(-1.5, 1.5))
    return [dict(name=str(z["names"][i]), ops=z["ops"][off[i]:off[i + 1]], finite=bool(z["finite"][i]), src=fin if z["finite"][i] else z["src"], out=z["out"][oo[i]:oo[i + 1]], words=z["words"][i],
                 chains=z["chains"][co[i]:co[i + 1]], chart=z["chart"][i]) for i in range(len(z["names"]))]


def layout_lines(exe):
    """What tests/cpp/noise_generator_layout.cpp prints, both ways, as {first word: the other words}."""
    text = subprocess.check_output([exe]).decode() + subprocess.check_output([exe, "behaviour"]).decode()
    return {l.split()[0]: l.split()[1:] for l in text.splitlines() if l.strip()}


def inventories(reference):
    """(dump keys, sizeof and offsetof of both classes from the layout program against the reference's headers; their public names)."""
    with tempfile.TemporaryDirectory() as d:
        got = layout_lines(compile_driver(reference, d, LAYOUT, os.path.join(d, "layout")))
    dump = {"SpectralTilt": {"keys": got["SpectralTilt"], "offsetof": [int(v) for v in got["offsetof_tilt"]]},
            "NoiseGenerator": {"keys": got["NoiseGenerator"], "offsetof": [int(v) for v in got["offsetof_generator"]],
                               "offsetof_params": [int(v) for v in got["offsetof_params"]]},
            "sizeof": [int(v) for v in got["sizeof"]]}
    names = {h: public_names(os.path.join(reference, "include", "lsp-plug.in", "dsp-units", h), cls) for h, cls in HEADERS.items()}
    return dump, names


if __name__ == "__main__":
    reference = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(ROOT), "reference")
    data = build(reference)
    assert len(data) <= 400000, len(data)
    with open(OUT, "wb") as f:
        f.write(data)
    dump, names = inventories(reference)
    for name, what in (("noise_generator_dump_keys.json", dump), ("noise_generator_public_names.json", names)):
        with open(os.path.join(HERE, name), "w") as f:
            json.dump(what, f, indent=1)
            f.write("\n")
    print("%d cases, %d bytes" % (len(load()), len(data)))
