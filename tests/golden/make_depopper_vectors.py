"""Writes tests/golden/depopper_ref_vectors.npz, depopper_dump_keys.json and depopper_public_names.json: what the reference's own
Depopper class computes on a list of cases.  Data only: settings, operation lists, inputs, the reference's env and gain, every
state word, the designed values, the fade tables and the logical contents of both buffers.  Run where the reference tree exists:

    python tests/golden/make_depopper_vectors.py [reference tree]

util/Depopper.cpp and iface/IStateDumper.cpp are compiled unmodified into a temporary directory (-O2 -ffp-contract=off -msse2
-mfpmath=sse) against oracle/ref_shim plus a small overlay, written here, of what that shim lacks: align_size (and lsp_max over two
types) beside DEFAULT_ALIGN, and dsp::h_sum, the serial float32 sum, oldest first -- the stand-in that the stereo meters' vectors
use.  units.h is the reference's as it is.  The program -- a stand-alone one with its own main -- is built a first time with
-fsanitize=address,undefined and run on the same cases before anything is recorded: every case stays inside the reference's
defined behaviour, which is the set of settings that the bank accepts.

The file holds the signals (x: [signals, N]) and case by case: names, signal (the row of x a case reads from its start), n (the
samples it processes), ops [k, 4] float64 (what, up to three arguments), env [n], gain [n], state [6] int64 (fRms's bits, nState,
nCounter, nDelay, nRmsOff, nLookOff), design [19] int64 (of both fades nSamples, nDelay and fPoly's bits; nRmsLen, nLookCount,
fRmsNorm's bits, nLookMin, nLookMax, nRmsMin, nRmsMax), rms_buf (the last nRmsMin squares), gain_buf (the last nLookMin gains),
tab_in and tab_out (crossfade(fade, x) for x = 0 .. nSamples - 1).  The rows of different lengths lie end to end."""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
from make_bypass_crossfade_vectors import npz_bytes, public_names  # noqa: E402

OUT = os.path.join(HERE, "depopper_ref_vectors.npz")
f32 = np.float32

N = 9400
SR = 48000
(INIT, IN_MODE, OUT_MODE, IN_TIME, OUT_TIME, IN_THRESH, OUT_THRESH, IN_DELAY, OUT_DELAY, RMS_LENGTH, PROCESS, RECONFIGURE) = range(12)
SIG_BURSTS, SIG_SPECIAL, SIG_SILENCES = range(3)
MODES = ("linear", "cubic", "sine", "gaussian", "parabolic")
MAX_FADE = 10.0

OVERLAY = {
    "lsp-plug.in/dsp-units/version.h": r'''
#ifndef DEPOPPER_OVERLAY_VERSION_H_
#define DEPOPPER_OVERLAY_VERSION_H_
#include <lsp-plug.in/common/types.h>
#ifndef LSP_DSP_UNITS_PUBLIC
#define LSP_DSP_UNITS_PUBLIC
#endif
#endif
''',
    "lsp-plug.in/common/alloc.h": r'''
#ifndef DEPOPPER_OVERLAY_ALLOC_H_
#define DEPOPPER_OVERLAY_ALLOC_H_
#include_next <lsp-plug.in/common/alloc.h>
namespace lsp
{
    inline size_t align_size(size_t size, size_t align) { size_t off = size % align; return (off == 0) ? size : size + align - off; }
    template <class A, class B> inline A lsp_max(A a, B b) { return (a > A(b)) ? a : A(b); }
}
#endif
''',
    "lsp-plug.in/dsp/dsp.h": r'''
#ifndef DEPOPPER_OVERLAY_DSP_H_
#define DEPOPPER_OVERLAY_DSP_H_
#include_next <lsp-plug.in/dsp/dsp.h>
namespace lsp
{
    namespace dsp
    {
        inline float h_sum(const float *src, size_t count)
        {
            float r = 0.0f;
            for (size_t i = 0; i < count; ++i)
                r += src[i];
            return r;
        }
    }
}
#endif
''',
}

# reads the cases, runs the class, writes what the module's text lists; with "keys" as its only argument it prints sizeof and
# offsetof of the class and what dump() writes
DRIVER = r'''
#define private public
#define protected public
#include <lsp-plug.in/dsp-units/util/Depopper.h>
#undef private
#undef protected
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
using namespace lsp;
struct keys: public dspu::IStateDumper
{
    std::string seen;
    int depth = 0;
    void note(const char *n) { seen += " "; seen += std::to_string(depth); seen += ":"; seen += n; }
    void begin_object(const char *n, const void *, size_t) override { note(n); ++depth; }
    void begin_object(const void *, size_t) override    { ++depth; }
    void end_object() override                          { --depth; }
    void begin_array(const char *n, const void *, size_t) override { note(n); ++depth; }
    void begin_array(const void *, size_t) override     { ++depth; }
    void end_array() override                           { --depth; }
    void write(const char *n, const void *) override    { note(n); }
    void write(const char *n, bool) override            { note(n); }
    void write(const char *n, signed int) override      { note(n); }
    void write(const char *n, unsigned int) override    { note(n); }
    void write(const char *n, signed long) override     { note(n); }
    void write(const char *n, unsigned long) override   { note(n); }
    void write(const char *n, signed long long) override { note(n); }
    void write(const char *n, unsigned long long) override { note(n); }
    void write(const char *n, float) override           { note(n); }
    void writev(const char *n, const float *, size_t) override { note(n); }
};
static uint32_t bits(float v) { uint32_t u; memcpy(&u, &v, 4); return u; }
static void put(FILE *g, const float *p, size_t n) { int64_t k = int64_t(n); fwrite(&k, 8, 1, g); if (n > 0) fwrite(p, 4, n, g); }
int main(int argc, char **argv)
{
    using dspu::Depopper;
    if (argc == 2 && strcmp(argv[1], "keys") == 0)
    {
        Depopper d;
        d.init(48000, 10.0f, 1.0f);
        keys k;
        d.dump(&k);
        printf("sizeof %zu %zu\n", sizeof(Depopper), sizeof(Depopper::fade_t));
        printf("offsetof %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", offsetof(Depopper, nSampleRate), offsetof(Depopper, nState),
               offsetof(Depopper, fLookMax), offsetof(Depopper, fRmsMax), offsetof(Depopper, nCounter), offsetof(Depopper, fRms),
               offsetof(Depopper, sFadeIn), offsetof(Depopper, sFadeOut), offsetof(Depopper, pGainBuf), offsetof(Depopper, bReconfigure));
        printf("Depopper%s\n", k.seen.c_str());
        return 0;
    }
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb"), *g = fopen(argv[2], "wb");
    if (!f || !g) return 2;
    uint32_t cases;
    if (fread(&cases, 4, 1, f) != 1) return 3;
    for (uint32_t c = 0; c < cases; ++c)
    {
        uint32_t h[2];
        if (fread(h, 4, 2, f) != 2) return 3;
        const uint32_t k = h[0], n = h[1];
        std::vector<double> ops(4 * size_t(k));
        if (fread(ops.data(), 8, ops.size(), f) != ops.size()) return 3;
        std::vector<float> src(n), env(n, 0.0f), gain(n, 0.0f);
        if (fread(src.data(), 4, n, f) != n) return 3;
        Depopper d;
        size_t at = 0;
        for (uint32_t j = 0; j < k; ++j)
        {
            const double *o = &ops[4 * size_t(j)];
            switch (int(o[0]))
            {
                case 0: if (!d.init(size_t(o[1]), float(o[2]), float(o[3]))) return 4; break;
                case 1: d.set_fade_in_mode(dspu::depopper_mode_t(int(o[1]))); break;
                case 2: d.set_fade_out_mode(dspu::depopper_mode_t(int(o[1]))); break;
                case 3: d.set_fade_in_time(float(o[1])); break;
                case 4: d.set_fade_out_time(float(o[1])); break;
                case 5: d.set_fade_in_threshold(float(o[1])); break;
                case 6: d.set_fade_out_threshold(float(o[1])); break;
                case 7: d.set_fade_in_delay(float(o[1])); break;
                case 8: d.set_fade_out_delay(float(o[1])); break;
                case 9: d.set_rms_length(float(o[1])); break;
                case 10:
                {
                    const size_t m = size_t(o[1]);
                    if (at + m > n) return 5;
                    d.process(&env[at], &gain[at], &src[at], m);
                    at += m;
                    break;
                }
                case 11: d.reconfigure(); break;
                default: return 6;
            }
        }
        if (at != n) return 7;
        fwrite(env.data(), 4, n, g);
        fwrite(gain.data(), 4, n, g);
        const int64_t words[25] = { bits(d.fRms), d.nState, d.nCounter, d.nDelay, d.nRmsOff, d.nLookOff,
            d.sFadeIn.nSamples, d.sFadeIn.nDelay, bits(d.sFadeIn.fPoly[0]), bits(d.sFadeIn.fPoly[1]), bits(d.sFadeIn.fPoly[2]), bits(d.sFadeIn.fPoly[3]),
            d.sFadeOut.nSamples, d.sFadeOut.nDelay, bits(d.sFadeOut.fPoly[0]), bits(d.sFadeOut.fPoly[1]), bits(d.sFadeOut.fPoly[2]), bits(d.sFadeOut.fPoly[3]),
            d.nRmsLen, d.nLookCount, bits(d.fRmsNorm), d.nLookMin, d.nLookMax, d.nRmsMin, d.nRmsMax };
        fwrite(words, 8, 25, g);
        put(g, &d.pRmsBuf[d.nRmsOff - d.nRmsMin], d.nRmsMin);
        put(g, &d.pGainBuf[d.nLookOff - d.nLookMin], d.nLookMin);
        for (dspu::Depopper::fade_t *fd : { &d.sFadeIn, &d.sFadeOut })
        {
            std::vector<float> t;
#ifndef DEPOPPER_NO_TABLES                  /* (a class that keeps its tables elsewhere has no crossfade()) */
            for (ssize_t x = 0; x < fd->nSamples; ++x)
                t.push_back(d.crossfade(fd, x));
#else
            (void)fd;
#endif
            put(g, t.data(), t.size());
        }
    }
    fclose(f);
    return fclose(g) == 0 ? 0 : 8;
}
'''

FLAGS = ["-std=c++11", "-O2", "-ffp-contract=off", "-msse2", "-mfpmath=sse", "-DLSP_DSP_UNITS_BUILTIN", "-Wall"]
SAN_FLAGS = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
REF_SOURCES = ("util/Depopper.cpp", "iface/IStateDumper.cpp")


def samples_of(ms, sr=SR):
    return int((f32(ms) * f32(0.001)) * f32(sr))


def ms_for(samples, sr=SR, most=None):
    """A time in milliseconds that millis_to_samples() turns into exactly `samples` (not above `most`)."""
    ms = f32(samples) / f32(sr) * f32(1000.0)
    for _ in range(64):
        got = samples_of(ms, sr)
        if got == samples and (most is None or ms <= f32(most)):
            return float(ms)
        ms = np.nextafter(ms, f32(np.inf) if got < samples else f32(-np.inf))
    raise AssertionError(samples)


def signals():
    rng = np.random.default_rng(4242)
    # bursts of noise and gaps of exact silence or of a low hiss, of every kind of length, over both buffer wraps
    bursts = np.zeros(N)
    at, k = 50, 0
    lengths = (350, 60, 3, 3, 800, 10, 1, 300, 700, 2, 40, 520)
    gaps = (300, 240, 3, 291, 500, 1, 2, 800, 5, 40, 200, 600)
    while at < N:
        n = lengths[k % len(lengths)]
        bursts[at:at + n] = 0.5 * rng.standard_normal(min(n, N - at))
        at += n
        gap = gaps[k % len(gaps)]
        if k % 3 == 1:
            bursts[at:at + gap] = 1e-3 * rng.standard_normal(min(gap, max(N - at, 0)))
        at += gap
        k += 1
    # levels at exactly the thresholds 0.25 and 0.125 (an RMS length of 32 keeps the mean exact), subnormal squares, NaN and Inf
    special = np.zeros(N)
    sign = (-1.0) ** np.arange(N)
    special[20:300] = 0.25 * sign[20:300]
    special[300:600] = 0.125 * sign[300:600]
    special[600:660] = 0.0625 * sign[600:660]
    special[700:900] = 1e-22 * rng.standard_normal(200)
    special[900:1100] = 0.5 * rng.standard_normal(200)
    special[1000] = np.nan
    special[1100:1300] = 0.25 * sign[1100:1300]
    special[1200] = np.inf
    special[1400:1700] = 0.5 * rng.standard_normal(300)
    special[1500] = -np.inf
    special[1501] = np.nan
    special[2500:2800] = 0.5 * rng.standard_normal(300)       # after 800 samples of silence
    special[2800:] = bursts[2800:]
    # silences of every length from 1 to 60 between bursts of 70 (longer ones are in the rows above)
    silences = np.zeros(N)
    at = 10
    for gap in range(1, 61):
        silences[at:at + 70] = 0.5 * rng.standard_normal(70)
        at += 70 + gap
    silences[at:] = bursts[at:]
    return np.stack([bursts, special, silences]).astype(f32)


def setup(max_rms=1.0, rms=48, fade_in=300, fade_out=480, in_delay=0, out_delay=0, in_mode=0, out_mode=0, in_thr=0.1, out_thr=0.05):
    """init and every setter; the times as sample counts"""
    return [(INIT, SR, MAX_FADE, max_rms), (IN_MODE, in_mode), (OUT_MODE, out_mode), (IN_TIME, ms_for(fade_in)),
            (OUT_TIME, ms_for(fade_out, most=MAX_FADE)), (IN_THRESH, float(f32(in_thr))), (OUT_THRESH, float(f32(out_thr))),
            (IN_DELAY, ms_for(in_delay)), (OUT_DELAY, ms_for(out_delay)), (RMS_LENGTH, ms_for(rms, most=max_rms))]


def ops_of(first, n, calls, events=()):
    """first: the operations before the first sample; events: (sample, [ops]) later on; the samples between in calls of the
    lengths `calls`, taken in turn."""
    ops, at, k = list(first), 0, 0
    for stop, more in list(events) + [(n, [])]:
        while at < stop:
            m = min(calls[k % len(calls)], stop - at)
            ops.append((PROCESS, m))
            at += m
            k += 1
        ops.extend(more)
    out = np.zeros((len(ops), 4))
    for i, op in enumerate(ops):
        out[i, :len(op)] = op
    return out


UNEVEN = (113, 1, 256, 31, 700, 257, 32, 33, 255, 515)


def cases():
    out = []

    def add(name, sig, n, ops):
        out.append((name, sig, n, ops))

    for m, mode in enumerate(MODES):
        add("mode %s both sides" % mode, SIG_BURSTS, 2400, ops_of(setup(in_mode=m, out_mode=m), 2400, (2400,)))
    add("modes gaussian in, sine out, in calls of 113", SIG_BURSTS, 2400, ops_of(setup(in_mode=3, out_mode=2), 2400, (113,)))
    for rms, fo, fi, di, do in ((1, 0, 0, 0, 0), (31, 1, 1, 1, 0), (32, 255, 300, 0, 1), (33, 257, 300, 40, 40), (48, 480, 1, 1, 40), (96, 480, 300, 0, 0),
                                (96, 0, 300, 40, 1), (1, 257, 0, 0, 40)):
        add("rms %d fade-out %d fade-in %d delays %d %d" % (rms, fo, fi, di, do), SIG_BURSTS, 2400,
            ops_of(setup(max_rms=2.0, rms=rms, fade_out=fo, fade_in=fi, in_delay=di, out_delay=do, out_mode=(rms + fo) % 5, in_mode=(fi + di) % 5),
                   2400, UNEVEN))
    add("both wraps max_rms 1", SIG_BURSTS, N, ops_of(setup(), N, UNEVEN))
    add("both wraps max_rms 2 rms 96", SIG_SILENCES, N, ops_of(setup(max_rms=2.0, rms=96, out_mode=1, in_mode=4), N, UNEVEN[::-1]))
    add("one call", SIG_SILENCES, 5000, ops_of(setup(fade_out=255, out_delay=1), 5000, (5000,)))
    add("the same in uneven calls", SIG_SILENCES, 5000, ops_of(setup(fade_out=255, out_delay=1), 5000, UNEVEN))
    add("thresholds met exactly, subnormals, NaN and Inf", SIG_SPECIAL, 3400,
        ops_of(setup(rms=32, in_thr=0.25, out_thr=0.125, fade_in=40, fade_out=100), 3400, UNEVEN))
    add("NaN and Inf with delays", SIG_SPECIAL, 3400,
        ops_of(setup(max_rms=2.0, rms=33, in_thr=0.25, out_thr=0.125, fade_in=300, fade_out=257, in_delay=40, out_delay=40, in_mode=2, out_mode=3),
               3400, (3400,)))
    # a fade-out begun before the fade-in is over: the bursts of 60, 3 and 10 against a fade-in of 300
    add("fade-out inside the fade-in", SIG_BURSTS, 2400, ops_of(setup(fade_in=300, fade_out=480, rms=31, max_rms=2.0), 2400, (256,)))
    change = [(500, [(RMS_LENGTH, ms_for(10))]), (900, [(OUT_TIME, ms_for(100))]), (1300, [(OUT_MODE, 3), (IN_MODE, 1)]),
              (1700, [(RMS_LENGTH, ms_for(96, most=2.0)), (OUT_TIME, ms_for(480, most=MAX_FADE)), (IN_DELAY, ms_for(5))]),
              (2100, [(IN_THRESH, 0.3), (OUT_THRESH, 0.2), (RECONFIGURE,)])]
    add("setters between calls", SIG_BURSTS, 2400, ops_of(setup(max_rms=2.0), 2400, UNEVEN, change))
    again = [(1000, [(INIT, SR, 5.0, 1.0), (OUT_TIME, ms_for(200)), (RMS_LENGTH, ms_for(40))]), (1800, [(INIT, 44100, MAX_FADE, 2.0)])]
    add("init with new maxima", SIG_BURSTS, 2400, ops_of(setup(max_rms=2.0, rms=96), 2400, UNEVEN, again))
    return out


def read_floats(raw, at):
    n = int(raw[at:at + 8].view(np.int64)[0])
    return raw[at + 8:at + 8 + 4 * n].view(f32).copy(), at + 8 + 4 * n


def run(exe, x, cs, cwd):
    src, dst = os.path.join(cwd, "cases.bin"), os.path.join(cwd, "results.bin")
    with open(src, "wb") as f:
        f.write(np.array([len(cs)], np.uint32).tobytes())
        for name, sig, n, ops in cs:
            f.write(np.array([len(ops), n], np.uint32).tobytes() + ops.astype(np.float64).tobytes() + x[sig, :n].tobytes())
    subprocess.run([exe, src, dst], check=True, timeout=600)
    raw = np.fromfile(dst, np.uint8)
    got, at = [], 0
    for name, sig, n, ops in cs:
        r = {"env": raw[at:at + 4 * n].view(f32).copy(), "gain": raw[at + 4 * n:at + 8 * n].view(f32).copy()}
        at += 8 * n
        words = raw[at:at + 200].view(np.int64).copy()
        at += 200
        r["state"], r["design"] = words[:6], words[6:]
        for key in ("rms_buf", "gain_buf", "tab_in", "tab_out"):
            r[key], at = read_floats(raw, at)
        got.append(r)
    assert at == raw.size, (at, raw.size)
    return got


def same(a, b):
    return all(np.array_equal(p[k].view(np.uint32) if p[k].dtype == f32 else p[k], q[k].view(np.uint32) if q[k].dtype == f32 else q[k])
               for p, q in zip(a, b) for k in p)


def compile_driver(reference, d, source, exe, extra=()):
    """`source` and the reference's class sources against the overlay (written into d), the shim and the reference's headers."""
    for rel, text in OVERLAY.items():
        os.makedirs(os.path.dirname(os.path.join(d, "overlay", rel)), exist_ok=True)
        with open(os.path.join(d, "overlay", rel), "w") as f:
            f.write(text)
    srcs = [source] + [os.path.join(reference, "src", "main", n) for n in REF_SOURCES]
    inc = ["-I" + os.path.join(d, "overlay"), "-I" + os.path.join(ROOT, "oracle", "ref_shim"), "-I" + os.path.join(reference, "include")]
    subprocess.check_call(["g++"] + FLAGS + list(extra) + inc + ["-o", exe] + srcs + ["-lm"])
    return exe


def run_reference(reference):
    x = signals()
    cs = cases()
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "driver.cpp"), "w") as f:
            f.write(DRIVER)
        for exe, extra in (("ref_san", SAN_FLAGS), ("ref", [])):
            compile_driver(reference, d, os.path.join(d, "driver.cpp"), os.path.join(d, exe), extra)
        san = run(os.path.join(d, "ref_san"), x, cs, d)                     # stand-alone, before anything is recorded
        got = run(os.path.join(d, "ref"), x, cs, d)
        keys = subprocess.check_output([os.path.join(d, "ref"), "keys"]).decode().splitlines()
    assert same(got, san)
    dump = {"sizeof": [int(v) for v in keys[0].split()[1:]], "offsetof": [int(v) for v in keys[1].split()[1:]],
            "Depopper": keys[2].split()[1:]}
    names = {"util/Depopper.h": public_names(os.path.join(reference, "include", "lsp-plug.in", "dsp-units", "util", "Depopper.h"), "Depopper")}
    return x, cs, got, dump, names


def check_branches(cs, got):
    """What the cases are there for has happened in them, and every case is one that the bank accepts."""
    by = {c[0]: r for c, r in zip(cs, got)}
    for c, r in zip(cs, got):
        d = r["design"]
        assert d[12] > 0 and 0 <= d[6] <= samples_of(MAX_FADE), (c[0], "nRmsLen == 0 or a fade-out outside [0, max_fade]")
        assert c[2] <= N
    r = by["both wraps max_rms 1"]
    assert r["env"].size > 2 * 0x1000 + 600, "no wrap of both buffers"
    g = by["mode linear both sides"]["gain"]
    assert np.any((g > 0) & (g < 1)) and np.any(g == 1) and np.any(g == 0)
    assert np.isnan(by["thresholds met exactly, subnormals, NaN and Inf"]["env"]).any()
    e = by["thresholds met exactly, subnormals, NaN and Inf"]["env"]
    assert np.any(e == f32(0.25)) and np.any(e == f32(0.125)) and np.any((e > 0) & (e < f32(1e-19)))
    assert not np.array_equal(by["rms 96 fade-out 0 fade-in 300 delays 40 1"]["gain"], by["rms 96 fade-out 480 fade-in 300 delays 0 0"]["gain"])
    a, b = by["one call"], by["the same in uneven calls"]
    assert same([a], [b]), "the output depends on how the stream is cut"
    return len(cs)


def build(reference):
    x, cs, got, dump, names = run_reference(reference)
    check_branches(cs, got)
    arrs = {"x": x, "names": np.array([c[0] for c in cs]), "signal": np.array([c[1] for c in cs], np.uint32),
            "n": np.array([c[2] for c in cs], np.uint32), "ops_n": np.array([len(c[3]) for c in cs], np.uint32),
            "ops": np.concatenate([c[3] for c in cs]), "state": np.stack([r["state"] for r in got]),
            "design": np.stack([r["design"] for r in got])}
    for key in ("env", "gain", "rms_buf", "gain_buf", "tab_in", "tab_out"):
        arrs[key] = np.concatenate([r[key] for r in got])
        arrs[key + "_n"] = np.array([r[key].size for r in got], np.uint32)
    return npz_bytes(arrs), dump, names


def load(path=OUT):
    """The stored file as (x, cases): dicts of name, signal, n, ops, env, gain, state, design, rms_buf, gain_buf, tab_in, tab_out."""
    z = np.load(path)
    count = len(z["names"])
    cs = [dict(name=str(z["names"][i]), signal=int(z["signal"][i]), n=int(z["n"][i]), state=z["state"][i], design=z["design"][i]) for i in range(count)]
    for key, lengths in [("ops", z["ops_n"])] + [(k, z[k + "_n"]) for k in ("env", "gain", "rms_buf", "gain_buf", "tab_in", "tab_out")]:
        off = np.concatenate([[0], np.cumsum(lengths.astype(np.int64))])
        for i in range(count):
            cs[i][key] = z[key][off[i]:off[i + 1]]
    return z["x"], cs


if __name__ == "__main__":
    data, dump, names = build(sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(ROOT), "reference"))
    with open(OUT, "wb") as f:
        f.write(data)
    with open(os.path.join(HERE, "depopper_dump_keys.json"), "w") as f:
        json.dump(dump, f, indent=1)
        f.write("\n")
    with open(os.path.join(HERE, "depopper_public_names.json"), "w") as f:
        json.dump(names, f, indent=1)
        f.write("\n")
    print("%d cases, %d bytes" % (len(load()[1]), len(data)))
