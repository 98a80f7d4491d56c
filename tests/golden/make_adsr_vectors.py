"""Writes tests/golden/adsr_ref_vectors.npz, adsr_dump_keys.json and adsr_public_names.json: what the reference's own ADSREnvelope
class computes on a list of cases.  Data only: settings as operation lists, inputs, outputs, the designed record's bits, nFlags.
Run where the reference tree exists:

    python tests/golden/make_adsr_vectors.py [reference tree]

util/ADSREnvelope.cpp, misc/interpolation.cpp and iface/IStateDumper.cpp are compiled unmodified into a temporary directory (-O2
-ffp-contract=off -msse2 -mfpmath=sse) against oracle/ref_shim.  The program -- a stand-alone one with its own main -- is built a
first time with -fsanitize=address,undefined and run on the same cases before anything is recorded.

The file holds the input rows (x: [rows, N]) and case by case: names, kind (process, process_mul, generate, generate_mul in place,
generate_mul with src), n (the samples recorded), first (the index of the first recorded sample: 0 but for the long call), tsig and
dsig (the rows of x that give the time values and the data; -1: none), start and step (bits), ops [k, 4] float64 (the setter's
number as tests/adsr_ref.py has it and up to three arguments), out [n], record [40] int64 (per curve fTime, fCurve, enFunction and
the six floats of gen_params_t as bits; fHoldTime, fBreakLevel, fSustainLevel as bits; nFlags) after the call, and flags_before
(nFlags after the last setter, before the call runs update_settings())."""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_bypass_crossfade_vectors import npz_bytes, public_names  # noqa: E402
import adsr_ref as A  # noqa: E402

OUT = os.path.join(HERE, "adsr_ref_vectors.npz")
f32 = np.float32
N = 4099
LONG = (1 << 24) + N
ROW_RAMP, ROW_RANDOM, ROW_SPECIAL, ROW_DATA = range(4)
POINTS = [f32(v) for v in (0.1, 0.2, 0.4, 0.6, 0.8, 1.0)]           # attack, hold, decay, slope, release, the end

# reads the cases, runs the class, writes the outputs and the designed record; with "keys" as its only argument it prints sizeof
# and offsetof of the class and what dump() writes
DRIVER = r'''
#define private public
#define protected public
#include <lsp-plug.in/dsp-units/util/ADSREnvelope.h>
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
    void begin_object(const void *, size_t) override    { note("{}"); ++depth; }
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
static int64_t bits(float v) { uint32_t u; memcpy(&u, &v, 4); return u; }
typedef dspu::ADSREnvelope E;
static void configure(E &e, int fn)
{
    e.set_attack(0.1f, 0.25f, E::function_t(fn));
    e.set_hold(0.2f, true);
    e.set_decay(0.4f, 0.25f, E::function_t(fn));
    e.set_break(0.5f, true);
    e.set_slope(0.6f, 0.25f, E::function_t(fn));
    e.set_release(0.8f, 0.25f, E::function_t(fn));
    e.set_sustain_level(0.3f);
    e.update_settings();
}
int main(int argc, char **argv)
{
    if (argc == 2 && strcmp(argv[1], "keys") == 0)
    {
        printf("sizeof %zu %zu %zu\n", sizeof(E), sizeof(E::curve_t), sizeof(E::gen_params_t));
        printf("offsetof %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", offsetof(E, vCurve), offsetof(E, fHoldTime), offsetof(E, fBreakLevel),
               offsetof(E, fSustainLevel), offsetof(E, nFlags), offsetof(E::curve_t, fCurve), offsetof(E::curve_t, enFunction),
               offsetof(E::curve_t, pGenerator), offsetof(E::curve_t, sParams));
        for (int fn = 0; fn < 6; ++fn)
        {
            E e;
            configure(e, fn);
            keys k;
            e.dump(&k);
            printf("%d%s\n", fn, k.seen.c_str());
        }
        return 0;
    }
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb"), *g = fopen(argv[2], "wb");
    if (!f || !g) return 2;
    uint32_t cases;
    if (fread(&cases, 4, 1, f) != 1) return 3;
    for (uint32_t c = 0; c < cases; ++c)
    {
        uint32_t h[6];                          // ops, kind, count, recorded, has a, has b
        float sv[2];
        if (fread(h, 4, 6, f) != 6 || fread(sv, 4, 2, f) != 2) return 3;
        const size_t k = h[0], count = h[2], n = h[3];
        std::vector<double> ops(4 * k);
        if (k && fread(ops.data(), 8, ops.size(), f) != ops.size()) return 3;
        std::vector<float> a(h[4] ? count : 0), b(h[5] ? count : 0), out(count, -77.0f);
        if (!a.empty() && fread(a.data(), 4, count, f) != count) return 3;
        if (!b.empty() && fread(b.data(), 4, count, f) != count) return 3;
        E e;
        for (size_t j = 0; j < k; ++j)
        {
            const double *o = &ops[4 * j];
            const float x = float(o[1]), y = float(o[2]);
            const E::function_t fx = E::function_t(int(o[1])), fz = E::function_t(int(o[3]));
            switch (int(o[0]))
            {
                case 0: e.set_attack_time(x); break;
                case 1: e.set_hold_time(x); break;
                case 2: e.set_decay_time(x); break;
                case 3: e.set_slope_time(x); break;
                case 4: e.set_relese_time(x); break;
                case 5: e.set_attack_curve(x); break;
                case 6: e.set_decay_curve(x); break;
                case 7: e.set_slope_curve(x); break;
                case 8: e.set_release_curve(x); break;
                case 9: e.set_attack_function(fx); break;
                case 10: e.set_decay_function(fx); break;
                case 11: e.set_slope_function(fx); break;
                case 12: e.set_release_function(fx); break;
                case 13: e.set_break_level(x); break;
                case 14: e.set_sustain_level(x); break;
                case 15: e.set_hold_enabled(o[1] != 0); break;
                case 16: e.set_break_enabled(o[1] != 0); break;
                case 17: e.set_attack(x, y, fz); break;
                case 18: e.set_hold(x, o[2] != 0); break;
                case 19: e.set_decay(x, y, fz); break;
                case 20: e.set_break(x, o[2] != 0); break;
                case 21: e.set_slope(x, y, fz); break;
                case 22: e.set_release(x, y, fz); break;
                case 23: e.update_settings(); break;
                default: return 6;
            }
        }
        const int64_t before = e.nFlags;
        switch (h[1])
        {
            case 0: e.process(out.data(), a.data(), count); break;                      // a: the time values
            case 1: out = b; e.process_mul(out.data(), a.data(), count); break;         // b: the data
            case 2: e.generate(out.data(), sv[0], sv[1], count); break;
            case 3: out = b; e.generate_mul(out.data(), sv[0], sv[1], count); break;
            case 4: e.generate_mul(out.data(), b.data(), sv[0], sv[1], count); break;
            default: return 7;
        }
        fwrite(out.data() + (count - n), 4, n, g);
        int64_t rec[41];
        int at = 0;
        for (int p = 0; p < 4; ++p)
        {
            const E::curve_t &cv = e.vCurve[p];
            rec[at++] = bits(cv.fTime), rec[at++] = bits(cv.fCurve), rec[at++] = int64_t(cv.enFunction);
            float six[6];
            memcpy(six, &cv.sParams, sizeof(six));
            for (int q = 0; q < 6; ++q)
                rec[at++] = bits(six[q]);
        }
        rec[at++] = bits(e.fHoldTime), rec[at++] = bits(e.fBreakLevel), rec[at++] = bits(e.fSustainLevel), rec[at++] = e.nFlags;
        rec[at++] = before;
        fwrite(rec, 8, 41, g);
    }
    fclose(f);
    return fclose(g) == 0 ? 0 : 8;
}
'''

FLAGS = ["-std=c++11", "-O2", "-ffp-contract=off", "-msse2", "-mfpmath=sse", "-DLSP_DSP_UNITS_BUILTIN", "-Wall"]
SAN_FLAGS = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
REF_SOURCES = ("util/ADSREnvelope.cpp", "misc/interpolation.cpp", "iface/IStateDumper.cpp")


def special_times():
    v = []
    for p in POINTS:
        v += [p, np.nextafter(p, f32(np.inf)), np.nextafter(p, f32(-np.inf))]
    v += [0.0, -0.0, 1e-45, -1e-45, 1e-39, np.nextafter(f32(0), f32(-1)), np.nextafter(f32(1), f32(2)), -0.5, 1.5, np.inf, -np.inf, np.nan,
          0.05, 0.15, 0.3, 0.5, 0.7, 0.9]
    return np.array(v, f32)


def special_data():
    return np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-45, -1e-39, -2.5, 1.0, 3.0], f32)


def rows():
    rng = np.random.default_rng(1515)
    x = np.zeros((4, N), f32)
    x[ROW_RAMP] = np.linspace(-0.05, 1.05, N).astype(f32)
    x[ROW_RANDOM] = rng.uniform(-0.1, 1.1, N).astype(f32)
    st, sd = special_times(), special_data()
    # every special time against every special datum, then random times
    grid_t, grid_d = np.repeat(st, sd.size), np.tile(sd, st.size)
    assert grid_t.size < N
    x[ROW_SPECIAL] = rng.uniform(-0.1, 1.1, N).astype(f32)
    x[ROW_SPECIAL, :grid_t.size] = grid_t
    x[ROW_DATA] = rng.standard_normal(N).astype(f32)
    x[ROW_DATA, :grid_d.size] = grid_d
    return x, grid_t.size


def base(fn, curve, hold=True, brk=True, times=(0.1, 0.2, 0.4, 0.6, 0.8), levels=(0.5, 0.3)):
    fns = fn if isinstance(fn, (tuple, list)) else (fn,) * 4
    cs = curve if isinstance(curve, (tuple, list)) else (curve,) * 4
    return [(A.SET_ATTACK, times[0], cs[0], fns[0]), (A.SET_HOLD, times[1], hold), (A.SET_DECAY, times[2], cs[1], fns[1]),
            (A.SET_BREAK, levels[0], brk), (A.SET_SLOPE, times[3], cs[2], fns[2]), (A.SET_RELEASE, times[4], cs[3], fns[3]),
            (A.SET_SUSTAIN_LEVEL, levels[1])]


def op_rows(ops):
    out = np.zeros((len(ops), 4))
    for i, op in enumerate(ops):
        out[i, :len(op)] = [float(v) for v in op]
    return out


FN_NAMES = ("none", "line", "line2", "cubic", "quadro", "exp")
CURVES = (0.0, 0.5, 1.0, 0.3)


def cases(grid):
    out = []

    def add(name, kind, ops, n, tsig=-1, dsig=-1, start=0.0, step=0.0, count=None):
        out.append(dict(name=name, kind=kind, ops=op_rows(ops), n=n, count=n if count is None else count, tsig=tsig, dsig=dsig,
                        start=f32(start), step=f32(step)))

    # every function in every segment at four curvatures; the specials and a dense ramp
    for fn in range(6):
        for cu in CURVES:
            add("process %s curve %g special" % (FN_NAMES[fn], cu), A.PROCESS, base(fn, cu), grid + 40, ROW_SPECIAL)
            add("process %s curve %g ramp" % (FN_NAMES[fn], cu), A.PROCESS, base(fn, cu), 640, ROW_RAMP if cu != 0.3 else ROW_RANDOM)
    add("process exp both signs ramp", A.PROCESS, base(A.EXP, (0.1, 0.9, 0.2, 0.7)), N, ROW_RAMP)
    add("process mixed functions random", A.PROCESS, base((A.CUBIC, A.EXP, A.QUADRO, A.LINE2), (0.2, 0.8, 0.6, 0.4)), N, ROW_RANDOM)
    # hold and break on and off
    for hold in (False, True):
        for brk in (False, True):
            for fn in (A.NONE, A.QUADRO):
                add("process %s hold %d break %d" % (FN_NAMES[fn], hold, brk), A.PROCESS, base(fn, 0.7, hold, brk), grid + 40, ROW_SPECIAL)
    # the special data against every special time
    for fn in (A.LINE, A.EXP):
        add("process_mul %s special" % FN_NAMES[fn], A.PROCESS_MUL, base(fn, 0.3), grid + 40, ROW_SPECIAL, ROW_DATA)
    add("process_mul cubic ramp", A.PROCESS_MUL, base(A.CUBIC, 0.6), N, ROW_RAMP, ROW_DATA)
    # empty segments, the constructor's state, all one, times out of order, setters that change nothing
    add("constructed", A.PROCESS, [], grid + 40, ROW_SPECIAL)
    add("constructed generate", A.GENERATE, [], 200, start=-0.1, step=0.01)
    for fn in range(6):
        add("all times 0.5 %s" % FN_NAMES[fn], A.PROCESS, base(fn, 0.5, times=(0.5,) * 5), 320, ROW_RAMP)
        add("all times one %s" % FN_NAMES[fn], A.PROCESS, base(fn, 0.5, times=(1.0,) * 5), 320, ROW_SPECIAL)
        add("no decay and no slope %s" % FN_NAMES[fn], A.PROCESS, base(fn, 0.5, times=(0.1, 0.2, 0.2, 0.2, 0.8)), 320, ROW_RANDOM)
    add("times out of order", A.PROCESS, base(A.LINE, 0.4, times=(0.5, 0.3, 0.2, 0.7, 0.6)), 640, ROW_RAMP)
    add("times out of order no hold", A.PROCESS, base(A.CUBIC, 0.4, hold=False, brk=False, times=(0.5, 0.9, 0.2, 0.95, 0.1)), 640, ROW_RAMP)
    add("values outside [0, 1] are clamped", A.PROCESS, [(A.SET_ATTACK, -0.5, 1.5, A.LINE), (A.SET_DECAY_TIME, 0.5), (A.SET_SUSTAIN_LEVEL, 7.0),
                                                     (A.SET_RELEASE_TIME, 2.0), (A.SET_BREAK_LEVEL, -1.0)], 320, ROW_RAMP)
    same = base(A.LINE2, 0.3) + [(A.UPDATE,)] + base(A.LINE2, 0.3) + [(A.SET_ATTACK_TIME, 0.1), (A.SET_HOLD_ENABLED, 1), (A.SET_BREAK_ENABLED, 1),
                                                                     (A.SET_DECAY_FUNCTION, A.LINE2), (A.SET_SLOPE_CURVE, 0.3), (A.SET_BREAK_LEVEL, 0.5)]
    add("the same values again", A.PROCESS, same, 320, ROW_RAMP)
    single = [(A.SET_ATTACK_TIME, 0.15), (A.SET_HOLD_TIME, 0.25), (A.SET_DECAY_TIME, 0.45), (A.SET_SLOPE_TIME, 0.65), (A.SET_RELEASE_TIME, 0.85),
              (A.SET_ATTACK_CURVE, 0.2), (A.SET_DECAY_CURVE, 0.4), (A.SET_SLOPE_CURVE, 0.6), (A.SET_RELEASE_CURVE, 0.8),
              (A.SET_ATTACK_FUNCTION, A.EXP), (A.SET_DECAY_FUNCTION, A.CUBIC), (A.SET_SLOPE_FUNCTION, A.LINE), (A.SET_RELEASE_FUNCTION, A.QUADRO),
              (A.SET_BREAK_LEVEL, 0.6), (A.SET_SUSTAIN_LEVEL, 0.4), (A.SET_HOLD_ENABLED, 1), (A.SET_BREAK_ENABLED, 1)]
    add("the single setters", A.PROCESS, single, 640, ROW_RAMP)
    add("a change after an update", A.PROCESS, single + [(A.UPDATE,), (A.SET_HOLD_ENABLED, 0), (A.SET_DECAY_TIME, 0.2), (A.UPDATE,), (A.SET_BREAK, 0.7, 0)],
        640, ROW_RANDOM)
    # generate*: starts before, in every stage, and after; every kind of step; the flavours in turn
    starts = (-0.25, 0.05, 0.15, 0.3, 0.5, 0.7, 0.9, 1.0, 1.5, np.nan)
    steps = (0.0, 1e-9, 0.011, 1.25, -0.013, np.inf, np.nan, -np.inf)
    k = 0
    for fn, cu in ((A.NONE, 0.5), (A.EXP, 0.2)):
        for start in starts:
            for step in steps:
                kind = (A.GENERATE, A.GENERATE_MUL, A.GENERATE_MUL_SRC)[k % 3]
                k += 1
                add("%s %s start %g step %g" % (("generate", "generate_mul", "generate_mul src")[kind - 2], FN_NAMES[fn], start, step), kind,
                    base(fn, cu), 128, dsig=-1 if kind == A.GENERATE else ROW_DATA, start=start, step=step)
    for kind, name in ((A.GENERATE, "generate"), (A.GENERATE_MUL, "generate_mul"), (A.GENERATE_MUL_SRC, "generate_mul src")):
        for fn, cu, hold, brk in ((A.CUBIC, 0.3, True, True), (A.LINE, 0.8, False, False)):
            add("%s %s whole row hold %d break %d" % (name, FN_NAMES[fn], hold, brk), kind, base(fn, cu, hold, brk), 1400,
                dsig=-1 if kind == A.GENERATE else ROW_DATA, start=-0.03, step=1.1 / 1400)
            add("%s %s backwards hold %d break %d" % (name, FN_NAMES[fn], hold, brk), kind, base(fn, cu, hold, brk), 700,
                dsig=-1 if kind == A.GENERATE else ROW_DATA, start=0.5 + 0.25 * hold, step=-1.0 / 700)
    add("generate mixed functions all of N", A.GENERATE, base((A.QUADRO, A.LINE2, A.EXP, A.CUBIC), (0.2, 0.8, 0.6, 0.4)), N, start=-0.01, step=1.02 / N)
    add("generate_mul src special data", A.GENERATE_MUL_SRC, base(A.EXP, 0.7), 640, dsig=ROW_DATA, start=-0.2, step=1.5 / 640)
    add("generate_mul special data", A.GENERATE_MUL, base(A.QUADRO, 0.7), 640, dsig=ROW_DATA, start=-0.2, step=1.5 / 640)
    # float(i) rounds: i above 2^24
    add("generate long", A.GENERATE, base((A.LINE, A.CUBIC, A.EXP, A.QUADRO), 0.35), N, start=-0.5, step=1.05 / (1 << 24), count=LONG)
    return out


def run(exe, x, cs, cwd):
    src, dst = os.path.join(cwd, "cases.bin"), os.path.join(cwd, "results.bin")
    with open(src, "wb") as f:
        f.write(np.array([len(cs)], np.uint32).tobytes())
        for c in cs:
            has_a, has_b = c["tsig"] >= 0, c["dsig"] >= 0
            f.write(np.array([len(c["ops"]), c["kind"], c["count"], c["n"], has_a, has_b], np.uint32).tobytes())
            f.write(np.array([c["start"], c["step"]], f32).tobytes())
            f.write(c["ops"].astype(np.float64).tobytes())
            for has, sig in ((has_a, c["tsig"]), (has_b, c["dsig"])):
                if has:
                    assert c["count"] == c["n"]
                    f.write(x[sig, :c["count"]].tobytes())
    subprocess.run([exe, src, dst], check=True, timeout=900)
    raw = np.fromfile(dst, np.uint8)
    got, at = [], 0
    for c in cs:
        n = c["n"]
        r = {"out": raw[at:at + 4 * n].view(f32).copy()}
        at += 4 * n
        words = raw[at:at + 328].view(np.int64).copy()
        at += 328
        r["record"], r["flags_before"] = words[:40], words[40]
        for part in range(4):                               # the floats of the union that the function does not design hold whatever
            used = {A.LINE: 5, A.LINE2: 5, A.CUBIC: 5, A.QUADRO: 6, A.EXP: 6}.get(int(r["record"][9 * part + 2]), 3)   # the memory held
            r["record"][9 * part + 3 + used:9 * part + 9] = 0
        got.append(r)
    assert at == raw.size, (at, raw.size)
    return got


def same(a, b):
    return all(np.array_equal(p["out"].view(np.uint32), q["out"].view(np.uint32)) and np.array_equal(p["record"], q["record"]) for p, q in zip(a, b))


def compile_driver(reference, d, source, exe, extra=()):
    srcs = [source] + [os.path.join(reference, "src", "main", n) for n in REF_SOURCES]
    inc = ["-I" + os.path.join(ROOT, "oracle", "ref_shim"), "-I" + os.path.join(reference, "include")]
    subprocess.check_call(["g++"] + FLAGS + list(extra) + inc + ["-o", exe] + srcs + ["-lm"])
    return exe


def run_reference(reference):
    x, grid = rows()
    cs = cases(grid)
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "driver.cpp"), "w") as f:
            f.write(DRIVER)
        for exe, extra in (("ref_san", SAN_FLAGS), ("ref", [])):
            compile_driver(reference, d, os.path.join(d, "driver.cpp"), os.path.join(d, exe), extra)
        san = run(os.path.join(d, "ref_san"), x, cs, d)                     # stand-alone, before anything is recorded
        got = run(os.path.join(d, "ref"), x, cs, d)
        keys = subprocess.check_output([os.path.join(d, "ref"), "keys"]).decode().splitlines()
    assert same(got, san)
    dump = {"sizeof": [int(v) for v in keys[0].split()[1:]], "offsetof": [int(v) for v in keys[1].split()[1:]]}
    for line in keys[2:]:
        dump[FN_NAMES[int(line.split()[0])]] = line.split()[1:]
    # public_names() looks for "class <export marker> <name>"; this class is declared without a marker
    header = open(os.path.join(reference, "include", "lsp-plug.in", "dsp-units", "util", "ADSREnvelope.h")).read()
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "marked.h"), "w") as f:
            f.write(header.replace("class ADSREnvelope", "class MARKER ADSREnvelope"))
        names = {"util/ADSREnvelope.h": public_names(os.path.join(d, "marked.h"), "ADSREnvelope")}
    return x, cs, got, dump, names


def build(reference):
    x, cs, got, dump, names = run_reference(reference)
    arrs = {"x": x, "names": np.array([c["name"] for c in cs]), "kind": np.array([c["kind"] for c in cs], np.uint32),
            "n": np.array([c["n"] for c in cs], np.uint32), "first": np.array([c["count"] - c["n"] for c in cs], np.uint32),
            "tsig": np.array([c["tsig"] for c in cs], np.int32), "dsig": np.array([c["dsig"] for c in cs], np.int32),
            "start": np.array([c["start"] for c in cs], f32), "step": np.array([c["step"] for c in cs], f32),
            "ops_n": np.array([len(c["ops"]) for c in cs], np.uint32), "ops": np.concatenate([c["ops"].reshape(-1, 4) for c in cs]),
            "out": np.concatenate([r["out"] for r in got]), "record": np.stack([r["record"] for r in got]),
            "flags_before": np.array([r["flags_before"] for r in got], np.int64)}
    return npz_bytes(arrs), dump, names


def load(path=OUT):
    """The stored file as (x, cases): dicts of name, kind, n, first, tsig, dsig, start, step, ops, out, record, flags_before."""
    z = np.load(path)
    count = len(z["names"])
    cs = [dict(name=str(z["names"][i]), kind=int(z["kind"][i]), n=int(z["n"][i]), first=int(z["first"][i]), tsig=int(z["tsig"][i]),
               dsig=int(z["dsig"][i]), start=z["start"][i], step=z["step"][i], record=z["record"][i], flags_before=int(z["flags_before"][i]))
          for i in range(count)]
    for key, lengths in (("ops", z["ops_n"]), ("out", z["n"])):
        off = np.concatenate([[0], np.cumsum(lengths.astype(np.int64))])
        for i in range(count):
            cs[i][key] = z[key][off[i]:off[i + 1]]
    return z["x"], cs


if __name__ == "__main__":
    data, dump, names = build(sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(ROOT), "reference"))
    with open(OUT, "wb") as f:
        f.write(data)
    with open(os.path.join(HERE, "adsr_dump_keys.json"), "w") as f:
        json.dump(dump, f, indent=1)
        f.write("\n")
    with open(os.path.join(HERE, "adsr_public_names.json"), "w") as f:
        json.dump(names, f, indent=1)
        f.write("\n")
    print("%d cases, %d bytes" % (len(load()[1]), len(data)))
