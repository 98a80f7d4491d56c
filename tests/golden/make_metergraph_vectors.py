"""Writes tests/golden/metergraph_ref_vectors.npz, metergraph_dump_keys.json and metergraph_public_names.json: what the reference's
own MeterGraph class leaves in its ring and its state on a list of cases.  Data only: inputs, operation lists, and after every
operation the ring's words, nHead, fCurrent and nCount, plus what read() and level() returned.  Run where the reference tree exists:

    python tests/golden/make_metergraph_vectors.py [reference tree]

util/MeterGraph.cpp, util/RingBuffer.cpp and iface/IStateDumper.cpp are compiled unmodified into a temporary directory (-O2
-ffp-contract=off -msse2 -mfpmath=sse) against oracle/ref_shim.  dsp::abs_max, abs_min, sign_max and sign_min, which the reference
tree does not carry, come from a header of this project's own text (PRIMITIVES below, DESIGN.md 3.30's definition) that is written
to that directory and passed with -include.  The program -- a stand-alone one with its own main -- is built a first time with
-fsanitize=address,undefined and run on every case before anything is recorded.

The file holds the input rows (x: [rows, N]) and case by case: names, frames, period, default (bits), ops [k, 5] float64 (code as
tests/metergraph_ref.py has it, row of x, offset, n or the setter's integer, the float argument), state [k, frames + 3] uint32 (the
ring in storage order, nHead, fCurrent, nCount after each operation) and answers (what the READ and LEVEL operations returned, in
order)."""
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
import metergraph_ref as M  # noqa: E402

OUT = os.path.join(HERE, "metergraph_ref_vectors.npz")
f32, u32 = np.float32, np.uint32
N = 4099
ROW_RANDOM, ROW_TIES, ROW_SPECIAL, ROW_NAN = range(4)

PRIMITIVES = r'''
// dsp::abs_max, abs_min, sign_max, sign_min as this project defines them (lsp-dsp-lib's generic ones): see DESIGN.md 3.30
#include <cmath>
#include <cstddef>
#include <cstdint>
namespace lsp
{
    // lsp_min of a uint32_t and a size_t (RingBuffer.cpp:198), which the stand-in for common/types.h has as one template only
    inline size_t lsp_min(uint32_t a, size_t b) { return (a < b) ? a : b; }

    namespace dsp
    {
        inline float abs_max(const float *s, size_t n)
        {
            if (n == 0) return 0.0f;
            float r = fabsf(s[0]);
            for (size_t i = 1; i < n; ++i) { const float v = fabsf(s[i]); if (v > r) r = v; }
            return r;
        }
        inline float abs_min(const float *s, size_t n)
        {
            if (n == 0) return 0.0f;
            float r = fabsf(s[0]);
            for (size_t i = 1; i < n; ++i) { const float v = fabsf(s[i]); if (v < r) r = v; }
            return r;
        }
        inline float sign_max(const float *s, size_t n)
        {
            if (n == 0) return 0.0f;
            float r = s[0], a = fabsf(r);
            for (size_t i = 1; i < n; ++i) { const float v = fabsf(s[i]); if (v > a) { r = s[i]; a = v; } }
            return r;
        }
        inline float sign_min(const float *s, size_t n)
        {
            if (n == 0) return 0.0f;
            float r = s[0], a = fabsf(r);
            for (size_t i = 1; i < n; ++i) { const float v = fabsf(s[i]); if (v < a) { r = s[i]; a = v; } }
            return r;
        }
    }
}
'''

# reads the rows and the cases, runs the class, writes the state after every operation; with "keys" as its only argument it prints
# sizeof and offsetof of the class and what dump() writes
DRIVER = r'''
#define private public
#define protected public
#include <lsp-plug.in/dsp-units/util/MeterGraph.h>
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
static uint32_t bits(float v) { uint32_t u; memcpy(&u, &v, 4); return u; }
typedef dspu::MeterGraph G;
int main(int argc, char **argv)
{
    if (argc == 2 && strcmp(argv[1], "keys") == 0)
    {
        printf("sizeof %zu %zu\n", sizeof(G), sizeof(dspu::RingBuffer));
        printf("offsetof %zu %zu %zu %zu %zu %zu\n", offsetof(G, sBuffer), offsetof(G, fCurrent), offsetof(G, fDefault), offsetof(G, nCount),
               offsetof(G, nPeriod), offsetof(G, enMethod));
        G g;
        g.init(16, 64, 0.5f);
        keys k;
        g.dump(&k);
        printf("dump%s\n", k.seen.c_str());
        return 0;
    }
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb"), *o = fopen(argv[2], "wb");
    if (!f || !o) return 2;
    uint32_t h[3];                              // rows, row length, cases
    if (fread(h, 4, 3, f) != 3) return 3;
    const size_t len = h[1];
    std::vector<float> x(size_t(h[0]) * len);
    if (fread(x.data(), 4, x.size(), f) != x.size()) return 3;
    for (uint32_t c = 0; c < h[2]; ++c)
    {
        uint32_t q[3];                          // frames, period, ops
        float def;
        if (fread(q, 4, 3, f) != 3 || fread(&def, 4, 1, f) != 1) return 3;
        std::vector<double> ops(5 * size_t(q[2]));
        if (fread(ops.data(), 8, ops.size(), f) != ops.size()) return 3;
        G g;
        if (!g.init(q[0], q[1], def)) return 4;
        for (size_t j = 0; j < q[2]; ++j)
        {
            const double *p = &ops[5 * j];
            const size_t n = size_t(p[3]);
            const float *s = &x[size_t(p[1]) * len + size_t(p[2])];
            const float v = float(p[4]);
            std::vector<float> answer;
            switch (int(p[0]))
            {
                case 0: g.set_method(dspu::meter_method_t(int(p[3]))); break;
                case 1: g.set_period(n); break;
                case 2: g.set_default_value(v); break;
                case 3: g.fill(v); break;
                case 4: g.clear(); break;
                case 5: { std::vector<float> t(s, s + n); g.process(t.data(), n); break; }      // a copy of its own: the
                case 6: { std::vector<float> t(s, s + n); g.process(t.data(), v, n); break; }   // sanitizer sees the call's ends
                case 7: for (size_t i = 0; i < n; ++i) g.process(s[i]); break;
                case 8: answer.assign(n, -77.0f); g.read(answer.data(), n); break;
                case 9: answer.assign(1, g.level()); break;
                default: return 6;
            }
            std::vector<uint32_t> w(q[0] + 3);
            memcpy(w.data(), g.sBuffer.pData, 4 * size_t(q[0]));
            w[q[0]] = g.sBuffer.nHead, w[q[0] + 1] = bits(g.fCurrent), w[q[0] + 2] = g.nCount;
            fwrite(w.data(), 4, w.size(), o);
            if (!answer.empty())
                fwrite(answer.data(), 4, answer.size(), o);
        }
    }
    fclose(f);
    return fclose(o) == 0 ? 0 : 8;
}
'''

FLAGS = ["-std=c++11", "-O2", "-ffp-contract=off", "-msse2", "-mfpmath=sse", "-DLSP_DSP_UNITS_BUILTIN", "-Wall"]
SAN_FLAGS = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
REF_SOURCES = ("util/MeterGraph.cpp", "util/RingBuffer.cpp", "iface/IStateDumper.cpp")


def rows():
    rng = np.random.default_rng(3030)
    x = np.zeros((4, N), f32)
    x[ROW_RANDOM] = rng.standard_normal(N).astype(f32)
    # few distinct magnitudes, both signs: ties in every frame
    x[ROW_TIES] = (rng.integers(-3, 4, N) * 0.25).astype(f32)
    # +-0, equal magnitudes of opposite sign, subnormals, +-Inf among ordinary values; finite but for the two Infs
    sp = rng.standard_normal(N).astype(f32)
    sp[0:8] = [0.0, -0.0, 0.5, -0.5, 1e-45, -1e-45, 1e-39, -1e-39]
    sp[8:16] = [-0.5, 0.5, -0.0, 0.0, 2.0, -2.0, 2.0, 1e-40]
    sp[40], sp[41] = np.inf, -np.inf
    sp[70:77] = [-3.0, 3.0, -3.0, 1e-38, -1e-38, 0.0, -0.0]
    sp[200:264] = 0.0
    sp[264:328] = -0.0
    x[ROW_SPECIAL] = sp
    # NaN in the first place of a chunk (for the periods 7 and 64 from offset 0) and in later places
    na = rng.standard_normal(N).astype(f32)
    na[[0, 3, 7 * 5, 7 * 9 + 2, 64, 64 * 3 + 10, 64 * 5, 64 * 5 + 1, 500, 501, 502]] = np.nan
    na[64 * 7:64 * 8] = np.nan
    x[ROW_NAN] = na
    return x


def cases():
    out = []

    def add(name, frames, period, ops, default=0.0):
        rows5 = np.zeros((len(ops), 5))
        for i, op in enumerate(ops):
            rows5[i, :len(op)] = [float(v) for v in op]
        out.append(dict(name=name, frames=frames, period=period, default=f32(default), ops=rows5))

    def method(m):
        return (M.SET_METHOD, 0, 0, m)

    def period(p):
        return (M.SET_PERIOD, 0, 0, p)

    def block(row, off, n):
        return (M.PROCESS, row, off, n)

    def gained(row, off, n, g):
        return (M.PROCESS_GAIN, row, off, n, g)

    def single(row, off, n):
        return (M.PROCESS_SINGLE, row, off, n)

    def cut(row, total, step, make=block, at=0):
        return [make(row, o, min(step, at + total - o)) for o in range(at, at + total, step)]

    for m in range(5):
        name = M.METHOD_NAMES[m]
        # the three forms, every gain, every kind of row
        for row, rname in ((ROW_RANDOM, "random"), (ROW_TIES, "ties"), (ROW_SPECIAL, "special"), (ROW_NAN, "nan")):
            add("%s block %s period 7" % (name, rname), 16, 7, [method(m)] + cut(row, 600, 100))
            add("%s block %s period 64" % (name, rname), 16, 64, [method(m)] + cut(row, 1000, 333))
            add("%s single %s period 7" % (name, rname), 16, 7, [method(m)] + cut(row, 330, 110, single))
            for g in (1.0, 0.5, -2.0, 0.0):
                add("%s gain %g %s period 7" % (name, g, rname), 16, 7, [method(m)] + cut(row, 400, 150, lambda r, o, n: gained(r, o, n, g)))
        # the same stream cut at 1, 7, 256 samples and in one call
        for step in (1, 7, 256, 520):
            add("%s cut at %d" % (name, step), 16, 20, [method(m)] + cut(ROW_TIES, 520, step))
        add("%s cut at 7 random" % name, 16, 20, [method(m)] + cut(ROW_RANDOM, 520, 7))
        add("%s one call random" % name, 16, 20, [method(m), block(ROW_RANDOM, 0, 520)])
        # the three forms in turn inside frames
        add("%s forms in turn" % name, 16, 50, [method(m), block(ROW_RANDOM, 0, 30), single(ROW_RANDOM, 30, 5), gained(ROW_RANDOM, 35, 40, -2.0),
                                                single(ROW_RANDOM, 75, 30), block(ROW_RANDOM, 105, 95), gained(ROW_RANDOM, 200, 7, 0.5),
                                                block(ROW_RANDOM, 207, 300)])
        # set_period down and up in mid-stream: nCount == nPeriod, nCount > nPeriod, and back
        add("%s set_period" % name, 16, 100,
            [method(m), block(ROW_RANDOM, 0, 60), period(60), block(ROW_RANDOM, 60, 50), period(100), block(ROW_RANDOM, 110, 30),
             period(10), block(ROW_RANDOM, 140, 25), period(7), block(ROW_RANDOM, 165, 3), period(3), block(ROW_RANDOM, 168, 1),
             period(200), block(ROW_RANDOM, 169, 150), period(150), single(ROW_RANDOM, 319, 2), period(40), gained(ROW_RANDOM, 321, 100, 0.5),
             block(ROW_RANDOM, 421, 39), period(39), block(ROW_RANDOM, 460, 200)])
        # every frame count; a ring overrun several times in one call
        for frames in (1, 2, 16, 333):
            add("%s frames %d" % (name, frames), frames, 3, [method(m)] + cut(ROW_RANDOM, 1100, 400) + [(M.READ, 0, 0, frames), (M.LEVEL,)])
        add("%s overrun period 1 frames 2" % name, 2, 1, [method(m), block(ROW_RANDOM, 0, N), block(ROW_TIES, 0, 5)])
        add("%s overrun period 2 frames 16" % name, 16, 2, [method(m), block(ROW_SPECIAL, 0, 1000), gained(ROW_RANDOM, 1, 999, -2.0)])
    # set_method inside a frame
    ops = []
    at = 0
    for m in (M.SIGN_MINIMUM, M.ABS_MAXIMUM, M.PEAK, M.SIGN_MAXIMUM, M.ABS_MINIMUM, 7, M.SIGN_MINIMUM):
        ops += [method(m), block(ROW_RANDOM, at, 13), single(ROW_RANDOM, at + 13, 4)]
        at += 17
    add("set_method in mid-frame", 16, 30, ops)
    # read, level, fill and clear
    reads = [(M.READ, 0, 0, n) for n in (0, 1, 16, 21)] + [(M.LEVEL,)]
    add("read and level", 16, 5, reads + [block(ROW_RANDOM, 0, 33)] + reads + [block(ROW_RANDOM, 33, 100)] + reads, default=-1.5)
    add("fill and clear", 16, 5, [block(ROW_RANDOM, 0, 33), (M.FILL, 0, 0, 0, 0.75)] + reads + [block(ROW_RANDOM, 33, 12), (M.SET_DEFAULT, 0, 0, 0, 2.5),
                                  (M.CLEAR,)] + reads + [block(ROW_RANDOM, 45, 60)] + reads, default=-1.5)
    add("read one frame", 1, 4, [(M.READ, 0, 0, n) for n in (0, 1, 6)] + [block(ROW_RANDOM, 0, 9)] + [(M.READ, 0, 0, n) for n in (0, 1, 6)] + [(M.LEVEL,)],
        default=3.0)
    return out


def run(exe, x, cs, cwd):
    src, dst = os.path.join(cwd, "cases.bin"), os.path.join(cwd, "results.bin")
    with open(src, "wb") as f:
        f.write(np.array([x.shape[0], x.shape[1], len(cs)], u32).tobytes())
        f.write(x.tobytes())
        for c in cs:
            f.write(np.array([c["frames"], c["period"], len(c["ops"])], u32).tobytes())
            f.write(np.array([c["default"]], f32).tobytes())
            f.write(c["ops"].astype(np.float64).tobytes())
    subprocess.run([exe, src, dst], check=True, timeout=900)
    raw = np.fromfile(dst, u32)
    got, at = [], 0
    for c in cs:
        w = c["frames"] + 3
        states, answers = [], []
        for op in c["ops"]:
            states.append(raw[at:at + w].copy())
            at += w
            extra = int(op[3]) if int(op[0]) == M.READ else 1 if int(op[0]) == M.LEVEL else 0
            answers.append(raw[at:at + extra].copy())
            at += extra
        got.append({"state": np.stack(states), "answers": np.concatenate(answers)})
    assert at == raw.size, (at, raw.size)
    return got


def same(a, b):
    return all(np.array_equal(p["state"], q["state"]) and np.array_equal(p["answers"], q["answers"]) for p, q in zip(a, b))


def compile_driver(reference, d, source, exe, extra=()):
    with open(os.path.join(d, "meter_primitives.h"), "w") as f:
        f.write(PRIMITIVES)
    srcs = [source] + [os.path.join(reference, "src", "main", n) for n in REF_SOURCES]
    inc = ["-I" + os.path.join(ROOT, "oracle", "ref_shim"), "-I" + os.path.join(reference, "include"), "-include", os.path.join(d, "meter_primitives.h")]
    subprocess.check_call(["g++"] + FLAGS + list(extra) + inc + ["-o", exe] + srcs + ["-lm"])
    return exe


def run_reference(reference):
    x, cs = rows(), cases()
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "driver.cpp"), "w") as f:
            f.write(DRIVER)
        for exe, extra in (("ref_san", SAN_FLAGS), ("ref", [])):
            compile_driver(reference, d, os.path.join(d, "driver.cpp"), os.path.join(d, exe), extra)
        san = run(os.path.join(d, "ref_san"), x, cs, d)                     # stand-alone, before anything is recorded
        got = run(os.path.join(d, "ref"), x, cs, d)
        keys = subprocess.check_output([os.path.join(d, "ref"), "keys"]).decode().splitlines()
    assert same(got, san)
    dump = {"sizeof": [int(v) for v in keys[0].split()[1:]], "offsetof": [int(v) for v in keys[1].split()[1:]], "dump": keys[2].split()[1:]}
    names = {"util/MeterGraph.h": public_names(os.path.join(reference, "include", "lsp-plug.in", "dsp-units", "util", "MeterGraph.h"), "MeterGraph")}
    return x, cs, got, dump, names


def build(reference):
    x, cs, got, dump, names = run_reference(reference)
    arrs = {"x": x, "names": np.array([c["name"] for c in cs]), "frames": np.array([c["frames"] for c in cs], u32),
            "period": np.array([c["period"] for c in cs], u32), "default": np.array([c["default"] for c in cs], f32),
            "ops_n": np.array([len(c["ops"]) for c in cs], u32), "ops": np.concatenate([c["ops"] for c in cs]),
            "state": np.concatenate([r["state"].reshape(-1) for r in got]), "answers_n": np.array([len(r["answers"]) for r in got], u32),
            "answers": np.concatenate([r["answers"] for r in got])}
    return npz_bytes(arrs), dump, names


def load(path=OUT):
    """The stored file as (x, cases): dicts of name, frames, period, default, ops, state [k, frames + 3], answers."""
    z = np.load(path)
    count = len(z["names"])
    ops_off = np.concatenate([[0], np.cumsum(z["ops_n"].astype(np.int64))])
    st_off = np.concatenate([[0], np.cumsum(z["ops_n"].astype(np.int64) * (z["frames"].astype(np.int64) + 3))])
    an_off = np.concatenate([[0], np.cumsum(z["answers_n"].astype(np.int64))])
    cs = []
    for i in range(count):
        frames = int(z["frames"][i])
        cs.append(dict(name=str(z["names"][i]), frames=frames, period=int(z["period"][i]), default=z["default"][i],
                       ops=z["ops"][ops_off[i]:ops_off[i + 1]], state=z["state"][st_off[i]:st_off[i + 1]].reshape(-1, frames + 3),
                       answers=z["answers"][an_off[i]:an_off[i + 1]]))
    return z["x"], cs


if __name__ == "__main__":
    data, dump, names = build(sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(ROOT), "reference"))
    with open(OUT, "wb") as f:
        f.write(data)
    with open(os.path.join(HERE, "metergraph_dump_keys.json"), "w") as f:
        json.dump(dump, f, indent=1)
        f.write("\n")
    with open(os.path.join(HERE, "metergraph_public_names.json"), "w") as f:
        json.dump(names, f, indent=1)
        f.write("\n")
    print("%d cases, %d bytes" % (len(load()[1]), len(data)))
