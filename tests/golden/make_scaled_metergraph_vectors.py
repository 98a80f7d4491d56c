"""Writes tests/golden/scaled_metergraph_ref_vectors.npz, scaled_metergraph_dump_keys.json and scaled_metergraph_public_names.json:
what the reference's own ScaledMeterGraph class leaves in its two rings and its state on a list of cases.  Data only: inputs,
operation lists, and after every operation both rings' words, both heads, both samplers' fCurrent, nCount and nPeriod and the
target nPeriod, plus what read() and level() returned.  Run where the reference tree exists:

    python tests/golden/make_scaled_metergraph_vectors.py [reference tree]

util/ScaledMeterGraph.cpp, util/RawRingBuffer.cpp and iface/IStateDumper.cpp are compiled unmodified into a temporary directory
(-O2 -ffp-contract=off -msse2 -mfpmath=sse) against oracle/ref_shim.  What the reference tree does not carry comes from a header of
this project's own text that is written to that directory and passed with -include: make_metergraph_vectors.py's PRIMITIVES
(dsp::abs_max, abs_min, sign_max, sign_min as DESIGN.md 3.30 defines them) and PRELUDE below (the lsp_min overload of a size_t
and a uint32_t).  The program -- a stand-alone one with its own main -- is built a first time with
-fsanitize=address,undefined and run on every case before anything is recorded.

The file holds the input rows (x: [rows, N]) and case by case: names, frames, subsampling, max_period, ops [k, 5] float64 (code as
tests/scaled_metergraph_ref.py has it, row of x, offset, n or the setter's integer, the float argument), state [k, history
capacity + frame capacity + 9] uint32 (scaled_metergraph_ref.ScaledMeterGraph.state_words after each operation) and answers (what
the READ and LEVEL operations returned, in order).  No case is one of those where the reference is undefined."""
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
import make_metergraph_vectors as mg  # noqa: E402
import scaled_metergraph_ref as M  # noqa: E402

OUT = os.path.join(HERE, "scaled_metergraph_ref_vectors.npz")
f32, u32 = np.float32, np.uint32
N = mg.N
ROW_RANDOM, ROW_TIES, ROW_SPECIAL, ROW_NAN, ROW_SENTINEL = range(5)

PRELUDE = r'''
// lsp_min of a size_t and a uint32_t (ScaledMeterGraph.cpp:152, :214, :367), which the stand-in for common/types.h has as one
// template only
namespace lsp
{
    inline size_t lsp_min(size_t a, uint32_t b) { return (a < b) ? a : b; }
}
'''

# reads the rows and the cases, runs the class, writes the state after every operation; with "keys" as its only argument it prints
# sizeof and offsetof of the class and what dump() writes
DRIVER = r'''
#define private public
#define protected public
#include <lsp-plug.in/dsp-units/util/ScaledMeterGraph.h>
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
typedef dspu::ScaledMeterGraph G;
struct open_graph: public G { typedef G::sampler_t sampler; };
int main(int argc, char **argv)
{
    if (argc == 2 && strcmp(argv[1], "keys") == 0)
    {
        printf("sizeof %zu %zu %zu\n", sizeof(G), sizeof(dspu::RawRingBuffer), sizeof(open_graph::sampler));
        printf("offsetof %zu %zu %zu %zu %zu\n", offsetof(G, sHistory), offsetof(G, sFrames), offsetof(G, nPeriod), offsetof(G, nMaxPeriod),
               offsetof(G, enMethod));
        printf("sampler %zu %zu %zu %zu %zu\n", offsetof(open_graph::sampler, sBuffer), offsetof(open_graph::sampler, fCurrent),
               offsetof(open_graph::sampler, nCount), offsetof(open_graph::sampler, nPeriod), offsetof(open_graph::sampler, nFrames));
        G g;
        g.init(16, 4, 64);
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
        uint32_t q[4];                          // frames, subsampling, max_period, ops
        if (fread(q, 4, 4, f) != 4) return 3;
        std::vector<double> ops(5 * size_t(q[3]));
        if (fread(ops.data(), 8, ops.size(), f) != ops.size()) return 3;
        G g;
        if (!g.init(q[0], q[1], q[2])) return 4;
        for (size_t j = 0; j < q[3]; ++j)
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
                case 2: g.fill(v); break;
                case 3: { std::vector<float> t(s, s + n); g.process(t.data(), n); break; }      // a copy of its own: the
                case 4: { std::vector<float> t(s, s + n); g.process(t.data(), v, n); break; }   // sanitizer sees the call's ends
                case 5: for (size_t i = 0; i < n; ++i) g.process(s[i]); break;
                case 6: answer.assign(n + 1, -77.0f); g.read(answer.data(), n); answer.resize(n); break;   // never a NULL dst
                case 7: answer.assign(1, g.level()); break;
                default: return 6;
            }
            const size_t ch = g.sHistory.sBuffer.nCapacity, cf = g.sFrames.sBuffer.nCapacity;
            std::vector<uint32_t> w(ch + cf + 9);
            memcpy(w.data(), g.sHistory.sBuffer.pData, 4 * ch);
            memcpy(w.data() + ch, g.sFrames.sBuffer.pData, 4 * cf);
            uint32_t *t = w.data() + ch + cf;
            t[0] = uint32_t(g.sHistory.sBuffer.nHead), t[1] = uint32_t(g.sFrames.sBuffer.nHead);
            t[2] = bits(g.sHistory.fCurrent), t[3] = g.sHistory.nCount, t[4] = g.sHistory.nPeriod;
            t[5] = bits(g.sFrames.fCurrent), t[6] = g.sFrames.nCount, t[7] = g.sFrames.nPeriod, t[8] = g.nPeriod;
            fwrite(w.data(), 4, w.size(), o);
            if (!answer.empty())
                fwrite(answer.data(), 4, answer.size(), o);
        }
    }
    fclose(f);
    return fclose(o) == 0 ? 0 : 8;
}
'''

REF_SOURCES = ("util/ScaledMeterGraph.cpp", "util/RawRingBuffer.cpp", "iface/IStateDumper.cpp")


def rows():
    x = np.zeros((5, N), f32)
    x[:4] = mg.rows()
    # history words that the sentinel of update_period() meets: negative ones, exactly -1.0f, zeros of both signs
    rng = np.random.default_rng(3131)
    x[ROW_SENTINEL] = rng.choice(np.array([-1.0, -1.0, -0.0, 0.0, -0.5, 0.5, -2.0, 2.0, 1.0, -0.25, 3.0, -3.0], f32), N)
    x[ROW_SENTINEL, :12] = [-1.0, 0.5, -0.0, -2.0, -1.0, -1.0, 0.25, -0.0, 0.0, -3.0, 2.0, -1.0]
    return x


def capacities(c):
    sub = M.subframes(c["frames"], c["subsampling"], c["max_period"])
    return sub + M.FRAMES_GAP, c["frames"] + M.FRAMES_GAP


def cases():
    out = []

    def add(name, frames, subsampling, max_period, ops):
        rows5 = np.zeros((len(ops), 5))
        for i, op in enumerate(ops):
            rows5[i, :len(op)] = [float(v) for v in op]
        out.append(dict(name=name, frames=frames, subsampling=subsampling, max_period=max_period, ops=rows5))

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

    def fill(v):
        return (M.FILL, 0, 0, 0, v)

    def cut(row, total, step, make=block, at=0):
        return [make(row, o, min(step, at + total - o)) for o in range(at, at + total, step)]

    kinds = ((ROW_RANDOM, "random"), (ROW_TIES, "ties"), (ROW_SPECIAL, "special"), (ROW_NAN, "nan"))
    reads = [(M.READ, 0, 0, n) for n in (0, 1, 16, 21)] + [(M.LEVEL,)]
    for m in range(5):
        name = M.METHOD_NAMES[m]
        # the three forms, every gain, every kind of row; a period that is no multiple of the subsampling, one that is
        for row, rname in kinds:
            add("%s block %s 4 to 7" % (name, rname), 16, 4, 64, [method(m), period(7)] + cut(row, 600, 100))
            add("%s block %s 4 to 64" % (name, rname), 16, 4, 64, [method(m), period(64)] + cut(row, 1000, 333))
            add("%s single %s 4 to 7" % (name, rname), 16, 4, 64, [method(m), period(7)] + cut(row, 220, 110, single))
            for g in (1.0, 0.5, -2.0, 0.0):
                add("%s gain %g %s 3 to 10" % (name, g, rname), 16, 3, 10,
                    [method(m), period(10)] + cut(row, 400, 150, lambda r, o, n: gained(r, o, n, g)) + [period(5), gained(row, 400, 7, g)])
        # every subsampling; a period equal to it; max_period == subsampling
        add("%s subsampling 1 period 1" % name, 16, 1, 1, [method(m), period(1)] + cut(ROW_RANDOM, 100, 37) + [single(ROW_TIES, 0, 5)])
        add("%s subsampling 3 period 3" % name, 16, 3, 9, [method(m), period(3)] + cut(ROW_RANDOM, 200, 77) + [period(9), block(ROW_RANDOM, 200, 50)])
        add("%s subsampling 64" % name, 16, 64, 192, [method(m), period(64)] + cut(ROW_RANDOM, 1500, 700) + [period(128), block(ROW_RANDOM, 1500, 900),
                                                      period(191), block(ROW_NAN, 0, 1000), period(64), gained(ROW_NAN, 1000, 500, -2.0)])
        add("%s subsampling 64 max 64" % name, 2, 64, 64, [method(m), period(1), block(ROW_TIES, 0, 300), period(1000), block(ROW_TIES, 300, 300)])
        # 4 -> 7, 10, 64 and back, in mid-stream
        add("%s 4 to 7 10 64" % name, 16, 4, 64,
            [method(m), period(4), block(ROW_RANDOM, 0, 131), period(7), block(ROW_RANDOM, 131, 100), period(10), block(ROW_RANDOM, 231, 333),
             period(64), block(ROW_RANDOM, 564, 700), period(4), block(ROW_RANDOM, 1264, 5), single(ROW_RANDOM, 1269, 9)])
        # the same stream cut at 1, 7, 256 samples and in one call
        for step in (1, 7, 256, 260):
            add("%s cut at %d" % (name, step), 16, 4, 20, [method(m), period(20)] + cut(ROW_TIES, 260, step))
        add("%s cut at 7 random" % name, 16, 4, 20, [method(m), period(20)] + cut(ROW_RANDOM, 260, 7))
        add("%s one call random" % name, 16, 4, 20, [method(m), period(20), block(ROW_RANDOM, 0, 260)])
        # the three forms in turn inside a frame
        add("%s forms in turn" % name, 16, 4, 64, [method(m), period(50), block(ROW_RANDOM, 0, 30), single(ROW_RANDOM, 30, 5), gained(ROW_RANDOM, 35, 40, -2.0),
                                                   single(ROW_RANDOM, 75, 30), block(ROW_RANDOM, 105, 95), gained(ROW_RANDOM, 200, 7, 0.5),
                                                   block(ROW_RANDOM, 207, 300)])
        # period changes in mid-stream: up, down, the same again, clamped below and above; with the history's frame open (50 % 4),
        # with only the frames' frame open (80 % 4 == 0, 80 % 8 == 2, then 128 + 4 against 12), with both closed (96 + 96), before
        # the history has filled, straight after fill(), and through the single-sample form
        add("%s period changes" % name, 16, 4, 64,
            [method(m), period(8), block(ROW_RANDOM, 0, 50), period(16), block(ROW_RANDOM, 50, 30), period(16), block(ROW_RANDOM, 80, 16),
             period(12), block(ROW_RANDOM, 96, 96), period(12), block(ROW_RANDOM, 192, 32), period(8), block(ROW_RANDOM, 224, 4),
             period(2), block(ROW_RANDOM, 228, 41), period(1000), gained(ROW_RANDOM, 269, 700, -2.0), period(9), single(ROW_RANDOM, 969, 3),
             fill(0.75), period(5), block(ROW_RANDOM, 972, 10), fill(-0.5), block(ROW_RANDOM, 982, 30), period(24), block(ROW_SPECIAL, 0, 100),
             period(7), single(ROW_SPECIAL, 100, 50)] + reads)
        # the sentinel: history words that are negative, -1.0f, +-0 (a subsampling of 1: the words are the samples), NaN as a
        # group's first sub-sample and elsewhere, ABS methods over the negative words of a negative gain
        add("%s sentinel" % name, 16, 1, 8, [method(m), period(1), block(ROW_SENTINEL, 0, 64), period(4), block(ROW_SENTINEL, 64, 3),
                                             period(3), block(ROW_SENTINEL, 67, 30), period(8), single(ROW_SENTINEL, 97, 2), period(2),
                                             block(ROW_SENTINEL, 99, 1)] + reads)
        add("%s sentinel nan" % name, 16, 7, 70, [method(m), period(7), block(ROW_NAN, 0, 700), period(21), block(ROW_NAN, 700, 7),
                                                  period(14), block(ROW_NAN, 707, 1), period(70), block(ROW_NAN, 0, 80)])
        add("%s sentinel negative gain" % name, 16, 4, 32, [method(m), period(4), gained(ROW_RANDOM, 0, 300, -2.0), period(12),
                                                            gained(ROW_RANDOM, 300, 50, -2.0), period(32), gained(ROW_TIES, 0, 7, -2.0)])
        # every frame count; both rings overrun several times in one call
        for frames in (1, 2, 16, 333):
            add("%s frames %d" % (name, frames), frames, 3, 6, [method(m), period(3)] + cut(ROW_RANDOM, 1100, 400) + [(M.READ, 0, 0, frames), (M.LEVEL,),
                                                               period(6), block(ROW_RANDOM, 1100, 100), (M.READ, 0, 0, frames + 5), (M.LEVEL,)])
        add("%s overrun frames 2" % name, 2, 1, 2, [method(m), period(1), block(ROW_RANDOM, 0, 5), block(ROW_RANDOM, 5, N - 5), block(ROW_TIES, 0, 5),
                                                    period(2), block(ROW_SPECIAL, 0, 1000), gained(ROW_RANDOM, 1, 999, -2.0)])
    # set_method inside a frame, and between a period change and the call that acts on it
    ops = [period(30)]
    at = 0
    for m in (M.SIGN_MINIMUM, M.ABS_MAXIMUM, M.PEAK, M.SIGN_MAXIMUM, M.ABS_MINIMUM, 7, M.SIGN_MINIMUM):
        ops += [method(m), block(ROW_RANDOM, at, 13), single(ROW_RANDOM, at + 13, 4)]
        at += 17
    ops += [period(9), method(M.SIGN_MAXIMUM), block(ROW_RANDOM, at, 20), period(17), method(7), block(ROW_RANDOM, at + 20, 20)]
    add("set_method in mid-frame", 16, 3, 30, ops)
    # read, level and fill
    add("read and level", 16, 5, 5, [period(5)] + reads + [block(ROW_RANDOM, 0, 33)] + reads + [block(ROW_RANDOM, 33, 100)] + reads)
    add("fill", 16, 5, 10, [period(5), block(ROW_RANDOM, 0, 33), fill(0.75)] + reads + [block(ROW_RANDOM, 33, 12), fill(-2.5)] + reads +
        [period(10), block(ROW_RANDOM, 45, 60)] + reads)
    add("read one frame", 1, 4, 4, [period(4)] + [(M.READ, 0, 0, n) for n in (0, 1, 6)] + [block(ROW_RANDOM, 0, 9)] + [(M.READ, 0, 0, n) for n in (0, 1, 6)] +
        [(M.LEVEL,)])
    return out


def answer_words(c, op):
    """How many floats an operation's answer has: read() writes min(count, frames), level() one."""
    code = int(op[0])
    return min(int(op[3]), c["frames"]) if code == M.READ else 1 if code == M.LEVEL else 0


def run(exe, x, cs, cwd):
    src, dst = os.path.join(cwd, "cases.bin"), os.path.join(cwd, "results.bin")
    with open(src, "wb") as f:
        f.write(np.array([x.shape[0], x.shape[1], len(cs)], u32).tobytes())
        f.write(x.tobytes())
        for c in cs:
            f.write(np.array([c["frames"], c["subsampling"], c["max_period"], len(c["ops"])], u32).tobytes())
            f.write(c["ops"].astype(np.float64).tobytes())
    subprocess.run([exe, src, dst], check=True, timeout=900)
    raw = np.fromfile(dst, u32)
    got, at = [], 0
    for c in cs:
        w = sum(capacities(c)) + M.STATE_WORDS
        states, answers = [], []
        for op in c["ops"]:
            states.append(raw[at:at + w].copy())
            at += w
            # the driver hands read() a buffer of `count` floats and writes all of it out: what read() left alone is -77
            extra = int(op[3]) if int(op[0]) == M.READ else 1 if int(op[0]) == M.LEVEL else 0
            answers.append(raw[at:at + answer_words(c, op)].copy())
            assert (raw[at + answer_words(c, op):at + extra] == f32(-77.0).view(u32)).all(), (c["name"], "read() wrote past min(count, frames)")
            at += extra
        got.append({"state": np.stack(states), "answers": np.concatenate(answers)})
    assert at == raw.size, (at, raw.size)
    return got


def same(a, b):
    return all(np.array_equal(p["state"], q["state"]) and np.array_equal(p["answers"], q["answers"]) for p, q in zip(a, b))


def compile_driver(reference, d, source, exe, extra=()):
    with open(os.path.join(d, "scaled_meter_primitives.h"), "w") as f:
        f.write(mg.PRIMITIVES + PRELUDE)
    srcs = [source] + [os.path.join(reference, "src", "main", n) for n in REF_SOURCES]
    inc = ["-I" + os.path.join(ROOT, "oracle", "ref_shim"), "-I" + os.path.join(reference, "include"), "-include",
           os.path.join(d, "scaled_meter_primitives.h")]
    subprocess.check_call(["g++"] + mg.FLAGS + list(extra) + inc + ["-o", exe] + srcs + ["-lm"])
    return exe


def run_reference(reference):
    x, cs = rows(), cases()
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "driver.cpp"), "w") as f:
            f.write(DRIVER)
        for exe, extra in (("ref_san", mg.SAN_FLAGS), ("ref", [])):
            compile_driver(reference, d, os.path.join(d, "driver.cpp"), os.path.join(d, exe), extra)
        san = run(os.path.join(d, "ref_san"), x, cs, d)                     # stand-alone, before anything is recorded
        got = run(os.path.join(d, "ref"), x, cs, d)
        keys = subprocess.check_output([os.path.join(d, "ref"), "keys"]).decode().splitlines()
    assert same(got, san)
    dump = {"sizeof": [int(v) for v in keys[0].split()[1:]], "offsetof": [int(v) for v in keys[1].split()[1:]],
            "sampler": [int(v) for v in keys[2].split()[1:]], "dump": keys[3].split()[1:]}
    header = os.path.join(reference, "include", "lsp-plug.in", "dsp-units", "util", "ScaledMeterGraph.h")
    names = {"util/ScaledMeterGraph.h": public_names(header, "ScaledMeterGraph")}
    return x, cs, got, dump, names


def build(reference):
    x, cs, got, dump, names = run_reference(reference)
    arrs = {"x": x, "names": np.array([c["name"] for c in cs]), "frames": np.array([c["frames"] for c in cs], u32),
            "subsampling": np.array([c["subsampling"] for c in cs], u32), "max_period": np.array([c["max_period"] for c in cs], u32),
            "ops_n": np.array([len(c["ops"]) for c in cs], u32), "ops": np.concatenate([c["ops"] for c in cs]),
            "state": np.concatenate([r["state"].reshape(-1) for r in got]), "answers_n": np.array([len(r["answers"]) for r in got], u32),
            "answers": np.concatenate([r["answers"] for r in got])}
    return npz_bytes(arrs), dump, names


def load(path=OUT):
    """The stored file as (x, cases): dicts of name, frames, subsampling, max_period, ops, state [k, words], answers."""
    z = np.load(path)
    count = len(z["names"])
    cs = [dict(name=str(z["names"][i]), frames=int(z["frames"][i]), subsampling=int(z["subsampling"][i]), max_period=int(z["max_period"][i]))
          for i in range(count)]
    words = np.array([sum(capacities(c)) + M.STATE_WORDS for c in cs], np.int64)
    ops_off = np.concatenate([[0], np.cumsum(z["ops_n"].astype(np.int64))])
    st_off = np.concatenate([[0], np.cumsum(z["ops_n"].astype(np.int64) * words)])
    an_off = np.concatenate([[0], np.cumsum(z["answers_n"].astype(np.int64))])
    for i, c in enumerate(cs):
        c.update(ops=z["ops"][ops_off[i]:ops_off[i + 1]], state=z["state"][st_off[i]:st_off[i + 1]].reshape(-1, words[i]),
                 answers=z["answers"][an_off[i]:an_off[i + 1]])
    return z["x"], cs


if __name__ == "__main__":
    data, dump, names = build(sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(ROOT), "reference"))
    with open(OUT, "wb") as f:
        f.write(data)
    with open(os.path.join(HERE, "scaled_metergraph_dump_keys.json"), "w") as f:
        json.dump(dump, f, indent=1)
        f.write("\n")
    with open(os.path.join(HERE, "scaled_metergraph_public_names.json"), "w") as f:
        json.dump(names, f, indent=1)
        f.write("\n")
    print("%d cases, %d bytes" % (len(load()[1]), len(data)))
