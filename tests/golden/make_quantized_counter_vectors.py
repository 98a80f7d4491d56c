"""Writes tests/golden/quantized_counter_ref_vectors.npz, quantized_counter_dump_keys.json and quantized_counter_public_names.json:
what the reference's own QuantizedCounter class leaves in its counters, its ring and its state on a list of cases.  Data only:
inputs, operation lists, after every operation the nMaxLevels + 2 counters and eight state words, and the ring after the last.
Run where the reference tree exists:

    python tests/golden/make_quantized_counter_vectors.py [reference tree]

stat/QuantizedCounter.cpp and iface/IStateDumper.cpp are compiled unmodified into a temporary directory (-O2 -ffp-contract=off
-msse2 -mfpmath=sse) against oracle/ref_shim.  The four names that the shim lacks (align_size, advance_ptr_bytes, STATUS_NO_MEM and
lsp_min of a size_t and a uint32_t) come from a header of this project's own text (PRELUDE below) that is written to that directory
and passed with -include.  The program -- a stand-alone one with its own main -- is built a first time with
-fsanitize=address,undefined and run on every case before anything is recorded.

The driver feeds every PROCESS operation in pieces of at most nCapacity - nPeriod samples: there the reference IS the histogram of
the last min(nPeriod, samples seen) samples.  A single longer call corrupts its window (the copy overwrites samples that are not
evicted yet); the one case whose name starts with DEFECT records such a call (PROCESS_WHOLE) so that the claim is pinned.  The cases
whose names start with "x86 conversion" hold samples whose conversion to int32_t is undefined in C++: what is recorded for them is
what the compiled class does on x86-64 (float-cast-overflow is not part of -fsanitize=undefined, so they run clean), and the bank
defines the case that way.

The file holds the input rows (x: [rows, N]) and case by case: names, max_period, max_levels, ops [k, 6] float64 (code as
tests/quantized_counter_ref.py has it, row of x, offset, n or the setter's integer, two float arguments), words [k, max_levels + 10]
uint32 (the counters, nHead, nCount, nPeriod, nLevels, fMinValue, fMaxValue, fRStep, bUpdate after each operation) and ring
[nCapacity] uint32 (after the last)."""
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_bypass_crossfade_vectors import npz_bytes  # noqa: E402
import quantized_counter_ref as Q  # noqa: E402

OUT = os.path.join(HERE, "quantized_counter_ref_vectors.npz")
f32, u32 = np.float32, np.uint32
N = 4100
ROW_UNIFORM, ROW_SPECIAL, ROW_EDGES, ROW_SUBNORMAL, ROW_CONSTANT, ROW_TWO, ROW_SORTED, ROW_SINE = range(8)
SPECIALS = [np.nan, np.inf, -np.inf, 1e30, -1e30, -1.05, -1.2, -1.25, -1.26, 1.0, 0.999999, -0.0, 7.5e8, 5.4e8]
DEFECT, X86 = "DEFECT", "x86 conversion"

PRELUDE = r'''
// what stat/QuantizedCounter.cpp takes from lsp-common-lib and the stand-in headers do not carry
#include <cstddef>
#include <cstdint>
namespace lsp
{
    enum { STATUS_NO_MEM = 5 };
    inline size_t align_size(size_t size, size_t align)     { const size_t off = size % align; return (off == 0) ? size : size + align - off; }
    template <class T> inline T *advance_ptr_bytes(uint8_t * &ptr, size_t bytes)
    {
        T *res = reinterpret_cast<T *>(ptr);
        ptr += bytes;
        return res;
    }
    inline size_t lsp_min(size_t a, uint32_t b)              { return (a < b) ? a : b; }
}
'''

# reads the rows and the cases, runs the class, writes the words after every operation and the ring after the last; with "keys" as
# its only argument it prints sizeof and offsetof of the class and what dump() writes
DRIVER = r'''
#define private public
#define protected public
#include <lsp-plug.in/dsp-units/stat/QuantizedCounter.h>
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
typedef dspu::QuantizedCounter C;
int main(int argc, char **argv)
{
    if (argc == 2 && strcmp(argv[1], "keys") == 0)
    {
        printf("sizeof %zu\n", sizeof(C));
        printf("offsetof %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", offsetof(C, nPeriod), offsetof(C, nLevels), offsetof(C, nHead),
               offsetof(C, nCapacity), offsetof(C, nCount), offsetof(C, nMaxPeriod), offsetof(C, nMaxLevels), offsetof(C, fMinValue),
               offsetof(C, fMaxValue), offsetof(C, fRStep), offsetof(C, bUpdate), offsetof(C, vHistory), offsetof(C, vCounters), offsetof(C, pData));
        C c;
        c.init(16, 4);
        keys k;
        c.dump(&k);
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
        uint32_t q[3];                          // max_period, max_levels, ops
        if (fread(q, 4, 3, f) != 3) return 3;
        std::vector<double> ops(6 * size_t(q[2]));
        if (fread(ops.data(), 8, ops.size(), f) != ops.size()) return 3;
        C g;
        if (g.init(q[0], q[1]) != STATUS_OK) return 4;
        for (size_t j = 0; j < q[2]; ++j)
        {
            const double *p = &ops[6 * j];
            const size_t n = size_t(p[3]);
            const float *s = &x[size_t(p[1]) * len + size_t(p[2])];
            const float a = float(p[4]), b = float(p[5]);
            switch (int(p[0]))
            {
                case 0: g.set_period(n); break;
                case 1: g.set_levels(n); break;
                case 2: g.set_min_value(a); break;
                case 3: g.set_max_value(a); break;
                case 4: g.set_value_range(a, b); break;
                case 5: g.set_range(a, b, n); break;
                case 6: g.update_settings(); break;
                case 7: g.clear(); break;
                case 8:                         // in pieces of at most nCapacity - nPeriod, each a copy of its own: the
                {                               // sanitizer sees the call's ends
                    const size_t piece = g.nCapacity - g.nPeriod;
                    size_t at = 0;
                    do
                    {
                        const size_t m = (n - at < piece) ? n - at : piece;
                        std::vector<float> t(s + at, s + at + m);
                        g.process(t.data(), m);
                        at += m;
                    } while (at < n);
                    break;
                }
                case 9: { std::vector<float> t(s, s + n); g.process(t.data(), n); break; }
                default: return 6;
            }
            std::vector<uint32_t> w(q[1] + 10);
            memcpy(w.data(), g.vCounters, 4 * size_t(q[1] + 2));
            uint32_t *t = &w[q[1] + 2];
            t[0] = g.nHead, t[1] = g.nCount, t[2] = g.nPeriod, t[3] = g.nLevels, t[4] = bits(g.fMinValue), t[5] = bits(g.fMaxValue);
            t[6] = bits(g.fRStep), t[7] = g.bUpdate ? 1 : 0;
            fwrite(w.data(), 4, w.size(), o);
        }
        fwrite(g.vHistory, 4, g.nCapacity, o);
    }
    fclose(f);
    return fclose(o) == 0 ? 0 : 8;
}
'''

FLAGS = ["-std=c++11", "-O2", "-ffp-contract=off", "-msse2", "-mfpmath=sse", "-DLSP_DSP_UNITS_BUILTIN", "-Wall"]
SAN_FLAGS = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
REF_SOURCES = ("stat/QuantizedCounter.cpp", "iface/IStateDumper.cpp")


def public_names(path, cls):
    """The names that the class declares in its public sections, in order (make_bypass_crossfade_vectors.public_names for a class
    that is declared without an export marker)."""
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    text = re.sub(r"//.*", "", text)
    body = text[text.index("{", re.search(r"\bclass\s+(\w+\s+)?%s\b" % cls, text).end()):]
    flat, depth = [], 0
    for c in body[1:]:                                      # inline bodies away
        depth += (c == "{") - (c == "}")
        if depth < 0:
            break
        flat.append(c if depth == 0 and c != "}" else ";" if c == "}" else "")
    names, access = [], "private"
    for part in re.split(r"\b(public|protected|private)\s*:", "".join(flat)):
        if part in ("public", "protected", "private"):
            access = part
        elif access == "public":
            for m in re.finditer(r"\b([A-Za-z_]\w*)\s*\(([^)]*)\)", part):
                for n in [m.group(1)] + re.findall(r"\b(I[A-Z]\w*)\b", m.group(2)):
                    if n != "operator" and n not in names:
                        names.append(n)
    return names


def rows():
    rng = np.random.default_rng(3232)
    x = np.zeros((8, N), f32)
    x[ROW_UNIFORM] = rng.uniform(-1.3, 1.3, N).astype(f32)
    sp = rng.uniform(-1.3, 1.3, N).astype(f32)
    sp[:len(SPECIALS)] = np.array(SPECIALS, f32)
    x[ROW_SPECIAL] = sp
    # range [-1, 1] in 8 levels: every bin edge and its two neighbours; the values just under the minimum that truncate into bin 0,
    # min - step exactly (the product is -1: below) and its neighbours
    ed = rng.uniform(-1.3, 1.3, N).astype(f32)
    edges = (f32(-1.0) + np.arange(9, dtype=f32) * f32(0.25)).astype(f32)
    pts = np.concatenate([np.nextafter(edges, f32(-np.inf)), edges, np.nextafter(edges, f32(np.inf))])
    under = np.array([-1.0000001, -1.001, -1.1, -1.2, -1.2499999, -1.25, -1.2500001, -1.3, -2.0], f32)
    under = np.concatenate([under, np.nextafter(f32(-1.25), f32(np.inf), dtype=f32).reshape(1), np.nextafter(f32(-1.25), f32(-np.inf), dtype=f32).reshape(1)])
    ed[:len(pts) + len(under)] = np.concatenate([pts, under])
    x[ROW_EDGES] = ed
    # min 0, max 2.4e-38, 8 levels: the step is about 3.3e38; a flushed difference or product changes the bin
    sn = rng.uniform(-3e-39, 2.6e-38, N).astype(f32)
    sn[:12] = np.array([6e-39, 3e-39, 1e-39, 1.2e-38, 2.3e-38, 2.4e-38, 1e-45, 0.0, -1e-45, -3e-39, -6e-39, 2.9e-39], f32)
    x[ROW_SUBNORMAL] = sn
    x[ROW_CONSTANT] = f32(0.3)
    # two values: runs of 128 samples (half a wave of 16-byte reads), of 4, of 2, then at random
    two = np.where(rng.integers(0, 2, N) == 0, f32(-0.6), f32(0.3)).astype(f32)
    two[:1024] = np.where((np.arange(1024) // 128) % 2 == 0, f32(-0.6), f32(0.3))
    two[1024:1536] = np.where((np.arange(512) // 4) % 2 == 0, f32(-0.6), f32(0.3))
    two[1536:2048] = np.where((np.arange(512) // 2) % 2 == 0, f32(-0.6), f32(0.3))
    x[ROW_TWO] = two
    x[ROW_SORTED] = np.sort(rng.uniform(-1.3, 1.3, N).astype(f32))
    x[ROW_SINE] = (1.1 * np.sin(2 * np.pi * 441.0 / 48000.0 * np.arange(N))).astype(f32)
    return x


def cases():
    out = []

    def add(name, max_period, max_levels, ops):
        rows6 = np.zeros((len(ops), 6))
        for i, op in enumerate(ops):
            rows6[i, :len(op)] = [float(v) for v in op]
        out.append(dict(name=name, max_period=max_period, max_levels=max_levels, ops=rows6))

    def period(p):
        return (Q.SET_PERIOD, 0, 0, p)

    def levels(n):
        return (Q.SET_LEVELS, 0, 0, n)

    def rng(lo, hi, n):
        return (Q.SET_RANGE, 0, 0, n, lo, hi)

    def vrange(lo, hi):
        return (Q.SET_VALUE_RANGE, 0, 0, 0, lo, hi)

    def run(row, off, n):
        return (Q.PROCESS, row, off, n)

    UPDATE, CLEAR = (Q.UPDATE,), (Q.CLEAR,)
    std = [rng(-1.0, 1.0, 8)]

    # ---- the conversion that C++ leaves undefined, as x86-64 has it
    add(X86 + ": the 14 specials", 100, 16, std + [period(100), run(ROW_SPECIAL, 0, 14)])
    add(X86 + ": specials inside a longer row, evicted again", 100, 16, std + [period(100), run(ROW_SPECIAL, 0, 90), run(ROW_UNIFORM, 0, 50),
                                                                              run(ROW_UNIFORM, 50, 60)])
    add(X86 + ": specials recounted under another range", 100, 16, std + [period(100), run(ROW_SPECIAL, 0, 60), vrange(-1e30, 1e30), run(ROW_SPECIAL, 60, 10),
                                                                         rng(-1.0, 1.0, 16), UPDATE])
    add(X86 + ": empty range, every sample below", 100, 16, [rng(0.5, 0.5, 8), period(100), run(ROW_EDGES, 0, 64), run(ROW_CONSTANT, 0, 10)])
    # ---- truncation
    add("truncation at every bin edge", 100, 16, std + [period(100), run(ROW_EDGES, 0, 38)])
    add("truncation, a longer row", 600, 16, std + [period(500), run(ROW_EDGES, 0, 700)])
    # ---- degenerate ranges
    add("reversed range", 100, 16, [rng(1.0, -1.0, 8), period(100), run(ROW_EDGES, 0, 64), run(ROW_UNIFORM, 0, 80)])
    add("one level", 100, 16, [rng(-1.0, 1.0, 1), period(100), run(ROW_EDGES, 0, 64), run(ROW_UNIFORM, 0, 80)])
    add("levels == max_levels", 100, 16, [rng(-1.0, 1.0, 16), period(100), run(ROW_EDGES, 0, 64), run(ROW_UNIFORM, 0, 80)])
    add("levels limited to 1 .. max_levels", 100, 16, [rng(-1.0, 1.0, 100), period(1000), run(ROW_UNIFORM, 0, 150), levels(0), run(ROW_UNIFORM, 150, 30),
                                                        period(0), run(ROW_UNIFORM, 180, 30)])
    add("300 levels", 600, 300, [rng(-1.3, 1.3, 300), period(500), run(ROW_UNIFORM, 0, 700), run(ROW_SINE, 0, 300)])
    # ---- subnormals
    add("subnormal range and samples", 100, 16, [rng(0.0, 2.4e-38, 8), period(100), run(ROW_SUBNORMAL, 0, 64), run(ROW_SUBNORMAL, 64, 80)])
    # ---- period changes
    add("period reduced and raised in mid-stream", 600, 16,
        std + [period(300), run(ROW_UNIFORM, 0, 500), period(100), UPDATE, run(ROW_UNIFORM, 500, 50), period(400), run(ROW_UNIFORM, 550, 600),
               period(7), run(ROW_UNIFORM, 1150, 3), period(600), run(ROW_UNIFORM, 1153, 0), run(ROW_UNIFORM, 1153, 1000)])
    # ---- setter rules
    head = std + [period(300), run(ROW_UNIFORM, 0, 500), period(100)]
    add("range change, update_settings called: the stale window is recounted", 600, 16, head + [vrange(-0.5, 0.5), UPDATE, run(ROW_UNIFORM, 500, 10)])
    add("range change, update_settings left to process", 600, 16, head + [vrange(-0.5, 0.5), run(ROW_UNIFORM, 500, 10)])
    add("setters with unchanged values", 600, 16, head + [vrange(-1.0, 1.0), levels(8), (Q.SET_MIN, 0, 0, 0, -1.0), (Q.SET_MAX, 0, 0, 0, 1.0),
                                                         rng(-1.0, 1.0, 8), run(ROW_UNIFORM, 500, 10)])
    add("a value changed and changed back", 600, 16, head + [(Q.SET_MIN, 0, 0, 0, 0.1), (Q.SET_MIN, 0, 0, 0, -1.0), run(ROW_UNIFORM, 500, 10),
                                                            (Q.SET_MAX, 0, 0, 0, 0.7), UPDATE, levels(5), run(ROW_UNIFORM, 510, 0)])
    add("update_settings before any sample, calls of no samples", 100, 16, std + [period(50), UPDATE, run(ROW_UNIFORM, 0, 0), run(ROW_UNIFORM, 0, 70),
                                                                                 vrange(-2.0, 2.0), run(ROW_UNIFORM, 0, 0)])
    # ---- clear
    add("clear, then more samples: the ring's words survive", 600, 16, std + [period(300), run(ROW_UNIFORM, 0, 500), CLEAR, run(ROW_UNIFORM, 500, 50),
                                                                             vrange(-0.5, 0.5), CLEAR, run(ROW_UNIFORM, 550, 20)])
    # ---- ring wrap: max_period 40, capacity 1072
    add("ring wrap", 40, 16, std + [period(40), run(ROW_UNIFORM, 0, 1071), run(ROW_UNIFORM, 1071, 1), run(ROW_UNIFORM, 1072, 1073), run(ROW_UNIFORM, 2145, 500),
                                    run(ROW_UNIFORM, 2645, 571), run(ROW_UNIFORM, 3216, 1), run(ROW_UNIFORM, 0, 1072), run(ROW_UNIFORM, 0, 4096)])
    add("ring wrap with a pending range change", 40, 16, std + [period(30), run(ROW_UNIFORM, 0, 1060), vrange(-0.5, 0.5), run(ROW_UNIFORM, 1060, 20),
                                                                period(40), rng(-1.0, 1.0, 16), run(ROW_UNIFORM, 1080, 3000)])
    # ---- call sizes at every offset of the row's base from the 16-byte grid
    for n in (0, 1, 3, 255, 256, 257, 1023, 1024, 1025, 4096):
        for base in range(4):
            add("call of %d samples, base %d bytes off" % (n, 4 * base), 600, 16, std + [period(500), run(ROW_UNIFORM, 3 - base, 300), run(ROW_UNIFORM, base, n)])
    for base in range(4):
        add("call of 4096 samples inside a period of 4500, base %d bytes off" % (4 * base), 5000, 16,
            std + [period(4500), run(ROW_SINE, base, 4096), run(ROW_UNIFORM, 3 - base, 1000)])
    # ---- same-bin waves, half-waves and runs
    for row, name in ((ROW_CONSTANT, "constant"), (ROW_TWO, "two-valued"), (ROW_SORTED, "sorted"), (ROW_SINE, "sine")):
        add("%s row" % name, 600, 16, std + [period(500), run(row, 1, 1024), run(row, 1025, 300), run(row, 1325, 2051), vrange(-0.7, 0.2), run(row, 0, 256)])
    # ---- the reference's defect: ONE call of 4096 samples on a ring of 2032 with a period of 900
    add(DEFECT + ": one reference call of 4096 samples, capacity 2032, period 900", 1000, 16,
        [rng(-1.3, 1.3, 16), period(900), (Q.PROCESS_WHOLE, ROW_UNIFORM, 0, 4096)])
    add("the same row in pieces", 1000, 16, [rng(-1.3, 1.3, 16), period(900), run(ROW_UNIFORM, 0, 4096)])
    return out


def run(exe, x, cs, cwd):
    src, dst = os.path.join(cwd, "cases.bin"), os.path.join(cwd, "results.bin")
    with open(src, "wb") as f:
        f.write(np.array([x.shape[0], x.shape[1], len(cs)], u32).tobytes())
        f.write(x.tobytes())
        for c in cs:
            f.write(np.array([c["max_period"], c["max_levels"], len(c["ops"])], u32).tobytes())
            f.write(c["ops"].astype(np.float64).tobytes())
    subprocess.run([exe, src, dst], check=True, timeout=900)
    raw = np.fromfile(dst, u32)
    got, at = [], 0
    for c in cs:
        w, k, cap = c["max_levels"] + 10, len(c["ops"]), Q.capacity_of(c["max_period"])
        words = raw[at:at + w * k].reshape(k, w).copy()
        at += w * k
        got.append({"words": words, "ring": raw[at:at + cap].copy()})
        at += cap
    assert at == raw.size, (at, raw.size)
    return got


def same(a, b):
    return all(np.array_equal(p["words"], q["words"]) and np.array_equal(p["ring"], q["ring"]) for p, q in zip(a, b))


def compile_driver(reference, d, source, exe, extra=()):
    with open(os.path.join(d, "qcounter_prelude.h"), "w") as f:
        f.write(PRELUDE)
    srcs = [source] + [os.path.join(reference, "src", "main", n) for n in REF_SOURCES]
    inc = ["-I" + os.path.join(ROOT, "oracle", "ref_shim"), "-I" + os.path.join(reference, "include"), "-include", os.path.join(d, "qcounter_prelude.h")]
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
    first = got[0]["words"][-1]                                             # the 14 specials: bins 2 0 0 0 1 0 0 1, below 9, above 1
    assert list(first[:8]) == [2, 0, 0, 0, 1, 0, 0, 1] and first[16] == 9 and first[17] == 1, first
    dump = {"sizeof": [int(v) for v in keys[0].split()[1:]], "offsetof": [int(v) for v in keys[1].split()[1:]], "dump": keys[2].split()[1:]}
    names = {"stat/QuantizedCounter.h": public_names(os.path.join(reference, "include", "lsp-plug.in", "dsp-units", "stat", "QuantizedCounter.h"),
                                                     "QuantizedCounter")}
    return x, cs, got, dump, names


def build(reference):
    x, cs, got, dump, names = run_reference(reference)
    arrs = {"x": x, "names": np.array([c["name"] for c in cs]), "max_period": np.array([c["max_period"] for c in cs], u32),
            "max_levels": np.array([c["max_levels"] for c in cs], u32), "ops_n": np.array([len(c["ops"]) for c in cs], u32),
            "ops": np.concatenate([c["ops"] for c in cs]), "words": np.concatenate([r["words"].reshape(-1) for r in got]),
            "ring": np.concatenate([r["ring"] for r in got])}
    return npz_bytes(arrs), dump, names


def load(path=OUT):
    """The stored file as (x, cases): dicts of name, max_period, max_levels, ops, words [k, max_levels + 10], ring [nCapacity]."""
    z = np.load(path)
    x, out = z["x"], []
    at_ops = at_words = at_ring = 0
    for i in range(len(z["names"])):
        mp, ml, k = int(z["max_period"][i]), int(z["max_levels"][i]), int(z["ops_n"][i])
        cap = Q.capacity_of(mp)
        out.append(dict(name=str(z["names"][i]), max_period=mp, max_levels=ml, ops=z["ops"][at_ops:at_ops + k],
                        words=z["words"][at_words:at_words + k * (ml + 10)].reshape(k, ml + 10), ring=z["ring"][at_ring:at_ring + cap]))
        at_ops, at_words, at_ring = at_ops + k, at_words + k * (ml + 10), at_ring + cap
    return x, out


if __name__ == "__main__":
    data, dump, names = build(sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(ROOT), "reference"))
    with open(OUT, "wb") as f:
        f.write(data)
    with open(os.path.join(HERE, "quantized_counter_dump_keys.json"), "w") as f:
        json.dump(dump, f, indent=1)
        f.write("\n")
    with open(os.path.join(HERE, "quantized_counter_public_names.json"), "w") as f:
        json.dump(names, f, indent=1)
        f.write("\n")
    print("%d cases, %d bytes" % (len(load()[1]), len(data)))
