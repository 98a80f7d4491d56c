"""Writes tests/golden/noise_ref_vectors.npz: what the reference's own LCG and MLS classes (and the Randomizer under LCG) compute on a
list of cases, and next to it noise_public_names.json and noise_dump_keys.json.  Data only: operation lists, one source row, the
reference's output, the state words each case ends with; names of public members; dump keys.  Run where the reference tree exists:

    python tests/golden/make_noise_vectors.py [reference tree]

noise/LCG.cpp, noise/MLS.cpp, util/Randomizer.cpp and iface/IStateDumper.cpp are compiled unmodified into a temporary directory
(-O2 -ffp-contract=off -msse2 -mfpmath=sse) against oracle/ref_shim plus an overlay, written here, of what that shim lacks: umword_t
and ARCH_64BIT (mls_t is uint64_t: the LP64 build), lsp_min / lsp_max of two types, and a lsp-plug.in/runtime/system.h whose
get_time reads the host clock (no recorded case calls the argument-less init()).  The program -- a stand-alone one with its own
main -- is built a first time with -fsanitize=address,undefined and run over every case before anything is recorded.

Every case is an operation list ops [k, 4] of (what, a, b, c) -- tests/noise_ref.py names them -- on a fresh object, and a source
row src [N] that the add and mul operations read; the process operations fill out [N] in order.  POKE_LAST writes one generator's
vLast (the class has no setter: the program reaches into the object), so that the draws 0 and >= 0xFFFFFF80 -- rv == 0.0f and
rv == 1.0f -- are reached by state and not by luck: the values come from a search over all 2^32 states of generator 0 of seed 1."""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)
import noise_ref as R  # noqa: E402
from make_bypass_crossfade_vectors import npz_bytes, public_names  # noqa: E402

OUT = os.path.join(HERE, "noise_ref_vectors.npz")
f32, u32, u64 = np.float32, np.uint32, np.uint64

N = 1100
PIECES = (N, 1, 3, 7, 255, 257, 1023)
WORDS = 17
EDGE_SEED = 1
ZERO_FROM, ONE_FROM = 0xE245766B, 0x00BA0F5D           # generator 0 of seed 1: the next draw is 0, is >= 0xFFFFFF80 (find_edges)
EXP_LAMBDA_BITS = 0x423AE418

OVERLAY_VERSION = r'''
#ifndef NOISE_OVERLAY_VERSION_H_
#define NOISE_OVERLAY_VERSION_H_
#include <lsp-plug.in/common/types.h>
#ifndef LSP_DSP_UNITS_PUBLIC
#define LSP_DSP_UNITS_PUBLIC
#endif
#endif
'''

OVERLAY_TYPES = r'''
#ifndef NOISE_OVERLAY_TYPES_H_
#define NOISE_OVERLAY_TYPES_H_
#include_next <lsp-plug.in/common/types.h>
#define ARCH_64BIT
namespace lsp
{
    typedef uint64_t umword_t;
    template <class A, class B> inline A lsp_min(A a, B b) { return (a < A(b)) ? a : A(b); }
    template <class A, class B> inline A lsp_max(A a, B b) { return (a > A(b)) ? a : A(b); }
}
#endif
'''

OVERLAY_SYSTEM = r'''
#ifndef NOISE_OVERLAY_SYSTEM_H_
#define NOISE_OVERLAY_SYSTEM_H_
#include <lsp-plug.in/common/types.h>
#include <time.h>
namespace lsp
{
    namespace system
    {
        typedef struct time_t { uint64_t seconds; uint32_t nanos; } time_t;
        inline void get_time(time_t *t)
        {
            struct timespec ts;
            clock_gettime(CLOCK_REALTIME, &ts);
            t->seconds = uint64_t(ts.tv_sec), t->nanos = uint32_t(ts.tv_nsec);
        }
    }
}
#endif
'''

# reads the cases, runs the class, writes out[n] and the state words of every case; with "keys" as its only argument it prints the
# objects' sizes, expf(float(M_E * M_SQRT2)) as the compiler folds it and as the C library computes it, and what dump() writes
DRIVER = r'''
#define private public
#define protected public
#include <lsp-plug.in/dsp-units/noise/LCG.h>
#include <lsp-plug.in/dsp-units/noise/MLS.h>
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
    void write(const char *n, unsigned long) override   { note(n); }
    void write(const char *n, unsigned long long) override { note(n); }
    void write(const char *n, float) override           { note(n); }
};
static uint32_t fb(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static void process(int what, float *out, const float *src, size_t n, dspu::LCG *l, dspu::MLS *m)
{
    #define RUN(call) do { if (l) l->call; else m->call; } while (0)
    switch (what)
    {
        case 0: RUN(process_overwrite(out, n)); break;
        case 1: RUN(process_add(out, src, n)); break;
        case 2: memcpy(out, src, 4 * n); RUN(process_add(out, out, n)); break;
        case 3: RUN(process_mul(out, src, n)); break;
        case 4: memcpy(out, src, 4 * n); RUN(process_mul(out, out, n)); break;
    }
    #undef RUN
}
int main(int argc, char **argv)
{
    if (argc == 2 && strcmp(argv[1], "keys") == 0)
    {
        dspu::Randomizer r; dspu::LCG l; dspu::MLS m;
        r.init(1); l.init(1);
        keys kr, kl, km;
        r.dump(&kr); l.dump(&kl); m.dump(&km);
        volatile float lambda = float(M_E * M_SQRT2);
        printf("sizeof %zu %zu %zu %zu\n", sizeof(r), sizeof(l), sizeof(m), sizeof(dspu::MLS::mls_t));
        printf("explambda %u %u\n", fb(expf(float(M_E * M_SQRT2))), fb(expf(lambda)));
        printf("Randomizer%s\nLCG%s\nMLS%s\n", kr.seen.c_str(), kl.seen.c_str(), km.seen.c_str());
        return 0;
    }
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb"), *g = fopen(argv[2], "wb");
    if (!f || !g) return 2;
    uint32_t hdr[2];
    if (fread(hdr, 4, 2, f) != 2) return 3;
    const uint32_t cases = hdr[0], n = hdr[1];
    std::vector<float> src(n), out(n);
    for (uint32_t c = 0; c < cases; ++c)
    {
        uint32_t kk[2];
        if (fread(kk, 4, 2, f) != 2) return 3;
        const uint32_t kind = kk[0], k = kk[1];
        std::vector<double> ops(4 * size_t(k));
        if (fread(ops.data(), 8, ops.size(), f) != ops.size()) return 3;
        if (fread(src.data(), 4, n, f) != n) return 3;
        std::fill(out.begin(), out.end(), 0.0f);
        dspu::LCG l; dspu::MLS m;
        size_t at = 0;
        for (uint32_t j = 0; j < k; ++j)
        {
            const int what = int(ops[4 * j]);
            const double a = ops[4 * j + 1], b = ops[4 * j + 2];
            const size_t cnt = (what <= 4) ? size_t(a) : 0;
            if (at + cnt > n) return 5;
            if (what <= 4)
                process(what, &out[at], &src[at], cnt, kind == 0 ? &l : NULL, &m);
            else if (kind == 0) switch (what)
            {
                case 5: l.init(uint32_t(a)); break;
                case 6: if (a < 0 || a > 3) return 6; l.set_distribution(dspu::lcg_dist_t(int(a))); break;
                case 7: l.set_amplitude(float(a)); break;
                case 8: l.set_offset(float(a)); break;
                case 9: l.sRand.vRandom[size_t(a) & 3].vLast = uint32_t(b); break;
                default: return 6;
            }
            else switch (what)
            {
                case 7: m.set_amplitude(float(a)); break;
                case 8: m.set_offset(float(a)); break;
                case 10: m.set_n_bits(size_t(a)); break;
                case 11: m.set_state(uint64_t(a) | (uint64_t(b) << 32)); break;
                case 12: m.set_state(m.nState); break;
                default: return 6;
            }
            at += cnt;
        }
        if (at != n) return 7;
        fwrite(out.data(), 4, n, g);
        uint64_t w[17] = { 0 };
        if (kind == 0)
        {
            for (int i = 0; i < 4; ++i)
                w[i] = l.sRand.vRandom[i].vLast, w[4 + i] = l.sRand.vRandom[i].vMul1, w[8 + i] = l.sRand.vRandom[i].vMul2, w[12 + i] = l.sRand.vRandom[i].vAdd;
            w[16] = l.sRand.nBufID;
        }
        else
        {
            const uint64_t v[9] = { m.nBits, m.nFeedbackBit, m.nFeedbackMask, m.nActiveMask, m.nTapsMask, m.nOutputMask, m.nState, m.bSync, m.get_period() };
            memcpy(w, v, sizeof(v));
        }
        fwrite(w, 8, 17, g);
    }
    fclose(f);
    return fclose(g) == 0 ? 0 : 8;
}
'''

FLAGS = ["-std=c++11", "-O2", "-ffp-contract=off", "-msse2", "-mfpmath=sse", "-DLSP_DSP_UNITS_BUILTIN", "-Wall"]
SAN_FLAGS = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
REF_SOURCES = ("noise/LCG.cpp", "noise/MLS.cpp", "util/Randomizer.cpp", "iface/IStateDumper.cpp")


def source_row():
    """What add and mul read: noise with +0, -0, Inf, NaN and subnormals in it."""
    rng = np.random.default_rng(24680)
    s = (rng.standard_normal(N) * 0.5).astype(f32)
    s[::50] = 0.0
    s[25::50] = -0.0
    s[3], s[302], s[777] = np.inf, -np.inf, np.inf
    for at in (11, 500, 1001):
        s[at] = np.nan
    s[40], s[41] = 1e-40, -1e-42
    return s


def find_edges(seed=EDGE_SEED):
    """All 2^32 states of generator 0 of `seed`: the states whose next draw is 0, and those whose next draw is >= 0xFFFFFF80."""
    _, mul1, mul2, add = R.seed_words(seed)[0]
    zero, one = [], []
    for lo in range(0, 1 << 32, 1 << 24):
        v = np.arange(lo, lo + (1 << 24), dtype=u64)
        nxt = (u64(mul1) * v + (((u64(mul2) * v) & u64(R.M32)) >> u64(16)) + u64(add)) & u64(R.M32)
        zero += [int(x) for x in v[nxt == 0]]
        one += [int(x) for x in v[nxt >= 0xFFFFFF80]]
    return zero, one


def pieces(call, what=R.P_OVERWRITE, n=N):
    ops, at = [], 0
    while at < n:
        k = min(call, n - at)
        ops.append((what, k))
        at += k
    return ops


def edge_ops(dist):
    """Draws of 0 and of >= 0xFFFFFF80 as the first draw of a sample and, for the two-draw distributions, as the second: single
    uniform samples turn nBufID to where generator 0 is next (first draw) or next but one (second draw)."""
    D = R.DRAWS[dist]
    ops, buf, at = [(R.INIT, EDGE_SEED), (R.SET_DISTRIBUTION, dist)], 0, 0
    for target in ((0, 3) if D == 2 else (0,)):
        for value in (ZERO_FROM, ONE_FROM):
            if dist == R.LCG_GAUSSIAN and target == 0 and value == ONE_FROM:
                continue            # logf(1.0f) is 0 with neighbours of both signs, and sqrtf of the negative one is NaN: no interval
            if buf != target:
                k = (target - buf) & 3
                ops += [(R.SET_DISTRIBUTION, R.LCG_UNIFORM), (R.P_OVERWRITE, k), (R.SET_DISTRIBUTION, dist)]
                buf, at = target, at + k
            ops += [(R.POKE_LAST, 0, value), (R.P_OVERWRITE, 5)]
            buf, at = (buf + 5 * D) & 3, at + 5
    return ops + pieces(257, n=N - at)


def cases():
    out = []

    def add(name, kind, ops):
        arr = np.array([tuple(float(v) for v in (list(o) + [0, 0, 0])[:4]) for o in ops], np.float64).reshape(-1, 4)
        out.append(dict(name=name, kind=kind, ops=arr))

    i = 0

    def call():
        nonlocal i
        i += 1
        return PIECES[i % len(PIECES)]

    sub = float(f32(1e-40))
    # ---- LCG: four distributions x four seeds, amplitude and offset from a list that has 0, a negative, a subnormal and Inf in it
    levels = ((1.0, 0.0), (0.5, 0.25), (0.0, 0.3), (-2.0, 0.1), (sub, 0.0), (np.inf, 0.0), (1.5, -0.75), (0.25, sub))
    j = 0
    for dist in range(4):
        for seed in (0, 1, 0x12345678, 0xFFFFFFFF):
            A, off = levels[j % len(levels)]
            j += 3
            add("LCG %s seed %#x amplitude %g offset %g" % (R.DISTRIBUTIONS[dist], seed, A, off), R.KIND_LCG,
                [(R.INIT, seed), (R.SET_DISTRIBUTION, dist), (R.SET_AMPLITUDE, A), (R.SET_OFFSET, off)] + pieces(call()))
    for dist in range(4):
        for A, off in ((np.inf, 0.5), (sub, sub), (0.0, 0.0), (-1.0, np.inf)):
            if (dist + int(A == 0.0) + int(off == np.inf)) % 2:
                continue
            add("LCG %s amplitude %g offset %g" % (R.DISTRIBUTIONS[dist], A, off), R.KIND_LCG,
                [(R.INIT, 0xC0FFEE), (R.SET_DISTRIBUTION, dist), (R.SET_AMPLITUDE, A), (R.SET_OFFSET, off)] + pieces(call()))
    # overwrite, add and mul, in place
    for dist in range(4):
        add("LCG %s add, mul and overwrite mixed" % R.DISTRIBUTIONS[dist], R.KIND_LCG,
            [(R.INIT, 0xBEEF + dist), (R.SET_DISTRIBUTION, dist), (R.SET_AMPLITUDE, 0.75), (R.SET_OFFSET, 0.125),
             (R.P_ADD, 100), (R.P_MUL, 200), (R.P_OVERWRITE, 300), (R.P_MUL_INPLACE, 250), (R.P_ADD_INPLACE, 250)])
    add("LCG uniform add in calls of 7", R.KIND_LCG, [(R.INIT, 77)] + pieces(7, R.P_ADD))
    add("LCG gaussian mul in place in calls of 3", R.KIND_LCG, [(R.INIT, 78), (R.SET_DISTRIBUTION, R.LCG_GAUSSIAN)] + pieces(3, R.P_MUL_INPLACE))
    # the distribution changes between calls: nBufID goes on from where the last call left it
    for piece in (255, 3):
        ops, at, d = [(R.INIT, 0xABCDEF01), (R.SET_AMPLITUDE, 0.9)], 0, 0
        while at < N:
            k = min(piece, N - at)
            ops += [(R.SET_DISTRIBUTION, (d * 3 + 1) % 4), (R.P_OVERWRITE, k)]
            at, d = at + k, d + 1
        add("LCG distribution changes every %d samples" % piece, R.KIND_LCG, ops)
    # the edge draws, reached by state
    for dist in range(4):
        add("LCG %s edge draws" % R.DISTRIBUTIONS[dist], R.KIND_LCG, edge_ops(dist))
    # ---- MLS: register widths x seeds
    seeds = ((0, "0"), (1, "1"), (0xDEADBEEFCAFEF00D, "with high bits"), (R.M64, "all ones"))
    mlevels = ((1.0, 0.0), (0.5, 0.25), (-2.0, 0.1), (1.0, -3.0))
    kinds = (R.P_OVERWRITE, R.P_OVERWRITE, R.P_ADD, R.P_OVERWRITE, R.P_MUL, R.P_OVERWRITE, R.P_ADD_INPLACE, R.P_OVERWRITE, R.P_MUL_INPLACE)
    j = 0
    for bits in (0, 1, 2, 3, 8, 23, 32, 33, 63, 64, 200):
        for seed, label in seeds:
            A, off = mlevels[j % len(mlevels)]
            what = kinds[j % len(kinds)]
            j += 1
            add("MLS %d bits, seed %s, amplitude %g offset %g" % (bits, label, A, off), R.KIND_MLS,
                [(R.SET_N_BITS, bits), (R.SET_STATE, seed & R.M32, seed >> 32), (R.SET_AMPLITUDE, A), (R.SET_OFFSET, off)] + pieces(call(), what))
    add("MLS 3 bits over 100 samples and on", R.KIND_MLS, [(R.SET_N_BITS, 3), (R.SET_STATE, 5, 0), (R.P_OVERWRITE, 100)] + pieces(1000, n=N - 100))
    add("MLS as constructed", R.KIND_MLS, pieces(257))
    add("MLS set_state with the current state", R.KIND_MLS,
        [(R.SET_N_BITS, 23), (R.SET_STATE, 0x1234, 0), (R.P_OVERWRITE, 300), (R.SET_STATE_CURRENT,), (R.P_OVERWRITE, 300), (R.SET_STATE, 0x1234, 0),
         (R.P_OVERWRITE, 250), (R.SET_STATE, 0, 0x80000000), (R.P_OVERWRITE, 250)])
    add("MLS set_n_bits on the way", R.KIND_MLS,
        [(R.SET_N_BITS, 33), (R.SET_STATE, 0x9ABCDEF1, 0x1), (R.P_OVERWRITE, 255), (R.SET_N_BITS, 8), (R.P_OVERWRITE, 257), (R.SET_N_BITS, 64),
         (R.P_OVERWRITE, 7), (R.SET_N_BITS, 0), (R.P_OVERWRITE, 81), (R.SET_N_BITS, 12), (R.SET_STATE, 0xF000, 0), (R.P_OVERWRITE, 500)])
    add("MLS amplitude 0", R.KIND_MLS, [(R.SET_N_BITS, 16), (R.SET_AMPLITUDE, 0.0), (R.SET_OFFSET, 0.3)] + pieces(1023, R.P_MUL))
    add("MLS amplitude Inf", R.KIND_MLS, [(R.SET_N_BITS, 16), (R.SET_AMPLITUDE, np.inf), (R.SET_OFFSET, 1.0)] + pieces(255, R.P_ADD))
    add("MLS amplitude and offset Inf", R.KIND_MLS, [(R.SET_N_BITS, 9), (R.SET_AMPLITUDE, np.inf), (R.SET_OFFSET, np.inf)] + pieces(3))
    add("MLS add, mul and overwrite mixed", R.KIND_MLS,
        [(R.SET_N_BITS, 31), (R.SET_STATE, 0x55555555, 0), (R.SET_AMPLITUDE, 0.75), (R.SET_OFFSET, 0.125),
         (R.P_ADD, 100), (R.P_MUL, 200), (R.P_OVERWRITE, 300), (R.P_MUL_INPLACE, 250), (R.P_ADD_INPLACE, 250)])
    return out


def write_cases(path, cs, src):
    with open(path, "wb") as f:
        f.write(np.array([len(cs), N], u32).tobytes())
        for c in cs:
            f.write(np.array([c["kind"], len(c["ops"])], u32).tobytes() + c["ops"].tobytes() + src.tobytes())


def read_results(path, cs):
    got = []
    with open(path, "rb") as f:
        for _ in cs:
            out = np.frombuffer(f.read(4 * N), f32)
            got.append(dict(out=out, words=np.frombuffer(f.read(8 * WORDS), u64)))
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
        for rel, text in (("lsp-plug.in/dsp-units/version.h", OVERLAY_VERSION), ("lsp-plug.in/common/types.h", OVERLAY_TYPES),
                          ("lsp-plug.in/runtime/system.h", OVERLAY_SYSTEM)):
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
        # the two builds may round a NaN's sign differently; everything else is the same bits
        assert R.same(a["out"], b["out"]).all() and np.array_equal(a["words"], b["words"]), c["name"]
    assert keys["explambda"] == [str(EXP_LAMBDA_BITS)] * 2, keys["explambda"]      # folded by the compiler, and the C library's
    assert keys["sizeof"][3] == "8", keys["sizeof"]                                 # mls_t is uint64_t
    inc = os.path.join(reference, "include", "lsp-plug.in", "dsp-units")
    names = {"util/Randomizer.h": public_names(os.path.join(inc, "util", "Randomizer.h"), "Randomizer"),
             "noise/LCG.h": public_names(os.path.join(inc, "noise", "LCG.h"), "LCG"),
             "noise/MLS.h": public_names(os.path.join(inc, "noise", "MLS.h"), "MLS")}
    return cs, src, got, keys, names


class LoggingLCG(R.LCG):
    def __init__(self):
        super().__init__()
        self.log = []

    def draws(self, n):
        out = super().draws(n)
        self.log.append(out)
        return out


def check_branches(cs, src, got):
    """What the cases are there for has happened in them."""
    by = {c["name"]: (c, g) for c, g in zip(cs, got)}
    _, mul1, mul2, add = R.seed_words(EDGE_SEED)[0]
    assert R.step(ZERO_FROM, mul1, mul2, add) == 0 and R.step(ONE_FROM, mul1, mul2, add) >= 0xFFFFFF80
    assert R.linear([0])[0] == 0 and R.linear([0xFFFFFF80])[0] == 1 and R.linear([0xFFFFFF7F])[0] < 1
    for dist in range(4):
        c, g = by["LCG %s edge draws" % R.DISTRIBUTIONS[dist]]
        # the restatement's draws: 0 and >= 0xFFFFFF80 in each role
        unit, roles = LoggingLCG(), set()
        for op in c["ops"]:
            if int(op[0]) in R.PROCESS_OPS:
                D = R.DRAWS.get(unit.dist, 1)
                raw = unit.draws(D * int(op[1]))
                if unit.dist == dist:
                    for k, v in enumerate(raw):
                        if v == 0 or v >= 0xFFFFFF80:
                            roles.add((k % D, int(v == 0)))
            else:
                R.apply(unit, op)
        assert len(roles) == 2 * R.DRAWS[dist] - (dist == R.LCG_GAUSSIAN), (dist, roles)
    assert np.isinf(by["LCG gaussian edge draws"][1]["out"]).any()             # sqrtf(-2 logf(0)) = Inf
    for c, g in zip(cs, got):
        if c["kind"] == R.KIND_LCG:
            assert g["words"][16] == sum(R.DRAWS[_dist_at(c, k)] * int(op[1]) for k, op in enumerate(c["ops"]) if int(op[0]) in R.PROCESS_OPS) % 4, c["name"]
    c, g = by["MLS 3 bits over 100 samples and on"]
    assert np.array_equal(g["out"][:93], g["out"][7:100]) and len(set(g["out"][:7])) == 2
    assert by["MLS 0 bits, seed 0, amplitude 1 offset 0"][1]["words"][0] == 1 and by["MLS 200 bits, seed 1, amplitude 0.5 offset 0.25"][1]["words"][0] == 64
    return len(cs)


def _dist_at(c, k):
    d = R.LCG_UNIFORM
    for op in c["ops"][:k]:
        if int(op[0]) == R.SET_DISTRIBUTION:
            d = int(op[1])
    return d


def build(reference):
    cs, src, got, keys, names = run_reference(reference)
    check_branches(cs, src, got)
    arrs = {"src": src, "names": np.array([c["name"] for c in cs]), "kind": np.array([c["kind"] for c in cs], u32),
            "ops_n": np.array([len(c["ops"]) for c in cs], u32), "ops": np.concatenate([c["ops"] for c in cs]),
            "out": np.array([g["out"] for g in got]), "words": np.array([g["words"] for g in got])}
    return npz_bytes(arrs), keys, names


def load(path=OUT):
    """The stored file as a list of cases: dicts of name, kind, ops [k, 4], src [N], out [N], words [17]."""
    z = np.load(path)
    off = np.concatenate([[0], np.cumsum(z["ops_n"].astype(np.int64))])
    return [dict(name=str(z["names"][i]), kind=int(z["kind"][i]), ops=z["ops"][off[i]:off[i + 1]], src=z["src"], out=z["out"][i],
                 words=z["words"][i]) for i in range(len(z["names"]))]


if __name__ == "__main__":
    reference = sys.argv[1] if len(sys.argv) > 1 and sys.argv[1] != "--search" else os.path.join(os.path.dirname(ROOT), "reference")
    if "--search" in sys.argv:                              # about a minute: all 2^32 states
        zero, one = find_edges()
        print("next draw 0: %s; next draw >= 0xFFFFFF80: %d states, e.g. %#x" % ([hex(v) for v in zero], len(one), one[0]))
        assert ZERO_FROM in zero and ONE_FROM in one
    data, keys, names = build(reference)
    assert len(data) <= 262601, len(data)
    with open(OUT, "wb") as f:
        f.write(data)
    with open(os.path.join(HERE, "noise_dump_keys.json"), "w") as f:
        json.dump({cls: {"keys": keys[cls], "sizeof": int(keys["sizeof"][k])} for k, cls in enumerate(("Randomizer", "LCG", "MLS"))}, f, indent=1)
        f.write("\n")
    with open(os.path.join(HERE, "noise_public_names.json"), "w") as f:
        json.dump(names, f, indent=1)
        f.write("\n")
    print("%d cases, %d bytes" % (len(load()), len(data)))
