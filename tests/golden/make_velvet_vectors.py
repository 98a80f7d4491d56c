"""Writes tests/golden/velvet_ref_vectors.npz: what the reference's own Velvet class computes on a list of cases, and next to it
velvet_public_names.json and velvet_dump_keys.json.  Data only: operation lists, one source row, the reference's output, the state
words (Randomizer and MLS) each case ends with; names of public members; dump keys, sizeof and offsetof.  Run where the reference
tree exists:

    python tests/golden/make_velvet_vectors.py [reference tree]

noise/Velvet.cpp, noise/MLS.cpp, util/Randomizer.cpp and iface/IStateDumper.cpp are compiled unmodified into a temporary directory
(-O2 -ffp-contract=off -msse2 -mfpmath=sse) against oracle/ref_shim, the overlay of make_noise_vectors.py and a one-function
stand-in for the five lsp::dsp routines that Velvet.cpp calls (fill_zero, mul_k2, add_k2, add3, mul3: one operation per sample).
The program -- a stand-alone one with its own main -- is built a first time with -fsanitize=address,undefined and run over every
case before anything is recorded.

Every case is an operation list ops [k, 4] of (what, a, b, c) -- tests/velvet_ref.py names them -- on a fresh object, and a source
row src [N] that the add and mul operations read; the process operations fill out [N] in order, and what they leave unfilled stays
0, so that a case and its prefixes give the state words after every call.  POKE_LAST writes one generator's vLast, as in
make_noise_vectors.py, whose ZERO_FROM and ONE_FROM (generator 0 of seed 1) make the draws rv == 0.0f and rv == 1.0f."""
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
import velvet_ref as V  # noqa: E402
import make_noise_vectors as noise  # noqa: E402
from make_bypass_crossfade_vectors import npz_bytes, public_names  # noqa: E402

OUT = os.path.join(HERE, "velvet_ref_vectors.npz")
f32, u32, u64 = np.float32, np.uint32, np.uint64

N = noise.N
PIECES = (N, 1, 3, 7, 255, 256, 257, 1023)
EDGE_SEED, ZERO_FROM, ONE_FROM = noise.EDGE_SEED, noise.ZERO_FROM, noise.ONE_FROM
MEMBERS = ("sRandomizer", "sMLS", "enCore", "enVelvetType", "sCrushParams", "fWindowWidth", "fARNdelta", "fAmplitude", "fOffset")

# lsp::dsp as Velvet.cpp uses it: one float operation per sample
OVERLAY_DSP = r'''
#ifndef VELVET_OVERLAY_DSP_H_
#define VELVET_OVERLAY_DSP_H_
#include <lsp-plug.in/common/types.h>
namespace lsp
{
    namespace dsp
    {
        inline void fill_zero(float *dst, size_t n)                 { for (size_t i = 0; i < n; ++i) dst[i] = 0.0f; }
        inline void mul_k2(float *dst, float k, size_t n)           { for (size_t i = 0; i < n; ++i) dst[i] = dst[i] * k; }
        inline void add_k2(float *dst, float k, size_t n)           { for (size_t i = 0; i < n; ++i) dst[i] = dst[i] + k; }
        inline void add3(float *dst, const float *a, const float *b, size_t n) { for (size_t i = 0; i < n; ++i) dst[i] = a[i] + b[i]; }
        inline void mul3(float *dst, const float *a, const float *b, size_t n) { for (size_t i = 0; i < n; ++i) dst[i] = a[i] * b[i]; }
    }
}
#endif
'''

# reads the cases, runs the class, writes out[n] and the state words of every case; with "keys" as its only argument it prints
# sizeof and offsetof of the class and what dump() writes
DRIVER = r'''
#define private public
#define protected public
#include <lsp-plug.in/dsp-units/noise/Velvet.h>
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
    void write(const char *n, unsigned long) override   { note(n); }
    void write(const char *n, unsigned long long) override { note(n); }
    void write(const char *n, float) override           { note(n); }
};
int main(int argc, char **argv)
{
    using dspu::Velvet;
    if (argc == 2 && strcmp(argv[1], "keys") == 0)
    {
        Velvet v;
        v.init(1, 23, 5);
        keys k;
        v.dump(&k);
        printf("sizeof %zu\n", sizeof(Velvet));
        printf("offsetof %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", offsetof(Velvet, sRandomizer), offsetof(Velvet, sMLS), offsetof(Velvet, enCore),
               offsetof(Velvet, enVelvetType), offsetof(Velvet, sCrushParams), offsetof(Velvet, fWindowWidth), offsetof(Velvet, fARNdelta),
               offsetof(Velvet, fAmplitude), offsetof(Velvet, fOffset), sizeof(Velvet::crush_t), offsetof(Velvet::crush_t, bCrush),
               offsetof(Velvet::crush_t, fCrushProb));
        printf("Velvet%s\n", k.seen.c_str());
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
        uint32_t k;
        if (fread(&k, 4, 1, f) != 1) return 3;
        std::vector<double> ops(4 * size_t(k));
        if (fread(ops.data(), 8, ops.size(), f) != ops.size()) return 3;
        if (fread(src.data(), 4, n, f) != n) return 3;
        std::fill(out.begin(), out.end(), 0.0f);
        Velvet v;
        size_t at = 0;
        for (uint32_t j = 0; j < k; ++j)
        {
            const int what = int(ops[4 * j]);
            const double a = ops[4 * j + 1], b = ops[4 * j + 2], d = ops[4 * j + 3];
            const bool runs = what <= 4 || what == 20 || what == 21;
            const size_t cnt = runs ? size_t(a) : 0;
            if (at + cnt > n) return 5;
            if (runs && v.sRandomizer.nBufID > 3) return 9;
            float *o = out.data() + at;
            const float *s = src.data() + at;
            switch (what)
            {
                case 0: v.process_overwrite(o, cnt); break;
                case 1: v.process_add(o, s, cnt); break;
                case 2: memcpy(o, s, 4 * cnt); v.process_add(o, o, cnt); break;
                case 3: v.process_mul(o, s, cnt); break;
                case 4: memcpy(o, s, 4 * cnt); v.process_mul(o, o, cnt); break;
                case 20: memcpy(o, s, 4 * cnt); v.process_add(o, NULL, cnt); break;
                case 21: memcpy(o, s, 4 * cnt); v.process_mul(o, NULL, cnt); break;
                case 5: v.init(uint32_t(a), uint8_t(b), uint64_t(d)); break;
                case 19: v.init(uint32_t(a), uint8_t(b), v.sMLS.nState); break;
                case 7: v.set_amplitude(float(a)); break;
                case 8: v.set_offset(float(a)); break;
                case 9: v.sRandomizer.vRandom[size_t(a) & 3].vLast = uint32_t(b); break;
                case 13: v.set_core_type(dspu::vn_core_t(int(a))); break;
                case 14: v.set_velvet_type(dspu::vn_velvet_type_t(int(a))); break;
                case 15: v.set_velvet_window_width(float(a)); break;
                case 16: v.set_delta_value(float(a)); break;
                case 17: v.set_crush(a != 0); break;
                case 18: v.set_crush_probability(float(a)); break;
                default: return 6;
            }
            at += cnt;
        }
        fwrite(out.data(), 4, n, g);
        uint64_t w[25] = { 0 };
        const dspu::Randomizer &r = v.sRandomizer;
        const dspu::MLS &m = v.sMLS;
        for (int i = 0; i < 4; ++i)
            w[i] = r.vRandom[i].vLast, w[4 + i] = r.vRandom[i].vMul1, w[8 + i] = r.vRandom[i].vMul2, w[12 + i] = r.vRandom[i].vAdd;
        w[16] = r.nBufID;
        const uint64_t mw[8] = { m.nBits, m.nFeedbackBit, m.nFeedbackMask, m.nActiveMask, m.nTapsMask, m.nOutputMask, m.nState, m.bSync };
        memcpy(w + 17, mw, sizeof(mw));
        fwrite(w, 8, 25, g);
    }
    fclose(f);
    return fclose(g) == 0 ? 0 : 8;
}
'''

FLAGS = noise.FLAGS
SAN_FLAGS = noise.SAN_FLAGS
REF_SOURCES = ("noise/Velvet.cpp", "noise/MLS.cpp", "util/Randomizer.cpp", "iface/IStateDumper.cpp")
OVERLAYS = (("lsp-plug.in/dsp-units/version.h", noise.OVERLAY_VERSION), ("lsp-plug.in/common/types.h", noise.OVERLAY_TYPES),
            ("lsp-plug.in/runtime/system.h", noise.OVERLAY_SYSTEM), ("lsp-plug.in/dsp/dsp.h", OVERLAY_DSP))

source_row = noise.source_row


def pieces(call, what=R.P_OVERWRITE, n=N):
    return noise.pieces(call, what, n)


def setup(seed=0x1234, n_bits=23, mls_seed=0x2F, core=V.CORE_LCG, type_=V.OVN, crush=None, width=10.0, delta=None, amplitude=None, offset=None):
    ops = [(V.INIT, seed, n_bits, mls_seed), (V.SET_CORE, core), (V.SET_TYPE, type_), (V.SET_WIDTH, width)]
    if crush is not None:
        ops += [(V.SET_CRUSH, 1), (V.SET_CRUSH_PROB, crush)]
    if delta is not None:
        ops.append((V.SET_DELTA, delta))
    if amplitude is not None:
        ops.append((R.SET_AMPLITUDE, amplitude))
    if offset is not None:
        ops.append((R.SET_OFFSET, offset))
    return ops


def as_ops(ops):
    return np.array([tuple(float(v) for v in (list(o) + [0, 0, 0])[:4]) for o in ops], np.float64).reshape(-1, 4)


def restated_draws(ops):
    """The restatement's log of (role, raw draw) over an operation list."""
    c = dict(ops=as_ops(ops), src=source_row())
    return V.run_case(c)[1].drawn


def edge_cases():
    """rv == 0.0f and rv == 1.0f on a position draw, a spike draw and a crush draw: uncrushed TRN samples (one draw each) turn nBufID
    to where generator 0 of seed 1 is the draw wanted, then its vLast is poked."""
    out = []
    for role, pre, crush in (("position", 0, None), ("spike", 3, None), ("crush", 3, 0.5)):
        for type_ in (V.OVN, V.OVNA, V.ARN):
            ops = [(V.INIT, EDGE_SEED, 16, 1), (V.SET_CORE, V.CORE_LCG), (V.SET_WIDTH, 10.0), (V.SET_TYPE, V.TRN), (R.P_OVERWRITE, 4 + pre)]
            ops += [(V.SET_TYPE, type_)] + ([(V.SET_CRUSH, 1), (V.SET_CRUSH_PROB, crush)] if crush is not None else [])
            ops += [(R.POKE_LAST, 0, ZERO_FROM), (R.P_OVERWRITE, 300), (V.SET_TYPE, V.TRN), (V.SET_CRUSH, 0)]
            # to the same place in the round robin again, whatever the segment consumed
            used = len(restated_draws(ops))
            ops += [(R.P_OVERWRITE, (pre - used) % 4 + 4), (V.SET_TYPE, type_)] + ([(V.SET_CRUSH, 1)] if crush is not None else [])
            ops += [(R.POKE_LAST, 0, ONE_FROM), (R.P_ADD, 300)]
            out.append(("%s edge draws on a %s draw" % (V.TYPES[type_], role), ops))
    # TRN: the sample draw and the sign draw
    ops = [(V.INIT, EDGE_SEED, 16, 1), (V.SET_TYPE, V.TRN), (V.SET_WIDTH, 2.0), (V.SET_CRUSH, 1), (V.SET_CRUSH_PROB, 1.0), (R.POKE_LAST, 0, ZERO_FROM),
           (R.P_OVERWRITE, 8), (R.POKE_LAST, 0, ONE_FROM), (R.P_OVERWRITE, 8), (V.SET_CRUSH_PROB, 0.0), (R.POKE_LAST, 0, ZERO_FROM), (R.P_OVERWRITE, 6),
           (R.POKE_LAST, 0, ONE_FROM), (R.P_OVERWRITE, 6)] + pieces(257, R.P_MUL, N - 28)
    out.append(("TRN edge draws", ops))
    # OVNA at W = 2: rv == 1.0f puts window 0 on sample 2, window 1's first sample; the number of TRN samples before is searched
    # for one where window 1 lands there too and replaces it
    for pre in range(0, 64, 4):
        ops = [(V.INIT, EDGE_SEED, 16, 1), (V.SET_CORE, V.CORE_LCG), (V.SET_WIDTH, 2.0), (V.SET_TYPE, V.TRN), (R.P_OVERWRITE, 4 + pre),
               (V.SET_TYPE, V.OVNA), (R.POKE_LAST, 0, ONE_FROM), (R.P_OVERWRITE, 500)]
        d = [x for x in restated_draws(ops) if x[0] != "t"]
        if d[0][1] >= 0xFFFFFF80 and int(f32(2) + R.linear([d[2][1]])[0] * f32(2)) == 2 and R.linear([d[1][1]])[0] >= 0.5 > R.linear([d[3][1]])[0]:
            out.append(("OVNA window 0 with rv 1 lands in window 1 and is replaced", ops))
            break
    else:
        raise AssertionError("no collision found")
    return out


def cases():
    out = []

    def add(name, ops):
        out.append(dict(name=name, ops=as_ops(ops)))

    i = 0

    def call():
        nonlocal i
        i += 1
        return PIECES[i % len(PIECES)]

    whats = (R.P_OVERWRITE, R.P_ADD, R.P_OVERWRITE, R.P_MUL, V.P_ADD_NULL, R.P_ADD_INPLACE, R.P_OVERWRITE, R.P_MUL_INPLACE)
    widths = (10.0, 2.0, 2.5, 10.7, 64.0, 5.0)
    j = 0
    # ---- types x cores x crush off / on with probability 0, 0.5, 1
    for type_ in range(4):
        for core in (V.CORE_MLS, V.CORE_LCG):
            for crush in (None, 0.0, 0.5, 1.0):
                w, what = widths[j % len(widths)], whats[j % len(whats)]
                j += 1
                add("%s core %d crush %s W %g" % (V.TYPES[type_], core, crush, w),
                    setup(seed=0x100 + j, core=core, type_=type_, crush=crush, width=w) + pieces(call(), what))
    # ---- widths (1.0 is clamped to 2) and ARN's delta (clamped to 0 .. 1)
    for w in (1.0, 2.0, 2.5, 10.0, 10.7, 64.0, 256.0, 257.0, 1000.0):
        for type_ in (V.OVN, V.OVNA, V.ARN):
            core = (V.CORE_MLS, V.CORE_LCG)[j % 2]
            what = (R.P_OVERWRITE, R.P_ADD)[(j // 2) % 2]
            j += 1
            add("%s W %g core %d" % (V.TYPES[type_], w, core), setup(seed=0x200 + j, core=core, type_=type_, width=w) + pieces(call(), what))
        add("TRN W %g" % w, setup(seed=0x300 + j, type_=V.TRN, width=w, crush=0.25 if w in (2.5, 257.0) else None) + pieces(call()))
    for delta in (-0.5, 0.0, 0.5, 1.0, 1.5):
        for core, w in ((V.CORE_MLS, 10.0), (V.CORE_LCG, 3.5)):
            add("ARN delta %g W %g core %d" % (delta, w, core), setup(seed=0x400 + j, core=core, type_=V.ARN, width=w, delta=delta) + pieces(call(), whats[j % 8]))
            j += 1
    # ---- the MLS under init(): widths, seed 0, seeds beyond the active mask
    for n_bits in (1, 2, 23, 64):
        for seed in (0, 0xDEADBEEFCAFE):
            for type_ in (V.OVN, V.ARN):
                add("MLS of %d bits, seed %#x, %s" % (n_bits, seed, V.TYPES[type_]),
                    setup(seed=0x500 + j, n_bits=n_bits, mls_seed=seed, core=V.CORE_MLS, type_=type_, width=4.0) + pieces(call(), whats[j % 8]))
                j += 1
    add("MLS of 0 bits and of 200", setup(n_bits=0, mls_seed=7, core=V.CORE_MLS, width=3.0) + [(R.P_OVERWRITE, 300), (V.INIT, 5, 200, 1 << 40), (R.P_OVERWRITE, 800)])
    # ---- a second init with the seed equal to the current nState: nothing happens to the MLS; and one with another seed
    add("init again with the current nState", setup(core=V.CORE_MLS, width=5.0) + [(R.P_OVERWRITE, 300), (V.INIT_SAME, 0x99, 23), (R.P_ADD, 300),
                                                                                   (V.INIT_SAME, 0x9A, 24), (R.P_OVERWRITE, 250), (V.INIT, 0x9B, 24, 0x2F), (R.P_OVERWRITE, 250)])
    add("init twice before the first call", [(V.INIT, 1, 23, 5), (V.INIT, 2, 64, 0)] + setup(seed=3, n_bits=64, mls_seed=0, core=V.CORE_MLS)[1:] + pieces(1100))
    add("init and no MLS spike: bSync stays", setup(core=V.CORE_LCG) + pieces(1100))
    add("crushed MLS core leaves the MLS alone", setup(core=V.CORE_MLS, crush=0.5) + pieces(257))
    # ---- the edge draws
    for name, ops in edge_cases():
        add(name, ops)
    # ---- call patterns: one, two and three calls (the state words after each), a call is not the sum of shorter calls
    for type_ in range(4):
        for core in (V.CORE_MLS, V.CORE_LCG):
            three = [(R.P_ADD, 257), (R.P_OVERWRITE, 257), (R.P_MUL_INPLACE, 513)]
            for k in (1, 2, 3):
                add("%s core %d: %d calls" % (V.TYPES[type_], core, k), setup(seed=0x600 + type_, core=core, type_=type_, width=7.3, crush=0.4 if core and type_ > 1 else None) + three[:k])
    for type_ in range(4):
        add("%s add of 1100 with a source" % V.TYPES[type_], setup(seed=0x700, core=type_ % 2, type_=type_) + [(R.P_ADD, N)])
        add("%s add of 1100 with NULL" % V.TYPES[type_], setup(seed=0x700, core=type_ % 2, type_=type_) + [(V.P_ADD_NULL, N)])
    add("mul with NULL between two calls", setup(core=V.CORE_MLS) + [(R.P_OVERWRITE, 400), (V.P_MUL_NULL, 300), (R.P_MUL, 400)])
    for type_ in (V.OVN, V.OVNA, V.ARN):
        add("%s count smaller than W" % V.TYPES[type_], setup(seed=0x800, type_=type_, width=64.0, core=V.CORE_MLS) + pieces(7) [:40] + pieces(3, R.P_ADD)[:40])
    # ---- special values
    for A, off in ((0.0, 0.3), (-2.0, 0.1), (np.inf, 0.0), (1.0, -0.0), (-1.5, -0.0), (0.0, -0.0), (np.inf, -np.inf)):
        for type_ in (V.OVN, V.TRN):
            add("%s amplitude %g offset %g" % (V.TYPES[type_], A, off),
                setup(seed=0x900 + j, type_=type_, core=j % 2, amplitude=A, offset=off) + [(R.P_OVERWRITE, 300), (R.P_ADD, 300), (R.P_MUL_INPLACE, 500)])
            j += 1
    # (a type or a core outside its enum is an invalid enum load in the reference's build: not recorded; the device tests hold the
    # bank to the restatement there, which takes the switch's default: branches)
    return out


def write_cases(path, cs, src):
    with open(path, "wb") as f:
        f.write(np.array([len(cs), N], u32).tobytes())
        for c in cs:
            f.write(np.array([len(c["ops"])], u32).tobytes() + c["ops"].tobytes() + src.tobytes())


def read_results(path, cs):
    got = []
    with open(path, "rb") as f:
        for _ in cs:
            out = np.frombuffer(f.read(4 * N), f32)
            got.append(dict(out=out, words=np.frombuffer(f.read(8 * V.WORDS), u64)))
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


def run_reference(reference):
    cs, src = cases(), source_row()
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "driver.cpp"), "w") as f:
            f.write(DRIVER)
        san_exe = compile_driver(reference, d, os.path.join(d, "driver.cpp"), os.path.join(d, "ref_san"), SAN_FLAGS)
        exe = compile_driver(reference, d, os.path.join(d, "driver.cpp"), os.path.join(d, "ref"))
        san = run(san_exe, cs, src, d)                      # stand-alone, before anything is recorded
        got = run(exe, cs, src, d)
        keys = {l.split()[0]: l.split()[1:] for l in subprocess.check_output([san_exe, "keys"]).decode().splitlines()}
    for c, a, b in zip(cs, san, got):
        assert R.same(a["out"], b["out"]).all() and np.array_equal(a["words"], b["words"]), c["name"]
    names = {"noise/Velvet.h": public_names(os.path.join(reference, "include", "lsp-plug.in", "dsp-units", "noise", "Velvet.h"), "Velvet")}
    return cs, src, got, keys, names


def check_branches(cs, src, got):
    """What the cases are there for has happened in them."""
    by = {c["name"]: (c, g) for c, g in zip(cs, got)}
    roles = {}
    for c in cs:
        if "edge draws" in c["name"]:
            for role, raw in V.run_case(dict(ops=c["ops"], src=src))[1].drawn:
                if raw == 0 or raw >= 0xFFFFFF80:
                    roles.setdefault(role, set()).add(int(raw == 0))
    assert all(roles.get(r) == {0, 1} for r in "psct"), roles
    c, g = by["OVNA window 0 with rv 1 lands in window 1 and is replaced"]
    at = int(c["ops"][4][1])
    assert g["out"][at + 2] == -1.0 and g["out"][at] == 0.0 and g["out"][at + 1] == 0.0      # window 0's spike was +1, window 1's is -1
    a, b = by["OVN add of 1100 with a source"][1], by["OVN add of 1100 with NULL"][1]
    assert not np.array_equal(a["words"], b["words"])               # a call is not the sum of shorter calls
    c, g = by["init again with the current nState"]
    assert g["words"][17 + 7] == 0
    assert by["init and no MLS spike: bSync stays"][1]["words"][17 + 7] == 1 and by["crushed MLS core leaves the MLS alone"][1]["words"][17 + 7] == 1
    assert by["MLS of 0 bits and of 200"][1]["words"][17] == 64
    g = by["mul with NULL between two calls"][1]
    assert not g["out"][400:700].any() and not np.signbit(g["out"][400:700]).any()
    return len(cs)


def build(reference):
    cs, src, got, keys, names = run_reference(reference)
    check_branches(cs, src, got)
    arrs = {"src": src, "names": np.array([c["name"] for c in cs]), "ops_n": np.array([len(c["ops"]) for c in cs], u32),
            "ops": np.concatenate([c["ops"] for c in cs]), "out": np.array([g["out"] for g in got]), "words": np.array([g["words"] for g in got])}
    return npz_bytes(arrs), keys, names


def load(path=OUT):
    """The stored file as a list of cases: dicts of name, ops [k, 4], src [N], out [N], words [25]."""
    z = np.load(path)
    off = np.concatenate([[0], np.cumsum(z["ops_n"].astype(np.int64))])
    return [dict(name=str(z["names"][i]), ops=z["ops"][off[i]:off[i + 1]], src=z["src"], out=z["out"][i], words=z["words"][i])
            for i in range(len(z["names"]))]


def inventories(keys, names):
    layout = {"keys": keys["Velvet"], "sizeof": int(keys["sizeof"][0]), "offsetof": [int(v) for v in keys["offsetof"]]}
    return {"Velvet": layout}, names


if __name__ == "__main__":
    reference = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(ROOT), "reference")
    data, keys, names = build(reference)
    assert len(data) <= 400000, len(data)
    with open(OUT, "wb") as f:
        f.write(data)
    dump, names = inventories(keys, names)
    with open(os.path.join(HERE, "velvet_dump_keys.json"), "w") as f:
        json.dump(dump, f, indent=1)
        f.write("\n")
    with open(os.path.join(HERE, "velvet_public_names.json"), "w") as f:
        json.dump(names, f, indent=1)
        f.write("\n")
    print("%d cases, %d bytes" % (len(load()), len(data)))
