"""Writes tests/golden/dyndelay_ref_vectors.npz: what the reference's own DynamicDelay class computes on a list of cases, and next
to it dyndelay_public_names.json and dyndelay_dump_keys.json.  Data only: operation lists, the four input rows, the reference's
output, final heads and lines; names of public members; dump keys.  Run where the reference tree exists:

    python tests/golden/make_dyndelay_vectors.py [reference tree]

util/DynamicDelay.cpp (and iface/IStateDumper.cpp, which its dump() needs) are compiled unmodified into a temporary directory (-O2
-ffp-contract=off -msse2 -mfpmath=sse) against oracle/ref_shim plus a small overlay, written here, of what that shim lacks
(version.h, STATUS_NO_MEM, advance_ptr_bytes and swap).  The program -- a stand-alone one with its own main -- is built a first time with
-fsanitize=address,undefined and run on the same cases before anything is recorded.

Every case has two lines, A (max_size) and B (other_size; copy() goes between the two), an operation list ops [k, 2] (what, argument:
tests/dyndelay_ref.py names them) and four rows of N samples (in, delay, fgain, fdelay) that the process operations use up in order.
The file holds a pool of distinct rows (pool: [rows, N]) and case by case: names, sizes [2], row [4] (the pool's rows), ops, out [N],
head [2] and the two lines as dyndelay_ref.ring_part() cuts them: whole up to 8192 floats, else the 4096 positions behind the head.
All delay and fdelay rows are finite: what the reference leaves undefined is not recorded."""
import io
import json
import os
import subprocess
import sys
import tempfile
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)
from dyndelay_ref import (CLEAR_A, COPY_A_FROM_B, COPY_B_FROM_A, P_A, P_B, SET_HEAD_A, SET_HEAD_B, capacity_of, indices,  # noqa: E402
                          ring_part)
from make_bypass_crossfade_vectors import npz_bytes, public_names  # noqa: E402

OUT = os.path.join(HERE, "dyndelay_ref_vectors.npz")
f32 = np.float32

N = 1100                                        # more than a stretch of 0x400 samples, and a piece of 1023 with a rest
PIECES = (N, 1, 7, 256, 1023)
BIG = (1 << 23) + 3000                          # a line longer than 2^23 floats: tails there have no fraction bits left

OVERLAY_VERSION = r'''
#ifndef DYNDELAY_OVERLAY_VERSION_H_
#define DYNDELAY_OVERLAY_VERSION_H_
#include <lsp-plug.in/common/types.h>
#ifndef LSP_DSP_UNITS_PUBLIC
#define LSP_DSP_UNITS_PUBLIC
#endif
#endif
'''

# the shim's status.h, and the one more code that init() returns
OVERLAY_STATUS = r'''
#ifndef DYNDELAY_OVERLAY_STATUS_H_
#define DYNDELAY_OVERLAY_STATUS_H_
#include_next <lsp-plug.in/common/status.h>
namespace lsp
{
    enum { STATUS_NO_MEM = 5 };
}
#endif
'''

# the shim's alloc.h, and the two helpers of lsp-common-lib that DynamicDelay.cpp takes besides: what their names say
OVERLAY_ALLOC = r'''
#ifndef DYNDELAY_OVERLAY_ALLOC_H_
#define DYNDELAY_OVERLAY_ALLOC_H_
#include_next <lsp-plug.in/common/alloc.h>
namespace lsp
{
    template <class T, class P> inline T *advance_ptr_bytes(P * &ptr, size_t size)
    {
        T *res = reinterpret_cast<T *>(ptr);
        ptr = reinterpret_cast<P *>(reinterpret_cast<uint8_t *>(ptr) + size);
        return res;
    }
    template <class T> inline void swap(T &a, T &b) { T t = a; a = b; b = t; }
}
#endif
'''

# reads the cases, runs the class, writes out[n], the two heads and the two lines for every case; with "keys" as its only argument
# it prints the object's size and what dump() writes
DRIVER = r'''
#define private public
#define protected public
#include <lsp-plug.in/dsp-units/util/DynamicDelay.h>
#undef private
#undef protected
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
using namespace lsp;
struct keys: public dspu::IStateDumper
{
    std::string seen;
    void note(const char *n) { seen += " "; seen += n; }
    void write(const char *n, const void *) override    { note(n); }
    void write(const char *n, signed int) override      { note(n); }
    void write(const char *n, unsigned int) override    { note(n); }
    void write(const char *n, unsigned long) override   { note(n); }
    void write(const char *n, float) override           { note(n); }
};
// the whole line: the reference's own memory, or (LINE_ON_DEVICE: the same program on a class that keeps it elsewhere) a copy
static bool line(dspu::DynamicDelay &d, FILE *g)
{
#ifdef LINE_ON_DEVICE
    std::vector<float> v(d.nCapacity);
    if (!dspu::dynamic_delay_read_line(&d, v.data(), 0, v.size())) return false;
    return fwrite(v.data(), 4, v.size(), g) == v.size();
#else
    return fwrite(d.vDelay, 4, d.nCapacity, g) == d.nCapacity;
#endif
}
int main(int argc, char **argv)
{
    if (argc == 2 && strcmp(argv[1], "keys") == 0)
    {
        dspu::DynamicDelay d, e;
        if (d.init(5) != STATUS_OK || e.init(3000) != STATUS_OK) return 2;
        d.swap(&e);
        keys k;
        d.dump(&k);
        printf("sizeof %zu\nswap %zu %zu %zu %zu\ndyndelay%s\n", sizeof(d), d.max_delay(), d.capacity(), e.max_delay(), e.capacity(), k.seen.c_str());
        return 0;
    }
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb"), *g = fopen(argv[2], "wb");
    if (!f || !g) return 2;
    uint32_t hdr[2];
    if (fread(hdr, 4, 2, f) != 2) return 3;
    const uint32_t cases = hdr[0], n = hdr[1];
    std::vector<float> rows(size_t(n) * 4), out(n);
    for (uint32_t c = 0; c < cases; ++c)
    {
        uint32_t h[3];
        if (fread(h, 4, 3, f) != 3) return 3;
        std::vector<uint32_t> ops(2 * h[2]);
        if (fread(ops.data(), 4, ops.size(), f) != ops.size()) return 3;
        if (fread(rows.data(), 4, rows.size(), f) != rows.size()) return 3;
        std::fill(out.begin(), out.end(), 0.0f);
        dspu::DynamicDelay a, b;
        if (a.init(h[0]) != STATUS_OK || b.init(h[1]) != STATUS_OK) return 4;
        size_t at = 0;
        for (uint32_t k = 0; k < h[2]; ++k)
        {
            const uint32_t what = ops[2 * k], arg = ops[2 * k + 1];
            switch (what)
            {
                case 0: case 1:
                    if (at + arg > n) return 5;
                    (what == 0 ? a : b).process(&out[at], &rows[at], &rows[n + at], &rows[2 * size_t(n) + at], &rows[3 * size_t(n) + at], arg);
                    at += arg;
                    break;
                case 2: a.clear(); break;
                case 3: a.copy(&b); break;
                case 4: b.copy(&a); break;
                case 5: if (arg >= a.nCapacity) return 6; a.nHead = arg; break;
                case 6: if (arg >= b.nCapacity) return 6; b.nHead = arg; break;
                default: return 6;
            }
        }
        if (at != n) return 7;
        fwrite(out.data(), 4, n, g);
        const uint32_t tail[4] = { a.nHead, b.nHead, a.nCapacity, b.nCapacity };
        fwrite(tail, 4, 4, g);
        if (!line(a, g) || !line(b, g)) return 9;
    }
    fclose(f);
    return fclose(g) == 0 ? 0 : 8;
}
'''

FLAGS = ["-std=c++11", "-O2", "-ffp-contract=off", "-msse2", "-mfpmath=sse", "-DLSP_DSP_UNITS_BUILTIN", "-Wall"]
SAN_FLAGS = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]


def const(v):
    return np.full(N, v, f32)


def signals():
    """The rows that the cases share: two of noise, random gains, an input with Inf and NaN, subnormals."""
    rng = np.random.default_rng(2468)
    a = (rng.standard_normal(N) * 0.5).astype(f32)
    b = (rng.standard_normal(N) * 0.5).astype(f32)
    gains = rng.uniform(-0.95, 0.95, N).astype(f32)
    special = (rng.standard_normal(N) * 0.25).astype(f32)
    for at in (3, 130, 241, 650, 900, 1099):
        special[at] = np.inf if at % 2 else -np.inf
    for at in (1, 100, 600, 1000):
        special[at] = np.nan
    sub = (10.0 ** rng.uniform(np.log10(1.4e-45), -38.0, N) * rng.choice([-1.0, 1.0], N)).astype(np.float64).astype(f32)
    sub[::97] = 0.0
    return dict(a=a, b=b, gains=gains, special=special, sub=sub)


def pieces(call, n=N, what=P_A):
    ops, at = [], 0
    while at < n:
        k = min(call, n - at)
        ops.append((what, k))
        at += k
    return ops


def sine(centre, depth, period, phase=0.0):
    return (centre + depth * np.sin(2 * np.pi * (np.arange(N) / period + phase))).astype(f32)


def cases():
    s = signals()
    rng = np.random.default_rng(1357)
    out = []

    def add(name, max_size, ops, inp, delay, fgain, fdelay, other=0):
        rows = np.stack([np.asarray(r, f32) for r in (inp, delay, fgain, fdelay)])
        assert rows.shape == (4, N) and np.isfinite(rows[1]).all() and np.isfinite(rows[3]).all(), name
        out.append(dict(name=name, max_size=max_size, other_size=other, ops=np.array(ops, np.uint32).reshape(-1, 2), rows=rows))

    # the conflict classes: the distance between a step's feed and the tails of its neighbours decides what may run side by side
    i = 0
    for max_size, d in ((1000, 300.0), (40000, 39000.0), (5, 5.0)):
        for fd in ("0", "0.99", "1", "7", "63", "64", "delay"):
            row = const(d) if fd == "delay" else const(float(fd))
            call = PIECES[i % len(PIECES)]
            add("max %d delay %g fdelay %s calls of %d" % (max_size, d, fd, call), max_size, pieces(call), s["a"], const(d), const(0.5), row)
            i += 1
    # max_size 0: every step reads what it wrote
    add("max 0 gains random", 0, pieces(N), s["a"], s["b"] * 8, s["gains"], const(0.0))
    add("max 0 delay rows beyond", 0, pieces(256), s["b"], const(3.0), const(1.0), const(2.0))
    # heads that wrap during the call: 2048 floats for max_size 1000, 41984 for 40000
    add("max 1000 head wraps", 1000, [(SET_HEAD_A, capacity_of(1000) - 700)] + pieces(N), s["a"], const(1000.0), const(0.7), const(1000.0))
    add("max 1000 head wraps, sine, calls of 7", 1000, [(SET_HEAD_A, capacity_of(1000) - 700)] + pieces(7), s["a"], sine(500, 480, 400),
        s["gains"], sine(200, 190, 170, 0.3))
    add("max 40000 head wraps", 40000, [(SET_HEAD_A, capacity_of(40000) - 700)] + pieces(1023), s["b"], const(39990.0), const(-0.6),
        const(39990.0))
    add("max 40000 head wraps, small and large delays", 40000, [(SET_HEAD_A, capacity_of(40000) - 300)] + pieces(N), s["b"],
        np.where(np.arange(N) % 400 < 200, 50.0, 39000.0), s["gains"], np.where(np.arange(N) % 300 < 150, 0.0, 45000.0))
    # sine-modulated rows (a chorus) and random rows, with negative values and values beyond max_size among them
    for max_size in (1000, 40000):
        centre = max_size * 0.5
        add("max %d chorus" % max_size, max_size, pieces(N), s["a"], sine(centre, centre * 0.9, 523), const(0.4), sine(centre * 0.5, centre * 0.45, 311, 0.25))
        add("max %d chorus beyond the range" % max_size, max_size, pieces(256), s["b"], sine(centre, centre * 1.3, 401), s["gains"],
            sine(centre, centre * 1.5, 207, 0.1))
        add("max %d random rows" % max_size, max_size, pieces(1023), s["a"], rng.uniform(-0.2 * max_size, 1.2 * max_size, N), s["gains"],
            rng.uniform(-0.2 * max_size, 1.2 * max_size, N))
        add("max %d random rows, small feedback delays" % max_size, max_size, pieces(N), s["b"], rng.uniform(0, max_size, N), s["gains"],
            rng.uniform(-2, 9, N))
    add("max 5 random rows", 5, pieces(7), s["a"], rng.uniform(-2, 8, N), s["gains"], rng.uniform(-2, 8, N))
    add("max 1000 fast downward sweep", 1000, pieces(N), s["a"], np.maximum(1000.0 - 3.0 * np.arange(N), 0.0), const(0.5),
        np.maximum(1000.0 - 3.0 * np.arange(N), 0.0) * 0.5)
    # shift == 0: in + in * g
    add("max 1000 shift 0", 1000, pieces(N), s["a"], const(0.0), s["gains"], const(0.0))
    add("max 1000 shift 0 by a negative delay", 1000, pieces(256), s["a"], const(-3.5), const(1.0), const(4.0))
    add("max 1000 delay below one", 1000, pieces(N), s["b"], const(0.75), const(2.0), const(0.5))
    # fgain 0, -0, 1, beyond 1, Inf, NaN and subnormal; Inf and NaN in the input
    g = np.tile(np.array([0.0, -0.0, 1.0, 1.5, -2.5, 1e-40, -1e-42, 0.25], f32), N // 8 + 1)[:N].copy()
    add("max 1000 gains 0, -0, 1, beyond 1 and subnormal", 1000, pieces(N), s["a"], const(100.0), g, const(100.0))
    add("max 1000 gains 0 and -0 at fdelay 0", 1000, pieces(N), -np.abs(s["a"]), const(10.0), np.where(np.arange(N) % 2 == 0, 0.0, -0.0), const(0.0))
    g = s["gains"].copy()
    g[40], g[300], g[301], g[800] = np.inf, np.nan, -np.inf, np.nan
    add("max 1000 gains Inf and NaN", 1000, pieces(256), s["a"], const(64.0), g, const(64.0))
    add("max 40000 gains Inf and NaN", 40000, pieces(N), s["a"], const(20000.0), g, const(7.0))
    add("max 1000 Inf and NaN in the input", 1000, pieces(N), s["special"], const(50.0), const(0.5), const(50.0))
    add("max 40000 Inf and NaN in the input, fdelay 0", 40000, pieces(1023), s["special"], const(30.0), s["gains"], const(0.0))
    add("max 1000 subnormal input, subnormal gains", 1000, pieces(N), s["sub"], const(200.0), np.roll(s["sub"], 17), const(200.0))
    add("max 1000 subnormal input", 1000, pieces(N), s["sub"], const(20.0), const(0.5), const(0.0))
    # clear() in the middle
    add("max 1000 cleared at 500", 1000, pieces(500) [:1] + [(CLEAR_A, 0)] + [(P_A, N - 500)], s["a"], const(300.0), const(0.8), const(300.0))
    add("max 40000 cleared at 600, head moved first", 40000, [(SET_HEAD_A, 12345), (P_A, 600), (CLEAR_A, 0), (P_A, N - 600)], s["b"],
        const(256.0), const(0.8), const(128.0))
    # copy() between lines of equal and unequal capacity, in both directions, and from a wrapped source
    echo = (s["a"], const(180.0), const(0.6), const(180.0))
    add("copy to an equal line", 1000, [(P_B, 600), (COPY_A_FROM_B, 0), (P_A, N - 600)], *echo, other=1000)
    add("copy to a longer line", 40000, [(P_B, 600), (COPY_A_FROM_B, 0), (P_A, N - 600)], *echo, other=1000)
    add("copy to a shorter line", 1000, [(P_B, 600), (COPY_A_FROM_B, 0), (P_A, N - 600)], *echo, other=40000)
    add("copy from a wrapped line", 1000, [(SET_HEAD_B, capacity_of(1000) - 250), (P_B, 600), (COPY_A_FROM_B, 0), (P_A, N - 600)], *echo, other=1000)
    add("copy from a wrapped longer line", 1000, [(SET_HEAD_B, capacity_of(40000) - 250), (P_B, 600), (COPY_A_FROM_B, 0), (P_A, N - 600)], *echo,
        other=40000)
    add("copy from a wrapped shorter line", 40000, [(SET_HEAD_B, capacity_of(5) - 250), (P_B, 600), (COPY_A_FROM_B, 0), (P_A, N - 600)],
        s["a"], const(4.0), const(0.6), const(2.0), other=5)
    add("copy there and back", 1000, [(P_A, 300), (COPY_B_FROM_A, 0), (P_B, 300), (COPY_A_FROM_B, 0), (P_A, N - 600)], *echo, other=40000)
    add("copy from a fresh line", 1000, [(P_A, 700), (COPY_A_FROM_B, 0), (P_A, N - 700)], *echo, other=5)
    # the head beyond 2^23: the float32 sum of tail and a fractional fdelay is not tail + int(fdelay)
    add("head beyond 2^23, fractional fdelay", BIG, [(SET_HEAD_A, (1 << 23) + 1500)] + pieces(N), s["a"], const(40.0), const(0.5),
        np.tile(np.array([2.75, 3.5, 0.5, 7.75, 1.25, 2.5], f32), N // 6 + 1)[:N])
    add("head beyond 2^23, chorus", BIG, [(SET_HEAD_A, (1 << 23) + 2000)] + pieces(256), s["b"], sine(500, 480, 523), s["gains"],
        sine(250, 240.3, 311, 0.25))
    # ... and a head so far up under a longer delay that tail (wrapped) plus fdelay passes 2^24 and rounds to an even cell: at times
    # one past the head, where the next input lands on it
    add("feed index beyond 2^24", BIG, [(SET_HEAD_A, (1 << 23) - 2000)] + pieces(N), s["a"], const(float(BIG)), const(0.5), const(float(BIG)))
    return out


def run(exe, cs, cwd):
    src, dst = os.path.join(cwd, "cases.bin"), os.path.join(cwd, "results.bin")
    with open(src, "wb") as f:
        f.write(np.array([len(cs), N], np.uint32).tobytes())
        for c in cs:
            f.write(np.array([c["max_size"], c["other_size"], len(c["ops"])], np.uint32).tobytes() + c["ops"].tobytes() + c["rows"].tobytes())
    subprocess.run([exe, src, dst], check=True, timeout=900)
    got = []
    with open(dst, "rb") as f:
        for c in cs:
            out = np.frombuffer(f.read(4 * N), f32)
            ha, hb, ca, cb = np.frombuffer(f.read(16), np.uint32).tolist()
            assert (ca, cb) == (capacity_of(c["max_size"]), capacity_of(c["other_size"])), c["name"]
            la, lb = np.frombuffer(f.read(4 * ca), f32), np.frombuffer(f.read(4 * cb), f32)
            got.append(dict(out=out, head=np.array([ha, hb], np.uint32), ring_a=ring_part(la, ha), ring_b=ring_part(lb, hb)))
        assert f.read(1) == b""
    return got


def run_reference(reference):
    cs = cases()
    with tempfile.TemporaryDirectory() as d:
        for rel, text in (("lsp-plug.in/dsp-units/version.h", OVERLAY_VERSION), ("lsp-plug.in/common/alloc.h", OVERLAY_ALLOC),
                          ("lsp-plug.in/common/status.h", OVERLAY_STATUS)):
            os.makedirs(os.path.dirname(os.path.join(d, "overlay", rel)), exist_ok=True)
            with open(os.path.join(d, "overlay", rel), "w") as f:
                f.write(text)
        with open(os.path.join(d, "driver.cpp"), "w") as f:
            f.write(DRIVER)
        srcs = [os.path.join(d, "driver.cpp")] + [os.path.join(reference, "src", "main", n) for n in ("util/DynamicDelay.cpp", "iface/IStateDumper.cpp")]
        inc = ["-I" + os.path.join(d, "overlay"), "-I" + os.path.join(ROOT, "oracle", "ref_shim"), "-I" + os.path.join(reference, "include")]
        for exe, extra in (("ref_san", SAN_FLAGS), ("ref", [])):
            subprocess.check_call(["g++"] + FLAGS + extra + inc + ["-o", os.path.join(d, exe)] + srcs + ["-lm"])
        san = run(os.path.join(d, "ref_san"), cs, d)                # stand-alone, before anything is recorded
        got = run(os.path.join(d, "ref"), cs, d)
        keys = {l.split()[0]: l.split()[1:] for l in subprocess.check_output([os.path.join(d, "ref_san"), "keys"]).decode().splitlines()}
    for a, b in zip(san, got):
        assert all(np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)) for k in a)
    assert keys["sizeof"] == ["32"], keys["sizeof"]
    assert keys["swap"] == [str(v) for v in (3000, capacity_of(3000), 5, capacity_of(5))], keys["swap"]
    names = {"util/DynamicDelay.h": public_names(os.path.join(reference, "include", "lsp-plug.in", "dsp-units", "util", "DynamicDelay.h"),
                                                 "DynamicDelay")}
    return cs, got, keys, names


def check_branches(cs, got):
    """What the cases are there for has happened in them."""
    by = {c["name"]: (c, g) for c, g in zip(cs, got)}
    c, g = by["head beyond 2^23, fractional fdelay"]
    head = int(c["ops"][0][1])
    shift, tail, feed = indices(head, capacity_of(BIG), BIG, c["rows"][1], c["rows"][3])
    whole = tail + np.minimum(np.maximum(c["rows"][3], 0), shift).astype(np.int64)
    assert tail.min() >= 1 << 23 and np.count_nonzero(feed != whole) > N // 3, "the float32 feed index is integer arithmetic here"
    c, g = by["feed index beyond 2^24"]
    cap = capacity_of(BIG)
    shift, tail, feed = indices(int(c["ops"][0][1]), cap, BIG, c["rows"][1], c["rows"][3])
    h = (int(c["ops"][0][1]) + np.arange(N)) % cap
    assert np.count_nonzero((feed - h) % cap == 1) > 100, "no feed index was rounded past the head"
    c, g = by["max 1000 shift 0"]
    with np.errstate(all="ignore"):
        assert np.array_equal(g["out"], c["rows"][0] + c["rows"][0] * c["rows"][2]), "shift 0 is in + in * g"
    c, g = by["max 1000 head wraps"]
    assert g["head"][0] == (capacity_of(1000) - 700 + N) % capacity_of(1000) < 700
    c, g = by["copy to a longer line"]
    assert g["head"][0] == N - 600 and g["head"][1] == 600
    c, g = by["max 1000 gains Inf and NaN"]
    assert np.isnan(g["out"]).any() and np.isfinite(g["out"]).any()
    return len(cs)


def build(reference):
    cs, got, keys, names = run_reference(reference)
    check_branches(cs, got)
    pool, where = [], {}
    rows = []
    for c in cs:
        idx = []
        for r in c["rows"]:
            k = r.tobytes()
            if k not in where:
                where[k] = len(pool)
                pool.append(r)
            idx.append(where[k])
        rows.append(idx)
    arrs = {"pool": np.array(pool, f32), "names": np.array([c["name"] for c in cs]),
            "sizes": np.array([(c["max_size"], c["other_size"]) for c in cs], np.uint32), "row": np.array(rows, np.uint32),
            "ops_n": np.array([len(c["ops"]) for c in cs], np.uint32), "ops": np.concatenate([c["ops"] for c in cs]),
            "out": np.array([g["out"] for g in got]), "head": np.array([g["head"] for g in got]),
            "ring_n": np.array([(g["ring_a"].size, g["ring_b"].size) for g in got], np.uint32),
            "rings": np.concatenate([np.concatenate([g["ring_a"], g["ring_b"]]) for g in got])}
    return npz_bytes(arrs), keys, names


def load(path=OUT):
    """The stored file as a list of cases: dicts of name, max_size, other_size, ops, rows [4, N], out, head [2], ring_a, ring_b."""
    z = np.load(path)
    off = np.concatenate([[0], np.cumsum(z["ops_n"].astype(np.int64))])
    roff = np.concatenate([[0], np.cumsum(z["ring_n"].astype(np.int64).reshape(-1))])
    cs = []
    for i in range(len(z["names"])):
        cs.append(dict(name=str(z["names"][i]), max_size=int(z["sizes"][i][0]), other_size=int(z["sizes"][i][1]), ops=z["ops"][off[i]:off[i + 1]],
                       rows=z["pool"][z["row"][i]], out=z["out"][i], head=z["head"][i], ring_a=z["rings"][roff[2 * i]:roff[2 * i + 1]],
                       ring_b=z["rings"][roff[2 * i + 1]:roff[2 * i + 2]]))
    return cs


if __name__ == "__main__":
    data, keys, names = build(sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(ROOT), "reference"))
    assert len(data) < (1 << 20), len(data)
    with open(OUT, "wb") as f:
        f.write(data)
    with open(os.path.join(HERE, "dyndelay_dump_keys.json"), "w") as f:
        json.dump({"keys": keys["dyndelay"], "closes": []}, f, indent=1)
        f.write("\n")
    with open(os.path.join(HERE, "dyndelay_public_names.json"), "w") as f:
        json.dump(names, f, indent=1)
        f.write("\n")
    print("%d cases, %d bytes" % (len(load()), len(data)))
