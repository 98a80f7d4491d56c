"""Writes tests/golden/stereo_meter_ref_vectors.npz: what the reference's own Correlometer and Panometer classes compute on a
list of cases.  Data only: settings, inputs, the reference's outputs and final state.  Run where the reference tree exists:

    python tests/golden/make_stereo_meter_vectors.py [reference tree]

The two class sources (and iface/IStateDumper.cpp, which their dump() needs) are compiled unmodified into a temporary directory (-O2 -ffp-contract=off -msse2 -mfpmath=sse) against
oracle/ref_shim plus a small overlay, written here, of the helper names that shim lacks.  lsp-dsp-lib is not part of the
reference tree: dsp::corr_init, dsp::corr_incr, dsp::h_sum and dsp::sqr2 are this file's own serial stand-ins (every product
and every sum rounds once, sums from 0, oldest first), and CORR_THRESHOLD is upstream knowledge of corr_incr (DESIGN.md
section 4).  The program is built a second time with -fsanitize=address,undefined and run stand-alone on the same cases before
anything is recorded.

The file holds a, b (the signal every case runs), and case by case: names, kind (0 Correlometer, 1 Panometer), max_period,
ops [k, 2] (OPS: what, argument), out [n] and state [5] (uint32: v, a, b or va, vb, 0 as bits, then nHead, nWindow)."""
import io
import os
import subprocess
import sys
import tempfile
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "stereo_meter_ref_vectors.npz")
f32 = np.float32

N = 3200
MAX_PERIOD = 480
SILENCE = (1000, 2000)                          # both channels: longer than two periods, so a refresh finds only zeros
B_SILENT = (2300, 2600)                         # only b
PERIODS = (1, 7, 255, 256, 257, 480)
OP_SET_PERIOD, OP_CLEAR, OP_PROCESS, OP_SET_LAW, OP_SET_DEFAULT = range(5)
CORRELOMETER, PANOMETER = range(2)
LINEAR, EQUAL_POWER = range(2)

OVERLAY_ALLOC = r'''
#ifndef STEREO_METER_OVERLAY_ALLOC_H_
#define STEREO_METER_OVERLAY_ALLOC_H_
#include_next <lsp-plug.in/common/alloc.h>
namespace lsp
{
    inline size_t align_size(size_t size, size_t align)     { return (size + align - 1) / align * align; }
    template <class T> inline T *advance_ptr_bytes(uint8_t * &ptr, size_t bytes)
    {
        T *res = reinterpret_cast<T *>(ptr);
        ptr += bytes;
        return res;
    }
    template <class A, class B> inline A lsp_min(A a, B b)  { return (a < A(b)) ? a : A(b); }
    template <class A, class B, class C, class D> inline A lsp_min(A a, B b, C c, D d)
    {
        return lsp_min(lsp_min(a, A(b)), lsp_min(A(c), A(d)));
    }
}
#endif
'''

OVERLAY_STATUS = r'''
#ifndef STEREO_METER_OVERLAY_STATUS_H_
#define STEREO_METER_OVERLAY_STATUS_H_
#include_next <lsp-plug.in/common/status.h>
namespace lsp
{
    enum { STATUS_NO_MEM = 5 };
}
#endif
'''

OVERLAY_DSP = r'''
#ifndef STEREO_METER_OVERLAY_DSP_H_
#define STEREO_METER_OVERLAY_DSP_H_
#include_next <lsp-plug.in/dsp/dsp.h>
#include <math.h>
namespace lsp
{
    namespace dsp
    {
        static const float CORR_THRESHOLD = 1e-10f;
        typedef struct correlation_t { float v, a, b; } correlation_t;
        inline void corr_init(correlation_t *corr, const float *a, const float *b, size_t count)
        {
            float xv = 0.0f, xa = 0.0f, xb = 0.0f;
            for (size_t i = 0; i < count; ++i)
            {
                xv += a[i] * b[i];
                xa += a[i] * a[i];
                xb += b[i] * b[i];
            }
            corr->v += xv;
            corr->a += xa;
            corr->b += xb;
        }
        inline void corr_incr(correlation_t *corr, float *dst, const float *a_head, const float *b_head, const float *a_tail,
                              const float *b_tail, size_t count)
        {
            float vv = corr->v, va = corr->a, vb = corr->b;
            for (size_t i = 0; i < count; ++i)
            {
                const float ah = a_head[i], bh = b_head[i], at = a_tail[i], bt = b_tail[i];
                vv += ah * bh - at * bt;
                va += ah * ah - at * at;
                vb += bh * bh - bt * bt;
                const float d = va * vb;
                dst[i] = (d >= CORR_THRESHOLD) ? vv / sqrtf(d) : 0.0f;
            }
            corr->v = vv;
            corr->a = va;
            corr->b = vb;
        }
        inline float h_sum(const float *src, size_t count)
        {
            float s = 0.0f;
            for (size_t i = 0; i < count; ++i)
                s += src[i];
            return s;
        }
        inline void sqr2(float *dst, const float *src, size_t count)
        {
            for (size_t i = 0; i < count; ++i)
                dst[i] = src[i] * src[i];
        }
    }
}
#endif
'''

# reads the cases, runs the classes, writes out[n] and five state words per case; the fields are read by name
DRIVER = r'''
#define private public
#include <lsp-plug.in/dsp-units/meters/Correlometer.h>
#include <lsp-plug.in/dsp-units/meters/Panometer.h>
#undef private
#include <cstdio>
#include <cstring>
#include <vector>
using namespace lsp;
static uint32_t bits(float v) { uint32_t u; memcpy(&u, &v, 4); return u; }
static float flt(uint32_t u) { float v; memcpy(&v, &u, 4); return v; }
int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb"), *g = fopen(argv[2], "wb");
    if (!f || !g) return 2;
    uint32_t hdr[2];
    if (fread(hdr, 4, 2, f) != 2) return 3;
    const uint32_t cases = hdr[0], n = hdr[1];
    std::vector<float> a(n), b(n), out(n);
    if (fread(a.data(), 4, n, f) != n || fread(b.data(), 4, n, f) != n) return 3;
    for (uint32_t c = 0; c < cases; ++c)
    {
        uint32_t h[3];
        if (fread(h, 4, 3, f) != 3) return 3;
        std::vector<uint32_t> ops(2 * h[2]);
        if (fread(ops.data(), 4, ops.size(), f) != ops.size()) return 3;
        dspu::Correlometer cm;
        dspu::Panometer pm;
        const bool pan = h[0] == 1;
        if ((pan ? pm.init(h[1]) : cm.init(h[1])) != STATUS_OK) return 4;
        size_t at = 0;
        for (uint32_t k = 0; k < h[2]; ++k)
        {
            const uint32_t what = ops[2 * k], arg = ops[2 * k + 1];
            switch (what)
            {
                case 0: if (pan) pm.set_period(arg); else cm.set_period(arg); break;
                case 1: if (pan) pm.clear(); else cm.clear(); break;
                case 2:
                    if (at + arg > n) return 5;
                    if (pan) pm.process(&out[at], &a[at], &b[at], arg); else cm.process(&out[at], &a[at], &b[at], arg);
                    at += arg;
                    break;
                case 3: pm.set_pan_law(arg == 0 ? dspu::PAN_LAW_LINEAR : dspu::PAN_LAW_EQUAL_POWER); break;
                case 4: pm.set_default_pan(flt(arg)); break;
                default: return 6;
            }
        }
        if (at != n) return 7;
        fwrite(out.data(), 4, n, g);
        const uint32_t st[5] = { pan ? bits(pm.fValueA) : bits(cm.sCorr.v), pan ? bits(pm.fValueB) : bits(cm.sCorr.a),
                                 pan ? 0u : bits(cm.sCorr.b), pan ? pm.nHead : cm.nHead, pan ? pm.nWindow : cm.nWindow };
        fwrite(st, 4, 5, g);
    }
    fclose(f);
    return fclose(g) == 0 ? 0 : 8;
}
'''

FLAGS = ["-std=c++11", "-O2", "-ffp-contract=off", "-msse2", "-mfpmath=sse", "-DLSP_DSP_UNITS_BUILTIN", "-Wall"]
SAN_FLAGS = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]


def signal():
    """A correlated pair whose level steps between 1 and 1e-3, silence in both, then silence in b alone."""
    rng = np.random.default_rng(1770)
    level = np.where((np.arange(N) // 97) % 3 == 1, 1e-3, 1.0)
    a = rng.standard_normal(N) * level
    b = 0.6 * a + 0.8 * rng.standard_normal(N) * level
    a[SILENCE[0]:SILENCE[1]] = 0.0
    b[SILENCE[0]:SILENCE[1]] = 0.0
    b[B_SILENT[0]:B_SILENT[1]] = 0.0
    return a.astype(f32), b.astype(f32)


def ops_of(first, call, events=()):
    """first: the setters before the first sample; events: (sample, [ops]) later on; the samples between in calls of `call`."""
    ops, at = list(first), 0
    for stop, more in list(events) + [(N, [])]:
        while at < stop:
            k = min(call, stop - at)
            ops.append((OP_PROCESS, k))
            at += k
        ops += more
    return np.array(ops, np.uint32).reshape(-1, 2)


def bits(v):
    return int(f32(v).view(np.uint32))


def cases():
    out = []
    for i, p in enumerate(PERIODS):
        out.append(("correlometer period %d" % p, CORRELOMETER, ops_of([(OP_SET_PERIOD, p)], N)))
        law = (LINEAR, EQUAL_POWER)[i % 2]
        out.append(("panometer period %d law %d" % (p, law), PANOMETER, ops_of([(OP_SET_PERIOD, p), (OP_SET_LAW, law)], N)))
    for call in (1, 113):
        out.append(("correlometer period 257 in calls of %d" % call, CORRELOMETER, ops_of([(OP_SET_PERIOD, 257)], call)))
        for law in (LINEAR, EQUAL_POWER):
            out.append(("panometer period 257 law %d in calls of %d" % (law, call), PANOMETER,
                        ops_of([(OP_SET_PERIOD, 257), (OP_SET_LAW, law)], call)))
    change = [(700, [(OP_SET_PERIOD, 100)]), (2700, [(OP_SET_PERIOD, 9999)])]             # the second one clamped to 480
    out.append(("correlometer period 257, 100, 480", CORRELOMETER, ops_of([(OP_SET_PERIOD, 257)], 113, change)))
    out.append(("panometer period 257, 100, 480", PANOMETER, ops_of([(OP_SET_PERIOD, 257), (OP_SET_LAW, LINEAR)], 113, change)))
    clear = [(600, [(OP_CLEAR, 0)]), (2450, [(OP_CLEAR, 0)])]
    out.append(("correlometer clear()", CORRELOMETER, ops_of([(OP_SET_PERIOD, 255)], 113, clear)))
    out.append(("panometer clear()", PANOMETER, ops_of([(OP_SET_PERIOD, 255)], 113, clear)))
    out.append(("panometer default 0.25", PANOMETER, ops_of([(OP_SET_PERIOD, 40), (OP_SET_DEFAULT, bits(0.25))], N)))
    out.append(("panometer default -1 linear", PANOMETER,
                ops_of([(OP_SET_PERIOD, 40), (OP_SET_LAW, LINEAR), (OP_SET_DEFAULT, bits(-1.0))], 113)))
    return out


def run(exe, a, b, cs, cwd):
    src, dst = os.path.join(cwd, "cases.bin"), os.path.join(cwd, "results.bin")
    with open(src, "wb") as f:
        f.write(np.array([len(cs), N], np.uint32).tobytes() + a.tobytes() + b.tobytes())
        for name, kind, ops in cs:
            f.write(np.array([kind, MAX_PERIOD, len(ops)], np.uint32).tobytes() + ops.tobytes())
    subprocess.run([exe, src, dst], check=True, timeout=600)
    raw = np.fromfile(dst, np.uint32)
    assert raw.size == len(cs) * (N + 5), raw.size
    raw = raw.reshape(len(cs), N + 5)
    return raw[:, :N].view(f32).copy(), raw[:, N:].copy()


def run_reference(reference):
    a, b = signal()
    cs = cases()
    with tempfile.TemporaryDirectory() as d:
        for rel, text in (("lsp-plug.in/common/alloc.h", OVERLAY_ALLOC), ("lsp-plug.in/common/status.h", OVERLAY_STATUS),
                          ("lsp-plug.in/dsp/dsp.h", OVERLAY_DSP)):
            os.makedirs(os.path.dirname(os.path.join(d, "overlay", rel)), exist_ok=True)
            with open(os.path.join(d, "overlay", rel), "w") as f:
                f.write(text)
        with open(os.path.join(d, "driver.cpp"), "w") as f:
            f.write(DRIVER)
        srcs = [os.path.join(d, "driver.cpp")] + [os.path.join(reference, "src", "main", n) for n in ("meters/Correlometer.cpp", "meters/Panometer.cpp", "iface/IStateDumper.cpp")]
        inc = ["-I" + os.path.join(d, "overlay"), "-I" + os.path.join(ROOT, "oracle", "ref_shim"), "-I" + os.path.join(reference, "include")]
        for exe, extra in (("ref_san", SAN_FLAGS), ("ref", [])):
            subprocess.check_call(["g++"] + FLAGS + extra + inc + ["-o", os.path.join(d, exe)] + srcs + ["-lm"])
        san_out, san_state = run(os.path.join(d, "ref_san"), a, b, cs, d)      # stand-alone, before anything is recorded
        out, state = run(os.path.join(d, "ref"), a, b, cs, d)
    assert np.array_equal(out.view(np.uint32), san_out.view(np.uint32)) and np.array_equal(state, san_state)
    return a, b, cs, out, state


def check_branches(cs, out):
    """Every case contains the silence: the Correlometer's zero branch and the Panometer's default branch are each taken and each
    not taken."""
    inside = slice(SILENCE[1] - 50, SILENCE[1])             # a refresh over zeros has happened by then in every case
    for (name, kind, ops), o in zip(cs, out):
        assert np.all(np.isfinite(o)), name
        if kind == CORRELOMETER:
            assert np.all(o[inside] == 0.0) and np.any(o[:SILENCE[0]] != 0.0), name
        else:
            dfl = [f32(0.5)] + [np.uint32(arg).view(f32) for what, arg in ops if what == OP_SET_DEFAULT]
            assert np.all(o[inside] == dfl[-1]) and np.any(o[:SILENCE[0]] != dfl[-1]), name
    return int((out[0] == 0.0).sum())


def npz_bytes(arrs):
    """An .npz without time stamps: the same arrays give the same bytes."""
    b = io.BytesIO()
    with zipfile.ZipFile(b, "w") as z:
        for name in sorted(arrs):
            a = io.BytesIO()
            np.lib.format.write_array(a, np.ascontiguousarray(arrs[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, a.getvalue(), compresslevel=9)
    return b.getvalue()


def build_bytes(reference):
    a, b, cs, out, state = run_reference(reference)
    zeros = check_branches(cs, out)
    arrs = {"a": a, "b": b, "names": np.array([c[0] for c in cs]), "kind": np.array([c[1] for c in cs], np.uint32),
            "max_period": np.full(len(cs), MAX_PERIOD, np.uint32), "ops_n": np.array([len(c[2]) for c in cs], np.uint32),
            "ops": np.concatenate([c[2] for c in cs]), "out": out, "state": state}
    return npz_bytes(arrs), zeros


def load(path=OUT):
    """The stored file as (a, b, cases): dicts of name, kind, max_period, ops, out, state."""
    z = np.load(path)
    off = np.concatenate([[0], np.cumsum(z["ops_n"].astype(np.int64))])
    cs = [dict(name=str(z["names"][i]), kind=int(z["kind"][i]), max_period=int(z["max_period"][i]), ops=z["ops"][off[i]:off[i + 1]],
               out=z["out"][i], state=z["state"][i]) for i in range(len(z["names"]))]
    return z["a"], z["b"], cs


if __name__ == "__main__":
    data, zeros = build_bytes(sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(ROOT), "reference"))
    with open(OUT, "wb") as f:
        f.write(data)
    print("%d cases, %d bytes; the first case's correlation is 0 at %d of %d samples" % (len(load()[2]), len(data), zeros, N))
