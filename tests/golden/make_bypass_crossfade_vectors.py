"""Writes tests/golden/bypass_crossfade_ref_vectors.npz: what the reference's own Bypass and Crossfade classes compute on a list of
cases, and next to it bypass_crossfade_public_names.json, bypass_dump_keys.json and crossfade_dump_keys.json.  Data only: operation
lists, inputs, the reference's outputs, answers and final state; names of public members; dump keys.  Run where the reference
tree exists:

    python tests/golden/make_bypass_crossfade_vectors.py [reference tree]

The two class sources (and iface/IStateDumper.cpp, which their dump() needs) are compiled unmodified into a temporary directory
(-O2 -ffp-contract=off -msse2 -mfpmath=sse) against oracle/ref_shim plus a small overlay, written here, of what that shim lacks
(version.h, dsp::fill_zero and dsp::mul_k3 where they are missing).  The program -- a stand-alone one with its own main -- is built
a first time with -fsanitize=address,undefined and run on the same cases before anything is recorded.

The file holds the signals (x: [signals, N]) and case by case: names, kind (0 Bypass, 1 Crossfade), signal [2] (the rows of x
that are dry | fade_out and wet | fade_in), ops [k, 5] (what, argument, flags, two floats' bits: tests/bypass_crossfade_ref.py
names them), out [N], answers [k] (what set_bypass and toggle returned, 0 for every other operation) and state [4] (uint32).
Bypass: nState, fDelta's bits, fGain's bits, 0.  Crossfade: nSamples, nCounter, fDelta's bits, fGain's bits."""
import io
import json
import os
import re
import subprocess
import sys
import tempfile
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from bypass_crossfade_ref import (B_INIT, B_PROCESS, B_PROCESS_DRYWET, B_PROCESS_WET, B_SET_BYPASS, B_SET_FIELDS, BYPASS, CROSSFADE,  # noqa: E402
                                  HAS_A, HAS_B, S_ACTIVE, S_OFF, S_ON, X_INIT, X_PROCESS, X_RESET, X_TOGGLE, bits)

OUT = os.path.join(HERE, "bypass_crossfade_ref_vectors.npz")
f32 = np.float32

N = 1200
LENGTHS = (1, 2, 7, 240, 300, 5000)             # sample_rate * time
CALLS = (N, 1, 7, 256, 936)
GAINS = (0.0, 1.0, -0.5, 1e-30)
NOISE_A, NOISE_B, SUBNORMAL, SPECIAL = range(4)
QUIET_NAN, SIGNALLING_NAN = 0x7fc12345, 0x7f812345

OVERLAY_VERSION = r'''
#ifndef BYPASS_CROSSFADE_OVERLAY_VERSION_H_
#define BYPASS_CROSSFADE_OVERLAY_VERSION_H_
#include <lsp-plug.in/common/types.h>
#ifndef LSP_DSP_UNITS_PUBLIC
#define LSP_DSP_UNITS_PUBLIC
#endif
#endif
'''

# the shim's dsp.h, and the array primitives of the two classes that it lacks: plain loops of what their names say
OVERLAY_DSP = r'''
#ifndef BYPASS_CROSSFADE_OVERLAY_DSP_H_
#define BYPASS_CROSSFADE_OVERLAY_DSP_H_
#include_next <lsp-plug.in/dsp/dsp.h>
namespace lsp
{
    namespace dsp
    {
        %s
    }
}
#endif
'''
OVERLAY_MUL_K3 = "inline void mul_k3(float *dst, const float *src, float k, size_t count) { for (size_t i = 0; i < count; ++i) dst[i] = src[i] * k; }"
OVERLAY_FILL_ZERO = "inline void fill_zero(float *dst, size_t count) { for (size_t i = 0; i < count; ++i) dst[i] = 0.0f; }"

# reads the cases, runs the classes, writes out[n], four state words and an answer per operation for every case; with "keys"
# as its only argument it prints the two sizes and what dump() writes
DRIVER = r'''
#define private public
#define protected public
#include <lsp-plug.in/dsp-units/ctl/Bypass.h>
#include <lsp-plug.in/dsp-units/ctl/Crossfade.h>
#undef private
#undef protected
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
using namespace lsp;
static uint32_t bits(float v) { uint32_t u; memcpy(&u, &v, 4); return u; }
static float flt(uint32_t u) { float v; memcpy(&v, &u, 4); return v; }
struct keys: public dspu::IStateDumper
{
    std::string seen;
    void note(const char *n) { seen += " "; seen += n; }
    void write(const char *n, signed int) override      { note(n); }
    void write(const char *n, unsigned int) override    { note(n); }
    void write(const char *n, unsigned long) override   { note(n); }
    void write(const char *n, float) override           { note(n); }
};
int main(int argc, char **argv)
{
    if (argc == 2 && strcmp(argv[1], "keys") == 0)
    {
        dspu::Bypass b;
        dspu::Crossfade c;
        keys kb, kc;
        b.dump(&kb);
        c.dump(&kc);
        printf("sizeof %zu %zu\nbypass%s\ncrossfade%s\n", sizeof(b), sizeof(c), kb.seen.c_str(), kc.seen.c_str());
        return 0;
    }
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb"), *g = fopen(argv[2], "wb");
    if (!f || !g) return 2;
    uint32_t hdr[3];
    if (fread(hdr, 4, 3, f) != 3) return 3;
    const uint32_t cases = hdr[0], n = hdr[1], signals = hdr[2];
    std::vector<float> x(size_t(n) * signals), out(n);
    if (fread(x.data(), 4, x.size(), f) != x.size()) return 3;
    for (uint32_t c = 0; c < cases; ++c)
    {
        uint32_t h[4];
        if (fread(h, 4, 4, f) != 4) return 3;
        std::vector<uint32_t> ops(5 * h[3]), answers(h[3], 0);
        if (fread(ops.data(), 4, ops.size(), f) != ops.size()) return 3;
        if (h[1] >= signals || h[2] >= signals) return 4;
        const float *a = &x[size_t(n) * h[1]], *b = &x[size_t(n) * h[2]];
        std::fill(out.begin(), out.end(), 0.0f);
        dspu::Bypass bp;
        dspu::Crossfade xf;
        size_t at = 0;
        for (uint32_t k = 0; k < h[3]; ++k)
        {
            const uint32_t what = ops[5 * k], arg = ops[5 * k + 1], flags = ops[5 * k + 2], u = ops[5 * k + 3], v = ops[5 * k + 4];
            const bool sample_op = (h[0] == 0) ? what >= 3 : what == 3;
            if (sample_op && at + arg > n) return 5;
            const float *ra = (flags & 1) ? &a[at] : NULL, *rb = (flags & 2) ? &b[at] : NULL;
            if (h[0] == 0)
            {
                switch (what)
                {
                    case 0: bp.init(int(arg), flt(u)); break;
                    case 1: answers[k] = bp.set_bypass(arg != 0) ? 1 : 0; break;
                    case 2: bp.nState = dspu::Bypass::state_t(flags); bp.fDelta = flt(u); bp.fGain = flt(v); break;
                    case 3: bp.process(&out[at], ra, rb, arg); break;
                    case 4: bp.process_wet(&out[at], ra, rb, flt(u), arg); break;
                    case 5: bp.process_drywet(&out[at], ra, rb, flt(v), flt(u), arg); break;
                    default: return 6;
                }
            }
            else
            {
                switch (what)
                {
                    case 0: xf.init(int(arg), flt(u)); break;
                    case 1: answers[k] = xf.toggle() ? 1 : 0; break;
                    case 2: xf.reset(); break;
                    case 3: xf.process(&out[at], ra, rb, arg); break;
                    default: return 6;
                }
            }
            if (sample_op)
                at += arg;
        }
        if (at != n) return 7;
        fwrite(out.data(), 4, n, g);
        uint32_t st[4];
        if (h[0] == 0)
            st[0] = uint32_t(bp.nState), st[1] = bits(bp.fDelta), st[2] = bits(bp.fGain), st[3] = 0;
        else
            st[0] = uint32_t(xf.nSamples), st[1] = uint32_t(xf.nCounter), st[2] = bits(xf.fDelta), st[3] = bits(xf.fGain);
        fwrite(st, 4, 4, g);
        fwrite(answers.data(), 4, answers.size(), g);
    }
    fclose(f);
    return fclose(g) == 0 ? 0 : 8;
}
'''

FLAGS = ["-std=c++11", "-O2", "-ffp-contract=off", "-msse2", "-mfpmath=sse", "-DLSP_DSP_UNITS_BUILTIN", "-Wall"]
SAN_FLAGS = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]


def signals():
    rng = np.random.default_rng(4321)
    a = (rng.standard_normal(N) * 0.5).astype(f32)
    b = (rng.standard_normal(N) * 0.5).astype(f32)
    # subnormals from the smallest one up to just below the smallest normal, both signs, and a few exact zeros
    sub = (10.0 ** rng.uniform(np.log10(1.4e-45), -38.0, N) * rng.choice([-1.0, 1.0], N)).astype(np.float64).astype(f32)
    sub[::97] = 0.0
    sub[5], sub[6] = f32(1.4e-45), f32(-1.4e-45)
    special = (rng.standard_normal(N) * 0.25).astype(f32)
    for at in (0, 3, 130, 241, 299, 650, 655, 900, 1199):
        special[at] = np.inf if at % 2 else -np.inf
    for at in (1, 100, 239, 600, 620, 1000):
        special[at] = np.nan
    special = special.view(np.uint32)
    special[50], special[700], special[1100] = QUIET_NAN, SIGNALLING_NAN, QUIET_NAN | 0x80000000    # payloads a copy has to keep
    special[320], special[1150] = SIGNALLING_NAN, QUIET_NAN
    return np.stack([a, b, sub, special.view(f32)]).astype(f32)


def ops_of(first, call, events, process):
    """first: the operations before the first sample; events: (sample, [ops]) later on; the samples between in calls of `call`
    (a number, or a list of call lengths that is used up first).  process: the operation of a call without its count."""
    ops, at = list(first), 0
    cuts = list(call) if isinstance(call, (list, tuple)) else []
    size = call if not cuts else N
    for stop, more in list(events) + [(N, [])]:
        while at < stop:
            k = min(cuts.pop(0) if cuts else size, stop - at)
            ops.append((process[0], k) + tuple(process[1:]))
            at += k
        ops.extend(more)
    return np.array(ops, np.uint32).reshape(-1, 5)


def b_init(length):
    return (B_INIT, 48000, 0, bits(0.005), 0) if length == 240 else (B_INIT, length, 0, bits(1.0), 0)


def b_switch(on):
    return (B_SET_BYPASS, 1 if on else 0, 0, 0, 0)


def b_fields(state, delta, gain):
    return (B_SET_FIELDS, 0, state, bits(delta), bits(gain))


def b_process(variant, dry, wet_gain=1.0, dry_gain=1.0):
    """(what, flags, wet gain, dry gain): ops_of() puts the count in"""
    return (variant, (HAS_A if dry else 0) | HAS_B, bits(wet_gain), bits(dry_gain))


def x_init(length):
    return (X_INIT, 48000, 0, bits(0.005), 0) if length == 240 else (X_INIT, length, 0, bits(1.0), 0)


X_TOG, X_RES = (X_TOGGLE, 0, 0, 0, 0), (X_RESET, 0, 0, 0, 0)


def x_process(fade_out, fade_in):
    return (X_PROCESS, (HAS_A if fade_out else 0) | (HAS_B if fade_in else 0), 0, 0)


def ramp_steps(length):
    """How many samples init(length) ramps down for: the serial float32 sum decides, not a division."""
    delta, g, k = f32(-1.0) / f32(length), f32(1.0), 0
    while g > 0:
        g, k = f32(g + delta), k + 1
    return k


def cases():
    out = []
    variants = [(B_PROCESS, True), (B_PROCESS, False), (B_PROCESS_WET, True), (B_PROCESS_WET, False), (B_PROCESS_DRYWET, True),
                (B_PROCESS_DRYWET, False)]
    # down from sample 0 and up again from sample 600 (a ramp of 5000 is turned round half-way), every variant with three lengths
    i = 0
    for li, length in enumerate(LENGTHS):
        for vi in range(3):
            what, dry = variants[2 * vi + (li + vi) % 2]
            wg, dg = GAINS[i % 4], GAINS[(i // 2 + 1) % 4]
            call = CALLS[i % len(CALLS)]
            name = "bypass %s%s ramp %d calls of %d gains %g %g" % (("process", "process_wet", "process_drywet")[what - B_PROCESS],
                                                                     " dry" if dry else "", length, call, wg, dg)
            out.append((name, BYPASS, (NOISE_A, NOISE_B),
                        ops_of([b_init(length), b_switch(True)], call, [(600, [b_switch(False)])], b_process(what, dry, wg, dg))))
            i += 1
    out.append(("bypass ramp 5000 in calls of 936", BYPASS, (NOISE_A, NOISE_B),
                ops_of([b_init(5000), b_switch(True)], 936, [], b_process(B_PROCESS_WET, True, 0.75))))
    out.append(("bypass ramp 300 in calls of 936", BYPASS, (NOISE_A, NOISE_B),
                ops_of([b_init(300), b_switch(True)], 936, [], b_process(B_PROCESS_DRYWET, True, 0.75, 0.5))))
    k = ramp_steps(240)
    # the ramp ends on the last sample of a call, and the next call clamps; then on the last sample of the block: nothing clamps
    out.append(("bypass ramp 240 ends with a call", BYPASS, (NOISE_A, NOISE_B),
                ops_of([b_init(240), b_switch(True)], [k, 100, N], [], b_process(B_PROCESS, True))))
    out.append(("bypass ramp 240 ends with the block", BYPASS, (NOISE_A, NOISE_B),
                ops_of([b_init(240)], N, [(N - k, [b_switch(True)])], b_process(B_PROCESS_DRYWET, True, 0.75, 0.5))))
    out.append(("bypass ramp 240 one sample short of the call", BYPASS, (NOISE_A, NOISE_B),
                ops_of([b_init(240), b_switch(True)], [k + 1, N], [], b_process(B_PROCESS_WET, True, 0.75))))
    turn = [(100, [b_switch(False)]), (130, [b_switch(False)]), (500, [b_switch(True), b_switch(True)]), (560, [b_switch(False)])]
    out.append(("bypass ramp 240 turned round half-way, and switches that change nothing", BYPASS, (NOISE_A, NOISE_B),
                ops_of([b_init(240), b_switch(False), b_switch(True)], 113, turn, b_process(B_PROCESS, True))))
    out.append(("bypass ramp below one sample", BYPASS, (NOISE_A, NOISE_B),
                ops_of([(B_INIT, 48000, 0, bits(0.0), 0), b_switch(True)], 256, [(600, [b_switch(False)])], b_process(B_PROCESS, True))))
    never = [(300, [b_switch(False)]), (600, [b_switch(False)]), (900, [b_switch(True)])]
    out.append(("bypass never initialised", BYPASS, (NOISE_A, NOISE_B), ops_of([], 256, never, b_process(B_PROCESS, True))))
    out.append(("bypass never initialised, switched first, no dry", BYPASS, (NOISE_A, NOISE_B),
                ops_of([b_switch(True)], 256, never, b_process(B_PROCESS_WET, False, -0.5))))
    odd = [(200, [b_fields(S_ACTIVE, np.nan, 0.5)]), (400, [b_fields(S_ACTIVE, 0.01, np.nan)]), (600, [b_fields(S_OFF, 0.01, 1.5)]),
           (800, [b_fields(S_ON, -np.inf, 0.25)]), (1000, [b_fields(S_ACTIVE, np.inf, -3.0), b_switch(True)])]
    out.append(("bypass NaN and Inf in the fields", BYPASS, (NOISE_A, NOISE_B),
                ops_of([b_fields(S_ACTIVE, np.nan, 0.5)], 113, odd, b_process(B_PROCESS, True))))
    out.append(("bypass NaN and Inf in the fields, drywet", BYPASS, (NOISE_A, NOISE_B),
                ops_of([b_fields(S_ON, 0.0, 0.5)], 113, odd, b_process(B_PROCESS_DRYWET, True, 0.5, -2.0))))
    for what, sa, sb, wg, dg in ((B_PROCESS, NOISE_A, SUBNORMAL, 1.0, 1.0), (B_PROCESS_DRYWET, SUBNORMAL, NOISE_B, 1e-30, 0.5),
                                 (B_PROCESS_WET, SUBNORMAL, SUBNORMAL, 0.5, 1.0), (B_PROCESS, SPECIAL, NOISE_B, 1.0, 1.0),
                                 (B_PROCESS, NOISE_A, SPECIAL, 1.0, 1.0), (B_PROCESS_DRYWET, SPECIAL, SPECIAL, 0.0, 0.0)):
        for dry in ((True, False) if sb != NOISE_B else (True,)):
            name = "bypass %d rows %d %d%s gains %g %g" % (what, sa, sb, " dry" if dry else "", wg, dg)
            out.append((name, BYPASS, (sa, sb), ops_of([b_init(300), b_switch(True)], 256, [(600, [b_switch(False)])],
                                                       b_process(what, dry, wg, dg))))

    combos = ((True, True), (False, True), (True, False), (False, False))
    for li, length in enumerate(LENGTHS):
        for ci, (fo, fi) in enumerate(combos):
            call = CALLS[(li + ci) % len(CALLS)]
            events = [(100, [X_TOG]), (150, [X_TOG]), (900, [X_TOG]), (1150, [X_TOG])]
            out.append(("crossfade%s%s length %d calls of %d" % (" out" if fo else "", " in" if fi else "", length, call), CROSSFADE,
                        (NOISE_A, NOISE_B), ops_of([x_init(length)], call, events, x_process(fo, fi))))
    out.append(("crossfade length 5000 in calls of 936", CROSSFADE, (NOISE_A, NOISE_B), ops_of([x_init(5000), X_TOG], 936, [], x_process(True, True))))
    for fo, fi in combos[:3]:
        out.append(("crossfade%s%s reset in the fade" % (" out" if fo else "", " in" if fi else ""), CROSSFADE, (NOISE_A, NOISE_B),
                    ops_of([x_init(300), X_TOG], 113, [(100, [X_RES]), (400, [X_TOG]), (500, [X_RES, X_TOG])], x_process(fo, fi))))
    out.append(("crossfade never initialised", CROSSFADE, (NOISE_A, NOISE_B), ops_of([], 256, [(300, [X_TOG]), (600, [X_TOG])], x_process(True, True))))
    out.append(("crossfade length below one sample", CROSSFADE, (NOISE_A, NOISE_B),
                ops_of([(X_INIT, 48000, 0, bits(-1.0), 0)], 256, [(300, [X_TOG]), (600, [X_TOG])], x_process(True, True))))
    # silence standing in for a part of the fade between two ordinary calls
    ops = [x_init(300), X_TOG, (X_PROCESS, 100, HAS_A | HAS_B, 0, 0), (X_PROCESS, 100, 0, 0, 0), (X_PROCESS, 50, HAS_A | HAS_B, 0, 0),
           (X_PROCESS, 7, 0, 0, 0), (X_PROCESS, 143, HAS_B, 0, 0), (X_PROCESS, 800, HAS_A | HAS_B, 0, 0)]
    out.append(("crossfade silence for a part of the fade", CROSSFADE, (NOISE_A, NOISE_B), np.array(ops, np.uint32)))
    # the reference's own unit test: init(128, 0.5), 192 samples in steps of 8, toggled at 64
    ops = [(X_INIT, 128, 0, bits(0.5), 0)]
    for at in range(0, 192, 8):
        ops += ([X_TOG] if at == 64 else []) + [(X_PROCESS, 8, HAS_A | HAS_B, 0, 0)]
    out.append(("crossfade the reference's unit test schedule", CROSSFADE, (NOISE_A, NOISE_B),
                np.array(ops + [(X_PROCESS, N - 192, HAS_A | HAS_B, 0, 0)], np.uint32)))
    for sa, sb in ((NOISE_A, SUBNORMAL), (SUBNORMAL, SUBNORMAL), (SPECIAL, NOISE_B), (NOISE_A, SPECIAL), (SPECIAL, SPECIAL)):
        for fo, fi in (combos[:3] if sa == sb else combos[:1]):
            out.append(("crossfade%s%s rows %d %d" % (" out" if fo else "", " in" if fi else "", sa, sb), CROSSFADE, (sa, sb),
                        ops_of([x_init(300)], 256, [(100, [X_TOG]), (700, [X_TOG])], x_process(fo, fi))))
    return out


def run(exe, x, cs, cwd):
    src, dst = os.path.join(cwd, "cases.bin"), os.path.join(cwd, "results.bin")
    with open(src, "wb") as f:
        f.write(np.array([len(cs), N, len(x)], np.uint32).tobytes() + x.tobytes())
        for name, kind, sig, ops in cs:
            f.write(np.array([kind, sig[0], sig[1], len(ops)], np.uint32).tobytes() + ops.tobytes())
    subprocess.run([exe, src, dst], check=True, timeout=600)
    raw, at, out, state, answers = np.fromfile(dst, np.uint32), 0, [], [], []
    for name, kind, sig, ops in cs:
        out.append(raw[at:at + N].view(f32))
        state.append(raw[at + N:at + N + 4])
        answers.append(raw[at + N + 4:at + N + 4 + len(ops)])
        at += N + 4 + len(ops)
    assert at == raw.size, (at, raw.size)
    return np.array(out), np.array(state), np.concatenate(answers)


def public_names(path, cls):
    """The names that the class declares in its public sections, in order: members, and the types of their arguments that are
    not built in."""
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    text = re.sub(r"//.*", "", text)
    body = text[text.index("{", re.search(r"\bclass\s+\w+\s+%s\b" % cls, text).end()):]
    flat, depth = [], 0
    for c in body[1:]:                                      # inline bodies and nested types away
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


def run_reference(reference):
    x = signals()
    cs = cases()
    have = open(os.path.join(ROOT, "oracle", "ref_shim", "lsp-plug.in", "dsp", "dsp.h")).read()
    more = "\n        ".join(t for n, t in (("mul_k3", OVERLAY_MUL_K3), ("fill_zero", OVERLAY_FILL_ZERO)) if not re.search(r"\b%s\s*\(" % n, have))
    with tempfile.TemporaryDirectory() as d:
        for rel, text in (("lsp-plug.in/dsp-units/version.h", OVERLAY_VERSION), ("lsp-plug.in/dsp/dsp.h", OVERLAY_DSP % more)):
            os.makedirs(os.path.dirname(os.path.join(d, "overlay", rel)), exist_ok=True)
            with open(os.path.join(d, "overlay", rel), "w") as f:
                f.write(text)
        with open(os.path.join(d, "driver.cpp"), "w") as f:
            f.write(DRIVER)
        srcs = [os.path.join(d, "driver.cpp")] + [os.path.join(reference, "src", "main", n)
                                                  for n in ("ctl/Bypass.cpp", "ctl/Crossfade.cpp", "iface/IStateDumper.cpp")]
        inc = ["-I" + os.path.join(d, "overlay"), "-I" + os.path.join(ROOT, "oracle", "ref_shim"), "-I" + os.path.join(reference, "include")]
        for exe, extra in (("ref_san", SAN_FLAGS), ("ref", [])):
            subprocess.check_call(["g++"] + FLAGS + extra + inc + ["-o", os.path.join(d, exe)] + srcs + ["-lm"])
        san = run(os.path.join(d, "ref_san"), x, cs, d)            # stand-alone, before anything is recorded
        got = run(os.path.join(d, "ref"), x, cs, d)
        keys = {l.split()[0]: l.split()[1:] for l in subprocess.check_output([os.path.join(d, "ref_san"), "keys"]).decode().splitlines()}
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(san, got))
    assert keys["sizeof"] == ["12", "24"], keys["sizeof"]
    inc = os.path.join(reference, "include", "lsp-plug.in", "dsp-units")
    names = {"ctl/Bypass.h": public_names(os.path.join(inc, "ctl", "Bypass.h"), "Bypass"),
             "ctl/Crossfade.h": public_names(os.path.join(inc, "ctl", "Crossfade.h"), "Crossfade")}
    return x, cs, got, keys, names


def check_branches(cs, out, state, answers):
    """What the cases are there for has happened in them."""
    off = np.concatenate([[0], np.cumsum([len(c[3]) for c in cs])])
    by = {c[0]: (o, s, answers[off[i]:off[i + 1]], c[3]) for i, (c, o, s) in enumerate(zip(cs, out, state))}
    a, b = signals()[:2]
    o, s, ans, ops = by["bypass ramp 240 ends with the block"]
    assert s[0] == S_ACTIVE and s[2] not in (bits(0.0), bits(1.0)) and not (np.uint32(s[2]).view(f32) > 0), "a ramp that ends with the block was clamped"
    o, s, ans, ops = by["bypass ramp 240 ends with a call"]
    k = ramp_steps(240)
    assert s[0] == S_ON and s[2] == bits(0.0) and np.array_equal(o[k:], a[k:]) and o[k - 1] != a[k - 1], "the next call did not clamp"
    o, s, ans, ops = by["bypass ramp 240 turned round half-way, and switches that change nothing"]
    assert list(ans[ops[:, 0] == B_SET_BYPASS]) == [0, 1, 1, 0, 1, 0, 1], "set_bypass answers"
    o, s, ans, ops = by["bypass never initialised"]
    assert np.array_equal(o[:300], a[:300]) and list(ans[ops[:, 0] == B_SET_BYPASS]) == [1, 1, 0]
    o, s, ans, ops = by["bypass NaN and Inf in the fields"]
    assert o[0] != a[0] and np.array_equal(o[1:200], a[1:200]), "a NaN delta goes down and stops after one sample"
    assert ramp_steps(5000) > N and len({ramp_steps(l) - l for l in LENGTHS}) > 1, "every ramp is as long as its division says"
    o, s, ans, ops = by["crossfade out in length 300 calls of %d" % CALLS[(4 + 0) % len(CALLS)]]
    assert list(ans[ops[:, 0] == X_TOGGLE]) == [1, 0, 1, 0] and np.array_equal(o[:100], b[:100]), "toggle refused in a fade, accepted after; fresh: fade_in"
    o, s, ans, ops = by["crossfade out in reset in the fade"]
    assert np.array_equal(o[100:400], a[100:400]) and not np.array_equal(o[:100], a[:100]), "after reset() the tail is fade_out"
    o, s, ans, ops = by["crossfade silence for a part of the fade"]
    assert np.all(o[100:200] == 0) and s[1] == 0 and np.array_equal(o[400:], b[400:]) and not np.array_equal(o[257:400], b[257:400])
    o, s, ans, ops = by["crossfade the reference's unit test schedule"]
    assert s[0] == 64 and np.array_equal(o[:64], b[:64]) and np.array_equal(o[128:], b[128:]) and o[64] == a[64]
    o, s, ans, ops = by["bypass 3 rows 3 1 dry gains 1 1"]
    sp = signals()[SPECIAL].view(np.uint32)
    assert o.view(np.uint32)[320] == SIGNALLING_NAN == sp[320], "a copied NaN lost its payload"
    return len(cs)


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


def build(reference):
    x, cs, (out, state, answers), keys, names = run_reference(reference)
    check_branches(cs, out, state, answers)
    arrs = {"x": x, "names": np.array([c[0] for c in cs]), "kind": np.array([c[1] for c in cs], np.uint32),
            "signal": np.array([c[2] for c in cs], np.uint32), "ops_n": np.array([len(c[3]) for c in cs], np.uint32),
            "ops": np.concatenate([c[3] for c in cs]), "out": out, "state": state, "answers": answers}
    return npz_bytes(arrs), keys, names


def load(path=OUT):
    """The stored file as (x, cases): dicts of name, kind, signal, ops, out, answers, state."""
    z = np.load(path)
    off = np.concatenate([[0], np.cumsum(z["ops_n"].astype(np.int64))])
    cs = [dict(name=str(z["names"][i]), kind=int(z["kind"][i]), signal=z["signal"][i], ops=z["ops"][off[i]:off[i + 1]],
               out=z["out"][i], answers=z["answers"][off[i]:off[i + 1]], state=z["state"][i]) for i in range(len(z["names"]))]
    return z["x"], cs


if __name__ == "__main__":
    data, keys, names = build(sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(ROOT), "reference"))
    with open(OUT, "wb") as f:
        f.write(data)
    for cls in ("bypass", "crossfade"):
        with open(os.path.join(HERE, cls + "_dump_keys.json"), "w") as f:
            json.dump({"keys": keys[cls], "closes": []}, f, indent=1)
            f.write("\n")
    with open(os.path.join(HERE, "bypass_crossfade_public_names.json"), "w") as f:
        json.dump(names, f, indent=1)
        f.write("\n")
    print("%d cases, %d bytes" % (len(load()[1]), len(data)))
