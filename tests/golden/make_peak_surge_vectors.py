"""Writes tests/golden/peak_surge_ref_vectors.npz: what the reference's own PeakMeter and SurgeProtector classes compute on a list
of cases.  Data only: settings, operation lists, inputs, the reference's outputs and final state.  Run where the reference tree
exists:

    python tests/golden/make_peak_surge_vectors.py [reference tree]

The two class sources (and iface/IStateDumper.cpp, which their dump() needs) are compiled unmodified into a temporary directory
(-O2 -ffp-contract=off -msse2 -mfpmath=sse) against oracle/ref_shim plus a small overlay, written here, of what that shim lacks.
The program -- a stand-alone one with its own main -- is built a first time with -fsanitize=address,undefined and run on the same
cases before anything is recorded.

The file holds the signals (x: [signals, N]) and case by case: names, kind (0 PeakMeter, 1 SurgeProtector), signal (the row of x
a case reads; a SurgeProtector's process_mul multiplies row AUDIO), ops [k, 2] (what, argument: a count, or a float's bits), out
[N] and state [4] (uint32).  PeakMeter: fPeak's bits, nCounter, fTau's bits, nHold.  SurgeProtector: fGain's bits,
nTransitionTime, nShutdownTime, bOn.

What a process operation leaves in out: P_PROCESS / S_PROCESS / S_PROCESS_MUL the n samples written; P_PROCESS_STATE (the
overload without dst) zeros and the returned peak at the last of its samples; P_PROCESS_VALUE (one sample consumed as `value`,
the argument is `count`) the returned peak; S_PROCESS_STATE zeros."""
import io
import os
import subprocess
import sys
import tempfile
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "peak_surge_ref_vectors.npz")
f32 = np.float32

N = 1200
SR = 48000
PEAKMETER, SURGE = range(2)
P_SET_SR, P_SET_HOLD, P_SET_RELEASE, P_CLEAR, P_PROCESS, P_PROCESS_STATE, P_PROCESS_VALUE = range(7)
S_SET_TRANSITION, S_SET_SHUTDOWN, S_SET_ON, S_SET_OFF, S_RESET, S_PROCESS, S_PROCESS_STATE, S_PROCESS_MUL = range(8)
SIG_PEAKS, SIG_SPECIAL, SIG_LEVEL, SIG_LEVEL_NAN, AUDIO = range(5)
HOLDS = (0, 1, 255, 256, 257, 700)
TRANSITIONS = (0, 1, 255, 257, 700)
SHUTDOWNS = (0, 1, 300)
RELEASE_HALF = 0.0369                           # ms at 48 kHz: tau just below 0.5, so the smallest subnormal decays to 0
RELEASE_STUCK = 0.037                           # ... and just above: 2^-149 * tau rounds back to 2^-149, the peak never gets to 0
ON, OFF = 0.5, 0.25

OVERLAY_VERSION = r'''
#ifndef PEAK_SURGE_OVERLAY_VERSION_H_
#define PEAK_SURGE_OVERLAY_VERSION_H_
#include <lsp-plug.in/common/types.h>
#ifndef LSP_DSP_UNITS_PUBLIC
#define LSP_DSP_UNITS_PUBLIC
#endif
#endif
'''

# reads the cases, runs the classes, writes out[n] and four state words per case; the fields are read by name
DRIVER = r'''
#define private public
#define protected public
#include <lsp-plug.in/dsp-units/meters/PeakMeter.h>
#include <lsp-plug.in/dsp-units/dynamics/SurgeProtector.h>
#undef private
#undef protected
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
    uint32_t hdr[3];
    if (fread(hdr, 4, 3, f) != 3) return 3;
    const uint32_t cases = hdr[0], n = hdr[1], signals = hdr[2];
    std::vector<float> x(size_t(n) * signals), out(n);
    if (fread(x.data(), 4, x.size(), f) != x.size()) return 3;
    const float *audio = &x[size_t(n) * (signals - 1)];
    for (uint32_t c = 0; c < cases; ++c)
    {
        uint32_t h[3];
        if (fread(h, 4, 3, f) != 3) return 3;
        std::vector<uint32_t> ops(2 * h[2]);
        if (fread(ops.data(), 4, ops.size(), f) != ops.size()) return 3;
        if (h[1] >= signals) return 4;
        const float *in = &x[size_t(n) * h[1]];
        std::fill(out.begin(), out.end(), 0.0f);
        dspu::PeakMeter pm;
        dspu::SurgeProtector sp;
        size_t at = 0;
        for (uint32_t k = 0; k < h[2]; ++k)
        {
            const uint32_t what = ops[2 * k], arg = ops[2 * k + 1];
            if (h[0] == 0)
            {
                switch (what)
                {
                    case 0: pm.set_sample_rate(arg); break;
                    case 1: pm.set_hold_time(flt(arg)); break;
                    case 2: pm.set_release_time(flt(arg)); break;
                    case 3: pm.clear(); break;
                    case 4: if (at + arg > n) return 5; pm.process(&out[at], &in[at], arg); at += arg; break;
                    case 5: if (at + arg > n || arg == 0) return 5; out[at + arg - 1] = pm.process(&in[at], arg); at += arg; break;
                    case 6: if (at + 1 > n) return 5; out[at] = pm.process(in[at], size_t(arg)); at += 1; break;
                    default: return 6;
                }
            }
            else
            {
                switch (what)
                {
                    case 0: sp.set_transition_time(arg); break;
                    case 1: sp.set_shutdown_time(arg); break;
                    case 2: sp.set_on_threshold(flt(arg)); break;
                    case 3: sp.set_off_threshold(flt(arg)); break;
                    case 4: sp.reset(); break;
                    case 5: if (at + arg > n) return 5; sp.process(&out[at], &in[at], arg); at += arg; break;
                    case 6: if (at + arg > n) return 5; sp.process((float *)NULL, &in[at], arg); at += arg; break;
                    case 7:
                        if (at + arg > n) return 5;
                        memcpy(&out[at], &audio[at], arg * sizeof(float));
                        sp.process_mul(&out[at], &in[at], arg);
                        at += arg;
                        break;
                    default: return 6;
                }
            }
        }
        if (at != n) return 7;
        fwrite(out.data(), 4, n, g);
        uint32_t st[4];
        if (h[0] == 0)
            st[0] = bits(pm.fPeak), st[1] = pm.nCounter, st[2] = bits(pm.fTau), st[3] = pm.nHold;
        else
            st[0] = bits(sp.fGain), st[1] = uint32_t(sp.nTransitionTime), st[2] = uint32_t(sp.nShutdownTime), st[3] = sp.bOn ? 1 : 0;
        fwrite(st, 4, 4, g);
    }
    fclose(f);
    return fclose(g) == 0 ? 0 : 8;
}
'''

FLAGS = ["-std=c++11", "-O2", "-ffp-contract=off", "-msse2", "-mfpmath=sse", "-DLSP_DSP_UNITS_BUILTIN", "-Wall"]
SAN_FLAGS = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]


def bits(v):
    return int(f32(v).view(np.uint32))


def hold_ms(samples, sr=SR):
    """A hold time in milliseconds that update_settings() turns into exactly `samples`: uint32_t((ms * 0.001f) * sr)."""
    ms = f32(samples) / f32(sr) * f32(1000.0)
    for _ in range(64):
        got = int((ms * f32(0.001)) * f32(sr))
        if got == samples:
            return ms
        ms = np.nextafter(ms, f32(np.inf) if got < samples else f32(-np.inf))
    raise AssertionError(samples)


def signals():
    rng = np.random.default_rng(1234)
    t = np.arange(N)
    # PeakMeter: bursts between stretches of exact silence, a plateau of equal samples, a slow swell, quiet noise
    peaks = rng.standard_normal(N) * 0.05
    for at, level in ((40, 0.9), (250, 0.6), (262, 0.8), (500, 1.5), (1020, 0.3)):
        peaks[at] = level * (-1.0) ** at
    peaks[100:240] = 0.0
    peaks[300:330] = -0.75                                  # s == peak again and again: the counter restarts
    peaks[330:480] = 0.0
    peaks[520:1000] = 0.0                                   # 480 samples: longer than any hold but 700
    peaks[1030:1100] = 0.2 * np.sin(t[1030:1100] * 0.05) ** 2 + 0.001
    peaks[1100:] = 0.0
    # ... and one with NaN, +Inf and -Inf samples among ordinary ones
    special = rng.standard_normal(N) * 0.1
    special[150] = np.nan
    special[400] = np.inf
    special[700] = -np.inf
    special[900] = np.nan
    special[1000:] = 0.0
    # SurgeProtector: a level that is there (>= ON), gone (< OFF) or in between, with gaps shorter and longer than 300 samples
    level = 0.01 + 0.2 * rng.random(N)                      # below OFF
    for lo, hi in ((90, 250), (300, 600), (1000, 1150)):    # on; the gap of 50 is shorter than 300, the gap of 400 longer
        level[lo:hi] = 0.55 + 0.4 * rng.random(hi - lo)
    level[90] = ON                                          # >= : exactly the threshold turns on
    level[400:420] = 0.3                                    # between OFF and ON while on: stays on
    level[420] = OFF                                        # exactly the off threshold: counts as there
    level[950:955] = 0.4                                    # between the thresholds while off: stays off
    level_nan = level.copy()
    level_nan[50] = np.nan                                  # off: does not turn on
    level_nan[350] = np.nan                                 # on: counts as gone
    level_nan[1050:1060] = np.nan
    audio = rng.standard_normal(N) * 0.5
    return np.stack([peaks, special, level, level_nan, audio]).astype(f32)


def ops_of(first, call, events=(), process=None):
    """first: the setters before the first sample; events: (sample, [ops]) later on; the samples between in calls of `call`."""
    ops, at = list(first), 0
    for stop, more in list(events) + [(N, [])]:
        while at < stop:
            k = min(call, stop - at)
            ops.append((process, k))
            at += k
        for op in more:
            ops.append(op)
            if op[0] == P_PROCESS_VALUE and process in (P_PROCESS, P_PROCESS_STATE):
                at += 1
    return np.array(ops, np.uint32).reshape(-1, 2)


def peak_setup(hold, release, sr=SR):
    return [(P_SET_SR, sr), (P_SET_HOLD, bits(hold_ms(hold, sr))), (P_SET_RELEASE, bits(release))]


def surge_setup(transition, shutdown):
    return [(S_SET_TRANSITION, transition), (S_SET_SHUTDOWN, shutdown), (S_SET_ON, bits(ON)), (S_SET_OFF, bits(OFF))]


def cases():
    out = []
    for i, h in enumerate(HOLDS):
        rel = (5.0, RELEASE_HALF, 0.0)[i % 3]
        out.append(("peakmeter hold %d release %g" % (h, rel), PEAKMETER, SIG_PEAKS, ops_of(peak_setup(h, rel), N, process=P_PROCESS)))
    out.append(("peakmeter fresh (5 ms at rate 0, release 0)", PEAKMETER, SIG_PEAKS, ops_of([], 113, process=P_PROCESS)))
    out.append(("peakmeter hold 255 release 0 in calls of 113", PEAKMETER, SIG_PEAKS, ops_of(peak_setup(255, 0.0), 113, process=P_PROCESS)))
    out.append(("peakmeter hold 257 tau half in calls of 113", PEAKMETER, SIG_PEAKS,
                ops_of(peak_setup(257, RELEASE_HALF), 113, process=P_PROCESS)))
    out.append(("peakmeter hold 0 tau above half", PEAKMETER, SIG_PEAKS, ops_of(peak_setup(0, RELEASE_STUCK), N, process=P_PROCESS)))
    out.append(("peakmeter hold 256 release 2 without dst", PEAKMETER, SIG_PEAKS, ops_of(peak_setup(256, 2.0), 113, process=P_PROCESS_STATE)))
    # the hold shortened while the counter runs (700 set at 500, 180 left of it at 600 -> 100), lengthened later, the rate changed
    change = [(600, [(P_SET_HOLD, bits(hold_ms(100)))]), (1025, [(P_SET_HOLD, bits(hold_ms(300))), (P_SET_RELEASE, bits(1.0))]),
              (1110, [(P_SET_SR, 44100)])]
    out.append(("peakmeter hold 700, 100, 300", PEAKMETER, SIG_PEAKS, ops_of(peak_setup(700, 5.0), 113, change, process=P_PROCESS)))
    clear = [(270, [(P_CLEAR, 0)]), (510, [(P_CLEAR, 0)]), (1050, [(P_CLEAR, 0)])]
    out.append(("peakmeter clear()", PEAKMETER, SIG_PEAKS, ops_of(peak_setup(255, 5.0), 113, clear, process=P_PROCESS)))
    out.append(("peakmeter NaN and Inf", PEAKMETER, SIG_SPECIAL, ops_of(peak_setup(40, 1.0), 113, process=P_PROCESS)))
    out.append(("peakmeter NaN and Inf tau 0", PEAKMETER, SIG_SPECIAL, ops_of(peak_setup(40, 0.0), N, process=P_PROCESS)))
    # process(value, count): every sample a block-rate step; counts 0, 1, 64 and 300 against a hold of 256 reach all three branches
    for count in (0, 1, 64, 300):
        out.append(("peakmeter value steps of %d" % count, PEAKMETER, SIG_PEAKS,
                    np.array(peak_setup(256, 5.0) + [(P_PROCESS_VALUE, count)] * N, np.uint32)))
    out.append(("peakmeter value steps of 64 tau 0", PEAKMETER, SIG_PEAKS,
                np.array(peak_setup(256, 0.0) + [(P_PROCESS_VALUE, 64)] * N, np.uint32)))
    mixed = [(200, [(P_PROCESS_VALUE, 64)]), (505, [(P_PROCESS_VALUE, 1000)]), (800, [(P_PROCESS_VALUE, 0)])]
    out.append(("peakmeter samples and value steps", PEAKMETER, SIG_PEAKS, ops_of(peak_setup(257, 5.0), 113, mixed, process=P_PROCESS)))

    for i, t in enumerate(TRANSITIONS):
        sd = (300, 1, 0, 300, 1)[i]
        out.append(("surge transition %d shutdown %d" % (t, sd), SURGE, SIG_LEVEL, ops_of(surge_setup(t, sd), N, process=S_PROCESS)))
    out.append(("surge transition 700 shutdown 300", SURGE, SIG_LEVEL, ops_of(surge_setup(700, 300), 113, process=S_PROCESS)))
    out.append(("surge transition 255 shutdown 300 in calls of 113", SURGE, SIG_LEVEL, ops_of(surge_setup(255, 300), 113, process=S_PROCESS)))
    out.append(("surge transition 257 shutdown 0", SURGE, SIG_LEVEL, ops_of(surge_setup(257, 0), N, process=S_PROCESS)))
    out.append(("surge fresh", SURGE, SIG_LEVEL, ops_of([], N, process=S_PROCESS)))
    # on at 90: the counter is 50 at 140; 5 and then 100 leaves it at 5
    order = [(140, [(S_SET_TRANSITION, 5), (S_SET_TRANSITION, 100)])]
    out.append(("surge transition 255, then 5 and 100 at a counter of 50", SURGE, SIG_LEVEL, ops_of(surge_setup(255, 300), 113, order, process=S_PROCESS)))
    # gone from 600: the shutdown counter is 100 at 700; 20 is below it, the protector goes off with the next sample ...
    below = [(700, [(S_SET_SHUTDOWN, 20)])]
    out.append(("surge shutdown 300, then 20 at a counter of 100", SURGE, SIG_LEVEL, ops_of(surge_setup(255, 300), 113, below, process=S_PROCESS)))
    # ... and with 300 set again right after, the counter goes on from 20: still on at 950, where the level comes back above
    # OFF, instead of off at 899
    below = [(700, [(S_SET_SHUTDOWN, 20), (S_SET_SHUTDOWN, 300)])]
    out.append(("surge shutdown 300, then 20 and 300 at a counter of 100", SURGE, SIG_LEVEL, ops_of(surge_setup(255, 300), 113, below, process=S_PROCESS)))
    reset = [(180, [(S_RESET, 0)]), (950, [(S_RESET, 0)])]                      # in the fade-in; in the fade-out (off at 900)
    out.append(("surge reset() in both fades", SURGE, SIG_LEVEL, ops_of(surge_setup(255, 300), 113, reset, process=S_PROCESS)))
    out.append(("surge process_mul", SURGE, SIG_LEVEL, ops_of(surge_setup(257, 300), 113, process=S_PROCESS_MUL)))
    out.append(("surge process_mul transition 0", SURGE, SIG_LEVEL, ops_of(surge_setup(0, 1), N, process=S_PROCESS_MUL)))
    out.append(("surge without out", SURGE, SIG_LEVEL, ops_of(surge_setup(255, 300), 113, process=S_PROCESS_STATE)))
    out.append(("surge NaN level", SURGE, SIG_LEVEL_NAN, ops_of(surge_setup(255, 300), 113, process=S_PROCESS)))
    out.append(("surge NaN level shutdown 1", SURGE, SIG_LEVEL_NAN, ops_of(surge_setup(7, 1), N, process=S_PROCESS)))
    thr = [(920, [(S_SET_ON, bits(0.35)), (S_SET_OFF, bits(0.1))])]             # 0.4 at 950 now turns it on
    out.append(("surge thresholds changed", SURGE, SIG_LEVEL, ops_of(surge_setup(255, 300), 113, thr, process=S_PROCESS)))
    return out


def run(exe, x, cs, cwd):
    src, dst = os.path.join(cwd, "cases.bin"), os.path.join(cwd, "results.bin")
    with open(src, "wb") as f:
        f.write(np.array([len(cs), N, len(x)], np.uint32).tobytes() + x.tobytes())
        for name, kind, sig, ops in cs:
            f.write(np.array([kind, sig, len(ops)], np.uint32).tobytes() + ops.tobytes())
    subprocess.run([exe, src, dst], check=True, timeout=600)
    raw = np.fromfile(dst, np.uint32)
    assert raw.size == len(cs) * (N + 4), raw.size
    raw = raw.reshape(len(cs), N + 4)
    return raw[:, :N].view(f32).copy(), raw[:, N:].copy()


def run_reference(reference):
    x = signals()
    cs = cases()
    with tempfile.TemporaryDirectory() as d:
        rel = "lsp-plug.in/dsp-units/version.h"
        os.makedirs(os.path.dirname(os.path.join(d, "overlay", rel)), exist_ok=True)
        with open(os.path.join(d, "overlay", rel), "w") as f:
            f.write(OVERLAY_VERSION)
        with open(os.path.join(d, "driver.cpp"), "w") as f:
            f.write(DRIVER)
        srcs = [os.path.join(d, "driver.cpp")] + [os.path.join(reference, "src", "main", n)
                                                  for n in ("meters/PeakMeter.cpp", "dynamics/SurgeProtector.cpp", "iface/IStateDumper.cpp")]
        inc = ["-I" + os.path.join(d, "overlay"), "-I" + os.path.join(ROOT, "oracle", "ref_shim"), "-I" + os.path.join(reference, "include")]
        for exe, extra in (("ref_san", SAN_FLAGS), ("ref", [])):
            subprocess.check_call(["g++"] + FLAGS + extra + inc + ["-o", os.path.join(d, exe)] + srcs + ["-lm"])
        san_out, san_state = run(os.path.join(d, "ref_san"), x, cs, d)         # stand-alone, before anything is recorded
        out, state = run(os.path.join(d, "ref"), x, cs, d)
    assert np.array_equal(out.view(np.uint32), san_out.view(np.uint32)) and np.array_equal(state, san_state)
    return x, cs, out, state


def check_branches(cs, out, state):
    """What the cases are there for has happened in them."""
    by = {c[0]: (o, s) for c, o, s in zip(cs, out, state)}
    o, s = by["peakmeter hold 1 release 0.0369"]
    tiny = f32(np.finfo(f32).tiny)
    assert np.any((o > 0) & (o < tiny)) and np.all(o[900:1000] == 0.0), "no subnormal decay to 0"
    o, s = by["peakmeter hold 0 tau above half"]
    assert np.all(o[900:1000].view(np.uint32) == 1), "the smallest subnormal did not stay"
    o, s = by["peakmeter hold 255 release 0"]
    assert s[2] == 0 and np.any(o[520:1000] == 0.0) and np.any(o[520:1000] == f32(1.5)), "tau 0: held, then 0"
    o, s = by["peakmeter NaN and Inf tau 0"]
    assert np.isnan(o).any() and np.isinf(o).any(), "inf * 0"
    o, s = by["surge transition 255, then 5 and 100 at a counter of 50"]
    assert o[139] == np.sqrt(f32(49) / f32(255)) and o[140] == np.sqrt(f32(5) / f32(100)), "the setters' order"
    o, s = by["surge shutdown 300, then 20 at a counter of 100"]
    assert o[700] == f32(1.0) and o[701] < f32(1.0), "the shutdown counter was not clamped"
    o, s = by["surge shutdown 300, then 20 and 300 at a counter of 100"]
    assert np.all(o[790:] == f32(1.0)), "the shutdown setters' order"
    o, s = by["surge transition 700 shutdown 1"]
    assert 0 < o[250] < 1 and o[251] < o[250], "no turn-off inside the fade-in"
    o, s = by["surge transition 255 shutdown 300 in calls of 113"]
    assert 0 < o[1000] < o[999] and o[1001] > o[1000], "no turn-on inside the fade-out"
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


def build_bytes(reference):
    x, cs, out, state = run_reference(reference)
    check_branches(cs, out, state)
    arrs = {"x": x, "names": np.array([c[0] for c in cs]), "kind": np.array([c[1] for c in cs], np.uint32),
            "signal": np.array([c[2] for c in cs], np.uint32), "ops_n": np.array([len(c[3]) for c in cs], np.uint32),
            "ops": np.concatenate([c[3] for c in cs]), "out": out, "state": state}
    return npz_bytes(arrs)


def load(path=OUT):
    """The stored file as (x, cases): dicts of name, kind, signal, ops, out, state."""
    z = np.load(path)
    off = np.concatenate([[0], np.cumsum(z["ops_n"].astype(np.int64))])
    cs = [dict(name=str(z["names"][i]), kind=int(z["kind"][i]), signal=int(z["signal"][i]), ops=z["ops"][off[i]:off[i + 1]],
               out=z["out"][i], state=z["state"][i]) for i in range(len(z["names"]))]
    return z["x"], cs


if __name__ == "__main__":
    data = build_bytes(sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(ROOT), "reference"))
    with open(OUT, "wb") as f:
        f.write(data)
    print("%d cases, %d bytes" % (len(load()[1]), len(data)))
