"""Writes tests/golden/limiter_ref_vectors.npz and tests/golden/autogain_ref_vectors.npz: what the reference's own Limiter,
AutoGain and SimpleAutoGain classes (oracle/_ref/gain_ref: their .cpp text compiled unmodified, see oracle/Makefile) derive and
compute on a list of cases.  Data only: settings, calls, setter events, inputs, the reference's results.  Run where the
reference tree exists, after the build:

    python tests/golden/make_gain_vectors.py

Every case first runs through oracle/_ref/gain_ref_san, the same program with the address and undefined-behaviour sanitizers
(a stand-alone host program); nothing is written unless that run is clean and gives the same bytes.  Both runs have a time
limit: the reference's patch loop has no bound of its own.

tests/test_gain_reference_host.py regenerates the files with build_bytes() and requires the committed bytes, so they are
written without time stamps.  Per class <c> in limiter, autogain, simple a file holds, case by case:

    <c>_names       the case names                  <c>_settings    float32 [cases, ns], in the order of SETTINGS[<c>]
    <c>_ncalls      calls of each case              <c>_calls       the call lengths, the cases one after the other
    <c>_nevents     setter events of each case      <c>_events      uint32 [events, 4]: ahead of which call, kind (EVENTS[<c>]), the
                                                                    two float32 arguments as bits
    <c>_n           samples of each case            <c>_in          float32 [inputs, samples]: the cases one after the other
    <c>_out         float32 [outputs, samples]      <c>_calli / <c>_callf   uint32 / float32 [calls, ...]: CALLI / CALLF[<c>], what
                                                                    update_settings() / update() derived ahead of each call and,
                                                                    last, the state after it
    limiter_input_of  the case whose input a case shares (itself, but for the later long cases): stored once
    simple_after    fCurrGain after every setter event
"""
import io
import os
import subprocess
import sys
import tempfile
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import autogain_ref as ar  # noqa: E402
import limiter_ref as lr  # noqa: E402

f32 = np.float32
GAIN_REF = os.path.join(ROOT, "oracle", "_ref", "gain_ref")
GAIN_SAN = os.path.join(ROOT, "oracle", "_ref", "gain_ref_san")
OUT = {"limiter": os.path.join(HERE, "limiter_ref_vectors.npz"), "autogain": os.path.join(HERE, "autogain_ref_vectors.npz")}
FILE_OF = {"limiter": "limiter", "autogain": "autogain", "simple": "autogain"}
CLASSES = ("limiter", "autogain", "simple")
MAGIC = 0x4741494E
INPUTS = {"limiter": 1, "autogain": 3, "simple": 1}
OUTPUTS = {"limiter": 1, "autogain": 2, "simple": 1}

SETTINGS = {
    "limiter": ("max_sample_rate", "max_lookahead", "sample_rate", "mode", "threshold", "lookahead", "attack", "release", "knee", "alr",
                "alr_attack", "alr_release", "alr_knee"),
    "autogain": ("sample_rate", "short_grow", "short_fall", "long_grow", "long_fall", "silence", "deviation", "max_gain", "quick_amp",
                 "limit", "level"),
    "simple": ("sample_rate", "grow", "fall", "threshold", "min_gain", "max_gain"),
}
# kind -> (setter, number of arguments, which of them are switches)
EVENTS = {
    "limiter": (("set_threshold", 2, (1,)), ("set_lookahead", 1, ()), ("set_mode", 1, ()), ("set_alr", 1, (0,)), ("set_alr_attack", 1, ()),
                ("set_alr_release", 1, ()), ("set_alr_knee", 1, ()), ("set_sample_rate", 1, ()), ("set_attack", 1, ()),
                ("set_release", 1, ()), ("set_knee", 1, ())),
    "autogain": (("set_deviation", 1, ()), ("enable_quick_amplifier", 1, (0,)), ("enable_max_gain", 1, (0,)), ("set_max_gain", 1, ()),
                 ("set_max_gain", 2, (1,)), ("set_short_speed", 2, ()), ("set_long_speed", 2, ()), ("set_silence_threshold", 1, ()),
                 ("set_sample_rate", 1, ())),
    "simple": (("set_min_gain", 1, ()), ("set_max_gain", 1, ()), ("set_gain", 2, ()), ("set_threshold", 1, ()), ("set_speed", 2, ()),
               ("set_sample_rate", 1, ())),
}
_CURVE = ("x1", "x2", "t", "a", "b", "c", "d")
CALLI = {"limiter": ("lookahead", "mode", "attack", "plane", "release", "middle", "max_lookahead", "latency", "head"),
         "autogain": ("flags_before", "flags"), "simple": ()}
CALLF = {
    "limiter": tuple("v_attack%d" % i for i in range(4)) + tuple("v_release%d" % i for i in range(4)) +
               ("threshold", "ks", "ke", "gain", "tau_attack", "tau_release", "hermite0", "hermite1", "hermite2", "envelope"),
    "autogain": ("short_kgrow", "short_kfall", "long_kgrow", "long_kfall") + tuple("short_comp.%s" % k for k in _CURVE) +
                tuple("out_comp.%s" % k for k in _CURVE) + ("silence", "deviation", "max_gain", "curr_gain", "out_gain"),
    "simple": ("kgrow", "kfall", "threshold", "min_gain", "max_gain", "curr_gain"),
}


def event(cls, before, setter, *args):
    """(ahead of which call, kind, a, b) for EVENTS[cls]'s setter of that name and number of arguments."""
    kind = [i for i, (name, n, _) in enumerate(EVENTS[cls]) if name == setter and n == len(args)][0]
    a = list(args) + [0.0] * (2 - len(args))
    return (int(before), kind, f32(a[0]), f32(a[1]))


def event_call(cls, ev):
    """-> (setter name, arguments) of a stored event; switches as bool, rates and modes as int."""
    name, n, switches = EVENTS[cls][int(ev[1])]
    args = [f32(ev[2]), f32(ev[3])][:n]
    args = [bool(v != 0) if i in switches else (int(v) if name in ("set_sample_rate", "set_mode") else float(v)) for i, v in enumerate(args)]
    return name, args


# ---- running the reference ----------------------------------------------------------------------------------------------
def case(cls, name, settings, inputs, calls, events=()):
    inputs = [np.ascontiguousarray(x, f32).reshape(-1) for x in inputs]
    assert len(inputs) == INPUTS[cls] and len({len(x) for x in inputs}) == 1 and sum(calls) == len(inputs[0]), (cls, name)
    events = sorted(events, key=lambda e: e[0])                 # stable: the order within a call is the list's
    assert all(0 <= e[0] < len(calls) for e in events)
    return dict(cls=cls, name=name, settings=np.array([settings[k] for k in SETTINGS[cls]], f32), inputs=inputs, calls=[int(v) for v in calls],
                events=[(int(e[0]), int(e[1]), f32(e[2]), f32(e[3])) for e in events])


def case_bytes(cases):
    b = io.BytesIO()
    u32 = lambda *v: b.write(np.array(v, np.uint32).tobytes())
    u32(MAGIC, len(cases))
    for c in cases:
        u32(CLASSES.index(c["cls"]), len(c["settings"]))
        b.write(np.asarray(c["settings"], f32).tobytes())
        u32(len(c["calls"]), *c["calls"])
        u32(len(c["events"]))
        for before, kind, a, bb in c["events"]:
            u32(before, kind)
            b.write(np.array([a, bb], f32).tobytes())
        u32(len(c["inputs"][0]))
        for x in c["inputs"]:
            b.write(np.asarray(x, f32).tobytes())
    return b.getvalue()


def parse_results(raw, cases):
    """What a driver wrote for `cases`: per case a dict of calli uint32 [calls, ni], callf float32 [calls, nf], after float32
    [events] (SimpleAutoGain), out float32 [outputs, n]."""
    w = np.frombuffer(raw, np.uint32)
    pos, out = 0, []

    def take(n):
        nonlocal pos
        v = w[pos:pos + n]
        assert len(v) == n, "short result file"
        pos += n
        return v

    for c in cases:
        cls = c["cls"]
        ncalls = int(take(1)[0])
        assert ncalls == len(c["calls"])
        ci, cf = [], []
        for _ in range(ncalls):
            ci.append(take(int(take(1)[0])).copy())
            cf.append(take(int(take(1)[0])).view(f32).copy())
        r = {"calli": np.array(ci, np.uint32).reshape(ncalls, len(CALLI[cls])), "callf": np.array(cf, f32).reshape(ncalls, len(CALLF[cls]))}
        r["after"] = take(int(take(1)[0])).view(f32).copy()
        assert len(r["after"]) == (len(c["events"]) if cls == "simple" else 0)
        nout, n = (int(v) for v in take(2))
        assert nout == OUTPUTS[cls] and n == len(c["inputs"][0])
        r["out"] = take(nout * n).view(f32).reshape(nout, n).copy()
        out.append(r)
    assert pos == len(w), "result file longer than its cases"
    return out


def run_driver(exe, cases, cwd=None, timeout=120, raw=False):
    """Runs a driver over the cases under a time limit; its standard error must stay empty (a sanitizer writes there)."""
    with tempfile.TemporaryDirectory() as d:
        src, dst = os.path.join(d, "cases.bin"), os.path.join(d, "results.bin")
        with open(src, "wb") as f:
            f.write(case_bytes(cases))
        p = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=timeout, cwd=cwd)
        if exe == GAIN_SAN and "LeakSanitizer has encountered a fatal error" in p.stderr:
            # the sanitizer twin's leak check needs ptrace, which a build machine may withhold: there, and only there, the run
            # is repeated for the bounds and the undefined arithmetic alone
            p = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=timeout, cwd=cwd,
                               env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
        if p.returncode != 0 or p.stderr.strip():
            raise RuntimeError("%s: exit status %d\n%s" % (exe, p.returncode, p.stderr[-4000:]))
        with open(dst, "rb") as f:
            data = f.read()
    return data if raw else parse_results(data, cases)


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same(a, b):
    """Equal bits, or NaN at the same places and equal bits elsewhere."""
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(bits(a)[~na], bits(b)[~nb])


# ---- the Limiter's cases --------------------------------------------------------------------------------------------------
# (maximum sample rate, maximum look-ahead in ms): ML = 48, 22 and, for the long cases, 240 samples; a bank has one of each
LIM_A, LIM_B, LIM_LONG = (48000, 1.0), (44100, 0.5), (96000, 2.5)
LIM_N = 1100
LIM_GENERAL = 16
LONG_N = lr.BUF_GRANULARITY + 300
LONG_CUT = 5000
LONG_CUTS = (LONG_CUT, 4096, 8191)                  # ... and on either side of it: a cut changes what a chunk is, and the result
# call lengths: with 8 ML = 384 (A) and 176 (B) the running count passes 8 ML inside a case and meets it exactly at a call's end
CALLS_A = ([150, 234, 200, 300, 216], [384, 100, 284, 332], [97, 300, 303, 400])
CALLS_B = ([100, 76, 200, 300, 424], [50, 60, 66, 500, 424], [175, 1, 177, 747])
PLANT = np.array([1.0, -1.3, 0.9, 1.6, -1.1], f32)


def plant(x, cuts, level=2.0):
    """A burst of five samples across every cut: two in the call that ends there, three in the next."""
    for c in cuts:
        if 2 <= c <= len(x) - 3:
            x[c - 2:c + 3] = f32(level) * PLANT
    return x


# attack and release of some cases, in samples as functions of the look-ahead la, so that every limit of init_sat / init_exp /
# init_line (Limiter.cpp:283-284, :318-325, :359-366) is met: just above the upper one (la, 2 la), far above it, and under 8
WIDTHS = {0: lambda la: (la + 2, 2 * la + 3), 2: lambda la: (3 * la, la), 1: lambda la: (3, 20),              # Hermite
          5: lambda la: (la + 2, 2 * la + 3), 4: lambda la: (4 * la, 5 * la),                                  # exponent (6: under 8)
          10: lambda la: (la + 2, 2 * la + 3), 8: lambda la: (3 * la, 6 * la), 9: lambda la: (3, 5)}           # line


def ms_of(samples, sr):
    """A time that millis_to_samples() turns into that many samples at sr."""
    ms = float(f32((samples + 0.5) * 1000.0 / sr))
    assert int(lr.millis_to_samples(sr, ms)) == samples, (samples, sr)
    return ms


def limiter_cases():
    rng = np.random.default_rng(2025)
    sig = lr.bursts(77, LIM_GENERAL, LIM_N)
    out = []
    for i in range(LIM_GENERAL):
        first = i < LIM_GENERAL // 2
        max_sr, max_la = LIM_A if first else LIM_B
        sr = ((48000, 44100, 32000) if first else (44100, 32000, 22050))[i % 3]
        la = ((1.0, 0.75, 0.5) if first else (0.5, 0.4, 0.5))[i % 3]
        mode = i if i < 12 else (1, 5, 9, 3)[i - 12]
        alr = i % 4 == 1
        s = dict(max_sample_rate=max_sr, max_lookahead=max_la, sample_rate=sr, mode=mode, threshold=float(rng.uniform(0.2, 0.6)), lookahead=la,
                 attack=float(rng.uniform(0.1, 0.5)), release=float(rng.uniform(0.1, 0.9)), knee=float(rng.uniform(0.5, 1.0)), alr=float(alr),
                 alr_attack=float(rng.uniform(0.05, 1.0)) if alr else 10.0, alr_release=float(rng.uniform(0.5, 5.0)) if alr else 50.0,
                 alr_knee=float(rng.uniform(0.3, 2.5)) if alr else 0.56234)
        if i in WIDTHS:
            a, r = WIDTHS[i](int(lr.millis_to_samples(sr, la)))
            s.update(attack=ms_of(a, sr), release=ms_of(r, sr))
        calls = list((CALLS_A if first else CALLS_B)[i % 3])
        cuts = np.cumsum(calls)[:-1]
        x = plant(sig[i].copy(), cuts)
        name, events = "%s at %d Hz" % (lr.MODES[mode], sr), []
        if i == 3:                                  # one peak in the second sample of a call: its patch begins in the call before
            c = int(cuts[1])
            x[c - 60:c + 60] = 0.0
            x[c + 1] = 2.5
            name += ", a peak at a call's second sample"
        elif i == 4:                                # one peak in the last sample of a call: its tail is the next call's
            c = int(cuts[1])
            x[c - 60:c + 60] = 0.0
            x[c - 1] = 2.5
            name += ", a peak at a call's last sample"
        elif i == 6:                                # most samples above the threshold: more than 32 patches in a chunk
            x = plant((1.2 * rng.standard_normal(LIM_N)).astype(f32), cuts)
            s.update(threshold=0.3, attack=0.05, release=0.05)      # the narrowest patch: 8 + 8 + 1 samples
            name += ", dense"
        elif i == 7:                                # two equal peaks six samples apart in silence, under a gain of exactly one
            x[:120] = 0.0
            x[40] = x[46] = 2.0
            name += ", two equal peaks"
        elif i == 14:
            calls = list(CALLS_B[0])
            x = plant(sig[i].copy(), np.cumsum(calls)[:-1])
            s.update(attack=ms_of(10, sr), release=ms_of(18, sr))                               # inside 11 and 22 ...
            events = [event("limiter", 1, "set_threshold", s["threshold"] * 0.6, False),       # lowered: the gains are scaled
                      event("limiter", 2, "set_threshold", s["threshold"] * 0.8, True),        # immediate: they are not
                      event("limiter", 3, "set_lookahead", 0.4),                               # ... and above 8 and 16
                      event("limiter", 4, "set_mode", 10)]
            name += ", threshold, look-ahead and mode change"
        elif i == 15:
            calls = list(CALLS_B[0])
            x = plant(sig[i].copy(), np.cumsum(calls)[:-1])
            events = [event("limiter", 1, "set_sample_rate", 22050),                            # refills the gain buffer
                      event("limiter", 2, "set_alr", True), event("limiter", 2, "set_alr_attack", 0.3),
                      event("limiter", 2, "set_alr_release", 2.0), event("limiter", 2, "set_alr_knee", 1.8),
                      event("limiter", 3, "set_alr", False), event("limiter", 3, "set_threshold", s["threshold"] * 0.5, False),
                      event("limiter", 4, "set_attack", 0.45), event("limiter", 4, "set_release", 0.2), event("limiter", 4, "set_knee", 0.7),
                      event("limiter", 4, "set_alr", True)]
            name += ", sample rate and ALR change"
        if alr:
            name += ", ALR"
        out.append(case("limiter", name, s, [x], calls, events))
    # the long cases: a chunk boundary inside a call, and the same input with the boundary elsewhere
    s = dict(max_sample_rate=LIM_LONG[0], max_lookahead=LIM_LONG[1], sample_rate=96000, mode=1, threshold=0.4, lookahead=2.0, attack=0.4,
             release=0.8, knee=0.7, alr=0.0, alr_attack=10.0, alr_release=50.0, alr_knee=0.56234)
    x = plant(lr.bursts(78, 1, LONG_N)[0], (lr.BUF_GRANULARITY,) + LONG_CUTS)
    out.append(case("limiter", "long, one call", s, [x], [LONG_N]))
    for cut in LONG_CUTS:
        out.append(case("limiter", "long, cut at %d" % cut, s, [x], [cut, LONG_N - cut]))
    return out


# ---- AutoGain's and SimpleAutoGain's cases ---------------------------------------------------------------------------------
AG_RATES = (1000, 1200, 800)
AG_CALLS = ([160, 200, 300, 440], [151, 209, 200, 540], [170, 185, 305, 440])      # 150: the surge up, 350: the deep drop
AG_GENERAL = 6
SAG_N = 900                                         # thirds of 300: far above, far below, across the threshold
SAG_CALLS = ([130, 370, 400], [75, 425, 400], [299, 2, 599])
SAG_GENERAL = 5


def autogain_settings(ch, sr, quick, limit, level=float(ar.LEXP), **over):
    """autogain_ref.settings_of(ch) at another sample rate: the speeds scaled with it, so that the gain moves as far per sample"""
    s = dict(ar.settings_of(ch), **over)
    k = sr / 1000.0
    for n in ("short_grow", "short_fall", "long_grow", "long_fall"):
        s[n] = s[n] * k
    return dict(s, sample_rate=sr, quick_amp=float(quick), limit=float(limit), level=level)


def autogain_cases():
    ll, ls, le = ar.signal(41, AG_GENERAL + 5)
    out = []
    for i in range(AG_GENERAL):
        quick, limit = ar.switches(i)
        out.append(case("autogain", "channel %d at %d Hz, quick %d, limit %d" % (i, AG_RATES[i % 3], quick, limit),
                        autogain_settings(i, AG_RATES[i % 3], quick, limit), [ll[i], ls[i], le[i]], AG_CALLS[i % 3]))
    i = AG_GENERAL
    ev = [event("autogain", 1, "set_deviation", 2.5), event("autogain", 1, "enable_quick_amplifier", False),
          event("autogain", 2, "enable_max_gain", False), event("autogain", 2, "set_long_speed", 8.0, 12.0),
          event("autogain", 3, "set_max_gain", 1.5, True), event("autogain", 3, "enable_quick_amplifier", True),
          event("autogain", 3, "set_short_speed", 120.0, 250.0), event("autogain", 3, "set_silence_threshold", 1e-3),
          event("autogain", 3, "set_max_gain", 1.8)]
    out.append(case("autogain", "setters between the calls", autogain_settings(i, 1000, True, True), [ll[i], ls[i], le[i]], AG_CALLS[0], ev))
    i += 1
    out.append(case("autogain", "all silence", autogain_settings(i, 1000, False, False), [ll[i] * f32(1e-4), ls[i] * f32(1e-4), le[i]], AG_CALLS[1]))
    # the gain falls until 20 times it meets 1e-37: a subnormal (20 / 1e-37 is still a float)
    n = 300
    big, small = np.full(n, 20.0, f32), np.full(n, 1e-37, f32)
    out.append(case("autogain", "subnormal gain", autogain_settings(0, 1000, True, False, level=1e-37, short_fall=20000.0, long_fall=2000.0),
                    [big, big, small], [150, 150]))
    for label, value in (("NaN", np.nan), ("+Inf", np.inf)):
        i += 1
        x = ls[i][:301].copy()
        x[100] = value
        out.append(case("autogain", "one " + label, autogain_settings(i, 1000, True, True), [ll[i][:301], x, le[i][:301]], [150, 151]))
    return out


def simple_settings(ch, sr=1000):
    """The settings of tests/test_simple_autogain_gpu.py: from one limit to the other within 250 samples"""
    k = ch % 5
    return dict(sample_rate=sr, grow=(100.0 + 2 * k) * sr / 1000.0, fall=(120.0 - 3 * k) * sr / 1000.0, threshold=0.1 + 0.005 * k,
                min_gain=0.25 - 0.01 * k, max_gain=4.0 + 0.25 * k)


def simple_cases():
    sig = ar.simple_signal(43, SAG_GENERAL + 6, SAG_N)
    out = []
    for i in range(SAG_GENERAL):
        out.append(case("simple", "channel %d at %d Hz" % (i, AG_RATES[i % 3]), simple_settings(i, AG_RATES[i % 3]), [sig[i]], SAG_CALLS[i % 3]))
    i = SAG_GENERAL
    # the gain sits at its lower limit of 0.25 when ten samples of 0.5 arrive: 0.5 x 0.25 is the threshold
    x = sig[i].copy()
    x[150:160] = 0.5
    out.append(case("simple", "a level at the threshold", dict(simple_settings(0), threshold=0.125, min_gain=0.25, max_gain=4.0), [x], SAG_CALLS[0]))
    # the three limit setters ahead of the second call, at a gain of 0.25, in two orders: 0.5, 0.3, 0.3 and 0.25, 0.5, 0.5
    i += 1
    tail = [event("simple", 2, "set_threshold", 0.08), event("simple", 2, "set_speed", 60.0, 90.0), event("simple", 2, "set_gain", 0.2, 3.0)]
    a = [event("simple", 1, "set_min_gain", 0.5), event("simple", 1, "set_max_gain", 0.3), event("simple", 1, "set_gain", 0.2, 3.0)]
    b = [event("simple", 1, "set_max_gain", 0.3), event("simple", 1, "set_min_gain", 0.5), event("simple", 1, "set_gain", 0.2, 3.0)]
    out.append(case("simple", "limit setters: min, max, both", simple_settings(0), [sig[i]], SAG_CALLS[0], a + tail))
    out.append(case("simple", "limit setters: max, min, both", simple_settings(0), [sig[i]], SAG_CALLS[0], b + tail))
    # no lower limit and a level of 3e38: the gain falls until their product meets the threshold, a subnormal
    out.append(case("simple", "decay into subnormals", dict(simple_settings(0), fall=2000.0, min_gain=0.0, max_gain=1.0),
                    [np.full(SAG_N, 3e38, f32)], SAG_CALLS[0]))
    for label, value in (("NaN", np.nan), ("+Inf", np.inf)):
        i += 1
        x = sig[i][:301].copy()
        x[100] = value
        out.append(case("simple", "one " + label, simple_settings(i), [x], [150, 151]))
    return out


# ---- the files ------------------------------------------------------------------------------------------------------------
def run_reference():
    cases = limiter_cases() + autogain_cases() + simple_cases()
    for exe in (GAIN_REF, GAIN_SAN):
        if not os.path.exists(exe):
            raise RuntimeError("%s is missing: make -C oracle" % exe)
    checked = run_driver(GAIN_SAN, cases, timeout=600, raw=True)           # refuses to go on if the sanitizers report anything
    plain = run_driver(GAIN_REF, cases, raw=True)
    if plain != checked:
        raise RuntimeError("the sanitizer build computes something else than the plain build")
    for c, r in zip(cases, parse_results(plain, cases)):
        c["ref"] = r
    return cases


def arrays(cases, which):
    out = {}
    for cls in [c for c in CLASSES if FILE_OF[c] == which]:
        cs = [c for c in cases if c["cls"] == cls]
        out[cls + "_names"] = np.array([c["name"] for c in cs])
        out[cls + "_settings"] = np.stack([c["settings"] for c in cs])
        out[cls + "_ncalls"] = np.array([len(c["calls"]) for c in cs], np.uint32)
        out[cls + "_calls"] = np.array([v for c in cs for v in c["calls"]], np.uint32)
        out[cls + "_nevents"] = np.array([len(c["events"]) for c in cs], np.uint32)
        ev = [[e[0], e[1], bits(e[2]).item(), bits(e[3]).item()] for c in cs for e in c["events"]]
        out[cls + "_events"] = np.array(ev, np.uint32).reshape(len(ev), 4)
        out[cls + "_n"] = np.array([len(c["inputs"][0]) for c in cs], np.uint32)
        own = list(range(len(cs)))
        if cls == "limiter":                                            # an input shared with an earlier case is stored once
            for i, c in enumerate(cs):
                for j in range(i):
                    if len(cs[j]["inputs"][0]) == len(c["inputs"][0]) and np.array_equal(bits(cs[j]["inputs"][0]), bits(c["inputs"][0])):
                        own[i] = j
                        break
            out["limiter_input_of"] = np.array(own, np.uint32)
        out[cls + "_in"] = np.concatenate([np.stack(c["inputs"]) for i, c in enumerate(cs) if own[i] == i], axis=1)
        out[cls + "_out"] = np.concatenate([c["ref"]["out"] for c in cs], axis=1)
        out[cls + "_calli"] = np.concatenate([c["ref"]["calli"] for c in cs])
        out[cls + "_callf"] = np.concatenate([c["ref"]["callf"] for c in cs])
        if cls == "simple":
            out["simple_after"] = np.concatenate([c["ref"]["after"] for c in cs])
    return out


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


def build_bytes():
    """{file name: bytes} of the two files."""
    cases = run_reference()
    return {which: npz_bytes(arrays(cases, which)) for which in OUT}


def load(paths=OUT):
    """The stored files as a list of cases per class: dicts of cls, name, settings (row), calls, events, inputs, out [outputs, n],
    calli, callf [calls, ...], and for SimpleAutoGain after [events]."""
    out = {}
    for which, path in paths.items():
        z = np.load(path)
        for cls in [c for c in CLASSES if FILE_OF[c] == which]:
            ns, ncalls, nev = (z[cls + k].astype(np.int64) for k in ("_n", "_ncalls", "_nevents"))
            own = z["limiter_input_of"].astype(np.int64) if cls == "limiter" else np.arange(len(ns))
            stored = np.array([own[i] == i for i in range(len(ns))])
            in_off = np.concatenate([[0], np.cumsum(np.where(stored, ns, 0))])
            off, coff, eoff = (np.concatenate([[0], np.cumsum(v)]) for v in (ns, ncalls, nev))
            cs = []
            for i in range(len(ns)):
                j = own[i]
                ev = z[cls + "_events"][eoff[i]:eoff[i + 1]]
                c = dict(cls=cls, name=str(z[cls + "_names"][i]), settings=z[cls + "_settings"][i],
                         calls=[int(v) for v in z[cls + "_calls"][coff[i]:coff[i + 1]]],
                         events=[(int(e[0]), int(e[1]), e[2:3].view(f32)[0], e[3:4].view(f32)[0]) for e in ev],
                         inputs=[row for row in z[cls + "_in"][:, in_off[j]:in_off[j + 1]]], out=z[cls + "_out"][:, off[i]:off[i + 1]],
                         calli=z[cls + "_calli"][coff[i]:coff[i + 1]], callf=z[cls + "_callf"][coff[i]:coff[i + 1]])
                if cls == "simple":
                    c["after"] = z["simple_after"][eoff[i]:eoff[i + 1]]
                cs.append(c)
            out[cls] = cs
    return out


if __name__ == "__main__":
    data = build_bytes()
    for which, path in OUT.items():
        with open(path, "wb") as f:
            f.write(data[which])
    got = load()
    print({cls: len(v) for cls, v in got.items()}, {which: "%d bytes" % len(v) for which, v in data.items()})
