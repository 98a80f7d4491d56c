"""Writes tests/golden/dynamics_ref_vectors.npz: what the reference's own Compressor, Expander, Gate and DynamicProcessor
classes (oracle/_ref/dyn_ref: their .cpp text compiled unmodified, see oracle/Makefile) derive and compute on a list of
cases.  Data only: settings, inputs, the reference's results.  Run where the reference tree exists, after the build:

    python tests/golden/make_dynamics_vectors.py

tests/test_dynamics_reference_host.py regenerates the file with build_bytes() and requires the committed bytes, so the file
is written without time stamps.  Per class <c> in compressor, expander, gate, dynproc the file holds, case by case:

    <c>_names       the case names                  <c>_settings    float32 [cases, ns], in the order of SETTINGS[<c>]
    <c>_calls       [cases, 2] call lengths         <c>_write       uint32 [cases, 5]: flag, e, peak (bits), hold, curve: the
                                                                    state a subclass writes after the first call
    <c>_n           samples of each case            <c>_in, <c>_env float32, the cases one after the other
    <c>_gain        float32, per case out[n] then the scalar overload on env[n]
    <c>_paramf      float32 [cases, nf]             <c>_parami      uint32 [cases, ni]      layouts: PARAMF / PARAMI
    <c>_states      uint32 [cases, 2, 4]: e, peak (bits), hold, curve after each call
    <c>_ladder      float32 [10, nl]                <c>_curves      float32 [10, nc, 2, nl]: CURVES[<c>], array form and
                                                                    scalar form (general cases only)
    gate_which      uint8, nCurve after every sample (from a run of one-sample calls, whose out / env are asserted equal)
    gate_hold       uint32, nHoldCounter after every sample, likewise
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

import compressor_ref as cr  # noqa: E402
import dynproc_ref as dr  # noqa: E402
import expander_ref as er  # noqa: E402
import gate_ref as gr  # noqa: E402

f32 = np.float32
DYN_REF = os.path.join(ROOT, "oracle", "_ref", "dyn_ref")
OUT = os.path.join(HERE, "dynamics_ref_vectors.npz")
CLASSES = ("compressor", "expander", "gate", "dynproc")
MAGIC = 0x44594E31
T = 256                                             # a tile of the banks
CALLS = (300, 3 * T + 7 - 300)                      # a tile end (256) and a call end (300) inside the signal
N = sum(CALLS)
GENERAL = 10                                        # three workgroups of four channels, the last partial
# the first of the ten channel_settings() taken: gate_ref's channels 0 to 10 all hold, 11 and 12 do not
FIRST = {"compressor": 0, "expander": 0, "gate": 4, "dynproc": 0}

SETTINGS = {
    "compressor": ("sample_rate", "mode", "attack_threshold", "release_threshold", "boost_threshold", "attack", "release", "hold",
                   "knee", "ratio"),
    "expander": ("sample_rate", "mode", "attack_threshold", "release_threshold", "attack", "release", "hold", "knee", "ratio"),
    "gate": ("sample_rate", "open_threshold", "close_threshold", "open_zone", "close_zone", "reduction", "attack", "release", "hold"),
    "dynproc": ("sample_rate", "hold", "in_ratio", "out_ratio") + tuple("dot%d.%s" % (i, k) for i in range(4) for k in ("in", "out", "knee"))
               + tuple("attack_level%d" % i for i in range(4)) + tuple("release_level%d" % i for i in range(4))
               + tuple("attack_time%d" % i for i in range(5)) + tuple("release_time%d" % i for i in range(5)),
}
_KNEE3 = ("start", "end", "gain", "herm0", "herm1", "herm2", "tilt0", "tilt1")
_GATE = ("start", "end", "gain_start", "gain_end", "herm0", "herm1", "herm2", "herm3")
_SPLINE = ("pre_ratio", "post_ratio", "knee_start", "knee_stop", "thresh", "makeup", "herm0", "herm1", "herm2")
PARAMF = {
    "compressor": ("tau_attack", "tau_release", "release_threshold") + tuple("k%d.%s" % (j, k) for j in range(2) for k in _KNEE3),
    "expander": ("tau_attack", "tau_release", "release_threshold", "start", "end", "threshold", "herm0", "herm1", "herm2", "tilt0", "tilt1"),
    "gate": ("tau_attack", "tau_release") + tuple("k%d.%s" % (j, k) for j in range(2) for k in _GATE),
    "dynproc": tuple("%s%d.%s" % (t, i, k) for t in ("attack", "release") for i in range(5) for k in ("level", "tau"))
               + tuple("spline%d.%s" % (i, k) for i in range(4) for k in _SPLINE),
}
PARAMI = {"compressor": ("hold",), "expander": ("hold", "upward"), "gate": ("hold",),
          "dynproc": ("hold", "splines", "attacks", "releases")}
CURVES = {"compressor": ("curve", "reduction"), "expander": ("curve", "amplification"),
          "gate": ("curve0", "curve1", "amplification0", "amplification1"), "dynproc": ("curve", "reduction", "model")}


# ---- settings as the driver reads them ---------------------------------------------------------------------------------
def settings_vector(cls, s):
    if cls != "dynproc":
        return np.array([s[k] for k in SETTINGS[cls]], f32)
    pad = lambda v, n, fill: [fill if x is None else x for x in list(v)] + [fill] * (n - len(v))
    v = [s.get("sample_rate", 0), s.get("hold", 0.0), s.get("in_ratio", 1.0), s.get("out_ratio", 1.0)]
    for d in pad(s.get("dots", ()), 4, (-1.0, -1.0, -1.0)):
        v += list(d)
    v += pad(s.get("attack_levels", ()), 4, -1.0) + pad(s.get("release_levels", ()), 4, -1.0)
    v += pad(s.get("attack_times", (0.0,)), 5, 0.0) + pad(s.get("release_times", (0.0,)), 5, 0.0)
    return np.array(v, f32)


def settings_dict(cls, v):
    """The keywords of <Bank>.configure / compute_params from a row of <c>_settings."""
    v = np.asarray(v, f32)
    if cls != "dynproc":
        d = {k: float(x) for k, x in zip(SETTINGS[cls], v)}
        d["sample_rate"] = int(d["sample_rate"])
        if "mode" in d:
            d["mode"] = int(d["mode"])
        return d
    dots = [tuple(float(x) for x in v[4 + 3 * i:7 + 3 * i]) for i in range(4)]
    off = lambda x: None if x < 0 else float(x)
    return dict(sample_rate=int(v[0]), hold=float(v[1]), in_ratio=float(v[2]), out_ratio=float(v[3]),
                dots=[None if max(d) < 0 else d for d in dots],
                attack_levels=[off(x) for x in v[16:20]], release_levels=[off(x) for x in v[20:24]],
                attack_times=[float(x) for x in v[24:29]], release_times=[float(x) for x in v[29:34]])


# ---- running the reference ----------------------------------------------------------------------------------------------
def case(cls, name, settings, x, calls=None, write=None, ladder=(), write_after=1):
    x = np.ascontiguousarray(x, f32).reshape(-1)
    calls = list(CALLS if calls is None else calls)
    assert sum(calls) == len(x), (name, calls, len(x))
    return dict(cls=cls, name=name, settings=settings_vector(cls, settings), x=x, calls=calls, write=write,
                write_after=write_after, ladder=np.asarray(ladder, f32))


def case_bytes(cases):
    b = io.BytesIO()
    u32 = lambda *v: b.write(np.array(v, np.uint32).tobytes())
    u32(MAGIC, len(cases))
    for c in cases:
        u32(CLASSES.index(c["cls"]), len(c["settings"]))
        b.write(c["settings"].tobytes())
        u32(len(c["calls"]), *c["calls"])
        w = c["write"]
        if w is None:
            u32(0, 0, 0, 0, 0)
        else:
            u32(c["write_after"], f32(w[0]).view(np.uint32), f32(w[1]).view(np.uint32), w[2], w[3] if len(w) > 3 else 0)
        u32(len(c["x"]))
        b.write(c["x"].tobytes())
        u32(len(c["ladder"]))
        b.write(c["ladder"].tobytes())
    return b.getvalue()


def parse_results(raw, cases):
    """What a driver wrote for `cases`: per case a dict of paramf, parami, out, env, sg0, sg1, states [calls, 4] (uint32),
    curves [nc, 2, nl]."""
    w = np.frombuffer(raw, np.uint32)
    pos, out = 0, []

    def take(n):
        nonlocal pos
        v = w[pos:pos + n]
        assert len(v) == n, "short result file"
        pos += n
        return v

    for c in cases:
        r = {}
        r["paramf"] = take(int(take(1)[0])).view(f32).copy()
        r["parami"] = take(int(take(1)[0])).copy()
        n = int(take(1)[0])
        assert n == len(c["x"])
        for k in ("out", "env", "sg0", "sg1"):
            r[k] = take(n).view(f32).copy()
        r["states"] = take(4 * int(take(1)[0])).reshape(-1, 4).copy()
        nc, nl = (int(v) for v in take(2))
        r["curves"] = take(nc * 2 * nl).view(f32).reshape(nc, 2, nl).copy()
        out.append(r)
    assert pos == len(w), "result file longer than its cases"
    return out


def run_driver(exe, cases, cwd=None):
    with tempfile.TemporaryDirectory() as d:
        src, dst = os.path.join(d, "cases.bin"), os.path.join(d, "results.bin")
        with open(src, "wb") as f:
            f.write(case_bytes(cases))
        subprocess.run([exe, src, dst], check=True, timeout=300, cwd=cwd)
        with open(dst, "rb") as f:
            return parse_results(f.read(), cases)


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same(a, b):
    """Equal bits, or NaN at the same places and equal bits elsewhere."""
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(bits(a)[~na], bits(b)[~nb])


# ---- the cases ----------------------------------------------------------------------------------------------------------
GATE_STEP = dict(sample_rate=48000, open_threshold=0.125, close_threshold=0.05, open_zone=0.5, close_zone=0.5, reduction=0.01,
                 attack=0.2, release=0.2, hold=0.0)
HI, LO = 0.5, 0.001


def _one_sample_twin(c):
    return dict(c, calls=[1] * len(c["x"]), ladder=np.zeros(0, f32), write_after=(c["calls"][0] if c["write"] is not None else 1))


def crossings(which, start=0):
    """Indices i with which[i] != which[i - 1] (the curve before sample 0 is `start`), and the direction: 1 opens, 0 closes."""
    prev = np.concatenate([[start], which[:-1]])
    idx = np.flatnonzero(which != prev)
    return [(int(i), int(which[i])) for i in idx]


def place_gate_crossings(settings, events, n=N):
    """A step signal between LO and HI whose crossing samples, in the reference's own run, are exactly `events`: (index, 1)
    an opening, (index, 0) a closing.  The offset from a step to its crossing is read from the reference and corrected."""
    lead = {1: 3, 0: 24}
    for _ in range(6):
        x = np.full(n, LO, f32)
        for idx, to in events:
            x[idx - lead[to] + 1:] = HI if to else LO
        c = case("gate", "probe", settings, x)
        which = run_driver(DYN_REF, [_one_sample_twin(c)])[0]["states"][:, 3]
        got = crossings(which)
        if got == list(events):
            return x
        assert len(got) == len(events), (got, events)
        for (gi, gd), (ei, ed) in zip(got, events):
            assert gd == ed
            if gi != ei:
                lead[ed] += gi - ei
                break
    raise AssertionError("no placement for %s" % (events,))


def special_cases():
    out = []
    # Gate: crossing samples at a tile's last sample (255) or the next tile's first (256), in both directions, and at the
    # first call's last sample (299)
    for name, events in (("gate opens at 255, closes at 299", [(255, 1), (299, 0)]),
                         ("gate opens at 256, closes at 511", [(256, 1), (511, 0)]),
                         ("gate closes at 255, opens at 299", [(120, 1), (255, 0), (299, 1), (600, 0)]),
                         ("gate closes at 256, opens at 512", [(100, 1), (256, 0), (512, 1)])):
        out.append(case("gate", name, GATE_STEP, place_gate_crossings(GATE_STEP, events)))
    # ... a crossing while the hold counter is positive: the envelope settles under the open threshold and arms the hold,
    # the input dips for five samples (counted down), then rises through the threshold
    held = dict(GATE_STEP, hold=1.0)
    x = np.full(N, LO, f32)
    x[100:250] = 0.1
    x[255:400] = HI
    x[500:520] = HI
    out.append(case("gate", "gate opens while the hold counts", held, x))

    # the envelope decays into the subnormals
    x = np.zeros(420, f32)
    x[:20] = 1.0
    sub = [200, 220]
    out.append(case("compressor", "subnormals", dict(sample_rate=48000, mode=cr.CM_DOWNWARD, attack_threshold=0.1, release_threshold=0.0,
                                                     boost_threshold=0.001, attack=0.05, release=0.05, hold=0.0, knee=0.5, ratio=4.0), x, sub))
    out.append(case("expander", "subnormals", dict(sample_rate=48000, mode=er.EM_DOWNWARD, attack_threshold=0.1, release_threshold=0.0,
                                                   attack=0.05, release=0.05, hold=0.0, knee=0.5, ratio=2.0), x, sub))
    out.append(case("gate", "subnormals", dict(GATE_STEP, attack=0.05, release=0.05), x, sub))
    out.append(case("dynproc", "subnormals", dict(sample_rate=48000, hold=0.0, in_ratio=1.0, out_ratio=4.0, dots=[(0.1, 0.1, 0.5)],
                                                  attack_times=[0.05], release_times=[0.05]), x, sub))

    # the re-arm test is >=: the envelope stops a few units under a constant input (the step rounds to nothing) with the
    # peak equal to it; the input dips for five samples (the counter goes from 24 to 19), returns for one (envelope == peak:
    # re-armed to 24) and leaves for good.  The first call ends 24 samples later, still held; under > the release would have
    # begun five samples before.
    x = np.full(300, LO, f32)
    x[:120] = 0.25
    x[125] = 0.25
    rearm = [150, 150]
    out.append(case("compressor", "re-arm on equality", dict(sample_rate=48000, mode=cr.CM_DOWNWARD, attack_threshold=0.1,
                                                             release_threshold=0.01, boost_threshold=0.001, attack=0.05, release=0.2,
                                                             hold=0.5, knee=0.5, ratio=4.0), x, rearm))
    out.append(case("expander", "re-arm on equality", dict(sample_rate=48000, mode=er.EM_UPWARD, attack_threshold=0.1, release_threshold=0.01,
                                                           attack=0.05, release=0.2, hold=0.5, knee=0.5, ratio=2.0), x, rearm))
    out.append(case("gate", "re-arm on equality", dict(GATE_STEP, attack=0.05, hold=0.5), x, rearm))
    out.append(case("dynproc", "re-arm on equality", dict(sample_rate=48000, hold=0.5, in_ratio=1.0, out_ratio=4.0, dots=[(0.1, 0.1, 0.5)],
                                                          attack_times=[0.05], release_times=[0.2]), x, rearm))

    # one +Inf, one NaN, each after 100 ordinary samples and followed by 200
    signals = {"compressor": cr.sidechain(91, 2, 301), "expander": cr.sidechain(92, 2, 301), "gate": gr.bursts(93, 2, 301),
               "dynproc": dr.sweep(94, 2, 301)}
    chan = {"compressor": cr.channel_settings, "expander": er.channel_settings, "gate": gr.channel_settings, "dynproc": dr.channel_settings}
    for cls in CLASSES:
        for row, (label, value) in enumerate((("+Inf", np.inf), ("NaN", np.nan))):
            x = signals[cls][row].copy()
            x[100] = value
            out.append(case(cls, "one " + label, chan[cls](2 + row), x, [150, 151]))

    # a subclass writes the follower's fields between the calls: a counter to count down and a peak above the envelope
    wcalls = [300, 300]
    out.append(case("compressor", "written state", chan["compressor"](0), cr.sidechain(61, 1, 600), wcalls, (1e-5, 0.75, 7)))
    out.append(case("expander", "written state", chan["expander"](1), cr.sidechain(62, 1, 600), wcalls, (1e-5, 0.75, 7)))
    out.append(case("dynproc", "written state", chan["dynproc"](2), dr.sweep(63, 1, 600), wcalls, (1e-5, 0.75, 7)))
    # Gate: an envelope above the open threshold under the open curve, a positive counter and a quiet input: the crossing
    # sample is a held one, and the second step counts it down a second time
    x = np.full(600, LO, f32)
    x[400:450] = HI
    out.append(case("gate", "written state", dict(GATE_STEP, hold=0.5), x, wcalls, (0.5, 0.5, 7, 0)))
    return out


def general_cases():
    sig = {"compressor": cr.sidechain(60, GENERAL, N), "expander": cr.sidechain(70, GENERAL, N), "gate": gr.bursts(80, GENERAL, N),
           "dynproc": np.concatenate([dr.sweep(90, GENERAL, N)[:5], cr.sidechain(95, GENERAL, N)[5:]])}
    chan = {"compressor": cr.channel_settings, "expander": er.channel_settings, "gate": gr.channel_settings, "dynproc": dr.channel_settings}
    out = []
    for cls in CLASSES:
        rates = set()
        for row in range(GENERAL):
            ch = FIRST[cls] + row
            s = chan[cls](ch)
            rates.add(s["sample_rate"])
            out.append(case(cls, "channel %d" % ch, s, sig[cls][row]))
        assert len(rates) == 3, (cls, rates)
    return out


def ladder(cls, paramf):
    """-120 dB to +24 dB, both signs, zero, and the knee ends themselves with their float32 neighbours."""
    db = np.arange(-120.0, 24.5, 2.0)
    lv = (10.0 ** (db / 20.0)).astype(f32)
    p = dict(zip(PARAMF[cls], paramf))
    if cls == "compressor":
        ends = [p["k%d.%s" % (j, k)] for j in range(2) for k in ("start", "end")]
    elif cls == "expander":
        ends = [p["start"], p["end"], p["threshold"]]
    elif cls == "gate":
        ends = [p["k%d.%s" % (j, k)] for j in range(2) for k in ("start", "end")]
    else:
        with np.errstate(all="ignore"):                                 # the splines keep logarithms; an unused one gives 1
            ends = [f32(np.exp(np.float64(p["spline%d.%s" % (i, k)]))) for i in range(4) for k in ("knee_start", "knee_stop", "thresh")]
    ends = np.array(ends, f32)
    ends = np.where(np.isfinite(ends), ends, f32(1.0)).astype(f32)
    near = np.concatenate([np.nextafter(ends, f32(0.0)), ends, np.nextafter(ends, f32(np.inf))]).astype(f32)
    return np.concatenate([lv, -lv[::6], [f32(0.0), f32(-0.0)], near]).astype(f32)


def run_reference():
    """Every case with the reference's results (`ref`), Gate cases with `which` and `holds` from a run of one-sample calls."""
    cases = general_cases() + special_cases()
    first = run_driver(DYN_REF, cases)                                  # the parameters, for the knee ends of the ladders
    for c, r in zip(cases, first):
        if c["name"].startswith("channel "):
            c["ladder"] = ladder(c["cls"], r["paramf"])
    gates = [c for c in cases if c["cls"] == "gate"]
    res = run_driver(DYN_REF, cases + [_one_sample_twin(c) for c in gates])
    for c, r in zip(cases, res):
        c["ref"] = r
    for c, t in zip(gates, res[len(cases):]):
        assert same(t["out"], c["ref"]["out"]) and same(t["env"], c["ref"]["env"]), c["name"]
        c["which"], c["holds"] = t["states"][:, 3].astype(np.uint8), t["states"][:, 2].copy()
        ends = np.cumsum(c["calls"]) - 1
        assert np.array_equal(t["states"][ends], c["ref"]["states"]), c["name"]
    return cases


def check_stand_ins(cases):
    """The stand-in array primitives against the reference's scalar overloads, on everything that is recorded."""
    for c in cases:
        r = c["ref"]
        what = (c["cls"], c["name"])
        sg = np.where(c["which"] != 0, r["sg1"], r["sg0"]) if c["cls"] == "gate" else r["sg0"]
        c["sgain"] = sg.astype(f32)
        if c["cls"] == "dynproc":
            # no stand-in here: reduction() is the class's own loop.  Its scalar form limits the level at 1e-10, the array
            # form at 1e-6 (DynamicProcessor.cpp:562-610): equal from 1e-6 up
            at = np.abs(r["env"]) >= dr.GAIN_AMP_MIN
            assert same(r["out"][at], sg[at]), what
        else:
            assert same(r["out"], sg), what
        for k, name in enumerate(CURVES[c["cls"]]):
            a, s = r["curves"][k]
            if c["cls"] == "dynproc" and name == "reduction":
                at = np.abs(c["ladder"]) >= dr.GAIN_AMP_MIN
                assert same(a[at], s[at]), what + (name,)
            elif c["cls"] == "compressor" and name == "reduction":
                assert same(a, r["curves"][0][0]), what + (name,)         # the array reduction() is the curve
            else:
                assert same(a, s), what + (name,)


def arrays(cases):
    out = {}
    for cls in CLASSES:
        cs = [c for c in cases if c["cls"] == cls]
        out[cls + "_names"] = np.array([c["name"] for c in cs])
        out[cls + "_settings"] = np.stack([c["settings"] for c in cs])
        out[cls + "_calls"] = np.array([c["calls"] for c in cs], np.uint32)
        out[cls + "_write"] = np.array([[0] * 5 if c["write"] is None else
                                        [1, f32(c["write"][0]).view(np.uint32), f32(c["write"][1]).view(np.uint32), c["write"][2],
                                         c["write"][3] if len(c["write"]) > 3 else 0] for c in cs], np.uint32)
        out[cls + "_n"] = np.array([len(c["x"]) for c in cs], np.uint32)
        out[cls + "_in"] = np.concatenate([c["x"] for c in cs])
        out[cls + "_env"] = np.concatenate([c["ref"]["env"] for c in cs])
        out[cls + "_gain"] = np.concatenate([np.concatenate([c["ref"]["out"], c["sgain"]]) for c in cs])
        out[cls + "_paramf"] = np.stack([c["ref"]["paramf"] for c in cs])
        out[cls + "_parami"] = np.stack([c["ref"]["parami"] for c in cs])
        out[cls + "_states"] = np.stack([c["ref"]["states"] for c in cs])
        gen = [c for c in cs if len(c["ladder"])]
        assert len(gen) == GENERAL
        out[cls + "_ladder"] = np.stack([c["ladder"] for c in gen])
        out[cls + "_curves"] = np.stack([c["ref"]["curves"] for c in gen])
        assert out[cls + "_paramf"].shape[1] == len(PARAMF[cls]) and out[cls + "_parami"].shape[1] == len(PARAMI[cls])
        assert out[cls + "_curves"].shape[1] == len(CURVES[cls])
    gates = [c for c in cases if c["cls"] == "gate"]
    out["gate_which"] = np.concatenate([c["which"] for c in gates])
    out["gate_hold"] = np.concatenate([c["holds"] for c in gates]).astype(np.uint32)
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
    cases = run_reference()
    check_stand_ins(cases)
    return npz_bytes(arrays(cases))


def load(path=OUT):
    """The stored file as a list of cases per class: dicts of name, settings (row), calls, write, x, env, out, sgain, paramf,
    parami, states, and for the general cases ladder and curves; Gate cases also which and holds."""
    z = np.load(path)
    out = {}
    for cls in CLASSES:
        ns = z[cls + "_n"].astype(np.int64)
        off = np.concatenate([[0], np.cumsum(ns)])
        cs = []
        for i, n in enumerate(ns):
            a, b = off[i], off[i + 1]
            g = z[cls + "_gain"][2 * a:2 * b]
            c = dict(cls=cls, name=str(z[cls + "_names"][i]), settings=z[cls + "_settings"][i], calls=[int(v) for v in z[cls + "_calls"][i]],
                     write=z[cls + "_write"][i], x=z[cls + "_in"][a:b], env=z[cls + "_env"][a:b], out=g[:n], sgain=g[n:],
                     paramf=z[cls + "_paramf"][i], parami=z[cls + "_parami"][i], states=z[cls + "_states"][i])
            if i < GENERAL:
                c["ladder"], c["curves"] = z[cls + "_ladder"][i], z[cls + "_curves"][i]
            if cls == "gate":
                c["which"], c["holds"] = z["gate_which"][a:b], z["gate_hold"][a:b]
            cs.append(c)
        out[cls] = cs
    return out


if __name__ == "__main__":
    data = build_bytes()
    with open(OUT, "wb") as f:
        f.write(data)
    got = load()
    print({cls: len(v) for cls, v in got.items()}, "%d bytes" % len(data))
