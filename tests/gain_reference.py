"""What tests/test_gain_reference_host.py and tests/test_gain_reference_gpu.py share: the recorded results of the reference's
own Limiter, AutoGain and SimpleAutoGain (tests/golden/limiter_ref_vectors.npz and autogain_ref_vectors.npz, written by
tests/golden/make_gain_vectors.py) in the shapes the restatements and the banks take, the setters replayed on the host, and
the restatements (limiter_ref, autogain_ref) run over a recorded case call by call on GIVEN parameters."""
import ctypes
import ctypes.util
import os
import sys

import numpy as np

import autogain_ref as ar
import limiter_ref as lr

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_gain_vectors as gv  # noqa: E402

f32 = np.float32
CLASSES = gv.CLASSES
same = gv.same
bits = gv.bits

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.expf.restype, _libm.expf.argtypes = ctypes.c_float, [ctypes.c_float]


def load():
    return gv.load()


def row(cls, c, k):
    """Call k of a case as a dict of its recorded fields: CALLI and CALLF by name."""
    d = {n: int(v) for n, v in zip(gv.CALLI[cls], c["calli"][k])}
    d.update((n, f32(v)) for n, v in zip(gv.CALLF[cls], c["callf"][k]))
    return d


def settings(c):
    return {k: f32(v) for k, v in zip(gv.SETTINGS[c["cls"]], c["settings"])}


def events_before(c, k):
    """[(setter, arguments)] of the events ahead of call k, in order."""
    return [gv.event_call(c["cls"], e) for e in c["events"] if e[0] == k]


def all_same(a, b):
    """Two get_params-like dicts: the integers equal, every float the same bits."""
    if set(a) != set(b):
        return False
    for k in a:
        if isinstance(a[k], dict):
            if not all_same(a[k], b[k]):
                return False
        elif isinstance(a[k], (int, np.integer)) and not isinstance(a[k], np.floating):
            if int(a[k]) != int(b[k]):
                return False
        elif not np.array_equal(bits(np.atleast_1d(a[k])), bits(np.atleast_1d(b[k]))):
            return False
    return True


# ---- Limiter ------------------------------------------------------------------------------------------------------------------
def limiter_params(c, k):
    """The recorded derived fields ahead of call k as LimiterBank.get_params() gives them."""
    r = row("limiter", c, k)
    p = {n: int(np.int32(np.uint32(r[n]))) for n in ("lookahead", "mode", "attack", "plane", "release", "middle")}
    p.update((n, r[n]) for n in ("threshold", "ks", "ke", "gain", "tau_attack", "tau_release"))
    p["v_attack"] = np.array([r["v_attack%d" % i] for i in range(4)], f32)
    p["v_release"] = np.array([r["v_release%d" % i] for i in range(4)], f32)
    p["hermite"] = np.array([r["hermite%d" % i] for i in range(3)], f32)
    return p


def limiter_table(p):
    """apply_sat_patch / apply_exp_patch / apply_line_patch (Limiter.cpp:609-673) without amp, in float32 on the coefficients of
    p, every product and sum rounded once, expf this machine's libm's: the table of p["release"] entries."""
    n, mode = max(int(p["release"]), 0), int(p["mode"])
    out = np.ones(n, f32)
    with np.errstate(all="ignore"):
        for t in range(n):
            if t < p["attack"]:
                v = p["v_attack"]
            elif t >= p["plane"]:
                v = p["v_release"]
            else:
                continue
            x = f32(t)
            if mode < 4:
                out[t] = f32(f32(f32(f32(f32(f32(v[0] * x) + v[1]) * x) + v[2]) * x) + v[3])
            elif mode < 8:
                out[t] = f32(v[0] + f32(v[1] * f32(_libm.expf(ctypes.c_float(float(f32(v[2] * x)))))))
            else:
                out[t] = f32(f32(v[0] * x) + v[1])
    return out


def limiter_unit(c, **kw):
    """limiter_ref.Unit after the driver's first setters (oracle/gain_driver.cpp, run_limiter)."""
    s = settings(c)
    u = lr.Unit(int(s["max_sample_rate"]), s["max_lookahead"], **kw)
    u.set_sample_rate(int(s["sample_rate"]))
    u.set_mode(int(s["mode"]))
    u.set_threshold(s["threshold"], True)
    for n in ("lookahead", "attack", "release", "knee", "alr_attack", "alr_release", "alr_knee"):
        getattr(u, "set_" + n)(s[n])
    u.set_alr(s["alr"] != 0)
    return u


def limiter_bank_setup(bank, ch, c):
    s = settings(c)
    bank.configure(ch, int(s["sample_rate"]), int(s["mode"]), float(s["threshold"]), float(s["lookahead"]), float(s["attack"]),
                   float(s["release"]), knee=float(s["knee"]), alr=bool(s["alr"] != 0), alr_attack=float(s["alr_attack"]),
                   alr_release=float(s["alr_release"]), alr_knee=float(s["alr_knee"]), immediate=True)


def limiter_bank_key(c):
    """Cases that can share a bank: the maxima are the bank's, and a chunk is counted from a call's first sample, so what the
    reference recorded for a case holds for its own cuts only."""
    s = settings(c)
    return (int(s["max_sample_rate"]), float(s["max_lookahead"]), tuple(c["calls"]))


def run_limiter(c, provider, calls=None, **kw):
    """The restatement over the case: provider(k, settings) -> (params, table) ahead of call k (settings: the keywords of
    LimiterBank.compute_params after the setters and the threshold rule).  `calls`: other cuts than the case's (no events then).
    -> gain [n], per call nHead, envelope, patches per chunk, and the settings the provider saw."""
    u = limiter_unit(c, **kw)
    x = c["inputs"][0]
    gain, heads, envs, patches, seen, pos = [], [], [], [], [], 0
    for k, n in enumerate(c["calls"] if calls is None else calls):
        if calls is None:
            for name, args in events_before(c, k):
                getattr(u, name)(*args)

        def compute(**s):
            seen.append((k, s))
            return provider(k, s)
        u.update_settings(compute)
        gain.append(u.process(x[pos:pos + n]))
        pos += n
        heads.append(u.lim.head)
        envs.append(f32(u.lim.env))
        patches.append(list(u.lim.patches_per_chunk))
    assert u.lim.overrun == 0
    return np.concatenate(gain), heads, envs, patches, seen


def recorded_limiter(c):
    """The provider of the reference's own recorded parameters, with the table evaluated from them (a run with other cuts asks
    for the first call's only: such a case has no events)."""
    def provider(k, s):
        p = limiter_params(c, min(k, len(c["calls"]) - 1))
        return p, limiter_table(p)
    return provider


# ---- AutoGain -----------------------------------------------------------------------------------------------------------------
def autogain_params(c, k):
    """The recorded derived fields ahead of call k as AutoGainBank.get_params() gives them."""
    r = row("autogain", c, k)
    p = {n: r[n] for n in ("short_kgrow", "short_kfall", "long_kgrow", "long_kfall", "silence", "deviation", "max_gain")}
    p["short_comp"] = {n: r["short_comp." + n] for n in ar.CURVE}
    p["out_comp"] = {n: r["out_comp." + n] for n in ar.CURVE}
    p["flags"] = r["flags_before"] & (ar.F_QUICK_AMP | ar.F_MAX_GAIN)
    return p


def autogain_settings_at(c):
    """The keywords of AutoGainBank.compute_params ahead of every call: the setters (AutoGain.cpp:90-153, :175-178) replayed."""
    s = settings(c)
    cur = {n: max(s[n], f32(0.0)) for n in ("short_grow", "short_fall", "long_grow", "long_fall", "silence", "max_gain")}
    cur["deviation"] = max(f32(1.0), s["deviation"])
    cur["sample_rate"] = int(s["sample_rate"])
    cur["flags"] = (ar.F_QUICK_AMP if s["quick_amp"] != 0 else 0) | (ar.F_MAX_GAIN if s["limit"] != 0 else 0)
    flag = lambda bit, on: (cur["flags"] | bit) if on else (cur["flags"] & ~bit)
    out = []
    for k in range(len(c["calls"])):
        for name, a in events_before(c, k):
            if name == "set_deviation":
                cur["deviation"] = max(f32(1.0), f32(a[0]))
            elif name == "enable_quick_amplifier":
                cur["flags"] = flag(ar.F_QUICK_AMP, a[0])
            elif name == "enable_max_gain":
                cur["flags"] = flag(ar.F_MAX_GAIN, a[0])
            elif name == "set_max_gain":
                cur["max_gain"] = max(f32(0.0), f32(a[0]))
                if len(a) > 1:
                    cur["flags"] = flag(ar.F_MAX_GAIN, a[1])
            elif name in ("set_short_speed", "set_long_speed"):
                which = name.split("_")[1]
                cur[which + "_grow"], cur[which + "_fall"] = max(f32(a[0]), f32(0.0)), max(f32(a[1]), f32(0.0))
            elif name == "set_silence_threshold":
                cur["silence"] = max(f32(0.0), f32(a[0]))
            elif name == "set_sample_rate":
                cur["sample_rate"] = int(a[0])
        out.append({n: (v if isinstance(v, int) else float(v)) for n, v in cur.items()})
    return out


def autogain_bank_setup(bank, ch, c):
    s = settings(c)
    bank.configure(ch, int(s["sample_rate"]), float(s["short_grow"]), float(s["short_fall"]), float(s["long_grow"]), float(s["long_fall"]),
                   float(s["silence"]), float(s["deviation"]), float(s["max_gain"]), quick_amp=bool(s["quick_amp"] != 0),
                   limit=bool(s["limit"] != 0))


def bank_event(bank, ch, name, args):
    """One recorded setter event on a bank's channel: the banks' setters carry the classes' names."""
    getattr(bank, name)(ch, *args)


def run_autogain(c, params_of, scalar=False):
    """The restatement over the case, params_of(k) ahead of call k; scalar: the level of the settings in the place of the lexp
    row.  -> vca [n], per call (fCurrGain, fOutGain, nFlags), the restatement's branch counters."""
    ag = ar.AutoGain([params_of(0)])
    ll, ls, le = (x[None, :] for x in c["inputs"])
    level = np.array([settings(c)["level"]], f32)
    vca, states, pos = [], [], 0
    for k, n in enumerate(c["calls"]):
        ag.set_params([params_of(k)])
        vca.append(ag.process(ll[:, pos:pos + n], ls[:, pos:pos + n], level if scalar else le[:, pos:pos + n])[0])
        pos += n
        states.append((f32(ag.gain[0]), f32(ag.out[0]), ag.flags(0)))
    return np.concatenate(vca), states, {k: int(v[0]) for k, v in ag.counters.items()}


# ---- SimpleAutoGain -----------------------------------------------------------------------------------------------------------
def simple_params(c, k):
    r = row("simple", c, k)
    return {n: r[n] for n in ("kgrow", "kfall", "threshold", "min_gain", "max_gain")}


def simple_settings_at(c):
    """The keywords of SimpleAutoGainBank.compute_params ahead of every call."""
    s = settings(c)
    cur = {n: s[n] for n in ("grow", "fall", "threshold", "min_gain", "max_gain")}
    cur["sample_rate"] = int(s["sample_rate"])
    out = []
    for k in range(len(c["calls"])):
        for name, a in events_before(c, k):
            if name == "set_min_gain":
                cur["min_gain"] = f32(a[0])
            elif name == "set_max_gain":
                cur["max_gain"] = f32(a[0])
            elif name == "set_gain":
                cur["min_gain"], cur["max_gain"] = f32(a[0]), f32(a[1])
            elif name == "set_threshold":
                cur["threshold"] = f32(a[0])
            elif name == "set_speed":
                cur["grow"], cur["fall"] = f32(a[0]), f32(a[1])
            elif name == "set_sample_rate":
                cur["sample_rate"] = int(a[0])
        out.append({n: (v if isinstance(v, int) else float(v)) for n, v in cur.items()})
    return out


def simple_bank_setup(bank, ch, c):
    s = settings(c)
    bank.set_sample_rate(ch, int(s["sample_rate"]))
    bank.set_speed(ch, float(s["grow"]), float(s["fall"]))
    bank.set_threshold(ch, float(s["threshold"]))
    bank.set_gain(ch, float(s["min_gain"]), float(s["max_gain"]))


def _simple_limit_setter(sg, name, a):
    """set_max_gain / set_min_gain / set_gain with their early returns (SimpleAutoGain.cpp:108-135)."""
    lo, hi = f32(sg.min_gain[0]), f32(sg.max_gain[0])
    if name == "set_max_gain" and hi != f32(a[0]):
        sg.set_max_gain(0, f32(a[0]))
    elif name == "set_min_gain" and lo != f32(a[0]):
        sg.set_min_gain(0, f32(a[0]))
    elif name == "set_gain" and not (lo == f32(a[0]) and hi == f32(a[1])):
        sg.set_gain(0, f32(a[0]), f32(a[1]))


def run_simple(c, params_of):
    """The restatement over the case, kgrow, kfall and threshold of params_of(k) ahead of call k; the limits are the setters'.
    -> dst [n], fCurrGain per call, fCurrGain after every event."""
    s = settings(c)
    sg = ar.SimpleAutoGain([dict(params_of(0), min_gain=f32(0.000001), max_gain=f32(1.0))])     # construct(), :43-56
    _simple_limit_setter(sg, "set_gain", (s["min_gain"], s["max_gain"]))
    x = c["inputs"][0][None, :]
    dst, states, after, pos = [], [], [], 0
    for k, n in enumerate(c["calls"]):
        for name, a in events_before(c, k):
            _simple_limit_setter(sg, name, a)
            after.append(f32(sg.gain[0]))
        p = params_of(k)
        for name in ("kgrow", "kfall", "threshold"):
            getattr(sg, name)[0] = p[name]
        assert bits(sg.min_gain)[0] == bits(p["min_gain"]) and bits(sg.max_gain)[0] == bits(p["max_gain"]), (c["name"], k)
        with np.errstate(all="ignore"):
            dst.append(sg.process(x[:, pos:pos + n])[0])
        pos += n
        states.append(f32(sg.gain[0]))
    return np.concatenate(dst), states, np.array(after, f32)


def case_for_driver(c):
    """A loaded case as make_gain_vectors.case_bytes() takes it."""
    return dict(cls=c["cls"], settings=np.asarray(c["settings"], f32), calls=list(c["calls"]), events=list(c["events"]),
                inputs=[np.asarray(x, f32) for x in c["inputs"]])
