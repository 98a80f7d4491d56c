"""CPU yardsticks for lsp::dspu::Expander (src/main/dynamics/Expander.cpp) for the tests, in the manner of compressor_ref.py.

follow()        the envelope follower of process() (:252-284).  It is the Compressor's statement for statement
                (Compressor.cpp:226-259), so it IS compressor_ref.follow: numpy float32, every product and sum rounded once.
gain64()        Expander::amplification(float) (:375-407) in float64 on float32 inputs, both modes; the branches (ceiling,
                floor, start, end) are chosen on the float32 values, as the device chooses them.
gain32()        the same in float32, logf / expf taken as the correctly rounded values.
gain_bound()    the a-priori relative bound on |float32 gain - gain64| in units of u = 2^-24, see below.
params64()      update_settings() (:200-245) with square_roots (:44-57) in float64 with a running first-order bound (class Q).

The gain bound, per sample, with lx = ln x as compressor_ref derives it for one knee (LIBM = 4 u for logf and for expf):
    tilt:   arg = t0 lx + t1                D = |t0 lx| (LIBM + 1) u + |arg| u
    knee:   q = h0 lx + h1, r = q lx, arg = r + h2
                                            Dq = |h0 lx| (LIBM + 1) u + |q| u
                                            D  = |lx| Dq + |q lx| (LIBM + 1) u + |arg| u
    bound = (D + LIBM u) SLACK              one expf, no product of knees
The constant results are exact: 1 outside the curve, 0 below the downward threshold.  Upward the level is first limited to
the threshold, which is exact as well, so above it the gain is the gain AT the threshold with that level's bound.  curve()
multiplies by the (limited) level: one more u.
"""
import numpy as np

import compressor_ref as cr
from compressor_ref import LIBM, SLACK, U, Q, fresh_state, hold_samples, sidechain  # noqa: F401

f32 = np.float32
EM_DOWNWARD, EM_UPWARD = range(2)
BRANCHES = cr.BRANCHES
follow = cr.follow

MINIMUM_TILT = float(f32(0.001))
UPPER_THRESHOLD = float(f32(13.815510558))
LOWER_THRESHOLD = float(f32(-16.118095651))
MIN_LOWER_THRESHOLD = float(f32(1e-7))
MAX_UPPER_THRESHOLD = float(f32(1e6))


def _col(params, name, idx=None):
    if idx is None:
        return np.array([p["k"][name] for p in params], f32)[:, None]
    return np.array([p["k"][name][idx] for p in params], f32)[:, None]


def _curve(e, params, dtype):
    """(gain, bound in u, limited level) of the envelope e [C, n] in `dtype` arithmetic; the branches from float32 values."""
    x32 = np.abs(np.ascontiguousarray(e, f32))
    up = np.array([bool(p["upward"]) for p in params])[:, None]
    start, end, thr = (_col(params, n) for n in ("start", "end", "threshold"))
    t0, t1 = (_col(params, "tilt", i).astype(dtype) for i in range(2))
    h0, h1, h2 = (_col(params, "herm", i).astype(dtype) for i in range(3))
    with np.errstate(all="ignore"):
        x32 = np.where(up & (x32 > thr), thr, x32).astype(f32)              # the ceiling, upward only
        floor = ~up & (x32 < thr)
        on = np.where(up, x32 > start, ~floor & (x32 < end))                # on the curve: a logf and an expf
        line = np.where(up, x32 >= end, x32 <= start)
        lx = np.log(x32.astype(np.float64)).astype(dtype)
        p = t0 * lx
        at = p + t1
        q = h0 * lx + h1
        r = q * lx
        ah = r + h2
        arg = np.where(line, at, ah)
        g = np.exp(arg.astype(np.float64)).astype(dtype)
        gain = np.where(floor, dtype(0.0), np.where(on, g, dtype(1.0)))
        dt = np.abs(p) * (LIBM + 1) + np.abs(at)
        dq = np.abs(h0 * lx) * (LIBM + 1) + np.abs(q)
        dh = np.abs(lx) * dq + np.abs(r) * (LIBM + 1) + np.abs(ah)
        D = np.where(line, dt, dh).astype(np.float64)
        bound = np.where(on, (D + LIBM) * SLACK, 0.0)
    return gain, bound, x32


def gain64(e, params):
    return _curve(e, params, np.float64)[0]


def gain32(e, params):
    return _curve(e, params, f32)[0]


def gain_bound(e, params):
    """Allowed |gain - gain64| / |gain64| in units of u = 2^-24, per sample (0 where the gain is the constant 0 or 1)."""
    return _curve(e, params, np.float64)[1]


def limited(e, params):
    """|e|, upward limited to the threshold: what curve() multiplies the gain by."""
    return _curve(e, params, np.float64)[2]


# ---- update_settings() in float64 with a first-order error bound -------------------------------------------------------
def _sqrt(q):
    v = np.sqrt(q.v)
    return Q(v, (q.err / (2.0 * v) + U * abs(v)) * SLACK)                    # sqrtf rounds once


def _hermite(x0, y0, k0, x1, k1):
    p0 = (Q.of(k0) - k1) * 0.5 / (x0 - x1)
    p1 = k0 - Q(2.0) * p0 * x0
    p2 = y0 - (p0 * x0 + p1) * x0
    return [p0, p1, p2]


def _root(herm, y, larger):
    a, b, c = herm[0], Q(0.0) - herm[1], herm[2] - y
    d = _sqrt(b * b - Q(4.0) * a * c)
    k = 1.0 / (a + a)
    x1, x2 = (b + d) * k, (b - d) * k
    if np.isnan(x1.v) or np.isnan(x2.v):
        return Q(np.nan)
    return (x1 if x1.v > x2.v else x2) if larger else (x1 if x1.v < x2.v else x2)


def params64(sample_rate, mode, attack_threshold, release_threshold, attack, release, hold, knee, ratio):
    """Every quantity of update_settings() as a Q, keyed like flatten(); the inputs are the float32 values the setters keep.
    The two comparisons that pick the formula of the threshold are made on the float64 values."""
    at, kn, ratio = (float(f32(v)) for v in (attack_threshold, knee, ratio))
    sr = float(f32(sample_rate))
    k707 = Q(float(f32(1.0 - np.sqrt(0.5)))).log()
    ms = Q(float(f32(0.001)))
    upward = mode == EM_UPWARD
    with np.errstate(all="ignore"):
        out = {"tau_attack": 1.0 - (k707 / (Q(float(f32(attack))) * ms * sr)).exp(),
               "tau_release": 1.0 - (k707 / (Q(float(f32(release))) * ms * sr)).exp(),
               "release_threshold": Q(float(f32(release_threshold)))}
        start, end = Q(at) * kn, Q(at) / kn
        log_ks, log_ke, log_th = start.log(), end.log(), Q(at).log()
        t0 = Q(ratio) - 1.0
        t1 = log_th * (1.0 - Q(ratio))
        tilt = t0 if t0.v > MINIMUM_TILT else Q(MINIMUM_TILT)
        if upward:
            herm = _hermite(log_ks, 0.0, 0.0, log_ke, t0)
            th = ((Q(UPPER_THRESHOLD) - t1) / tilt).exp()
            if th.v < end.v:
                th = _root(herm, UPPER_THRESHOLD, True).exp()
            if not th.v < MAX_UPPER_THRESHOLD:
                th = Q(MAX_UPPER_THRESHOLD)
        else:
            herm = _hermite(log_ke, 0.0, 0.0, log_ks, t0)
            th = ((Q(LOWER_THRESHOLD) - t1) / tilt).exp()
            if th.v > start.v:
                th = _root(herm, LOWER_THRESHOLD, False).exp()
            if not th.v > MIN_LOWER_THRESHOLD:
                th = Q(MIN_LOWER_THRESHOLD)
    out.update({"start": start, "end": end, "threshold": th, "tilt0": t0, "tilt1": t1,
                "herm0": herm[0], "herm1": herm[1], "herm2": herm[2]})
    return out


def flatten(p):
    """A get_params / compute_params dict with the keys of params64()."""
    out = {n: float(p[n]) for n in ("tau_attack", "tau_release", "release_threshold")}
    for n in ("start", "end", "threshold"):
        out[n] = float(p["k"][n])
    for i in range(2):
        out["tilt%d" % i] = float(p["k"]["tilt"][i])
    for i in range(3):
        out["herm%d" % i] = float(p["k"]["herm"][i])
    return out


# ---- the settings of the device tests ----------------------------------------------------------------------------------
def channel_settings(ch):
    """Different settings for every channel: upward and downward in turn (so a workgroup of four holds both), the knee at 1
    on every fifth.  The thresholds sit inside the range compressor_ref.sidechain() sweeps (0 to -60 dB)."""
    r = np.random.default_rng(2000 + ch)
    return dict(sample_rate=int(r.choice([44100, 48000, 96000])), mode=(EM_DOWNWARD, EM_UPWARD)[ch % 2],
                attack_threshold=float(f32(10.0 ** (r.uniform(-36.0, -10.0) / 20.0))),
                release_threshold=float(f32(10.0 ** (r.uniform(-50.0, -25.0) / 20.0))),
                attack=float(f32(r.uniform(0.05, 2.0))), release=float(f32(r.uniform(0.2, 5.0))),
                hold=float(f32(r.choice([0.0, 0.05, 0.3]))),
                knee=1.0 if ch % 5 == 4 else float(f32(10.0 ** (r.uniform(-12.0, -1.0) / 20.0))),
                ratio=float(f32(r.uniform(1.2, 6.0))))
