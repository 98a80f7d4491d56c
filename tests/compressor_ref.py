"""CPU yardsticks for lsp::dspu::Compressor (src/main/dynamics/Compressor.cpp) for the tests.

follow()        the envelope follower of process() (:231-256) in numpy float32: vectorised across channels, a loop over the
                samples; every product and every sum rounds once, so the device must give its bits.
gain64()        the gain curve of the scalar overload (:297-309) in float64 on float32 inputs: the branch (x <= start,
                x >= end, knee) is chosen on the float32 values, as the device chooses it.
gain32()        the same in float32, logf / expf taken as the correctly rounded values (float64 numpy, rounded): a float32
                evaluation of the curve, held against gain_bound() by a host test.
gain_bound()    the a-priori relative bound on |float32 gain - gain64| in units of u = 2^-24, see below.
params64()      update_settings() (:89-220) in float64 with a running first-order error bound (class Q).

The gain bound.  u = 2^-24 is the relative error of one float32 rounding.  logf and expf are taken to be within 2 ulp = 4 u
(LIBM; glibc and the device library document 1 ulp).  With lx = ln x, for one knee:
    tilt:   arg = lx t0 + t1        lx carries LIBM u |lx|, the product one rounding, the sum one rounding:
                                    D = |lx t0| (LIBM + 1) u + |arg| u
    knee:   q = h0 lx + h1, r = q lx, arg = r + h2:
                                    Dq = |h0 lx| (LIBM + 1) u + |q| u
                                    D  = |lx| Dq + |q lx| (LIBM + 1) u + |arg| u
    constant gain:                  D = 0, and no expf
an absolute error D of the argument is a relative error D of exp(arg), expf adds LIBM u, the product of the two knees u:
    bound = D0 + D1 + (LIBM [knee 0 not constant] + LIBM [knee 1 not constant] + 1) u,
times SLACK for the second-order terms.  Below both starts the gain is gain0 * gain1: one rounding, u.  It is a formula in the
argument of expf (and in what the argument was summed from), not a constant: a ratio of 20 at 40 dB above the threshold has
|lx t0| around 4 and is allowed about 25 u, a gentle knee near the threshold 6 u.  curve() multiplies by x: one more u.
"""
import numpy as np

U = 2.0 ** -24
LIBM = 4.0              # logf / expf: 2 ulp, in units of u
SLACK = 1.01            # second-order terms of the first-order bounds
f32 = np.float32

CM_DOWNWARD, CM_UPWARD, CM_BOOSTING = range(3)
BRANCHES = ("attack", "release_above", "release_below", "hold", "rearm")


def follow(x, state, ta, tr, rt, nhold):
    """x: float32 [C, n]; state: dict of e, peak (float32 [C]) and hold (uint32 [C]), advanced in place; ta, tr, rt, nhold:
    per-channel arrays.  Returns the envelope [C, n] and how often each branch of :235-253 was taken."""
    x = np.ascontiguousarray(x, f32)
    C, n = x.shape
    ta, tr, rt = (np.broadcast_to(np.asarray(v, f32), (C,)) for v in (ta, tr, rt))
    nhold = np.broadcast_to(np.asarray(nhold, np.uint32), (C,))
    e, peak, hold = state["e"].astype(f32), state["peak"].astype(f32), state["hold"].astype(np.uint32)
    env = np.empty((C, n), f32)
    taken = dict.fromkeys(BRANCHES, 0)
    one = np.uint32(1)
    for i in range(n):
        d = x[:, i] - e
        neg = d < 0
        held = neg & (hold > 0)
        above = e > rt
        en = e + np.where(neg & above, tr, ta) * d            # float32 arrays: the product rounds, then the sum
        rearm = ~neg & (en >= peak)
        rel = neg & ~held
        taken["attack"] += int(np.count_nonzero(~neg))
        taken["release_above"] += int(np.count_nonzero(rel & above))
        taken["release_below"] += int(np.count_nonzero(rel & ~above))
        taken["hold"] += int(np.count_nonzero(held))
        taken["rearm"] += int(np.count_nonzero(rearm))
        e = np.where(held, e, en)
        peak = np.where(rel | rearm, en, peak)
        hold = np.where(held, hold - one, np.where(rearm, nhold, hold)).astype(np.uint32)
        env[:, i] = e
    state["e"], state["peak"], state["hold"] = e, peak, hold
    return env, taken


def fresh_state(C):
    return {"e": np.zeros(C, f32), "peak": np.zeros(C, f32), "hold": np.zeros(C, np.uint32)}


def _knee_arrays(params):
    """params: list of per-channel dicts (CompressorBank.get_params) -> arrays [C] of every knee quantity, float32."""
    out = []
    for j in range(2):
        k = {n: np.array([p["k"][j][n] for p in params], f32) for n in ("start", "end", "gain")}
        k["herm"] = np.array([p["k"][j]["herm"] for p in params], f32)
        k["tilt"] = np.array([p["k"][j]["tilt"] for p in params], f32)
        out.append(k)
    return out


def _col(v):
    return v[:, None]


def _curve(e, params, dtype):
    """(gain, bound in u) of the envelope e [C, n] in `dtype` arithmetic; the branches from the float32 values."""
    x32 = np.abs(np.ascontiguousarray(e, f32))
    k = _knee_arrays(params)
    with np.errstate(all="ignore"):
        x = x32.astype(dtype)
        lx64 = np.log(x32.astype(np.float64))
        lx = lx64.astype(dtype)
        gains, D, expfs = [], np.zeros(x32.shape), np.zeros(x32.shape)
        for kk in k:
            lo, hi = x32 <= _col(kk["start"]), x32 >= _col(kk["end"])
            t0, t1 = _col(kk["tilt"][:, 0]).astype(dtype), _col(kk["tilt"][:, 1]).astype(dtype)
            h0, h1, h2 = (_col(kk["herm"][:, i]).astype(dtype) for i in range(3))
            p = lx * t0
            at = p + t1
            q = h0 * lx + h1
            r = q * lx
            ah = r + h2
            arg = np.where(hi, at, ah)
            g = np.exp(arg.astype(np.float64)).astype(dtype)
            gains.append(np.where(lo, _col(kk["gain"]).astype(dtype), g))
            dt = np.abs(p) * (LIBM + 1) + np.abs(at)
            dq = np.abs(h0 * lx) * (LIBM + 1) + np.abs(q)
            dh = np.abs(lx) * dq + np.abs(r) * (LIBM + 1) + np.abs(ah)
            D += np.where(lo, 0.0, np.where(hi, dt, dh).astype(np.float64))
            expfs += np.where(lo, 0.0, LIBM)
        both = (x32 <= _col(k[0]["start"])) & (x32 <= _col(k[1]["start"]))
        const = (_col(k[0]["gain"]).astype(dtype) * _col(k[1]["gain"]).astype(dtype)) * np.ones_like(x)
        gain = np.where(both, const, gains[0] * gains[1])
        bound = np.where(both, 1.0, (D + expfs + 1.0) * SLACK)
    return gain, bound


def gain64(e, params):
    return _curve(e, params, np.float64)[0]


def gain32(e, params):
    return _curve(e, params, f32)[0]


def gain_bound(e, params):
    """Allowed |gain - gain64| / |gain64| in units of u = 2^-24, per sample."""
    return _curve(e, params, np.float64)[1]


# ---- update_settings() in float64 with a first-order error bound -------------------------------------------------------
class Q:
    """A float64 value and a bound on how far a float32 evaluation of the same expression may be from it: every operation
    adds one rounding (u |v|) to the errors its operands carry; logf / expf add LIBM u |v|."""

    def __init__(self, v, err=0.0):
        self.v, self.err = np.float64(v), np.float64(err)      # numpy: a knee at 1 divides by zero without raising

    @staticmethod
    def of(x):
        return x if isinstance(x, Q) else Q(x)

    def _new(self, v, carried, roundings=1.0):
        return Q(v, (carried + roundings * U * abs(v)) * SLACK)

    def __add__(self, o):
        o = Q.of(o)
        return self._new(self.v + o.v, self.err + o.err)

    def __sub__(self, o):
        o = Q.of(o)
        return self._new(self.v - o.v, self.err + o.err)

    def __rsub__(self, o):
        return Q.of(o) - self

    def __mul__(self, o):
        o = Q.of(o)
        return self._new(self.v * o.v, abs(self.v) * o.err + abs(o.v) * self.err)

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = Q.of(o)
        return self._new(self.v / o.v, self.err / abs(o.v) + abs(self.v) * o.err / (o.v * o.v))

    def __rtruediv__(self, o):
        return Q.of(o) / self

    def log(self):
        return self._new(np.log(self.v), self.err / abs(self.v), LIBM)

    def exp(self):
        v = np.exp(self.v)
        return self._new(v, v * self.err, LIBM)


def _hermite(x0, y0, k0, x1, k1):
    """interpolation::hermite_quadratic, src/main/misc/interpolation.cpp:103-109"""
    p0 = (Q.of(k0) - k1) * 0.5 / (x0 - x1)
    p1 = k0 - Q(2.0) * p0 * x0
    p2 = y0 - (p0 * x0 + p1) * x0
    return [p0, p1, p2]


def hold_samples(sample_rate, hold):
    """nHold in the reference's float32: millis_to_samples(sr, hold) truncated (exact, no tolerance)."""
    return int(np.uint32(f32(f32(hold) * f32(0.001)) * f32(sample_rate)))


def params64(sample_rate, mode, attack_threshold, release_threshold, boost_threshold, attack, release, hold, knee, ratio):
    """Every quantity of update_settings() as a Q, keyed like flatten(); the inputs are the float32 values the setters keep."""
    at, bt, kn, ratio = (float(f32(v)) for v in (attack_threshold, boost_threshold, knee, ratio))
    sr = float(f32(sample_rate))
    k707 = Q(float(f32(1.0 - np.sqrt(0.5)))).log()
    ms = Q(float(f32(0.001)))
    out = {"tau_attack": 1.0 - (k707 / (Q(float(f32(attack))) * ms * sr)).exp(),
           "tau_release": 1.0 - (k707 / (Q(float(f32(release))) * ms * sr)).exp(),
           "release_threshold": Q(float(f32(release_threshold)))}

    def put(j, start, end, gain, tilt0, tilt1, herm):
        for n, v in (("start", start), ("end", end), ("gain", gain), ("tilt0", tilt0), ("tilt1", tilt1),
                     ("herm0", herm[0]), ("herm1", herm[1]), ("herm2", herm[2])):
            out["k%d.%s" % (j, n)] = Q.of(v)

    zero3 = [Q(0.0)] * 3
    with np.errstate(all="ignore"):
        if mode == CM_UPWARD:
            rr = 1.0 / Q(ratio)
            th1, th2 = Q(at).log(), Q(bt).log()
            b = (rr - 1.0) * (th2 - th1)
            s0, e0, s1, e1 = Q(at) * kn, Q(at) / kn, Q(bt) * kn, Q(bt) / kn
            t00, t10 = 1.0 - rr, rr - 1.0
            put(0, s0, e0, 1.0, t00, (rr - 1.0) * th1, _hermite(s0.log(), 0.0, 0.0, e0.log(), t00))
            put(1, s1, e1, b.exp(), t10, (1.0 - rr) * th1, _hermite(s1.log(), b, 0.0, e1.log(), t10))
        elif mode == CM_BOOSTING:
            lim = float(f32(f32(1.0) + f32(1e-5)))
            rr = 1.0 / Q(max(ratio, lim))
            b, th1 = Q(bt).log(), Q(at).log()
            th2 = th1 + b / (rr - 1.0)
            eth2 = th2.exp()
            s0, e0, s1, e1 = Q(at) * kn, Q(at) / kn, eth2 * kn, eth2 / kn
            if bt >= 1.0:
                t00, t10 = 1.0 - rr, rr - 1.0
                put(0, s0, e0, 1.0, t00, (rr - 1.0) * th1, _hermite(s0.log(), 0.0, 0.0, e0.log(), t00))
                put(1, s1, e1, bt, t10, (1.0 - rr) * th1, _hermite(s1.log(), b, 0.0, e1.log(), t10))
            else:
                t00, t10 = rr - 1.0, 1.0 - rr
                put(0, s0, e0, 1.0, t00, (1.0 - rr) * th1, _hermite(s0.log(), 0.0, 0.0, e0.log(), t00))
                put(1, s1, e1, 1.0, t10, (rr - 1.0) * th2, _hermite(s1.log(), 0.0, 0.0, e1.log(), t10))
        else:
            rr = 1.0 / Q(ratio)
            th1 = Q(at).log()
            s0, e0 = Q(at) * kn, Q(at) / kn
            t00 = rr - 1.0
            put(0, s0, e0, 1.0, t00, (1.0 - rr) * th1, _hermite(s0.log(), 0.0, 0.0, e0.log(), t00))
            put(1, 1e10, 1e10, 1.0, 0.0, 0.0, zero3)
            for n in ("start", "end"):
                out["k1." + n] = Q(float(f32(1e10)))
    return out


def flatten(p):
    """A get_params / compute_params dict with the keys of params64()."""
    out = {n: float(p[n]) for n in ("tau_attack", "tau_release", "release_threshold")}
    for j in range(2):
        k = p["k"][j]
        for n in ("start", "end", "gain"):
            out["k%d.%s" % (j, n)] = float(k[n])
        for i in range(2):
            out["k%d.tilt%d" % (j, i)] = float(k["tilt"][i])
        for i in range(3):
            out["k%d.herm%d" % (j, i)] = float(k["herm"][i])
    return out


# ---- the settings and the input of the device tests ---------------------------------------------------------------------
def channel_settings(ch):
    """Different settings for every channel: the three modes and both boosting cases in turn, the knee at 1 on every fifth."""
    case = ch % 4
    mode = (CM_DOWNWARD, CM_UPWARD, CM_BOOSTING, CM_BOOSTING)[case]
    r = np.random.default_rng(1000 + ch)
    return dict(sample_rate=int(r.choice([44100, 48000, 96000])), mode=mode,
                attack_threshold=float(f32(10.0 ** (r.uniform(-30.0, -10.0) / 20.0))),
                release_threshold=float(f32(10.0 ** (r.uniform(-50.0, -25.0) / 20.0))),
                boost_threshold=float(f32(10.0 ** ((r.uniform(2.0, 9.0) if case == 2 else r.uniform(-70.0, -45.0)) / 20.0))),
                attack=float(f32(r.uniform(0.05, 2.0))), release=float(f32(r.uniform(0.2, 5.0))),
                hold=float(f32(r.choice([0.0, 0.05, 0.3]))),
                knee=1.0 if ch % 5 == 4 else float(f32(10.0 ** (r.uniform(-9.0, -1.0) / 20.0))),
                ratio=float(f32(r.uniform(1.5, 20.0))))


def sidechain(seed, C, n):
    """Band-limited noise (a one-pole low-pass of white noise, rectified on the even channels) whose level steps between
    0 dB and -60 dB every few dozen samples: attack, both releases, hold countdowns and re-arms all occur."""
    r = np.random.default_rng(seed)
    w = r.standard_normal((C, n + 8))
    lp = np.zeros_like(w)
    acc = np.zeros(C)
    for i in range(n + 8):
        acc = 0.6 * acc + 0.4 * w[:, i]
        lp[:, i] = acc
    lp = lp[:, 8:] * 1.5
    seg = 37
    steps = r.integers(0, 2, size=(C, n // seg + 1))
    level = np.repeat(np.where(steps == 1, 1.0, 1e-3), seg, axis=1)[:, :n]
    x = lp * level
    x[0::2] = np.abs(x[0::2])
    return x.astype(f32)
