"""CPU yardsticks for lsp::dspu::Gate (src/main/dynamics/Gate.cpp) for the tests, in the manner of compressor_ref.py.

process_transcribed()   Gate::process(out, env, in, samples) (:267-367) for ONE channel, transcribed: the outer while, the
                        two inner loops, the break without advancing, the follower run again on the same input sample
                        under the other curve.  Scalar numpy float32, every product and sum rounded once.  Returns the
                        envelope and the curve index that the gain of every sample is taken from.
process()               the same per sample and vectorised across channels (what the device tests are held against):
                        step; where the envelope left the curve in force, toggle and step once more.  A host test holds
                        the two against each other.
BOTH CARRY THE CAP of the bank: a sample is stepped again at most once, then the walk advances (the reference's loop has
no such cap and, with inverted thresholds, may never return).  Both count in `stats` the toggles and, as "capped", the
samples on which the envelope after the second step had left the NEW curve as well, i.e. where the reference would have gone
round again.  With close start <= open end and taus in [0, 1] that never happens; the tests assert
stats["capped"] == 0 on every signal with sane settings.

gain64() / gain32() / gain_bound()   Gate::amplification (:250-265) with the knee the curve index selects.  With lx = ln x
    carrying LIBM u |lx| and q1 = h0 lx + h1, r1 = q1 lx, q2 = r1 + h2, r2 = q2 lx, arg = r2 + h3:
        Dq1 = |h0 lx| (LIBM + 1) u + |q1| u
        Dr1 = |lx| Dq1 + |r1| (LIBM + 1) u
        Dq2 = Dr1 + |q2| u
        Dr2 = |lx| Dq2 + |r2| (LIBM + 1) u
        D   = Dr2 + |arg| u
        bound = (D + LIBM u) SLACK
    The cubic is evaluated in monomial form around ln x of -3 .. -7, so its terms cancel and D is hundreds of u for a narrow
    zone: that is the formula's own conditioning, not an allowance.  gain_start and gain_end are returned as stored: 0.
params64()              update_settings() (:180-205) with interpolation::hermite_cubic in float64 and a first-order bound
                        (class Q: one float32 rounding per operation, which covers the reference's double intermediates).
"""
import numpy as np

import compressor_ref as cr
from compressor_ref import LIBM, SLACK, U, Q, hold_samples  # noqa: F401

f32 = np.float32


def fresh_state(C):
    return {"e": np.zeros(C, f32), "peak": np.zeros(C, f32), "hold": np.zeros(C, np.uint32), "curve": np.zeros(C, np.uint32)}


def fresh_stats():
    return {"toggles": 0, "capped": 0, "restep_hold": 0, "per_channel": None}


def _step1(s, e, peak, hold, ta, tr, nhold):
    """Gate.cpp:284-306, one sample of one channel, float32 scalars."""
    d = f32(s - e)
    if d < 0:
        if hold > 0:
            hold -= 1
        else:
            e = f32(e + f32(tr * d))
            peak = e
    else:
        e = f32(e + f32(ta * d))
        if e >= peak:
            peak = e
            hold = nhold
    return e, peak, hold


def process_transcribed(x, state, ta, tr, nhold, end0, start1, stats=None):
    """One channel: x float32 [n]; state: (e, peak, hold, curve) as Python / numpy scalars, returned advanced.
    Returns env [n], curve_of_sample [n], state."""
    x = np.ascontiguousarray(x, f32)
    ta, tr, end0, start1 = f32(ta), f32(tr), f32(end0), f32(start1)
    nhold = int(nhold)
    fE, fPeak, nHoldCounter, nCurve = f32(state[0]), f32(state[1]), int(state[2]), int(state[3])
    samples = len(x)
    out = np.zeros(samples, f32)
    which = np.zeros(samples, np.uint32)
    stats = stats if stats is not None else fresh_stats()
    curr_i = prev_i = 0
    resteps = 0                                 # second steps taken on sample curr_i
    while prev_i < samples:
        c = nCurve
        e, peak, hold = fE, fPeak, nHoldCounter
        broke = False
        if nCurve == 0:
            while curr_i < samples:
                hold_before = hold
                e, peak, hold = _step1(x[curr_i], e, peak, hold, ta, tr, nhold)
                out[curr_i] = e
                if e > end0:
                    if resteps >= 1:            # THE CAP: this sample was stepped twice already; it keeps curve 0
                        stats["capped"] += 1
                    else:
                        nCurve = 1
                        broke = True
                        if hold_before > 0 and hold < hold_before:
                            stats["restep_hold"] += 1
                        break
                which[curr_i] = 0
                curr_i += 1
                resteps = 0
        else:
            while curr_i < samples:
                hold_before = hold
                e, peak, hold = _step1(x[curr_i], e, peak, hold, ta, tr, nhold)
                out[curr_i] = e
                if e < start1:
                    if resteps >= 1:
                        stats["capped"] += 1
                    else:
                        nCurve = 0
                        broke = True
                        if hold_before > 0 and hold < hold_before:
                            stats["restep_hold"] += 1
                        break
                which[curr_i] = 1
                curr_i += 1
                resteps = 0
        fE, fPeak, nHoldCounter = e, peak, hold
        if broke:
            stats["toggles"] += 1
            resteps = 1
        # dsp::gate_x1_gain(&out[prev_i], ..., &c->sKnee, curr_i - prev_i): samples [prev_i, curr_i) take curve c
        assert np.all(which[prev_i:curr_i] == c)
        prev_i = curr_i
    return out, which, (fE, fPeak, nHoldCounter, nCurve)


def process(x, state, ta, tr, nhold, end0, start1, stats=None):
    """x: float32 [C, n]; state: fresh_state() dict, advanced in place; the rest per-channel arrays.  Returns env [C, n] and
    the curve index of every sample [C, n] (uint32)."""
    x = np.ascontiguousarray(x, f32)
    C, n = x.shape
    ta, tr, end0, start1 = (np.broadcast_to(np.asarray(v, f32), (C,)) for v in (ta, tr, end0, start1))
    nhold = np.broadcast_to(np.asarray(nhold, np.uint32), (C,))
    e, peak, hold, curve = (state[k].copy() for k in ("e", "peak", "hold", "curve"))
    env, which = np.empty((C, n), f32), np.empty((C, n), np.uint32)
    stats = stats if stats is not None else fresh_stats()
    per = np.zeros(C, np.int64) if stats["per_channel"] is None else stats["per_channel"]
    one = np.uint32(1)

    def step(s, e, peak, hold, on):
        d = s - e
        neg = d < 0
        held = neg & (hold > 0)
        en = e + np.where(neg, tr, ta) * d                      # float32 arrays: the product rounds, then the sum
        rearm = ~neg & (en >= peak)
        e2 = np.where(held, e, en)
        peak2 = np.where((neg & ~held) | rearm, en, peak)
        hold2 = np.where(held, hold - one, np.where(rearm, nhold, hold)).astype(np.uint32)
        return np.where(on, e2, e), np.where(on, peak2, peak), np.where(on, hold2, hold), held & on

    def left(e, curve):
        return np.where(curve != 0, e < start1, e > end0)

    everyone = np.ones(C, bool)
    for i in range(n):
        s = x[:, i]
        e, peak, hold, held = step(s, e, peak, hold, everyone)
        crossed = left(e, curve)
        if crossed.any():
            curve = np.where(crossed, curve ^ one, curve).astype(np.uint32)
            e, peak, hold, _ = step(s, e, peak, hold, crossed)  # once, whatever it gives
            stats["toggles"] += int(np.count_nonzero(crossed))
            stats["restep_hold"] += int(np.count_nonzero(crossed & held))
            stats["capped"] += int(np.count_nonzero(crossed & left(e, curve)))
            per += crossed
        env[:, i], which[:, i] = e, curve
    state["e"], state["peak"], state["hold"], state["curve"] = e, peak, hold, curve
    stats["per_channel"] = per
    return env, which


# ---- the curves -------------------------------------------------------------------------------------------------------
def _curve(e, which, params, dtype):
    """(gain, bound in u) of the envelope e [C, n] with the knee which [C, n] selects; branches from the float32 values."""
    x32 = np.abs(np.ascontiguousarray(e, f32))
    which = np.broadcast_to(np.asarray(which), x32.shape) != 0

    def sel(name, idx=None):
        a, b = ([p["k"][j][name] if idx is None else p["k"][j][name][idx] for p in params] for j in range(2))
        return np.where(which, np.array(b, f32)[:, None], np.array(a, f32)[:, None])

    start, end = sel("start"), sel("end")
    gs, ge = sel("gain_start").astype(dtype), sel("gain_end").astype(dtype)
    h0, h1, h2, h3 = (sel("herm", i).astype(dtype) for i in range(4))
    with np.errstate(all="ignore"):
        lo, hi = x32 <= start, x32 >= end
        lx = np.log(x32.astype(np.float64)).astype(dtype)
        q1 = h0 * lx + h1
        r1 = q1 * lx
        q2 = r1 + h2
        r2 = q2 * lx
        arg = r2 + h3
        g = np.exp(arg.astype(np.float64)).astype(dtype)
        gain = np.where(lo, gs, np.where(hi, ge, g))
        alx = np.abs(lx)
        d = np.abs(h0 * lx) * (LIBM + 1) + np.abs(q1)
        d = alx * d + np.abs(r1) * (LIBM + 1)
        d = d + np.abs(q2)
        d = alx * d + np.abs(r2) * (LIBM + 1)
        d = (d + np.abs(arg)).astype(np.float64)
        bound = np.where(lo | hi, 0.0, (d + LIBM) * SLACK)
    return gain, bound


def gain64(e, which, params):
    return _curve(e, which, params, np.float64)[0]


def gain32(e, which, params):
    return _curve(e, which, params, f32)[0]


def gain_bound(e, which, params):
    return _curve(e, which, params, np.float64)[1]


# ---- update_settings() in float64 with a first-order error bound -------------------------------------------------------
def _hermite_cubic(x0, y0, k0, x1, y1, k1):
    """interpolation::hermite_cubic, src/main/misc/interpolation.cpp:112-131"""
    dx, dy = x1 - x0, y1 - y0
    kx = dy / dx
    xx1, xx2 = x1 * x1, x0 + x1
    a = ((Q.of(k0) + k1) * dx - Q(2.0) * dy) / (dx * dx * dx)
    b = ((kx - k0) + a * ((Q(2.0) * x0 - x1) * x0 - xx1)) / dx
    c = kx - a * (xx1 + xx2 * x0) - b * xx2
    d = y0 - x0 * (c + x0 * (b + x0 * a))
    return [a, b, c, d]


def params64(sample_rate, open_threshold, close_threshold, open_zone, close_zone, reduction, attack, release, hold):
    """Every quantity of update_settings() as a Q, keyed like flatten()."""
    sr = float(f32(sample_rate))
    red = float(f32(reduction))
    k707 = Q(float(f32(1.0 - np.sqrt(0.5)))).log()
    ms = Q(float(f32(0.001)))
    with np.errstate(all="ignore"):
        out = {"tau_attack": 1.0 - (k707 / (Q(float(f32(attack))) * ms * sr)).exp(),
               "tau_release": 1.0 - (k707 / (Q(float(f32(release))) * ms * sr)).exp()}
        for j, (th, zone) in enumerate(((open_threshold, open_zone), (close_threshold, close_zone))):
            th, zone = float(f32(th)), float(f32(zone))
            start, end = Q(th) * zone, Q(th)
            gs = Q(red) if red <= 1.0 else Q(1.0)
            ge = Q(1.0) if red <= 1.0 else 1.0 / Q(red)
            herm = _hermite_cubic(start.log(), gs.log(), 0.0, end.log(), ge.log(), 0.0)
            for n, v in (("start", start), ("end", end), ("gain_start", gs), ("gain_end", ge)):
                out["k%d.%s" % (j, n)] = v
            for i in range(4):
                out["k%d.herm%d" % (j, i)] = herm[i]
    return out


def flatten(p):
    out = {n: float(p[n]) for n in ("tau_attack", "tau_release")}
    for j in range(2):
        k = p["k"][j]
        for n in ("start", "end", "gain_start", "gain_end"):
            out["k%d.%s" % (j, n)] = float(k[n])
        for i in range(4):
            out["k%d.herm%d" % (j, i)] = float(k["herm"][i])
    return out


# ---- the settings and the input of the device tests ---------------------------------------------------------------------
def channel_settings(ch):
    """Different settings for every channel.  Open and close curves differ in threshold AND zone (close below open, as a
    gate with hysteresis is set), so a sample given the wrong curve gets a gain far outside its bound; every fifth channel
    has both zones at 1 (hard switches, no cubic), every seventh a reduction above 1."""
    r = np.random.default_rng(3000 + ch)
    open_db = r.uniform(-20.0, -14.0)
    close_db = open_db - r.uniform(6.0, 10.0)
    hard = ch % 5 == 4
    # The close curve's start stays above -40 dB and the times are short against the 40 to 90 samples of a burst of bursts():
    # the envelope gets through both curves within a segment.
    return dict(sample_rate=int(r.choice([44100, 48000, 96000])),
                open_threshold=float(f32(10.0 ** (open_db / 20.0))), close_threshold=float(f32(10.0 ** (close_db / 20.0))),
                open_zone=1.0 if hard else float(f32(10.0 ** (r.uniform(-9.0, -3.0) / 20.0))),
                close_zone=1.0 if hard else float(f32(10.0 ** (r.uniform(-10.0, -4.0) / 20.0))),
                reduction=float(f32(4.0 if ch % 7 == 6 else 10.0 ** (r.uniform(-40.0, -12.0) / 20.0))),
                attack=float(f32(r.uniform(0.05, 0.4))), release=float(f32(r.uniform(0.05, 0.15))),
                hold=float(f32(r.choice([0.0, 0.05, 0.1]))))


def bursts(seed, C, n):
    """Rectified noise whose level steps between -6 dB and -50 dB every 40 to 90 samples: the envelope rises through the open
    threshold and falls through the close one again and again."""
    r = np.random.default_rng(seed)
    x = np.empty((C, n), f32)
    for c in range(C):
        level, pos, loud = np.empty(n), 0, bool(r.integers(0, 2))
        while pos < n:
            seg = int(r.integers(40, 91))
            level[pos:pos + seg] = 10.0 ** ((-6.0 if loud else -50.0) / 20.0)
            pos, loud = pos + seg, not loud
        x[c] = (np.abs(r.standard_normal(n)) * 0.6 + 0.4) * level
    return x


def quiet(seed, C, n):
    """The same noise at -60 dB: below every close curve's start, so no gate ever toggles.  The odd channels are negative:
    their envelopes are, and the gain is that of the magnitude."""
    r = np.random.default_rng(seed)
    x = ((np.abs(r.standard_normal((C, n))) * 0.6 + 0.4) * 1e-3).astype(f32)
    x[1::2] *= f32(-1.0)
    return x
