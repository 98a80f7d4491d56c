"""CPU yardsticks for lsp::dspu::Limiter (src/main/dynamics/Limiter.cpp) for the tests, in the manner of compressor_ref.py.

params_ref()    update_settings() (:396-548) with init_sat / init_exp / init_line (:278-394).  Integer fields exactly; float
                fields as (float64 value, bound).  interpolation::hermite_cubic and ::exponent (interpolation.cpp:112-131,
                :224-230) run in double on arguments that are exact in float32 (or, 2.0f / attack and its products, are
                formed in float32 here as there), so their coefficients are held to the one rounding of the final store
                (u = 2^-24 relative); everything else is float32 and carries one rounding per operation (class Q).
shape64()       the patch of apply_*_patch (:609-673) without amp, in float64 on given coefficients, with the bound
                (operations + 4 for expf) u on the magnitudes of the partial results.
Limiter         process() (:695-784) and what update_settings() does to the gain buffer (:402-419), for ONE channel in numpy
                float32, every product, sum and quotient rounded once.  It keeps the reference's long buffer, nHead and the
                move at nHead >= 8 ML, with 8 guard floats in front and 3 ML + 32 behind (the reference writes outside its
                allocation with ML < 8).  The table shape[t] and the ALR parameters are GIVEN (the library's own), so what
                is compared bit for bit is the loop, not libm.  dsp::max_index is "first index of the maximum"
                (numpy argmax), dsp::abs_mul3(dst, a, b) is a |b|: lsp-dsp-lib is absent, DESIGN section 4 says so.
                The patch loop carries the bank's bound of 2 n patches per chunk and counts the patches.

tests/test_gain_reference_host.py holds Limiter and Unit, fed the reference's own recorded parameters, to what the reference's
compiled class computed (tests/golden/limiter_ref_vectors.npz): gain, nHead and the ALR envelope bit for bit.  The two primitives
above stay this file's reading.
"""
import numpy as np

from compressor_ref import LIBM, SLACK, U, Q

f32 = np.float32
f64 = np.float64

MODES = ("HERM_THIN", "HERM_WIDE", "HERM_TAIL", "HERM_DUCK", "EXP_THIN", "EXP_WIDE", "EXP_TAIL", "EXP_DUCK",
         "LINE_THIN", "LINE_WIDE", "LINE_TAIL", "LINE_DUCK")
BUF_GRANULARITY = 8192
PEAKS_MAX = 32                      # LIMITER_PEAKS_MAX
GAIN_LOWERING = f32(0.9886)
GUARD = 8
DEFAULTS = {"sample_rate": 0, "mode": 0, "threshold": 1.0, "lookahead": 0.0, "attack": 0.0, "release": 0.0, "knee": 0.50118,
            "alr_attack": 10.0, "alr_release": 50.0, "alr_knee": 0.56234}       # construct(), :47-73


def millis_to_samples(sr, ms):
    """units.h: (time * 0.001f) * sr in float32."""
    return f32(f32(f32(ms) * f32(0.001)) * f32(sr))


def stored_alr_knee(knee):
    """set_alr_knee, :220-229."""
    knee = f32(knee)
    return f32(f32(1.0) / knee) if knee > 1 else knee


def _limit(v, lo, hi):
    """lsp_limit: below lo it is lo, else above hi it is hi -- hi may be under lo."""
    return lo if v < lo else (hi if v > hi else v)


def _widths(width, attack, release):
    """:286-308 (and :368-390): nAttack, nPlane, nRelease, nMiddle for THIN, WIDE, TAIL, DUCK = 0 .. 3."""
    if width == 0:
        a, p = attack, attack
    elif width == 2:
        a, p = attack // 2, attack
    elif width == 3:
        a, p = attack, attack + release // 2
    else:
        a, p = attack // 2, attack + release // 2
    return {"attack": a, "plane": p, "release": attack + release + 1, "middle": attack}


def _rounded(v):
    """A coefficient computed in double and stored as a float: the value, and the one rounding."""
    v = f64(v)
    return v, (U * abs(v)) * SLACK + 1e-300 if np.isfinite(v) else np.inf


def _hermite_cubic(x0, y0, k0, x1, y1, k1):
    """interpolation.cpp:112-131; the arguments are small integers, every float32 stretch of the reference is exact."""
    x0, y0, k0, x1, y1, k1 = (f64(v) for v in (x0, y0, k0, x1, y1, k1))
    with np.errstate(all="ignore"):
        dx, dy = x1 - x0, y1 - y0
        kx = dy / dx
        xx1, xx2 = x1 * x1, x0 + x1
        a = ((k0 + k1) * dx - 2.0 * dy) / (dx * dx * dx)
        b = ((kx - k0) + a * ((2.0 * x0 - x1) * x0 - xx1)) / dx
        c = kx - a * (xx1 + xx2 * x0) - b * xx2
        d = y0 - x0 * (c + x0 * (b + x0 * a))
    return [_rounded(v) for v in (a, b, c, d)]


def _exponent(x0, y0, x1, y1, k):
    """interpolation.cpp:224-230: k (x0 - x1) and k x0 in float32, exp and the quotients in double, p[0] read back as stored."""
    x0, y0, x1, y1, k = (f32(v) for v in (x0, y0, x1, y1, k))
    with np.errstate(all="ignore"):
        e = np.exp(f64(f32(k * f32(x0 - x1))))
        p0 = (f64(y0) - e * f64(y1)) / (1.0 - e)
        p1 = f64(f32(y0 - f32(p0))) / np.exp(f64(f32(k * x0)))
    # p[1] hangs on the stored p[0]: its rounding may move y0 - p[0] by u |p0|
    v1, b1 = _rounded(p1)
    with np.errstate(all="ignore"):
        b1 = b1 + (U * abs(p0) / np.exp(f64(f32(k * x0)))) * SLACK
    return [_rounded(p0), (v1, b1), (f64(k), 0.0)]


def _linear(x0, y0, x1, y1):
    """interpolation.cpp:233-237, float32."""
    p0 = (Q(y1) - y0) / (Q(x1) - x0)
    p1 = y0 - p0 * x0
    return [(p0.v, p0.err), (p1.v, p1.err)]


def params_ref(**settings):
    """-> (ints, floats): ints the exact fields, floats name -> (float64 value, bound).  settings: DEFAULTS' keys, the float32
    values the setters keep (alr_knee as stored)."""
    s = dict(DEFAULTS, **settings)
    sr, mode = int(s["sample_rate"]), int(s["mode"])
    la = int(millis_to_samples(sr, s["lookahead"]))                                 # :406
    attack = int(millis_to_samples(sr, s["attack"]))                                # :280-281, truncation towards zero
    release = int(millis_to_samples(sr, s["release"]))
    floats = {}
    with np.errstate(all="ignore"):
        if mode < 4:                                                                # init_sat, :278-312
            attack = _limit(attack, 8, la)
            release = _limit(attack, 8, la * 2)                                     # :284: from ATTACK
            w = _widths(mode, attack, release)
            va = _hermite_cubic(-1.0, 0.0, 0.0, w["attack"], 1.0, 0.0)
            vr = _hermite_cubic(w["plane"], 1.0, 0.0, w["release"], 0.0, 0.0)
        else:                                                                       # :316-325, :357-366: the upper limit wins
            attack = la if attack > la else (8 if attack < 8 else attack)
            release = la * 2 if release > la * 2 else (8 if release < 8 else release)
            if mode < 8:                                                            # init_exp, :314-353
                w = _widths(1, attack, release)                                     # :327-346 test for LM_HERM_*: always WIDE
                va = _exponent(-1.0, 0.0, w["attack"], 1.0, f32(2.0) / f32(attack)) + [(0.0, 0.0)]
                vr = _exponent(w["plane"], 1.0, w["release"], 0.0, f32(2.0) / f32(release)) + [(0.0, 0.0)]
            else:                                                                   # init_line, :355-394
                w = _widths(mode - 8, attack, release)
                va = _linear(-1.0, 0.0, float(w["attack"]), 1.0) + [(0.0, 0.0)] * 2
                vr = _linear(float(w["plane"]), 1.0, float(w["release"]), 0.0) + [(0.0, 0.0)] * 2
        for i in range(4):
            floats["v_attack%d" % i], floats["v_release%d" % i] = va[i], vr[i]

        # :459-469
        thr, knee, aknee = (float(f32(s[n])) for n in ("threshold", "knee", "alr_knee"))
        thresh = (Q(thr) * knee) * 0.354813                                         # GAIN_AMP_M_9_DB
        ks = thresh * aknee
        ke = 2.0 * thresh - ks
        h0 = (Q(1.0) - 0.0) * 0.5 / (ks - ke)                                       # hermite_quadratic(ks, ks, 1, ke, 0), :103-109
        h1 = 1.0 - 2.0 * h0 * ks
        h2 = ks - (h0 * ks + h1) * ks
        k707 = Q(float(f32(1.0 - np.sqrt(0.5)))).log()
        att, rel = millis_to_samples(sr, s["alr_attack"]), millis_to_samples(sr, s["alr_release"])
        ta = Q(1.0) if att < 1 else 1.0 - (k707 / (Q(float(f32(s["alr_attack"]))) * float(f32(0.001)) * float(sr))).exp()
        tr = Q(1.0) if rel < 1 else 1.0 - (k707 / (Q(float(f32(s["alr_release"]))) * float(f32(0.001)) * float(sr))).exp()
    for n, q in (("ks", ks), ("ke", ke), ("gain", thresh), ("hermite0", h0), ("hermite1", h1), ("hermite2", h2),
                 ("tau_attack", ta), ("tau_release", tr), ("threshold", Q(thr))):
        floats[n] = (q.v, q.err)
    ints = dict(w, lookahead=la, mode=mode)
    return ints, floats


def flatten(p):
    """LimiterBank.compute_params()'s dict -> (ints, floats) keyed like params_ref()."""
    ints = dict((n, int(p[n])) for n in ("lookahead", "mode", "attack", "plane", "release", "middle"))
    floats = dict((n, float(p[n])) for n in ("threshold", "ks", "ke", "gain", "tau_attack", "tau_release"))
    for n, k in (("v_attack", 4), ("v_release", 4), ("hermite", 3)):
        for i in range(k):
            floats["%s%d" % (n, i)] = float(p[n][i])
    return ints, floats


def shape64(p):
    """-> (shape, bound) float64 [nRelease] on the coefficients of p (LimiterBank.compute_params()'s dict)."""
    n, mode = int(p["release"]), int(p["mode"])
    t = np.arange(n, dtype=f64)
    out, bound = np.ones(n, f64), np.zeros(n, f64)
    for sel, v in ((t < p["attack"], p["v_attack"]), (t >= p["plane"], p["v_release"])):
        v = [f64(c) for c in v]
        x = t[sel]
        if mode < 4:                                    # ((v0 x + v1) x + v2) x + v3: six operations
            q1 = v[0] * x + v[1]
            q2 = q1 * x + v[2]
            y = q2 * x + v[3]
            mag = (np.abs(v[0] * x) + np.abs(q1)) * x * x + (np.abs(q1 * x) + np.abs(q2)) * x + np.abs(q2 * x) + np.abs(y)
            ops = 1.0
        elif mode < 8:                                  # v0 + v1 expf(v2 x): three operations and expf
            arg = v[2] * x
            ex = np.exp(arg)
            y = v[0] + v[1] * ex
            mag = np.abs(v[1] * ex) * (np.abs(arg) + LIBM + 1.0) + np.abs(y)
            ops = 1.0
        else:                                           # v0 x + v1: two operations
            y = v[0] * x + v[1]
            mag = np.abs(v[0] * x) + np.abs(y)
            ops = 1.0
        out[sel], bound[sel] = y, ops * U * mag * SLACK
    return out, bound


class Limiter:
    """One channel.  params: LimiterBank.get_params()'s dict (nLookahead, nMiddle, fThreshold and the ALR fields are read);
    shape: the float32 table of nRelease entries."""

    def __init__(self, max_lookahead, last_of_ties=False):
        self.last_of_ties = last_of_ties                # NOT the reference: for showing that a test can tell the two apart
        self.ml = ml = int(max_lookahead)                                           # init, :87-109
        self.size = ml * 12 + BUF_GRANULARITY
        self.buf = np.ones(GUARD + self.size + 3 * ml + 32, f32)
        self.head = 0
        self.env = f32(0.0)
        self.alr = False
        self.patches = self.chunks = self.overrun = 0
        self.patches_per_chunk = []
        self.outside = 0                                # patch entries outside [vGainBuf, vGainBuf + buf_size)

    def set_alr(self, enable):                                                      # :211-218
        self.alr = bool(enable)
        if not enable:
            self.env = f32(0.0)

    def refill(self):                                                               # UP_SR, :403-404
        g = GUARD + self.head
        self.buf[g:g + self.ml * 3 + BUF_GRANULARITY] = 1.0

    def lower_threshold(self, new, old):                                            # :411-416
        g = GUARD + self.head
        self.buf[g:g + self.ml] *= f32(f32(new) / f32(old))

    def _alr(self, gbuf, tmp, p):                                                   # process_alr, :675-693
        e = self.env
        ta, tr, ks, ke, gain = (f32(p[n]) for n in ("tau_attack", "tau_release", "ks", "ke", "gain"))
        h0, h1, h2 = (f32(v) for v in p["hermite"])
        for i in range(len(tmp)):
            s = tmp[i]
            e = f32(e + f32((ta if s > e else tr) * f32(s - e)))
            if e >= ke:
                gbuf[i] = f32(gbuf[i] * f32(gain / e))
            elif e > ks:
                gbuf[i] = f32(gbuf[i] * f32(f32(f32(h0 * e) + h1) + f32(h2 / e)))
        self.env = e

    def process(self, sc, params, shape):
        """-> gain float32 [len(sc)]."""
        sc = np.ascontiguousarray(sc, f32)
        shape = np.ascontiguousarray(shape, f32)
        thr, la, middle = f32(params["threshold"]), int(params["lookahead"]), int(params["middle"])
        nrel = len(shape)
        assert nrel == max(int(params["release"]), 0)
        ml, out = self.ml, np.empty(len(sc), f32)
        self.patches = self.chunks = 0
        self.patches_per_chunk = []
        with np.errstate(all="ignore"):
            for c0 in range(0, len(sc), BUF_GRANULARITY):
                x = np.abs(sc[c0:c0 + BUF_GRANULARITY])
                n = len(x)
                g0 = GUARD + self.head + ml                                         # gbuf = &vGainBuf[nHead + ML]
                gbuf = self.buf[g0:]
                gbuf[3 * ml:3 * ml + n] = 1.0                                       # :707
                tmp = gbuf[:n] * x                                                  # :708
                if self.alr:                                                        # :709-713
                    self._alr(gbuf, tmp, params)
                    tmp = gbuf[:n] * x
                knee, count = f32(1.0), 0
                for it in range(2 * n + 1):                                         # the bank's bound; the reference: while (true)
                    peak = int(np.argmax(tmp))                                      # first index of the maximum
                    if self.last_of_ties:
                        peak = n - 1 - int(np.argmax(tmp[::-1]))
                    s = tmp[peak]
                    if s <= thr:
                        break
                    if it == 2 * n:
                        self.overrun = 1
                        break
                    k = f32(f32(s - f32(f32(thr * knee) - f32(0.000001))) / s)      # :727
                    a = g0 + peak - middle
                    if a < GUARD or a + nrel > GUARD + self.size:
                        self.outside += 1
                    self.buf[a:a + nrel] *= f32(1.0) - k * shape                    # :609-673 with the table
                    lo, hi = max(peak - middle, 0), min(peak - middle + nrel, n)
                    tmp[lo:hi] = gbuf[lo:hi] * x[lo:hi]                             # :763, where it can have changed
                    count += 1
                    if count % PEAKS_MAX == 0:                                      # :766-767
                        knee = f32(knee * GAIN_LOWERING)
                out[c0:c0 + n] = self.buf[g0 - la:g0 - la + n]                      # :771
                self.head += n
                if self.head >= ml * 8:                                             # :773-777
                    self.buf[GUARD:GUARD + ml * 4] = self.buf[GUARD + self.head:GUARD + self.head + ml * 4].copy()
                    self.head = 0
                self.patches += count
                self.chunks += 1
                self.patches_per_chunk.append(count)
        return out


UP_SR, UP_LK, UP_MODE, UP_OTHER, UP_THRESH, UP_ALR, UP_ALL = 1, 2, 4, 8, 16, 32, 63          # Limiter.h:60-70


class Unit:
    """The setters (:111-229) and update_settings() (:396-548) around a Limiter: nUpdate, fThreshold beside fReqThreshold, and
    what an update does to the gain buffer.  The computed parameters and the table come from `compute`, a callable that takes the
    settings as keywords (threshold: fThreshold after the update) and returns (params, shape): the library's."""

    def __init__(self, max_sample_rate, max_lookahead_ms, **kw):
        self.max_lookahead = f32(max_lookahead_ms)
        self.lim = Limiter(int(millis_to_samples(max_sample_rate, max_lookahead_ms)), **kw)
        self.s = dict((k, f32(v) if isinstance(v, float) else v) for k, v in DEFAULTS.items())
        self.thr = f32(1.0)
        self.update = UP_ALL
        self.params = self.shape = None

    def _set(self, name, value, flags):
        value = f32(value) if isinstance(self.s[name], np.floating) else int(value)
        if self.s[name] == value:
            return
        self.s[name] = value
        self.update |= flags

    def set_sample_rate(self, sr):
        self._set("sample_rate", sr, UP_SR | UP_ALR | UP_MODE)

    def set_mode(self, mode):
        self._set("mode", mode, UP_MODE)

    def set_threshold(self, threshold, immediate=False):                            # :133-144
        if self.s["threshold"] == f32(threshold):
            return
        self.s["threshold"] = f32(threshold)
        if immediate:
            self.thr = f32(threshold)
        self.update |= UP_THRESH | UP_ALR

    def set_attack(self, v):
        self._set("attack", v, UP_OTHER)

    def set_release(self, v):
        self._set("release", v, UP_OTHER)

    def set_lookahead(self, v):                                                     # :164-176
        self._set("lookahead", min(f32(v), self.max_lookahead), UP_LK)

    def set_knee(self, v):
        self._set("knee", v, UP_ALR)

    def set_alr(self, enable):
        self.lim.set_alr(enable)

    def set_alr_attack(self, v):
        self._set("alr_attack", v, UP_ALR)

    def set_alr_release(self, v):
        self._set("alr_release", v, UP_ALR)

    def set_alr_knee(self, v):                                                      # :220-229: compared before it is inverted
        if f32(v) == self.s["alr_knee"]:
            return
        self.s["alr_knee"] = stored_alr_knee(v)
        self.update |= UP_ALR

    def latency(self):
        return int(millis_to_samples(self.s["sample_rate"], self.s["lookahead"]))

    def update_settings(self, compute):
        if self.update == 0:
            return
        if self.update & UP_SR:
            self.lim.refill()
        if self.update & UP_THRESH:
            if self.s["threshold"] < self.thr:
                self.lim.lower_threshold(self.s["threshold"], self.thr)
            self.thr = self.s["threshold"]
        self.params, self.shape = compute(**dict(self.s, threshold=self.thr))
        self.update = 0

    def process(self, sc):
        return self.lim.process(sc, self.params, self.shape)


def bursts(seed, channels, n, bed=0.05, level=1.0, every=97):
    """A quiet bed of noise with bursts of a few samples to a few dozen, of 1 .. 3 x level, about every `every` samples."""
    rng = np.random.default_rng(seed)
    x = (bed * rng.standard_normal((channels, n))).astype(f32)
    for c in range(channels):
        at = int(rng.integers(0, every))
        while at < n:
            ln = int(rng.integers(1, 40))
            x[c, at:at + ln] += (level * rng.uniform(1.0, 3.0) * rng.standard_normal(min(ln, n - at))).astype(f32)
            at += int(rng.integers(every // 2, 2 * every))
    return x


def delayed(stream, start, count, latency):
    """audio_stream[i - latency] for i in [start, start + count), zero in front of the stream."""
    idx = np.arange(start, start + count) - latency
    return np.where(idx >= 0, stream[np.maximum(idx, 0)], f32(0.0)).astype(f32)
