"""float32 restatements of lsp::dspu::AutoGain and lsp::dspu::SimpleAutoGain (src/main/dynamics/AutoGain.cpp,
SimpleAutoGain.cpp of lsp-dsp-units) in numpy: vectorised over channels, one Python step per sample, every product, sum and
quotient rounded to float32 on its own.  Both count the branches they take, per channel, so that a test can say what its
input reached.  Line numbers are the reference's.  tests/test_gain_reference_host.py holds both, fed the reference's own recorded
parameters, to what the reference's compiled classes computed (tests/golden/autogain_ref_vectors.npz), bit for bit."""
import itertools
import math

import numpy as np

f32 = np.float32
F_QUICK_AMP, F_MAX_GAIN, F_SURGE_UP, F_SURGE_DOWN = 2, 4, 8, 16        # AutoGain.h:60-67
CURVE = ("x1", "x2", "t", "a", "b", "c", "d")


def ulp_of(x):
    return float(np.spacing(f32(abs(x))))


# ---- update() --------------------------------------------------------------------------------------------------------

def calc_compressor(x1, x2, y2):
    """AutoGain.cpp:180-195; c.a has a double literal in its expression and is rounded once."""
    x1, x2, y2 = f32(x1), f32(x2), f32(y2)
    dy = f32(y2 - x1)
    dx = f32(x2 - x1)
    dx1 = f32(f32(1.0) / dx)
    dx2 = f32(dx1 * dx1)
    b = f32(f32(f32(f32(3.0) * dy) * dx2) - f32(f32(2.0) * dx1))
    a = f32((1.0 - 2.0 * float(dy) * float(dx1)) * float(dx2))
    return {"x1": x1, "x2": x2, "t": y2, "a": a, "b": b, "c": f32(1.0), "d": x1}


def k_arguments(sample_rate, speeds, literal="div"):
    """The float32 arguments of the expf calls of update() (AutoGain.cpp:160-165, SimpleAutoGain.cpp:147-150): ksr goes
    through double and is rounded once; fall speeds are negated before the product."""
    with np.errstate(divide="ignore"):
        lit = (math.log(10.0) / float(f32(20.0))) if literal == "div" else (math.log(10.0) * float(f32(0.05)))
        ksr = f32(np.float64(lit) / np.float64(sample_rate))
        return [f32(f32(s) * ksr) for s in speeds]


def autogain_params(sample_rate=0, flags=0, short_grow=0.0, short_fall=0.0, long_grow=0.0, long_fall=0.0, silence=2.5119e-4,
                    deviation=1.99526, max_gain=3.98107):
    """AutoGain::update, :155-173.  The K's are exp in float64 of the float32 argument, rounded once (numpy's float32 exp is
    up to 2 ulp off): within half an ulp of the exact value, as libm's expf is within one."""
    dev = f32(deviation)
    args = k_arguments(sample_rate, (short_grow, -f32(short_fall), long_grow, -f32(long_fall)))
    q = np.sqrt(dev)
    with np.errstate(all="ignore"):
        k = [f32(np.exp(np.float64(a))) for a in args]
        p = {"short_kgrow": k[0], "short_kfall": k[1], "long_kgrow": k[2], "long_kfall": k[3],
             "short_comp": calc_compressor(f32(1.0) / dev, dev, 1.0), "out_comp": calc_compressor(q, f32(dev * q), dev),
             "silence": f32(silence), "deviation": dev, "max_gain": f32(max_gain), "flags": flags & (F_QUICK_AMP | F_MAX_GAIN)}
    return p, args


def simple_params(sample_rate=0, grow=0.0, fall=0.0, threshold=0.0, min_gain=0.000001, max_gain=1.0):
    """SimpleAutoGain::update, SimpleAutoGain.cpp:142-153."""
    args = k_arguments(sample_rate, (grow, -f32(fall)), literal="mul")
    with np.errstate(all="ignore"):
        return {"kgrow": f32(np.exp(np.float64(args[0]))), "kfall": f32(np.exp(np.float64(args[1]))), "threshold": f32(threshold), "min_gain": f32(min_gain),
                "max_gain": f32(max_gain)}, args


# ---- AutoGain::process -----------------------------------------------------------------------------------------------

AG_COUNTERS = ("silence", "surge_up_set", "surge_up_reset", "surge_down_set", "surge_down_reset", "short_fall", "short_grow",
               "long_fall", "long_grow", "long_equal", "knee", "saturated", "max_gain_hit", "max_gain_not_hit", "creep")
# what needs the quick amplifier (:240, :252) and what needs F_MAX_GAIN or its absence (:215-218)
AG_NEED_QUICK = ("surge_down_set", "surge_down_reset", "short_grow")
AG_NEED_LIMIT = ("max_gain_hit", "max_gain_not_hit")
# ... and both: without the quick amplifier the gain rises by 5 dB/s only and is nowhere near max_gain = +6 dB when the level returns
AG_NEED_BOTH = ("max_gain_hit",)
AG_NEED_NO_LIMIT = ("creep",)


class AutoGain:
    """`channels` units; params: one dict per channel as AutoGainBank.get_params / autogain_params returns."""

    def __init__(self, params):
        self.channels = len(params)
        self.gain = np.ones(self.channels, f32)             # fCurrGain
        self.out = np.ones(self.channels, f32)              # fOutGain
        self.surge = np.zeros(self.channels, np.uint32)     # F_SURGE_UP | F_SURGE_DOWN of nFlags
        self.counters = {k: np.zeros(self.channels, np.int64) for k in AG_COUNTERS}
        self.set_params(params)

    def set_params(self, params):
        col = lambda f: np.array([f(p) for p in params])
        for name in ("short_kgrow", "short_kfall", "long_kgrow", "long_kfall", "silence", "deviation", "max_gain"):
            setattr(self, name, col(lambda p: p[name]).astype(f32))
        self.sc = {k: col(lambda p: p["short_comp"][k]).astype(f32) for k in CURVE}
        self.oc = {k: col(lambda p: p["out_comp"][k]).astype(f32) for k in CURVE}
        self.quick = col(lambda p: (p["flags"] & F_QUICK_AMP) != 0)
        self.limit = col(lambda p: (p["flags"] & F_MAX_GAIN) != 0)

    def flags(self, ch):
        return int(self.surge[ch]) | (F_QUICK_AMP if self.quick[ch] else 0) | (F_MAX_GAIN if self.limit[ch] else 0)

    def _count(self, name, where):
        self.counters[name] += where

    def _eval_gain(self, c, x, active):
        """eval_curve(c, x) / x, :197-211"""
        v = x - c["x1"]
        y = ((c["a"] * v + c["b"]) * v + c["c"] * v) + c["d"]
        above, below = x >= c["x2"], x <= c["x1"]
        self._count("knee", active & ~above & ~below)
        return np.where(above, c["t"], np.where(below, x, y)) / x, above

    def step(self, sl, ss, le):
        """process_sample, :223-276, of every channel"""
        g, f, dev = self.gain, self.surge, self.deviation
        active = ~(ss <= self.silence)                                              # :226
        self._count("silence", ~active)
        nl, ns = sl * g, ss * g                                                     # :230-231
        is_up, is_down = f == F_SURGE_UP, self.quick & (f == F_SURGE_DOWN)          # :234-246
        up_reset = is_up & (ns <= le * dev)
        down_reset = ~is_up & is_down & (ns * dev > le)
        self._count("surge_up_reset", active & up_reset)
        self._count("surge_down_reset", active & down_reset)
        f = np.where(is_up, np.where(up_reset, 0, f), np.where(is_down, np.where(down_reset, 0, f), 0)).astype(np.uint32)
        red, _ = self._eval_gain(self.sc, ns / le, active)                          # :249-253
        set_up = red * dev < f32(1.0)
        set_down = ~set_up & self.quick & (ns * dev <= le)
        self._count("surge_up_set", active & set_up & ((f & F_SURGE_UP) == 0))
        self._count("surge_down_set", active & set_down & ((f & F_SURGE_DOWN) == 0))
        f = f | np.where(set_up, F_SURGE_UP, 0).astype(np.uint32) | np.where(set_down, F_SURGE_DOWN, 0).astype(np.uint32)
        up, down = (f & F_SURGE_UP) != 0, (f & F_SURGE_DOWN) != 0                   # :256-268
        calm = ~up & ~down
        self._count("short_fall", active & up)
        self._count("short_grow", active & ~up & down)
        self._count("long_fall", active & calm & (nl > le))
        self._count("long_grow", active & calm & (nl < le))
        self._count("long_equal", active & calm & (nl == le))
        k = np.where(up, self.short_kfall, np.where(down, self.short_kgrow,
                     np.where(nl > le, self.long_kfall, np.where(nl < le, self.long_kgrow, f32(1.0))))).astype(f32)
        g2 = g * k
        red2, saturated = self._eval_gain(self.oc, (ss * g2) / le, active)          # :271-272
        self._count("saturated", active & saturated)
        g2 = g2 * red2
        self.gain = np.where(active, g2, g).astype(f32)                             # :274
        self.surge = np.where(active, f, self.surge).astype(np.uint32)
        hit = self.gain >= self.max_gain                                            # apply_gain_limiting, :213-221
        self._count("max_gain_hit", self.limit & hit)
        self._count("max_gain_not_hit", self.limit & ~hit)
        self._count("creep", ~self.limit)
        grown = self.out * self.long_kgrow
        self.out = np.where(self.limit, np.where(hit, self.max_gain / self.gain, f32(1.0)),
                            np.where(grown < f32(1.0), grown, f32(1.0))).astype(f32)
        return self.gain * self.out

    def process(self, llong, lshort, lexp):
        """process(vca, llong, lshort, lexp, count), :278-296; rows [channels][count]; lexp rows or one level per channel"""
        llong, lshort, lexp = np.asarray(llong, f32), np.asarray(lshort, f32), np.asarray(lexp, f32)
        vca = np.empty_like(llong)
        with np.errstate(all="ignore"):
            for i in range(llong.shape[1]):
                vca[:, i] = self.step(llong[:, i], lshort[:, i], lexp if lexp.ndim == 1 else lexp[:, i])
        return vca


# the signal of the tests: sample rate 1000 Hz, so that gains move visibly within a thousand samples
SETTINGS = dict(sample_rate=1000, short_grow=160.0, short_fall=320.0, long_grow=5.0, long_fall=10.0,
                silence=float(f32(2.5119e-4)), deviation=float(f32(1.99526)), max_gain=2.0)
LEXP = f32(0.1)
LEVELS = (0.1, 1.0, 0.004, 1e-5, 0.1, 0.13, 0.1)
LENGTHS = (150, 200, 200, 100, 150, 150, 150)


def signal(seed, channels, lengths=LENGTHS):
    """(llong, lshort, lexp) rows: lshort steps through LEVELS (a surge up, a deep drop, silence, back, a slow rise and fall)
    times exp(0.05 N(0, 1)); llong is a one-pole (0.02) of it.  The crafted sample: llong[0] is lexp, which a unit with gain 1
    meets as `nl == le`."""
    rng = np.random.default_rng(seed)
    n = sum(lengths)
    steps = np.concatenate([np.full(k, v) for v, k in zip(itertools.cycle(LEVELS), lengths)])
    lshort = (steps[None, :] * np.exp(0.05 * rng.standard_normal((channels, n)))).astype(f32)
    llong = np.empty_like(lshort)
    y = lshort[:, 0].copy()
    for i in range(n):
        y = (y + f32(0.02) * (lshort[:, i] - y)).astype(f32)
        llong[:, i] = y
    llong[:, 0] = LEXP
    return llong, lshort, np.full((channels, n), LEXP, f32)


def settings_of(ch):
    """SETTINGS with speeds, deviation and max_gain of the channel's own (within a few percent)"""
    k = ch % 7
    return dict(SETTINGS, short_grow=160.0 + k, short_fall=320.0 - 2 * k, long_grow=5.0 + 0.125 * k, long_fall=10.0 - 0.25 * k,
                deviation=float(f32(1.99526 + 0.01 * k)), max_gain=2.0 - 0.03125 * k)


def switches(ch):
    """all four combinations of quick amplifier x max-gain limiting across channels; channel 0 has both"""
    return (ch % 2 == 0), (ch % 4 < 2)


def expected_counters(quick, limit):
    """the counters signal() reaches with these switches on a fresh unit (`creep` counts the samples of the other mode of
    apply_gain_limiting; that fOutGain really creeps up from below 1 takes a unit whose limiting was just switched off)"""
    return [k for k in AG_COUNTERS if (quick or k not in AG_NEED_QUICK) and (limit or k not in AG_NEED_LIMIT) and
            (not limit or k not in AG_NEED_NO_LIMIT) and ((quick and limit) or k not in AG_NEED_BOTH)]


# ---- SimpleAutoGain --------------------------------------------------------------------------------------------------

SAG_COUNTERS = ("grow", "fall", "equal", "at_min", "at_max", "inside")


def lsp_limit(x, lo, hi):
    return np.where(x < lo, lo, np.where(x > hi, hi, x)).astype(f32)


class SimpleAutoGain:
    """`channels` units; params: one dict per channel as SimpleAutoGainBank.get_params / simple_params returns."""

    def __init__(self, params):
        self.channels = len(params)
        self.gain = np.ones(self.channels, f32)
        self.counters = {k: np.zeros(self.channels, np.int64) for k in SAG_COUNTERS}
        self.set_params(params)

    def set_params(self, params):
        for name in ("kgrow", "kfall", "threshold", "min_gain", "max_gain"):
            setattr(self, name, np.array([p[name] for p in params], f32))

    # the three setters that act on fCurrGain at once, SimpleAutoGain.cpp:108-135 (their early returns are the caller's)
    def set_max_gain(self, ch, value):
        self.max_gain[ch] = value
        self.gain[ch] = self.gain[ch] if self.gain[ch] < f32(value) else f32(value)         # lsp_min

    def set_min_gain(self, ch, value):
        self.min_gain[ch] = value
        self.gain[ch] = self.gain[ch] if self.gain[ch] > f32(value) else f32(value)         # lsp_max

    def set_gain(self, ch, lo, hi):
        self.min_gain[ch], self.max_gain[ch] = lo, hi
        self.gain[ch] = lsp_limit(self.gain[ch], f32(lo), f32(hi))

    def process(self, src):
        """process(dst, src, count), :155-175"""
        src = np.asarray(src, f32)
        dst = np.empty_like(src)
        g = self.gain
        for i in range(src.shape[1]):
            s = src[:, i] * g
            below, above = s < self.threshold, s > self.threshold
            g = g * np.where(below, self.kgrow, np.where(above, self.kfall, f32(1.0))).astype(f32)
            lo, hi = g < self.min_gain, ~(g < self.min_gain) & (g > self.max_gain)
            g = np.where(lo, self.min_gain, np.where(hi, self.max_gain, g)).astype(f32)
            for name, where in (("grow", below), ("fall", above), ("equal", ~below & ~above), ("at_min", lo), ("at_max", hi),
                                ("inside", ~lo & ~hi)):
                self.counters[name] += where
            dst[:, i] = g
        self.gain = g
        return dst


def simple_signal(seed, channels, n):
    """levels around a threshold of 0.1: far above, far below (so that a gain within [0.2, 5] ends at either limit), and noise
    across it"""
    rng = np.random.default_rng(seed)
    third = n // 3
    steps = np.concatenate([np.full(third, 0.9), np.full(third, 0.005), np.full(n - 2 * third, 0.1)])
    return (steps[None, :] * np.exp(0.2 * rng.standard_normal((channels, n)))).astype(f32)
