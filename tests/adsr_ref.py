"""A numpy restatement of lsp::dspu::ADSREnvelope (src/main/util/ADSREnvelope.cpp): construct(), the setters, update_settings()
with the two Hermite designs of misc/interpolation.cpp, and the five array operations in closed form.  float32 throughout, one
rounding per operation, in the reference's order; expf(-fKT) of the designer is the host libm's, as in the reference.  In an EXP
segment e = expf(u * fKT) is the float64 exp rounded once to float32 (what the device computes); `shift` moves it to one of its two
float32 neighbours, which is as far as a C library's expf is allowed to be from it in the tests.

MUTATION names one deliberate mistake at a time; tests/test_adsr_host.py checks that the recorded vectors catch each of them."""
import ctypes
import ctypes.util

import numpy as np

f32 = np.float32
NONE, LINE, LINE2, CUBIC, QUADRO, EXP = range(6)
ATTACK, DECAY, SLOPE, RELEASE = range(4)
USE_HOLD, USE_BREAK, RECONFIGURE = 1, 2, 4
(SET_ATTACK_TIME, SET_HOLD_TIME, SET_DECAY_TIME, SET_SLOPE_TIME, SET_RELEASE_TIME, SET_ATTACK_CURVE, SET_DECAY_CURVE, SET_SLOPE_CURVE,
 SET_RELEASE_CURVE, SET_ATTACK_FUNCTION, SET_DECAY_FUNCTION, SET_SLOPE_FUNCTION, SET_RELEASE_FUNCTION, SET_BREAK_LEVEL,
 SET_SUSTAIN_LEVEL, SET_HOLD_ENABLED, SET_BREAK_ENABLED, SET_ATTACK, SET_HOLD, SET_DECAY, SET_BREAK, SET_SLOPE, SET_RELEASE,
 UPDATE) = range(24)
ST_BEFORE, ST_ATTACK, ST_HOLD, ST_DECAY, ST_SLOPE, ST_SUSTAIN, ST_RELEASE, ST_AFTER = range(8)
PROCESS, PROCESS_MUL, GENERATE, GENERATE_MUL, GENERATE_MUL_SRC = range(5)
MUTATIONS = ("le_segment_end", "no_hold", "zero_step_t0", "no_floor", "stage0_multiply", "fma")
MUTATION = None

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.expf.restype, _libm.expf.argtypes = ctypes.c_float, [ctypes.c_float]


def expf(x):
    return f32(_libm.expf(float(x)))


def limit01(x):
    x = f32(x)
    return f32(0) if x < 0 else (f32(1) if x > 1 else x)


def limit_range(t, prev):
    return limit01(t if t > prev else prev)


def solve_matrix(m, nvars):
    """interpolation.cpp:61-98 on a float64 [nvars, nvars + 1] matrix"""
    eps = np.float64(f32(1e-20))
    for i in range(nvars):
        if abs(m[i, i]) < eps:
            for j in range(i, nvars):
                if abs(m[j, i]) >= eps:
                    m[[i, j], i:] = m[[j, i], i:]
                    break
        for j in range(i + 1, nvars):
            if abs(m[j, i]) < eps:
                continue
            k = m[j, i] / m[i, i]
            m[j, i] = 0.0
            for c in range(i + 1, nvars + 1):
                m[j, c] -= k * m[i, c]
    c = np.zeros(nvars, np.float64)
    for i in range(nvars - 1, -1, -1):
        s = m[i, nvars]
        for q in range(i + 1, nvars):
            s += m[i, q] * c[q]
        c[i] = -s / m[i, i]
    return c


def hermite_cubic(x0, y0, k0, x1, y1, k1):
    """interpolation.cpp:112-131: differences and products of the float arguments are float32, the rest float64"""
    d = np.float64
    x0, y0, k0, x1, y1, k1 = (f32(v) for v in (x0, y0, k0, x1, y1, k1))
    with np.errstate(all="ignore"):
        dx, dy = d(x1 - x0), d(y1 - y0)
        kx = dy / dx
        xx1, xx2 = d(x1 * x1), d(x0 + x1)
        a = (d(k0 + k1) * dx - d(f32(2)) * dy) / (dx * dx * dx)
        b = ((kx - d(k0)) + a * (d((f32(2) * x0 - x1) * x0) - xx1)) / dx
        c = kx - a * (xx1 + xx2 * d(x0)) - b * xx2
        e = d(y0) - d(x0) * (c + d(x0) * (b + d(x0) * a))
        return np.array([a, b, c, e]).astype(f32)


def hermite_quadro(x0, y0, k0, x1, y1, k1, x2, y2):
    """interpolation.cpp:134-177"""
    m = np.zeros((5, 6), np.float64)
    X, Y, K = [np.float64(f32(v)) for v in (x0, x1, x2)], [np.float64(f32(v)) for v in (y0, y1, y2)], [np.float64(f32(v)) for v in (k0, k1)]
    with np.errstate(all="ignore"):
        for i in range(3):
            x = X[i]
            x2_ = x * x
            x3 = x * x2_
            m[i] = [x2_ * x2_, x3, x2_, x, 1.0, -Y[i]]
            if i < 2:
                m[i + 3] = [4.0 * x3, 3.0 * x2_, 2.0 * x, 1.0, 0.0, -K[i]]
        return solve_matrix(m, 5).astype(f32)


def _fma(a, b, c):
    return (np.asarray(a, np.float64) * np.float64(b) + np.float64(c)).astype(f32)


class Envelope:
    def __init__(self):                                     # construct(), :40-58
        self.time = [f32(0)] * 4
        self.curve = [f32(0.5)] * 4
        self.fn = [NONE] * 4
        self.params = [np.zeros(6, f32) for _ in range(4)]
        self.hold_time = self.break_level = self.sustain_level = f32(0)
        self.flags = RECONFIGURE

    # -- the setters, :65-117
    def _param(self, get, put, value):
        v = limit01(value)
        if get() == v:
            return
        put(v)
        self.flags |= RECONFIGURE

    def _list_param(self, lst, k, value):
        self._param(lambda: lst[k], lambda v: lst.__setitem__(k, v), value)

    def _attr_param(self, name, value):
        self._param(lambda: getattr(self, name), lambda v: setattr(self, name, v), value)

    def _function(self, part, fn):
        if self.fn[part] != fn:
            self.fn[part] = fn
            self.flags |= RECONFIGURE

    def _flag(self, flag, on):
        if bool(on) != bool(self.flags & flag):
            self.flags = ((self.flags | flag) if on else (self.flags & ~flag)) | RECONFIGURE

    def _curve(self, part, time, curve, fn):
        time, curve = limit01(time), limit01(curve)
        if self.time[part] == time and self.curve[part] == curve and self.fn[part] == fn:
            return
        self.time[part], self.curve[part], self.fn[part] = time, curve, fn
        self.flags |= RECONFIGURE

    def apply(self, op):
        """One row of an operation list: the setter's number and up to three arguments."""
        what, a, b, c = int(op[0]), op[1], op[2], op[3]
        parts = (ATTACK, DECAY, SLOPE, RELEASE)
        if what == SET_HOLD_TIME:
            self._attr_param("hold_time", a)
        elif what <= SET_RELEASE_TIME:
            self._list_param(self.time, {SET_ATTACK_TIME: ATTACK, SET_DECAY_TIME: DECAY, SET_SLOPE_TIME: SLOPE, SET_RELEASE_TIME: RELEASE}[what], a)
        elif what <= SET_RELEASE_CURVE:
            self._list_param(self.curve, parts[what - SET_ATTACK_CURVE], a)
        elif what <= SET_RELEASE_FUNCTION:
            self._function(parts[what - SET_ATTACK_FUNCTION], int(a))
        elif what == SET_BREAK_LEVEL:
            self._attr_param("break_level", a)
        elif what == SET_SUSTAIN_LEVEL:
            self._attr_param("sustain_level", a)
        elif what == SET_HOLD_ENABLED:
            self._flag(USE_HOLD, a != 0)
        elif what == SET_BREAK_ENABLED:
            self._flag(USE_BREAK, a != 0)
        elif what == SET_HOLD:
            self._attr_param("hold_time", a)
            self._flag(USE_HOLD, b != 0)
        elif what == SET_BREAK:
            self._attr_param("break_level", a)
            self._flag(USE_BREAK, b != 0)
        elif what == UPDATE:
            self.update_settings()
        else:
            self._curve({SET_ATTACK: ATTACK, SET_DECAY: DECAY, SET_SLOPE: SLOPE, SET_RELEASE: RELEASE}[what], a, b, int(c))
        return self

    # -- configure_curve, :124-236
    def _configure(self, part, x0, x1, y0, y1):
        x0, x1, y0, y1 = f32(x0), f32(x1), f32(y0), f32(y1)
        g, fn, cu = self.params[part], self.fn[part], self.curve[part]
        with np.errstate(all="ignore"):
            if fn in (LINE, LINE2):
                g[0] = f32(0.5) * (x0 + x1) if fn == LINE else x1 + (x0 - x1) * cu
                cy = y0 + (y1 - y0) * cu
                g[1] = (cy - y0) / (g[0] - x0)
                g[2] = y0 - g[1] * x0
                g[3] = (y1 - cy) / (x1 - g[0])
                g[4] = cy - g[3] * g[0]
            elif fn == CUBIC:
                cx = f32(0.5) * (x0 + x1)
                cy = y0 + (y1 - y0) * cu
                k0 = (cy - y0) / (cx - x0)
                k1 = (y1 - cy) / (x1 - cx)
                g[0] = x0
                g[1:5] = hermite_cubic(f32(0), y0, k0, x1 - x0, y1, k1)
            elif fn == QUADRO:
                cx = f32(0.5) * (x0 + x1)
                cy = y0 + (y1 - y0) * (f32(0.3) + cu * f32(0.4))
                g[0] = x0
                g[1:6] = hermite_quadro(f32(0), y0, f32(0), x1 - x0, y1, f32(0), cx - x0, cy)
            elif fn == EXP:
                kt = f32(0.5) - cu
                ndx = f32(1) / (x1 - x0)
                g[0] = x0
                g[1] = np.abs(kt) * f32(40)
                ny = expf(-g[1])
                if kt >= 0:
                    g[2], g[3], g[4], g[5] = y0, (y1 - y0) * ny, ndx, f32(0)
                else:
                    g[2], g[3], g[4], g[5] = y1, (y0 - y1) * ny, -ndx, f32(1)
            else:
                g[0] = x0
                g[1] = (y1 - y0) / (x1 - x0)
                g[2] = y0

    def update_settings(self):                              # :238-293
        if not self.flags & RECONFIGURE:
            return self
        t = self.time
        t[ATTACK] = limit_range(t[ATTACK], f32(0))
        if self.flags & USE_HOLD:
            self.hold_time = limit_range(self.hold_time, t[ATTACK])
            t[DECAY] = limit_range(t[DECAY], self.hold_time)
        else:
            t[DECAY] = limit_range(t[DECAY], t[ATTACK])
        if self.flags & USE_BREAK:
            t[SLOPE] = limit_range(t[SLOPE], t[DECAY])
            t[RELEASE] = limit_range(t[RELEASE], t[SLOPE])
        else:
            t[RELEASE] = limit_range(t[RELEASE], t[DECAY])
        self._configure(ATTACK, 0, t[ATTACK], 0, 1)
        hold = self.hold_time if self.flags & USE_HOLD else t[ATTACK]
        if self.flags & USE_BREAK:
            self._configure(DECAY, hold, t[DECAY], 1, self.break_level)
            self._configure(SLOPE, t[DECAY], t[SLOPE], self.break_level, self.sustain_level)
        else:
            self._configure(DECAY, hold, t[DECAY], 1, self.sustain_level)
        self._configure(RELEASE, t[RELEASE], 1, self.sustain_level, 0)
        self.flags &= ~RECONFIGURE
        return self

    def used_params(self, part):
        """How many of a curve's six floats its function designs."""
        return {LINE: 5, LINE2: 5, CUBIC: 5, QUADRO: 6, EXP: 6}.get(self.fn[part], 3)

    def segments(self):
        """(x0, x1) of the four curves as update_settings() configures them; slope only with F_USE_BREAK."""
        t = self.time
        hold = self.hold_time if self.flags & USE_HOLD else t[ATTACK]
        return {ATTACK: (f32(0), t[ATTACK]), DECAY: (hold, t[DECAY]), SLOPE: (t[DECAY], t[SLOPE]) if self.flags & USE_BREAK else None,
                RELEASE: (t[RELEASE], f32(1))}

    # -- the generators, :350-383
    def _generator(self, part, t, shift):
        p, fn = self.params[part], self.fn[part]
        if fn in (LINE, LINE2):
            return np.where(t < p[0], t * p[1] + p[2], t * p[3] + p[4])
        u = t - p[0]
        if fn == CUBIC:
            return ((p[1] * u + p[2]) * u + p[3]) * u + p[4]
        if fn == QUADRO:
            return (((p[1] * u + p[2]) * u + p[3]) * u + p[4]) * u + p[5]
        if fn == EXP:
            u = u * p[4] + p[5]
            e = np.exp((u * p[1]).astype(np.float64)).astype(f32)
            if shift:
                e = np.nextafter(e, f32(np.inf if shift > 0 else -np.inf))
            return p[2] + p[3] * u * e
        return _fma(u, p[1], p[2]) if MUTATION == "fma" else u * p[1] + p[2]

    def stages(self, t, nan_stage):
        """The first loop condition of generate() that t meets, which is do_process's chain of compares."""
        t = np.asarray(t, f32)
        hold = self.hold_time if (self.flags & USE_HOLD and MUTATION != "no_hold") else self.time[ATTACK]
        before_attack = (t <= self.time[ATTACK]) if MUTATION == "le_segment_end" else (t < self.time[ATTACK])
        conds = [np.isnan(t), t <= 0, t >= 1, before_attack, t < hold, t < self.time[DECAY],
                 (t < self.time[SLOPE]) & bool(self.flags & USE_BREAK), t < self.time[RELEASE]]
        return np.select(conds, [nan_stage, ST_BEFORE, ST_AFTER, ST_ATTACK, ST_HOLD, ST_DECAY, ST_SLOPE, ST_SUSTAIN], ST_RELEASE)

    def values(self, stage, t, shift=0):
        """(the envelope at t for the given stages, which samples went through an EXP generator)"""
        t = np.asarray(t, f32)
        out, exp = np.zeros(t.shape, f32), np.zeros(t.shape, bool)
        out[stage == ST_HOLD] = 1
        out[stage == ST_SUSTAIN] = self.sustain_level
        for st, part in ((ST_ATTACK, ATTACK), (ST_DECAY, DECAY), (ST_SLOPE, SLOPE), (ST_RELEASE, RELEASE)):
            m = stage == st
            if m.any():
                out[m] = self._generator(part, t[m], shift)
                exp |= m & (self.fn[part] == EXP)
        return out, exp

    def times(self, first, n, start, step):
        """t_i of generate(), i = first .. first + n - 1: t_0 is start itself"""
        start, step = f32(start), f32(step)
        i = np.arange(first, first + n, dtype=np.uint64)
        t = start + i.astype(f32) * step
        if MUTATION != "zero_step_t0":
            t[i == 0] = start
        return t

    def run(self, kind, n=None, src=None, dst=None, start=0, step=0, first=0, shift=0):
        """One of the five operations; (result, EXP mask, stages).  For generate* the samples first .. first + n - 1 of a longer call."""
        with np.errstate(all="ignore"):
            self.update_settings()
            if kind in (PROCESS, PROCESS_MUL):
                t = np.asarray(src, f32)
                stage = self.stages(t, ST_RELEASE)
                g, exp = self.values(stage, t, shift)
                return (g if kind == PROCESS else np.asarray(dst, f32) * g), exp, stage
            t = self.times(first, n, start, step)
            stage = self.stages(t, ST_AFTER)
            if f32(step) < 0 and MUTATION != "no_floor":
                stage = np.maximum(stage, self.stages(f32(start), ST_AFTER))
            g, exp = self.values(stage, t, shift)
            if kind == GENERATE:
                return g, exp, stage
            x = np.asarray(dst if kind == GENERATE_MUL else src, f32)
            outside = (stage == ST_BEFORE) | (stage == ST_AFTER)
            if MUTATION == "stage0_multiply":
                outside = stage == ST_AFTER
            return np.where(outside, f32(0), np.where(stage == ST_HOLD, x, x * g)), exp, stage

    def record(self):
        """The designed record as the recording has it: per curve fTime, fCurve, enFunction and six floats (bits); fHoldTime,
        fBreakLevel, fSustainLevel (bits), nFlags."""
        out = []
        for k in range(4):
            out += [int(f32(self.time[k]).view(np.uint32)), int(f32(self.curve[k]).view(np.uint32)), int(self.fn[k])]
            out += [int(v) for v in self.params[k].view(np.uint32)]
        out += [int(f32(v).view(np.uint32)) for v in (self.hold_time, self.break_level, self.sustain_level)] + [int(self.flags)]
        return np.array(out, np.int64)


def design(ops):
    e = Envelope()
    for op in ops:
        e.apply(op)
    return e
