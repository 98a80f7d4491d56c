"""lsp::dspu::Depopper (src/main/util/Depopper.cpp) restated in numpy float32, one operation per rounding, one object per
channel, with the reference's shifted linear buffers and its own nRmsOff / nLookOff.

The designer (init :108-151, calc_fade :153-252, reconfigure :254-270, the setters :272-379) is restated line for line; sinf and
expf are the host's C library's, as in the reference.  A test of the device hands the BANK's designed values and tables in
instead (feed): then nothing here depends on a libm.  dsp::h_sum is the serial float32 sum, oldest first (numpy's accumulate; its
sum() is pairwise)."""
import ctypes
import ctypes.util

import numpy as np

f32 = np.float32
LINEAR, CUBIC, SINE, GAUSSIAN, PARABOLIC = range(5)
CLOSED, FADE, OPENED, WAIT = range(4)
DEFAULT_ALIGN = 0x40            # lsp-common-lib's, unpinned: the value of oracle/ref_shim
BUF_SIZE = 0x1000
GAIN_AMP_M_80_DB = f32(0.0001)

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
for _n in ("expf", "sinf"):
    getattr(_libm, _n).restype = ctypes.c_float
    getattr(_libm, _n).argtypes = [ctypes.c_float]


def expf(v):
    return f32(_libm.expf(ctypes.c_float(float(v))))


def sinf(v):
    return f32(_libm.sinf(ctypes.c_float(float(v))))


def once(fn):
    """The float64 function rounded once to float32."""
    return lambda v: f32(fn(np.float64(v)))


def millis_to_samples(sr, ms):
    return (f32(ms) * f32(0.001)) * f32(sr)


def align_size(v, a):
    return v if v % a == 0 else v + a - v % a


def h_sum(a):
    return f32(np.add.accumulate(a, dtype=f32)[-1]) if len(a) else f32(0.0)


def lsp_max(a, b):
    return a if a > b else b


def lsp_limit(x, lo, hi):
    return lo if x < lo else (hi if x > hi else x)


class Fade:
    def __init__(self):
        self.enMode, self.fThresh, self.fTime, self.fDelay = LINEAR, GAIN_AMP_M_80_DB, f32(0.0), f32(0.0)
        self.nSamples, self.nDelay = 0, 0
        self.fPoly = np.zeros(4, f32)
        self.table = None                   # crossfade(x) for x = 0 .. nSamples - 1 where somebody else has tabulated it

    def words(self):
        return [self.nSamples, self.nDelay] + [int(v) for v in self.fPoly.view(np.uint32)]


def crossfade(fade, x, sin=sinf, exp=expf):
    """:381-420, x an integer as the callers pass it"""
    xf = f32(x)
    if xf < f32(0.0):
        return f32(0.0)
    if xf >= f32(fade.nSamples):
        return f32(1.0)
    if fade.table is not None:
        return f32(fade.table[x])
    p = fade.fPoly
    with np.errstate(all="ignore"):
        if fade.enMode in (LINEAR, CUBIC, PARABOLIC):
            return f32(p[0] + xf * f32(p[1] + xf * f32(p[2] + f32(xf * p[3]))))
        if fade.enMode == SINE:
            v = sin(f32(f32(p[0] * xf) + p[1]))
            return f32(v * v)
        if fade.enMode == GAUSSIAN:
            v = f32(f32(p[0] * xf) + p[1])
            return f32(f32(p[2] * exp(f32(-v * v))) + p[3])
    return f32(0.0)


def fade_table(fade, sin=sinf, exp=expf):
    return np.array([crossfade(fade, x, sin, exp) for x in range(max(fade.nSamples, 0))], f32)


class Depopper:
    def __init__(self):
        self.nSampleRate = -1
        self.nState = CLOSED
        self.fLookMax, self.nLookMin, self.nLookMax, self.nLookOff, self.nLookCount = f32(0.0), 0, 0, 0, 0
        self.fRmsMax, self.fRmsLength, self.nRmsMin, self.nRmsMax, self.nRmsOff, self.nRmsLen = f32(0.0), f32(0.0), 0, 0, 0, 0
        self.fRmsNorm = f32(0.0)
        self.nCounter, self.nDelay, self.fRms = 0, 0, f32(0.0)
        self.sFadeIn, self.sFadeOut = Fade(), Fade()
        self.sFadeIn.fTime = f32(50.0)
        self.gbuf = self.rbuf = None
        self.bReconfigure = True
        self.feed = None            # callable -> (params, fade-in table, fade-out table) of a bank's getters

    def init(self, srate, max_fade, max_rms):
        max_fade, max_rms = f32(max_fade), f32(max_rms)
        if self.nSampleRate == srate and self.fLookMax == max_fade and self.fRmsMax == max_rms:
            return
        self.nSampleRate, self.fLookMax, self.fRmsMax = srate, max_fade, max_rms
        lk_buf = align_size(int(millis_to_samples(srate, max_fade)), DEFAULT_ALIGN)
        rms_buf = align_size(int(millis_to_samples(srate, max_rms)), DEFAULT_ALIGN)
        self.nLookMin = lk_buf + rms_buf
        self.nLookMax = self.nLookMin + max(lk_buf * 4, BUF_SIZE)
        self.nLookOff = self.nLookMin
        self.nRmsMin = rms_buf
        self.nRmsMax = self.nRmsMin + max(rms_buf * 4, BUF_SIZE)
        self.nRmsOff = self.nRmsMin
        self.gbuf, self.rbuf = np.zeros(self.nLookMax, f32), np.zeros(self.nRmsMax, f32)
        self.nState = CLOSED
        self.bReconfigure = True

    def calc_fade(self, fade, is_in):
        with np.errstate(all="ignore"):
            time = millis_to_samples(self.nSampleRate, fade.fTime)
            fade.nDelay = int(millis_to_samples(self.nSampleRate, fade.fDelay))
            fade.nSamples = int(time)
            k = f32(1.0) / time
            p = np.zeros(4, f32)
            if fade.enMode == LINEAR:
                p[0], p[1] = (0.0, k) if is_in else (1.0, -k)
            elif fade.enMode == CUBIC:
                if is_in:
                    p[2], p[3] = f32(f32(3.0) * k) * k, f32(f32(f32(-2.0) * k) * k) * k
                else:
                    p[0], p[2], p[3] = 1.0, f32(f32(-3.0) * k) * k, f32(f32(f32(2.0) * k) * k) * k
            elif fade.enMode == SINE:
                p[0] = f32(np.float64(np.pi) * np.float64(f32(0.5)) * np.float64(k))
                p[1] = f32(0.0) if is_in else f32(np.pi / 2)
            elif fade.enMode == PARABOLIC:
                if is_in:
                    p[2] = k * k
                else:
                    p[0], p[1], p[2] = 1.0, f32(-2.0) * k, k * k
            elif fade.enMode == GAUSSIAN:
                f0 = expf(-16.0)
                p[0], p[1], p[2], p[3] = f32(4.0) * k, (-4.0 if is_in else 0.0), f32(1.0) / f32(f32(1.0) - f0), -f0
            fade.fPoly = p

    def reconfigure(self):
        if not self.bReconfigure:
            return
        if self.feed is not None:
            p, tin, tout = self.feed()
            for fade, q, t in ((self.sFadeIn, p["fade_in"], tin), (self.sFadeOut, p["fade_out"], tout)):
                fade.nSamples, fade.nDelay, fade.fPoly, fade.table = q["samples"], q["delay_samples"], q["poly"], t
            self.nRmsLen, self.nLookCount, self.fRmsNorm = p["rms_len"], p["look_count"], f32(p["rms_norm"])
        else:
            self.calc_fade(self.sFadeIn, True)
            self.calc_fade(self.sFadeOut, False)
            self.nRmsLen = int(millis_to_samples(self.nSampleRate, self.fRmsLength))
            self.nLookCount = self.sFadeOut.nSamples + self.nRmsLen
            with np.errstate(all="ignore"):
                self.fRmsNorm = f32(1.0) / f32(self.nRmsLen)
        self.fRms = h_sum(self.rbuf[self.nRmsOff - self.nRmsLen:self.nRmsOff])
        self.bReconfigure = False

    def accepted(self):
        """The settings stay inside the reference's defined behaviour (what the bank accepts); call after reconfigure()."""
        return (self.rbuf is not None and self.nRmsLen > 0 and f32(0.0) <= self.sFadeOut.fTime <= self.fLookMax)

    def _set(self, obj, name, old, new):
        if old == new:
            return old
        setattr(obj, name, new)
        self.bReconfigure = True
        return old

    def set_fade_in_mode(self, mode):
        return self._set(self.sFadeIn, "enMode", self.sFadeIn.enMode, mode)

    def set_fade_out_mode(self, mode):
        return self._set(self.sFadeOut, "enMode", self.sFadeOut.enMode, mode)

    def set_fade_in_time(self, v):
        return self._set(self.sFadeIn, "fTime", lsp_max(f32(0.0), self.sFadeIn.fTime), f32(v))

    def set_fade_out_time(self, v):
        return self._set(self.sFadeOut, "fTime", lsp_limit(self.sFadeOut.fTime, f32(0.0), self.fLookMax), f32(v))

    def set_fade_in_threshold(self, v):
        return self._set(self.sFadeIn, "fThresh", lsp_max(f32(0.0), self.sFadeIn.fThresh), f32(v))

    def set_fade_out_threshold(self, v):
        return self._set(self.sFadeOut, "fThresh", lsp_max(f32(0.0), self.sFadeOut.fThresh), f32(v))

    def set_fade_in_delay(self, v):
        return self._set(self.sFadeIn, "fDelay", lsp_max(f32(0.0), self.sFadeIn.fDelay), f32(v))

    def set_fade_out_delay(self, v):
        return self._set(self.sFadeOut, "fDelay", lsp_max(f32(0.0), self.sFadeOut.fThresh), f32(v))        # fThresh: :358

    def set_rms_length(self, v):
        return self._set(self, "fRmsLength", self.fRmsLength, lsp_limit(f32(v), f32(0.0), self.fRmsMax))

    def latency(self):
        return self.sFadeOut.nSamples

    def apply_fadeout(self, at, samples):
        """:422-441, dst = &gbuf[at]"""
        out = self.sFadeOut
        if out.nSamples <= 0:
            return
        samples = min(samples, out.nSamples)
        g = self.gbuf
        g[at] = 0.0
        d = at - (samples + self.nRmsLen)
        with np.errstate(all="ignore"):
            for x in range(out.nSamples - samples, out.nSamples):
                g[d] = g[d] * crossfade(out, x)
                d += 1
        g[d:d + self.nRmsLen] = 0.0

    def calc_rms(self, s):
        """:443-462"""
        if self.nRmsOff >= self.nRmsMax:
            self.rbuf[:self.nRmsMin] = self.rbuf[self.nRmsOff - self.nRmsMin:self.nRmsOff].copy()
            self.nRmsOff = self.nRmsMin
            self.fRms = h_sum(self.rbuf[self.nRmsOff - self.nRmsLen:self.nRmsOff])
        elif (self.nRmsOff & 0x1f) == 0:
            self.fRms = h_sum(self.rbuf[self.nRmsOff - self.nRmsLen:self.nRmsOff])
        s = f32(s * s)
        g = self.rbuf[self.nRmsOff - self.nRmsLen]
        self.fRms = f32(abs(f32(f32(self.fRms + s) - g)))
        self.rbuf[self.nRmsOff] = s
        self.nRmsOff += 1
        return f32(np.sqrt(f32(self.fRms * self.fRmsNorm)))

    def process(self, src):
        """src [n] -> (env [n], gain [n]), :464-562"""
        self.reconfigure()
        src = np.asarray(src, f32)
        n = src.size
        env, gain = np.empty(n, f32), np.empty(n, f32)
        fin, fout, g = self.sFadeIn, self.sFadeOut, self.gbuf
        done = 0
        with np.errstate(all="ignore"):
            while done < n:
                if self.nLookMax - self.nLookOff <= 0:
                    g[:self.nLookMin] = g[self.nLookOff - self.nLookMin:self.nLookOff].copy()
                    self.nLookOff = self.nLookMin
                base = self.nLookOff
                to_do = min(n - done, self.nLookMax - self.nLookOff)
                for i in range(to_do):
                    s = self.calc_rms(src[done + i])
                    env[done + i] = s
                    at = base + i
                    if self.nState == CLOSED:
                        g[at] = 0.0
                        if not (s < fin.fThresh):
                            self.nCounter, self.nDelay, self.nState = 0, fin.nDelay, FADE
                            g[at] = crossfade(fin, self.nCounter)
                            self.nCounter += 1
                    elif self.nState == FADE:
                        g[at] = crossfade(fin, self.nCounter)
                        self.nCounter += 1
                        if s < fout.fThresh:
                            self.nDelay -= 1
                            if self.nDelay <= 0:
                                self.apply_fadeout(at, self.nCounter)
                                self.nCounter, self.nState = 0, WAIT
                        else:
                            self.nDelay = fin.nDelay
                            if self.nCounter >= fin.nSamples:
                                self.nState = OPENED
                    elif self.nState == OPENED:
                        g[at] = 1.0
                        if self.nCounter < fout.nSamples:
                            self.nCounter += 1
                        if s < fout.fThresh:
                            self.apply_fadeout(at, self.nCounter)
                            self.nState, self.nDelay = WAIT, fout.nDelay
                    else:
                        g[at] = 0.0
                        self.nDelay -= 1
                        if self.nDelay <= 0:
                            self.nState = CLOSED
                gain[done:done + to_do] = g[base - self.nLookCount:base - self.nLookCount + to_do]
                self.nLookOff += to_do
                done += to_do
        return env, gain

    def state_words(self):
        """fRms's bits, nState, nCounter, nDelay, nRmsOff, nLookOff"""
        return np.array([int(f32(self.fRms).view(np.uint32)), self.nState, self.nCounter, self.nDelay, self.nRmsOff, self.nLookOff], np.int64)

    def design_words(self):
        """both fades' nSamples, nDelay and fPoly's bits, then nRmsLen, nLookCount, fRmsNorm's bits, nLookMin, nLookMax, nRmsMin, nRmsMax"""
        return np.array(self.sFadeIn.words() + self.sFadeOut.words() +
                        [self.nRmsLen, self.nLookCount, int(f32(self.fRmsNorm).view(np.uint32)), self.nLookMin, self.nLookMax,
                         self.nRmsMin, self.nRmsMax], np.int64)

    def buffers(self):
        """the logical contents: the last nRmsMin squares and the last nLookMin gains"""
        return self.rbuf[self.nRmsOff - self.nRmsMin:self.nRmsOff].copy(), self.gbuf[self.nLookOff - self.nLookMin:self.nLookOff].copy()
