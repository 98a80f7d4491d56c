"""lsp::dspu::PeakMeter and lsp::dspu::SurgeProtector restated in numpy float32, one operation per rounding, vectorised over
channels with a Python loop over samples (1024 x 4096 in about a second).

PeakMeter (src/main/meters/PeakMeter.cpp): process() :127-183, process(value, count) :185-205, clear() :110-114 and what
update_settings() does to the state (:124).  fTau and nHold are INPUTS (a bank's getter, a recorded case, or design() below, which
forms them with this machine's libm as the reference does).  SurgeProtector (src/main/dynamics/SurgeProtector.cpp): process(float)
:99-149 with its branches as they stand, the setters' clamps :71-81 and reset() :65-69."""
import ctypes
import ctypes.util

import numpy as np

f32 = np.float32
u32 = np.uint32

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
for _n in ("expf", "logf"):
    getattr(_libm, _n).restype = ctypes.c_float
    getattr(_libm, _n).argtypes = [ctypes.c_float]


def expf(v):
    return f32(_libm.expf(ctypes.c_float(float(v))))


def logf(v):
    return f32(_libm.logf(ctypes.c_float(float(v))))


def millis_to_samples(sr, ms):
    return (f32(ms) * f32(0.001)) * f32(sr)


def design(sample_rate, hold_ms, release_ms):
    """update_settings(), :122-123: (fTau, nHold), every expression float32, expf and logf the C library's."""
    with np.errstate(divide="ignore", invalid="ignore"):
        hold = int(millis_to_samples(sample_rate, hold_ms))
        tau = expf(logf(f32(1.0) - f32(np.sqrt(0.5))) / millis_to_samples(sample_rate, release_ms))
    return tau, hold


def value_factor(tau, count):
    """expf(logf(fTau) * float(count)), :202"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return expf(logf(tau) * f32(count))


class PeakMeters:
    def __init__(self, tau, hold):
        self.tau = np.asarray(tau, f32).copy()
        self.hold = np.asarray(hold, np.int64).copy()
        C = self.tau.size
        self.peak, self.counter = np.zeros(C, f32), np.zeros(C, np.int64)

    def clear(self, ch=None):
        sel = slice(None) if ch is None else ch
        self.peak[sel], self.counter[sel] = 0.0, 0

    def process(self, x):
        """x [C, n] -> the peak after every sample [C, n]"""
        x = np.abs(np.asarray(x, f32))
        out = np.empty_like(x)
        self.counter = np.minimum(self.counter, self.hold)             # update_settings()
        peak, counter, tau, hold = self.peak, self.counter, self.tau, self.hold
        with np.errstate(invalid="ignore", under="ignore"):
            for i in range(x.shape[1]):
                s = x[:, i]
                ge = s >= peak
                run = ~ge & (counter > 0)
                decay = ~ge & ~run
                counter = np.where(ge, hold, counter - run)
                peak = np.where(ge, s, np.where(decay, peak * tau, peak))
                out[:, i] = peak
        self.peak, self.counter = peak.astype(f32), counter
        return out

    def process_value(self, value, count, factor=None):
        """process(value, count) of every channel -> the peaks [C]"""
        value = np.abs(np.asarray(value, f32))
        if factor is None:
            factor = np.array([value_factor(t, count) for t in self.tau], f32)
        self.counter = np.minimum(self.counter, self.hold)
        with np.errstate(invalid="ignore", under="ignore"):
            ge = value >= self.peak
            run = ~ge & (self.counter >= count)
            decayed = self.peak * np.asarray(factor, f32)
            lsp_max = np.where(decayed > value, decayed, value)         # a NaN product gives `value`
            self.peak = np.where(ge, value, np.where(run, self.peak, lsp_max)).astype(f32)
            self.counter = np.where(ge, self.hold, np.where(run, self.counter - count, self.counter))
        return self.peak.copy()


class SurgeProtectors:
    def __init__(self, channels):
        C = channels
        self.tmax, self.sdmax = np.zeros(C, np.int64), np.zeros(C, np.int64)
        self.on_thr, self.off_thr = np.zeros(C, f32), np.zeros(C, f32)
        self.gain = np.zeros(C, f32)
        self.t, self.sd, self.on = np.zeros(C, np.int64), np.zeros(C, np.int64), np.zeros(C, bool)

    def set_transition_time(self, ch, samples):
        self.tmax[ch] = samples
        self.t[ch] = min(self.t[ch], samples)

    def set_shutdown_time(self, ch, samples):
        self.sdmax[ch] = samples
        self.sd[ch] = min(self.sd[ch], samples)

    def reset(self, ch=None):
        sel = slice(None) if ch is None else ch
        self.on[sel], self.t[sel] = False, 0

    def process(self, level):
        """level [C, n] -> the gain after every sample [C, n]"""
        level = np.asarray(level, f32)
        out = np.empty_like(level)
        t, sd, on, gain = self.t, self.sd, self.on, self.gain
        tmax, sdmax = self.tmax, self.sdmax
        ftmax = tmax.astype(f32)
        with np.errstate(invalid="ignore", divide="ignore"):
            for i in range(level.shape[1]):
                v = level[:, i]
                sd_on = np.where(v >= self.off_thr, 0, sd + 1)
                turn_on = ~on & (v >= self.on_thr)
                sd = np.where(on, sd_on, np.where(turn_on, 0, sd))
                on = np.where(on, sd_on < sdmax, turn_on)
                ramp = np.sqrt(t.astype(f32) / ftmax)
                moving = np.where(on, t < tmax, t > 0)
                gain = np.where(moving, ramp, np.where(on, f32(1.0), f32(0.0))).astype(f32)
                t = t + np.where(moving, np.where(on, 1, -1), 0)
                out[:, i] = gain
        self.t, self.sd, self.on, self.gain = t, sd, on, gain
        return out
