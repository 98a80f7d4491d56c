"""lsp::dspu::Sidechain restated in numpy float32, one operation per rounding: the block overload of process() (source selection,
magnitude, gain, ring, the refresh every 0x2000 samples with its two partial sums, the four detectors) for C channels at once,
vectorised over channels and serial over samples.  The project's own statement of what the device has to compute; the ring,
its capacity and position and the refresh counter are the reference's.  The refresh sums are taken serially, oldest sample
first, each term rounded, then each sum (the order plain C gives)."""
import numpy as np

f32 = np.float32
U = 2.0 ** -24                                  # half a unit in the last place of a float32 in [1, 2)
REFRESH_RATE = 0x2000
RING_EXTRA = 0x200
SCS_MIDDLE, SCS_SIDE, SCS_LEFT, SCS_RIGHT, SCS_AMIN, SCS_AMAX = range(6)
SCM_PEAK, SCM_RMS, SCM_LPF, SCM_UNIFORM = range(4)
SCSM_STEREO, SCSM_MIDSIDE = range(2)
SCF_MIDSIDE = 1
MODES = (SCM_PEAK, SCM_RMS, SCM_LPF, SCM_UNIFORM)
SOURCES = (SCS_MIDDLE, SCS_SIDE, SCS_LEFT, SCS_RIGHT, SCS_AMIN, SCS_AMAX)


def millis_to_samples(sr, ms):
    return (f32(ms) * f32(0.001)) * f32(sr)


def capacity(sr, max_reactivity):
    """The ring of set_sample_rate(): max(millis_to_samples, 1) + 0x200 in float32, truncated."""
    return int(max(millis_to_samples(sr, max_reactivity), f32(1.0)) + f32(RING_EXTRA))


def reactivity_samples(sr, reactivity):
    return max(int(millis_to_samples(sr, reactivity)), 1)


def tau64(n):
    """(tau in float64, bound of the float32 computation's error): tau = 1 - exp(ln(c) / n), c the float32 nearest 1 - sqrt(1/2).
    logf and expf are taken to be within one unit in the last place (2 U relative); the quotient and the difference round once
    (U each).  An error d of exp's argument is a relative error d of its value.  First order, 1 % on top for the rest."""
    k = np.log(np.float64(f32(1.0 - np.sqrt(0.5))))
    e = np.exp(k / n)
    tau = 1.0 - e
    arg_err = 3 * U * abs(k) / n                    # logf (2 U) and the division (U)
    return tau, 1.01 * (e * (2 * U + arg_err) + U * abs(tau))


def pick_source(a, b, source, midside, two):
    """preprocess() before the magnitude: the signed source (psmin3 / psmax3 for AMIN / AMAX).  a, b: float32 rows."""
    if not two:
        return a.copy()
    half = f32(0.5)
    if midside:
        l, r = a + b, a - b
        return {SCS_MIDDLE: a, SCS_SIDE: b, SCS_LEFT: l, SCS_RIGHT: r,
                SCS_AMIN: np.where(np.abs(l) < np.abs(r), l, r), SCS_AMAX: np.where(np.abs(r) < np.abs(l), l, r)}[source].astype(f32)
    return {SCS_MIDDLE: (a + b) * half, SCS_SIDE: (a - b) * half, SCS_LEFT: a, SCS_RIGHT: b,
            SCS_AMIN: np.where(np.abs(a) < np.abs(b), a, b), SCS_AMAX: np.where(np.abs(b) < np.abs(a), a, b)}[source].astype(f32)


def serial_sum(terms):
    """Float32 terms added one after the other from 0."""
    return f32(np.add.accumulate(terms, dtype=f32)[-1]) if len(terms) else f32(0.0)


class Sidechains:
    """C sidechains.  params: per channel a dict with reactivity, tau, interval, capacity, mode, source, flags, gain (what
    SidechainBank.get_params returns); inputs: 1 or 2."""

    def __init__(self, params, inputs=1):
        self.C, self.inputs = len(params), inputs
        self.set_params(params)
        self.ring = np.zeros((self.C, int(self.cap.max())), f32)
        self.head = np.zeros(self.C, np.int64)
        self.rms = np.zeros(self.C, f32)
        self.refresh = np.zeros(self.C, np.int64)
        self.fresh = np.ones(self.C, bool)      # nothing was pushed into the ring yet: the only time its position is 0
        self.refreshes = []                     # (channel, samples seen by it in this object, wrapped) of every window refresh

    def set_params(self, params):
        self.N = np.array([p["reactivity"] for p in params], np.int64)
        self.tau = np.array([p["tau"] for p in params], f32)
        self.interval = np.array([p["interval"] for p in params], f32)
        self.cap = np.array([p["capacity"] for p in params], np.int64)
        self.mode = np.array([p["mode"] for p in params], np.int64)
        self.source = [int(p["source"]) for p in params]
        self.midside = [bool(p["flags"] & SCF_MIDSIDE) for p in params]
        self.gain = np.array([p["gain"] for p in params], f32)

    # the setters' effects on the state (the parameters come from the library: set_params)
    def set_mode(self, ch, mode):
        if self.mode[ch] != mode:
            self.rms[ch] = 0.0
            self.mode[ch] = mode

    def updated(self, ch):
        self.refresh[ch] = REFRESH_RATE         # update_settings() with SCF_UPDATE: force a refresh

    def clear(self, ch):
        self.rms[ch] = 0.0
        self.refresh[ch] = 0
        self.ring[ch] = 0.0                     # the position stays

    def premix(self, in0, in1):
        n = (in0 if in0 is not None else in1).shape[1]
        out = np.zeros((self.C, n), f32)
        if in0 is None:
            return out
        for ch in range(self.C):
            out[ch] = pick_source(in0[ch], None if in1 is None else in1[ch], self.source[ch], self.midside[ch], self.inputs == 2)
        return out

    def _refresh(self, ch):
        mode, N, cap, head = self.mode[ch], int(self.N[ch]), int(self.cap[ch]), int(self.head[ch])
        if mode == SCM_PEAK:
            self.rms[ch] = 0.0
        elif mode in (SCM_RMS, SCM_UNIFORM):
            term = (lambda v: v * v) if mode == SCM_RMS else np.abs
            tail = (head + cap - N) % cap
            row = self.ring[ch]
            if tail < head:
                self.rms[ch] = serial_sum(term(row[tail:tail + N]))
            else:
                self.rms[ch] = serial_sum(term(row[tail:cap])) + serial_sum(term(row[:head]))
            self.refreshes.append((ch, tail >= head))

    def process(self, in0, in1=None, count=None, premixed=False):
        """-> (out, trace): the output rows and fRmsValue after every sample.  in0 None: silence."""
        C = self.C
        if in0 is None:
            sig = np.zeros((C, count), f32)
        elif premixed:
            sig = np.asarray(in0, f32)
        else:
            sig = self.premix(in0, in1)
        x = (np.abs(sig) * self.gain[:, None]).astype(f32)
        n = x.shape[1]
        if n > 0:
            self.fresh[:] = False
        out, trace = np.empty((C, n), f32), np.empty((C, n), f32)
        rows = np.arange(C)
        is_rms, is_uni, is_lpf, is_peak = (self.mode == m for m in (SCM_RMS, SCM_UNIFORM, SCM_LPF, SCM_PEAK))
        zero = f32(0.0)
        with np.errstate(invalid="ignore", under="ignore"):
            for t in range(n):
                due = self.refresh >= REFRESH_RATE
                if due.any():
                    for ch in np.flatnonzero(due):
                        self._refresh(ch)
                    self.refresh[due] %= REFRESH_RATE
                s = x[:, t]
                self.ring[rows, self.head] = s
                self.head = (self.head + 1) % self.cap
                last = self.ring[rows, (self.head + self.cap - (self.N + 1)) % self.cap]
                rms = self.rms
                d_rms = s * s - last * last
                d_uni = s - last
                d_lpf = self.tau * (s - rms)
                rms = np.where(is_peak, rms, rms + np.where(is_rms, d_rms, np.where(is_uni, d_uni, d_lpf))).astype(f32)
                self.rms = rms
                trace[:, t] = rms
                q = rms * self.interval
                o_rms = np.where(q > zero, np.sqrt(np.maximum(q, zero)), zero)
                o_uni = np.where(rms < zero, zero, q)
                o_lpf = np.where(rms > zero, rms, zero)
                out[:, t] = np.where(is_peak, s, np.where(is_rms, o_rms, np.where(is_uni, o_uni, o_lpf)))
                self.refresh += 1
        return out, trace

    def state(self):
        """head is RawRingBuffer::position(): push() of a block that ends at the ring's end leaves it AT the capacity
        (RawRingBuffer.cpp:118-122: it wraps only where nHead + count > nCapacity), and the next push starts over from there."""
        head = np.where((self.head == 0) & ~self.fresh, self.cap, self.head)
        return {"rms": self.rms.copy(), "refresh": self.refresh.astype(np.uint32), "head": head.astype(np.uint32)}
