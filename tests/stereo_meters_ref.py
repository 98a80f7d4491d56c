"""lsp::dspu::Correlometer and lsp::dspu::Panometer restated in numpy float32, one operation per rounding: process() for C
channels at once, vectorised over channels and serial over samples -- the two rings, the refresh every `period` samples with its
two partial sums where the window wraps, the per-sample step and the formula on top.  The project's own statement of what the
device has to compute.  dsp::corr_init, dsp::corr_incr, dsp::h_sum and dsp::sqr2 are taken as plain serial C: every product and
every sum rounds once, no fused multiply-add, sums serially from 0, oldest sample first."""
import numpy as np

f32 = np.float32
U = 2.0 ** -24                                  # half a unit in the last place of a float32 in [1, 2)
RING_EXTRA = 0x400                              # BUFFER_SIZE
RING_ALIGN = 0x40                               # DEFAULT_ALIGN
CORR_THRESHOLD = f32(1e-10)                     # dsp::corr_incr: below it the correlation is 0 (upstream)
PAN_LAW_LINEAR, PAN_LAW_EQUAL_POWER = range(2)
LINEAR_THRESHOLD, POWER_THRESHOLD = f32(1e-18), f32(1e-36)


def capacity(max_period):
    """init(): align_size(max_period + BUFFER_SIZE, DEFAULT_ALIGN)."""
    return (max_period + RING_EXTRA + RING_ALIGN - 1) // RING_ALIGN * RING_ALIGN


def serial_sum(terms):
    """Float32 terms added one after the other from 0."""
    return f32(np.add.accumulate(terms, dtype=f32)[-1]) if len(terms) else f32(0.0)


class _Meters:
    """What the two share: rings, nHead, nWindow, the window of a refresh.  params: per channel a dict with period and capacity
    (what <Bank>.get_params returns)."""

    def __init__(self, params):
        self.C = len(params)
        self.cap = np.array([p["capacity"] for p in params], np.int64)
        self.period = np.zeros(self.C, np.int64)
        self.ring_a = np.zeros((self.C, int(self.cap.max())), f32)
        self.ring_b = np.zeros((self.C, int(self.cap.max())), f32)
        self.head = np.zeros(self.C, np.int64)
        self.window = np.zeros(self.C, np.int64)
        self.refreshes = []                     # (channel, wrapped) of every refresh
        self.rows = np.arange(self.C)

    def _pieces(self, ch):
        """The window [tail, head) of channel ch as slices of its rings, oldest first."""
        head, cap, P = int(self.head[ch]), int(self.cap[ch]), int(self.period[ch])
        tail = (head + cap - P) % cap
        wrapped = head < tail
        self.refreshes.append((ch, wrapped))
        return [slice(tail, cap), slice(0, head)] if wrapped else [slice(tail, tail + P)]

    def _clear_rings(self, ch):
        self.ring_a[ch] = 0.0
        self.ring_b[ch] = 0.0
        self.head[ch] = self.period[ch]


class Correlometers(_Meters):
    def __init__(self, params):
        super().__init__(params)
        self.v, self.a, self.b = (np.zeros(self.C, f32) for _ in range(3))
        self.update = np.zeros(self.C, bool)
        for ch, p in enumerate(params):
            self.set_period(ch, p["period"])

    def set_period(self, ch, period, max_period=None):
        period = period if max_period is None else min(period, max_period)
        if period == self.period[ch]:
            return
        self.period[ch] = period
        self.update[ch] = True

    def clear(self, ch):
        self._clear_rings(ch)
        self.v[ch] = self.a[ch] = self.b[ch] = 0.0

    def _refresh(self, ch):
        v = a = b = f32(0.0)
        for s in self._pieces(ch):
            x, y = self.ring_a[ch, s], self.ring_b[ch, s]
            v, a, b = v + serial_sum(x * y), a + serial_sum(x * x), b + serial_sum(y * y)
        self.v[ch], self.a[ch], self.b[ch] = v, a, b

    def process(self, in_a, in_b):
        """-> (out, trace): the output rows and (v, a, b) after every sample, [3, C, n]."""
        in_a, in_b = np.asarray(in_a, f32), np.asarray(in_b, f32)
        C, n = in_a.shape
        self.window[self.update] = self.period[self.update]
        self.update[:] = False
        out, trace = np.empty((C, n), f32), np.empty((3, C, n), f32)
        rows, zero = self.rows, f32(0.0)
        with np.errstate(all="ignore"):
            for t in range(n):
                due = self.window >= self.period
                if due.any():
                    for ch in np.flatnonzero(due):
                        self._refresh(ch)
                    self.window[due] = 0
                tail = (self.head + self.cap - self.period) % self.cap
                at, bt = self.ring_a[rows, tail], self.ring_b[rows, tail]
                ah, bh = in_a[:, t], in_b[:, t]
                self.ring_a[rows, self.head], self.ring_b[rows, self.head] = ah, bh
                self.v = self.v + (ah * bh - at * bt)
                self.a = self.a + (ah * ah - at * at)
                self.b = self.b + (bh * bh - bt * bt)
                d = self.a * self.b
                ok = d >= CORR_THRESHOLD
                out[:, t] = np.where(ok, self.v / np.sqrt(np.where(ok, d, f32(1.0))), zero)
                trace[0, :, t], trace[1, :, t], trace[2, :, t] = self.v, self.a, self.b
                self.head = (self.head + 1) % self.cap
                self.window += 1
        return out, trace

    def state(self):
        return {"v": self.v.copy(), "a": self.a.copy(), "b": self.b.copy(), "head": self.head.astype(np.uint32),
                "window": self.window.astype(np.uint32)}


class Panometers(_Meters):
    """params: also law, norm and default_pan."""

    def __init__(self, params):
        super().__init__(params)
        self.va, self.vb = np.zeros(self.C, f32), np.zeros(self.C, f32)
        self.norm = np.zeros(self.C, f32)
        for ch, p in enumerate(params):
            self.set_period(ch, p["period"])
        self.set_params(params)

    def set_params(self, params):
        self.law = np.array([p["law"] for p in params], np.int64)
        self.dflt = np.array([p["default_pan"] for p in params], f32)
        assert np.array_equal(self.norm.view(np.uint32), np.array([p["norm"] for p in params], f32).view(np.uint32))

    def set_period(self, ch, period, max_period=None):
        period = period if max_period is None else min(period, max_period)
        if period == self.period[ch]:
            return
        self.period[ch] = self.window[ch] = period
        self.va[ch] = self.vb[ch] = 0.0
        self.norm[ch] = f32(1.0) / f32(period) if period > 0 else f32(1.0)

    def clear(self, ch):
        self._clear_rings(ch)                   # the sums stay

    def _refresh(self, ch):
        pieces = self._pieces(ch)
        sa = [serial_sum(self.ring_a[ch, s]) for s in pieces]
        sb = [serial_sum(self.ring_b[ch, s]) for s in pieces]
        self.va[ch] = sa[0] + sa[1] if len(sa) == 2 else sa[0]     # sum(tail part) + sum(head part)
        self.vb[ch] = sb[0] + sb[1] if len(sb) == 2 else sb[0]

    def process(self, in_a, in_b):
        """-> (out, trace): the output rows and (va, vb) after every sample, [2, C, n]."""
        in_a, in_b = np.asarray(in_a, f32), np.asarray(in_b, f32)
        C, n = in_a.shape
        out, trace = np.empty((C, n), f32), np.empty((2, C, n), f32)
        rows = self.rows
        linear = self.law == PAN_LAW_LINEAR
        thresh = np.where(linear, LINEAR_THRESHOLD, POWER_THRESHOLD).astype(f32)
        sq_a, sq_b = in_a * in_a, in_b * in_b                               # dsp::sqr2
        with np.errstate(all="ignore"):
            for t in range(n):
                due = self.window >= self.period
                if due.any():
                    for ch in np.flatnonzero(due):
                        self._refresh(ch)
                    self.window[due] = 0
                tail = (self.head + self.cap - self.period) % self.cap
                at, bt = self.ring_a[rows, tail], self.ring_b[rows, tail]
                ah, bh = sq_a[:, t], sq_b[:, t]
                self.ring_a[rows, self.head], self.ring_b[rows, self.head] = ah, bh
                self.va = (self.va + ah) - at
                self.vb = (self.vb + bh) - bt
                sl, sr = np.abs(self.va) * self.norm, np.abs(self.vb) * self.norm
                sl, sr = np.where(linear, np.sqrt(sl), sl), np.where(linear, np.sqrt(sr), sr)
                den = sl + sr
                ok = den > thresh
                out[:, t] = np.where(ok, sr / np.where(ok, den, f32(1.0)), self.dflt)
                trace[0, :, t], trace[1, :, t] = self.va, self.vb
                self.head = (self.head + 1) % self.cap
                self.window += 1
        return out, trace

    def state(self):
        return {"value_a": self.va.copy(), "value_b": self.vb.copy(), "head": self.head.astype(np.uint32),
                "window": self.window.astype(np.uint32)}
