"""CPU restatement of lsp::dspu::Oversampler (src/main/util/Oversampler.cpp) for the tests: numpy float32, so every
product and every sum is rounded on its own, as the kernels round them.

The reference scatters each input into a zero-filled buffer of pending sums with lsp-dsp-lib's lanczos_resample_NxK.
Gathered, oldest input first, the sum starting from +0.0f as the zero-filled buffer makes it:
    y[N i + k] = (((+0 + h_k[2a-1] x[i-2a+1]) + h_k[2a-2] x[i-2a+2]) + ...) + h_k[0] x[i],   y[N i] = x[i - a] (copied)
with the table h of mi_oversampler_coefficients.  The state is the last 2a inputs of each channel.  The anti-alias filter
is the oracle's design of the reference's parameters (:108-126) run by the oracle's biquad bank."""
import numpy as np

from oracle import binding, filter_design

OM_NONE = 0
TIMES = (2, 3, 4, 6, 8)
WIDTHS = (2, 3, 4, 4, 10, 62)               # X2, X3, X4, 12BIT, 16BIT, 24BIT
NAMES = ("2", "3", "4", "12BIT", "16BIT", "24BIT")
MODES = {"%dX%s" % (n, k): 1 + 6 * g + j for g, n in enumerate(TIMES) for j, k in enumerate(NAMES)}
UP_MODE, UP_SAMPLE_RATE, UP_OTHER = 1, 4, 8
FLT_NONE, FLT_BT_BWC_LOPASS = 0, 29


def oversampling(mode):
    """Oversampler::get_oversampling, Oversampler.cpp:146-195."""
    return TIMES[(mode - 1) // 6] if 1 <= mode <= 30 else 1


def latency(mode):
    """Oversampler::latency, Oversampler.cpp:955-1006."""
    return WIDTHS[(mode - 1) % 6] if 1 <= mode <= 30 else 0


def filter_params(sr):
    """Oversampler::set_sample_rate, :117-125: (type, slope, freq, freq2, gain, quality)."""
    f = min(np.float32(20000.0), np.float32(np.float32(sr) * np.float32(0.42)))
    return FLT_BT_BWC_LOPASS, 30, f, f, np.float32(1.0), np.float32(0.1)


def gather(ext, h, n, dtype=np.float32):
    """The N x n oversampled values behind ext = [2a inputs before the block, the block of n] in `dtype`; phase 0 copied."""
    N, taps = h.shape
    a = taps // 2
    ext = ext.astype(dtype)
    out = np.empty((ext.shape[0], n, N), dtype)
    out[:, :, 0] = ext[:, taps - a:taps - a + n]
    acc, prod = np.empty((ext.shape[0], n), dtype), np.empty((ext.shape[0], n), dtype)
    for k in range(1, N):
        acc[:] = 0
        for t in range(taps - 1, -1, -1):
            np.multiply(ext[:, taps - t:taps - t + n], dtype(h[k, t]), out=prod)
            np.add(acc, prod, out=acc)
        out[:, :, k] = acc
    return out.reshape(ext.shape[0], n * N)


class OversamplerRef:
    """`channels` oversamplers; `table(mode)` returns the [N][2a] float32 coefficients."""

    def __init__(self, channels, table):
        self.channels, self.table = channels, table
        self.mode, self.sample_rate, self.filter, self.update = OM_NONE, 0, True, UP_MODE | UP_SAMPLE_RATE | UP_OTHER
        self.params, self.design_rate = None, 0             # None: FLT_NONE
        self.state = np.zeros((channels, 0), np.float32)
        self.sections = np.zeros((0, 5), np.float32)
        self.memory = np.zeros((channels, 1, 2), np.float32)

    # -- settings -------------------------------------------------------------------------------------------------
    def set_sample_rate(self, sr):                          # :108-126
        if sr == self.sample_rate:
            return
        self.sample_rate = sr
        self.update |= UP_SAMPLE_RATE
        self.params = filter_params(sr)
        self.design_rate = sr * oversampling(self.mode)

    def set_mode(self, mode):                               # :1055-1063
        if mode != self.mode:
            self.mode = mode
            self.update |= UP_MODE

    def set_filtering(self, on):                            # Oversampler.h:191-197
        if bool(on) != self.filter:
            self.filter = bool(on)
            self.update |= UP_MODE

    def modified(self):
        return self.update != 0

    def update_settings(self):                              # :128-144
        clear = bool(self.update & (UP_MODE | UP_SAMPLE_RATE))
        self.design_rate = self.sample_rate * oversampling(self.mode)
        if self.params is None or self.design_rate == 0:
            sections = np.zeros((0, 5), np.float32)
        else:
            mode, _, sections = filter_design.design(filter_design.Params(*self.params), self.design_rate)
            if mode == filter_design.FM_BYPASS:
                sections = np.zeros((0, 5), np.float32)
        if clear or len(sections) != len(self.sections):    # FilterBank::end(clear), FilterBank.cpp:233-235
            self.memory = np.zeros((self.channels, max(1, len(sections)), 2), np.float32)
        self.sections = sections
        if clear:
            self.state = np.zeros((self.channels, 0), np.float32)
        self.update = 0

    def oversampling(self):
        return oversampling(self.mode)

    def latency(self):
        return latency(self.mode)

    # -- processing -----------------------------------------------------------------------------------------------
    def _state(self, taps):
        """The last `taps` inputs; what is missing is zero (a cleared state)."""
        st = np.zeros((self.channels, taps), np.float32)
        have = min(taps, self.state.shape[1])
        if have:
            st[:, taps - have:] = self.state[:, -have:]
        return st

    def upsample(self, x):                                  # :197-367
        x = np.ascontiguousarray(x, np.float32)
        if self.mode == OM_NONE:
            return x.copy()
        h = np.asarray(self.table(self.mode), np.float32)
        taps = h.shape[1]
        ext = np.concatenate([self._state(taps), x], axis=1)
        self.state = ext[:, -taps:].copy()
        return gather(ext, h, x.shape[1])

    def _filtered(self, y):
        if not self.filter or len(self.sections) == 0:
            return y
        C, S = self.channels, len(self.sections)
        coef = np.ascontiguousarray(np.broadcast_to(self.sections, (C, S, 5)), np.float32)
        return binding.biquad_bank(y, coef, np.full(C, S, np.uint32), self.memory)

    def downsample(self, y):                                # :369-525
        y = np.ascontiguousarray(y, np.float32)
        if self.mode == OM_NONE:
            return y.copy()
        return np.ascontiguousarray(self._filtered(y)[:, ::oversampling(self.mode)])

    def process(self, x, callback=None):                    # :527-953; callback(block) returns the worked-on block
        if self.mode == OM_NONE:
            x = np.ascontiguousarray(x, np.float32).copy()
            return callback(x) if callback is not None else x
        y = self.upsample(x)
        if callback is not None:
            y = np.ascontiguousarray(callback(y), np.float32)
        return self.downsample(y)
