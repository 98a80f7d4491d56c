"""CPU restatement of lsp::dspu::TruePeakMeter (src/main/meters/TruePeakMeter.cpp) for the tests: numpy float32, so every
product and every sum is rounded on its own, as the kernels round them.

The reference scatters each input into a buffer of pending sums with lsp-dsp-lib's lanczos_resample_Nx16bit (a = 10) and
reduces every N oversampled values to their largest magnitude (reduce_Nx, :115-147).  Gathered, oldest input first:
    y[N i + k] = ((h_k[19] x[i-19] + h_k[18] x[i-18]) + ...) + h_k[0] x[i],   y[N i] = x[i - 10]
with the table h of mi_truepeak_coefficients.  The state is the last 20 inputs of each channel."""
import numpy as np

A = 10
TAPS = 2 * A


def oversampling(sample_rate):
    """TruePeakMeter::calc_oversampling_multiplier, TruePeakMeter.cpp:85-100."""
    f = 4 * 44100
    for times, mul in ((0, 1), (2, 2), (3, 3), (4, 4), (6, 6)):
        if sample_rate * mul >= f:
            return times
    return 8


class TruePeakRef:
    """`channels` meters; `table(times)` returns the [times][20] float32 coefficients."""

    def __init__(self, channels, table):
        self.channels, self.table = channels, table
        self.sample_rate, self.times, self.pending = 0, 0, True
        self.state = np.zeros((channels, TAPS), np.float32)

    def set_sample_rate(self, sr):                  # :102-109
        if sr != self.sample_rate:
            self.sample_rate, self.pending = sr, True

    def update_settings(self):                      # :149-189
        if not self.pending:
            return
        self.pending = False
        times = oversampling(self.sample_rate)
        if times != self.times:
            self.times = times
            self.clear()

    def clear(self):                                # :191-195
        self.state[:] = 0

    def latency(self):                              # :274-277
        return A if self.times else 0

    def process(self, x):                           # :197-236
        self.update_settings()
        x = np.asarray(x, np.float32)
        n, N = x.shape[1], self.times
        if N == 0:
            return np.abs(x)
        h = np.asarray(self.table(N), np.float32)
        ext = np.concatenate([self.state, x], axis=1)          # ext[:, TAPS + i] = x[i]
        out = np.abs(ext[:, TAPS - A:TAPS - A + n])
        for k in range(1, N):
            acc = h[k, TAPS - 1] * ext[:, 1:1 + n]
            for t in range(TAPS - 2, -1, -1):
                acc = acc + h[k, t] * ext[:, TAPS - t:TAPS - t + n]
            out = np.maximum(out, np.abs(acc))
        self.state = ext[:, -TAPS:].copy()
        return out

    def process_max(self, x):
        """The largest value process() writes per channel (what the header documents; the reference's returns 0.0f)."""
        return self.process(x).max(axis=1) if np.asarray(x).shape[1] else np.zeros(self.channels, np.float32)
