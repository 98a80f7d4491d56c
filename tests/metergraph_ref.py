"""lsp::dspu::MeterGraph restated in numpy (src/main/util/MeterGraph.cpp, RingBuffer.cpp), line for line where it matters: the
chunks of a call, the folds into fCurrent with their compares as the reference writes them, the ring.  float32 throughout; every
result is compared in bits.

The four primitives that the reference tree does not carry are defined here as DESIGN.md 3.30 defines them (lsp-dsp-lib's generic
ones): the result starts as the first element (its fabsf for the abs_* pair), a later element replaces it only where its magnitude
is strictly larger (smaller), the sign_* pair returns the signed element; no samples give 0."""
import numpy as np

f32, u32 = np.float32, np.uint32
ABS_MAXIMUM, ABS_MINIMUM, SIGN_MAXIMUM, SIGN_MINIMUM, PEAK = range(5)
METHOD_NAMES = ("abs_maximum", "abs_minimum", "sign_maximum", "sign_minimum", "peak")

# the operations of a recorded case: (code, row, offset, n, value)
SET_METHOD, SET_PERIOD, SET_DEFAULT, FILL, CLEAR, PROCESS, PROCESS_GAIN, PROCESS_SINGLE, READ, LEVEL = range(10)


def _winner(mag, larger):
    """Index of the first strictly largest (smallest) magnitude, the way a serial loop from element 0 finds it: a NaN in first place
    stays (no compare with it holds), a NaN elsewhere never wins."""
    if np.isnan(mag[0]):
        return 0
    m = np.where(np.isnan(mag), f32(-1.0) if larger else f32(np.inf), mag)
    return int(np.argmax(m)) if larger else int(np.argmin(m))      # the first of equals: index 0 is never a stand-in


def abs_max(s):
    return f32(0.0) if len(s) == 0 else np.abs(s)[_winner(np.abs(s), True)]


def abs_min(s):
    return f32(0.0) if len(s) == 0 else np.abs(s)[_winner(np.abs(s), False)]


def sign_max(s):
    return f32(0.0) if len(s) == 0 else s[_winner(np.abs(s), True)]


def sign_min(s):
    return f32(0.0) if len(s) == 0 else s[_winner(np.abs(s), False)]


class RingBuffer:
    """RingBuffer.cpp: init (:48-63), append(float) (:102-106), fill (:115-120), get (:122-129, :147-183)."""

    def __init__(self, size, fill):
        self.data = np.full(size, f32(fill), f32)
        self.head = 0

    def append(self, v):
        self.data[self.head] = v
        self.head = (self.head + 1) % len(self.data)

    def fill(self, v):
        self.head = 0
        self.data[:] = f32(v)

    def get(self, offset):
        cap = len(self.data)
        return f32(0.0) if offset >= cap else self.data[(self.head + cap - offset - 1) % cap]

    def get_block(self, offset, count):
        cap = len(self.data)
        dst = np.zeros(count, f32)
        at = 0
        if offset >= cap:
            lead = min(count, offset - cap + 1)
            offset -= lead
            if offset >= cap:
                return dst
            count -= lead
            at = lead
        tail = (self.head + cap - offset - 1) % cap
        to_read = min(count, offset + 1)
        idx = (tail + np.arange(to_read)) % cap
        dst[at:at + to_read] = self.data[idx]
        return dst


class MeterGraph:
    def __init__(self, frames, period, default_value=0.0):          # construct() and init(), :40-68
        assert period > 0, "init() refuses a period of 0"
        self.buffer = RingBuffer(frames, default_value)
        self.current = f32(0.0)
        self.default = f32(default_value)
        self.count = 0
        self.period = int(period) & 0xFFFFFFFF
        self.method = ABS_MAXIMUM

    def set_method(self, m):
        self.method = int(m)

    def set_period(self, p):
        self.period = int(p) & 0xFFFFFFFF

    def set_default_value(self, v):
        self.default = f32(v)

    def fill(self, v):
        self.buffer.fill(v)

    def clear(self):
        self.buffer.fill(self.default)

    def level(self):
        return self.buffer.get(0)

    def process_single(self, sample):                               # :70-111
        sample = f32(sample)
        m, cur = self.method, self.current
        if m == SIGN_MINIMUM:
            if self.count == 0 or np.abs(cur) > np.abs(sample):     # :76
                cur = sample
        elif m == SIGN_MAXIMUM:
            if self.count == 0 or np.abs(cur) < np.abs(sample):     # :81
                cur = sample
        elif m == ABS_MINIMUM:
            sample = np.abs(sample)
            if self.count == 0 or cur > sample:                     # :87
                cur = sample
        elif m == PEAK:
            if self.count == 0:                                     # :92
                cur = sample
        else:
            sample = np.abs(sample)
            if self.count == 0 or cur < sample:                     # :99
                cur = sample
        self.current = f32(cur)
        self.count = (self.count + 1) & 0xFFFFFFFF
        if self.count >= self.period:                               # :105
            self.buffer.append(self.current)
            self.count = 0

    def process(self, s, gain=None):                                # :113-178 and :180-244
        assert self.period != 0, "the reference never returns with a period of 0"
        s = np.asarray(s, f32)
        n, at = len(s), 0
        g = None if gain is None else f32(gain)
        with np.errstate(all="ignore"):
            while n > 0:
                can_do = min(n, (self.period - self.count) & 0xFFFFFFFF)   # uint32_t arithmetic, :118
                if can_do > 0:
                    chunk = s[at:at + can_do]
                    m, cur = self.method, self.current
                    if m == SIGN_MINIMUM:
                        sample = sign_min(chunk) if g is None else f32(sign_min(chunk) * g)
                        if self.count == 0 or np.abs(cur) > np.abs(sample):    # :129
                            cur = sample
                    elif m == SIGN_MAXIMUM:
                        sample = sign_max(chunk) if g is None else f32(sign_max(chunk) * g)
                        if self.count == 0 or np.abs(cur) < np.abs(sample):    # :136
                            cur = sample
                    elif m == ABS_MINIMUM:
                        sample = abs_min(chunk) if g is None else f32(abs_min(chunk) * g)
                        if self.count == 0 or cur > sample:                    # :143
                            cur = sample
                    elif m == PEAK:
                        if self.count == 0:                                    # :149
                            cur = chunk[0] if g is None else f32(chunk[0] * g)
                    else:
                        sample = abs_max(chunk) if g is None else f32(abs_max(chunk) * g)
                        if self.count == 0 or cur > sample:                    # :158: > where process(float) has <
                            cur = sample
                    self.current = f32(cur)
                    self.count = (self.count + can_do) & 0xFFFFFFFF
                    n -= can_do
                    at += can_do
                if self.count >= self.period:                                  # :171
                    self.buffer.append(self.current)
                    self.count = 0

    def read(self, count):                                          # :246-258
        cap = len(self.buffer.data)
        lead = max(0, count - cap)
        if lead:
            count = cap
        if count == 0:
            return np.full(lead, self.default, f32)
        return np.concatenate([np.full(lead, self.default, f32), self.buffer.get_block(count - 1, count)])

    def state_words(self):
        """The ring's words, then nHead, fCurrent's bits and nCount."""
        return np.concatenate([self.buffer.data.view(u32), np.array([self.buffer.head, np.array(self.current, f32).view(u32), self.count], u32)])


def run_case(x, case):
    """The operations of one case on a fresh graph: the state words after every operation and what READ and LEVEL returned."""
    g = MeterGraph(case["frames"], case["period"], case["default"])
    states, answers = [], []
    for code, row, off, n, value in case["ops"]:
        code, row, off, n = int(code), int(row), int(off), int(n)
        value = f32(value)
        if code == SET_METHOD:
            g.set_method(n)
        elif code == SET_PERIOD:
            g.set_period(n)
        elif code == SET_DEFAULT:
            g.set_default_value(value)
        elif code == FILL:
            g.fill(value)
        elif code == CLEAR:
            g.clear()
        elif code == PROCESS:
            g.process(x[row, off:off + n])
        elif code == PROCESS_GAIN:
            g.process(x[row, off:off + n], value)
        elif code == PROCESS_SINGLE:
            for v in x[row, off:off + n]:
                g.process_single(v)
        elif code == READ:
            answers.append(g.read(n).view(u32))
        elif code == LEVEL:
            answers.append(np.array([g.level()], f32).view(u32))
        else:
            raise ValueError(code)
        states.append(g.state_words())
    return np.stack(states), (np.concatenate(answers) if answers else np.zeros(0, u32))
