"""lsp::dspu::ScaledMeterGraph restated in numpy (src/main/util/ScaledMeterGraph.cpp, RawRingBuffer.cpp), line for line where it
matters: two samplers over one row, the folds with their compares as the reference writes them, update_period() with its -1.0f
sentinel as the counted loop that the reference runs, the two raw rings.  float32 throughout; every result is compared in bits.

The four primitives are tests/metergraph_ref.py's.  `without` names quirks to take out, for the tests that show
that each of them matters:
    "carry"      the block forms fold MM_ABS_MAXIMUM into an open frame with > (MeterGraph's sense) instead of <
    "push"       the single-sample form pushes fCurrent instead of the sample
    "else_if"    update_period() does not push sFrames.fCurrent where the history's frame is closed
    "sentinel"   "unset" is "first sub-sample of the group" instead of fCurrent < 0.0f
    "reset"      sFrames.sBuffer.reset() zeroes the words too"""
import numpy as np

from metergraph_ref import (ABS_MAXIMUM, ABS_MINIMUM, SIGN_MAXIMUM, SIGN_MINIMUM, PEAK, METHOD_NAMES,  # noqa: F401
                            abs_max, abs_min, sign_max, sign_min)

f32, u32 = np.float32, np.uint32
FRAMES_GAP = 0x10                                                   # :30

# the operations of a recorded case: (code, row, offset, n, value)
SET_METHOD, SET_PERIOD, FILL, PROCESS, PROCESS_GAIN, PROCESS_SINGLE, READ, LEVEL = range(8)
STATE_WORDS = 9         # behind the two rings: both heads, sHistory's fCurrent, nCount, nPeriod, sFrames' three, nPeriod


class RawRingBuffer:
    """RawRingBuffer.cpp: init (:47-59), reset (:79-82), push(float) (:127-131), read (:133-155), fill (:187-190)."""

    def __init__(self, size):
        self.data = np.zeros(size, f32)
        self.head = 0

    def reset(self):
        self.head = 0

    def push(self, v):
        self.data[self.head] = v
        self.head = (self.head + 1) % len(self.data)

    def read(self, offset):
        cap = len(self.data)
        return self.data[(self.head + cap - offset) % cap]

    def read_block(self, offset, count):
        cap = len(self.data)
        count = min(count, cap)
        tail = (self.head + cap - offset) % cap
        return self.data[(tail + np.arange(count)) % cap].copy()

    def fill(self, v):
        self.data[:] = f32(v)


class Sampler:
    def __init__(self, capacity, period, frames):
        self.buffer = RawRingBuffer(capacity)
        self.current = f32(0.0)
        self.count = 0
        self.period = period
        self.frames = frames


def subframes(frames, subsampling, max_period):
    return (frames * max_period + subsampling - 1) // subsampling   # :69-70


class ScaledMeterGraph:
    def __init__(self, frames, subsampling, max_period, without=()):    # construct() and init(), :42-91
        assert subsampling >= 1 and frames >= 1 and max_period >= subsampling, "the reference is undefined there"
        sub = subframes(frames, subsampling, max_period)
        self.history = Sampler(sub + FRAMES_GAP, subsampling, sub)
        self.frames = Sampler(frames + FRAMES_GAP, 0, frames)
        self.period = 0
        self.max_period = max_period
        self.method = ABS_MAXIMUM
        self.without = frozenset(without)

    def set_method(self, m):
        self.method = int(m)

    def set_period(self, p):                                        # :95
        p = int(p) & 0xFFFFFFFF
        lo, hi = self.history.period, self.max_period
        self.period = lo if p < lo else hi if p > hi else p

    def fill(self, v):                                              # :376-383
        self.frames.buffer.fill(v)
        self.frames.count = 0
        self.history.buffer.fill(v)
        self.history.count = 0

    def level(self):                                                # :373
        return self.frames.buffer.read(1)

    def read(self, count):                                          # :365-369
        count = min(count, self.frames.frames)
        return self.frames.buffer.read_block(count, count)

    def _single(self, sp, sample):                                  # :103-145
        sample = f32(sample)
        m, cur = self.method, sp.current
        if m == SIGN_MINIMUM:
            if sp.count == 0 or np.abs(cur) > np.abs(sample):       # :109
                cur = sample
        elif m == SIGN_MAXIMUM:
            if sp.count == 0 or np.abs(cur) < np.abs(sample):       # :114
                cur = sample
        elif m == ABS_MINIMUM:
            sample = np.abs(sample)
            if sp.count == 0 or cur > sample:                       # :120
                cur = sample
        elif m == PEAK:
            if sp.count == 0:                                       # :125
                cur = sample
        else:
            sample = np.abs(sample)
            if sp.count == 0 or cur < sample:                       # :132
                cur = sample
        sp.current = f32(cur)
        sp.count += 1
        if sp.count >= sp.period:                                   # :140
            sp.buffer.push(sp.current if "push" in self.without else sample)    # :142: the sample
            sp.count = 0

    def _block(self, sp, s, g):                                     # :147-206 and :208-267
        at, n = 0, len(s)
        with np.errstate(all="ignore"):
            while at < n:
                todo = min(n - at, (sp.period - sp.count) & 0xFFFFFFFF)    # :152
                if todo > 0:
                    chunk = s[at:at + todo]
                    m, cur = self.method, sp.current
                    if m == SIGN_MINIMUM:
                        sample = sign_min(chunk) if g is None else f32(sign_min(chunk) * g)
                        if sp.count == 0 or np.abs(cur) > np.abs(sample):   # :161
                            cur = sample
                    elif m == SIGN_MAXIMUM:
                        sample = sign_max(chunk) if g is None else f32(sign_max(chunk) * g)
                        if sp.count == 0 or np.abs(cur) < np.abs(sample):   # :168
                            cur = sample
                    elif m == ABS_MINIMUM:
                        sample = abs_min(chunk) if g is None else f32(abs_min(chunk) * g)
                        if sp.count == 0 or cur > sample:                   # :175
                            cur = sample
                    elif m == PEAK:
                        if sp.count == 0:                                   # :181
                            cur = chunk[0] if g is None else f32(chunk[0] * g)
                    else:
                        sample = abs_max(chunk) if g is None else f32(abs_max(chunk) * g)
                        carry = (cur > sample) if "carry" in self.without else (cur < sample)   # :189: <
                        if sp.count == 0 or carry:
                            cur = sample
                    sp.current = f32(cur)
                    sp.count += todo
                    at += todo
                if sp.count >= sp.period:                                   # :200
                    sp.buffer.push(sp.current)
                    sp.count = 0

    def update_period(self):                                        # :269-342
        h, fr = self.history, self.frames
        if self.period == fr.period:
            return False
        if h.count > 0:                                             # :275
            h.buffer.push(h.current)
            h.count = 0
        elif fr.count > 0 and "else_if" not in self.without:        # :280
            h.buffer.push(fr.current)
        fr.count = 0
        fr.period = self.period
        fr.current = f32(-1.0)
        samples = (fr.period * fr.frames) & 0xFFFFFFFF              # :288, uint32_t
        subsamples = (samples + h.period - 1) // h.period
        fr.buffer.reset()                                           # :291: the head; the words stay
        if "reset" in self.without:
            fr.buffer.data[:] = 0
        m = self.method
        first = True
        for i in range(subsamples):
            sub = h.buffer.read(subsamples - i)
            cur = fr.current
            unset = first if "sentinel" in self.without else cur < 0.0
            if m == SIGN_MINIMUM:
                if unset or np.abs(cur) > np.abs(sub):              # :302
                    cur = sub
            elif m == SIGN_MAXIMUM:
                if unset or np.abs(cur) < np.abs(sub):              # :308
                    cur = sub
            elif m == ABS_MINIMUM:
                sample = np.abs(sub)
                if unset or cur > sample:                           # :315
                    cur = sample
            else:                                                   # MM_PEAK too
                sample = np.abs(sub)
                if unset or cur < sample:                           # :324
                    cur = sample
            fr.current = f32(cur)
            first = False
            fr.count += h.period
            if fr.count >= fr.period:                               # :333
                fr.buffer.push(fr.current)
                fr.count -= fr.period
                fr.current = f32(-1.0)
                first = True
        return True

    def process_single(self, sample):                               # :344-349
        self._single(self.history, sample)
        if not self.update_period():
            self._single(self.frames, sample)

    def process(self, s, gain=None):                                # :351-363
        assert self.period != 0, "the reference never returns with sFrames.nPeriod == 0"
        s = np.asarray(s, f32)
        g = None if gain is None else f32(gain)
        self._block(self.history, s, g)
        if not self.update_period():
            self._block(self.frames, s, g)

    def state_words(self):
        """The history ring, the frame ring, then both heads, sHistory's fCurrent, nCount, nPeriod, sFrames' three and nPeriod."""
        h, fr = self.history, self.frames
        tail = [h.buffer.head, fr.buffer.head, np.array(h.current, f32).view(u32), h.count, h.period,
                np.array(fr.current, f32).view(u32), fr.count, fr.period, self.period]
        return np.concatenate([h.buffer.data.view(u32), fr.buffer.data.view(u32), np.array(tail, u32)])


def group_bounds(hp, P, frames):
    """The closed form of update_period()'s counting: (subsamples, [(first, last) of every frame, 1-based], leftover nCount)."""
    sub = (P * frames + hp - 1) // hp
    last = [((k + 1) * P + hp - 1) // hp for k in range(frames)]
    first = [1] + [v + 1 for v in last[:-1]]
    return sub, list(zip(first, last)), sub * hp - P * frames


def counted_bounds(hp, P, frames):
    """The same from the reference's loop, :294-339."""
    sub = (P * frames + hp - 1) // hp
    groups, count, start = [], 0, 1
    for i in range(1, sub + 1):
        count += hp
        if count >= P:
            groups.append((start, i))
            count -= P
            start = i + 1
    return sub, groups, count, start


def run_case(x, case, without=()):
    """The operations of one case on a fresh graph: the state words after every operation and what READ and LEVEL returned."""
    g = ScaledMeterGraph(case["frames"], case["subsampling"], case["max_period"], without)
    states, answers = [], []
    for code, row, off, n, value in case["ops"]:
        code, row, off, n = int(code), int(row), int(off), int(n)
        value = f32(value)
        if code == SET_METHOD:
            g.set_method(n)
        elif code == SET_PERIOD:
            g.set_period(n)
        elif code == FILL:
            g.fill(value)
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
