"""lsp::dspu::DynamicDelay (src/main/util/DynamicDelay.cpp) restated in numpy, serial, one step per sample as the reference's loop
has it.  tests/test_dyndelay_host.py pins it to the recorded reference cases bit for bit (out, the line and the head); the GPU
tests hold the bank to it.

Where the reference has no defined behaviour this restatement has the bank's: a delay converts with saturation (NaN: 0, beyond the
range: the largest delay), a NaN feedback delay counts as 0."""
import numpy as np

f32 = np.float32
BUF_SIZE = 0x400

# the operations of a recorded case, (what, argument); A is the case's line, B a second one for copy()
P_A, P_B, CLEAR_A, COPY_A_FROM_B, COPY_B_FROM_A, SET_HEAD_A, SET_HEAD_B = range(7)
# the ring of a recorded case: whole up to RING_WHOLE floats, else the RING_BEHIND positions behind the head
RING_WHOLE, RING_BEHIND = 8192, 4096


def capacity_of(max_size):
    d = max_size + 1
    return d - d % BUF_SIZE + 2 * BUF_SIZE


def indices(head, capacity, max_delay, delay, fdelay):
    """shift, tail and feed of every step of a call that starts with the head at `head` (int64 arrays)."""
    delay, fdelay = np.asarray(delay, f32), np.asarray(fdelay, f32)
    n = delay.size
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.where(np.isnan(delay), f32(0), delay)
        shift = np.where(d >= f32(max_delay), np.int64(max_delay), np.where(d > 0, np.trunc(np.clip(d, 0, 1e9)), 0).astype(np.int64))
        h = (head + np.arange(n, dtype=np.int64)) % capacity
        tail = h - shift
        tail = np.where(tail < 0, tail + capacity, tail)
        lim = shift.astype(f32)
        back = np.where(fdelay < 0, f32(0), np.where(fdelay > lim, lim, np.where(np.isnan(fdelay), f32(0), fdelay))).astype(f32)
        feed = (tail.astype(f32) + back).astype(f32).astype(np.int64)       # the float32 sum, then truncated
        feed = np.where(feed >= capacity, feed - capacity, feed)
    return shift, tail, feed


class DynamicDelay:
    def __init__(self, max_size):
        self.max_delay = int(max_size)
        self.capacity = capacity_of(self.max_delay)
        self.line = np.zeros(self.capacity, f32)
        self.made = np.zeros(self.capacity, bool)           # the cell holds a sum (not a copy of an input, nor what was put there)
        self.out_made = np.zeros(0, bool)                   # ... and so did the cells that the last call's output was read from
        self.head = 0

    def clear(self):
        self.line[:] = 0
        self.made[:] = False
        self.head = 0

    def process(self, inp, delay, fgain, fdelay):
        inp, fgain = np.asarray(inp, f32), np.asarray(fgain, f32)
        n = inp.size
        _, tail, feed = indices(self.head, self.capacity, self.max_delay, delay, fdelay)
        out, line, cap, h = np.empty(n, f32), self.line, self.capacity, self.head
        made, self.out_made = self.made, np.empty(n, bool)
        tail, feed = tail.tolist(), feed.tolist()
        with np.errstate(all="ignore"):
            for i in range(n):
                t, f = tail[i], feed[i]
                line[h] = inp[i]
                made[h] = False
                s = line[t]
                line[f] = line[f] + s * fgain[i]            # two roundings
                made[f] = True
                out[i] = line[t]
                self.out_made[i] = made[t]
                h = h + 1 if h + 1 < cap else 0
        self.head = h
        return out

    def copy(self, s):
        count = min(self.capacity, s.capacity)
        dt = self.capacity - count
        newest = np.take(s.line, (s.head - count + np.arange(count)) % s.capacity)
        self.line[dt:] = newest
        self.line[:dt] = 0
        self.made[dt:] = np.take(s.made, (s.head - count + np.arange(count)) % s.capacity)
        self.made[:dt] = False
        self.head = 0

    def ring(self):
        """What a recorded case keeps of the line."""
        return ring_part(self.line, self.head)


def ring_part(line, head):
    if line.size <= RING_WHOLE:
        return line.copy()
    return np.take(line, (head - RING_BEHIND + np.arange(RING_BEHIND)) % line.size)


def run_case(case):
    """A recorded case (max_size, other_size, ops, rows [4, N]: in, delay, fgain, fdelay) -> out [N], the two lines, and which of
    the outputs are sums."""
    a, b = DynamicDelay(case["max_size"]), DynamicDelay(case["other_size"])
    rows, at, out = case["rows"], 0, np.zeros(case["rows"].shape[1], f32)
    made = np.zeros(out.size, bool)
    for what, arg in case["ops"].tolist():
        if what in (P_A, P_B):
            r, unit = rows[:, at:at + arg], (a if what == P_A else b)
            out[at:at + arg] = unit.process(r[0], r[1], r[2], r[3])
            made[at:at + arg] = unit.out_made
            at += arg
        elif what == CLEAR_A:
            a.clear()
        elif what == COPY_A_FROM_B:
            a.copy(b)
        elif what == COPY_B_FROM_A:
            b.copy(a)
        elif what == SET_HEAD_A:
            a.head = arg
        elif what == SET_HEAD_B:
            b.head = arg
        else:
            raise ValueError(what)
    assert at == out.size
    return out, a, b, made


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same(got, want, made=True):
    """Bit for bit; where arithmetic made a NaN (`made`: the value is a sum), a NaN: IEEE 754 leaves the sign and the payload of
    such a NaN to the machine, and the machines differ.  A NaN that was only carried along keeps its bits."""
    got, want = np.asarray(got, f32), np.asarray(want, f32)
    return bool(got.shape == want.shape and np.all((bits(got) == bits(want)) | (np.asarray(made, bool) & np.isnan(got) & np.isnan(want))))
