"""The DynamicDelay bank and the C++ class on the device, held to the serial numpy restatement bit for bit: out, the whole line and
the head.  Shapes on both sides of the kernel's stretch of 0x400 samples and of its runs of 256 steps, lines in LDS and in global
memory, every conflict class, single conflicts, shared feeds, calls cut in pieces, in-place and strided rows, special values, what
the bank defines where the reference does not, heads beyond 2^23, copy and clear, streams, capture, misuse, lifetimes, and every
recorded case of the reference through the C-ABI and through the class.

The comparison is uint32 equality (dyndelay_ref.same).  One kind of value cannot be held to it: a NaN that an addition or a product
MADE (Inf - Inf, 0 * Inf, or a NaN operand).  IEEE 754 leaves its sign and payload open, the host's SSE unit and the GPU choose
differently, so there a NaN is asked for, not its bits.  A NaN that is only carried along (an input that reaches out or the line
without taking part in a sum) keeps its bits and is compared bit for bit."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import dyndelay_ref as dd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "lsp-dsp-units_amd")
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_dyndelay_vectors as gen  # noqa: E402

f32 = np.float32
u32 = np.uint32
EINVAL, ESTATE = -1, -5
COUNTS = [1, 63, 64, 65, 1023, 1024, 1025, 2500]
CHANNELS = [1, 5]
SIZES = [0, 5, 1000, 40000]             # the line of 1000 is worked on in LDS, that of 40000 (delays near it) in global memory
KINDS = ("echo", "chorus", "random", "fdelay 7", "small and large")
BIG = gen.BIG


def delay_rows(kind, max_size, n, rng):
    """delay and fdelay of one channel"""
    near = float(max_size) * 0.97
    t = np.arange(n)
    if kind == "echo":
        return np.full(n, near, f32), np.full(n, near, f32)
    if kind == "chorus":
        return ((near / 2 + near / 2.1 * np.sin(t / 83.0)).astype(f32), (near / 4 + near / 4.3 * np.sin(t / 47.0 + 1.0)).astype(f32))
    if kind == "random":
        return (rng.uniform(-0.2 * max_size - 2, 1.2 * max_size + 2, n).astype(f32), rng.uniform(-0.2 * max_size - 2, 1.2 * max_size + 2, n).astype(f32))
    if kind == "fdelay 7":
        return np.full(n, near, f32), np.full(n, 7, f32)
    # small and large delays in turn, changing inside and between the stretches: both placements meet the same line
    return (np.where((t // 700) % 2 == 0, 40.0, near).astype(f32), np.where((t // 300) % 2 == 0, 3.0, near).astype(f32))


def make_rows(C, n, max_size, seed, kinds=KINDS, shift=0):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((C, n)) * 0.5).astype(f32)
    g = rng.uniform(-0.95, 0.95, (C, n)).astype(f32)
    d, fd = np.empty((C, n), f32), np.empty((C, n), f32)
    for ch in range(C):
        d[ch], fd[ch] = delay_rows(kinds[(ch + shift) % len(kinds)], max_size, n, rng)
    return x, d, g, fd


class Pair:
    """A bank and the restatement of each of its channels, with the same lines and heads."""

    def __init__(self, gpu, C, max_size, head=None, seed=5, fill=True):
        self.gpu, self.C = gpu, C
        self.bank = gpu.DynamicDelayBank(C, max_size)
        self.refs = [dd.DynamicDelay(max_size) for _ in range(C)]
        assert self.bank.capacity == self.refs[0].capacity and self.bank.max_delay == max_size
        rng = np.random.default_rng(seed)
        for ch, r in enumerate(self.refs):
            if fill:
                r.line[:] = (rng.standard_normal(r.capacity) * 0.5).astype(f32)
                self.bank.write_line(ch, r.line)
            if head is not None:
                r.head = (head + 3 * ch) % r.capacity
                self.bank.set_state(ch, r.head)

    def process(self, rows, out=None, stream=None, **strides):
        """rows: four [C, n] arrays; the restatement moves on, the bank's output comes back"""
        x, d, g, fd = rows
        n = x.shape[1]
        bufs = [self.gpu.DeviceBuffer.from_host(np.ascontiguousarray(r)) for r in rows]
        o = self.gpu.DeviceBuffer((self.C, n)) if out is None else out
        self.bank.process(o, *bufs, n, stream=stream, **strides)
        want = np.array([r.process(x[ch], d[ch], g[ch], fd[ch]) for ch, r in enumerate(self.refs)])
        return o.download(stream=stream), want

    def check(self, got, want, what=""):
        """Right behind the restatement's call: out, the head and the whole line of every channel (dyndelay_ref.same: bit for
        bit, and a NaN where a sum made a NaN)."""
        for ch, r in enumerate(self.refs):
            if got.shape[1]:
                assert dd.same(got[ch], want[ch], r.out_made), (what, ch, int(np.flatnonzero(dd.bits(got[ch]) != dd.bits(want[ch]))[0]))
            assert self.bank.get_state(ch)["head"] == r.head, (what, ch)
            line = self.bank.read_line(ch)
            assert dd.same(line, r.line, r.made), (what, ch, int(np.flatnonzero(dd.bits(line) != dd.bits(r.line))[0]))

    def run(self, rows, what="", **kw):
        got, want = self.process(rows, **kw)
        self.check(got, want, what)
        return got

    def close(self):
        self.bank.close()


@pytest.mark.gpu
@pytest.mark.parametrize("max_size", SIZES)
@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("C", CHANNELS)
def test_bit_exact_shapes(gpu, C, count, max_size):
    """Every channel another kind of rows, the head 700 in front of the wrap, the line full of old samples."""
    p = Pair(gpu, C, max_size, head=dd.capacity_of(max_size) - 700)
    p.run(make_rows(C, count, max_size, 11 + count), "first call")
    p.run(make_rows(C, count, max_size, 12 + count, shift=2), "second call")
    p.close()


CLASSES = ("0", "0.99", "1", "7", "63", "64", "delay")


@pytest.mark.gpu
@pytest.mark.parametrize("max_size,delay", [(1000, 300.0), (1000, 1000.0), (40000, 39000.0), (5, 5.0)])
def test_every_conflict_class(gpu, max_size, delay):
    """A constant delay and the feedback delays that decide how far apart a step's feed and its neighbours' tails are: one channel
    each, on a line that is staged in LDS and on one that is not."""
    C, n = len(CLASSES), 2500
    rng = np.random.default_rng(21)
    x, g = (rng.standard_normal((C, n)) * 0.5).astype(f32), rng.uniform(-0.95, 0.95, (C, n)).astype(f32)
    d = np.full((C, n), delay, f32)
    fd = np.array([np.full(n, delay if c == "delay" else float(c), f32) for c in CLASSES])
    p = Pair(gpu, C, max_size, head=dd.capacity_of(max_size) - 700)
    p.bank.count_steps(True)
    p.run((x, d, g, fd))
    side, total = p.bank.steps()
    assert total == C * n and 0 < side <= total
    p.close()


def _echo_with_conflicts(n, delay, at):
    """fdelay == delay (every feed is the step's own head) but at the steps `at`, whose feed is the head of the step before."""
    fd = np.full(n, delay, f32)
    fd[list(at)] = delay - 1
    return np.full(n, delay, f32), fd


@pytest.mark.gpu
@pytest.mark.parametrize("max_size", [1000, 40000])
def test_a_single_conflict_at_the_first_the_last_and_a_middle_step_of_a_run(gpu, max_size):
    """Runs are 256 steps at most: a conflict of step k with step k - 1 for k = 1 (the earliest there is), 128, 255, 256 (across two
    runs: none at all), 1023, 1024 (across two stretches), 1025 and 1279, one per channel, and all of them in the last channel."""
    spots = [1, 128, 255, 256, 1023, 1024, 1025, 1279]
    C, n, delay = len(spots) + 1, 1400, max_size * 0.9
    rng = np.random.default_rng(22)
    x, g = (rng.standard_normal((C, n)) * 0.5).astype(f32), rng.uniform(-0.95, 0.95, (C, n)).astype(f32)
    rows = [_echo_with_conflicts(n, delay, [s]) for s in spots] + [_echo_with_conflicts(n, delay, spots)]
    d, fd = np.array([r[0] for r in rows]), np.array([r[1] for r in rows])
    p = Pair(gpu, C, max_size, head=100)
    p.bank.count_steps(True)
    p.run((x, d, g, fd))
    side, total = p.bank.steps()
    assert total == C * n and side > 0.95 * total, "single conflicts must not send whole stretches down the serial path"
    p.close()


@pytest.mark.gpu
@pytest.mark.parametrize("max_size", [1000, 40000])
def test_two_steps_of_a_run_share_a_feed_and_the_order_of_the_adds_shows(gpu, max_size):
    n, delay, k = 600, max_size * 0.5, 300
    rng = np.random.default_rng(23)
    x, g = (rng.standard_normal((1, n)) * 0.5).astype(f32), rng.uniform(0.5, 0.95, (1, n)).astype(f32)
    d, fd = _echo_with_conflicts(n, delay, [k])
    # on the restatement: the cell is in[k - 1]; step k - 1 adds a, step k adds b, and (c + a) + b is not (c + b) + a
    probe = dd.DynamicDelay(max_size)
    probe.line[:] = (np.random.default_rng(5).standard_normal(probe.capacity) * 0.5).astype(f32)
    probe.head = 100
    probe.process(x[0, :k - 1], d[:k - 1], g[0, :k - 1], fd[:k - 1])
    _, tail, feed = dd.indices(probe.head, probe.capacity, max_size, d[k - 1:k + 1], fd[k - 1:k + 1])
    assert feed[0] == feed[1] == probe.head and tail[0] != tail[1]
    # the first addend takes the cell's input away, the second is a small fraction of it: added first, it is rounded away
    x[0, k - 1], g[0, k - 1], g[0, k] = 1.0, f32(-1.0) / probe.line[tail[0]], f32(2.0 ** -26) / probe.line[tail[1]]
    c, a, b = x[0, k - 1], probe.line[tail[0]] * g[0, k - 1], probe.line[tail[1]] * g[0, k]
    assert f32(f32(c + a) + b) != f32(f32(c + b) + a), "choose addends whose order shows"
    p = Pair(gpu, 1, max_size, head=100)
    p.run((x, d[None], g, fd[None]))
    assert dd.bits(p.refs[0].line[feed[0]]) == dd.bits(f32(f32(c + a) + b))
    p.close()


@pytest.mark.gpu
@pytest.mark.parametrize("max_size", [5, 1000, 40000])
def test_calls_cut_in_pieces_equal_one_call(gpu, max_size):
    C, n = 5, 2500
    rows = make_rows(C, n, max_size, 31)
    whole = Pair(gpu, C, max_size, head=dd.capacity_of(max_size) - 700)
    want = whole.run(rows, "one call")
    for piece in (1, 7, 256, 1023):
        m = n if piece > 1 else 300                                 # (300 calls of one sample)
        cut = Pair(gpu, C, max_size, head=dd.capacity_of(max_size) - 700)
        bufs = [gpu.DeviceBuffer.from_host(r) for r in rows]
        out = gpu.DeviceBuffer((C, n))
        for at in range(0, m, piece):
            k = min(piece, m - at)
            cut.bank.process(out.ptr + 4 * at, *[b.ptr + 4 * at for b in bufs], k, out_stride=n, in_stride=n, delay_stride=n, fgain_stride=n,
                             fdelay_stride=n)
        got = out.download()[:, :m]
        assert np.array_equal(dd.bits(got), dd.bits(want[:, :m])), piece
        if m == n:
            for ch in range(C):
                assert dd.same(cut.bank.read_line(ch), whole.refs[ch].line, whole.refs[ch].made), (piece, ch)
                assert cut.bank.get_state(ch)["head"] == whole.refs[ch].head
        cut.close()
    whole.close()


@pytest.mark.gpu
@pytest.mark.parametrize("alias", ["in", "delay", "fgain", "fdelay"])
@pytest.mark.parametrize("max_size", [1000, 40000])
def test_out_may_be_any_input(gpu, alias, max_size):
    C, n = 3, 2500
    rows = make_rows(C, n, max_size, 41)
    p = Pair(gpu, C, max_size, head=50)
    bufs = [gpu.DeviceBuffer.from_host(r) for r in rows]
    out = bufs[("in", "delay", "fgain", "fdelay").index(alias)]
    p.bank.process(out, *bufs, n)
    want = np.array([r.process(*[row[ch] for row in rows]) for ch, r in enumerate(p.refs)])
    p.check(out.download(), want, alias)
    p.close()


@pytest.mark.gpu
def test_strides_that_are_no_multiple_of_four_and_offset_rows(gpu):
    C, n, max_size = 5, 1100, 1000
    rows = make_rows(C, n, max_size, 42)
    strides, offsets = (n + 1, n + 3, n + 7, n + 2, n + 5), (1, 3, 2, 5, 7)
    wide = []
    for r, s, o in zip((np.zeros((C, n), f32),) + rows, strides, offsets):
        w = np.full(C * s + o, np.nan, f32)
        for ch in range(C):
            w[o + ch * s:o + ch * s + n] = r[ch]
        wide.append(gpu.DeviceBuffer.from_host(w))
    p = Pair(gpu, C, max_size, head=dd.capacity_of(max_size) - 700)
    p.bank.process(*[b.ptr + 4 * o for b, o in zip(wide, offsets)], n, out_stride=strides[0], in_stride=strides[1], delay_stride=strides[2],
                   fgain_stride=strides[3], fdelay_stride=strides[4])
    raw = wide[0].download()
    got = np.array([raw[offsets[0] + ch * strides[0]:offsets[0] + ch * strides[0] + n] for ch in range(C)])
    want = np.array([r.process(*[row[ch] for row in rows]) for ch, r in enumerate(p.refs)])
    p.check(got, want)
    between = np.ones(raw.size, bool)
    for ch in range(C):
        between[offsets[0] + ch * strides[0]:offsets[0] + ch * strides[0] + n] = False
    assert np.isnan(raw[between]).all(), "the call wrote between its rows"
    p.close()


@pytest.mark.gpu
@pytest.mark.parametrize("max_size", [1000, 40000])
def test_inf_nan_subnormal_and_negative_zero_rows(gpu, max_size):
    C, n = 6, 1300
    x, d, g, fd = make_rows(C, n, max_size, 43, kinds=("echo", "fdelay 7", "chorus"))
    s = gen.signals()
    pad = lambda r: np.resize(r, n).astype(f32)                                     # noqa: E731
    x[0], g[1], x[2], g[2] = pad(s["special"]), pad(s["special"]), pad(s["sub"]), np.roll(pad(s["sub"]), 5)
    g[3] = np.resize(np.array([0.0, -0.0, 1.0, np.inf, -np.inf, 1e-40, np.nan, 2.5], f32), n)
    x[4], fd[4], d[4] = -np.abs(x[4]), 0.0, 3.0                                       # -x + -x * -0 and the like
    g[4] = np.where(np.arange(n) % 2 == 0, 0.0, -0.0)
    x[5] = np.where(np.arange(n) % 3 == 0, -0.0, 0.0)
    p = Pair(gpu, C, max_size, head=dd.capacity_of(max_size) - 300, fill=False)
    old = np.concatenate([s["special"], s["sub"], np.where(np.arange(64) % 2 == 0, -0.0, 0.0).astype(f32)])
    for ch, r in enumerate(p.refs):                                 # and the same in the lines: the long delays read it first
        r.line[:] = np.resize(np.roll(old, 7 * ch), r.capacity)
        p.bank.write_line(ch, r.line)
    got = p.run((x, d, g, fd))
    assert np.isnan(got).any() and np.isinf(got).any() and (dd.bits(got) == 0x80000000).any()
    p.close()


@pytest.mark.gpu
@pytest.mark.parametrize("max_size", [1000, 40000])
def test_nan_and_out_of_range_delays_are_what_the_bank_defines(gpu, max_size):
    """A NaN delay is 0, a delay beyond every integer is max_size, a NaN fdelay is 0: against the restatement only."""
    C, n = 2, 1100
    x, d, g, fd = make_rows(C, n, max_size, 44, kinds=("echo", "chorus"))
    odd = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, 3e9, 9.3e18, -0.0, 2147483648.0, 4294967296.0, -2147483904.0], f32)
    d[0, ::3] = np.resize(odd, d[0, ::3].size)
    fd[0, ::5] = np.resize(odd, fd[0, ::5].size)
    fd[1, ::2] = np.nan
    d[1, 1::7] = np.nan
    shift, tail, feed = dd.indices(0, dd.capacity_of(max_size), max_size, odd, odd)
    assert shift.tolist() == [0, max_size, 0, max_size, 0, max_size, max_size, 0, max_size, max_size, 0]
    p = Pair(gpu, C, max_size, head=dd.capacity_of(max_size) - 500)
    p.run((x, d, g, fd))
    p.close()


@pytest.mark.gpu
def test_the_head_beyond_2_23_and_a_fractional_feedback_delay(gpu):
    """One channel, a line longer than 2^23 floats, the head set beyond 2^23: tail + fdelay is a float32 sum there."""
    n = 1500
    rng = np.random.default_rng(45)
    x, g = (rng.standard_normal((1, n)) * 0.5).astype(f32), rng.uniform(-0.9, 0.9, (1, n)).astype(f32)
    d = np.full((1, n), 40.0, f32)
    fd = np.resize(np.array([2.75, 3.5, 0.5, 7.75, 1.25, 2.5], f32), n)[None]
    p = Pair(gpu, 1, BIG, fill=False)
    head = (1 << 23) + 1500
    p.refs[0].head = head
    p.bank.set_state(0, head)
    assert p.bank.get(0) == {"max_delay": BIG, "capacity": dd.capacity_of(BIG), "head": head}
    shift, tail, feed = dd.indices(head, p.refs[0].capacity, BIG, d[0], fd[0])
    assert np.count_nonzero(feed != tail + fd[0].astype(np.int64)) > n // 3
    got, want = p.process((x, d, g, fd))
    assert np.array_equal(dd.bits(got), dd.bits(want)) and p.bank.get_state(0)["head"] == head + n          # (no NaN in these rows)
    at = head - 100
    assert np.array_equal(dd.bits(p.bank.read_line(0, at, n + 200)), dd.bits(p.refs[0].line[at:at + n + 200]))
    p.close()


@pytest.mark.gpu
def test_a_feed_index_that_rounds_past_the_head(gpu):
    """Beyond 2^24 the float32 sum lands on even cells only: a feed one past the head, where the next input overwrites it.  Such
    stretches are walked as the reference's loop stands; the stretches around them are not."""
    n = 2500
    rng = np.random.default_rng(46)
    x, g = (rng.standard_normal((1, n)) * 0.5).astype(f32), rng.uniform(-0.9, 0.9, (1, n)).astype(f32)
    d = np.full((1, n), float(BIG), f32)
    d[0, 1024:2048] = 1000.0                                        # a stretch without, short enough for LDS
    fd = d.copy()
    p = Pair(gpu, 1, BIG, fill=False)
    head, cap = (1 << 23) - 2000, dd.capacity_of(BIG)
    p.refs[0].head = head
    p.bank.set_state(0, head)
    shift, tail, feed = dd.indices(head, cap, BIG, d[0], fd[0])
    ahead = (feed - (head + np.arange(n)) % cap) % cap == 1
    assert np.count_nonzero(ahead[:1024]) > 100 and np.count_nonzero(ahead[2048:]) > 50 and not ahead[1024:2048].any()
    p.bank.count_steps(True)
    got, want = p.process((x, d, g, fd))
    assert np.array_equal(dd.bits(got), dd.bits(want)) and p.bank.get_state(0)["head"] == head + n
    assert p.bank.steps() == (1024, n)
    for at, k in ((head - 10, n + 20), (0, 4096), (cap - 4096, 4096)):
        assert np.array_equal(dd.bits(p.bank.read_line(0, at, k)), dd.bits(p.refs[0].line[at:at + k])), at
    p.close()


@pytest.mark.gpu
def test_copy_and_clear(gpu):
    """copy between lines of equal and unequal length, within a bank and between banks, from a wrapped source; clear."""
    C, n = 3, 900
    small, large = Pair(gpu, C, 1000, head=dd.capacity_of(1000) - 250), Pair(gpu, C, 40000, head=dd.capacity_of(40000) - 250)
    small.run(make_rows(C, n, 1000, 51))
    large.run(make_rows(C, n, 40000, 52))
    for dst, i, src, j in ((small, 0, small, 1), (large, 0, small, 2), (small, 2, large, 1), (large, 2, large, 1)):
        dst.bank.copy(i, src.bank, j)
        dst.refs[i].copy(src.refs[j])
    with pytest.raises(gpu.MiError) as e:
        small.bank.copy(1, small.bank, 1)
    assert e.value.code == EINVAL
    small.run(make_rows(C, n, 1000, 53), "after copy")
    large.run(make_rows(C, n, 40000, 54), "after copy")
    for p in (small, large):
        p.bank.clear()
        for r in p.refs:
            r.clear()
        p.check(np.zeros((C, 0), f32), np.zeros((C, 0), f32), "cleared")
    small.run(make_rows(C, n, 1000, 55), "after clear")
    small.close()
    large.close()


@pytest.mark.gpu
@pytest.mark.parametrize("max_size", [1000, 40000])
def test_the_serial_and_the_parallel_path_alone_give_the_same_bits(gpu, monkeypatch, max_size):
    """MI_DSPU_TEST_PATH=dyndelay_serial: lane 0 walks every step; dyndelay_parallel: every step runs in a run, however short."""
    C, n = 5, 2500
    rows = make_rows(C, n, max_size, 61)
    outs, shares = {}, {}
    for path in ("", "dyndelay_serial", "dyndelay_parallel"):
        if path:
            monkeypatch.setenv("MI_DSPU_TEST_PATH", path)
        else:
            monkeypatch.delenv("MI_DSPU_TEST_PATH", raising=False)
        p = Pair(gpu, C, max_size, head=dd.capacity_of(max_size) - 700)
        p.bank.count_steps(True)
        outs[path] = p.run(rows, path)
        shares[path] = p.bank.steps()
        p.close()
    monkeypatch.delenv("MI_DSPU_TEST_PATH", raising=False)
    assert shares["dyndelay_serial"] == (0, C * n) and shares["dyndelay_parallel"] == (C * n, C * n)
    assert 0 < shares[""][0] < C * n                                # the rows have both kinds of runs
    assert np.array_equal(dd.bits(outs["dyndelay_serial"]), dd.bits(outs["dyndelay_parallel"]))


# ---- streams, capture, lifetime, arguments -------------------------------------------------------------------------------

def _stream(gpu):
    st = ctypes.c_void_p()
    gpu.check(gpu.lib.mi_dspu_stream_create(ctypes.byref(st)))
    return st


@pytest.mark.gpu
def test_two_banks_on_two_streams_and_destroy_with_work_in_flight(gpu):
    C, n, calls = 4, 700, 3
    streams = [_stream(gpu) for _ in range(2)]
    pairs = [Pair(gpu, C, 1000, head=1500), Pair(gpu, C, 40000, head=41000)]
    rows = [make_rows(C, calls * n, 1000, 71), make_rows(C, calls * n, 40000, 72)]
    bufs = [[gpu.DeviceBuffer.from_host(r) for r in rs] for rs in rows]
    outs = [gpu.DeviceBuffer((C, calls * n)) for _ in range(2)]
    s = dict(out_stride=calls * n, in_stride=calls * n, delay_stride=calls * n, fgain_stride=calls * n, fdelay_stride=calls * n)
    for k in range(calls):
        for i in range(2):
            pairs[i].bank.process(outs[i].ptr + 4 * k * n, *[b.ptr + 4 * k * n for b in bufs[i]], n, stream=streams[i].value, **s)
    for i in range(2):
        got = outs[i].download(stream=streams[i].value)
        want = np.array([r.process(*[row[ch] for row in rows[i]]) for ch, r in enumerate(pairs[i].refs)])
        pairs[i].check(got, want, i)
    for k in range(calls):
        for i in range(2):
            pairs[i].bank.process(outs[i], *bufs[i], n, stream=streams[i].value, **s)
    for p in pairs:
        p.close()                                                   # right behind their last launches
    for st in streams:
        gpu.check(gpu.lib.mi_dspu_stream_synchronize(st))
        gpu.check(gpu.lib.mi_dspu_stream_destroy(st))
    again = Pair(gpu, C, 1000, head=1500)
    again.run(make_rows(C, n, 1000, 73))
    again.close()


BAD_ARGS = r'''
import ctypes, importlib, sys
import numpy as np
sys.path.insert(0, %r)
gpu = importlib.import_module("lsp-dsp-units_amd")
capi = importlib.import_module("lsp-dsp-units_amd.capi")
C, n = 3, 64
bad, calls = [], 0
ones, nil = gpu.DeviceBuffer.from_host(np.ones((C, n), np.float32)), gpu.DeviceBuffer.from_host(np.zeros((C, n), np.float32))
def works(b):
    out = gpu.DeviceBuffer((C, n))
    b.process(out, ones, nil, ones, nil, n)
    return np.array_equal(out.download(), np.full((C, n), 2.0, np.float32))       # no delay and a gain of one: in + in
for name, (res, args) in sorted(capi.PROTOTYPES.items()):
    if not name.startswith("mi_dyndelay_bank_") or name.endswith(("_create", "_destroy")):
        continue
    b = gpu.DynamicDelayBank(C, 0)
    print("CALL", name, flush=True)
    zeros = [ctypes.c_void_p(b.handle.value)]
    for a in args[1:]:
        zeros.append(0 if a in (ctypes.c_int, ctypes.c_uint32, ctypes.c_size_t) else None)
    code = getattr(capi.lib, name)(*zeros)
    calls += 1
    if code > 0:
        bad.append((name, code))
    if getattr(capi.lib, name)(None, *zeros[1:]) >= 0:
        bad.append((name, "NULL bank"))
    sizes = [i for i, a in enumerate(args[1:]) if a is ctypes.c_size_t]
    if name.endswith(("_process", "_read_line", "_write_line")):    # a count, and NULL buffers
        zeros[1 + (sizes[0] if name.endswith("_process") else sizes[1])] = 64
        code = getattr(capi.lib, name)(*zeros)
        if code >= 0 or not capi.lib.mi_dspu_last_error().decode().startswith(name):
            bad.append((name, "NULL buffers", code))
    if args[1:2] == [ctypes.c_uint32]:                              # a channel out of range
        zeros[1] = C
        code = getattr(capi.lib, name)(*zeros)
        if code >= 0 or not capi.lib.mi_dspu_last_error().decode().startswith(name):
            bad.append((name, "channel", code))
    if not works(b):
        bad.append((name, "the bank no longer works"))
    b.close()
b = gpu.DynamicDelayBank(C, 1000)
p, h = ctypes.c_void_p(ones.ptr), b.handle
fn = lambda o, i, d, g, f, *r: capi.lib.mi_dyndelay_bank_process(h, o, i, d, g, f, *r, None)
for code, what in ((fn(None, None, None, None, None, 0, 0, 0, 0, 0, 0), "nothing to do"),):
    if code != 0:
        bad.append(("process", what, code))
for code, what in ((fn(p, p, p, p, None, n, n, n, n, n, n), "a row missing"), (fn(None, p, p, p, p, n, n, n, n, n, n), "no out"),
                   (fn(p, p, p, p, p, n, n - 1, n, n, n, n), "a stride shorter than the count"),
                   (fn(p, p, p, p, p, n, n, n, n, n, n - 1), "a stride shorter than the count"),
                   (fn(p, p, p, p, p, n, n, n + 4, n, n, n), "in place with different strides"),
                   (fn(p, p, p, p, p, 1 << 31, 1 << 31, 1 << 31, 1 << 31, 1 << 31, 1 << 31), "count"),
                   (capi.lib.mi_dyndelay_bank_set_state(h, 0, ctypes.byref(capi.DynDelayState(b.capacity)), None), "a head outside the line"),
                   (capi.lib.mi_dyndelay_bank_read_line(h, 0, p, b.capacity - 3, 4, None), "a stretch outside the line"),
                   (capi.lib.mi_dyndelay_bank_write_line(h, 0, p, b.capacity + 1, 0, None), "a stretch outside the line"),
                   (capi.lib.mi_dyndelay_bank_steps(h, ctypes.byref(ctypes.c_uint64()), ctypes.byref(ctypes.c_uint64()), None), "not counting")):
    if code >= 0:
        bad.append(("refused", what, code))
if not np.all(ones.download() == 1.0):
    bad.append("a refused call wrote")
if not works(b):
    bad.append("the bank no longer works")
hh = ctypes.c_void_p()
for channels, size in ((0, 10), (1 << 21, 10), (1, 1 << 24)):
    code = capi.lib.mi_dyndelay_bank_create(ctypes.byref(hh), channels, size)
    if code >= 0 or hh.value:
        bad.append(("create", channels, size, code))
print("DONE", calls, bad, flush=True)
sys.exit(1 if bad or calls != 10 else 0)
'''


@pytest.mark.gpu
def test_zero_and_null_arguments_on_a_live_bank_in_a_child_process(gpu):
    r = subprocess.run([sys.executable, "-c", BAD_ARGS % ROOT], capture_output=True, text=True, timeout=240)
    calls = [ln.split()[1] for ln in r.stdout.splitlines() if ln.startswith("CALL")]
    assert r.returncode == 0 and "DONE" in r.stdout, "last call: %s\n%s\n%s" % (calls[-1] if calls else None, r.stdout[-1500:], r.stderr[-2500:])


@pytest.mark.gpu
@pytest.mark.parametrize("max_size", [1000, 40000])
def test_capture_of_a_steady_process_and_its_replay(gpu, max_size):
    """The head lives on the device: a captured call moves on with every replay, as eager calls on a twin do; get_state, set_state,
    read_line and write_line are refused on a capturing stream."""
    C, n = 5, 1300
    st = _stream(gpu)
    rows = make_rows(C, n, max_size, 81)
    bufs = [gpu.DeviceBuffer.from_host(r) for r in rows]
    out, direct = gpu.DeviceBuffer((C, n)), gpu.DeviceBuffer((C, n))
    p, twin = Pair(gpu, C, max_size, head=dd.capacity_of(max_size) - 700), Pair(gpu, C, max_size, head=dd.capacity_of(max_size) - 700)
    gpu.check(gpu.lib.mi_dspu_graph_begin_capture(st))
    for refused in (lambda: p.bank.get_state(0, stream=st.value), lambda: p.bank.set_state(0, 5, stream=st.value),
                    lambda: p.bank.read_line(0, 0, 4, stream=st.value), lambda: p.bank.write_line(0, np.zeros(4, f32), stream=st.value),
                    lambda: p.bank.count_steps(True, stream=st.value)):
        with pytest.raises(gpu.MiError) as e:
            refused()
        assert e.value.code == ESTATE
    p.bank.process(out, *bufs, n, stream=st.value)
    exe = ctypes.c_void_p()
    gpu.check(gpu.lib.mi_dspu_graph_end_capture(st, ctypes.byref(exe)))
    assert exe.value
    for rep in range(3):
        gpu.check(gpu.lib.mi_dspu_graph_launch(exe, st))
        twin.bank.process(direct, *bufs, n, stream=st.value)
        want = np.array([r.process(*[row[ch] for row in rows]) for ch, r in enumerate(p.refs)])
        got = out.download(stream=st.value)
        assert np.array_equal(dd.bits(got), dd.bits(direct.download(stream=st.value))), rep
        assert np.array_equal(dd.bits(got), dd.bits(want)), rep
    p.check(got, want, "after three replays")
    gpu.lib.mi_dspu_graph_destroy(exe)
    p.close()
    twin.close()
    gpu.check(gpu.lib.mi_dspu_stream_destroy(st))


@pytest.mark.gpu
def test_forty_create_use_destroy_cycles_return_device_memory(gpu):
    hip = ctypes.CDLL("libamdhip64.so")

    def free_bytes():
        free, total = ctypes.c_size_t(), ctypes.c_size_t()
        assert hip.hipDeviceSynchronize() == 0 and hip.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) == 0
        return free.value

    C, n = 4, 300
    rows = make_rows(C, n, 40000, 91)
    bufs = [gpu.DeviceBuffer.from_host(r) for r in rows]
    out = gpu.DeviceBuffer((C, n))

    def cycle():
        b, other = gpu.DynamicDelayBank(C, 40000), gpu.DynamicDelayBank(1, 1000)
        b.count_steps(True)
        b.process(out, *bufs, n)
        other.copy(0, b, 1)
        got = out.download()
        b.close()
        other.close()
        return got

    first = cycle()
    before = free_bytes()
    for _ in range(40):
        assert np.array_equal(dd.bits(cycle()), dd.bits(first))
    assert before - free_bytes() < (4 << 20), "device memory does not come back: %d bytes" % (before - free_bytes())


# ---- the reference's recorded cases: through the C-ABI and through the C++ class ---------------------------------------------

def _ring_part(bank, head):
    if bank.capacity <= dd.RING_WHOLE:
        return bank.read_line(0)
    lo = head - dd.RING_BEHIND
    if lo >= 0:
        return bank.read_line(0, lo, dd.RING_BEHIND)
    return np.concatenate([bank.read_line(0, bank.capacity + lo, -lo), bank.read_line(0, 0, head)])


_RESTATED = {}


def _restated(case):
    """The restatement of a recorded case, for which of its values are sums (computed once, shared by the two tests below)."""
    if case["name"] not in _RESTATED:
        _RESTATED[case["name"]] = dd.run_case(case)
    return _RESTATED[case["name"]]


@pytest.mark.gpu
def test_every_recorded_reference_case_through_the_c_abi(gpu):
    """tests/golden/dyndelay_ref_vectors.npz, operation by operation, through two banks of one channel: out, the heads and the lines
    are the reference's."""
    cases = gen.load()
    assert len(cases) >= 60
    for c in cases:
        a, b = gpu.DynamicDelayBank(1, c["max_size"]), gpu.DynamicDelayBank(1, c["other_size"])
        n = c["rows"].shape[1]
        bufs = [gpu.DeviceBuffer.from_host(np.ascontiguousarray(r)) for r in c["rows"]]
        out, at = gpu.DeviceBuffer.from_host(np.zeros(n, f32)), 0
        for what, arg in c["ops"].tolist():
            if what in (dd.P_A, dd.P_B):
                (a if what == dd.P_A else b).process(out.ptr + 4 * at, *[r.ptr + 4 * at for r in bufs], arg)
                at += arg
            elif what == dd.CLEAR_A:
                a.clear()
            elif what == dd.COPY_A_FROM_B:
                a.copy(0, b, 0)
            elif what == dd.COPY_B_FROM_A:
                b.copy(0, a, 0)
            else:
                (a if what == dd.SET_HEAD_A else b).set_state(0, arg)
        _, ra, rb, made = _restated(c)
        assert dd.same(out.download(), c["out"], made), c["name"]
        heads = [a.get_state(0)["head"], b.get(0)["head"]]
        assert heads == [int(v) for v in c["head"]], c["name"]
        assert dd.same(_ring_part(a, heads[0]), c["ring_a"], dd.ring_part(ra.made, ra.head)), c["name"]
        assert dd.same(_ring_part(b, heads[1]), c["ring_b"], dd.ring_part(rb.made, rb.head)), c["name"]
        a.close()
        b.close()


@pytest.mark.gpu
def test_every_recorded_reference_case_through_the_cpp_class(gpu, tmp_path):
    """The program that recorded the cases from the reference's class, compiled against this library's class instead."""
    src, exe = str(tmp_path / "driver.cpp"), str(tmp_path / "driver")
    open(src, "w").write(gen.DRIVER)
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-DLINE_ON_DEVICE", "-I" + os.path.join(PKG, "include"), "-I" + os.path.join(ROOT, "include"),
                           src, "-o", exe, "-L" + PKG, "-lmi_dspu", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    cases = gen.load()
    got = gen.run(exe, cases, str(tmp_path))
    for c, g in zip(cases, got):
        _, ra, rb, made = _restated(c)
        assert np.array_equal(g["head"], c["head"]), c["name"]
        for k, m in (("out", made), ("ring_a", dd.ring_part(ra.made, ra.head)), ("ring_b", dd.ring_part(rb.made, rb.head))):
            assert dd.same(g[k], c[k], m), (c["name"], k)
    keys = subprocess.check_output([exe, "keys"]).decode().split("\n")
    assert keys[0].split() == ["sizeof", "32"]
    assert keys[1].split() == ["swap", "3000", str(dd.capacity_of(3000)), "5", str(dd.capacity_of(5))]
    assert keys[2].split() == ["dyndelay", "vDelay", "nHead", "nCapacity", "nMaxDelay", "pData"]


@pytest.mark.gpu
@pytest.mark.parametrize("max_size", [1000, 40000])
def test_full_size_every_channel(gpu, max_size):
    """1024 x 4096; eight kinds of channels (the five kinds of rows, three of them twice with other samples), every channel held to
    its kind's restatement."""
    C, n, K = 1024, 4096, 8
    x, d, g, fd = make_rows(K, n, max_size, 95)
    tile = lambda r: np.ascontiguousarray(np.tile(r, (C // K, 1)))                   # noqa: E731
    bank = gpu.DynamicDelayBank(C, max_size)
    refs = [dd.DynamicDelay(max_size) for _ in range(K)]
    for ch in range(C):
        bank.set_state(ch, bank.capacity - 700)
    for r in refs:
        r.head = r.capacity - 700
    out = gpu.DeviceBuffer((C, n))
    bank.process(out, *[gpu.DeviceBuffer.from_host(tile(r)) for r in (x, d, g, fd)], n)
    got = out.download()
    want = np.array([r.process(x[k], d[k], g[k], fd[k]) for k, r in enumerate(refs)])
    assert np.array_equal(dd.bits(got), dd.bits(tile(want)))        # (no NaN in these rows)
    for ch in range(0, C, 41):
        assert bank.get_state(ch)["head"] == refs[ch % K].head
        assert np.array_equal(dd.bits(bank.read_line(ch)), dd.bits(refs[ch % K].line)), ch
    bank.close()
