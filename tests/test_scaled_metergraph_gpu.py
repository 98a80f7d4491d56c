"""mi_scaled_metergraph_bank on the device against tests/scaled_metergraph_ref.py, bit for bit in every word of both rings, both
heads and both samplers' fCurrent, nCount and nPeriod: every recorded case, 1, 3 and 70 channels with a method, subsampling, period
and frame count each over the counts around every vector and workgroup boundary (subsamplings and periods on either side of 64,
256 and 1024, where the kernel changes how it reduces a chunk; frame counts on either side of the workgroup's 256 lanes, which is
all that the re-decimation's lane-per-frame fold changes at), calls in which some channels re-decimate and others do not, both
rings overrun inside one call, odd strides and row bases off the 16-byte grid, guard words around read() and level(), gains NULL
and given, a stream of its own, a captured graph that appends at every replay and re-decimates at one, destroy with work in
flight, every misuse code, and the C++ class over the recorded cases."""
import ctypes

import numpy as np
import pytest

import scaled_metergraph_ref as M
import test_scaled_metergraph_host as H
import test_scaled_metergraph_class_host as CH

gen = H.gen
f32, u32 = np.float32, np.uint32
EINVAL, ESTATE = -1, -5
COUNTS = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4099)
SUBS = (1, 3, 4, 32, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025)
FRAMES = (1, 2, 16, 333, 255, 256, 257)
GUARD = f32(-1234.5)
GAP = M.FRAMES_GAP


def same(a, b):
    return np.array_equal(np.asarray(a).view(u32), np.asarray(b).view(u32))


def state_words(bank, ch, stream=None):
    """The bank's channel in the layout of ScaledMeterGraph.state_words()."""
    s, p = bank.get_state(ch, stream), bank.get_params(ch)
    tail = [s["history_head"], s["frames_head"], np.array(s["history_current"], f32).view(u32), s["history_count"], p["subsampling"],
            np.array(s["frames_current"], f32).view(u32), s["frames_count"], s["frames_period"], p["period"]]
    return np.concatenate([s["history"].view(u32), s["ring"].view(u32), np.array(tail, u32)])


def geometry(k):
    """Channel k's frames, subsampling and max_period: every subsampling with a max_period of 1 .. 4 times it and a little."""
    sub = SUBS[k % len(SUBS)]
    return FRAMES[(k // 2) % len(FRAMES)], sub, sub * (1 + k % 4) + (k % 3 if k % 4 else 0)


def period_of(k, step):
    """The period that channel k asks for at step `step`: its subsampling, its maximum and two in between (one no multiple)."""
    _, sub, maxp = geometry(k)
    return (sub, maxp, (sub + maxp) // 2, min(sub + 1, maxp))[(k + step) % 4]


class Unit:
    """A bank and the restatement's graphs: channel ch has method (ch + first) % 6 (5: no such method) and geometry(ch + first)."""

    def __init__(self, gpu, channels, first=0):
        self.gpu, self.channels, self.first = gpu, channels, first
        geo = [geometry(ch + first) for ch in range(channels)]
        self.bank = gpu.ScaledMeterGraphBank(channels, max(g[0] for g in geo), max(M.subframes(*g) for g in geo))
        self.refs = []
        for ch, (fr, sub, maxp) in enumerate(geo):
            self.bank.init(ch, fr, sub, maxp)
            self.bank.set_method(ch, (ch + first) % 6)
            g = M.ScaledMeterGraph(fr, sub, maxp)
            g.set_method((ch + first) % 6)
            self.refs.append(g)
        self.periods(0)

    def periods(self, step, only=None):
        for ch, g in enumerate(self.refs):
            if only is None or ch in only:
                self.bank.set_period(ch, period_of(ch + self.first, step))
                g.set_period(period_of(ch + self.first, step))

    def process(self, x, gains=None):
        for ch, g in enumerate(self.refs):
            g.process(x[ch], None if gains is None else gains[ch])

    def check(self, what="", stream=None):
        for ch, g in enumerate(self.refs):
            got, want = state_words(self.bank, ch, stream), g.state_words()
            assert np.array_equal(got, want), (what, ch, g.method, g.history.period, g.period, g.frames.frames, np.flatnonzero(got != want)[:4])

    def close(self):
        self.bank.close()


def rows(channels, n, seed):
    """Random rows; every other channel has few magnitudes (ties in every frame), every fifth the special values in front."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((channels, n)).astype(f32)
    x[1::2] = (rng.integers(-3, 4, (len(x[1::2]), n)) * 0.25).astype(f32)
    k = min(n, 80)
    x[::5, :k] = H.X[gen.ROW_SPECIAL, :k]
    x[3::7, :k] = H.X[gen.ROW_NAN, :k]
    x[4::9, :k] = H.X[gen.ROW_SENTINEL, :k]
    return x


def staged(gpu, x, stride, lead, stream=None):
    """x in a device buffer with rows `stride` apart that start `lead` floats in: (buffer, address of row 0)."""
    flat = np.full(lead + x.shape[0] * stride + 8, GUARD, f32)
    for ch in range(x.shape[0]):
        flat[lead + ch * stride:lead + ch * stride + x.shape[1]] = x[ch]
    buf = gpu.DeviceBuffer.from_host(flat, stream)
    return buf, buf.ptr + 4 * lead


# ---- every recorded case ------------------------------------------------------------------------------------------------------
CHUNK = 32


@pytest.fixture(scope="module")
def xdev(gpu):
    buf = gpu.DeviceBuffer.from_host(H.X)
    gains = gpu.DeviceBuffer.from_host(np.array([1.0, 0.5, -2.0, 0.0], f32))
    yield buf, gains
    buf.free(), gains.free()


@pytest.mark.gpu
@pytest.mark.parametrize("part", range((len(H.CASES) + CHUNK - 1) // CHUNK))
def test_every_recorded_case(gpu, xdev, part):
    xbuf, gains = xdev
    n_row = H.X.shape[1]
    gain_at = {1.0: 0, 0.5: 1, -2.0: 2, 0.0: 3}
    for c in H.CASES[part * CHUNK:(part + 1) * CHUNK]:
        bank = gpu.ScaledMeterGraphBank(1, c["frames"], M.subframes(c["frames"], c["subsampling"], c["max_period"]))
        bank.init(0, c["frames"], c["subsampling"], c["max_period"])
        guards = np.full(c["frames"] + 16, GUARD, f32)
        out = gpu.DeviceBuffer.from_host(guards)
        answers = []
        period_set = False
        for k, (code, row, off, n, value) in enumerate(c["ops"]):
            code, n = int(code), int(n)
            src = xbuf.ptr + 4 * (int(row) * n_row + int(off))
            if code == M.SET_METHOD:
                bank.set_method(0, n)
            elif code == M.SET_PERIOD:
                bank.set_period(0, n)
                period_set = True
            elif code == M.FILL:
                bank.fill(value, 0)
            elif code == M.PROCESS:
                bank.process(src, n)
            elif code == M.PROCESS_GAIN:
                bank.process(src, n, gains=gains.ptr + 4 * gain_at[float(value)])
            elif code == M.PROCESS_SINGLE:
                for i in range(n):
                    bank.process_value(src + 4 * i)
            elif code in (M.READ, M.LEVEL):
                assert period_set, c["name"]                        # no recorded case reads before set_period()
                out.upload(guards)
                if code == M.READ:
                    bank.read(out, n)
                    took = min(n, c["frames"])
                else:
                    bank.level(out)
                    took = 1
                got = out.download()
                assert (got[took:] == GUARD).all()
                answers.append(got[:took].view(u32))
            got = state_words(bank, 0)
            assert np.array_equal(got, c["state"][k]), (c["name"], k, c["ops"][k], np.flatnonzero(got != c["state"][k])[:4])
        assert np.array_equal(np.concatenate(answers) if answers else np.zeros(0, u32), c["answers"]), c["name"]
        out.free()
        bank.close()


# ---- shapes ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("channels", (1, 3, 70))
def test_channels_counts_periods_and_frames(gpu, channels):
    """One stream per bank: a call of every count in turn, gains NULL and given alternately, rows an odd stride apart that start
    off the 16-byte grid; the state of every channel after every call.  Before every third call every channel asks for another
    period, before the others every third channel does: calls in which some channels re-decimate and others do not."""
    for first in ((0, 5, 9) if channels == 1 else (channels,)):
        u = Unit(gpu, channels, first=first)
        rng = np.random.default_rng(channels)
        gains = rng.choice(np.array([1.0, 0.5, -2.0, 0.0, 3.0], f32), channels).astype(f32)
        gbuf = gpu.DeviceBuffer.from_host(gains)
        for k, n in enumerate(COUNTS + (4099, 1025)):
            if k % 3 == 2:
                u.periods(k)
            else:
                u.periods(k, only=range(k % 3, channels, 3))
            x = rows(channels, n, 100 * channels + k)
            stride = n + (k % 3) * 2 + 1
            buf, src = staged(gpu, x, stride, 1 + k % 4)
            given = k % 2 == 1
            u.bank.process(src, n, gains=gbuf if given else None, stride=stride)
            u.process(x, gains if given else None)
            u.check((first, k, n))
            buf.free()
        gbuf.free()
        u.close()


@pytest.mark.gpu
@pytest.mark.parametrize("sub", (63, 64, 65, 255, 256, 257, 1023, 1024, 1025))
def test_every_threshold_in_both_samplers(gpu, sub):
    """Four channels of one subsampling with 1, 2, 16 and 257 frames: the history sampler at `sub`, the frames sampler at `sub` and
    at sub + 1, then at 2 * sub; every count; the five methods in turn from call to call."""
    frames = (1, 2, 16, 257)
    bank = gpu.ScaledMeterGraphBank(4, 257, 2 * 257)
    refs = []
    for ch, fr in enumerate(frames):
        bank.init(ch, fr, sub, 2 * sub)
        refs.append(M.ScaledMeterGraph(fr, sub, 2 * sub))
    for k, n in enumerate(COUNTS):
        for ch, g in enumerate(refs):
            period = sub + (ch % 2) if k < 8 else 2 * sub
            bank.set_method(ch, (k + ch) % 5), bank.set_period(ch, period)
            g.set_method((k + ch) % 5), g.set_period(period)
        x = rows(4, n, 7 * sub + k)
        buf, src = staged(gpu, x, n + 3, 3)
        bank.process(src, n, stride=n + 3)
        for ch, g in enumerate(refs):
            g.process(x[ch])
            assert np.array_equal(state_words(bank, ch), g.state_words()), (sub, n, ch)
        buf.free()
    bank.close()


@pytest.mark.gpu
def test_both_rings_overrun_in_one_call(gpu):
    """A subsampling and a period of 1 or 2 with 1 or 2 frames and 4099 samples: thousands of words for rings of 17 .. 20.  The
    last stores must win, whichever lane makes them; three calls, so that the heads move on from odd places; then a new period."""
    channels = 70
    bank = gpu.ScaledMeterGraphBank(channels, 2, 4)
    refs = []
    for ch in range(channels):
        fr, sub = (2 if ch % 3 else 1), 1 + (ch % 2)
        bank.init(ch, fr, sub, 2)
        bank.set_method(ch, ch % 5), bank.set_period(ch, sub)
        g = M.ScaledMeterGraph(fr, sub, 2)
        g.set_method(ch % 5), g.set_period(sub)
        refs.append(g)
    for k, n in enumerate((4099, 4099, 4098, 4099)):
        if k == 3:
            for ch, g in enumerate(refs):
                bank.set_period(ch, 2), g.set_period(2)
        x = rows(channels, n, 900 + k)
        buf, src = staged(gpu, x, n + 1, 1)
        bank.process(src, n, stride=n + 1)
        for ch, g in enumerate(refs):
            g.process(x[ch])
            assert np.array_equal(state_words(bank, ch), g.state_words()), (k, ch)
        buf.free()
    bank.close()


# ---- layout -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_read_and_level_write_their_rows_and_nothing_else(gpu):
    u = Unit(gpu, 7, first=1)
    x = rows(7, 1025, 5)
    buf, src = staged(gpu, x, 1027, 2)
    for rep in range(2):
        u.bank.process(src, 1025, stride=1027)
        u.process(x)
        for count in (0, 1, 2, 16, 21, 333, 338):
            for stride, lead in ((count + 3, 1), (count + 4, 4)):
                flat = np.full(lead + 7 * stride + 9, GUARD, f32)
                dst = gpu.DeviceBuffer.from_host(flat)
                u.bank.read(dst.ptr + 4 * lead, count, stride=stride)
                got = dst.download()
                want = flat.copy()
                for ch, g in enumerate(u.refs):
                    r = g.read(count)
                    want[lead + ch * stride:lead + ch * stride + len(r)] = r
                assert same(got, want), (rep, count, stride)
                dst.free()
        lv = gpu.DeviceBuffer.from_host(np.full(7 + 10, GUARD, f32))
        u.bank.level(lv.ptr + 4 * 3)
        want = np.full(17, GUARD, f32)
        want[3:10] = [g.level() for g in u.refs]
        assert same(lv.download(), want)
        lv.free()
        u.periods(1)
    u.check()
    buf.free()
    u.close()


@pytest.mark.gpu
def test_setters_fill_and_state_round_trip(gpu):
    """fill() leaves heads and fCurrent; set_state() hands over both rings; init() starts over and keeps the method."""
    u = Unit(gpu, 3, first=2)
    x = rows(3, 333, 8)
    buf = gpu.DeviceBuffer.from_host(x)
    u.bank.process(buf, 333)
    u.process(x)
    u.bank.fill(0.75, 1)
    u.refs[1].fill(0.75)
    u.bank.fill(-0.5)
    for g in u.refs:
        g.fill(-0.5)
    u.bank.fill(0.125, 1)                                           # the later one of two pending fills
    u.refs[1].fill(0.125)
    u.check("fill")
    g = u.refs[0]
    p = u.bank.get_params(0)
    assert p == {"method": g.method, "period": g.period, "max_period": g.max_period, "subsampling": g.history.period, "frames": g.frames.frames,
                 "subframes": g.history.frames}
    # a state made by hand: the words go round, and the next call goes on from them (a period of its own: a re-decimation)
    hist = (np.arange(len(g.history.buffer.data), dtype=f32) * f32(0.25) - f32(3.5)).astype(f32)
    ring = (np.arange(len(g.frames.buffer.data), dtype=f32) - f32(2.0)).astype(f32)
    st = {"history_current": -0.0, "history_count": g.history.period - 1, "history_head": len(hist) - 1, "frames_current": 2.5,
          "frames_count": 0, "frames_head": len(ring) - 1, "frames_period": g.history.period}
    u.bank.set_state(0, st, hist, ring)
    back = u.bank.get_state(0)
    assert same(back["history"], hist) and same(back["ring"], ring) and all(back[k] == v for k, v in st.items() if not k.endswith("current"))
    assert same(back["history_current"], f32(-0.0)) and same(back["frames_current"], f32(2.5))
    g.history.buffer.data[:], g.history.buffer.head, g.history.current, g.history.count = hist, len(hist) - 1, f32(-0.0), g.history.period - 1
    g.frames.buffer.data[:], g.frames.buffer.head, g.frames.current, g.frames.count, g.frames.period = ring, len(ring) - 1, f32(2.5), 0, g.history.period
    for rep in range(2):
        u.bank.process(buf, 333)
        u.process(x)
        u.check("set_state %d" % rep)
    u.bank.init(2, 5, 3, 7)
    u.bank.set_period(2, 6)
    keep = u.refs[2].method
    u.refs[2] = M.ScaledMeterGraph(5, 3, 7)
    u.refs[2].set_method(keep)                                      # init() keeps enMethod
    u.refs[2].set_period(6)
    u.bank.process(buf, 10, stride=333)
    for ch, g in enumerate(u.refs):
        g.process(x[ch, :10])
    u.check("init")
    buf.free()
    u.close()


# ---- streams and graphs -----------------------------------------------------------------------------------------------------------
def _stream(gpu):
    st = ctypes.c_void_p()
    gpu.check(gpu.lib.mi_dspu_stream_create(ctypes.byref(st)))
    return st


@pytest.mark.gpu
def test_a_stream_of_its_own(gpu):
    st = _stream(gpu)
    u = Unit(gpu, 3, first=4)
    for k, n in enumerate((1025, 65, 4099)):
        u.periods(k)
        x = rows(3, n, 40 + k)
        buf, src = staged(gpu, x, n + 1, 1, st.value)
        u.bank.process(src, n, stride=n + 1, stream=st.value)
        u.process(x)
        u.check(k, st.value)
        gpu.check(gpu.lib.mi_dspu_stream_synchronize(st))
        buf.free()
    u.close()
    gpu.check(gpu.lib.mi_dspu_stream_destroy(st))


@pytest.mark.gpu
def test_captured_process_and_read_replay(gpu):
    """The kernel keeps both samplers and decides on the device whether to re-decimate: a replayed graph goes on where the last
    launch stopped, re-decimates at the replay where sFrames.nPeriod differs from the captured target, and at no other."""
    n, stride, count = 1025, 1028, 21
    st = _stream(gpu)
    u = Unit(gpu, 3, first=3)
    x = rows(3, n, 77)
    buf, src = staged(gpu, x, stride, 0, st.value)
    gains = gpu.DeviceBuffer.from_host(np.array([0.5, -2.0, 1.0], f32), st.value)
    out = gpu.DeviceBuffer.from_host(np.full((3, count + 3), GUARD, f32), st.value)
    lv = gpu.DeviceBuffer.from_host(np.full(3, GUARD, f32), st.value)
    u.bank.process(src, n, stride=stride, stream=st.value)         # the first call of a graph re-decimates: have it behind
    u.process(x)
    u.periods(1)                                                    # ... and ask for other periods
    # pending settings are refused inside a capture
    gpu.check(gpu.lib.mi_dspu_graph_begin_capture(st))
    with pytest.raises(gpu.MiError) as e:
        u.bank.process(src, n, stride=stride, stream=st.value)
    assert e.value.code == ESTATE
    exe = ctypes.c_void_p()
    gpu.check(gpu.lib.mi_dspu_graph_end_capture(st, ctypes.byref(exe)))
    gpu.lib.mi_dspu_graph_destroy(exe)
    u.bank.update_settings(st.value)
    gpu.check(gpu.lib.mi_dspu_graph_begin_capture(st))
    u.bank.process(src, n, gains=gains, stride=stride, stream=st.value)
    u.bank.process_value(src, stream=st.value)                      # the first three floats of row 0: a sample per channel
    u.bank.read(out, count, stride=count + 3, stream=st.value)
    u.bank.level(lv, stream=st.value)
    gpu.check(gpu.lib.mi_dspu_graph_end_capture(st, ctypes.byref(exe)))
    assert exe.value
    for rep in range(3):
        before = [g.frames.period for g in u.refs]
        gpu.check(gpu.lib.mi_dspu_graph_launch(exe, st))
        got, levels = out.download(st.value), lv.download(st.value)
        for ch, g in enumerate(u.refs):
            g.process(x[ch], [0.5, -2.0, 1.0][ch])
            g.process_single(x[0, ch])
            r = g.read(count)
            assert same(got[ch, :len(r)], r) and (got[ch, len(r):] == GUARD).all(), (rep, ch)
            assert same(levels[ch], g.level()), (rep, ch)
            assert rep == 0 or before[ch] == g.period, (rep, ch)               # the periods differ at the first replay only
        assert rep != 0 or any(b != g.period for b, g in zip(before, u.refs))
        u.check(rep, st.value)
    gpu.lib.mi_dspu_graph_destroy(exe)
    for b in (buf, gains, out, lv):
        b.free()
    u.close()
    gpu.check(gpu.lib.mi_dspu_stream_destroy(st))


# ---- lifetime and misuse ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_destroy_with_work_in_flight(gpu):
    n = 4099
    st = _stream(gpu)
    u = Unit(gpu, 3)
    x = rows(3, n, 3)
    buf = gpu.DeviceBuffer.from_host(x, st.value)
    out = gpu.DeviceBuffer.from_host(np.zeros((3, 16), f32), st.value)
    u.bank.update_settings(st.value)
    for _ in range(4):
        u.bank.process(buf, n, stream=st.value)
        u.bank.read(out, 16, stream=st.value)
    for _ in range(4):
        u.process(x)
    want = np.zeros((3, 16), f32)
    for ch, g in enumerate(u.refs):
        r = g.read(16)
        want[ch, :len(r)] = r
    u.close()                                                       # right behind the last launch
    gpu.check(gpu.lib.mi_dspu_stream_synchronize(st))
    assert same(out.download(), want)
    gpu.check(gpu.lib.mi_dspu_stream_destroy(st))
    again = Unit(gpu, 3)
    again.bank.process(buf, 257, stride=n)
    for ch, g in enumerate(again.refs):
        g.process(x[ch, :257])
    again.check()
    again.close()
    buf.free(), out.free()


@pytest.mark.gpu
def test_misuse(gpu):
    lib = gpu.lib
    u = Unit(gpu, 3)
    u.bank.close()                                                  # a bank of known sizes: 16 frames of 4 .. 16 samples, 64 + 16 and 16 + 16 words
    u.bank = gpu.ScaledMeterGraphBank(3, 16, 64)
    u.refs = [M.ScaledMeterGraph(16, 4, 16) for _ in range(3)]
    for ch, g in enumerate(u.refs):
        u.bank.init(ch, 16, 4, 16), u.bank.set_method(ch, ch), u.bank.set_period(ch, 8)
        g.set_method(ch), g.set_period(8)
    h = u.bank.handle
    ones = gpu.DeviceBuffer.from_host(np.ones((3, 64), f32))
    p = ctypes.c_void_p(ones.ptr)
    st8 = ctypes.c_void_p()
    from importlib import import_module
    capi = import_module("lsp-dsp-units_amd.capi")
    state = capi.ScaledMeterGraphState()
    params = capi.ScaledMeterGraphParams()
    pre = "mi_scaled_metergraph_bank_"
    fn = {n[len(pre):]: getattr(lib, n) for n in capi.PROTOTYPES if n.startswith(pre)}
    assert len(fn) == 14
    bad = capi.ScaledMeterGraphState
    for code, what in ((fn["init"](h, 0, 16, 0, 64), "subsampling 0: the reference divides by it"),
                       (fn["init"](h, 0, 0, 4, 64), "no frames"),
                       (fn["init"](h, 0, 16, 8, 7), "max_period below the subsampling"),
                       (fn["init"](h, 0, 17, 4, 64), "frames above max_frames"),
                       (fn["init"](h, 0, 16, 1, 64), "more sub-frames than max_subframes"),
                       (fn["init"](h, 0, 16, 1 << 20, 1 << 28), "frames * max_period beyond 31 bits"),
                       (fn["init"](h, 3, 16, 4, 64), "channel"),
                       (fn["set_method"](h, 3, 0), "channel"), (fn["set_period"](h, 3, 5), "channel"), (fn["fill"](h, 3, 0.0), "channel"),
                       (fn["get_params"](h, 3, ctypes.byref(params)), "channel"), (fn["get_params"](h, 0, None), "no result"),
                       (fn["get_state"](h, 3, ctypes.byref(state), None, None, None), "channel"),
                       (fn["get_state"](h, 0, None, None, None, None), "no result"),
                       (fn["set_state"](h, 3, ctypes.byref(state), None, None, None), "channel"),
                       (fn["set_state"](h, 0, None, None, None, None), "no state"),
                       (fn["set_state"](h, 0, ctypes.byref(bad(0.0, 0, 64 + 16, 0.0, 0, 0, 0)), None, None, None), "history head outside its ring"),
                       (fn["set_state"](h, 0, ctypes.byref(bad(0.0, 0, 0, 0.0, 0, 16 + 16, 0)), None, None, None), "frames head outside its ring"),
                       (fn["set_state"](h, 0, ctypes.byref(bad(0.0, 4, 0, 0.0, 0, 0, 0)), None, None, None), "sHistory.nCount not below its period"),
                       (fn["set_state"](h, 0, ctypes.byref(bad(0.0, 0, 0, 0.0, 8, 0, 8)), None, None, None), "sFrames.nCount not below its period"),
                       (fn["set_state"](h, 0, ctypes.byref(bad(0.0, 0, 0, 0.0, 0, 0, 17)), None, None, None), "sFrames.nPeriod above max_period"),
                       (fn["set_state"](h, 0, ctypes.byref(bad(0.0, 0, 0, 0.0, 0, 0, 3)), None, None, None), "sFrames.nPeriod below the subsampling"),
                       (fn["process"](h, None, None, 64, 64, None), "no src"),
                       (fn["process"](h, p, None, 64, 63, None), "a stride shorter than the count"),
                       (fn["process"](h, p, None, 1 << 31, 1 << 31, None), "count"),
                       (fn["process_value"](h, None, None), "no values"),
                       (fn["read"](h, None, 16, 16, None), "no dst"),
                       (fn["read"](h, p, 16, 15, None), "a stride shorter than the count"),
                       (fn["level"](h, None, None), "no levels"),
                       (fn["create"](None, 3, 16, 64), "no result"),
                       (fn["create"](ctypes.byref(st8), 0, 16, 64), "no channels"),
                       (fn["create"](ctypes.byref(st8), 3, 0, 64), "no frames"),
                       (fn["create"](ctypes.byref(st8), 3, 16, 15), "fewer sub-frames than frames"),
                       (fn["create"](ctypes.byref(st8), 3, (1 << 20) + 1, 1 << 21), "too many frames"),
                       (fn["create"](ctypes.byref(st8), 3, 16, (1 << 24) + 1), "too many sub-frames")):
        assert code == EINVAL, (what, code)
        assert lib.mi_dspu_last_error().decode().startswith("mi_scaled_metergraph_"), (what, lib.mi_dspu_last_error())
    assert st8.value is None
    assert (ones.download() == 1.0).all(), "a refused call wrote"
    # the refusals changed nothing: the bank runs as it was set up; counts of 0 do nothing
    assert fn["process"](h, None, None, 0, 0, None) == 0 and fn["read"](h, None, 0, 0, None) == 0
    u.bank.process(ones, 64)
    for g in u.refs:
        g.process(np.ones(64, f32))
    u.check()
    # a channel without rings, and one with rings but no period yet (the reference's process() would never return)
    fresh = gpu.ScaledMeterGraphBank(2, 4, 16)
    with pytest.raises(gpu.MiError) as e:
        fresh.set_period(0, 5)                                      # before init() there is nothing to limit the period to
    assert e.value.code == ESTATE
    for step in range(2):
        for entry in (lambda: fresh.process(ones, 8, stride=64), lambda: fresh.process_value(ones), lambda: fresh.read(ones, 4, stride=64),
                      lambda: fresh.level(ones)):
            with pytest.raises(gpu.MiError) as e:
                entry()
            assert e.value.code == ESTATE, step
        fresh.init(0, 4, 2, 8), fresh.init(1, 4, 2, 8)
        fresh.set_period(0, 4)                                      # channel 1 still has none
    assert (ones.download() == 1.0).all()
    fresh.set_period(1, 4)
    fresh.process(ones, 8, stride=64)
    fresh.close()
    for entry in (lambda: fn["process"](None, p, None, 64, 64, None), lambda: fn["process_value"](None, p, None),
                  lambda: fn["read"](None, p, 16, 16, None), lambda: fn["level"](None, p, None),
                  lambda: fn["init"](None, 0, 16, 4, 64), lambda: fn["set_method"](None, 0, 0),
                  lambda: fn["set_period"](None, 0, 5), lambda: fn["fill"](None, 0, 0.0),
                  lambda: fn["update_settings"](None, None), lambda: fn["get_params"](None, 0, ctypes.byref(params)),
                  lambda: fn["get_state"](None, 0, ctypes.byref(state), None, None, None),
                  lambda: fn["set_state"](None, 0, ctypes.byref(state), None, None, None)):
        assert entry() == ESTATE
    # get_state and set_state synchronise: not on a stream that is being captured; neither do pending setters pass there
    st = _stream(gpu)
    gpu.check(gpu.lib.mi_dspu_graph_begin_capture(st))
    assert fn["get_state"](h, 0, ctypes.byref(state), None, None, st) == ESTATE
    assert fn["set_state"](h, 0, ctypes.byref(state), None, None, st) == ESTATE
    u.bank.set_method(0, 3)
    assert fn["update_settings"](h, st) == ESTATE and fn["level"](h, p, st) == ESTATE and fn["process"](h, p, None, 64, 64, st) == ESTATE
    exe = ctypes.c_void_p()
    gpu.check(gpu.lib.mi_dspu_graph_end_capture(st, ctypes.byref(exe)))
    gpu.lib.mi_dspu_graph_destroy(exe)
    gpu.check(gpu.lib.mi_dspu_stream_destroy(st))
    u.close()
    with pytest.raises(gpu.MiError) as e:
        u.bank.process(ones, 64)
    assert e.value.code == ESTATE
    u.close()                                                       # twice is fine
    assert fn["destroy"](None) == 0
    ones.free()


# ---- the class ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("part", range(4))
def test_the_cpp_class_over_the_recorded_cases(gpu, tmp_path, part):
    """tests/cpp/scaled_metergraph_layout.cpp with the generator's protocol: lsp::dspu::ScaledMeterGraph of this library on every
    recorded case, every word of both host rings and of the object's state."""
    exe = CH.compile_program(str(tmp_path / "scaled_metergraph_layout"))
    cases = H.CASES[part::4]
    got = gen.run(exe, H.X, cases, str(tmp_path))
    for c, r in zip(cases, got):
        bad = np.argwhere(r["state"] != c["state"])
        assert bad.size == 0, (c["name"], "operation %d, word %d of %d" % (bad[0][0], bad[0][1], c["state"].shape[1]), c["ops"][bad[0][0]])
        assert np.array_equal(r["answers"], c["answers"]), c["name"]
