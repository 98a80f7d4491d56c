"""mi_metergraph_bank on the device against tests/metergraph_ref.py, bit for bit in every ring word, fCurrent, nCount and nHead:
every recorded case, 1, 3 and 70 channels with a method, period and frame count each over the counts around every vector and
workgroup boundary, the ring overrun inside one call, odd strides and row bases off the 16-byte grid, guard words around read() and
level(), gains NULL and given, a stream of its own, a captured graph that appends at every replay, destroy with work in flight,
every misuse code, and the C++ class over the recorded cases."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import metergraph_ref as M
import test_metergraph_host as H
import test_metergraph_class_host as CH

gen = H.gen
f32, u32 = np.float32, np.uint32
EINVAL, ESTATE = -1, -5
COUNTS = (1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1025, 4099)
PERIODS = (1, 2, 3, 7, 64, 100, 257, 4099, 5000)
FRAMES = (1, 2, 16, 333)
GUARD = f32(-1234.5)


def same(a, b):
    return np.array_equal(np.asarray(a).view(u32), np.asarray(b).view(u32))


def state_words(bank, ch, stream=None):
    s = bank.get_state(ch, stream)
    return np.concatenate([s["ring"].view(u32), np.array([s["head"], np.array(s["current"], f32).view(u32), s["count"]], u32)])


class Unit:
    """A bank and the restatement's graphs: channel ch has method (ch + first) % 6 (5: no such method), a period and a frame count
    that move through PERIODS and FRAMES at different paces, and a default of its own."""

    def __init__(self, gpu, channels, first=0, periods=PERIODS, frames=FRAMES):
        self.gpu, self.channels = gpu, channels
        self.bank = gpu.MeterGraphBank(channels, max(frames))
        self.refs = []
        for ch in range(channels):
            k = ch + first
            fr, pe, de = frames[(k // 2) % len(frames)], periods[k % len(periods)], f32(0.25 * (k % 5) - 0.5)
            self.bank.init(ch, fr, pe, de)
            self.bank.set_method(ch, k % 6)
            g = M.MeterGraph(fr, pe, de)
            g.set_method(k % 6)
            self.refs.append(g)

    def check(self, what="", stream=None):
        for ch, g in enumerate(self.refs):
            got, want = state_words(self.bank, ch, stream), g.state_words()
            assert np.array_equal(got, want), (what, ch, g.method, g.period, len(g.buffer.data), np.flatnonzero(got != want)[:4])

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
    return x


def staged(gpu, x, stride, lead, stream=None):
    """x in a device buffer with rows `stride` apart that start `lead` floats in: (buffer, address of row 0)."""
    flat = np.full(lead + x.shape[0] * stride + 8, GUARD, f32)
    for ch in range(x.shape[0]):
        flat[lead + ch * stride:lead + ch * stride + x.shape[1]] = x[ch]
    buf = gpu.DeviceBuffer.from_host(flat, stream)
    return buf, buf.ptr + 4 * lead


# ---- every recorded case ------------------------------------------------------------------------------------------------------
CHUNK = 27


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
        bank = gpu.MeterGraphBank(1, c["frames"])
        bank.init(0, c["frames"], c["period"], c["default"])
        guards = np.full(c["frames"] + 16, GUARD, f32)
        out = gpu.DeviceBuffer.from_host(guards)
        answers = []
        for k, (code, row, off, n, value) in enumerate(c["ops"]):
            code, n = int(code), int(n)
            src = xbuf.ptr + 4 * (int(row) * n_row + int(off))
            if code == M.SET_METHOD:
                bank.set_method(0, n)
            elif code == M.SET_PERIOD:
                bank.set_period(0, n)
            elif code == M.SET_DEFAULT:
                bank.set_default_value(0, value)
            elif code == M.FILL:
                bank.fill(value, 0)
            elif code == M.CLEAR:
                bank.clear(0)
            elif code == M.PROCESS:
                bank.process(src, n)
            elif code == M.PROCESS_GAIN:
                bank.process(src, n, gains=gains.ptr + 4 * gain_at[float(value)])
            elif code == M.PROCESS_SINGLE:
                for i in range(n):
                    bank.process_value(src + 4 * i)
            elif code == M.READ:
                out.upload(guards)
                bank.read(out, n)
                got = out.download()
                assert (got[n:] == GUARD).all()
                answers.append(got[:n].view(u32))
            elif code == M.LEVEL:
                out.upload(guards)
                bank.level(out)
                got = out.download()
                assert (got[1:] == GUARD).all()
                answers.append(got[:1].view(u32))
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
    off the 16-byte grid; the state of every channel after every call.  Over the three banks every period meets every count."""
    for first in ((0, 5) if channels == 1 else (channels,)):
        u = Unit(gpu, channels, first=first)
        rng = np.random.default_rng(channels)
        gains = rng.choice(np.array([1.0, 0.5, -2.0, 0.0, 3.0], f32), channels).astype(f32)
        gbuf = gpu.DeviceBuffer.from_host(gains)
        for k, n in enumerate(COUNTS + COUNTS[::-1][:4]):
            x = rows(channels, n, 100 * channels + k)
            stride = n + (k % 3) * 2 + 1
            buf, src = staged(gpu, x, stride, 1 + k % 4)
            given = k % 2 == 1
            u.bank.process(src, n, gains=gbuf if given else None, stride=stride)
            for ch, g in enumerate(u.refs):
                g.process(x[ch], gains[ch] if given else None)
            u.check((first, k, n))
            buf.free()
        gbuf.free()
        u.close()


@pytest.mark.gpu
@pytest.mark.parametrize("period", PERIODS)
def test_every_period_against_every_count_and_frame_count(gpu, period):
    """Four channels of one period with 1, 2, 16 and 333 frames, the five methods in turn from call to call."""
    bank = gpu.MeterGraphBank(4, 333)
    refs = []
    for ch, fr in enumerate(FRAMES):
        bank.init(ch, fr, period, 0.5)
        refs.append(M.MeterGraph(fr, period, 0.5))
    for k, n in enumerate(COUNTS):
        for ch, g in enumerate(refs):
            bank.set_method(ch, (k + ch) % 5)
            g.set_method((k + ch) % 5)
        x = rows(4, n, 7 * period + k)
        buf, src = staged(gpu, x, n + 3, 3)
        bank.process(src, n, stride=n + 3)
        for ch, g in enumerate(refs):
            g.process(x[ch])
            assert np.array_equal(state_words(bank, ch), g.state_words()), (period, n, ch)
        buf.free()
    bank.close()


@pytest.mark.gpu
def test_ring_overrun_in_one_call(gpu):
    """Period 1 with 2 frames and 4099 samples: 4099 frames for 2 slots.  The last stores must win, whichever lane makes them;
    three calls, so that the head moves on from an odd place."""
    channels = 70
    bank = gpu.MeterGraphBank(channels, 2)
    refs = []
    for ch in range(channels):
        bank.init(ch, 2 if ch % 3 else 1, 1 + (ch % 2), -1.0)
        bank.set_method(ch, ch % 5)
        g = M.MeterGraph(2 if ch % 3 else 1, 1 + (ch % 2), -1.0)
        g.set_method(ch % 5)
        refs.append(g)
    for k, n in enumerate((4099, 4099, 4098)):
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
    u = Unit(gpu, 7, first=1, periods=(1, 2, 3, 7))
    x = rows(7, 1025, 5)
    buf, src = staged(gpu, x, 1027, 2)
    for rep in range(2):
        u.bank.process(src, 1025, stride=1027)
        for ch, g in enumerate(u.refs):
            g.process(x[ch])
        for count in (0, 1, 2, 16, 21, 333, 338):
            for stride, lead in ((count + 3, 1), (count + 4, 4)):
                flat = np.full(lead + 7 * stride + 9, GUARD, f32)
                dst = gpu.DeviceBuffer.from_host(flat)
                u.bank.read(dst.ptr + 4 * lead, count, stride=stride)
                got = dst.download()
                want = flat.copy()
                for ch, g in enumerate(u.refs):
                    want[lead + ch * stride:lead + ch * stride + count] = g.read(count)
                assert same(got, want), (rep, count, stride)
                dst.free()
        lv = gpu.DeviceBuffer.from_host(np.full(7 + 10, GUARD, f32))
        u.bank.level(lv.ptr + 4 * 3)
        want = np.full(17, GUARD, f32)
        want[3:10] = [g.level() for g in u.refs]
        assert same(lv.download(), want)
        lv.free()
    u.check()
    buf.free()
    u.close()


@pytest.mark.gpu
def test_setters_fill_and_state_round_trip(gpu):
    """fill() and clear() reset the head and leave fCurrent and nCount; set_state() hands over a ring; init() starts over."""
    u = Unit(gpu, 3, first=2, periods=(7, 64, 100), frames=(16,))
    x = rows(3, 333, 8)
    buf = gpu.DeviceBuffer.from_host(x)
    u.bank.process(buf, 333)
    for ch, g in enumerate(u.refs):
        g.process(x[ch])
    u.bank.fill(0.75, 1)
    u.refs[1].fill(0.75)
    u.bank.set_default_value(2, 9.0)
    u.refs[2].set_default_value(9.0)
    u.bank.clear()
    for g in u.refs:
        g.clear()
    u.bank.fill(0.125, 1)                                           # the later one of two pending fills
    u.refs[1].fill(0.125)
    u.check("fill and clear")
    assert u.bank.get_params(2) == {"method": u.refs[2].method, "period": u.refs[2].period, "frames": 16, "default_value": f32(9.0)}
    ring = np.arange(16, dtype=f32) - f32(3.5)
    u.bank.set_state(0, -0.0, 5, 11, ring)
    g = u.refs[0]
    g.buffer.data[:], g.buffer.head, g.current, g.count = ring, 11, f32(-0.0), 5
    u.bank.set_state(1, 4.0, u.refs[1].period, 15)                  # nCount == nPeriod by hand: a frame first; the ring stays
    u.refs[1].current, u.refs[1].count, u.refs[1].buffer.head = f32(4.0), u.refs[1].period, 15
    u.bank.process(buf, 333)
    for ch, g in enumerate(u.refs):
        g.process(x[ch])
    u.check("set_state")
    u.bank.init(2, 5, 3, -2.0)
    u.refs[2] = M.MeterGraph(5, 3, -2.0)
    u.refs[2].set_method(4)                                         # init() keeps enMethod
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
        x = rows(3, n, 40 + k)
        buf, src = staged(gpu, x, n + 1, 1, st.value)
        u.bank.process(src, n, stride=n + 1, stream=st.value)
        for ch, g in enumerate(u.refs):
            g.process(x[ch])
            s = u.bank.get_state(ch, st.value)
            assert same(s["ring"], g.buffer.data) and s["head"] == g.buffer.head and s["count"] == g.count, (k, ch)
        gpu.check(gpu.lib.mi_dspu_stream_synchronize(st))
        buf.free()
    u.close()
    gpu.check(gpu.lib.mi_dspu_stream_destroy(st))


@pytest.mark.gpu
def test_captured_process_and_read_append_at_every_replay(gpu):
    """The kernel keeps fCurrent, nCount and nHead on the device, so a replayed graph goes on where the last launch stopped."""
    n, stride, count = 1025, 1028, 21
    st = _stream(gpu)
    u = Unit(gpu, 3, first=3, periods=(7, 64, 100), frames=(16, 2))
    x = rows(3, n, 77)
    buf, src = staged(gpu, x, stride, 0, st.value)
    gains = gpu.DeviceBuffer.from_host(np.array([0.5, -2.0, 1.0], f32), st.value)
    out = gpu.DeviceBuffer.from_host(np.full((3, count + 3), GUARD, f32), st.value)
    lv = gpu.DeviceBuffer.from_host(np.full(3, GUARD, f32), st.value)
    u.bank.set_period(1, 5)
    u.refs[1].set_period(5)
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
    for rep in range(2):
        gpu.check(gpu.lib.mi_dspu_graph_launch(exe, st))
        got, levels = out.download(st.value), lv.download(st.value)
        for ch, g in enumerate(u.refs):
            g.process(x[ch], [0.5, -2.0, 1.0][ch])
            g.process_single(x[0, ch])
            assert same(got[ch, :count], g.read(count)) and (got[ch, count:] == GUARD).all(), (rep, ch)
            assert same(levels[ch], g.level()), (rep, ch)
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
    out = gpu.DeviceBuffer((3, 16))
    u.bank.update_settings(st.value)
    for _ in range(4):
        u.bank.process(buf, n, stream=st.value)
        u.bank.read(out, 16, stream=st.value)
    for ch, g in enumerate(u.refs):
        for _ in range(4):
            g.process(x[ch])
    want = np.stack([g.read(16) for g in u.refs])
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
    u = Unit(gpu, 3, frames=(16,))
    h = u.bank.handle
    ones = gpu.DeviceBuffer.from_host(np.ones((3, 64), f32))
    p = ctypes.c_void_p(ones.ptr)
    st8 = ctypes.c_void_p()
    from importlib import import_module
    capi = import_module("lsp-dsp-units_amd.capi")
    state = capi.MeterGraphState(0.0, 0, 0)
    params = capi.MeterGraphParams()
    for code, what in ((lib.mi_metergraph_bank_set_period(h, 0, 0), "period 0"),
                       (lib.mi_metergraph_bank_set_period(h, 0, 1 << 32), "a period beyond 32 bits"),
                       (lib.mi_metergraph_bank_init(h, 0, 16, 0, 0.0), "period 0"),
                       (lib.mi_metergraph_bank_init(h, 0, 17, 5, 0.0), "frames above max_frames"),
                       (lib.mi_metergraph_bank_init(h, 0, 0, 5, 0.0), "no frames"),
                       (lib.mi_metergraph_bank_init(h, 3, 16, 5, 0.0), "channel"),
                       (lib.mi_metergraph_bank_set_method(h, 3, 0), "channel"), (lib.mi_metergraph_bank_set_period(h, 3, 5), "channel"),
                       (lib.mi_metergraph_bank_set_default_value(h, 3, 0.0), "channel"), (lib.mi_metergraph_bank_fill(h, 3, 0.0), "channel"),
                       (lib.mi_metergraph_bank_clear(h, 3), "channel"),
                       (lib.mi_metergraph_bank_get_params(h, 3, ctypes.byref(params)), "channel"),
                       (lib.mi_metergraph_bank_get_params(h, 0, None), "no result"),
                       (lib.mi_metergraph_bank_get_state(h, 3, ctypes.byref(state), None, None), "channel"),
                       (lib.mi_metergraph_bank_get_state(h, 0, None, None, None), "no result"),
                       (lib.mi_metergraph_bank_set_state(h, 3, ctypes.byref(state), None, None), "channel"),
                       (lib.mi_metergraph_bank_set_state(h, 0, None, None, None), "no state"),
                       (lib.mi_metergraph_bank_set_state(h, 0, ctypes.byref(capi.MeterGraphState(0.0, 0, 16)), None, None), "head outside the ring"),
                       (lib.mi_metergraph_bank_process(h, None, None, 64, 64, None), "no src"),
                       (lib.mi_metergraph_bank_process(h, p, None, 64, 63, None), "a stride shorter than the count"),
                       (lib.mi_metergraph_bank_process(h, p, None, 1 << 31, 1 << 31, None), "count"),
                       (lib.mi_metergraph_bank_process_value(h, None, None), "no values"),
                       (lib.mi_metergraph_bank_read(h, None, 16, 16, None), "no dst"),
                       (lib.mi_metergraph_bank_read(h, p, 16, 15, None), "a stride shorter than the count"),
                       (lib.mi_metergraph_bank_level(h, None, None), "no levels"),
                       (lib.mi_metergraph_bank_create(None, 3, 16), "no result"),
                       (lib.mi_metergraph_bank_create(ctypes.byref(st8), 0, 16), "no channels"),
                       (lib.mi_metergraph_bank_create(ctypes.byref(st8), 3, 0), "no frames"),
                       (lib.mi_metergraph_bank_create(ctypes.byref(st8), 3, (1 << 20) + 1), "too many frames")):
        assert code == EINVAL, (what, code)
        assert lib.mi_dspu_last_error().decode().startswith("mi_metergraph_"), (what, lib.mi_dspu_last_error())
    assert st8.value is None
    assert (ones.download() == 1.0).all(), "a refused call wrote"
    # the refusals changed nothing: the bank runs as it was set up; counts of 0 do nothing
    assert lib.mi_metergraph_bank_process(h, None, None, 0, 0, None) == 0 and lib.mi_metergraph_bank_read(h, None, 0, 0, None) == 0
    u.bank.process(ones, 64)
    for g in u.refs:
        g.process(np.ones(64, f32))
    u.check()
    # a channel without a ring: the bank does not process
    fresh = gpu.MeterGraphBank(2, 4)
    fresh.init(0, 4, 3)
    for entry in (lambda: fresh.process(ones, 8, stride=64), lambda: fresh.process_value(ones), lambda: fresh.read(ones, 4, stride=64),
                  lambda: fresh.level(ones)):
        with pytest.raises(gpu.MiError) as e:
            entry()
        assert e.value.code == ESTATE
    assert (ones.download() == 1.0).all()
    fresh.close()
    for entry in (lambda: lib.mi_metergraph_bank_process(None, p, None, 64, 64, None), lambda: lib.mi_metergraph_bank_process_value(None, p, None),
                  lambda: lib.mi_metergraph_bank_read(None, p, 16, 16, None), lambda: lib.mi_metergraph_bank_level(None, p, None),
                  lambda: lib.mi_metergraph_bank_init(None, 0, 16, 5, 0.0), lambda: lib.mi_metergraph_bank_set_method(None, 0, 0),
                  lambda: lib.mi_metergraph_bank_set_period(None, 0, 5), lambda: lib.mi_metergraph_bank_set_default_value(None, 0, 0.0),
                  lambda: lib.mi_metergraph_bank_fill(None, 0, 0.0), lambda: lib.mi_metergraph_bank_clear(None, 0),
                  lambda: lib.mi_metergraph_bank_update_settings(None, None), lambda: lib.mi_metergraph_bank_get_params(None, 0, ctypes.byref(params)),
                  lambda: lib.mi_metergraph_bank_get_state(None, 0, ctypes.byref(state), None, None),
                  lambda: lib.mi_metergraph_bank_set_state(None, 0, ctypes.byref(state), None, None)):
        assert entry() == ESTATE
    # get_state and set_state synchronise: not on a stream that is being captured
    st = _stream(gpu)
    gpu.check(gpu.lib.mi_dspu_graph_begin_capture(st))
    assert lib.mi_metergraph_bank_get_state(h, 0, ctypes.byref(state), None, st) == ESTATE
    assert lib.mi_metergraph_bank_set_state(h, 0, ctypes.byref(state), None, st) == ESTATE
    u.bank.fill(1.0)
    assert lib.mi_metergraph_bank_update_settings(h, st) == ESTATE and lib.mi_metergraph_bank_level(h, p, st) == ESTATE
    exe = ctypes.c_void_p()
    gpu.check(gpu.lib.mi_dspu_graph_end_capture(st, ctypes.byref(exe)))
    gpu.lib.mi_dspu_graph_destroy(exe)
    gpu.check(gpu.lib.mi_dspu_stream_destroy(st))
    u.close()
    with pytest.raises(gpu.MiError) as e:
        u.bank.process(ones, 64)
    assert e.value.code == ESTATE
    u.close()                                                       # twice is fine
    assert lib.mi_metergraph_bank_destroy(None) == 0
    ones.free()


# ---- the class ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("part", range(4))
def test_the_cpp_class_over_the_recorded_cases(gpu, tmp_path, part):
    """tests/cpp/metergraph_layout.cpp with the generator's protocol: lsp::dspu::MeterGraph of this library on every recorded case.
    This library's RingBuffer reports nHead == capacity where a block ends at the ring's end (its positions are taken modulo the
    capacity): the head is compared modulo the frame count."""
    exe = CH.compile_program(str(tmp_path / "metergraph_layout"))
    cases = H.CASES[part::4]
    got = gen.run(exe, H.X, cases, str(tmp_path))
    for c, r in zip(cases, got):
        fr = c["frames"]
        state = r["state"].copy()
        state[:, fr] %= fr
        bad = np.argwhere(state != c["state"])
        assert bad.size == 0, (c["name"], "operation %d, word %d of %d" % (bad[0][0], bad[0][1], fr + 3), c["ops"][bad[0][0]])
        assert np.array_equal(r["answers"], c["answers"]), c["name"]
