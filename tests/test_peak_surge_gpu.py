"""mi_peakmeter_bank and mi_surge_bank (lsp::dspu::PeakMeter, lsp::dspu::SurgeProtector) on the device against
tests/peak_surge_ref.py: every output sample and every state word bit for bit on every channel (the restatement fed fTau and nHold
from the bank's getter); across tiles, workgroups, every entry point, holds and transition times on both sides of the tile, events
on tile and call edges, split calls, the setters' order, in place, strides, NULL outputs, subnormals, NaN and Inf, graph capture,
two streams, lifetime, bad arguments, the reference's recorded cases and the C++ classes."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import peak_surge_ref as ps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "lsp-dsp-units_amd")
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_peak_surge_vectors as gen  # noqa: E402

T, G = 256, 4                           # tile_chain_device.h: samples of a tile, channels of a workgroup
f32 = np.float32
u32 = np.uint32
SR = 48000
HOLDS = (0, 1, T - 1, T, T + 1, 700)
RELEASES = (5.0, gen.RELEASE_HALF, 0.0, 1.0, gen.RELEASE_STUCK)
TRANSITIONS = (0, 1, T - 1, T + 1, 700)
SHUTDOWNS = (0, 1, 300)
ON, OFF = 0.5, 0.25
COUNTS = [1, T - 1, T, T + 1, 2 * T + 3]
CHANNELS = [1, G - 1, G, G + 1, 2 * G + 1]


def _bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a, f32).view(u32), np.ascontiguousarray(b, f32).view(u32))


def _same(got, want):
    """bit for bit; NaN at the same positions whatever its payload"""
    got, want = np.asarray(got, f32), np.asarray(want, f32)
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(u32)[~nan], want.view(u32)[~nan])


def _f(word):
    return u32(word).view(f32)


# ---- PeakMeter ------------------------------------------------------------------------------------------------------------

def _pm(gpu, settings):
    """A bank with (hold in samples, release in ms) per channel at 48 kHz, and the restatement fed the bank's own fTau and nHold."""
    C = len(settings)
    bank = gpu.PeakMeterBank(C)
    for ch, (hold, release) in enumerate(settings):
        bank.configure(ch, SR, gen.hold_ms(hold), release)
    bank.update_settings()
    params = [bank.get_params(ch) for ch in range(C)]
    assert [p["hold"] for p in params] == [s[0] for s in settings]
    return bank, ps.PeakMeters([p["tau"] for p in params], [p["hold"] for p in params])


def _pm_settings(C, shift=0):
    return [(HOLDS[(ch + shift) % len(HOLDS)], RELEASES[(ch + shift) % len(RELEASES)]) for ch in range(C)]


def _pm_signal(seed, C, n):
    """Quiet noise, a loud sample every 300 or so, a plateau of equal samples, stretches of exact silence of every length up to
    800: bursts, holds and decays fall on tile and call edges in one channel or another."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((C, n)) * 0.05
    for ch in range(C):
        at = int(rng.integers(0, 40))
        while at < n:
            x[ch, at] = rng.choice([-1.0, 1.0]) * (0.3 + rng.random())
            quiet = int(rng.choice([3, 40, T - 2, T, T + 3, 800]))
            x[ch, at + 1 + int(rng.integers(0, 20)):at + 1 + quiet] = 0.0
            at += 2 + quiet + int(rng.integers(0, 60))
        if n > 40:
            p = int(rng.integers(0, n - 30))
            x[ch, p:p + 30] = -np.abs(x[ch, p])                 # s == peak again and again
    return x.astype(f32)


def _pm_state(bank):
    s = [bank.get_state(ch) for ch in range(bank.channels)]
    return np.array([v["peak"] for v in s], f32), np.array([v["counter"] for v in s], np.int64)


def _pm_same_state(bank, ref):
    peak, counter = _pm_state(bank)
    return _same(peak, ref.peak) and np.array_equal(counter, ref.counter)


def _pm_run(gpu, bank, x, entry="process", stream=None):
    """-> (dst or None, peaks)"""
    C, n = x.shape
    dx, peaks = gpu.DeviceBuffer.from_host(x), gpu.DeviceBuffer.from_host(np.full(C, 7.0, f32))
    dst = None
    if entry == "process":
        dst = gpu.DeviceBuffer.from_host(np.full((C, n), 7.0, f32))
    bank.process(dst, dx, n, peaks=peaks, stream=stream)
    return (None if dst is None else dst.download(stream)), peaks.download(stream)


def _pm_check(gpu, bank, ref, x, entry="process", what=""):
    got, peaks = _pm_run(gpu, bank, x, entry)
    want = ref.process(x)
    if got is not None:
        bad = np.argwhere(got.view(u32) != want.view(u32))
        assert _same(got, want), (what, len(bad), bad[:4].tolist())
    assert _same(peaks, want[:, -1]), what
    assert _pm_same_state(bank, ref), (what, _pm_state(bank), ref.peak, ref.counter)
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("C", CHANNELS)
@pytest.mark.parametrize("entry", ["process", "state"])
def test_peakmeter_bit_exact_shapes(gpu, entry, C, count):
    bank, ref = _pm(gpu, _pm_settings(C, C))
    for blk in range(2):                                        # the second call starts from the first one's state
        _pm_check(gpu, bank, ref, _pm_signal(100 * count + 10 * C + blk, C, count), entry, what=blk)
    bank.close()


@pytest.mark.gpu
@pytest.mark.parametrize("C", CHANNELS)
def test_peakmeter_value_bit_exact_shapes(gpu, C):
    """process(value, count): counts of 0, 1, 64 and 300 against holds from 0 to 700 reach its three branches."""
    bank, ref = _pm(gpu, _pm_settings(C, C + 1))
    x = _pm_signal(7 + C, C, 40)
    x[:, 5:9] = 0.0
    peaks, branches = gpu.DeviceBuffer((C,)), set()
    for i in range(x.shape[1]):
        count = (0, 1, 64, 300)[i % 4]
        before, counter = ref.peak.copy(), np.minimum(ref.counter, ref.hold)
        want = ref.process_value(x[:, i], count)
        branches |= set(np.where(np.abs(x[:, i]) >= before, 0, np.where(counter >= count, 1, 2)).tolist())
        bank.process_value(peaks, gpu.DeviceBuffer.from_host(x[:, i]), count)
        assert _same(peaks.download(), want), i
        p = bank.get_params(0)
        assert p["count"] == count and _same([p["factor"]], [ps.value_factor(p["tau"], count)])
    assert _pm_same_state(bank, ref) and (branches == {0, 1, 2} or C < G)
    bank.close()


@pytest.mark.gpu
def test_peakmeter_every_hold_across_tile_and_call_edges(gpu):
    """Every hold with every release, calls of 515, 257 and 1200 samples: a burst two samples before a tile's or a call's end holds
    into the next one, runs out there and decays."""
    settings = [(h, r) for h in HOLDS for r in (5.0, gen.RELEASE_HALF, 0.0)]
    bank, ref = _pm(gpu, settings)
    C = len(settings)
    for blk, n in enumerate((2 * T + 3, T + 1, 1200)):
        x = _pm_signal(70 + blk, C, n)
        for edge in (T, 2 * T, n):
            if edge <= n:
                x[:, edge - 2] = 2.0 + blk
                x[:, edge - 1:edge + 30] = 0.0
        want = _pm_check(gpu, bank, ref, x, what=blk)
        assert np.all(want[:, T - 2] == f32(2.0 + blk))
    bank.close()


@pytest.mark.gpu
def test_peakmeter_calls_of_113_samples_equal_one_long_call(gpu):
    C, n = G + 1, 1972
    settings = _pm_settings(C, 2)
    one, ref = _pm(gpu, settings)
    x = _pm_signal(41, C, n)
    whole = _pm_check(gpu, one, ref, x, what="one call")
    parts, _ = _pm(gpu, settings)
    got = np.concatenate([_pm_run(gpu, parts, np.ascontiguousarray(x[:, p:p + 113]))[0] for p in range(0, n, 113)], axis=1)
    assert _same(got, whole) and _pm_same_state(parts, ref)
    one.close()
    parts.close()


@pytest.mark.gpu
def test_peakmeter_in_place_strides_and_null_dst(gpu):
    C, n = G + 1, 2 * T + 9
    settings = _pm_settings(C, 1)
    x = _pm_signal(91, C, n)
    apart, ref = _pm(gpu, settings)
    want = _pm_check(gpu, apart, ref, x, what="apart")
    apart.close()
    bank, _ = _pm(gpu, settings)
    dx = gpu.DeviceBuffer.from_host(x)
    bank.process(dx, dx, n)                                     # dst == src
    assert _same(dx.download(), want) and _pm_same_state(bank, ref)
    bank.close()
    bank, _ = _pm(gpu, settings)
    dx = gpu.DeviceBuffer.from_host(x)
    bank.process(None, dx, n)                                   # no dst: the same state, the input untouched
    assert _pm_same_state(bank, ref) and np.array_equal(dx.download(), x)
    bank.close()
    k = 300
    for ds, ss in ((301, 303), (304, 312), (k, k + 1)):         # unaligned rows, unequal strides
        bank, ref2 = _pm(gpu, settings)
        pad = lambda v, s, fill: np.concatenate([v, np.full((C, s - v.shape[1]), fill, f32)], axis=1)
        hx = pad(x[:, :k], ss, 3.0)
        dx, do = gpu.DeviceBuffer.from_host(hx), gpu.DeviceBuffer.from_host(np.full((C, ds), 7.0, f32))
        bank.process(do, dx, k, dst_stride=ds, src_stride=ss)
        got = do.download()
        assert _same(got[:, :k], ref2.process(x[:, :k])) and np.all(got[:, k:] == 7.0), "written past count"
        assert np.array_equal(dx.download(), hx) and _pm_same_state(bank, ref2)
        bank.close()


@pytest.mark.gpu
def test_peakmeter_settings_clear_and_set_state_between_calls(gpu):
    C = G + 1
    bank, ref = _pm(gpu, [(700, 5.0)] * C)
    x = _pm_signal(61, C, T + 40)
    x[:, T + 30] = 3.0                                          # the hold of 700 is running when the call ends
    _pm_check(gpu, bank, ref, x, what="before")
    assert np.all(ref.counter == 700 - 9)
    # the hold shortened while the counter runs: the next launch takes the counter down to it, as update_settings() does
    bank.set_hold_time(0, gen.hold_ms(100))
    bank.set_time(1, gen.hold_ms(300), 1.0)
    bank.set_sample_rate(2, 44100)
    bank.set_release_time(3, 0.0)
    params = [bank.get_params(ch) for ch in range(C)]           # as update_settings() will leave them
    assert [p["hold"] for p in params][:2] == [100, 300] and params[3]["tau"] == 0.0
    ref.tau, ref.hold = np.array([p["tau"] for p in params], f32), np.array([p["hold"] for p in params], np.int64)
    assert bank.get_state(0)["counter"] == 691                  # lazy: the state is clamped by the next process()
    _pm_check(gpu, bank, ref, np.zeros((C, 150), f32) + f32(0.01), what="after the setters")
    assert bank.get_state(0)["counter"] == 0 and bank.get_state(1)["counter"] == 150 and bank.get_state(4)["counter"] == 541
    # clear(): at once, one channel and all; set_state after a clear is not undone by it
    bank.clear(1)
    ref.clear(1)
    assert bank.get_state(1) == {"peak": 0.0, "counter": 0} and bank.get_state(4)["peak"] == 3.0
    _pm_check(gpu, bank, ref, _pm_signal(63, C, T + 3), what="after clear(1)")
    bank.clear()
    bank.set_state(2, 0.5, 10 ** 6)                             # a counter above the hold: taken down by the next launch
    ref.clear()
    ref.peak[2], ref.counter[2] = 0.5, 10 ** 6
    assert bank.get_state(2) == {"peak": 0.5, "counter": 10 ** 6}
    _pm_check(gpu, bank, ref, np.zeros((C, 40), f32), what="after clear() and set_state")
    assert bank.get_state(2)["counter"] == ref.hold[2] - 40
    # set_params: tau and the hold as given
    bank.set_params(0, 0.25, 3)
    ref.tau[0], ref.hold[0] = 0.25, 3
    assert bank.get_params(0)["tau"] == 0.25 and bank.get_params(0)["hold"] == 3
    _pm_check(gpu, bank, ref, _pm_signal(64, C, 2 * T), what="after set_params")
    # a hold the reference cannot convert is refused and changes nothing
    bank.set_hold_time(1, 5000.0)                               # 240000 samples at 48 kHz; at 4 GHz they would be 2e10
    before = bank.get_params(1)
    for call in (lambda: bank.set_hold_time(1, -1.0), lambda: bank.set_hold_time(1, float("nan")), lambda: bank.set_time(1, 1e8, 1.0),
                 lambda: bank.set_sample_rate(1, 4000000000)):
        with pytest.raises(gpu.MiError) as e:
            call()
        assert e.value.code == -1
    assert bank.get_params(1) == before
    bank.close()


@pytest.mark.gpu
def test_peakmeter_subnormal_decay_is_kept(gpu):
    """tau just below a half: from 0.05 the peak halves through the subnormals to 0 within one tile; tau just above a half: it
    stays at the smallest subnormal for ever, as 2^-149 * tau rounds back up in the reference."""
    bank, ref = _pm(gpu, [(1, gen.RELEASE_HALF), (0, gen.RELEASE_STUCK), (3, gen.RELEASE_HALF), (0, gen.RELEASE_HALF)])
    x = np.zeros((4, 2 * T + 5), f32)
    x[:, 3] = 0.05
    x[:, 100] = 1e-40                                           # a subnormal sample below a decaying peak ... and above one later
    x[:, 400] = 1e-44
    want = _pm_check(gpu, bank, ref, x, what="subnormal")
    tiny = f32(np.finfo(f32).tiny)
    assert np.all(((want > 0) & (want < tiny)).sum(axis=1) >= 20)
    assert want[0, 250] == 0.0 and want[1, -1].view(u32) == 1 and want[0, 400] == f32(1e-44)
    bank.close()


@pytest.mark.gpu
def test_peakmeter_nan_and_inf(gpu):
    settings = [(40, 1.0), (40, 0.0), (0, 5.0), (T, gen.RELEASE_HALF), (1, 0.0)]
    bank, ref = _pm(gpu, settings)
    C, n = len(settings), 2 * T + 40
    x = _pm_signal(95, C, n)
    x[:, 50], x[:, T - 1], x[:, T + 100], x[:, 2 * T + 1] = np.nan, np.inf, -np.inf, np.nan
    x[:, T:T + 60] = 0.0
    want = _pm_check(gpu, bank, ref, x, what="NaN and Inf")
    assert np.isposinf(want).any() and np.isnan(want[1]).any() and not np.isnan(want[0]).any()   # inf * 0 where tau is 0
    _pm_check(gpu, bank, ref, _pm_signal(96, C, 100), what="after")
    bank.close()


# ---- SurgeProtector -------------------------------------------------------------------------------------------------------

def _sp(gpu, settings):
    """A bank with (transition, shutdown) per channel, thresholds 0.5 and 0.25, and the restatement."""
    C = len(settings)
    bank, ref = gpu.SurgeProtectorBank(C), ps.SurgeProtectors(C)
    for ch, (t, sd) in enumerate(settings):
        bank.configure(ch, t, sd, ON, OFF)
        ref.set_transition_time(ch, t)
        ref.set_shutdown_time(ch, sd)
    ref.on_thr[:], ref.off_thr[:] = ON, OFF
    assert [bank.get_params(ch)["transition_max"] for ch in range(C)] == [s[0] for s in settings]
    return bank, ref


def _sp_settings(C, shift=0):
    return [(TRANSITIONS[(ch + shift) % len(TRANSITIONS)], SHUTDOWNS[(ch + shift) % len(SHUTDOWNS)]) for ch in range(C)]


def _sp_level(seed, C, n):
    """A level that is there (>= ON), gone (< OFF) or in between, in stretches of 1 to 800 samples, with samples exactly on the
    thresholds."""
    rng = np.random.default_rng(seed)
    x = np.empty((C, n))
    for ch in range(C):
        at, there = 0, bool(rng.integers(2))
        while at < n:
            k = int(rng.choice([1, 5, 50, 200, T - 1, T + 1, 400, 800]))
            x[ch, at:at + k] = (0.55 + 0.4 * rng.random(min(k, n - at))) if there else 0.2 * rng.random(min(k, n - at))
            if there and k > 20:
                x[ch, at + 3:at + 8] = 0.3                      # between the thresholds while on
                x[ch, at] = ON
            at, there = at + k, not there
    x[:, n // 2] = OFF
    return x.astype(f32)


def _sp_state(bank):
    s = [bank.get_state(ch) for ch in range(bank.channels)]
    return (np.array([v["gain"] for v in s], f32), np.array([v["transition_time"] for v in s], np.int64),
            np.array([v["shutdown_time"] for v in s], np.int64), np.array([v["on"] for v in s], bool))


def _sp_same_state(bank, ref):
    gain, t, sd, on = _sp_state(bank)
    return _bits_equal(gain, ref.gain) and np.array_equal(t, ref.t) and np.array_equal(sd, ref.sd) and np.array_equal(on, ref.on)


def _sp_audio(C, n):
    return (np.random.default_rng(5).standard_normal((C, n)) * 0.5).astype(f32)


def _sp_run(gpu, bank, level, entry="process", stream=None):
    C, n = level.shape
    dl = gpu.DeviceBuffer.from_host(level)
    if entry == "state":
        bank.process(None, dl, n, stream=stream)
        return None
    out = gpu.DeviceBuffer.from_host(_sp_audio(C, n) if entry == "mul" else np.full((C, n), 7.0, f32))
    (bank.process_mul if entry == "mul" else bank.process)(out, dl, n, stream=stream)
    return out.download(stream)


def _sp_check(gpu, bank, ref, level, entry="process", what=""):
    got = _sp_run(gpu, bank, level, entry)
    want = ref.process(level)
    if entry == "mul":
        want = _sp_audio(*level.shape) * want
    if got is not None:
        bad = np.argwhere(got.view(u32) != want.view(u32))
        assert bad.size == 0, (what, len(bad), bad[:4].tolist())
    assert _sp_same_state(bank, ref), (what, _sp_state(bank), ref.gain, ref.t, ref.sd, ref.on)
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("C", CHANNELS)
@pytest.mark.parametrize("entry", ["process", "state", "mul"])
def test_surge_bit_exact_shapes(gpu, entry, C, count):
    bank, ref = _sp(gpu, _sp_settings(C, C))
    for blk in range(2):
        _sp_check(gpu, bank, ref, _sp_level(100 * count + 10 * C + blk, C, count), entry, what=blk)
    bank.close()


@pytest.mark.gpu
def test_surge_every_transition_across_tile_and_call_edges(gpu):
    """Every transition time with every shutdown time; the level appears two samples before a tile's or a call's end and stops
    two samples before the next one: fades start on one side of an edge and are turned round on the other."""
    settings = [(t, sd) for t in TRANSITIONS for sd in SHUTDOWNS]
    bank, ref = _sp(gpu, settings)
    C = len(settings)
    moved = np.zeros(C, bool)
    for blk, n in enumerate((2 * T + 3, T + 1, 1200)):
        x = _sp_level(70 + blk, C, n)
        x[:, :T - 2] = 0.1
        x[:, T - 2:min(2 * T - 2, n)] = 0.9
        x[:, 2 * T - 2:2 * T + 40] = 0.1
        x[:, n - 2:] = 0.9
        want = _sp_check(gpu, bank, ref, x, what=blk)
        moved |= ((want > 0) & (want < 1)).any(axis=1)
    assert np.array_equal(moved, np.array([t > 1 for t, sd in settings]))
    bank.close()


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ["process", "mul"])
def test_surge_calls_of_113_samples_equal_one_long_call(gpu, entry):
    C, n = G + 1, 1972
    settings = _sp_settings(C, 2)
    one, ref = _sp(gpu, settings)
    x = _sp_level(41, C, n)
    whole = ref.process(x) * (_sp_audio(C, n) if entry == "mul" else f32(1.0))
    got = _sp_run(gpu, one, x, entry)
    assert _bits_equal(got, whole) and _sp_same_state(one, ref)
    parts, _ = _sp(gpu, settings)
    audio = _sp_audio(C, n)
    pieces = []
    for p in range(0, n, 113):
        lv = gpu.DeviceBuffer.from_host(x[:, p:p + 113])
        k = lv.shape[1]
        out = gpu.DeviceBuffer.from_host(audio[:, p:p + k])
        (parts.process_mul if entry == "mul" else parts.process)(out, lv, k)
        pieces.append(out.download())
    assert _bits_equal(np.concatenate(pieces, axis=1), whole) and _sp_same_state(parts, ref)
    one.close()
    parts.close()


@pytest.mark.gpu
def test_surge_in_place_strides_and_null_out(gpu):
    C, n = G + 1, 2 * T + 9
    settings = _sp_settings(C, 1)
    x = _sp_level(91, C, n)
    bank, ref = _sp(gpu, settings)
    gain = _sp_check(gpu, bank, ref, x, what="apart")
    bank.close()
    for entry in ("process", "mul"):                            # out == in
        bank, _ = _sp(gpu, settings)
        dx = gpu.DeviceBuffer.from_host(x)
        (bank.process_mul if entry == "mul" else bank.process)(dx, dx, n)
        assert _bits_equal(dx.download(), x * gain if entry == "mul" else gain), entry
        assert _sp_same_state(bank, ref)
        bank.close()
    for entry in ("process", "mul"):                            # out NULL: the state alone, whichever entry
        bank, _ = _sp(gpu, settings)
        dx = gpu.DeviceBuffer.from_host(x)
        (bank.process_mul if entry == "mul" else bank.process)(None, dx, n)
        assert _sp_same_state(bank, ref) and np.array_equal(dx.download(), x)
        bank.close()
    k = 300
    for entry in ("process", "mul"):
        for os_, is_ in ((301, 303), (304, 312), (k, k + 1)):   # unaligned rows, unequal strides
            bank, ref2 = _sp(gpu, settings)
            pad = lambda v, s, fill: np.concatenate([v, np.full((C, s - v.shape[1]), fill, f32)], axis=1)
            hx, ho = pad(x[:, :k], is_, 3.0), pad(_sp_audio(C, k), os_, 7.0)
            dx, do = gpu.DeviceBuffer.from_host(hx), gpu.DeviceBuffer.from_host(ho)
            (bank.process_mul if entry == "mul" else bank.process)(do, dx, k, out_stride=os_, in_stride=is_)
            got = do.download()
            want = ref2.process(x[:, :k]) * (_sp_audio(C, k) if entry == "mul" else f32(1.0))
            assert _bits_equal(got[:, :k], want) and np.all(got[:, k:] == 7.0), "written past count"
            assert np.array_equal(dx.download(), hx) and _sp_same_state(bank, ref2)
            bank.close()


@pytest.mark.gpu
def test_surge_setters_act_at_once_in_call_order(gpu):
    """set_transition_time(5) and then (100) with the counter at 50 leaves 5; set_shutdown_time(20) and then (300) with the counter
    at 100 leaves 20; reset() in the middle of a fade; set_state between calls.  A bank that clamped against the last maximum
    alone would keep 50 and 100."""
    C = G + 2
    bank, ref = _sp(gpu, [(255, 300)] * C)
    x = np.full((C, 50), 0.9, f32)
    _sp_check(gpu, bank, ref, x, what="fade-in")
    assert np.all(ref.t == 50)
    for b in (bank, ref):
        b.set_transition_time(0, 5)
        b.set_transition_time(0, 100)
        b.set_transition_time(1, 100)                           # 50 <= 100: stays
        b.reset(2)
        b.set_transition_time(3, 5)
        b.reset(3)
        b.set_transition_time(3, 700)
    assert [bank.get_state(ch)["transition_time"] for ch in range(C)] == [5, 50, 0, 0, 50, 50]
    assert bank.get_state(2)["on"] == 0 and bank.get_state(2)["gain"] == ref.gain[2]          # reset leaves fGain
    want = _sp_check(gpu, bank, ref, np.full((C, T + 5), 0.9, f32), what="after the transition setters")
    assert want[0, 0] == np.sqrt(f32(5) / f32(100)) and want[1, 0] == np.sqrt(f32(50) / f32(100)) and want[2, 0] == 0.0
    # the shutdown counter
    _sp_check(gpu, bank, ref, np.full((C, 100), 0.1, f32), what="gone")
    assert np.all(ref.sd == 100) and np.all(ref.on)
    for b in (bank, ref):
        b.set_shutdown_time(0, 20)
        b.set_shutdown_time(0, 300)
        b.set_shutdown_time(1, 20)                              # off with the next sample
    assert [bank.get_state(ch)["shutdown_time"] for ch in range(3)] == [20, 20, 100]
    _sp_check(gpu, bank, ref, np.full((C, 190), 0.1, f32), what="after the shutdown setters")
    assert list(ref.on[:3]) == [True, False, True] and ref.sd[0] == 210
    _sp_check(gpu, bank, ref, np.full((C, 40), 0.1, f32), what="shutdown")
    assert list(ref.on[:3]) == [True, False, False]
    # set_state: as given; counters above their maxima and a flag above 1 are refused
    bank.reset()
    ref.reset()
    bank.set_state(4, 0.5, 255, 299, 1)
    ref.gain[4], ref.t[4], ref.sd[4], ref.on[4] = 0.5, 255, 299, True
    assert bank.get_state(4) == {"gain": 0.5, "transition_time": 255, "shutdown_time": 299, "on": 1}
    for args in ((0.5, 256, 0, 1), (0.5, 0, 301, 1), (0.5, 0, 0, 2)):
        with pytest.raises(gpu.MiError) as e:
            bank.set_state(4, *args)
        assert e.value.code == -1
    _sp_check(gpu, bank, ref, _sp_level(3, C, T + 9), what="after reset() and set_state")
    bank.set_threshold(0, 0.05, 0.01)
    bank.set_on_threshold(1, 2.0)
    bank.set_off_threshold(2, 0.6)
    ref.on_thr[0], ref.off_thr[0], ref.on_thr[1], ref.off_thr[2] = 0.05, 0.01, 2.0, 0.6
    _sp_check(gpu, bank, ref, _sp_level(4, C, 2 * T), what="after the thresholds")
    bank.close()


@pytest.mark.gpu
def test_surge_nan_level_never_passes(gpu):
    settings = [(255, 300), (7, 1), (0, 5), (T + 1, 0), (1, 300)]
    bank, ref = _sp(gpu, settings)
    C, n = len(settings), 2 * T + 40
    x = _sp_level(95, C, n)
    x[:, :40] = 0.1
    x[:, 20] = np.nan                                           # off: does not turn on
    x[:, 40:T + 60] = 0.9
    x[:, 100], x[:, T - 1:T + 4] = np.nan, np.nan               # on: counts as gone
    want = _sp_check(gpu, bank, ref, x, what="NaN")
    assert not np.isnan(want).any() and np.all(want[:, 20] == 0.0) and want[1, 101] < want[1, 99]
    bank.close()


# ---- both: capture, streams, lifetime, arguments --------------------------------------------------------------------------

def _stream(gpu):
    st = ctypes.c_void_p()
    gpu.check(gpu.lib.mi_dspu_stream_create(ctypes.byref(st)))
    return st


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["peakmeter", "surge", "surge-mul"])
def test_graph_capture_replays_direct_calls(gpu, kind):
    C, n = 9, T + 100
    st = _stream(gpu)
    if kind == "peakmeter":
        (bank, ref), (twin, _) = _pm(gpu, _pm_settings(C)), _pm(gpu, _pm_settings(C))
        x = _pm_signal(70, C, 3 * n)
    else:
        (bank, ref), (twin, _) = _sp(gpu, _sp_settings(C)), _sp(gpu, _sp_settings(C))
        x = _sp_level(70, C, 3 * n)
        bank.process(None, None, 0)                             # what the setters recorded goes out before the capture
    audio = _sp_audio(C, 3 * n)
    dx = [gpu.DeviceBuffer.from_host(x[:, i * n:(i + 1) * n]) for i in range(3)]
    o, t = ([gpu.DeviceBuffer((C, n)) for _ in range(3)] for _ in range(2))

    def call(b, out, i):
        if kind == "peakmeter":
            b.process(out, dx[i], n, stream=st.value)
        elif kind == "surge":
            b.process(out, dx[i], n, stream=st.value)
        else:
            gpu.check(gpu.lib.mi_dspu_copy_d2d(ctypes.c_void_p(out.ptr), ctypes.c_void_p(da[i].ptr), C * n * 4, st))
            b.process_mul(out, dx[i], n, stream=st.value)

    da = [gpu.DeviceBuffer.from_host(audio[:, i * n:(i + 1) * n]) for i in range(3)]
    gpu.check(gpu.lib.mi_dspu_graph_begin_capture(st))
    for i in range(3):
        call(bank, o[i], i)
    exe = ctypes.c_void_p()
    gpu.check(gpu.lib.mi_dspu_graph_end_capture(st, ctypes.byref(exe)))
    for rep in range(3):
        gpu.check(gpu.lib.mi_dspu_graph_launch(exe, st))
        for i in range(3):
            call(twin, t[i], i)
        got = np.concatenate([v.download(stream=st.value) for v in o], axis=1)
        direct = np.concatenate([v.download(stream=st.value) for v in t], axis=1)
        want = ref.process(x) * (audio if kind == "surge-mul" else f32(1.0))
        assert _same(got, direct) and _same(got, want), rep     # the state advances on every replay
        assert (_pm_same_state if kind == "peakmeter" else _sp_same_state)(bank, ref)
    gpu.lib.mi_dspu_graph_destroy(exe)
    bank.close()
    twin.close()
    gpu.check(gpu.lib.mi_dspu_stream_destroy(st))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["peakmeter", "surge"])
def test_setter_and_state_access_inside_a_capture_are_refused(gpu, kind):
    """A setter leaves work to the next call; on a capturing stream that call answers MI_ESTATE.  get_state() and set_state() end
    in a synchronisation and answer MI_ESTATE too; so does a process_value() whose count is not the cached one.  Nothing changes
    on the device, the capture stays valid, and what is captured after the refusals replays with the restatement's bits."""
    C, n = 5, T + 100
    st = _stream(gpu)
    if kind == "peakmeter":
        bank, ref = _pm(gpu, _pm_settings(C, 3))
        x0, x1 = _pm_signal(80, C, n), _pm_signal(81, C, n)
        same = _pm_same_state
    else:
        bank, ref = _sp(gpu, _sp_settings(C, 3))
        x0, x1 = _sp_level(80, C, n), _sp_level(81, C, n)
        same = _sp_same_state
    d0, d1, out = gpu.DeviceBuffer.from_host(x0), gpu.DeviceBuffer.from_host(x1), gpu.DeviceBuffer((C, n))
    bank.process(out, d0, n, stream=st.value)
    assert _same(out.download(stream=st.value), ref.process(x0))
    if kind == "peakmeter":
        bank.process_value(None, d0, 64, stream=st.value)       # the factor of 64 samples is on the device now
        ref.process_value(x0[0, :C], 64)                   # the values: the buffer's first C floats
    assert same(bank, ref)
    gpu.check(gpu.lib.mi_dspu_graph_begin_capture(st))
    if kind == "peakmeter":
        with pytest.raises(gpu.MiError) as e:
            bank.process_value(None, d0, 65, stream=st.value)   # another count: an upload
        assert e.value.code == -5 and "update_settings" in str(e.value)
        with pytest.raises(gpu.MiError) as e:                   # back to the cached one: the table is still to be sent
            bank.process_value(None, d0, 64, stream=st.value)
        assert e.value.code == -5
    else:
        bank.set_transition_time(0, 3)
    calls = [lambda: bank.process(out, d1, n, stream=st.value)]
    if kind == "peakmeter":
        calls.append(lambda: bank.update_settings(stream=st.value))
    for call in calls:
        with pytest.raises(gpu.MiError) as e:
            call()
        assert e.value.code == -5
    for call in (lambda: bank.get_state(2, stream=st.value),
                 lambda: bank.set_state(2, *((0.5, 0) if kind == "peakmeter" else (0.0, 0, 0, 0)), stream=st.value)):
        with pytest.raises(gpu.MiError) as e:
            call()
        assert e.value.code == -5 and "captured" in str(e.value)
    gpu.check(gpu.lib.mi_dspu_memset(ctypes.c_void_p(out.ptr), 0, 16, st))          # (so that the capture is not empty)
    exe = ctypes.c_void_p()
    gpu.check(gpu.lib.mi_dspu_graph_end_capture(st, ctypes.byref(exe)))
    assert exe.value
    gpu.lib.mi_dspu_graph_destroy(exe)
    if kind == "surge":
        ref.set_transition_time(0, 3)
    assert same(bank, ref)                                      # (the surge bank's clamp acts on the state from before)
    bank.process(out, d1, n, stream=st.value)                   # eager
    assert _same(out.download(stream=st.value), ref.process(x1)) and same(bank, ref)
    gpu.check(gpu.lib.mi_dspu_graph_begin_capture(st))          # with nothing pending everything is captured and replays
    bank.process(out, d0, n, stream=st.value)
    if kind == "peakmeter":
        bank.process_value(None, d0, 64, stream=st.value)
    gpu.check(gpu.lib.mi_dspu_graph_end_capture(st, ctypes.byref(exe)))
    for rep in range(3):
        gpu.check(gpu.lib.mi_dspu_graph_launch(exe, st))
        assert _same(out.download(stream=st.value), ref.process(x0)), rep
        if kind == "peakmeter":
            ref.process_value(x0[0, :C], 64)                   # the values: the buffer's first C floats
    assert same(bank, ref)
    gpu.lib.mi_dspu_graph_destroy(exe)
    bank.close()
    gpu.check(gpu.lib.mi_dspu_stream_destroy(st))


@pytest.mark.gpu
def test_two_banks_on_two_streams(gpu):
    """A peak meter bank and a surge bank fed alternately on two streams, nothing waited for until the end."""
    C, n, calls = 6, T + 57, 4
    streams = [_stream(gpu) for _ in range(2)]
    made = [_pm(gpu, _pm_settings(C, 2)), _sp(gpu, _sp_settings(C, 2))]
    sig = [_pm_signal(120, C, calls * n), _sp_level(121, C, calls * n)]
    ins = [[gpu.DeviceBuffer.from_host(sig[i][:, k * n:(k + 1) * n]) for k in range(calls)] for i in range(2)]
    outs = [[gpu.DeviceBuffer((C, n)) for _ in range(calls)] for _ in range(2)]
    made[1][0].process(None, None, 0, stream=streams[1].value)
    for k in range(calls):
        for i in range(2):
            made[i][0].process(outs[i][k], ins[i][k], n, stream=streams[i].value)
    for i in range(2):
        got = np.concatenate([v.download(stream=streams[i].value) for v in outs[i]], axis=1)
        assert _same(got, made[i][1].process(sig[i])), i
        made[i][0].close()
    for s in streams:
        gpu.check(gpu.lib.mi_dspu_stream_destroy(s))


def _free_bytes():
    hip = ctypes.CDLL("libamdhip64.so")             # the runtime the library itself runs on (already loaded)
    free, total = ctypes.c_size_t(), ctypes.c_size_t()
    assert hip.hipDeviceSynchronize() == 0
    assert hip.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) == 0
    return free.value


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["peakmeter", "surge"])
def test_create_use_destroy_returns_device_memory(gpu, kind):
    x = _pm_signal(1, 8, 1024)
    dx, out = gpu.DeviceBuffer.from_host(x), gpu.DeviceBuffer((8, 1024))

    def cycle():
        if kind == "peakmeter":
            bank = gpu.PeakMeterBank(8)
            for ch in range(8):
                bank.configure(ch, SR, 1.0 + ch, 5.0)
            bank.process(out, dx, 1024)
            bank.process_value(None, dx, 64)
        else:
            bank = gpu.SurgeProtectorBank(8)
            for ch in range(8):
                bank.configure(ch, 40 + 30 * ch, 100, 0.5, 0.25)
            bank.process(out, dx, 1024)
            bank.process_mul(out, dx, 1024)
        bank.close()

    for _ in range(3):
        cycle()
    before = _free_bytes()
    for _ in range(40):
        cycle()
    after = _free_bytes()
    assert before - after < 8 << 20, "%s: %.1f MiB of device memory did not come back after 40 objects" % (kind, (before - after) / 2 ** 20)


@pytest.mark.gpu
def test_zero_and_null_arguments_on_a_live_bank(gpu):
    """Every bad argument comes back as an error code before any launch; nothing is written."""
    lib, C, n = gpu.lib, 3, 64
    buf = gpu.DeviceBuffer.from_host(np.zeros((C, n), f32))
    p = ctypes.c_void_p(buf.ptr)
    pm = gpu.PeakMeterBank(C)
    h = pm.handle
    assert lib.mi_peakmeter_bank_process(h, p, p, None, 0, 0, 0, None) == 0                 # nothing to do
    assert lib.mi_peakmeter_bank_process(h, p, None, None, n, n, n, None) == -1             # no input
    assert lib.mi_peakmeter_bank_process(h, p, p, None, n, n - 1, n, None) == -1            # a stride shorter than count
    assert lib.mi_peakmeter_bank_process(h, p, p, None, n, n, n + 4, None) == -1            # in place with different strides
    assert lib.mi_peakmeter_bank_process(h, p, p, None, 1 << 31, 1 << 31, 1 << 31, None) == -1
    assert lib.mi_peakmeter_bank_process_value(h, None, None, 4, None) == -1 and lib.mi_peakmeter_bank_process_value(h, None, p, 1 << 32, None) == -1
    assert lib.mi_peakmeter_bank_set_sample_rate(h, C, SR) == -1 and lib.mi_peakmeter_bank_set_hold_time(h, C, 1.0) == -1
    assert lib.mi_peakmeter_bank_set_release_time(h, C, 1.0) == -1 and lib.mi_peakmeter_bank_set_time(h, C, 1.0, 1.0) == -1
    assert lib.mi_peakmeter_bank_clear(h, C) == -1 and lib.mi_peakmeter_bank_get_params(h, C, None) == -1
    assert lib.mi_peakmeter_bank_get_params(h, 0, None) == -1 and lib.mi_peakmeter_bank_set_params(h, 0, None) == -1
    assert lib.mi_peakmeter_bank_get_state(h, 0, None, None) == -1 and lib.mi_peakmeter_bank_get_state(h, C, None, None) == -1
    assert lib.mi_peakmeter_bank_set_state(h, 0, None, None) == -1
    sp = gpu.SurgeProtectorBank(C)
    h = sp.handle
    for fn in (lib.mi_surge_bank_process, lib.mi_surge_bank_process_mul):
        assert fn(h, p, p, 0, 0, 0, None) == 0
        assert fn(h, p, None, n, n, n, None) == -1
        assert fn(h, p, p, n, n - 1, n, None) == -1
        assert fn(h, p, p, n, n, n + 4, None) == -1
        assert fn(h, p, p, 1 << 31, 1 << 31, 1 << 31, None) == -1
    assert lib.mi_surge_bank_set_transition_time(h, C, 1) == -1 and lib.mi_surge_bank_set_shutdown_time(h, C, 1) == -1
    assert lib.mi_surge_bank_set_on_threshold(h, C, 0.5) == -1 and lib.mi_surge_bank_set_off_threshold(h, C, 0.5) == -1
    assert lib.mi_surge_bank_set_threshold(h, C, 0.5, 0.5) == -1 and lib.mi_surge_bank_reset(h, C) == -1
    assert lib.mi_surge_bank_get_params(h, C, None) == -1 and lib.mi_surge_bank_get_params(h, 0, None) == -1
    assert lib.mi_surge_bank_get_state(h, 0, None, None) == -1 and lib.mi_surge_bank_get_state(h, C, None, None) == -1
    assert lib.mi_surge_bank_set_state(h, 0, None, None) == -1
    assert np.all(buf.download() == 0.0), "a refused call wrote"
    assert lib.mi_peakmeter_bank_process(pm.handle, p, p, None, n, n, n, None) == 0          # and the banks still work
    assert lib.mi_surge_bank_process(h, p, p, n, n, n, None) == 0
    pm.close()
    sp.close()


# ---- the reference's recorded cases, the C++ classes, full size ------------------------------------------------------------

def _bank_design(bank):
    def design(sr, hold, release):
        bank.set_sample_rate(0, sr)
        bank.set_hold_time(0, hold)
        bank.set_release_time(0, release)
        p = bank.get_params(0)
        return p["tau"], p["hold"]
    return design


@pytest.mark.gpu
def test_every_recorded_reference_case_through_the_c_abi(gpu):
    """tests/golden/peak_surge_ref_vectors.npz, operation by operation, through the bank: out and the final state are the
    reference's (fTau within 1 ulp of the recorded one: it is this machine's libm against the recording machine's; where it is
    the recorded one, so is every sample)."""
    x, cases = gen.load()
    audio = x[gen.AUDIO]
    exact = 0
    for c in cases:
        sig = x[c["signal"]]
        out, at = np.zeros(gen.N, f32), 0
        if c["kind"] == gen.PEAKMETER:
            bank = gpu.PeakMeterBank(1)
            peaks = gpu.DeviceBuffer((1,))
            for what, arg in c["ops"]:
                what, arg = int(what), int(arg)
                if what == gen.P_SET_SR:
                    bank.set_sample_rate(0, arg)
                elif what == gen.P_SET_HOLD:
                    bank.set_hold_time(0, _f(arg))
                elif what == gen.P_SET_RELEASE:
                    bank.set_release_time(0, _f(arg))
                elif what == gen.P_CLEAR:
                    bank.clear(0)
                elif what == gen.P_PROCESS_VALUE:
                    bank.process_value(peaks, gpu.DeviceBuffer.from_host(sig[at:at + 1]), arg)
                    out[at] = peaks.download()[0]
                    at += 1
                else:
                    dx, do = gpu.DeviceBuffer.from_host(sig[at:at + arg]), gpu.DeviceBuffer((arg,))
                    bank.process(do if what == gen.P_PROCESS else None, dx, arg, peaks=peaks)
                    if what == gen.P_PROCESS:
                        out[at:at + arg] = do.download()
                    else:
                        out[at + arg - 1] = peaks.download()[0]
                    at += arg
            s, p = bank.get_state(0), bank.get_params(0)
            assert p["hold"] == int(c["state"][3]) and abs(int(p["tau"].view(u32)) - int(c["state"][2])) <= 1, c["name"]
            if int(p["tau"].view(u32)) == int(c["state"][2]):
                exact += 1
                assert _same(out, c["out"]), c["name"]
                assert _same(np.array([s["peak"]], f32), _f(c["state"][0]).reshape(1)) and s["counter"] == int(c["state"][1]), c["name"]
        else:
            bank = gpu.SurgeProtectorBank(1)
            for what, arg in c["ops"]:
                what, arg = int(what), int(arg)
                if what == gen.S_SET_TRANSITION:
                    bank.set_transition_time(0, arg)
                elif what == gen.S_SET_SHUTDOWN:
                    bank.set_shutdown_time(0, arg)
                elif what == gen.S_SET_ON:
                    bank.set_on_threshold(0, _f(arg))
                elif what == gen.S_SET_OFF:
                    bank.set_off_threshold(0, _f(arg))
                elif what == gen.S_RESET:
                    bank.reset(0)
                else:
                    dx = gpu.DeviceBuffer.from_host(sig[at:at + arg])
                    do = gpu.DeviceBuffer.from_host(audio[at:at + arg])
                    if what == gen.S_PROCESS_STATE:
                        bank.process(None, dx, arg)
                    else:
                        (bank.process_mul if what == gen.S_PROCESS_MUL else bank.process)(do, dx, arg)
                        out[at:at + arg] = do.download()
                    at += arg
            s = bank.get_state(0)
            assert _bits_equal(out, c["out"]), c["name"]
            assert [int(s["gain"].view(u32)), s["transition_time"], s["shutdown_time"], s["on"]] == [int(v) for v in c["state"]], c["name"]
        assert at == gen.N
        bank.close()
    assert exact >= 1


CPP = r'''
#include <lsp-plug.in/dsp-units/meters/PeakMeter.h>
#include <lsp-plug.in/dsp-units/dynamics/SurgeProtector.h>
#include <cstdio>
#include <vector>
using namespace lsp::dspu;
static const size_t N = 1200, STEP = 113, GUARD = 16;
static const float MARK = 12345.0f;
struct guarded                                                  // guard words around the samples
{
    std::vector<float> v;
    guarded(): v(N + 2 * GUARD, MARK) {}
    float *data() { return v.data() + GUARD; }
    bool intact() const { for (size_t i = 0; i < GUARD; ++i) if (v[i] != MARK || v[GUARD + N + i] != MARK) return false; return true; }
};
struct fields: public lsp::dspu::IStateDumper                   // what dump() writes, in order, as 32-bit words
{
    FILE *f;
    void write(const char *, float v) override          { fwrite(&v, 4, 1, f); }
    void write(const char *, unsigned int v) override   { fwrite(&v, 4, 1, f); }
    void write(const char *, unsigned long v) override  { unsigned int w = (unsigned int)(v); fwrite(&w, 4, 1, f); }
    void write(const char *, bool v) override           { unsigned int w = v ? 1 : 0; fwrite(&w, 4, 1, f); }
};
template <class M> static void dump(const M &m, FILE *f)
{
    fields d;
    d.f = f;
    m.dump(&d);
}
int main(int argc, char **argv)
{
    guarded x, level, audio, out;
    FILE *f = fopen(argv[1], "rb");
    if (fread(x.data(), 4, N, f) != N || fread(level.data(), 4, N, f) != N || fread(audio.data(), 4, N, f) != N) return 2;
    fclose(f);
    f = fopen(argv[2], "wb");

    // PeakMeter: steps of 113 with dst, then without, then block-rate steps
    PeakMeter pm;
    pm.set_sample_rate(48000);
    pm.set_time(257.0f / 48.0f + 0.001f, 5.0f);
    float last = 0.0f;
    for (size_t i = 0; i < N; i += STEP)
        last = pm.process(out.data() + i, x.data() + i, (N - i < STEP) ? N - i : STEP);
    if (!out.intact() || !x.intact() || last != pm.value() || last != out.data()[N - 1]) return 4;
    fwrite(out.data(), 4, N, f);
    dump(pm, f);
    pm.clear();
    if (pm.value() != 0.0f) return 5;
    pm.set_hold_time(0.5f);
    for (size_t i = 0; i < N; i += STEP)
        out.data()[i] = pm.process(x.data() + i, (N - i < STEP) ? N - i : STEP);
    fwrite(out.data(), 4, N, f);
    dump(pm, f);
    for (size_t i = 0; i < 64; ++i)
        out.data()[i] = pm.process(x.data()[i], size_t(i % 3 == 0 ? 0 : 64));
    fwrite(out.data(), 4, 64, f);
    dump(pm, f);
    PeakMeter fresh;                                            // release 0: tau = 0
    fresh.process(out.data(), x.data(), 300);
    fwrite(out.data(), 4, 300, f);
    dump(fresh, f);

    // SurgeProtector: steps of 113, the setters' order at a counter of 50, process_mul, single samples, reset
    SurgeProtector sp;
    sp.set_transition_time(255);
    sp.set_shutdown_time(300);
    sp.set_threshold(0.5f, 0.25f);
    sp.process(out.data(), level.data(), 140);
    sp.set_transition_time(5);
    sp.set_transition_time(100);
    for (size_t i = 140; i < N; i += STEP)
        sp.process(out.data() + i, level.data() + i, (N - i < STEP) ? N - i : STEP);
    if (!out.intact() || !level.intact()) return 6;
    fwrite(out.data(), 4, N, f);
    dump(sp, f);
    sp.reset();
    for (size_t i = 0; i < N; ++i)
        out.data()[i] = audio.data()[i];
    for (size_t i = 0; i < N; i += STEP)
        sp.process_mul(out.data() + i, level.data() + i, (N - i < STEP) ? N - i : STEP);
    if (!out.intact() || !audio.intact()) return 7;
    fwrite(out.data(), 4, N, f);
    dump(sp, f);
    sp.process(level.data(), 200);                              // the state only
    sp.process_mul(NULL, level.data() + 200, 100);
    for (size_t i = 300; i < 364; ++i)
        out.data()[i - 300] = sp.process(level.data()[i]);
    fwrite(out.data(), 4, 64, f);
    dump(sp, f);
    fclose(f);
    return 0;
}
'''


@pytest.mark.gpu
def test_cpp_classes_on_the_device(gpu, tmp_path):
    """lsp::dspu::PeakMeter and lsp::dspu::SurgeProtector from a small compiled program: every overload, guard words around the
    buffers; the samples and what dump() writes afterwards against the restatement."""
    src, exe = str(tmp_path / "ps.cpp"), str(tmp_path / "ps")
    open(src, "w").write(CPP)
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-I" + os.path.join(PKG, "include"), "-I" + os.path.join(ROOT, "include"), src,
                           "-o", exe, "-L" + PKG, "-lmi_dspu", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    sig = gen.signals()
    x, level, audio = sig[gen.SIG_PEAKS], sig[gen.SIG_LEVEL], sig[gen.AUDIO]
    n = gen.N
    np.concatenate([x, level, audio]).tofile(str(tmp_path / "in.bin"))
    out = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out
    r = np.fromfile(str(tmp_path / "out.bin"), u32)
    bits = lambda v: int(f32(v).view(u32))
    at = 0

    def take(k):
        nonlocal at
        at += k
        return r[at - k:at]

    # PeakMeter: dump() writes fPeak, fTau, fHold, fRelease, nHold, nCounter, nSampleRate, bUpdate
    hold_ms = f32(257.0) / f32(48.0) + f32(0.001)
    tau, hold = ps.design(SR, hold_ms, 5.0)
    assert hold == 257
    m = ps.PeakMeters([tau], [hold])
    want = m.process(x[None])[0]
    assert np.array_equal(take(n), want.view(u32))
    assert list(take(8)) == [bits(m.peak[0]), bits(tau), bits(hold_ms), bits(5.0), hold, m.counter[0], SR, 0]
    m.clear()
    tau, hold = ps.design(SR, 0.5, 5.0)
    m.tau[0], m.hold[0] = tau, hold
    got = take(n).view(f32)
    for i in range(0, n, 113):
        assert got[i].view(u32) == m.process(x[None, i:i + 113])[0, -1].view(u32), i
    assert list(take(8)) == [bits(m.peak[0]), bits(tau), bits(0.5), bits(5.0), hold, m.counter[0], SR, 0]
    got = take(64).view(f32)
    for i in range(64):
        assert got[i].view(u32) == m.process_value(x[i:i + 1], 0 if i % 3 == 0 else 64)[0].view(u32), i
    assert list(take(8)) == [bits(m.peak[0]), bits(tau), bits(0.5), bits(5.0), hold, m.counter[0], SR, 0]
    fresh = ps.PeakMeters([0.0], [0])
    assert np.array_equal(take(300), fresh.process(x[None, :300])[0].view(u32))
    assert list(take(8)) == [bits(fresh.peak[0]), 0, bits(5.0), 0, 0, 0, 0, 0]
    # SurgeProtector: fGain, nTransitionTime, nTransitionMax, nShutdownTime, nShutdownMax, fOnThreshold, fOffThreshold, bOn
    s = ps.SurgeProtectors(1)
    s.set_transition_time(0, 255)
    s.set_shutdown_time(0, 300)
    s.on_thr[0], s.off_thr[0] = 0.5, 0.25
    first = s.process(level[None, :140])[0]
    s.set_transition_time(0, 5)
    s.set_transition_time(0, 100)
    want = np.concatenate([first, s.process(level[None, 140:])[0]])
    assert want[140] == np.sqrt(f32(5) / f32(100))
    assert np.array_equal(take(n), want.view(u32))
    words = lambda: [bits(s.gain[0]), int(s.t[0]), int(s.tmax[0]), int(s.sd[0]), int(s.sdmax[0]), bits(0.5), bits(0.25), int(s.on[0])]
    assert list(take(8)) == words()
    s.reset()
    assert np.array_equal(take(n), (audio * s.process(level[None])[0]).view(u32))
    assert list(take(8)) == words()
    s.process(level[None, :300])
    assert np.array_equal(take(64), s.process(level[None, 300:364])[0].view(u32))
    assert list(take(8)) == words()
    assert at == r.size


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["peakmeter", "surge"])
def test_full_size_every_channel(gpu, kind):
    C, n = 1024, 4096
    if kind == "peakmeter":
        bank, ref = _pm(gpu, [(HOLDS[ch % 6], RELEASES[ch % 5]) for ch in range(C)])
        _pm_check(gpu, bank, ref, _pm_signal(99, C, n), what="1024 x 4096")
    else:
        bank, ref = _sp(gpu, [(TRANSITIONS[ch % 5], SHUTDOWNS[ch % 3]) for ch in range(C)])
        _sp_check(gpu, bank, ref, _sp_level(99, C, n), what="1024 x 4096")
    bank.close()
