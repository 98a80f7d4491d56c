"""mi_correlometer_bank and mi_panometer_bank (lsp::dspu::Correlometer, lsp::dspu::Panometer) on the device against
tests/stereo_meters_ref.py: out, every state word, nHead and nWindow bit for bit on every channel (the float32 restatement fed
the library's own parameters); across tiles, workgroups, periods on both sides of the tile and down to one sample, refreshes
with the window wrapped and not, split calls, changed settings, in place, strides, silence, subnormals, graph capture, two
streams, lifetime, bad arguments and the C++ classes."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import stereo_meters_ref as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "lsp-dsp-units_amd")
T, G = 256, 4                           # tile_chain_device.h: samples of a tile, channels of a workgroup
f32 = np.float32
MAX_PERIOD = 480                        # rings of 1536 samples
PERIODS = (1, 2, 3, 7, T - 1, T, T + 1, MAX_PERIOD)
KINDS = ("correlometer", "panometer")
VARIANTS = (("correlometer", None), ("panometer", sm.PAN_LAW_LINEAR), ("panometer", sm.PAN_LAW_EQUAL_POWER))
IDS = ["correlometer", "panometer-linear", "panometer-equal-power"]


def _bank(gpu, kind, periods, law=None, defaults=None, max_period=MAX_PERIOD):
    """A bank with the periods given, its parameters as the library reports them and the restatement fed those."""
    C = len(periods)
    if kind == "correlometer":
        bank = gpu.CorrelometerBank(C, max_period)
        for ch, p in enumerate(periods):
            bank.configure(ch, p)
    else:
        bank = gpu.PanometerBank(C, max_period)
        for ch, p in enumerate(periods):
            bank.configure(ch, p, law=(ch % 2) if law is None else law, default_pan=0.5 if defaults is None else defaults[ch])
    bank.update_settings()
    params = [bank.get_params(ch) for ch in range(C)]
    assert [p["period"] for p in params] == [min(p, max_period) for p in periods]
    assert all(p["capacity"] == sm.capacity(max_period) for p in params)
    ref = sm.Correlometers(params) if kind == "correlometer" else sm.Panometers(params)
    return bank, params, ref


def _signal(seed, C, n):
    """A correlated pair whose level steps between 1 and 1e-3: the running sums meet cancellation."""
    rng = np.random.default_rng(seed)
    level = np.where((np.arange(n) // 97) % 3 == 1, 1e-3, 1.0)
    a = rng.standard_normal((C, n)) * level
    b = 0.6 * a + 0.8 * rng.standard_normal((C, n)) * level
    return a.astype(f32), b.astype(f32)


def _run(gpu, bank, a, b, stream=None):
    C, n = a.shape
    da, db = gpu.DeviceBuffer.from_host(a), gpu.DeviceBuffer.from_host(b)
    out = gpu.DeviceBuffer((C, n))
    out.upload(np.full((C, n), 7.0, f32))
    bank.process(out, da, db, n, stream=stream)
    return out.download()


def _bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a, f32).view(np.uint32), np.ascontiguousarray(b, f32).view(np.uint32))


def _state(bank):
    s = [bank.get_state(ch) for ch in range(bank.channels)]
    return {k: np.array([v[k] for v in s], f32 if isinstance(s[0][k], np.floating) else np.uint32) for k in s[0]}


def _same_state(bank, ref):
    a, b = _state(bank), ref.state()
    return set(a) == set(b) and all(np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)) for k in a)


def _check(gpu, bank, ref, a, b, what=""):
    got = _run(gpu, bank, a, b)
    want, trace = ref.process(a, b)
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, (what, len(bad), bad[:4].tolist())
    assert _same_state(bank, ref), (what, _state(bank), ref.state())
    return got, trace


@pytest.mark.gpu
@pytest.mark.parametrize("count", [1, T - 1, T, T + 1, 2 * T + 3])
@pytest.mark.parametrize("C", [1, G - 1, G, G + 1, 2 * G + 1])
@pytest.mark.parametrize("kind,law", VARIANTS, ids=IDS)
def test_bit_exact_shapes(gpu, kind, law, C, count):
    bank, params, ref = _bank(gpu, kind, [PERIODS[(ch + C) % 8] for ch in range(C)], law)
    for blk in range(2):                                        # the second call starts from the first one's rings and state
        a, b = _signal(100 * count + 10 * C + blk, C, count)
        _check(gpu, bank, ref, a, b, what=blk)
    bank.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind,law", VARIANTS, ids=IDS)
def test_every_period_with_the_window_wrapped_and_in_one_piece(gpu, kind, law):
    """Eight different periods in two workgroups, from one refresh per sample to one per 480, over calls of 515, 257 and 1200
    samples: 1972 samples in rings of 1536, past the first wrapped refresh of every period."""
    bank, params, ref = _bank(gpu, kind, PERIODS, law)
    for blk, n in enumerate((2 * T + 3, T + 1, 1200)):
        a, b = _signal(7 + blk, len(PERIODS), n)
        _check(gpu, bank, ref, a, b, what=blk)
    for ch, p in enumerate(PERIODS):
        seen = {w for c, w in ref.refreshes if c == ch}
        assert seen == {False, True} or p == 1, (p, seen)
        assert len([1 for c, w in ref.refreshes if c == ch]) == -(-1972 // p), p      # one at the first sample, then every p
    bank.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind,law", VARIANTS, ids=IDS)
def test_calls_of_113_samples_equal_one_long_call(gpu, kind, law):
    C, n = G + 1, 1972
    periods = [(T + 1, 7, MAX_PERIOD, 40, 1)[ch] for ch in range(C)]
    one, params, ref = _bank(gpu, kind, periods, law)
    a, b = _signal(41, C, n)
    whole, _ = _check(gpu, one, ref, a, b, what="one call")
    parts, _, _ = _bank(gpu, kind, periods, law)
    got = np.concatenate([_run(gpu, parts, np.ascontiguousarray(a[:, p:p + 113]), np.ascontiguousarray(b[:, p:p + 113]))
                          for p in range(0, n, 113)], axis=1)
    assert _bits_equal(got, whole)
    assert _same_state(parts, ref) and _same_state(one, ref)
    one.close()
    parts.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind,law", VARIANTS, ids=IDS)
def test_set_period_and_clear_between_calls(gpu, kind, law):
    C = G + 1
    bank, params, ref = _bank(gpu, kind, [T + 1] * C, law)
    a, b = _signal(61, C, T + 40)
    _check(gpu, bank, ref, a, b, what="before")
    # a new period: the next sample starts with a refresh over the new window; unchanged and clamped values
    bank.set_period(0, 100)
    bank.set_period(1, T + 1)                                   # unchanged: ignored
    bank.set_period(2, 10 ** 6)                                 # clamped
    ref.set_period(0, 100)
    ref.set_period(2, 10 ** 6, MAX_PERIOD)
    bank.update_settings()
    new = [bank.get_params(ch) for ch in range(C)]
    assert [p["period"] for p in new] == [100, T + 1, MAX_PERIOD, T + 1, T + 1]
    if kind == "panometer":
        ref.set_params(new)
        assert bank.get_state(0)["value_a"] == 0.0 and bank.get_state(1)["value_a"] != 0.0
    assert bank.get_state(0)["window"] == 100 and bank.get_state(1)["window"] == T + 40 - (T + 1)
    before = len(ref.refreshes)
    a, b = _signal(62, C, T + 3)
    _check(gpu, bank, ref, a, b, what="after set_period")
    assert (0, False) in ref.refreshes[before:before + 2]
    # clear: the rings zero, nHead = nPeriod; the Correlometer's sums too
    window = _state(bank)["window"].copy()
    bank.clear(1)
    bank.update_settings()
    ref.clear(1)
    assert _same_state(bank, ref)
    s = bank.get_state(1)
    assert (s["head"], s["window"]) == (T + 1, int(window[1]))
    assert (s["v"], s["a"], s["b"]) == (0.0, 0.0, 0.0) if kind == "correlometer" else s["value_a"] != 0.0
    a, b = _signal(64, C, T + 3)
    _check(gpu, bank, ref, a, b, what="after clear(1)")
    bank.clear()
    bank.set_period(3, 33)                                      # after the clear: nHead stays at the old period
    for ch in range(C):
        ref.clear(ch)
    ref.set_period(3, 33)
    if kind == "panometer":
        bank.update_settings()
        ref.set_params([bank.get_params(ch) for ch in range(C)])
    a, b = _signal(65, C, 2 * T)
    _check(gpu, bank, ref, a, b, what="after clear()")
    assert bank.get_state(3)["head"] == (T + 1 + 2 * T) % sm.capacity(MAX_PERIOD)
    bank.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind,law", VARIANTS, ids=IDS)
def test_in_place(gpu, kind, law):
    C, n = G + 1, 2 * T + 9
    periods = [PERIODS[(2 * ch + 1) % 8] for ch in range(C)]
    a, b = _signal(91, C, n)
    apart, params, ref = _bank(gpu, kind, periods, law)
    want, _ = _check(gpu, apart, ref, a, b, what="apart")
    apart.close()
    for alias in (0, 1):
        bank, _, _ = _bank(gpu, kind, periods, law)
        da, db = gpu.DeviceBuffer.from_host(a), gpu.DeviceBuffer.from_host(b)
        bank.process((da, db)[alias], da, db, n)                # out == a, out == b
        assert _bits_equal((da, db)[alias].download(), want), alias
        assert np.array_equal((db, da)[alias].download(), (b, a)[alias])
        assert _same_state(bank, ref)
        bank.close()


@pytest.mark.gpu
@pytest.mark.parametrize("strides", [(301, 303, 307), (304, 312, 308), (300, 300, 300)])
@pytest.mark.parametrize("kind", KINDS)
def test_strides_and_unaligned_rows(gpu, kind, strides):
    C, n = G + 1, T + 44
    os_, s0, s1 = strides
    bank, params, ref = _bank(gpu, kind, [PERIODS[(ch + 3) % 8] for ch in range(C)])
    a, b = _signal(81, C, n)
    pad = lambda v, s, fill: np.concatenate([v, np.full((C, s - n), fill, f32)], axis=1)
    ha, hb = pad(a, s0, 3.0), pad(b, s1, 5.0)
    da, db, do = gpu.DeviceBuffer.from_host(ha), gpu.DeviceBuffer.from_host(hb), gpu.DeviceBuffer((C, os_))
    do.upload(np.full((C, os_), 7.0, f32))
    bank.process(do, da, db, n, out_stride=os_, a_stride=s0, b_stride=s1)
    got = do.download()
    want, _ = ref.process(a, b)
    assert _bits_equal(got[:, :n], want) and np.all(got[:, n:] == 7.0), "written past count"
    assert np.array_equal(da.download(), ha) and np.array_equal(db.download(), hb), "an input was written"
    assert _same_state(bank, ref)
    bank.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind,law", VARIANTS, ids=IDS)
def test_silence_reaches_the_zero_and_default_branches(gpu, kind, law):
    """Signal, silence in both rows for more than two periods (a refresh then finds only zeros and the sums are exactly 0), silence
    in b alone, signal again."""
    periods = [1, 7, 100, T, T + 1]
    C, n = len(periods), 1400
    bank, params, ref = _bank(gpu, kind, periods, law, defaults=[0.5, 0.25, -1.0, 0.5, 2.0])
    a, b = _signal(93, C, n)
    a[:, 300:900] = 0.0
    b[:, 300:900] = 0.0
    b[:, 1000:1200] = 0.0
    got, trace = _check(gpu, bank, ref, a, b, what="silence")
    assert np.all(trace[:, :, 850:900] == 0.0)
    rest = f32(0.0) if kind == "correlometer" else np.array([p["default_pan"] for p in params], f32)[:, None]
    assert np.all(got[:, 850:900] == rest) and np.all((got[:, :300] != rest).any(axis=1))
    if kind == "panometer":
        assert np.all(got[:3, 1150:1200] == 0.0)                # only a sounds: hard left
    else:
        assert np.all(got[:3, 1150:1200] == 0.0)                # b's sum of squares is 0: a * b is under the threshold
    bank.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind,law", VARIANTS, ids=IDS)
def test_subnormal_inputs_are_kept(gpu, kind, law):
    C, n = G, 2 * T + 5
    bank, params, ref = _bank(gpu, kind, [1, 7, T + 1, 40], law)
    rng = np.random.default_rng(95)
    a = (rng.standard_normal((C, n)) * 1e-19).astype(f32)       # squares around 1e-38 and below: subnormal
    b = (rng.standard_normal((C, n)) * 1e-19).astype(f32)
    a[:, ::3] = (rng.standard_normal((C, len(range(0, n, 3)))) * 1e-40).astype(f32)    # subnormal samples
    got, trace = _check(gpu, bank, ref, a, b, what="subnormal")
    tiny = f32(1.1754944e-38)
    assert np.any((np.abs(trace) > 0) & (np.abs(trace) < tiny)), "the sums never were subnormal"
    bank.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_graph_capture_replays_direct_calls(gpu, kind):
    C, n = 9, T + 100
    st = ctypes.c_void_p()
    gpu.check(gpu.lib.mi_dspu_stream_create(ctypes.byref(st)))
    periods = [PERIODS[ch % 8] for ch in range(C)]
    bank, params, ref = _bank(gpu, kind, periods)
    twin, _, _ = _bank(gpu, kind, periods)
    a, b = _signal(70, C, 3 * n)
    da = [gpu.DeviceBuffer.from_host(a[:, i * n:(i + 1) * n]) for i in range(3)]
    db = [gpu.DeviceBuffer.from_host(b[:, i * n:(i + 1) * n]) for i in range(3)]
    o = [gpu.DeviceBuffer((C, n)) for _ in range(3)]
    gpu.check(gpu.lib.mi_dspu_graph_begin_capture(st))
    for i in range(3):
        bank.process(o[i], da[i], db[i], n, stream=st.value)
    exe = ctypes.c_void_p()
    gpu.check(gpu.lib.mi_dspu_graph_end_capture(st, ctypes.byref(exe)))
    t = [gpu.DeviceBuffer((C, n)) for _ in range(3)]
    for rep in range(3):
        gpu.check(gpu.lib.mi_dspu_graph_launch(exe, st))
        for i in range(3):
            twin.process(t[i], da[i], db[i], n, stream=st.value)
        got = np.concatenate([v.download(stream=st.value) for v in o], axis=1)
        direct = np.concatenate([v.download(stream=st.value) for v in t], axis=1)
        want, _ = ref.process(a, b)
        assert _bits_equal(got, direct) and _bits_equal(got, want), rep         # the state advances on every replay
        assert _same_state(bank, ref)
    gpu.lib.mi_dspu_graph_destroy(exe)
    bank.close()
    twin.close()
    gpu.check(gpu.lib.mi_dspu_stream_destroy(st))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_setter_and_state_read_inside_a_capture_are_refused(gpu, kind):
    """A setter leaves work to the next call; on a capturing stream that call answers MI_ESTATE and names update_settings().
    get_state() ends in a synchronisation and answers MI_ESTATE too.  Nothing changes on the device, the capture stays valid,
    and a process() captured after the refusals replays with the bits of the restatement."""
    C, n = 5, T + 100
    st = ctypes.c_void_p()
    gpu.check(gpu.lib.mi_dspu_stream_create(ctypes.byref(st)))
    bank, params, ref = _bank(gpu, kind, [T + 1, 7, 40, 1, MAX_PERIOD])
    a0, b0 = _signal(80, C, n)
    a1, b1 = _signal(81, C, n)
    d0, e0, d1, e1 = (gpu.DeviceBuffer.from_host(v) for v in (a0, b0, a1, b1))
    out = gpu.DeviceBuffer((C, n))
    bank.process(out, d0, e0, n, stream=st.value)
    out0 = out.download(stream=st.value)
    assert _bits_equal(out0, ref.process(a0, b0)[0])
    before = _state(bank)
    gpu.check(gpu.lib.mi_dspu_graph_begin_capture(st))
    bank.set_period(0, 100)
    for call in (lambda: bank.process(out, d1, e1, n, stream=st.value), lambda: bank.update_settings(stream=st.value)):
        with pytest.raises(gpu.MiError) as e:
            call()
        assert e.value.code == -5 and "update_settings" in str(e.value)
    with pytest.raises(gpu.MiError) as e:
        bank.get_state(2, stream=st.value)
    assert e.value.code == -5 and "captured" in str(e.value)
    gpu.check(gpu.lib.mi_dspu_memset(ctypes.c_void_p(out.ptr), 0, 16, st))         # (so that the capture is not empty)
    exe = ctypes.c_void_p()
    gpu.check(gpu.lib.mi_dspu_graph_end_capture(st, ctypes.byref(exe)))             # ends and instantiates normally
    assert exe.value
    gpu.lib.mi_dspu_graph_destroy(exe)
    after = _state(bank)
    assert all(np.array_equal(after[k], before[k]) for k in before)
    bank.process(out, d1, e1, n, stream=st.value)               # eager: the setting is applied to the state from before
    ref.set_period(0, 100)
    if kind == "panometer":
        ref.set_params([bank.get_params(ch) for ch in range(C)])
    assert _bits_equal(out.download(stream=st.value), ref.process(a1, b1)[0])
    assert _same_state(bank, ref)
    # with nothing pending a process() is captured and replays
    gpu.check(gpu.lib.mi_dspu_graph_begin_capture(st))
    bank.process(out, d0, e0, n, stream=st.value)
    gpu.check(gpu.lib.mi_dspu_graph_end_capture(st, ctypes.byref(exe)))
    for rep in range(3):
        gpu.check(gpu.lib.mi_dspu_graph_launch(exe, st))
        assert _bits_equal(out.download(stream=st.value), ref.process(a0, b0)[0]), rep
    assert _same_state(bank, ref)
    gpu.lib.mi_dspu_graph_destroy(exe)
    bank.close()
    gpu.check(gpu.lib.mi_dspu_stream_destroy(st))


@pytest.mark.gpu
def test_two_banks_on_two_streams(gpu):
    """A correlometer bank and a panometer bank fed alternately on two streams, nothing waited for until the end."""
    C, n, calls = 6, T + 57, 4
    streams = []
    for _ in range(2):
        s = ctypes.c_void_p()
        gpu.check(gpu.lib.mi_dspu_stream_create(ctypes.byref(s)))
        streams.append(s)
    periods = [PERIODS[(ch + 2) % 8] for ch in range(C)]
    made = [_bank(gpu, kind, periods) for kind in KINDS]
    sig = [_signal(120 + i, C, calls * n) for i in range(2)]
    ins = [[(gpu.DeviceBuffer.from_host(sig[i][0][:, k * n:(k + 1) * n]), gpu.DeviceBuffer.from_host(sig[i][1][:, k * n:(k + 1) * n]))
            for k in range(calls)] for i in range(2)]
    outs = [[gpu.DeviceBuffer((C, n)) for _ in range(calls)] for _ in range(2)]
    for k in range(calls):
        for i in range(2):
            made[i][0].process(outs[i][k], ins[i][k][0], ins[i][k][1], n, stream=streams[i].value)
    for i in range(2):
        got = np.concatenate([v.download(stream=streams[i].value) for v in outs[i]], axis=1)
        assert _bits_equal(got, made[i][2].process(*sig[i])[0]), KINDS[i]
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
@pytest.mark.parametrize("kind", KINDS)
def test_create_use_destroy_returns_device_memory(gpu, kind):
    a, b = _signal(1, 8, 1024)
    da, db, out = gpu.DeviceBuffer.from_host(a), gpu.DeviceBuffer.from_host(b), gpu.DeviceBuffer((8, 1024))

    def cycle():
        bank = (gpu.CorrelometerBank if kind == "correlometer" else gpu.PanometerBank)(8, 2400)
        for ch in range(8):
            bank.set_period(ch, 40 + 300 * ch)
        bank.process(out, da, db, 1024)
        bank.close()

    for _ in range(3):
        cycle()
    before = _free_bytes()
    for _ in range(40):
        cycle()
    after = _free_bytes()
    assert before - after < 8 << 20, "%s: %.1f MiB of device memory did not come back after 40 objects" % (kind, (before - after) / 2 ** 20)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_zero_and_null_arguments_on_a_live_bank(gpu, kind):
    lib, C, n = gpu.lib, 3, 64
    fn = lambda what: getattr(lib, "mi_%s_bank_%s" % (kind, what))
    bank = (gpu.CorrelometerBank if kind == "correlometer" else gpu.PanometerBank)(C, MAX_PERIOD)
    h = bank.handle
    buf = gpu.DeviceBuffer((C, n))
    buf.upload(np.zeros((C, n), f32))
    p = ctypes.c_void_p(buf.ptr)
    # a channel without a period: refused by name, nothing launched
    bank.set_period(0, 10)
    bank.set_period(2, 10)
    assert fn("process")(h, p, p, p, n, n, n, n, None) == -5 and b"channel 1" in lib.mi_dspu_last_error()
    assert fn("set_period")(h, 1, 0) == -1 and fn("set_period")(h, C, 5) == -1
    assert fn("process")(h, p, p, p, 0, 0, 0, 0, None) == 0                   # nothing to do
    bank.set_period(1, 10)
    for args in ((None, p, p), (p, None, p), (p, p, None)):
        assert fn("process")(h, *args, n, n, n, n, None) == -1
    assert fn("process")(h, p, p, p, n, n - 1, n, n, None) == -1               # a stride shorter than count
    assert fn("process")(h, p, p, p, n, n, n + 4, n, None) == -1               # in place with different strides
    assert fn("process")(h, p, p, p, 1 << 31, 1 << 31, 1 << 31, 1 << 31, None) == -1
    assert fn("clear")(h, C) == -1 and fn("get_params")(h, C, None) == -1 and fn("get_params")(h, 0, None) == -1
    assert fn("get_state")(h, 0, None, None) == -1 and fn("get_state")(h, C, None, None) == -1
    assert fn("set_state")(h, 0, None, 0, None) == -1
    if kind == "panometer":
        assert lib.mi_panometer_bank_set_pan_law(h, 0, 2) == -1 and lib.mi_panometer_bank_set_pan_law(h, C, 0) == -1
        assert lib.mi_panometer_bank_set_default_pan(h, C, 0.5) == -1
    assert np.all(buf.download() == 0.0), "a refused call wrote"
    assert fn("process")(h, p, p, p, n, n, n, n, None) == 0                   # and the bank still works
    # set_state: nHead modulo the capacity, nWindow at most the period
    if kind == "correlometer":
        bank.set_state(0, 1.0, 2.0, 3.0, sm.capacity(MAX_PERIOD) + 5, 99, zero_rings=True)
        assert bank.get_state(0) == {"v": 1.0, "a": 2.0, "b": 3.0, "head": 5, "window": 10}
    else:
        bank.set_state(0, 1.0, 2.0, sm.capacity(MAX_PERIOD) + 5, 99, zero_rings=True)
        assert bank.get_state(0) == {"value_a": 1.0, "value_b": 2.0, "head": 5, "window": 10}
    bank.close()


CPP = r'''
#include <lsp-plug.in/dsp-units/meters/Correlometer.h>
#include <lsp-plug.in/dsp-units/meters/Panometer.h>
#include <cstdio>
#include <vector>
using namespace lsp::dspu;
static const size_t N = 2300, RANGE = 257, STEP = 113, GUARD = 16;
static const float MARK = 12345.0f;
struct guarded                                                  // guard words around the samples
{
    std::vector<float> v;
    guarded(): v(N + 2 * GUARD, MARK) {}
    float *data() { return v.data() + GUARD; }
    bool intact() const { for (size_t i = 0; i < GUARD; ++i) if (v[i] != MARK || v[GUARD + N + i] != MARK) return false; return true; }
};
struct fields: public lsp::dspu::IStateDumper                   // the floats and the 32-bit words dump() writes, in order
{
    FILE *f;
    void write(const char *, float v) override          { fwrite(&v, 4, 1, f); }
    void write(const char *, unsigned int v) override   { fwrite(&v, 4, 1, f); }
    void write(const char *, int v) override            { fwrite(&v, 4, 1, f); }
};
template <class M> static int run(M &m, guarded &out, guarded &a, guarded &b, FILE *f)
{
    for (size_t i = 0; i < N; i += STEP)                        // the loop of the reference's unit test: steps of 113
    {
        const size_t count = (N - i < STEP) ? N - i : STEP;
        m.process(out.data() + i, a.data() + i, b.data() + i, count);
    }
    if (!out.intact() || !a.intact() || !b.intact())
        return 4;
    fwrite(out.data(), sizeof(float), N, f);
    fields d;
    d.f = f;
    m.dump(&d);
    return 0;
}
int main(int argc, char **argv)
{
    guarded out, a, b;
    FILE *f = fopen(argv[1], "rb");
    if (fread(a.data(), sizeof(float), N, f) != N || fread(b.data(), sizeof(float), N, f) != N) return 2;
    fclose(f);
    f = fopen(argv[2], "wb");
    Correlometer cm;
    if (cm.init(RANGE) != 0) return 3;
    cm.set_period(RANGE);                                       // the period equal to the range
    if (!cm.needs_update()) return 5;
    int r = run(cm, out, a, b, f);
    if (r != 0 || cm.needs_update() || cm.period() != RANGE) return 6;
    cm.destroy();
    static const pan_law_t laws[2] = { PAN_LAW_LINEAR, PAN_LAW_EQUAL_POWER };
    for (int k = 0; k < 2; ++k)
    {
        Panometer pm;
        if (pm.init(RANGE) != 0) return 3;
        pm.set_pan_law(laws[k]);
        pm.set_default_pan(0.25f);
        pm.set_period(RANGE);
        r = run(pm, out, a, b, f);
        if (r != 0 || pm.pan_law() != laws[k] || pm.default_pan() != 0.25f) return 7;
    }
    // a period of 0: process() returns without writing
    Correlometer zero;
    zero.init(RANGE);
    out.data()[0] = MARK;
    zero.process(out.data(), a.data(), b.data(), 8);
    Panometer pzero;
    pzero.init(RANGE);
    pzero.process(out.data() + 8, a.data(), b.data(), 8);
    if (out.data()[0] != MARK) return 8;
    fclose(f);
    return 0;
}
'''


@pytest.mark.gpu
def test_cpp_classes_on_the_device(gpu, tmp_path):
    """The reference's utest/meters/correlometer.cpp in shape: steps of 113 samples with the period equal to the range, guard words
    around the buffers; out and what dump() writes afterwards against the restatement."""
    src, exe = str(tmp_path / "sm.cpp"), str(tmp_path / "sm")
    open(src, "w").write(CPP)
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-I" + os.path.join(PKG, "include"), "-I" + os.path.join(ROOT, "include"), src,
                           "-o", exe, "-L" + PKG, "-lmi_dspu", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    n, rng_ = 2300, 257
    a, b = _signal(60, 1, n)
    a[:, 1200:1800] = 0.0
    b[:, 1200:1800] = 0.0
    np.concatenate([a[0], b[0]]).tofile(str(tmp_path / "in.bin"))
    out = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out
    r = np.fromfile(str(tmp_path / "out.bin"), np.uint32)
    cap = sm.capacity(rng_)
    # Correlometer: out, then sCorr.v, a, b, nCapacity, nHead, nMaxPeriod, nPeriod, nWindow, nFlags
    ref = sm.Correlometers([dict(period=rng_, capacity=cap)])
    want, _ = ref.process(a, b)
    assert np.array_equal(r[:n], want[0].view(np.uint32))
    s = ref.state()
    assert list(r[n:n + 9]) == [s["v"].view(np.uint32)[0], s["a"].view(np.uint32)[0], s["b"].view(np.uint32)[0], cap, s["head"][0], rng_,
                                rng_, s["window"][0], 0]
    assert np.any(want == 0.0) and np.any(want != 0.0)
    # Panometer: out, then enPanLaw, fValueA, fValueB, fNorm, fDefault, nCapacity, nHead, nMaxPeriod, nPeriod, nWindow
    at = n + 9
    for law in (sm.PAN_LAW_LINEAR, sm.PAN_LAW_EQUAL_POWER):
        norm = f32(1.0) / f32(rng_)
        ref = sm.Panometers([dict(period=rng_, capacity=cap, law=law, norm=norm, default_pan=0.25)])
        want, _ = ref.process(a, b)
        assert np.array_equal(r[at:at + n], want[0].view(np.uint32)), law
        s = ref.state()
        assert list(r[at + n:at + n + 10]) == [law, s["value_a"].view(np.uint32)[0], s["value_b"].view(np.uint32)[0], norm.view(np.uint32),
                                               f32(0.25).view(np.uint32), cap, s["head"][0], rng_, rng_, s["window"][0]], law
        assert np.any(want == f32(0.25))
        at += n + 10
    assert at == r.size


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_full_size_every_channel(gpu, kind):
    C, n = 1024, 4096
    lengths = (40, T - 1, T, T + 1, 1000, 2400)
    bank, params, ref = _bank(gpu, kind, [lengths[ch % 6] for ch in range(C)], max_period=2400)
    assert {p["period"] for p in params} == set(lengths)
    a, b = _signal(99, C, n)
    _check(gpu, bank, ref, a, b, what="1024 x 4096")
    bank.close()
