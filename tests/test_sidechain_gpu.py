"""mi_sidechain_bank (lsp::dspu::Sidechain) on the device against tests/sidechain_ref.py: out, fRmsValue, nRefresh and the ring
position bit for bit on every channel (the float32 restatement fed the library's own nReactivity, tau, interval and capacity);
across tiles, workgroups, window lengths on both sides of the tile, the refresh with its window wrapped and not, split calls,
changed settings, every source, in place, strides, mixed modes, subnormals, graph capture, the chain into the compressor bank
and the C++ class."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import compressor_ref as cr
import sidechain_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "lsp-dsp-units_amd")
T, G = 256, 4                           # tile_chain_device.h: samples of a tile, channels of a workgroup
f32 = np.float32
RATE, MAX_MS, N_MAX = 48000, 10.0, 480  # the banks of most tests: 10 ms at 48 kHz, rings of 992 samples
LENGTHS = (1, T - 1, T, T + 1, N_MAX)   # last = x[i - N] out of the same tile, across the straddle, out of the ring


def _ms(n, rate=RATE):
    """A reactivity that is n samples: n + 1/2 samples, truncated (the maximum as it is)."""
    return MAX_MS if (n, rate) == (N_MAX, RATE) else (n + 0.5) * 1000.0 / rate


def _settings(ch, mode=None, n=None):
    return dict(sample_rate=RATE, reactivity=_ms(LENGTHS[ch % 5] if n is None else n), mode=sr.MODES[ch % 4] if mode is None else mode,
                gain=(1.0, 0.5, -1.5, 2.0, 1.0)[ch % 5])


def _bank(gpu, settings, inputs=1, max_ms=MAX_MS):
    bank = gpu.SidechainBank(len(settings), inputs, max_ms)
    for ch, s in enumerate(settings):
        bank.configure(ch, **s)
    bank.update_settings()
    params = [bank.get_params(ch) for ch in range(len(settings))]
    return bank, params, sr.Sidechains(params, inputs)


def _signal(seed, C, n):
    """Gaussian samples whose level steps between 1 and 1e-3: the window detectors' running sums meet cancellation."""
    rng = np.random.default_rng(seed)
    level = np.where((np.arange(n) // 97) % 3 == 1, 1e-3, 1.0)
    return (rng.standard_normal((C, n)) * level).astype(f32)


def _run(gpu, bank, in0, in1=None, count=None):
    C = bank.channels
    n = count if in0 is None else in0.shape[1]
    d0 = None if in0 is None else gpu.DeviceBuffer.from_host(in0)
    d1 = None if in1 is None else gpu.DeviceBuffer.from_host(in1)
    out = gpu.DeviceBuffer((C, n))
    out.upload(np.full((C, n), 7.0, f32))
    bank.process(out, d0, d1, n)
    return out.download()


def _bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a, f32).view(np.uint32), np.ascontiguousarray(b, f32).view(np.uint32))


def _state(bank):
    s = [bank.get_state(ch) for ch in range(bank.channels)]
    return {"rms": np.array([v[0] for v in s], f32), "refresh": np.array([v[1] for v in s], np.uint32),
            "head": np.array([v[2] for v in s], np.uint32)}


def _same_state(bank, ref):
    a, b = _state(bank), ref.state()
    return all(np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)) for k in ("rms", "refresh", "head"))


def _check(gpu, bank, ref, in0, in1=None, count=None, what=""):
    got = _run(gpu, bank, in0, in1, count)
    want, trace = ref.process(in0, in1, count)
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, (what, len(bad), bad[:4].tolist())
    assert _same_state(bank, ref), (what, _state(bank), ref.state())
    return got, trace


@pytest.mark.gpu
@pytest.mark.parametrize("count", [1, T - 1, T, T + 1, 2 * T + 3])
@pytest.mark.parametrize("C", [1, G - 1, G, G + 1, 2 * G + 1])
def test_bit_exact_shapes_in_every_mode(gpu, C, count):
    for mode in sr.MODES:
        bank, params, ref = _bank(gpu, [_settings(ch + mode, mode=mode) for ch in range(C)])
        for blk in range(2):                                    # the second call starts from the first one's ring and state
            _check(gpu, bank, ref, _signal(100 * count + 10 * C + blk, C, count), what=(mode, blk))
        bank.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [sr.SCM_RMS, sr.SCM_UNIFORM])
def test_window_lengths_around_the_tile(gpu, mode):
    bank, params, ref = _bank(gpu, [_settings(0, mode=mode, n=n) for n in LENGTHS])
    assert [p["reactivity"] for p in params] == list(LENGTHS) and all(p["capacity"] == N_MAX + 512 for p in params)
    for blk, n in enumerate((2 * T + 3, T + 1, 700)):           # 1472 samples: the ring of 992 wraps
        _, trace = _check(gpu, bank, ref, _signal(7 + blk, len(LENGTHS), n), what=(mode, blk))
    bank.close()


@pytest.mark.gpu
def test_refresh_with_the_window_wrapped_and_in_one_piece(gpu):
    """One call of 0x2000 + 300 samples.  At the refresh the ring of 2912 (48 kHz, 50 ms, N 2400) stands at 2368 < N: two partial
    sums; the ring of 552 (8 kHz, 5 ms, N 40) at 464: one."""
    for rate, max_ms, ms, N, cap, wrapped in ((48000, 50.0, 50.0, 2400, 2912, True), (8000, 5.0, 5.0, 40, 552, False)):
        bank, params, ref = _bank(gpu, [dict(sample_rate=rate, reactivity=ms, mode=m) for m in sr.MODES] +
                                  [dict(sample_rate=rate, reactivity=ms, mode=sr.SCM_RMS, gain=-0.75)], max_ms=max_ms)
        assert all((p["reactivity"], p["capacity"]) == (N, cap) for p in params)
        n = sr.REFRESH_RATE + 300
        _, trace = _check(gpu, bank, ref, _signal(31, len(params), n), what=rate)
        assert sorted(ref.refreshes) == [(1, wrapped), (3, wrapped), (4, wrapped)]     # the window modes, each once
        assert all(int(v) == 300 for v in ref.refresh) and all(int(h) == n % cap for h in ref.head)
        bank.close()


@pytest.mark.gpu
def test_calls_of_511_samples_equal_one_long_call(gpu):
    C, n = G + 1, 2 * sr.REFRESH_RATE + 17
    settings = [dict(sample_rate=48000, reactivity=50.0 if ch < 4 else 1.0, mode=sr.MODES[ch % 4]) for ch in range(C)]
    one, params, ref = _bank(gpu, settings, max_ms=50.0)
    x = _signal(41, C, n)
    whole, _ = _check(gpu, one, ref, x, what="one call")
    parts, _, _ = _bank(gpu, settings, max_ms=50.0)
    got = np.concatenate([_run(gpu, parts, np.ascontiguousarray(x[:, p:p + 511])) for p in range(0, n, 511)], axis=1)
    assert _bits_equal(got, whole)
    assert _same_state(parts, ref) and _same_state(one, ref)
    assert [int(v) for v in ref.refresh] == [17] * C            # the counter depends on the samples seen, not on the calls
    one.close()
    parts.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [sr.SCM_RMS, sr.SCM_UNIFORM])
def test_set_mode_zeroes_the_sum_and_the_output_sits_on_the_clamp(gpu, mode):
    """PEAK over a loud stretch and a quiet one, then set_mode: fRmsValue is 0 with the loud samples still in the ring, so the
    running sum goes negative as they leave the window and the output is the clamp's 0 until the refresh."""
    C, N = 2, 300
    bank, params, ref = _bank(gpu, [_settings(0, mode=sr.SCM_PEAK, n=N) for _ in range(C)])
    rng = np.random.default_rng(51)
    loud = (rng.standard_normal((C, 400)) + 3.0).astype(f32)
    quiet = (rng.standard_normal((C, 3 * T)) * 1e-3).astype(f32)
    _check(gpu, bank, ref, np.concatenate([loud, quiet[:, :100]], axis=1), what="peak")
    for ch in range(C):
        bank.set_mode(ch, mode)
        ref.set_mode(ch, mode)
    got, trace = _check(gpu, bank, ref, np.ascontiguousarray(quiet[:, 100:]), what="after set_mode")
    assert np.all(trace[:, N - 100:] < 0) and np.all(got[:, N - 100:] == 0.0)          # once every loud sample has left the window
    assert np.all(trace[:, :20] <= 0)
    # the refresh puts the sum right: 0x2000 samples after the bank's first one
    rest = sr.REFRESH_RATE - 500 - (3 * T - 100)
    got, trace = _check(gpu, bank, ref, (rng.standard_normal((C, rest + 50)) * 1e-3).astype(f32), what="to the refresh")
    assert np.all(got[:, :rest] == 0.0) and np.all(got[:, rest:] > 0.0) and len(ref.refreshes) == C
    bank.close()


@pytest.mark.gpu
def test_reactivity_clear_and_gains_between_calls(gpu):
    C = G + 1
    bank, params, ref = _bank(gpu, [_settings(ch, mode=(sr.SCM_RMS, sr.SCM_UNIFORM)[ch % 2], n=T + 1) for ch in range(C)])
    _check(gpu, bank, ref, _signal(61, C, T + 40), what="before")
    # set_reactivity: a refresh at the next sample, over the new window
    bank.set_reactivity(0, _ms(100))
    bank.set_reactivity(1, 1e6)                                 # outside [0, maximum]: ignored
    bank.set_reactivity(2, -1.0)
    bank.update_settings()
    new = [bank.get_params(ch) for ch in range(C)]
    assert new[0]["reactivity"] == 100 and [p["reactivity"] for p in new[1:]] == [T + 1] * (C - 1)
    assert bank.get_state(0)[1] == sr.REFRESH_RATE and bank.get_state(1)[1] == T + 40
    ref.set_params(new)
    ref.updated(0)
    _, trace = _check(gpu, bank, ref, _signal(62, C, T + 3), what="after set_reactivity")
    assert ref.refreshes == [(0, False)] and bank.get_state(0)[1] == T + 3
    # a negative gain, and gain exactly 1 on a channel that had another
    bank.set_gain(0, -2.0)
    bank.set_gain(1, 1.0)
    bank.set_gain(2, 1.0)
    bank.update_settings()
    new = [bank.get_params(ch) for ch in range(C)]
    assert new[0]["gain"] == -2.0 and new[1]["gain"] == 1.0 and params[1]["gain"] == 0.5
    ref.set_params(new)
    got, _ = _check(gpu, bank, ref, _signal(63, C, T + 3), what="gains")
    # clear: fRmsValue, nRefresh and the ring to zero, the position stays
    head = _state(bank)["head"].copy()
    bank.clear(1)
    bank.update_settings()
    ref.clear(1)
    assert _same_state(bank, ref) and bank.get_state(1) == (0.0, 0, int(head[1])) and bank.get_state(0)[1] > 0
    _check(gpu, bank, ref, _signal(64, C, T + 3), what="after clear(1)")
    bank.clear()
    for ch in range(C):
        ref.clear(ch)
    _check(gpu, bank, ref, _signal(65, C, 2 * T), what="after clear()")
    bank.close()


def _stereo(seed, C, n):
    rng = np.random.default_rng(seed)
    a, b = rng.standard_normal((C, n)).astype(f32), rng.standard_normal((C, n)).astype(f32)
    b[:, 0:40] = -a[:, 0:40]                                   # l == -r, l == r, zeros of both signs: the tie rules
    b[:, 40:80] = a[:, 40:80]
    a[:, 80:90], b[:, 80:90] = 0.0, -0.0
    a[:, 90:100], b[:, 90:100] = -0.0, 0.0
    a[:, 100:110], b[:, 110:120] = 0.0, -0.0
    return a, b


@pytest.mark.gpu
@pytest.mark.parametrize("inputs", [1, 2])
def test_every_source_and_premix_then_process_premixed(gpu, inputs):
    combos = [(s, m) for m in (sr.SCSM_STEREO, sr.SCSM_MIDSIDE) for s in sr.SOURCES]
    C, n = len(combos), T + 130
    settings = [dict(sample_rate=RATE, reactivity=_ms(33), mode=sr.MODES[ch % 4], source=s, stereo_mode=m, gain=(1.0, -0.5)[ch % 2])
                for ch, (s, m) in enumerate(combos)]
    bank, params, ref = _bank(gpu, settings, inputs)
    assert [(p["source"], p["flags"] & 1) for p in params] == combos
    a, b = _stereo(71, C, n)
    b_in = b if inputs == 2 else None
    got, _ = _check(gpu, bank, ref, a, b_in, what="process")
    # premix: the signed source
    da, db, dm = gpu.DeviceBuffer.from_host(a), gpu.DeviceBuffer.from_host(b), gpu.DeviceBuffer((C, n))
    bank.premix(dm, da, db if inputs == 2 else None, n)
    mixed = dm.download()
    assert _bits_equal(mixed, ref.premix(a, b_in))
    if inputs == 2:
        assert np.any(mixed < 0) and np.any(np.signbit(mixed) & (mixed == 0))
        amin = combos.index((sr.SCS_AMIN, sr.SCSM_STEREO))
        assert _bits_equal(mixed[amin, :40], b[amin, :40])      # |l| == |r|: psmin3 takes r, psmax3 takes r as well
        amax = combos.index((sr.SCS_AMAX, sr.SCSM_STEREO))
        assert _bits_equal(mixed[amax, :40], b[amax, :40])
    else:
        assert _bits_equal(mixed, a)                            # one input: the source is not looked at
    # process == premix, then process_premixed, on a twin from the same state
    twin, _, _ = _bank(gpu, settings, inputs)
    out = gpu.DeviceBuffer((C, n))
    twin.process_premixed(out, dm, n)
    assert _bits_equal(out.download(), got) and _same_state(twin, ref)
    twin.process_premixed(dm, dm, n)                            # in place
    bank.process(da, da, db if inputs == 2 else None, n)
    assert _bits_equal(dm.download(), da.download())
    bank.close()
    twin.close()


@pytest.mark.gpu
@pytest.mark.parametrize("strides", [(301, 303, 307), (304, 312, 308), (300, 300, 300)])
def test_strides_and_unaligned_rows(gpu, strides):
    C, n = G + 1, T + 44
    os_, s0, s1 = strides
    settings = [dict(_settings(ch), source=sr.SOURCES[ch % 6]) for ch in range(C)]
    bank, params, ref = _bank(gpu, settings, 2)
    a, b = _stereo(81, C, n)
    pad = lambda v, s, fill: np.concatenate([v, np.full((C, s - n), fill, f32)], axis=1)
    ha, hb = pad(a, s0, 3.0), pad(b, s1, 5.0)
    da, db, do = gpu.DeviceBuffer.from_host(ha), gpu.DeviceBuffer.from_host(hb), gpu.DeviceBuffer((C, os_))
    do.upload(np.full((C, os_), 7.0, f32))
    bank.process(do, da, db, n, out_stride=os_, in0_stride=s0, in1_stride=s1)
    got = do.download()
    want, _ = ref.process(a, b)
    assert _bits_equal(got[:, :n], want) and np.all(got[:, n:] == 7.0), "written past count"
    assert np.array_equal(da.download(), ha) and np.array_equal(db.download(), hb), "an input was written"
    assert _same_state(bank, ref)
    bank.close()


@pytest.mark.gpu
def test_silence_and_in_place(gpu):
    C, n = G + 1, 2 * T + 9
    settings = [dict(_settings(ch), source=sr.SOURCES[ch % 6]) for ch in range(C)]
    a, b = _stereo(91, C, n)
    ref_bank, params, ref = _bank(gpu, settings, 2)
    want, _ = _check(gpu, ref_bank, ref, a, b, what="apart")
    for alias in (0, 1):
        bank, _, _ = _bank(gpu, settings, 2)
        da, db = gpu.DeviceBuffer.from_host(a), gpu.DeviceBuffer.from_host(b)
        bank.process((da, db)[alias], da, db, n)                # out == in0, out == in1
        assert _bits_equal((da, db)[alias].download(), want), alias
        assert np.array_equal((db, da)[alias].download(), (b, a)[alias])
        bank.close()
    # in0 == NULL: silence still runs through gain, ring and detector (the windows empty, the low-pass decays)
    got, trace = _check(gpu, ref_bank, ref, None, None, count=n, what="silence")
    assert np.any(trace != 0) and np.any(got != 0)
    one, _, ref1 = _bank(gpu, [_settings(ch) for ch in range(C)], 1)
    _check(gpu, one, ref1, None, None, count=T + 1, what="silence from a fresh bank")
    assert gpu.lib.mi_sidechain_bank_process(ref_bank.handle, ctypes.c_void_p(16), ctypes.c_void_p(16), None, 4, 4, 4, 4, None) == -1
    ref_bank.close()
    one.close()


@pytest.mark.gpu
def test_four_modes_in_one_workgroup(gpu):
    bank, params, ref = _bank(gpu, [_settings(ch, mode=sr.MODES[ch], n=(40, T + 1, 40, 40)[ch]) for ch in range(G)])
    assert [p["mode"] for p in params] == list(sr.MODES)
    for blk in range(3):
        _check(gpu, bank, ref, _signal(95 + blk, G, T + 77), what=blk)
    bank.close()


@pytest.mark.gpu
def test_low_pass_decays_into_subnormals(gpu):
    C, n = 2, 3 * T
    bank, params, ref = _bank(gpu, [dict(sample_rate=RATE, reactivity=_ms(1 + ch), mode=sr.SCM_LPF) for ch in range(C)])
    x = np.zeros((C, n), f32)
    x[:, :8] = 1.0
    got, trace = _check(gpu, bank, ref, x, what="decay")
    tiny = f32(1.1754944e-38)
    sub = (trace[0] > 0) & (trace[0] < tiny)
    assert sub.sum() > 10 and trace[0][trace[0] > 0].min() == f32(1.4e-45), "the restatement does not reach the smallest subnormal"
    assert _bits_equal(got, trace)                              # positive: the clamp passes them on
    bank.close()


@pytest.mark.gpu
def test_graph_capture_replays_direct_calls(gpu):
    C, n = 64, T + 100
    st = ctypes.c_void_p()
    gpu.check(gpu.lib.mi_dspu_stream_create(ctypes.byref(st)))
    settings = [_settings(ch) for ch in range(C)]
    bank, params, ref = _bank(gpu, settings)
    twin, _, _ = _bank(gpu, settings)
    x = _signal(70, C, 3 * n)
    d = [gpu.DeviceBuffer.from_host(x[:, i * n:(i + 1) * n]) for i in range(3)]
    o = [gpu.DeviceBuffer((C, n)) for _ in range(3)]
    gpu.check(gpu.lib.mi_dspu_graph_begin_capture(st))
    for i in range(3):
        bank.process(o[i], d[i], None, n, stream=st.value)
    exe = ctypes.c_void_p()
    gpu.check(gpu.lib.mi_dspu_graph_end_capture(st, ctypes.byref(exe)))
    t = [gpu.DeviceBuffer((C, n)) for _ in range(3)]
    for rep in range(3):
        gpu.check(gpu.lib.mi_dspu_graph_launch(exe, st))
        for i in range(3):
            twin.process(t[i], d[i], None, n, stream=st.value)
        got = np.concatenate([b.download(stream=st.value) for b in o], axis=1)
        direct = np.concatenate([b.download(stream=st.value) for b in t], axis=1)
        want, _ = ref.process(x)
        assert _bits_equal(got, direct) and _bits_equal(got, want), rep         # the state advances on every replay
        assert _same_state(bank, ref)
    gpu.lib.mi_dspu_graph_destroy(exe)
    bank.close()
    twin.close()
    gpu.check(gpu.lib.mi_dspu_stream_destroy(st))


@pytest.mark.gpu
def test_changed_setting_inside_a_capture_is_refused(gpu):
    """A setter leaves work to the next call.  On a capturing stream that call -- process() or update_settings() -- answers
    MI_ESTATE and names update_settings(), changes nothing on the device and leaves the capture valid; the next eager process()
    applies the setting to the ring and the state from before the capture."""
    C, n = 5, T + 100
    st = ctypes.c_void_p()
    gpu.check(gpu.lib.mi_dspu_stream_create(ctypes.byref(st)))
    bank, params, ref = _bank(gpu, [_settings(ch) for ch in range(C)])
    x0, x1 = _signal(80, C, n), _signal(81, C, n)
    d0, d1 = gpu.DeviceBuffer.from_host(x0), gpu.DeviceBuffer.from_host(x1)
    out = gpu.DeviceBuffer((C, n))
    bank.process(out, d0, None, n, stream=st.value)
    out0 = out.download(stream=st.value)
    assert _bits_equal(out0, ref.process(x0)[0])
    before = _state(bank)
    gpu.check(gpu.lib.mi_dspu_graph_begin_capture(st))
    bank.set_reactivity(0, _ms(100))
    bank.set_gain(1, -0.75)
    bank.set_mode(2, sr.SCM_UNIFORM)
    for call in (lambda: bank.process(out, d1, None, n, stream=st.value), lambda: bank.update_settings(stream=st.value)):
        with pytest.raises(gpu.MiError) as e:
            call()
        assert e.value.code == -5 and "update_settings" in str(e.value)
    gpu.check(gpu.lib.mi_dspu_memset(ctypes.c_void_p(out.ptr), 0, 16, st))         # (so that the capture is not empty)
    exe = ctypes.c_void_p()
    gpu.check(gpu.lib.mi_dspu_graph_end_capture(st, ctypes.byref(exe)))             # ends and instantiates normally
    assert exe.value
    gpu.lib.mi_dspu_graph_destroy(exe)
    # nothing changed on the device: the state, and the rows no refused call wrote to
    after = _state(bank)
    assert all(np.array_equal(after[k], before[k]) for k in before) and _same_state(bank, ref)
    assert _bits_equal(out.download(stream=st.value), out0)
    bank.process(out, d1, None, n, stream=st.value)
    new = [bank.get_params(ch) for ch in range(C)]
    assert new[0]["reactivity"] == 100 != params[0]["reactivity"] and new[1]["gain"] == f32(-0.75)
    assert new[2]["mode"] == sr.SCM_UNIFORM != params[2]["mode"]
    ref.set_mode(2, sr.SCM_UNIFORM)
    ref.set_params(new)
    ref.updated(0)
    assert _bits_equal(out.download(stream=st.value), ref.process(x1)[0])           # the ring and the state carried over
    assert _same_state(bank, ref)
    bank.close()
    gpu.check(gpu.lib.mi_dspu_stream_destroy(st))


@pytest.mark.gpu
def test_state_access_inside_a_capture_is_refused(gpu):
    """get_state() ends in a synchronisation, which a capturing stream does not allow: it answers MI_ESTATE with a message and
    leaves the capture valid -- a process() captured after it replays three times with the bits of an eager twin."""
    C, n = 5, T + 100
    st = ctypes.c_void_p()
    gpu.check(gpu.lib.mi_dspu_stream_create(ctypes.byref(st)))
    settings = [_settings(ch) for ch in range(C)]
    bank, params, ref = _bank(gpu, settings)
    twin, _, _ = _bank(gpu, settings)
    x = _signal(82, C, n)
    d = gpu.DeviceBuffer.from_host(x)
    o, t = gpu.DeviceBuffer((C, n)), gpu.DeviceBuffer((C, n))
    gpu.check(gpu.lib.mi_dspu_graph_begin_capture(st))
    with pytest.raises(gpu.MiError) as err:
        bank.get_state(2, stream=st.value)
    assert err.value.code == -5 and "captured" in str(err.value)
    bank.process(o, d, None, n, stream=st.value)
    exe = ctypes.c_void_p()
    gpu.check(gpu.lib.mi_dspu_graph_end_capture(st, ctypes.byref(exe)))
    for rep in range(3):
        gpu.check(gpu.lib.mi_dspu_graph_launch(exe, st))
        twin.process(t, d, None, n, stream=st.value)
        got, direct = o.download(stream=st.value), t.download(stream=st.value)
        assert _bits_equal(got, direct) and _bits_equal(got, ref.process(x)[0]), rep    # the state advances on every replay
    assert _same_state(bank, ref)                                                   # ... and can be read again after the capture
    gpu.lib.mi_dspu_graph_destroy(exe)
    bank.close()
    twin.close()
    gpu.check(gpu.lib.mi_dspu_stream_destroy(st))


@pytest.mark.gpu
def test_sidechain_feeds_the_compressor_on_the_device(gpu):
    C, n = G + 1, 3 * T + 7
    bank, params, ref = _bank(gpu, [_settings(ch, mode=(sr.SCM_RMS, sr.SCM_LPF, sr.SCM_PEAK, sr.SCM_UNIFORM)[ch % 4], n=48) for ch in range(C)])
    comp = gpu.CompressorBank(C)
    for ch in range(C):
        comp.configure(ch, **cr.channel_settings(ch))
    comp.update_settings()
    cp = [comp.get_params(ch) for ch in range(C)]
    x = _signal(77, C, n)
    audio = (np.random.default_rng(78).standard_normal((C, n)) * 0.5).astype(f32)
    dx, dsc, da, dout = gpu.DeviceBuffer.from_host(x), gpu.DeviceBuffer((C, n)), gpu.DeviceBuffer.from_host(audio), gpu.DeviceBuffer((C, n))
    denv, dgain = gpu.DeviceBuffer((C, n)), gpu.DeviceBuffer((C, n))
    twin = gpu.CompressorBank(C)
    for ch in range(C):
        twin.configure(ch, **cr.channel_settings(ch))
    bank.process(dsc, dx, None, n)                              # sidechain -> compressor, no host trip
    comp.process_apply(dout, da, dsc, n)
    twin.process(dgain, denv, dsc, n)                           # the same rows once more, for the envelope
    sc, _ = ref.process(x)
    assert _bits_equal(dsc.download(), sc)
    env, _ = cr.follow(sc, cr.fresh_state(C), [p["tau_attack"] for p in cp], [p["tau_release"] for p in cp],
                       [p["release_threshold"] for p in cp], [p["hold"] for p in cp])
    assert _bits_equal(denv.download(), env)
    gain = dgain.download()
    g64, bound = cr.gain64(env, cp), cr.gain_bound(env, cp)
    err = np.abs(gain.astype(np.float64) - g64) / np.abs(g64) / cr.U
    assert np.all(err <= bound), (err / bound).max()
    assert _bits_equal(dout.download(), audio * gain)
    for k in (bank, comp, twin):
        k.close()


CPP = r'''
#include <lsp-plug.in/dsp-units/util/Sidechain.h>
#include <mi_dspu.h>
#include <cstdio>
#include <cstring>
#include <vector>
using namespace lsp::dspu;
static const size_t N = 0x2000 + 600, BLOCK = 511, GUARD = 16;
static const float MARK = 12345.0f;
struct guarded                                                  // guard words around the samples
{
    std::vector<float> v;
    guarded(): v(N + 2 * GUARD, MARK) {}
    float *data() { return v.data() + GUARD; }
    bool intact() const { for (size_t i = 0; i < GUARD; ++i) if (v[i] != MARK || v[GUARD + N + i] != MARK) return false; return true; }
};
static void make_eq(Equalizer &eq)
{
    eq.init(1, 0);
    eq.set_mode(EQM_IIR);
    eq.set_sample_rate(48000);
    filter_params_t fp = { MI_FLT_BT_RLC_HIPASS, 1, 300.0f, 300.0f, 1.0f, 0.0f };
    eq.set_params(0, &fp);
}
int main(int argc, char **argv)
{
    static const sidechain_mode_t modes[] = { SCM_PEAK, SCM_LPF, SCM_RMS, SCM_UNIFORM };
    static const sidechain_source_t sources[] = { SCS_MIDDLE, SCS_SIDE, SCS_LEFT, SCS_RIGHT, SCS_AMIN, SCS_AMAX };
    static const sidechain_stereo_mode_t scmodes[] = { SCSM_STEREO, SCSM_MIDSIDE };
    guarded out, a, b;
    FILE *f = fopen(argv[1], "rb");
    if (fread(a.data(), sizeof(float), N, f) != N || fread(b.data(), sizeof(float), N, f) != N) return 2;
    fclose(f);
    f = fopen(argv[2], "wb");
    Sidechain sc;
    for (size_t channels = 1; channels <= 2; ++channels)       // the loop of the reference's unit test, blocks of 511
    {
        if (!sc.init(channels, 50.0f)) return 3;
        sc.set_sample_rate(48000);
        sc.set_reactivity(20.0f);
        for (size_t mode = 0; mode < 4; ++mode)
        {
            sc.set_mode(modes[mode]);
            for (size_t source = 0; source < 6; ++source)
            {
                sc.set_source(sources[source]);
                for (size_t scmode = 0; scmode < 2; ++scmode)
                {
                    sc.set_stereo_mode(scmodes[scmode]);
                    const float *src[2] = { a.data(), b.data() };
                    float *dst = out.data();
                    for (size_t i = 0; i < N; )
                    {
                        const size_t count = (N - i < BLOCK) ? N - i : BLOCK;
                        sc.process(dst, src, count);
                        dst += count; src[0] += count; src[1] += count; i += count;
                    }
                    if (!out.intact() || !a.intact() || !b.intact()) return 4;
                    fwrite(out.data(), sizeof(float), N, f);
                }
            }
        }
    }
    // the single-sample form: one sample through the block path
    sc.set_mode(SCM_RMS);
    for (size_t i = 0; i < 8; ++i)
    {
        const float in[2] = { a.data()[i], b.data()[i] };
        out.data()[i] = sc.process(in);
    }
    fwrite(out.data(), sizeof(float), 8, f);
    sc.destroy();

    // a pre-equalizer: the class against premix -> a second identical equalizer -> process_premixed
    Equalizer eq1, eq2;
    make_eq(eq1);
    make_eq(eq2);
    Sidechain se;
    se.init(2, 50.0f);
    se.set_sample_rate(48000);
    se.set_reactivity(20.0f);
    se.set_source(SCS_AMIN);
    se.set_pre_equalizer(&eq1);
    const size_t M = 3 * BLOCK;
    const float *src[2] = { a.data(), b.data() };
    for (size_t i = 0; i < M; i += BLOCK)
    {
        const float *s[2] = { src[0] + i, src[1] + i };
        se.process(out.data() + i, s, BLOCK);
    }
    fwrite(out.data(), sizeof(float), M, f);
    mi_sidechain_bank_t *bank = NULL;
    float *d = NULL;
    std::vector<float> h(M);
    if (mi_sidechain_bank_create(&bank, 1, 2, 50.0f) != MI_OK || mi_dspu_malloc((void **)&d, 3 * M * sizeof(float)) != MI_OK) return 5;
    mi_sidechain_bank_set_sample_rate(bank, 0, 48000);
    mi_sidechain_bank_set_reactivity(bank, 0, 20.0f);
    mi_sidechain_bank_set_source(bank, 0, MI_SCS_AMIN);
    mi_dspu_copy_h2d(d, a.data(), M * sizeof(float), NULL);
    mi_dspu_copy_h2d(d + M, b.data(), M * sizeof(float), NULL);
    for (size_t i = 0; i < M; i += BLOCK)
    {
        if (mi_sidechain_bank_premix(bank, d + 2 * M + i, d + i, d + M + i, BLOCK, BLOCK, BLOCK, BLOCK, NULL) != MI_OK) return 6;
        mi_dspu_copy_d2h(h.data() + i, d + 2 * M + i, BLOCK * sizeof(float), NULL);
        eq2.process(h.data() + i, h.data() + i, BLOCK);
        mi_dspu_copy_h2d(d + 2 * M + i, h.data() + i, BLOCK * sizeof(float), NULL);
        if (mi_sidechain_bank_process_premixed(bank, d + 2 * M + i, d + 2 * M + i, BLOCK, BLOCK, BLOCK, NULL) != MI_OK) return 7;
    }
    mi_dspu_copy_d2h(h.data(), d + 2 * M, M * sizeof(float), NULL);
    fwrite(h.data(), sizeof(float), M, f);
    fclose(f);
    mi_dspu_free(d);
    mi_sidechain_bank_destroy(bank);
    se.destroy();
    eq1.destroy();
    eq2.destroy();
    return 0;
}
'''


@pytest.mark.gpu
def test_cpp_class_on_the_device(gpu, tmp_path):
    src, exe = str(tmp_path / "sc.cpp"), str(tmp_path / "sc")
    open(src, "w").write(CPP)
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-I" + os.path.join(PKG, "include"), "-I" + os.path.join(ROOT, "include"), src,
                           "-o", exe, "-L" + PKG, "-lmi_dspu", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    n = sr.REFRESH_RATE + 600
    rng = np.random.default_rng(60)
    ab = (rng.random((2, n)) * np.where(rng.random((2, n)) < 0.5, -1.0, 1.0)).astype(f32)      # randomize_sign
    ab.tofile(str(tmp_path / "in.bin"))
    out = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out
    r = np.fromfile(str(tmp_path / "out.bin"), f32)
    m = 3 * 511
    assert r.size == 96 * n + 8 + 2 * m
    # Every pass of the loop starts from a cleared sidechain (the stereo mode changes every time) whose ring stands where the
    # samples so far left it: 48 independent channels per number of inputs, one vectorised run each.
    p = gpu.SidechainBank.compute_params(48000, 50.0, 20.0)
    modes = (sr.SCM_PEAK, sr.SCM_LPF, sr.SCM_RMS, sr.SCM_UNIFORM)
    combos = [(mo, so, st) for mo in modes for so in sr.SOURCES for st in (sr.SCSM_STEREO, sr.SCSM_MIDSIDE)]
    last = None
    for inputs in (1, 2):
        params = [dict(p, mode=mo, source=so, flags=st) for mo, so, st in combos]
        ref = sr.Sidechains(params, inputs)
        ref.head = (np.arange(48, dtype=np.int64) * n) % p["capacity"]
        want, _ = ref.process(np.tile(ab[0], (48, 1)), np.tile(ab[1], (48, 1)))
        got = r[(inputs - 1) * 48 * n:inputs * 48 * n].reshape(48, n)
        bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
        assert bad.size == 0, (inputs, len(bad), bad[:4].tolist())
        last = ref
    # the eight single samples follow the last pass (UNIFORM, AMAX, mid-side) after set_mode(RMS): fRmsValue zeroed, no clear
    tail = sr.Sidechains([dict(p, mode=sr.SCM_RMS, source=sr.SCS_AMAX, flags=1)], 2)
    tail.ring[0], tail.head[0], tail.refresh[0] = last.ring[47], last.head[47], last.refresh[47]
    want, _ = tail.process(ab[0:1, :8], ab[1:2, :8])
    assert _bits_equal(r[96 * n:96 * n + 8], want[0])
    cls, capi = r[96 * n + 8:96 * n + 8 + m], r[96 * n + 8 + m:]
    assert _bits_equal(cls, capi) and np.any(cls > 0)
    plain = sr.Sidechains([dict(p, mode=sr.SCM_RMS, source=sr.SCS_AMIN, flags=0)], 2).process(ab[0:1, :m], ab[1:2, :m])[0][0]
    assert not _bits_equal(cls, plain)                          # the equalizer was in the path


@pytest.mark.gpu
def test_full_size_every_channel(gpu):
    C, n = 1024, 4096
    lengths = (1, 40, T - 1, T, T + 1, 2400)
    settings = [dict(sample_rate=48000, reactivity=50.0 if lengths[ch % 6] == 2400 else (lengths[ch % 6] + 0.5) / 48.0,
                     mode=sr.MODES[(ch // 6) % 4], gain=(1.0, 0.5, -1.5)[ch % 3]) for ch in range(C)]
    bank, params, ref = _bank(gpu, settings, max_ms=50.0)
    assert {p["reactivity"] for p in params} == set(lengths) and {p["mode"] for p in params} == set(sr.MODES)
    _check(gpu, bank, ref, _signal(99, C, n), what="1024 x 4096")
    bank.close()
