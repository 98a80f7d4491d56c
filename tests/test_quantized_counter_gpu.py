"""mi_qcounter_bank on the device against tests/quantized_counter_ref.py and the reference's recorded cases, bit for bit in every
counter, ring word, nHead and nCount: every recorded case through the C ABI (each process() as ONE call, whatever its length), 1, 3
and 70 channels with parameters and pending flags of their own in one launch, the LDS histogram and the global-atomic path on the
same inputs, the wave-level combining against its absence, a stream of its own, captured graphs that count at every replay and
recount at the first only, get_state / set_state, every misuse code, and the C++ class over the recorded cases."""
import ctypes

import numpy as np
import pytest

import quantized_counter_ref as Q
import test_quantized_counter_host as H
import test_quantized_counter_class_host as CH

gen = H.gen
f32, u32 = np.float32, np.uint32
EINVAL, ESTATE = -1, -5
LDS_WORDS = 8192                                # the kernel's budget: nLevels + 2 words of LDS at the most
GUARD = f32(-1234.5)


def words_of(bank, ch, stream=None):
    """counters, nHead, nCount, nPeriod, nLevels, fMinValue, fMaxValue, fRStep, bUpdate, as the restatement's settings_words()"""
    s, p = bank.get_state(ch, stream), bank.get_params(ch)
    tail = np.array([s["head"], s["count"], p["period"], p["levels"], 0, 0, 0, int(p["update"])], u32)
    tail[4:7] = np.array([p["min_value"], p["max_value"], p["rstep"]], f32).view(u32)
    return np.concatenate([s["counters"], tail]), s["ring"].view(u32)


def check(bank, refs, what="", stream=None):
    for ch, q in enumerate(refs):
        got, ring = words_of(bank, ch, stream)
        want = q.settings_words()
        assert np.array_equal(got, want), (what, ch, np.flatnonzero(got != want)[:6], got[-8:], want[-8:])
        assert np.array_equal(ring, q.history.view(u32)), (what, ch, "ring", np.flatnonzero(ring != q.history.view(u32))[:4])


def _stream(gpu):
    st = ctypes.c_void_p()
    gpu.check(gpu.lib.mi_dspu_stream_create(ctypes.byref(st)))
    return st


# ---- every recorded case ------------------------------------------------------------------------------------------------------
CHUNK = 18


@pytest.fixture(scope="module")
def xdev(gpu):
    buf = gpu.DeviceBuffer.from_host(H.X)
    yield buf
    buf.free()


def run_case(gpu, xbuf, c):
    n_row = H.X.shape[1]
    bank = gpu.QuantizedCounterBank(1, c["max_period"], c["max_levels"])
    for k, (code, row, off, n, a, b) in enumerate(c["ops"]):
        code, n = int(code), int(n)
        if code == Q.SET_PERIOD:
            bank.set_period(0, n)
        elif code == Q.SET_LEVELS:
            bank.set_levels(0, n)
        elif code == Q.SET_MIN:
            bank.set_min_value(0, a)
        elif code == Q.SET_MAX:
            bank.set_max_value(0, a)
        elif code == Q.SET_VALUE_RANGE:
            bank.set_value_range(0, a, b)
        elif code == Q.SET_RANGE:
            bank.set_range(0, a, b, n)
        elif code == Q.UPDATE:
            bank.update_settings()
        elif code == Q.CLEAR:
            bank.clear(0)
        elif code == Q.PROCESS:
            bank.process(xbuf.ptr + 4 * (int(row) * n_row + int(off)), n)
        got, ring = words_of(bank, 0)
        assert np.array_equal(got, c["words"][k]), (c["name"], k, Q.OP_NAMES[code], np.flatnonzero(got != c["words"][k])[:6], got[-8:], c["words"][k][-8:])
    assert np.array_equal(ring, c["ring"]), (c["name"], "ring", np.flatnonzero(ring != c["ring"])[:4])
    bank.close()


@pytest.mark.gpu
@pytest.mark.parametrize("part", range((len(H.PLAIN) + CHUNK - 1) // CHUNK))
def test_every_recorded_case(gpu, xdev, part):
    for c in H.PLAIN[part * CHUNK:(part + 1) * CHUNK]:
        run_case(gpu, xdev, c)


# ---- many channels ------------------------------------------------------------------------------------------------------------
RANGES = ((-1.0, 1.0), (-0.5, 0.25), (0.0, 2.4e-38), (1.0, -1.0), (0.3, 0.3), (-1e30, 1e30))


def rows(channels, n, seed):
    """Uniform rows; every third channel constant, every fourth two-valued, every fifth sorted, the specials in front of every seventh."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1.3, 1.3, (channels, n)).astype(f32)
    x[2::3] = f32(0.3)
    x[3::4] = np.where(rng.integers(0, 2, x[3::4].shape) == 0, f32(-0.6), f32(0.3))
    x[4::5] = np.sort(x[4::5], axis=1)
    k = min(n, 14)
    x[::7, :k] = H.X[gen.ROW_SPECIAL, :k]
    x[5::6] *= f32(1e-38)
    return x


class Unit:
    """A bank and the restatement's counters: channel ch has a period, a level count and a range of its own."""

    def __init__(self, gpu, channels, max_period=600, max_levels=64, first=0):
        self.bank = gpu.QuantizedCounterBank(channels, max_period, max_levels)
        self.refs = []
        for ch in range(channels):
            k = ch + first
            q = Q.QuantizedCounter(max_period, max_levels)
            lo, hi = RANGES[k % len(RANGES)]
            levels, period = (1, 8, 16, 37, max_levels)[k % 5], (1, 7, 100, 500, max_period)[(k // 2) % 5]
            for unit in (q, _Channel(self.bank, ch)):
                unit.set_range(lo, hi, levels)
                unit.set_period(period)
            self.refs.append(q)

    def each(self, ch):
        return (self.refs[ch], _Channel(self.bank, ch))

    def close(self):
        self.bank.close()


class _Channel:
    """One channel of a bank with the restatement's setter names."""

    def __init__(self, bank, ch):
        self.bank, self.ch = bank, ch

    def __getattr__(self, name):
        return lambda *args: getattr(self.bank, name)(self.ch, *args)


@pytest.mark.gpu
@pytest.mark.parametrize("channels", (1, 3, 70))
def test_channels_with_settings_and_pending_flags_of_their_own(gpu, channels):
    u = Unit(gpu, channels)
    stride = 4096 + 5
    for step, n in enumerate((257, 4096, 0, 1025, 3, 700)):
        x = rows(channels, max(n, 1), 10 * channels + step)[:, :n]
        flat = np.full((channels, stride), GUARD, f32)
        flat[:, :n] = x
        buf = gpu.DeviceBuffer.from_host(np.concatenate([[GUARD], flat.reshape(-1)]))       # rows 4 bytes off the grid, an odd stride
        # between the calls: some channels change their range (pending), some their period, some nothing, some are cleared
        for ch in range(channels):
            for unit in u.each(ch):
                if (ch + step) % 3 == 0:
                    unit.set_value_range(*RANGES[(ch + step) % len(RANGES)])
                if (ch + step) % 4 == 1:
                    unit.set_period((3, 50, 600)[(ch + step) % 3])
                if (ch + step) % 5 == 2:
                    unit.set_levels((5, 64)[step % 2])
            if (ch + step) % 11 == 3:
                u.refs[ch].clear(), u.bank.clear(ch)
        pending = [q.update for q in u.refs]
        assert channels != 70 or step == 0 or (any(pending) and not all(pending)), "the launch mixes pending and settled channels"
        assert [u.bank.needs_update(ch) for ch in range(channels)] == pending
        u.bank.process(buf.ptr + 4, n, stride=stride)
        for ch, q in enumerate(u.refs):
            q.process(x[ch])
        check(u.bank, u.refs, (step, n))
        assert (buf.download()[1:].reshape(channels, stride)[:, n:] == GUARD).all()
        buf.free()
    u.close()


@pytest.mark.gpu
def test_explicit_update_settings_of_some_channels(gpu):
    """update_settings() recounts the channels whose bUpdate is set over ALL the samples they hold, those beyond a period that was
    reduced included, and touches no other channel."""
    u = Unit(gpu, 5, first=2)
    x = rows(5, 600, 77)
    buf = gpu.DeviceBuffer.from_host(x)
    u.bank.process(buf, 600)
    for ch, q in enumerate(u.refs):
        q.process(x[ch])
        for unit in u.each(ch):
            unit.set_period(1)
            if ch % 2 == 0:
                unit.set_range(-1.3, 1.3, 9)
    u.bank.update_settings()
    for q in u.refs:
        q.update_settings()
    check(u.bank, u.refs, "update_settings")
    assert any(q.count > q.period for q in u.refs)
    u.bank.update_settings()                                        # nothing pending: nothing happens
    check(u.bank, u.refs, "again")
    u.bank.process(buf, 2, stride=600)
    for ch, q in enumerate(u.refs):
        q.process(x[ch, :2])
    check(u.bank, u.refs, "process")
    buf.free()
    u.close()


# ---- the two histogram paths --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ("uniform", "constant", "sorted"))
def test_lds_and_global_atomic_paths_on_the_same_inputs(gpu, kind):
    """nLevels + 2 words fit the LDS budget with nLevels = LDS_WORDS - 2 and do not with one more; rows of 300 samples.  Both banks
    also run a small level count (always LDS) as their second channel."""
    n = 300
    x = rows(2, 3 * n, 5)
    if kind == "constant":
        x[:] = f32(0.3)
    elif kind == "sorted":
        x = np.sort(x, axis=1)
    buf = gpu.DeviceBuffer.from_host(x)
    for levels in (LDS_WORDS - 2, LDS_WORDS - 1):
        bank = gpu.QuantizedCounterBank(2, 400, levels)
        refs = [Q.QuantizedCounter(400, levels), Q.QuantizedCounter(400, levels)]
        for ch, (q, lv) in enumerate(zip(refs, (levels, 8))):
            for unit in (q, _Channel(bank, ch)):
                unit.set_range(-1.3, 1.3, lv)
                unit.set_period(400)
        for step in range(3):
            if step == 2:                                           # a pending recount on both paths
                for ch in range(2):
                    for unit in (refs[ch], _Channel(bank, ch)):
                        unit.set_value_range(-1.0, 1.2)
            bank.process(buf.ptr + 4 * step * n, n, stride=3 * n)
            for ch, q in enumerate(refs):
                q.process(x[ch, step * n:(step + 1) * n])
            check(bank, refs, (levels, step))
        assert refs[0].counters[:levels].max() >= 1 and refs[0].count == 400
        bank.close()
    buf.free()


@pytest.mark.gpu
def test_wave_combining_changes_nothing(gpu):
    x = rows(12, 4096, 9)
    buf = gpu.DeviceBuffer.from_host(x)
    states = []
    for on in (True, False):
        u = Unit(gpu, 12, max_period=5000)
        u.bank.set_wave_combining(on)
        for n in (4096, 1000):
            u.bank.process(buf, n, stride=4096)
            for ch, q in enumerate(u.refs):
                q.process(x[ch, :n])
        check(u.bank, u.refs, on)
        states.append([words_of(u.bank, ch)[0] for ch in range(12)])
        u.close()
    assert all(np.array_equal(a, b) for a, b in zip(*states))
    buf.free()


# ---- read ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_read_gives_bins_below_and_above_of_every_channel(gpu):
    u = Unit(gpu, 7)
    x = rows(7, 900, 21)
    buf = gpu.DeviceBuffer.from_host(x)
    u.bank.process(buf, 900)
    most = max(q.levels for q in u.refs)
    stride = most + 2 + 3
    out = gpu.DeviceBuffer.from_host(np.full((7, stride), GUARD, f32))
    u.bank.read(out, stride)
    got = out.download()
    for ch, q in enumerate(u.refs):
        q.process(x[ch])
        want = np.concatenate([q.counters[:most], q.counters[q.max_levels:]])
        assert np.array_equal(got[ch, :most + 2].view(u32), want), ch
        assert (got[ch, most + 2:] == GUARD).all()
    buf.free(), out.free()
    u.close()


# ---- streams and graphs ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_process_on_a_stream_of_its_own(gpu):
    st = _stream(gpu)
    u = Unit(gpu, 3, first=1)
    for k, n in enumerate((1025, 65, 4096)):
        x = rows(3, n, 40 + k)
        buf = gpu.DeviceBuffer.from_host(x, st.value)
        u.bank.process(buf, n, stream=st.value)
        for ch, q in enumerate(u.refs):
            q.process(x[ch])
        check(u.bank, u.refs, k, st.value)
        gpu.check(gpu.lib.mi_dspu_stream_synchronize(st))
        buf.free()
    u.close()
    gpu.check(gpu.lib.mi_dspu_stream_destroy(st))


@pytest.mark.gpu
@pytest.mark.parametrize("pending", (False, True))
def test_captured_process_counts_at_every_replay(gpu, pending):
    """The kernel keeps nHead, nCount and the serial of the settings that the counters hold on the device: three replays are three
    plain calls, and a range change that was pending at the capture recounts at the first replay only."""
    n = 700
    st = _stream(gpu)
    u = Unit(gpu, 3, first=2)
    x = rows(3, n, 88)
    buf = gpu.DeviceBuffer.from_host(x, st.value)
    out = gpu.DeviceBuffer.from_host(np.full((3, 70), GUARD, f32), st.value)
    u.bank.process(buf, 300, stride=n, stream=st.value)
    for ch, q in enumerate(u.refs):
        q.process(x[ch, :300])
    if pending:
        for unit in u.each(1):
            unit.set_value_range(-0.2, 0.9)
        # changed settings are sent outside a capture only
        gpu.check(gpu.lib.mi_dspu_graph_begin_capture(st))
        with pytest.raises(gpu.MiError) as e:
            u.bank.process(buf, n, stream=st.value)
        assert e.value.code == ESTATE
        exe = ctypes.c_void_p()
        gpu.check(gpu.lib.mi_dspu_graph_end_capture(st, ctypes.byref(exe)))
        gpu.lib.mi_dspu_graph_destroy(exe)
        u.bank.read(out, 70, stream=st.value)                       # sends them, recounts nothing
        assert u.bank.needs_update(1) and not u.bank.needs_update(0)
        check(u.bank, u.refs, "before the capture", st.value)
    exe = ctypes.c_void_p()
    gpu.check(gpu.lib.mi_dspu_graph_begin_capture(st))
    u.bank.process(buf, n, stream=st.value)
    u.bank.read(out, 70, stream=st.value)
    gpu.check(gpu.lib.mi_dspu_graph_end_capture(st, ctypes.byref(exe)))
    assert exe.value
    for rep in range(3):
        gpu.check(gpu.lib.mi_dspu_graph_launch(exe, st))
        got = out.download(st.value)
        for ch, q in enumerate(u.refs):
            q.process(x[ch])
            assert np.array_equal(got[ch, :66].view(u32), np.concatenate([q.counters[:64], q.counters[64:]])), (rep, ch)
        check(u.bank, u.refs, rep, st.value)
    gpu.lib.mi_dspu_graph_destroy(exe)
    buf.free(), out.free()
    u.close()
    gpu.check(gpu.lib.mi_dspu_stream_destroy(st))


# ---- state ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_get_state_and_set_state_round_trip(gpu):
    u, v = Unit(gpu, 2, first=3), Unit(gpu, 2, first=3)
    x = rows(2, 1500, 4)
    buf = gpu.DeviceBuffer.from_host(x)
    u.bank.process(buf, 1000, stride=1500)
    v.bank.update_settings()
    for ch in range(2):
        s = u.bank.get_state(ch)
        assert s["capacity"] == Q.capacity_of(600) and len(s["ring"]) == s["capacity"] and len(s["counters"]) == 66
        v.bank.set_state(ch, s["head"], s["count"], s["ring"], s["counters"])
        u.refs[ch].process(x[ch, :1000])
    check(v.bank, u.refs, "set_state")
    for bank in (u.bank, v.bank):
        bank.process(buf.ptr + 4 * 1000, 500, stride=1500)
    for ch in range(2):
        u.refs[ch].process(x[ch, 1000:])
    check(u.bank, u.refs, "u")
    check(v.bank, u.refs, "v")
    buf.free()
    u.close(), v.close()


# ---- misuse -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_misuse(gpu):
    lib = gpu.lib
    u = Unit(gpu, 3)
    h = u.bank.handle
    ones = gpu.DeviceBuffer.from_host(np.ones((3, 128), f32))
    p = ctypes.c_void_p(ones.ptr)
    made = ctypes.c_void_p()
    from importlib import import_module
    capi = import_module("lsp-dsp-units_amd.capi")
    state, params, flag = capi.QuantizedCounterState(0, 0, 0), capi.QuantizedCounterParams(), ctypes.c_int()
    cap = Q.capacity_of(600)
    for code, what in ((lib.mi_qcounter_bank_set_period(h, 3, 5), "channel"), (lib.mi_qcounter_bank_set_levels(h, 3, 5), "channel"),
                       (lib.mi_qcounter_bank_set_min_value(h, 3, 0.0), "channel"), (lib.mi_qcounter_bank_set_max_value(h, 3, 0.0), "channel"),
                       (lib.mi_qcounter_bank_set_value_range(h, 3, 0.0, 1.0), "channel"), (lib.mi_qcounter_bank_set_range(h, 3, 0.0, 1.0, 4), "channel"),
                       (lib.mi_qcounter_bank_clear(h, 3), "channel"), (lib.mi_qcounter_bank_needs_update(h, 3, ctypes.byref(flag)), "channel"),
                       (lib.mi_qcounter_bank_needs_update(h, 0, None), "no result"),
                       (lib.mi_qcounter_bank_get_params(h, 3, ctypes.byref(params)), "channel"), (lib.mi_qcounter_bank_get_params(h, 0, None), "no result"),
                       (lib.mi_qcounter_bank_get_state(h, 3, ctypes.byref(state), None, None, None), "channel"),
                       (lib.mi_qcounter_bank_get_state(h, 0, None, None, None, None), "no result"),
                       (lib.mi_qcounter_bank_set_state(h, 3, ctypes.byref(state), None, None, None), "channel"),
                       (lib.mi_qcounter_bank_set_state(h, 0, None, None, None, None), "no state"),
                       (lib.mi_qcounter_bank_set_state(h, 0, ctypes.byref(capi.QuantizedCounterState(cap, 0, 0)), None, None, None), "head outside the ring"),
                       (lib.mi_qcounter_bank_set_state(h, 0, ctypes.byref(capi.QuantizedCounterState(0, cap + 1, 0)), None, None, None), "count above the ring"),
                       (lib.mi_qcounter_bank_process(h, None, 64, 128, None), "no src"),
                       (lib.mi_qcounter_bank_process(h, p, 64, 63, None), "a stride shorter than the count"),
                       (lib.mi_qcounter_bank_process(h, p, 1 << 31, 1 << 31, None), "count"),
                       (lib.mi_qcounter_bank_read(h, None, 66, None), "no dst"), (lib.mi_qcounter_bank_read(h, p, 17, None), "a stride shorter than the 16 + 2 words of a row"),
                       (lib.mi_qcounter_bank_create(None, 3, 16, 4), "no result"),
                       (lib.mi_qcounter_bank_create(ctypes.byref(made), 0, 16, 4), "no channels"),
                       (lib.mi_qcounter_bank_create(ctypes.byref(made), 3, 0, 4), "max_period 0"),
                       (lib.mi_qcounter_bank_create(ctypes.byref(made), 3, 16, 0), "max_levels 0"),
                       (lib.mi_qcounter_bank_create(ctypes.byref(made), 3, 16, (1 << 24) + 1), "too many levels"),
                       (lib.mi_qcounter_bank_create(ctypes.byref(made), 3, (1 << 32) - 1024, 4), "a capacity beyond 32 bits"),
                       (lib.mi_qcounter_bank_create(ctypes.byref(made), 3, 1 << 33, 4), "a capacity beyond 32 bits")):
        assert code == EINVAL, (what, code)
        assert lib.mi_dspu_last_error().decode().startswith("mi_qcounter_"), (what, lib.mi_dspu_last_error())
    assert made.value is None
    assert (ones.download() == 1.0).all(), "a refused call wrote"
    # the refusals changed nothing: the bank runs as it was set up
    u.bank.process(ones, 128)
    for q in u.refs:
        q.process(np.ones(128, f32))
    check(u.bank, u.refs, "after the refusals")
    # process before a period and levels were ever set
    fresh = gpu.QuantizedCounterBank(2, 100, 8)
    fresh.set_range(0, -1.0, 1.0, 8), fresh.set_period(0, 50)
    for prepare in (lambda: None, lambda: fresh.set_period(1, 50), lambda: fresh.set_levels(1, 4)):
        prepare()
        with pytest.raises(gpu.MiError) as e:
            fresh.process(ones, 64, stride=128)
        assert e.value.code == ESTATE and lib.mi_dspu_last_error().decode().startswith("mi_qcounter_bank_process: channel 1")
        fresh.close()
        fresh = gpu.QuantizedCounterBank(2, 100, 8)
        fresh.set_range(0, -1.0, 1.0, 8), fresh.set_period(0, 50)
    with pytest.raises(gpu.MiError) as e:
        fresh.update_settings()                                     # channel 1 is pending and has no levels
    assert e.value.code == ESTATE
    s = fresh.get_state(0)
    assert s["head"] == 0 and s["count"] == 0 and not s["counters"].any() and not s["ring"].any()
    fresh.close()
    for entry in (lambda: lib.mi_qcounter_bank_process(None, p, 64, 64, None), lambda: lib.mi_qcounter_bank_read(None, p, 66, None),
                  lambda: lib.mi_qcounter_bank_set_period(None, 0, 5), lambda: lib.mi_qcounter_bank_set_levels(None, 0, 5),
                  lambda: lib.mi_qcounter_bank_set_min_value(None, 0, 0.0), lambda: lib.mi_qcounter_bank_set_max_value(None, 0, 0.0),
                  lambda: lib.mi_qcounter_bank_set_value_range(None, 0, 0.0, 1.0), lambda: lib.mi_qcounter_bank_set_range(None, 0, 0.0, 1.0, 4),
                  lambda: lib.mi_qcounter_bank_clear(None, 0), lambda: lib.mi_qcounter_bank_needs_update(None, 0, ctypes.byref(flag)),
                  lambda: lib.mi_qcounter_bank_update_settings(None, None), lambda: lib.mi_qcounter_bank_get_params(None, 0, ctypes.byref(params)),
                  lambda: lib.mi_qcounter_bank_get_state(None, 0, ctypes.byref(state), None, None, None),
                  lambda: lib.mi_qcounter_bank_set_state(None, 0, ctypes.byref(state), None, None, None),
                  lambda: lib.mi_qcounter_bank_set_wave_combining(None, 1)):
        assert entry() == ESTATE
    # get_state and set_state synchronise: not on a stream that is being captured; neither is a pending clear sent there
    st = _stream(gpu)
    gpu.check(gpu.lib.mi_dspu_graph_begin_capture(st))
    assert lib.mi_qcounter_bank_get_state(h, 0, ctypes.byref(state), None, None, st) == ESTATE
    assert lib.mi_qcounter_bank_set_state(h, 0, ctypes.byref(state), None, None, st) == ESTATE
    u.bank.clear(0)
    assert lib.mi_qcounter_bank_process(h, p, 64, 128, st) == ESTATE and lib.mi_qcounter_bank_update_settings(h, st) == ESTATE
    exe = ctypes.c_void_p()
    gpu.check(gpu.lib.mi_dspu_graph_end_capture(st, ctypes.byref(exe)))
    gpu.lib.mi_dspu_graph_destroy(exe)
    gpu.check(gpu.lib.mi_dspu_stream_destroy(st))
    u.close()
    with pytest.raises(gpu.MiError) as e:
        u.bank.process(ones, 64)
    assert e.value.code == ESTATE
    u.close()                                                       # twice is fine
    assert lib.mi_qcounter_bank_destroy(None) == 0
    ones.free()


# ---- the class ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("part", range(3))
def test_the_cpp_class_over_the_recorded_cases(gpu, tmp_path, part):
    """tests/cpp/quantized_counter_layout.cpp with the generator's protocol: lsp::dspu::QuantizedCounter of this library on every
    recorded case, each process() as one call."""
    exe = CH.compile_program(str(tmp_path / "quantized_counter_layout"))
    cases = H.PLAIN[part::3]
    got = gen.run(exe, H.X, cases, str(tmp_path))
    for c, r in zip(cases, got):
        bad = np.argwhere(r["words"] != c["words"])
        assert bad.size == 0, (c["name"], "operation %d, word %d of %d" % (bad[0][0], bad[0][1], c["max_levels"] + 10), c["ops"][bad[0][0]])
        assert np.array_equal(r["ring"], c["ring"]), c["name"]


@pytest.mark.gpu
def test_the_class_against_the_bank(gpu, tmp_path):
    """The class and a bank of one channel on a stream of operations of their own: the class's words are the bank's."""
    rng = np.random.default_rng(12)
    x = np.zeros_like(H.X)
    x[0] = rng.uniform(-2.0, 2.0, x.shape[1]).astype(f32)
    ops = [(Q.SET_RANGE, 0, 0, 40, -1.5, 1.5), (Q.SET_PERIOD, 0, 0, 777)]
    at = 0
    for n in (4000, 100, 0, 2049, 1, 4096):
        ops += [(Q.PROCESS, 0, at % 5, n), (Q.SET_VALUE_RANGE, 0, 0, 0, -1.0 - 0.1 * (at % 3), 1.5), (Q.SET_PERIOD, 0, 0, 300 + 100 * (at % 4))]
        at += 1
        if at == 3:
            ops += [(Q.UPDATE,), (Q.CLEAR,)]
    rows6 = np.zeros((len(ops), 6))
    for i, op in enumerate(ops):
        rows6[i, :len(op)] = op
    case = dict(name="class against bank", max_period=900, max_levels=48, ops=rows6)
    exe = CH.compile_program(str(tmp_path / "quantized_counter_layout"))
    got = gen.run(exe, x, [case], str(tmp_path))[0]
    xbuf = gpu.DeviceBuffer.from_host(x)
    case["words"], case["ring"] = got["words"], got["ring"]
    run_case(gpu, xbuf, case)                                       # x has the recorded rows' length
    assert got["words"][-1][:50].sum() == got["words"][-1][51] > 0
    xbuf.free()
