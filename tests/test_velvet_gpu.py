"""mi_velvet_bank on the device: every recorded reference case through a bank of one channel, bit for bit with the state words; banks
of several channels with different settings in one launch; counts around the batch, tile and segment sizes; the 256-sample
segmentation of a call with a source; later-wins collisions; strides and in place; states in and out; what the bank defines where
the reference does not; capture, streams, lifetime; and the lsp::dspu::Velvet class on host rows."""
import ctypes
import gc
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import noise_ref as R
import velvet_ref as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_velvet_vectors as gen  # noqa: E402

f32, u32, u64 = np.float32, np.uint32, np.uint64
EINVAL, ESTATE = -1, -5
OVERWRITE, ADD, MUL = 0, 1, 2
KIND = {R.P_OVERWRITE: OVERWRITE, R.P_ADD: ADD, R.P_ADD_INPLACE: ADD, R.P_MUL: MUL, R.P_MUL_INPLACE: MUL, V.P_ADD_NULL: ADD, V.P_MUL_NULL: MUL}
PKG = os.path.join(ROOT, "lsp-dsp-units_amd")


@pytest.fixture(scope="module")
def recorded():
    return gen.load()


def words(bank, ch=0):
    s = bank.get_state(ch)
    r, m = s.rand, s.mls
    return np.array(list(r.last) + list(r.mul1) + list(r.mul2) + list(r.add) + [r.buf_id if r.buf_id != bank.UNSET else R.UNSET] +
                    [m.n_bits, m.feedback_bit, m.feedback_mask, m.active_mask, m.taps_mask, m.output_mask, m.state, m.sync], u64)


def configure(bank, ch, unit):
    """The settings of a restatement unit, and its states, on a channel."""
    capi = sys.modules[type(bank).__module__.rsplit(".", 1)[0] + ".capi"]
    s = capi.VelvetState()
    r, m = unit.rand, unit.mls
    for k in range(4):
        s.rand.last[k], s.rand.mul1[k], s.rand.mul2[k], s.rand.add[k] = r.last[k], r.mul1[k], r.mul2[k], r.add[k]
    s.rand.buf_id = r.buf_id & 0xFFFFFFFF
    s.mls.n_bits, s.mls.feedback_bit, s.mls.feedback_mask, s.mls.active_mask = m.n_bits, m.feedback_bit, m.feedback_mask, m.active_mask
    s.mls.taps_mask, s.mls.output_mask, s.mls.state, s.mls.sync = m.taps_mask, m.output_mask, m.state, int(m.sync)
    bank.set_state(ch, s)
    bank.set_core_type(ch, unit.core)
    bank.set_velvet_type(ch, unit.type)
    bank.set_velvet_window_width(ch, unit.width)
    bank.set_delta_value(ch, unit.delta)
    bank.set_crush(ch, unit.crush)
    bank.set_crush_probability(ch, unit.prob)
    bank.set_amplitude(ch, unit.amplitude)
    bank.set_offset(ch, unit.offset)


def through_the_bank(gpu, case):
    """A recorded case on a bank of one channel."""
    bank = gpu.VelvetBank(1)
    src = gpu.DeviceBuffer.from_host(case["src"])
    start = np.zeros(case["src"].size, f32)
    out = gpu.DeviceBuffer.from_host(start)
    at = 0
    for op in case["ops"]:
        what, a, b, c = int(op[0]), op[1], op[2], op[3]
        if what in V.PROCESS_OPS:
            n = int(a)
            dst = out.ptr + 4 * at
            if what in (R.P_ADD_INPLACE, R.P_MUL_INPLACE):  # the in-place operations find their source in dst
                gpu.check(gpu.lib.mi_dspu_copy_d2d(dst, src.ptr + 4 * at, 4 * n, None))
            s = None if what in (R.P_OVERWRITE, V.P_ADD_NULL, V.P_MUL_NULL) else dst if what in (R.P_ADD_INPLACE, R.P_MUL_INPLACE) else src.ptr + 4 * at
            bank.process(dst, n, src=s, op=KIND[what])
            at += n
        elif what == V.INIT: bank.init(0, int(a), int(b), int(c))
        elif what == V.INIT_SAME: bank.init(0, int(a), int(b), bank.get_state(0).mls.state)
        elif what == R.SET_AMPLITUDE: bank.set_amplitude(0, f32(a))
        elif what == R.SET_OFFSET: bank.set_offset(0, f32(a))
        elif what == R.POKE_LAST:
            s = bank.get_state(0)
            s.rand.last[int(a)] = int(b)
            bank.set_state(0, s)
        elif what == V.SET_CORE: bank.set_core_type(0, int(a))
        elif what == V.SET_TYPE: bank.set_velvet_type(0, int(a))
        elif what == V.SET_WIDTH: bank.set_velvet_window_width(0, f32(a))
        elif what == V.SET_DELTA: bank.set_delta_value(0, f32(a))
        elif what == V.SET_CRUSH: bank.set_crush(0, bool(a))
        elif what == V.SET_CRUSH_PROB: bank.set_crush_probability(0, f32(a))
        else: raise ValueError(what)
    got = out.download()
    w = words(bank)
    bank.close()
    src.free()
    out.free()
    return got, w


@pytest.mark.gpu
def test_every_recorded_reference_case_through_the_bank(gpu, recorded):
    for c in recorded:
        got, w = through_the_bank(gpu, c)
        bad = np.nonzero(~R.same(got, c["out"]))[0]
        assert bad.size == 0, (c["name"], bad[:5], got[bad[:5]], c["out"][bad[:5]])
        assert np.array_equal(w, c["words"]), (c["name"], w, c["words"])


def unit_of(k, seed=0x4000):
    """Channel k of a bank of mixed channels: type, core, crush, width, delta and levels all differ."""
    u = V.Velvet()
    u.init(seed + 77 * k, (23, 64, 1, 2, 8, 33)[k % 6], (0x2F, 0, 0xDEADBEEFCAFE, 5)[k % 4])
    u.type, u.core, u.crush = k % 4, (k // 4) % 2, (k // 2) % 3 == 1
    u.set_width((10.0, 2.0, 2.5, 10.7, 64.0, 257.0, 3.0)[k % 7])
    u.set_delta((0.5, 0.0, 1.0, 0.25)[k % 4])
    u.set_crush_prob((0.5, 0.0, 1.0, 0.3)[k % 4])
    u.amplitude, u.offset = f32((1.0, 0.5, -2.0)[k % 3]), f32((0.0, 0.25, -0.0, -1.0)[k % 4])
    return u


class Bank:
    """A bank of C mixed channels and the restatement units that say what it has to give."""

    def __init__(self, gpu, C, seed=0x4000, make=unit_of):
        self.bank, self.units = gpu.VelvetBank(C), [make(k, seed) for k in range(C)]
        for k, u in enumerate(self.units):
            configure(self.bank, k, u)

    def want(self, what, src, n):
        return np.stack([u.process(what, None if src is None else src[k], n) for k, u in enumerate(self.units)])

    def check_words(self, label=""):
        for k, u in enumerate(self.units):
            assert np.array_equal(words(self.bank, k), u.words()), (label, k)

    def close(self):
        self.bank.close()


def same_rows(got, want, label=""):
    bad = np.argwhere(~R.same(got, want))
    assert bad.size == 0, (label, bad[:5], got[tuple(bad[0])], want[tuple(bad[0])])


def source(C, n, seed=5):
    row = gen.source_row()
    return np.stack([np.roll(np.resize(row, n), 13 * k) for k in range(C)]).astype(f32)


@pytest.mark.gpu
@pytest.mark.parametrize("C", [1, 3, 17])
def test_banks_of_one_three_and_seventeen_mixed_channels(gpu, C):
    n, stride = 700, 704
    b = Bank(gpu, C)
    src = source(C, stride)
    s = gpu.DeviceBuffer.from_host(src)
    for what in (R.P_OVERWRITE, R.P_ADD, R.P_MUL, V.P_ADD_NULL):
        out = gpu.DeviceBuffer.from_host(np.full((C, stride), 9.0, f32))
        b.bank.process(out, n, src=s if what in (R.P_ADD, R.P_MUL) else None, op=KIND[what], dst_stride=stride, src_stride=stride)
        got = out.download()
        same_rows(got[:, :n], b.want(what, src[:, :n], n), (C, what))
        assert (got[:, n:] == 9.0).all()
        out.free()
    b.check_words(C)
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("type_", range(4))
def test_counts_around_the_batch_the_tile_and_the_segment(gpu, type_):
    """One channel per (core, crush) pair and count after count on the same bank: the states go on from call to call."""
    def make(k, seed):
        u = unit_of(k, seed)
        u.type, u.core, u.crush = type_, k % 2, k // 2 == 1
        u.set_width((10.0, 2.0, 2.5, 64.0)[k])
        return u

    C = 4
    b = Bank(gpu, C, 0x5000 + type_, make)
    src = source(C, 4100)
    s = gpu.DeviceBuffer.from_host(src)
    out = gpu.DeviceBuffer((C, 4100))
    for i, n in enumerate((1, 2, 63, 64, 65, 255, 256, 257, 511, 513, 1100, 4097)):
        what = (R.P_OVERWRITE, R.P_ADD, R.P_OVERWRITE, R.P_MUL)[i % 4]
        b.bank.process(out, n, src=s if what != R.P_OVERWRITE else None, op=KIND[what], dst_stride=4100, src_stride=4100)
        same_rows(out.download()[:, :n], b.want(what, src[:, :n], n), (type_, n))
    b.check_words(type_)
    b.close()


@pytest.mark.gpu
def test_a_call_with_a_source_is_five_calls_and_an_overwrite_is_not(gpu):
    C, n = 8, 1100
    cuts = (256, 256, 256, 256, 76)
    src = source(C, n)
    s = gpu.DeviceBuffer.from_host(src)
    whole, cut, over, over_cut = (Bank(gpu, C, 0x6000) for _ in range(4))
    a, c, o, oc = (gpu.DeviceBuffer((C, n)) for _ in range(4))
    whole.bank.process(a, n, src=s, op=ADD)
    over.bank.process(o, n)
    at = 0
    for k in cuts:
        cut.bank.process(c.ptr + 4 * at, k, src=s.ptr + 4 * at, op=ADD, dst_stride=n, src_stride=n)
        over_cut.bank.process(oc.ptr + 4 * at, k, dst_stride=n)
        at += k
    got = a.download()
    assert np.array_equal(R.bits(got), R.bits(c.download()))
    same_rows(got, whole.want(R.P_ADD, src, n))
    got_over, got_cut = o.download(), oc.download()
    same_rows(got_over, over.want(R.P_OVERWRITE, None, n))
    for k in range(C):
        equal = np.array_equal(R.bits(got_over[k]), R.bits(got_cut[k]))
        assert equal == (over.units[k].type == V.TRN and not over.units[k].crush), k      # one segment is not five, but for one draw per sample
        assert np.array_equal(words(whole.bank, k), words(cut.bank, k))
    whole.check_words()
    over.check_words()
    for x in (whole, cut, over, over_cut):
        x.close()


@pytest.mark.gpu
def test_later_windows_win_where_two_hit_one_sample(gpu):
    """OVNA at W = 2.5 over 4096 samples, both cores, crushed and not: windows land on each other's samples, and within a batch of 60
    windows as across two of them the sample is the spike of the higher scan.  (At W = 2, the other four channels, only rv == 1.0f
    reaches the next window: as many spikes as windows, or one less.)"""
    def make(k, seed):
        u = unit_of(k, seed)
        u.type, u.core, u.crush = V.OVNA, k % 2, k // 2 % 2 == 1
        u.set_width(2.5 if k < 4 else 2.0)
        u.amplitude, u.offset = f32(1), f32(0)
        return u

    C, n = 8, 4096
    b = Bank(gpu, C, 0x7000, make)
    out = gpu.DeviceBuffer((C, n))
    b.bank.process(out, n)
    want = b.want(R.P_OVERWRITE, None, n)
    same_rows(out.download(), want)
    # collisions did happen: fewer spikes than windows
    spikes = (want != 0).sum(axis=1)
    windows = [sum(1 for role, _ in u.drawn if role == "p") - 1 for u in b.units]
    assert all(s < w - 10 for s, w in zip(spikes[:4], windows[:4])) and all(w - 1 <= s <= w for s, w in zip(spikes[4:], windows[4:])), (spikes, windows)
    b.check_words()
    b.close()


@pytest.mark.gpu
def test_strides_in_place_and_mul_with_null(gpu):
    C, n, stride = 5, 600, 1001                             # an odd stride: the rows are not aligned
    b = Bank(gpu, C, 0x8000)
    src = source(C, stride)
    buf = gpu.DeviceBuffer.from_host(src)
    b.bank.process(buf, n, src=buf, op=ADD, dst_stride=stride, src_stride=stride)
    got = buf.download()
    same_rows(got[:, :n], b.want(R.P_ADD_INPLACE, src[:, :n], n))
    assert np.array_equal(R.bits(got[:, n:]), R.bits(src[:, n:]))
    before = [words(b.bank, k) for k in range(C)]
    b.bank.process(buf, n, src=None, op=MUL, dst_stride=stride)
    got2 = buf.download()
    assert not got2[:, :n].any() and not np.signbit(got2[:, :n]).any() and np.array_equal(R.bits(got2[:, n:]), R.bits(src[:, n:]))
    for k in range(C):
        assert np.array_equal(words(b.bank, k), before[k]), k      # not a state word changed
    b.bank.process(buf.ptr + 4, n, src=buf.ptr + 4, op=MUL, dst_stride=stride, src_stride=stride)     # in place, off by one sample
    same_rows(buf.download()[:, 1:n + 1], b.want(R.P_MUL_INPLACE, got2[:, 1:n + 1], n))
    b.check_words()
    b.close()


@pytest.mark.gpu
def test_states_in_and_out_and_a_pending_init_against_the_devices_state(gpu, recorded):
    bank = gpu.VelvetBank(2)
    ref = [V.Velvet(), V.Velvet()]
    for k in range(2):
        assert words(bank, k)[16] == R.UNSET and np.array_equal(words(bank, k), ref[k].words())       # as constructed
        bank.init(k, 11 + k, 23, 0x55)
        ref[k].init(11 + k, 23, 0x55)
        assert np.array_equal(words(bank, k), ref[k].words())                                        # pending, as the kernel will take it
    out = gpu.DeviceBuffer((2, 500))
    bank.process(out, 500)
    same_rows(out.download(), np.stack([u.process(R.P_OVERWRITE, None, 500) for u in ref]))
    # an init with the device's own nState: nothing happens to the MLS; with another one bSync is set
    s0 = bank.get_state(0)
    assert s0.mls.sync == 0 and s0.mls.state == ref[0].mls.state
    bank.init(0, 99, 23, s0.mls.state)
    bank.init(1, 98, 23, s0.mls.state ^ 1 if s0.mls.state ^ 1 != ref[1].mls.state else 3)
    ref[0].init(99, 23, ref[0].mls.state)
    ref[1].init(98, 23, s0.mls.state ^ 1 if s0.mls.state ^ 1 != ref[1].mls.state else 3)
    assert bank.get_state(0).mls.sync == 0 and bank.get_state(1).mls.sync == 1
    # two inits before a launch: the first meets the device's state, the second the first
    bank.init(1, 97, 24, 0x55)
    ref[1].init(97, 24, 0x55)
    bank.process(out, 500)
    same_rows(out.download(), np.stack([u.process(R.P_OVERWRITE, None, 500) for u in ref]))
    for k in range(2):
        assert np.array_equal(words(bank, k), ref[k].words()), k
    # a round trip: the state out of one bank into another one goes on as the first
    twin = gpu.VelvetBank(2)
    for k in range(2):
        twin.set_state(k, bank.get_state(k))
    out2 = gpu.DeviceBuffer((2, 300))
    bank.process(out, 300, dst_stride=500)
    twin.process(out2, 300)
    assert np.array_equal(R.bits(out.download()[:, :300]), R.bits(out2.download()))
    for k in range(2):
        assert np.array_equal(words(bank, k), words(twin, k))
    s = bank.get_state(0)
    s.rand.buf_id = 4
    with pytest.raises(gpu.MiError) as e:
        bank.set_state(0, s)
    assert e.value.code == EINVAL
    s = bank.get_state(0)
    s.mls.state |= 1 << 40                                  # bSync clear and a bit beyond the register
    with pytest.raises(gpu.MiError) as e:
        bank.set_state(0, s)
    assert e.value.code == EINVAL
    bank.close()
    twin.close()


@pytest.mark.gpu
def test_what_the_bank_defines_where_the_reference_does_not(gpu):
    out = gpu.DeviceBuffer.from_host(np.full((2, 64), 5.0, f32))
    src = gpu.DeviceBuffer.from_host(np.ones((2, 64), f32))
    bank = gpu.VelvetBank(2)
    bank.init(0, 1, 23, 1)                                  # channel 1 was never init()ed: for every type and core, and every operation
    for type_ in range(4):
        for core in (0, 1):
            bank.set_velvet_type(1, type_)
            bank.set_core_type(1, core)
            for op, s in ((OVERWRITE, None), (ADD, src), (ADD, None), (MUL, src), (MUL, None)):
                with pytest.raises(gpu.MiError) as e:
                    bank.process(out, 64, src=s, op=op)
                assert e.value.code == ESTATE
    assert (out.download() == 5.0).all()
    bank.init(1, 2, 23, 1)
    before = [words(bank, k) for k in range(2)]
    bank.process(out, 0)                                    # count == 0: nothing
    bank.process(None, 0, src=None, op=ADD)
    assert (out.download() == 5.0).all() and all(np.array_equal(words(bank, k), before[k]) for k in range(2))
    for count in ((1 << 24) + 1, 1 << 27):
        with pytest.raises(gpu.MiError) as e:
            bank.process(out, count)
        assert e.value.code == EINVAL
        with pytest.raises(gpu.MiError) as e:
            bank.reserve(count)
        assert e.value.code == EINVAL
    bank.reserve(1 << 24)
    for width in (np.nan, np.inf, -np.inf):
        with pytest.raises(gpu.MiError) as e:
            bank.set_velvet_window_width(0, width)
        assert e.value.code == EINVAL
    with pytest.raises(gpu.MiError) as e:
        bank.process(out, 64, op=3)
    assert e.value.code == EINVAL
    with pytest.raises(gpu.MiError) as e:
        bank.process(None, 64)
    assert e.value.code == EINVAL
    assert all(np.array_equal(words(bank, k), before[k]) for k in range(2))
    bank.close()
    # a type and a core outside the enums: the switch's default: branches -- zero fill (then amplitude and offset), the LCG core
    def make(k, seed):
        u = unit_of(k, seed)
        u.type, u.core, u.crush = (9, V.OVN, 4, V.ARN)[k], (0, 7, 1, 2)[k], False
        return u
    b = Bank(gpu, 4, 0x9000, make)
    row = gpu.DeviceBuffer((4, 300))
    b.bank.process(row, 300)
    for u in b.units:
        u.core = V.CORE_LCG if u.core not in (0, 1) else u.core
    want = b.want(R.P_OVERWRITE, None, 300)
    same_rows(row.download(), want)
    assert len(np.unique(want[0])) == 1 and len(b.units[0].drawn) == 0
    b.check_words()
    b.close()
    # a step that is out of range saturates and ends the segment: the widest finite width
    big = Bank(gpu, 3, 0xA000, lambda k, seed: unit_of(k, seed))
    for k, u in enumerate(big.units):
        u.type, u.core, u.crush = (V.OVN, V.OVNA, V.ARN)[k], V.CORE_LCG, False
        u.set_width(3.0e38)
        u.set_delta(1.0)
        configure(big.bank, k, u)
    big.bank.process(row, 300, dst_stride=300)
    same_rows(row.download()[:3], big.want(R.P_OVERWRITE, None, 300))
    big.check_words()
    big.close()


# ---- streams, capture, lifetime -------------------------------------------------------------------------------------------------
def _stream(gpu):
    st = ctypes.c_void_p()
    gpu.check(gpu.lib.mi_dspu_stream_create(ctypes.byref(st)))
    return st


@pytest.mark.gpu
def test_one_capture_of_an_add_of_257_replayed_twice_is_three_calls(gpu):
    C, n = 6, 257
    st = _stream(gpu)
    b = Bank(gpu, C, 0xB000)
    src = source(C, n)
    s = gpu.DeviceBuffer.from_host(src)
    out = gpu.DeviceBuffer((C, n))
    held = b.bank.get_state(0)
    gc.collect()
    gc.disable()
    try:
        gpu.check(gpu.lib.mi_dspu_graph_begin_capture(st))
        for call in (lambda: b.bank.process(out, n, src=s, op=ADD, stream=st.value), lambda: b.bank.get_state(0, stream=st.value),
                     lambda: b.bank.set_state(0, held, stream=st.value)):
            with pytest.raises(gpu.MiError) as e:
                call()                                      # records that have not been sent; a state access
            assert e.value.code == ESTATE
        exe = ctypes.c_void_p()
        gpu.check(gpu.lib.mi_dspu_graph_end_capture(st, ctypes.byref(exe)))
        gpu.lib.mi_dspu_graph_destroy(exe)
        b.bank.process(out, n, src=s, op=ADD, stream=st.value)         # the first of the three calls sends the records
        same_rows(out.download(stream=st.value), b.want(R.P_ADD, src, n), "plain")
        b.bank.reserve(n)
        gpu.check(gpu.lib.mi_dspu_graph_begin_capture(st))
        b.bank.process(out, n, src=s, op=ADD, stream=st.value)
        exe = ctypes.c_void_p()
        gpu.check(gpu.lib.mi_dspu_graph_end_capture(st, ctypes.byref(exe)))
    finally:
        gc.enable()
    assert exe.value
    for rep in range(2):
        gpu.check(gpu.lib.mi_dspu_graph_launch(exe, st))
        same_rows(out.download(stream=st.value), b.want(R.P_ADD, src, n), rep)
    gpu.check(gpu.lib.mi_dspu_stream_synchronize(st))
    b.check_words("three calls")
    gpu.lib.mi_dspu_graph_destroy(exe)
    b.close()
    gpu.check(gpu.lib.mi_dspu_stream_destroy(st))


@pytest.mark.gpu
def test_two_banks_on_two_streams_and_destroy_with_work_in_flight(gpu):
    n, calls, C = 700, 3, 4
    streams = [_stream(gpu) for _ in range(2)]
    banks = [Bank(gpu, C, 0xC000 + i) for i in range(2)]
    outs = [gpu.DeviceBuffer((C, calls * n)) for _ in range(2)]
    wants = [[], []]
    for k in range(calls):
        for i in range(2):
            banks[i].bank.process(outs[i].ptr + 4 * k * n, n, dst_stride=calls * n, stream=streams[i].value)
            wants[i].append(banks[i].want(R.P_OVERWRITE, None, n))
    for i in range(2):
        got = outs[i].download(stream=streams[i].value)
        for k in range(calls):
            same_rows(got[:, k * n:(k + 1) * n], wants[i][k], (i, k))
    for k in range(calls):
        for i in range(2):
            banks[i].bank.process(outs[i], n, dst_stride=calls * n, stream=streams[i].value)
    for b in banks:
        b.close()                                           # right behind their last launches
    for st in streams:
        gpu.check(gpu.lib.mi_dspu_stream_synchronize(st))
        gpu.check(gpu.lib.mi_dspu_stream_destroy(st))
    again = Bank(gpu, C, 0xC000)
    out = gpu.DeviceBuffer((C, n))
    again.bank.process(out, n)
    same_rows(out.download(), again.want(R.P_OVERWRITE, None, n), "after the destroys")
    again.close()
    with pytest.raises(Exception):
        again.bank.process(out, n)                          # a closed bank


# ---- the C++ class ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """The program that recorded the cases from the reference's class, compiled against this library's class instead."""
    d = tmp_path_factory.mktemp("velvet_driver")
    src, exe = str(d / "driver.cpp"), str(d / "driver")
    open(src, "w").write(gen.DRIVER)
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-I" + os.path.join(PKG, "include"), "-I" + os.path.join(ROOT, "include"),
                           src, "-o", exe, "-L" + PKG, "-lmi_dspu", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    return exe, str(d)


@pytest.mark.gpu
def test_every_recorded_reference_case_through_the_cpp_class(gpu, driver, recorded):
    exe, cwd = driver
    got = gen.run(exe, recorded, recorded[0]["src"], cwd)
    for c, g in zip(recorded, got):
        bad = np.nonzero(~R.same(g["out"], c["out"]))[0]
        assert bad.size == 0, (c["name"], bad[:5], g["out"][bad[:5]], c["out"][bad[:5]])
        assert np.array_equal(g["words"], c["words"]), (c["name"], g["words"], c["words"])
    keys = {l.split()[0]: l.split()[1:] for l in subprocess.check_output([exe, "keys"]).decode().splitlines()}
    dump, _ = gen.inventories(keys, None)
    assert dump == json.load(open(os.path.join(ROOT, "tests", "golden", "velvet_dump_keys.json")))
