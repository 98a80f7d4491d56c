"""Oscillator on the device: every recorded reference case through the bank (as recorded and cut into other pieces), the tile
split against single-sample calls, add and mul (in place, without a source, with special values), changes between calls with no
read-back, the band-limited functions (exact mode against the restatement, default mode against an oversampler bank of the
test's own), capture, streams, lifetime, misuse, and the oscillator -> DynamicDelay chain.

Non-sinusoid samples are compared bit for bit (a NaN that arithmetic made need only be a NaN); sinusoid samples must lie in the
closed interval that the restatement's outputs with S*, its float32 predecessor and its successor span (tests/oscillator_ref.py)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import dyndelay_ref as dd
import oscillator_ref as R
from oversampler_ref import OversamplerRef

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_oscillator_vectors as gen  # noqa: E402

f32, u32 = np.float32, np.uint32
PKG = os.path.join(ROOT, "lsp-dsp-units_amd")
N = 1100
EINVAL, ESTATE = -1, -5
SETTER_OF = {R.SET_FUNCTION: 0, R.SET_FREQUENCY: 1, R.SET_SAMPLE_RATE: 2, R.SET_PHASE: 3, R.SET_BITS: 4, R.SET_DC_OFFSET: 5, R.SET_DC_REFERENCE: 6,
             R.SET_AMPLITUDE: 7, R.SET_DUTY: 8, R.SET_WIDTH: 9, R.SET_TRAPEZOID: 10, R.SET_PULSETRAIN: 11, R.SET_PARABOLIC_WIDTH: 12,
             R.SET_SQUARED_INVERSION: 13, R.SET_PARABOLIC_INVERSION: 14, R.SET_OVER_MODE: 15, R.RESET_PHASE: 16}
KIND = {R.P_OVERWRITE: 0, R.P_ADD: 1, R.P_ADD_NULL: 1, R.P_ADD_INPLACE: 1, R.P_MUL: 2, R.P_MUL_NULL: 2, R.P_MUL_INPLACE: 2}


def oversampler():
    return OversamplerRef(1, None)


@pytest.fixture(scope="module")
def recorded():
    return gen.load()


@pytest.fixture(scope="module")
def restated(recorded):
    """Every recorded case through the restatement with S* and, where a sinusoid made samples, with its two neighbours."""
    out = []
    for c in recorded:
        star = R.run_case(c, oversampler=oversampler)
        sinus = star[3]
        lo = R.run_case(c, sine=R.sine_prev, oversampler=oversampler)[0] if sinus.any() else star[0]
        hi = R.run_case(c, sine=R.sine_next, oversampler=oversampler)[0] if sinus.any() else star[0]
        out.append((star[0], lo, hi, sinus))
        assert R.same(star[1], c["periods"]), c["name"]     # the restatement's get_periods is the recorded one
    return out


def agree(got, want, star, lo, hi, sinus, what):
    bad = np.nonzero(~((R.bits(got) == R.bits(want)) | (np.isnan(got) & np.isnan(want))) & ~sinus)[0]
    assert bad.size == 0, (what, bad[:5], got[bad[:5]], want[bad[:5]])
    off = np.nonzero(~R.inside(got, star, lo, hi) & sinus)[0]
    assert off.size == 0, (what, off[:5], got[off[:5]], star[off[:5]])


def through_the_bank(gpu, case, piece=None):
    """A recorded case on a bank of one channel in exact mode; process operations in calls of `piece` samples (None: as recorded)."""
    bank = gpu.OscillatorBank(1)
    bank.set_exact(True)
    src = gpu.DeviceBuffer.from_host(case["src"])
    out = gpu.DeviceBuffer.from_host(case["src"])           # the in-place operations find their source in dst
    at, periods = 0, []
    for op in case["ops"]:
        what = int(op[0])
        if what == R.GET_PERIODS:
            row = gpu.DeviceBuffer((int(op[3]),))
            bank.get_periods(0, row, int(op[1]), int(op[2]), int(op[3]))
            periods.append(row.download())
            row.free()
        elif what in R.PROCESS_OPS:
            n = int(op[1])
            step = n if piece is None else piece
            for lo in range(0, n, step):
                k = min(step, n - lo)
                dst = out.ptr + 4 * (at + lo)
                s = None if what in (R.P_OVERWRITE, R.P_ADD_NULL, R.P_MUL_NULL) else dst if what in (R.P_ADD_INPLACE, R.P_MUL_INPLACE) \
                    else src.ptr + 4 * (at + lo)
                bank.process(dst, k, src=s, op=KIND[what])
            at += n
        elif what == R.UPDATE:
            bank.update_settings()
        else:
            bank.set(0, SETTER_OF[what], op[1], op[2])
    got = out.download()
    phase = bank.get_state(0)["phase"]
    bank.close()
    src.free()
    out.free()
    return got, phase, (np.concatenate(periods) if periods else np.zeros(0, f32))


@pytest.mark.gpu
@pytest.mark.parametrize("piece", [None, N, 7, 256, 1023])
def test_every_recorded_reference_case_through_the_bank(gpu, recorded, restated, piece):
    for c, (star, lo, hi, sinus) in zip(recorded, restated):
        got, phase, periods = through_the_bank(gpu, c, piece)
        agree(got, c["out"], star, lo, hi, sinus, (c["name"], piece))
        assert phase == int(c["words"][0]), (c["name"], piece)
        assert R.same(periods, c["periods"]), (c["name"], piece)        # get_periods, and the stream goes on behind it unchanged


@pytest.mark.gpu
def test_single_sample_calls(gpu, recorded, restated):
    """Calls of one sample, for the cases that were recorded that way and one per function."""
    seen = set()
    for c, (star, lo, hi, sinus) in zip(recorded, restated):
        fn = next(int(op[1]) for op in c["ops"][::-1] if int(op[0]) == R.SET_FUNCTION)
        if fn in seen and not any(int(op[0]) in R.PROCESS_OPS and int(op[1]) == 1 for op in c["ops"][:-1]):
            continue
        seen.add(fn)
        got, phase, _ = through_the_bank(gpu, c, 1)
        agree(got, c["out"], star, lo, hi, sinus, c["name"])
        assert phase == int(c["words"][0]), c["name"]
    assert seen == set(range(14))


class Unit:
    """A bank of C channels and C restatements side by side."""

    def __init__(self, gpu, C, exact=True):
        self.gpu, self.C = gpu, C
        self.bank = gpu.OscillatorBank(C)
        self.bank.set_exact(exact)
        self.refs = [R.Oscillator(oversampler=oversampler) for _ in range(C)]
        self.lo = [R.Oscillator(sine=R.sine_prev, oversampler=oversampler) for _ in range(C)]
        self.hi = [R.Oscillator(sine=R.sine_next, oversampler=oversampler) for _ in range(C)]

    def set(self, ch, what, a=0.0, b=0.0):
        self.bank.set(ch, SETTER_OF[what], a, b)
        for o in (self.refs[ch], self.lo[ch], self.hi[ch]):
            R.apply(o, (what, a, b, 0))

    def want(self, n, op=0, src=None):
        """What the three restatements make of a call: star, lo, hi [C, n] and which channels are sinusoids."""
        rows = [np.array([o.process(n, op, None if src is None else src[ch]) for ch, o in enumerate(os_)]) for os_ in (self.refs, self.lo, self.hi)]
        sinus = np.array([[o.function in R.SINUSOIDS] * n for o in self.refs], bool)
        return rows[0], rows[1], rows[2], sinus

    def check(self, got, want, what):
        star, lo, hi, sinus = want
        for ch in range(self.C):
            agree(got[ch], star[ch], star[ch], lo[ch], hi[ch], sinus[ch], (what, ch))

    def close(self):
        self.bank.close()


def three_channels(gpu, **kw):
    """Three channels, each with its own function and settings: a sawtooth on 24 bits, a sine, a trapezoid with a phase."""
    u = Unit(gpu, 3, **kw)
    for ch, (rate, freq, fn) in enumerate(((48000, 1000.5, R.FG_SAWTOOTH), (44100, 7777.25, R.FG_SINE), (96000, 312.125, R.FG_TRAPEZOID))):
        u.set(ch, R.SET_SAMPLE_RATE, rate)
        u.set(ch, R.SET_FREQUENCY, freq)
        u.set(ch, R.SET_FUNCTION, fn)
        u.set(ch, R.SET_AMPLITUDE, 0.5 + ch)
        u.set(ch, R.SET_DC_OFFSET, 0.25 * ch)
    u.set(0, R.SET_BITS, 24)
    u.set(0, R.SET_WIDTH, 0.3)
    u.set(2, R.SET_PHASE, 1.25)
    u.set(2, R.SET_TRAPEZOID, 0.2, 0.3)
    return u


@pytest.mark.gpu
def test_three_channels_with_strides_that_differ_from_the_count(gpu):
    u = three_channels(gpu)
    stride = N + 5                                          # no multiple of four: the scalar stores
    out = gpu.DeviceBuffer.from_host(np.full((3, stride), 9.0, f32))
    u.bank.process(out, N, dst_stride=stride)
    got = out.download()
    u.check(got[:, :N], u.want(N), "odd stride")
    assert (got[:, N:] == 9.0).all(), "wrote behind the rows"
    stride = N + 8                                          # ... and one that is: 16-byte stores, the tail by element
    out2 = gpu.DeviceBuffer.from_host(np.full((3, stride), 9.0, f32))
    u.bank.process(out2, N - 2, dst_stride=stride)
    got = out2.download()
    u.check(got[:, :N - 2], u.want(N - 2), "even stride")
    assert (got[:, N - 2:] == 9.0).all(), "wrote behind the rows"
    u.close()


@pytest.mark.gpu
def test_the_tile_split_is_invisible(gpu):
    """A row of more than three tiles per channel equals the same row made in single-sample calls, bit for bit."""
    n = 3 * 1024 + 77
    fns = (R.FG_SAWTOOTH, R.FG_TRAPEZOID, R.FG_PARABOLIC)

    def make(gpu):
        u = Unit(gpu, 3)
        for ch, fn in enumerate(fns):
            u.set(ch, R.SET_SAMPLE_RATE, 48000)
            u.set(ch, R.SET_FREQUENCY, 997.5 * (ch + 1))
            u.set(ch, R.SET_FUNCTION, fn)
            u.set(ch, R.SET_PARABOLIC_WIDTH, 0.6)
            u.set(ch, R.SET_BITS, (32, 24, 8)[ch])
        return u
    a, b = make(gpu), make(gpu)
    whole, single = gpu.DeviceBuffer((3, n)), gpu.DeviceBuffer((3, n))
    a.bank.process(whole, n)
    for i in range(n):
        b.bank.process(single.ptr + 4 * i, 1, dst_stride=n)
    got = whole.download()
    assert np.array_equal(R.bits(got), R.bits(single.download()))
    a.check(got, a.want(n), "whole")
    assert [a.bank.get_state(ch)["phase"] for ch in range(3)] == [b.bank.get_state(ch)["phase"] for ch in range(3)] == [o.acc for o in a.refs]
    a.close()
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("op", [R.OP_ADD, R.OP_MUL])
def test_add_and_mul_in_place_without_a_source_and_with_special_values(gpu, op):
    u = three_channels(gpu)
    rng = np.random.default_rng(5 + op)
    src = (rng.standard_normal((3, N)) * 0.5).astype(f32)
    src[:, ::9] = 0.0
    src[:, 4::9] = -0.0
    src[:, 100], src[:, 101], src[:, 102], src[:, 103] = np.nan, np.inf, -np.inf, 1e-41
    s, out = gpu.DeviceBuffer.from_host(src), gpu.DeviceBuffer((3, N))
    u.bank.process(out, N, src=s, op=op)
    u.check(out.download(), u.want(N, op, src), "with a source")
    assert np.array_equal(R.bits(s.download()), R.bits(src)), "the source was written"
    u.bank.process(s, N, src=s, op=op)                      # in place
    u.check(s.download(), u.want(N, op, src), "in place")
    u.bank.process(out, N, src=None, op=op)
    got = out.download()
    u.check(got, u.want(N, op, None), "without a source")
    if op == R.OP_MUL:                                      # 0.0f * s: zeros of both signs, as the wave's sign has it
        assert (got == 0).all() and np.signbit(got).any() and not np.signbit(got).all()
    u.close()


@pytest.mark.gpu
def test_changes_between_calls_with_no_read_back(gpu):
    u = three_channels(gpu)
    out = gpu.DeviceBuffer((3, 4 * 300))
    got = []
    changes = ([], [(0, R.SET_PHASE, 2.0), (1, R.SET_PHASE, -1.0)], [(0, R.SET_FUNCTION, R.FG_PULSETRAIN), (1, R.SET_FUNCTION, R.FG_SQUARED_COSINE),
               (2, R.SET_FREQUENCY, 5000.0)], [(0, R.SET_BITS, 32), (1, R.SET_BITS, 9), (2, R.RESET_PHASE, 0), (2, R.SET_PHASE, 0.5), (2, R.SET_PHASE, 0.75)])
    wants = []
    for k, cs in enumerate(changes):
        for ch, what, a in cs:
            u.set(ch, what, a)
        if k == 2:
            u.bank.update_settings()                        # twice before the next launch: the pending changes add up
            u.set(0, R.SET_PHASE, 2.5)
            for o in (u.refs, u.lo, u.hi):
                for ch in range(3):
                    o[ch].update_settings()
        u.bank.process(out.ptr + 4 * 300 * k, 300, dst_stride=1200)
        wants.append(u.want(300))
    got = out.download()
    for k, w in enumerate(wants):
        u.check(got[:, 300 * k:300 * (k + 1)], w, "call %d" % k)
    assert [u.bank.get_state(ch)["phase"] for ch in range(3)] == [o.acc for o in u.refs]
    u.bank.set_state(1, 12345)
    assert u.refs[1].mask == 511 and u.bank.get_state(1)["phase"] == 12345 & 511      # masked on entry: what the device will hold
    u.refs[1].acc = u.lo[1].acc = u.hi[1].acc = 12345 & u.refs[1].mask
    u.bank.process(out, 300, dst_stride=1200)
    u.check(out.download()[:, :300], u.want(300), "after set_state")
    u.close()


def band_limited(gpu, exact, mode, fns=(R.FG_BL_SAWTOOTH, R.FG_BL_RECTANGULAR, R.FG_BL_PARABOLIC)):
    u = Unit(gpu, len(fns), exact=exact)
    for ch, fn in enumerate(fns):
        u.set(ch, R.SET_SAMPLE_RATE, 48000)
        u.set(ch, R.SET_FREQUENCY, 440.25 * (ch + 1))
        u.set(ch, R.SET_FUNCTION, fn)
        u.set(ch, R.SET_WIDTH, 0.5)
        u.set(ch, R.SET_PARABOLIC_WIDTH, 0.8)
        u.set(ch, R.SET_AMPLITUDE, 0.7)
        u.set(ch, R.SET_OVER_MODE, mode)
    return u


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [1, 8, 15, 22, 29, 0])
def test_band_limited_functions_in_exact_mode_equal_the_restatement(gpu, mode):
    """One mode per N and OM_NONE, three channels, two calls (the filter's state runs on); then add on a bank that also has a
    channel without a BL function: the combine kernel."""
    u = band_limited(gpu, True, mode)
    out = gpu.DeviceBuffer((3, N))
    for n in (700, 400):
        u.bank.process(out, n, dst_stride=N)
        u.check(out.download()[:, :n], u.want(n), (mode, n))
    u.close()
    u = band_limited(gpu, True, mode, (R.FG_BL_TRAPEZOID, R.FG_SAWTOOTH, R.FG_BL_PULSETRAIN))
    rng = np.random.default_rng(mode)
    src = rng.standard_normal((3, 500)).astype(f32)
    s = gpu.DeviceBuffer.from_host(src)
    for op in (R.OP_OVERWRITE, R.OP_ADD, R.OP_MUL):
        u.bank.process(out, 500, src=s, op=op, dst_stride=N)
        u.check(out.download()[:, :500], u.want(500, op, src), (mode, "mixed", op))
    # a shorter call behind the longer ones, then the plain channel takes a BL function: its oversampler has seen zeros only, as
    # the reference's untouched sOver has seen nothing
    u.bank.process(out, 200, dst_stride=N)
    u.check(out.download()[:, :200], u.want(200), (mode, "mixed, shorter"))
    u.set(1, R.SET_FUNCTION, R.FG_BL_SAWTOOTH)
    u.bank.process(out, 300, dst_stride=N)
    u.check(out.download()[:, :300], u.want(300), (mode, "the plain channel band-limited"))
    u.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [1, 8, 15, 22, 29])
def test_band_limited_functions_in_default_mode_equal_an_oversampler_bank_fed_the_synth_rows(gpu, mode):
    n, times = 900, R.times_of(mode)
    u = band_limited(gpu, False, mode)
    over = gpu.OversamplerBank(3)
    over.set_sample_rate(48000)
    over.set_mode(mode)
    over.update_settings()
    out, mine = gpu.DeviceBuffer((3, n)), gpu.DeviceBuffer((3, n))
    for call in range(2):
        u.bank.process(out, n)
        rows, stride = u.bank.synth_rows()
        assert rows and stride >= n * times
        over.downsample(mine, rows, n, in_stride=stride)
        assert np.array_equal(R.bits(out.download()), R.bits(mine.download())), (mode, call)
    # ... and the rows themselves are the restatement's oversampled rows
    got = np.empty((3, stride), f32)
    gpu.check(gpu.lib.mi_dspu_copy_d2h(got.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(rows), got.nbytes, None))
    u.want(n), u.want(n)
    for ch in range(3):
        assert R.same(got[ch, :n * times], u.refs[ch].last_synth), (mode, ch)
    u.close()
    over.close()


@pytest.mark.gpu
def test_band_limited_channels_must_agree_and_an_unset_rate_is_refused(gpu):
    u = band_limited(gpu, True, 1)
    u.bank.set(1, SETTER_OF[R.SET_OVER_MODE], 8)
    with pytest.raises(gpu.MiError) as e:
        u.bank.update_settings()
    assert e.value.code == EINVAL
    u.bank.set(1, SETTER_OF[R.SET_OVER_MODE], 1)
    u.bank.update_settings()
    u.close()
    b = gpu.OscillatorBank(2)
    b.set_sample_rate(0, 48000)
    out = gpu.DeviceBuffer.from_host(np.full((2, 64), 3.0, f32))
    with pytest.raises(gpu.MiError) as e:
        b.process(out, 64)
    assert e.value.code == ESTATE and (out.download() == 3.0).all()
    b.set_sample_rate(1, 48000)
    b.process(out, 64)
    assert (out.download() == 0.0).all()                    # a sine of frequency 0 at phase 0
    b.close()


# ---- streams, capture, lifetime, arguments -------------------------------------------------------------------------------

def _stream(gpu):
    st = ctypes.c_void_p()
    gpu.check(gpu.lib.mi_dspu_stream_create(ctypes.byref(st)))
    return st


@pytest.mark.gpu
def test_capture_of_three_calls_and_two_replays(gpu):
    """nPhaseAcc lives on the device: a graph of three calls moves the phase on with every replay, as eager calls on a twin do.  A
    pending update, a state access and scratch rows that would have to grow are refused on a capturing stream."""
    n = 400
    st = _stream(gpu)
    p, twin = three_channels(gpu), three_channels(gpu)
    out, direct = gpu.DeviceBuffer((3, 3 * n)), gpu.DeviceBuffer((3, 3 * n))
    p.bank.set(0, SETTER_OF[R.SET_PHASE], 0.5)
    twin.set(0, R.SET_PHASE, 0.5)
    gpu.check(gpu.lib.mi_dspu_graph_begin_capture(st))
    for refused in (lambda: p.bank.process(out, n, dst_stride=3 * n, stream=st.value), lambda: p.bank.get_state(0, stream=st.value),
                    lambda: p.bank.set_state(0, 5, stream=st.value)):
        with pytest.raises(gpu.MiError) as e:
            refused()                                       # the changed phase has not been sent yet
        assert e.value.code == ESTATE
    exe = ctypes.c_void_p()
    gpu.check(gpu.lib.mi_dspu_graph_end_capture(st, ctypes.byref(exe)))
    gpu.lib.mi_dspu_graph_destroy(exe)
    p.bank.update_settings(stream=st.value)
    gpu.check(gpu.lib.mi_dspu_graph_begin_capture(st))
    for k in range(3):
        p.bank.process(out.ptr + 4 * n * k, n, dst_stride=3 * n, stream=st.value)
    gpu.check(gpu.lib.mi_dspu_graph_end_capture(st, ctypes.byref(exe)))
    assert exe.value
    for rep in range(2):
        gpu.check(gpu.lib.mi_dspu_graph_launch(exe, st))
        wants = []
        for k in range(3):
            twin.bank.process(direct.ptr + 4 * n * k, n, dst_stride=3 * n, stream=st.value)
            wants.append(twin.want(n))
        got = out.download(stream=st.value)
        assert np.array_equal(R.bits(got), R.bits(direct.download(stream=st.value))), rep
        for k, w in enumerate(wants):
            twin.check(got[:, n * k:n * (k + 1)], w, (rep, k))
    assert [p.bank.get_state(ch, stream=st.value)["phase"] for ch in range(3)] == [o.acc for o in twin.refs]      # six calls' worth
    gpu.lib.mi_dspu_graph_destroy(exe)
    # a BL call whose scratch rows do not exist yet
    b = band_limited(gpu, True, 15)
    b.bank.update_settings(stream=st.value)
    gpu.check(gpu.lib.mi_dspu_graph_begin_capture(st))
    with pytest.raises(gpu.MiError) as e:
        b.bank.process(out, n, dst_stride=3 * n, stream=st.value)
    assert e.value.code == ESTATE
    gpu.check(gpu.lib.mi_dspu_graph_end_capture(st, ctypes.byref(exe)))
    gpu.lib.mi_dspu_graph_destroy(exe)
    b.bank.reserve(n)
    gpu.check(gpu.lib.mi_dspu_graph_begin_capture(st))
    b.bank.process(out, n, dst_stride=3 * n, stream=st.value)
    gpu.check(gpu.lib.mi_dspu_graph_end_capture(st, ctypes.byref(exe)))
    gpu.check(gpu.lib.mi_dspu_graph_launch(exe, st))
    b.check(out.download(stream=st.value)[:, :n], b.want(n), "captured BL call")
    gpu.lib.mi_dspu_graph_destroy(exe)
    for u in (p, twin, b):
        u.close()
    gpu.check(gpu.lib.mi_dspu_stream_destroy(st))


@pytest.mark.gpu
def test_two_banks_on_two_streams_and_destroy_with_work_in_flight(gpu):
    n, calls = 700, 3
    streams = [_stream(gpu) for _ in range(2)]
    units = [three_channels(gpu), band_limited(gpu, True, 8)]
    outs = [gpu.DeviceBuffer((3, calls * n)) for _ in range(2)]
    wants = [[], []]
    for k in range(calls):
        for i in range(2):
            units[i].bank.process(outs[i].ptr + 4 * k * n, n, dst_stride=calls * n, stream=streams[i].value)
            wants[i].append(units[i].want(n))
    for i in range(2):
        got = outs[i].download(stream=streams[i].value)
        for k in range(calls):
            units[i].check(got[:, k * n:(k + 1) * n], wants[i][k], (i, k))
    for k in range(calls):
        for i in range(2):
            units[i].bank.process(outs[i], n, dst_stride=calls * n, stream=streams[i].value)
    for u in units:
        u.close()                                           # right behind their last launches
    for st in streams:
        gpu.check(gpu.lib.mi_dspu_stream_synchronize(st))
        gpu.check(gpu.lib.mi_dspu_stream_destroy(st))
    again = three_channels(gpu)
    out = gpu.DeviceBuffer((3, n))
    again.bank.process(out, n)
    again.check(out.download(), again.want(n), "after the destroys")
    again.close()


@pytest.mark.gpu
def test_a_closed_bank_a_wrong_channel_and_missing_rows_are_refused(gpu):
    u = three_channels(gpu)
    from importlib import import_module
    capi = import_module(gpu.__name__ + ".capi")
    ones = gpu.DeviceBuffer.from_host(np.ones((3, 64), f32))
    lib, h = gpu.lib, u.bank.handle
    for code, what in ((lib.mi_oscillator_bank_process(h, None, None, 64, 64, 64, 0, None), "no dst"),
                       (lib.mi_oscillator_bank_process(h, ctypes.c_void_p(ones.ptr), None, 64, 63, 64, 0, None), "a stride shorter than the count"),
                       (lib.mi_oscillator_bank_process(h, ctypes.c_void_p(ones.ptr), ctypes.c_void_p(ones.ptr), 60, 64, 68, 1, None),
                        "in place with different strides"),
                       (lib.mi_oscillator_bank_process(h, ctypes.c_void_p(ones.ptr), None, 1 << 27, 1 << 27, 1 << 27, 0, None), "count"),
                       (lib.mi_oscillator_bank_process(h, ctypes.c_void_p(ones.ptr), None, 64, 64, 64, 3, None), "no such operation"),
                       (lib.mi_oscillator_bank_set_frequency(h, 3, 1.0), "channel"), (lib.mi_oscillator_bank_set(h, 3, 0, 0.0, 0.0), "channel"),
                       (lib.mi_oscillator_bank_set(h, 0, 17, 0.0, 0.0), "no such setter"),
                       (lib.mi_oscillator_bank_reset_phase_accumulator(h, 7), "channel"),
                       (lib.mi_oscillator_bank_needs_update(h, 3, ctypes.byref(ctypes.c_int())), "channel"),
                       (lib.mi_oscillator_bank_get_state(h, 3, ctypes.byref(capi.OscillatorState()), None), "channel"),
                       (lib.mi_oscillator_bank_get_state(h, 0, None, None), "no state"),
                       (lib.mi_oscillator_bank_reserve(h, 1 << 27), "count")):
        assert code == EINVAL, (what, code)
        assert lib.mi_dspu_last_error().decode().startswith("mi_oscillator_"), what
    assert lib.mi_oscillator_bank_process(h, None, None, 0, 0, 0, 0, None) == 0             # nothing to do (update_settings has run)
    assert not u.bank.needs_update(0)
    u.bank.set(0, SETTER_OF[R.SET_FUNCTION], R.FG_SAWTOOTH)
    assert (ones.download() == 1.0).all(), "a refused call wrote"
    assert u.bank.needs_update(0)
    out = gpu.DeviceBuffer((3, 64))
    u.bank.process(out, 64)
    u.check(out.download(), u.want(64), "after the refusals")
    for ch in range(3):
        assert not u.bank.needs_update(ch)
        assert np.float32(u.bank.get_exact_frequency(ch)) == u.refs[ch].get_exact_frequency()
        assert np.float32(u.bank.get_exact_phase(ch)) == u.refs[ch].get_exact_phase()
    u.close()
    with pytest.raises(gpu.MiError) as e:
        u.bank.process(out, 64)
    assert e.value.code == ESTATE
    u.close()                                               # twice is fine


@pytest.mark.gpu
def test_an_oscillator_modulates_a_dynamic_delay_on_one_stream_with_no_host_copy(gpu):
    """The chorus: the oscillator bank writes the delay row that the DynamicDelay bank reads."""
    C, n, max_size = 3, 1500, 1000
    st = _stream(gpu)
    u = Unit(gpu, C)
    for ch in range(C):
        u.set(ch, R.SET_SAMPLE_RATE, 48000)
        u.set(ch, R.SET_FREQUENCY, 3.5 * (ch + 1) * 40)
        u.set(ch, R.SET_FUNCTION, (R.FG_TRAPEZOID, R.FG_SAWTOOTH, R.FG_PARABOLIC)[ch])      # non-sinusoids: the chain is bit-exact
        u.set(ch, R.SET_AMPLITUDE, 400.0)
        u.set(ch, R.SET_DC_OFFSET, 500.0)
        u.set(ch, R.SET_WIDTH, 0.5)
        u.set(ch, R.SET_PARABOLIC_WIDTH, 1.0)
    rng = np.random.default_rng(42)
    inp = (rng.standard_normal((C, n)) * 0.5).astype(f32)
    fgain, fdelay = np.full((C, n), 0.4, f32), np.full((C, n), 100.0, f32)
    d_in, d_gain, d_fd = (gpu.DeviceBuffer.from_host(a, stream=st.value) for a in (inp, fgain, fdelay))
    d_delay, d_out = gpu.DeviceBuffer((C, n)), gpu.DeviceBuffer((C, n))
    delay = gpu.DynamicDelayBank(C, max_size)
    refs = [dd.DynamicDelay(max_size) for _ in range(C)]
    for call in range(2):
        u.bank.process(d_delay, n, stream=st.value)
        delay.process(d_out, d_in, d_delay, d_gain, d_fd, n, stream=st.value)
        rows = u.want(n)[0]
        want = np.array([refs[ch].process(inp[ch], rows[ch], fgain[ch], fdelay[ch]) for ch in range(C)])
        assert np.array_equal(R.bits(d_out.download(stream=st.value)), R.bits(want)), call
        assert rows.min() >= 99 and rows.max() <= 901
    delay.close()
    u.close()
    gpu.check(gpu.lib.mi_dspu_stream_destroy(st))


# ---- the C++ class ---------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """The program that recorded the cases from the reference's class, compiled against this library's class instead."""
    d = tmp_path_factory.mktemp("oscillator_driver")
    src, exe = str(d / "driver.cpp"), str(d / "driver")
    open(src, "w").write(gen.DRIVER)
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-DEXACT_FILTERS", "-I" + os.path.join(PKG, "include"), "-I" + os.path.join(ROOT, "include"),
                           src, "-o", exe, "-L" + PKG, "-lmi_dspu", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    return exe, str(d)


@pytest.mark.gpu
def test_every_recorded_reference_case_through_the_cpp_class(gpu, driver, recorded, restated):
    exe, cwd = driver
    got = gen.run(exe, recorded, recorded[0]["src"], cwd)
    for c, g, (star, lo, hi, sinus) in zip(recorded, got, restated):
        agree(g["out"], c["out"], star, lo, hi, sinus, c["name"])
        assert R.same(g["periods"], c["periods"]), c["name"]
        assert np.array_equal(g["words"], c["words"]), (c["name"], [R.WORDS[i] for i in np.nonzero(g["words"] != c["words"])[0]])
    keys = subprocess.check_output([exe, "keys"]).decode().split("\n")
    assert keys[0].split() == ["sizeof", "608", "168"] and keys[1].split() == ["sinsize", "4"]
    assert keys[2].split()[1:] == gen.json.load(open(os.path.join(ROOT, "tests", "golden", "oscillator_dump_keys.json")))["keys"]


def undefined_cases():
    """get_periods calls that refill: positions in front of the buffer read 0.0f by the bank's rule; plain and BL, more than one buffer."""
    base = [(R.SET_SAMPLE_RATE, 48000, 0, 0), (R.SET_AMPLITUDE, 0.8, 0, 0), (R.SET_DC_OFFSET, 0.1, 0, 0), (R.SET_PHASE, 0.3, 0, 0), (R.SET_WIDTH, 0.5, 0, 0),
            (R.SET_PARABOLIC_WIDTH, 0.8, 0, 0)]
    body = [(R.P_OVERWRITE, 400, 0, 0), (R.GET_PERIODS, 2, 0, 100), (R.P_OVERWRITE, 300, 0, 0), (R.GET_PERIODS, 3, 5, 64), (R.GET_PERIODS, 1, 0, 17),
            (R.P_OVERWRITE, 400, 0, 0)]
    cases = []
    for name, fn, freq, mode in (("sawtooth", R.FG_SAWTOOTH, 1000.5, 0), ("trapezoid", R.FG_TRAPEZOID, 333.25, 0),
                                 ("parabolic over more than a buffer", R.FG_PARABOLIC, 10.0, 0), ("BL sawtooth at 4x", R.FG_BL_SAWTOOTH, 1000.5, 15),
                                 ("BL parabolic over more than a buffer at 2x", R.FG_BL_PARABOLIC, 10.0, 1)):
        ops = base + [(R.SET_FREQUENCY, freq, 0, 0), (R.SET_OVER_MODE, mode, 0, 0), (R.SET_FUNCTION, fn, 0, 0)] + body
        cases.append(dict(name=name, ops=np.array(ops, np.float64), src=gen.source_row()))
    return cases


def check_undefined(c, out, periods, words):
    want, per, osc, _ = R.run_case(c, oversampler=oversampler)
    assert per.size == 181 and R.same(periods, per), c["name"]
    assert R.same(out, want) and np.array_equal(words, osc.words()), c["name"]          # the stream is where it would be without the calls
    # without skipped periods the read position is in front of the buffer from the first refill on (:684): zeros
    assert (per[:100] == 0).all() and (per[164:] == 0).all()
    assert np.count_nonzero(per[100:164] != per[100]) > 32, "the periods are flat"


@pytest.mark.gpu
def test_get_periods_where_the_reference_reads_in_front_of_its_buffer(gpu, driver):
    """Bank and class against the restatement: a position in front of the buffer reads 0.0f, the rest is the wave; the streaming
    phase and, for the band-limited functions, the streaming filter go on untouched; a period that is not positive and finite is
    refused."""
    exe, cwd = driver
    cases = undefined_cases()
    for c in cases:
        got, phase, periods = through_the_bank(gpu, c)
        words = R.run_case(c, oversampler=oversampler)[2].words()
        assert phase == int(words[0]), c["name"]
        check_undefined(c, got, periods, words)
    for c, g in zip(cases, gen.run(exe, cases, cases[0]["src"], cwd)):
        check_undefined(c, g["out"], g["periods"], g["words"])
    b = gpu.OscillatorBank(1)
    b.set_sample_rate(0, 48000)
    row = gpu.DeviceBuffer.from_host(np.full(8, 5.0, f32))
    with pytest.raises(gpu.MiError) as e:
        b.get_periods(0, row, 1, 0, 8)                      # frequency 0
    assert e.value.code == EINVAL and (row.download() == 5.0).all()
    with pytest.raises(gpu.MiError) as e:
        b.get_periods(1, row, 1, 0, 8)
    assert e.value.code == EINVAL
    b.close()


def double_hit_cases():
    """fFallRatio == 0: nPoints[1] == nPoints[2] == 2^31, and a word of 2^30 (2^29 oversampled) puts every fourth phase exactly there."""
    cases = []
    for name, fn, mode in (("trapezoid", R.FG_TRAPEZOID, 0), ("BL trapezoid at 2x", R.FG_BL_TRAPEZOID, 1), ("BL trapezoid at OM_NONE", R.FG_BL_TRAPEZOID, 0)):
        ops = [(R.SET_SAMPLE_RATE, 48000, 0, 0), (R.SET_FREQUENCY, 12000.0, 0, 0), (R.SET_FUNCTION, fn, 0, 0), (R.SET_TRAPEZOID, 0.5, 0.0, 0),
               (R.SET_OVER_MODE, mode, 0, 0), (R.SET_AMPLITUDE, 0.75, 0, 0), (R.SET_DC_OFFSET, 0.125, 0, 0), (R.P_OVERWRITE, N, 0, 0)]
        cases.append(dict(name=name, ops=np.array(ops, np.float64), src=gen.source_row()))
    return cases


@pytest.mark.gpu
def test_a_trapezoid_phase_that_satisfies_two_branches_takes_the_first(gpu, driver):
    """Kernel and class against the restatement on phases that :433 and :439 both accept."""
    exe, cwd = driver
    cases = double_hit_cases()
    wants = []
    for c in cases:
        want, _, osc, _ = R.run_case(c, oversampler=oversampler)
        assert osc.points[1] == osc.points[2] == 1 << 31 and osc.double_writes >= N // 4, c["name"]
        if osc.function == R.FG_TRAPEZOID:
            assert want[2] == f32(0.875) and want[3] == f32(-0.625)         # :434, amplitude + DC, not :440
        wants.append(want)
        got, _, _ = through_the_bank(gpu, c)
        assert R.same(got, want), c["name"]
    for c, g, want in zip(cases, gen.run(exe, cases, cases[0]["src"], cwd), wants):
        assert R.same(g["out"], want), c["name"]
