"""mi_spectral_tilt_bank on the device.  In the exact mode: every recorded reference case through a bank of one channel, and banks of
1, 3 and 17 channels with filtering, bypassed and disabled channels side by side, bit for bit in samples, members and filter memory
against the restatement (tests/noise_generator_ref.py), whose sections are the bank's own get_chains and whose cascade is
oracle/biquad_oracle.c; the recorded samples themselves wherever this machine's designer gives the recorded sections.  In the fast
mode: the criterion of the biquad bank.  Strides, in place, unaligned rows, count 0, refusals, capture,
streams, lifetime."""
import ctypes
import gc
import os
import subprocess
import sys

import numpy as np
import pytest

import noise_ref as R
import noise_generator_ref as G
import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_noise_generator_vectors as gen  # noqa: E402

f32, u32 = np.float32, np.uint32
EINVAL, ESTATE = -1, -5
OVERWRITE, ADD, MUL = 0, 1, 2
OP = {G.T_OVER: OVERWRITE, G.T_ADD: ADD, G.T_MUL: MUL}
MARK = f32(9.0)


@pytest.fixture(scope="module")
def recorded():
    return [c for c in gen.load() if int(c["ops"][0][0]) < G.G_OVER]


@pytest.fixture(scope="module")
def restated(recorded):
    """Every recorded case through the restatement on THIS machine's designer: once for all tests."""
    return [G.run_case(c) for c in recorded]


def same_rows(got, want, label=""):
    bad = np.argwhere(~R.same(got, want))
    assert bad.size == 0, (label, bad[:5], np.asarray(got)[tuple(bad[0])], np.asarray(want)[tuple(bad[0])])


def through_the_bank(gpu, case):
    """A recorded case on a bank of one channel in the exact mode: samples, members, sections, filter memory and the chart."""
    bank = gpu.SpectralTiltBank(1)
    bank.set_exact(True)
    src = gpu.DeviceBuffer.from_host(case["src"])
    out = gpu.DeviceBuffer.from_host(G.second(case["src"]))
    chart = np.zeros(2 * G.CHART_F.size, f32)
    at = 0
    for op in case["ops"]:
        what, a, b = int(op[0]), op[1], op[2]
        if what in G.T_PROCESS:
            n = int(a)
            dst, s = out.ptr + 4 * at, src.ptr + 4 * at
            if what in (G.T_OVER_IN, G.T_ADD_IN, G.T_MUL_IN):
                gpu.check(gpu.lib.mi_dspu_copy_d2d(dst, s, 4 * n, None))
                s = dst
            bank.process(dst, n, src=None if what in (G.T_OVER_NULL, G.T_ADD_NULL, G.T_MUL_NULL) else s, op=what % 3)
            at += n
        elif what == G.T_ORDER: bank.set_order(0, int(a))
        elif what == G.T_SLOPE: bank.set_slope(0, f32(a), int(b))
        elif what == G.T_NORM: bank.set_norm(0, int(a))
        elif what == G.T_LOWER: bank.set_lower_frequency(0, f32(a))
        elif what == G.T_UPPER: bank.set_upper_frequency(0, f32(a))
        elif what == G.T_RANGE: bank.set_frequency_range(0, f32(a), f32(b))
        elif what == G.T_RATE: bank.set_sample_rate(0, int(a))
        elif what == G.T_CHART:
            c = bank.freq_chart(0, G.CHART_F, packed=a != 0)
            chart[0::2], chart[1::2] = c.real, c.imag
        else: raise ValueError(what)
    got = out.download()[:at]
    words = np.zeros(G.WORDS, np.uint64)
    words[G.TILT_AT:G.TILT_AT + 11] = G.settings_words(bank.get_settings(0))
    chains, memory = bank.get_chains(0), bank.get_state(0)
    bank.close()
    src.free()
    out.free()
    return got, words, chains, chart, memory


@pytest.mark.gpu
def test_every_recorded_reference_case_through_the_bank_in_the_exact_mode(gpu, recorded, restated):
    on_the_recorded_sections = 0
    for c, (out, words, chains, chart, _, unit) in zip(recorded, restated):
        got, w, ch, chart_got, memory = through_the_bank(gpu, c)
        assert G.same_sections(ch, chains), c["name"]
        same_rows(got, out, c["name"])
        assert np.array_equal(w, words), (c["name"], w[G.TILT_AT:G.TILT_AT + 11], words[G.TILT_AT:G.TILT_AT + 11])
        same_rows(chart_got, chart, (c["name"], "chart"))
        same_rows(memory, unit.mem, (c["name"], "filter memory"))
        if G.same_sections(chains, c["chains"]):
            on_the_recorded_sections += 1                   # this machine's libm designs what the recording machine's did
            same_rows(got, c["out"], (c["name"], "recorded"))
            assert np.array_equal(w, c["words"]), c["name"]
            same_rows(chart_got, c["chart"], (c["name"], "recorded chart"))
    print("cases on the recorded sections: %d of %d" % (on_the_recorded_sections, len(recorded)))


PKG = os.path.join(ROOT, "lsp-dsp-units_amd")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """The program that recorded the cases from the reference's classes, compiled against this library's classes instead."""
    d = tmp_path_factory.mktemp("tilt_driver")
    src, exe = str(d / "driver.cpp"), str(d / "driver")
    open(src, "w").write(gen.DRIVER)
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-I" + os.path.join(PKG, "include"), "-I" + os.path.join(ROOT, "include"),
                           src, "-o", exe, "-L" + PKG, "-lmi_dspu", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    return exe, str(d)


@pytest.mark.gpu
def test_every_recorded_reference_case_through_the_cpp_class(gpu, driver, recorded, restated, monkeypatch):
    """lsp::dspu::SpectralTilt on host rows, its FilterBank in the exact mode (the process-wide default, by the environment)."""
    exe, cwd = driver
    monkeypatch.setenv("MI_DSPU_EXACT_IIR", "1")
    got = gen.run(exe, recorded, gen.source_row(), cwd)
    for c, g, (out, words, chains, chart, _, _) in zip(recorded, got, restated):
        assert G.same_sections(g["chains"], chains), c["name"]
        same_rows(g["out"], out, c["name"])
        assert np.array_equal(g["words"], words), (c["name"], g["words"][G.TILT_AT:G.TILT_AT + 11], words[G.TILT_AT:G.TILT_AT + 11])
        same_rows(g["chart"], chart, (c["name"], "chart"))
        if G.same_sections(chains, c["chains"]):
            same_rows(g["out"], c["out"], (c["name"], "recorded"))
            assert np.array_equal(g["words"], c["words"]), c["name"]


def noise_rows(C, n, seed=7):
    lcg = R.LCG()
    lcg.init(seed)
    return lcg.process(C * n).reshape(C, n)


class Bank:
    """A bank of C channels of mixed settings in the exact mode, and the restatement units that say what it has to give."""
    ORDERS = (50, 0, 8, 128, 3, 12, 2)

    def __init__(self, gpu, C, exact=True):
        self.gpu, self.C = gpu, C
        self.bank = gpu.SpectralTiltBank(C)
        self.bank.set_exact(exact)
        self.units = [G.Tilt() for _ in range(C)]
        self.on = [True] * C
        for k in range(C):
            self.set(k, "sample_rate", (48000, 44100, 96000)[k % 3])
            self.set(k, "order", self.ORDERS[k % len(self.ORDERS)])
            self.set(k, "slope", (-0.5, 0.0, 1.0, -3.0, 0.5)[k % 5], (G.NEPER, G.NEPER, G.NEPER, G.DB_OCT, G.UNIT_NONE)[k % 5])     # 1, 4 mod 5: bypassed
            self.set(k, "norm", k % 7)
            if k % 4 == 2:
                self.set(k, "lower_frequency", 10.0)
                self.set(k, "upper_frequency", 18000.0)

    def set(self, k, name, *args):
        getattr(self.units[k], "set_" + name)(*args)
        getattr(self.bank, "set_" + name)(k, *[f32(a) if isinstance(a, float) else a for a in args])

    def enable(self, k, on):
        self.on[k] = on
        self.bank.set_row_enabled(k, on)

    def want(self, what, dst, src, n):
        """The rows that dst holds after the call (disabled rows: what they held)."""
        rows = [u.process(what, dst[k], None if src is None else src[k], n) if self.on[k] else np.array(dst[k], f32) for k, u in enumerate(self.units)]
        return np.stack(rows)

    def check_state(self, label=""):
        for k, u in enumerate(self.units):
            same_rows(self.bank.get_state(k), u.mem, (label, k, "filter memory"))
            s = self.bank.get_settings(k)
            assert np.array_equal(G.settings_words(s), u.words()), (label, k)

    def close(self):
        self.bank.close()


@pytest.mark.gpu
@pytest.mark.parametrize("C", [1, 3, 17])
def test_banks_of_one_three_and_seventeen_mixed_channels(gpu, C):
    """Filtering and bypassed channels side by side, every operation, with a source, in place and with NULL; counts around 256 and
    1100 on the same bank (the memory goes on from call to call); an odd stride (scalar loads and stores) and one of a multiple of four."""
    b = Bank(gpu, C)
    for n, stride in ((1, 5), (255, 260), (256, 256), (257, 261), (1100, 1104)):
        src = np.zeros((C, stride), f32)
        src[:, :n] = noise_rows(C, n, seed=n)
        start = np.full((C, stride), MARK, f32)
        start[:, :n] = noise_rows(C, n, seed=n + 1)
        s = gpu.DeviceBuffer.from_host(src)
        out = gpu.DeviceBuffer((C, stride))
        for what in (G.T_OVER, G.T_ADD, G.T_MUL):
            out.upload(start)
            b.bank.process(out, n, src=s, op=OP[what], dst_stride=stride, src_stride=stride)
            got = out.download()
            same_rows(got[:, :n], b.want(what, start[:, :n], src[:, :n], n), (C, n, what))
            assert (got[:, n:] == MARK).all(), "wrote behind the rows"
            out.upload(src)                                 # in place: dst is the source
            b.bank.process(out, n, src=out, op=OP[what], dst_stride=stride, src_stride=stride)
            same_rows(out.download()[:, :n], b.want(what, src[:, :n], src[:, :n], n), (C, n, what, "in place"))
            out.upload(start)
            b.bank.process(out, n, src=None, op=OP[what], dst_stride=stride)
            same_rows(out.download()[:, :n], b.want(what, start[:, :n], None, n), (C, n, what, "NULL"))
        s.free()
        out.free()
    b.check_state(C)
    b.close()


@pytest.mark.gpu
def test_row_enable_unaligned_rows_and_a_redesign_in_mid_stream(gpu):
    C, n, stride = 17, 700, 704
    b = Bank(gpu, C)
    off = (0, 5, 6, 16)                                     # a filtering channel, two neighbours (one bypassed), the last
    src = noise_rows(C, stride + 4, seed=3)[:, :stride + 4]
    start = noise_rows(C, stride + 4, seed=4)
    s = gpu.DeviceBuffer.from_host(src)
    out = gpu.DeviceBuffer((C, stride + 4))

    def call(what, at, label):
        """Rows that start `at` floats into the buffers: at = 1 is no multiple of 16 bytes."""
        out.upload(start)
        b.bank.process(out.ptr + 4 * at, n, src=s.ptr + 4 * at, op=OP[what], dst_stride=stride, src_stride=stride)
        got = out.download().reshape(-1)[at:at + C * stride].reshape(C, stride)
        flat_s, flat_d = src.reshape(-1)[at:at + C * stride].reshape(C, stride), start.reshape(-1)[at:at + C * stride].reshape(C, stride)
        same_rows(got[:, :n], b.want(what, flat_d[:, :n], flat_s[:, :n], n), label)
        same_rows(got[:, n:], flat_d[:, n:], (label, "gap"))

    for what in (G.T_OVER, G.T_ADD, G.T_MUL):
        call(what, 0, ("all on", what))
    for k in off:
        b.enable(k, False)
    b.set(5, "order", 20)                                   # pending on a disabled row: waits
    for what in (G.T_OVER, G.T_ADD, G.T_MUL):
        call(what, 1, ("some off, unaligned", what))
    assert b.bank.get_settings(5).sync == 1 and b.bank.get_settings(4).sync == 0
    b.check_state("some off")
    b.set(2, "order", 10)                                   # a new design clears the memory of this channel alone
    b.set(3, "slope", 0.0, G.NEPER)                         # into bypass: sections and memory stay
    b.set(1, "slope", -1.0, G.NEPER)                        # out of bypass
    for k in off:
        b.enable(k, True)
    call(G.T_ADD, 0, "enabled again")
    b.check_state("enabled again")
    assert b.bank.get_settings(3).bypass == 1 and b.bank.get_chains(3).shape[0] == 64
    # set_state and reset
    mem = b.bank.get_state(2)
    b.bank.set_state(0, mem)
    b.units[0].mem[:] = mem
    b.bank.reset(4)
    b.units[4].mem[:] = 0
    call(G.T_OVER, 0, "after set_state and reset")
    b.check_state("after set_state and reset")
    for k in range(C):
        b.enable(k, False)
    out.upload(start)
    b.bank.process(out, n, src=s, op=MUL, dst_stride=stride, src_stride=stride)     # a bank with no enabled row does nothing
    b.bank.process(out, n, src=None, op=OVERWRITE, dst_stride=stride)
    assert np.array_equal(out.download(), start)
    s.free()
    out.free()
    b.close()


def design(order, slope, rate=48000):
    t = G.Tilt()
    t.set_sample_rate(rate)
    t.set_order(order)
    t.set_slope(slope, G.NEPER)
    t.update_settings()
    return t.chains()


@pytest.mark.gpu
@pytest.mark.parametrize("slope", [-0.5, 1.0], ids=["pink", "violet"])
@pytest.mark.parametrize("order", [2, 50, 128])
def test_the_fast_mode_meets_the_biquad_banks_criterion(gpu, order, slope):
    """The criterion of smoke() and DESIGN.md section 4: the error against the exact cascade, relative to the peak, is at most
    max(1e-5, 3 x the float32 noise of the reference arithmetic itself against float64).  Measured on an MI355X (order, colour:
    error, noise): see DESIGN.md 3.27."""
    C, n = 3, 1100
    x = noise_rows(C, n, seed=order)
    bank = gpu.SpectralTiltBank(C)
    bank.set_exact(False)
    for k in range(C):
        bank.set_sample_rate(k, 48000)
        bank.set_order(k, order)
        bank.set_slope(k, f32(slope), G.NEPER)
    s, out = gpu.DeviceBuffer.from_host(x), gpu.DeviceBuffer((C, n))
    bank.process(out, n, src=s)
    y = out.download()
    coef = bank.get_chains(0)
    assert np.array_equal(coef.view(u32), design(order, slope).view(u32))
    bank.close()
    for k in range(C):
        ref, _ = oracle.biquad_cascade(x[k], coef)
        exact = oracle.biquad_cascade_f64(x[k], coef)
        peak = np.abs(exact).max()
        noise = np.abs(ref - exact).max() / peak
        err = np.abs(y[k] - ref).max() / peak
        print("fast mode: order %d slope %g channel %d: error %.3g, float32 noise %.3g, ratio %.3g" % (order, slope, k, err, noise, err / max(noise, 1e-30)))
        assert np.isfinite(y[k]).all() and err <= max(1e-5, 3.0 * noise), (order, slope, k, err, noise)
    s.free()
    out.free()


@pytest.mark.gpu
def test_count_zero_and_every_refusal(gpu):
    C, n = 3, 64
    b = Bank(gpu, C)
    start = np.full((C, n), MARK, f32)
    out, s = gpu.DeviceBuffer.from_host(start), gpu.DeviceBuffer.from_host(start)
    b.bank.process(out, 0, src=s)                           # count 0: nothing, not even update_settings()
    assert np.array_equal(out.download(), start) and b.bank.get_settings(0).sync == 1

    def refused(code, call):
        with pytest.raises(gpu.MiError) as e:
            call()
        assert e.value.code == code, e.value

    refused(EINVAL, lambda: b.bank.process(None, n, src=s))
    refused(EINVAL, lambda: b.bank.process(out, n, src=s, op=3))
    refused(EINVAL, lambda: b.bank.process(out, n, src=s, dst_stride=n - 1))
    refused(EINVAL, lambda: b.bank.process(out, n, src=s, src_stride=n - 1))
    refused(EINVAL, lambda: b.bank.process(out, n, src=out, dst_stride=n, src_stride=n + 4))
    refused(EINVAL, lambda: b.bank.process(out, 1 << 31, src=s))
    refused(EINVAL, lambda: b.bank.set_order(C, 2))
    refused(EINVAL, lambda: b.bank.set_row_enabled(C, True))
    refused(EINVAL, lambda: b.bank.get_chains(C))
    refused(EINVAL, lambda: b.bank.get_state(C))
    refused(EINVAL, lambda: b.bank.freq_chart(C, G.CHART_F))
    refused(EINVAL, lambda: b.bank.reset(C))
    refused(EINVAL, lambda: b.bank.reserve(1 << 31))
    refused(EINVAL, lambda: gpu.SpectralTiltBank(0))
    assert gpu.lib.mi_spectral_tilt_bank_process(None, None, None, 1, 1, 1, 0, None) == ESTATE
    assert gpu.lib.mi_spectral_tilt_bank_destroy(None) == 0
    assert np.array_equal(out.download(), start)
    out.free()
    s.free()
    b.close()


def _stream(gpu):
    st = ctypes.c_void_p()
    gpu.check(gpu.lib.mi_dspu_stream_create(ctypes.byref(st)))
    return st


@pytest.mark.gpu
def test_one_capture_of_an_add_of_257_replayed_twice_is_three_calls(gpu):
    C, n = 6, 257
    st = _stream(gpu)
    b = Bank(gpu, C)
    src, start = noise_rows(C, n, seed=11), noise_rows(C, n, seed=12)
    s, out = gpu.DeviceBuffer.from_host(src), gpu.DeviceBuffer.from_host(start)
    gc.collect()
    gc.disable()
    try:
        gpu.check(gpu.lib.mi_dspu_graph_begin_capture(st))
        for call in (lambda: b.bank.process(out, n, src=s, op=ADD, stream=st.value), lambda: b.bank.get_state(0, stream=st.value),
                     lambda: b.bank.set_state(0, np.zeros((64, 2), f32), stream=st.value), lambda: b.bank.update_settings(stream=st.value)):
            with pytest.raises(gpu.MiError) as e:
                call()                                      # sections that have not been sent; a state access
            assert e.value.code == ESTATE
        exe = ctypes.c_void_p()
        gpu.check(gpu.lib.mi_dspu_graph_end_capture(st, ctypes.byref(exe)))
        gpu.lib.mi_dspu_graph_destroy(exe)
        b.bank.update_settings(stream=st.value)
        gpu.check(gpu.lib.mi_dspu_graph_begin_capture(st))
        with pytest.raises(gpu.MiError) as e:
            b.bank.process(out, n, src=s, op=ADD, stream=st.value)     # no scratch rows yet
        assert e.value.code == ESTATE and "reserve" in str(e.value)
        exe = ctypes.c_void_p()
        gpu.check(gpu.lib.mi_dspu_graph_end_capture(st, ctypes.byref(exe)))
        gpu.lib.mi_dspu_graph_destroy(exe)
        b.bank.reserve(n, stream=st.value)
        gpu.check(gpu.lib.mi_dspu_graph_begin_capture(st))
        b.bank.process(out, n, src=s, op=ADD, stream=st.value)
        exe = ctypes.c_void_p()
        gpu.check(gpu.lib.mi_dspu_graph_end_capture(st, ctypes.byref(exe)))
    finally:
        gc.enable()
    assert exe.value
    want = start
    for rep in range(3):
        if rep == 1:
            b.bank.process(out, n, src=s, op=ADD, stream=st.value)      # a plain call between the two replays
        else:
            gpu.check(gpu.lib.mi_dspu_graph_launch(exe, st))
        want = b.want(G.T_ADD, want, src, n)
        same_rows(out.download(stream=st.value), want, rep)
    gpu.check(gpu.lib.mi_dspu_stream_synchronize(st))
    b.check_state("three calls")
    gpu.lib.mi_dspu_graph_destroy(exe)
    b.close()
    s.free()
    out.free()
    gpu.check(gpu.lib.mi_dspu_stream_destroy(st))


@pytest.mark.gpu
def test_two_banks_on_two_streams_and_destroy_with_work_in_flight(gpu):
    n, calls, C = 700, 3, 4
    streams = [_stream(gpu) for _ in range(2)]
    banks = [Bank(gpu, C) for _ in range(2)]
    src = [noise_rows(C, calls * n, seed=20 + i) for i in range(2)]
    ins = [gpu.DeviceBuffer.from_host(x) for x in src]
    outs = [gpu.DeviceBuffer.from_host(x) for x in src]
    wants = [[], []]
    for k in range(calls):
        for i in range(2):
            at = 4 * k * n
            banks[i].bank.process(outs[i].ptr + at, n, src=ins[i].ptr + at, op=MUL, dst_stride=calls * n, src_stride=calls * n, stream=streams[i].value)
            seg = src[i][:, k * n:(k + 1) * n]
            wants[i].append(banks[i].want(G.T_MUL, seg, seg, n))
    for i in range(2):
        got = outs[i].download(stream=streams[i].value)
        for k in range(calls):
            same_rows(got[:, k * n:(k + 1) * n], wants[i][k], (i, k))
    for k in range(calls):
        for i in range(2):
            banks[i].bank.process(outs[i], n, src=ins[i], op=ADD, dst_stride=calls * n, src_stride=calls * n, stream=streams[i].value)
    for b in banks:
        b.close()                                           # right behind their last launches
    for st in streams:
        gpu.check(gpu.lib.mi_dspu_stream_synchronize(st))
        gpu.check(gpu.lib.mi_dspu_stream_destroy(st))
    again = Bank(gpu, C)
    out = gpu.DeviceBuffer((C, n))
    again.bank.process(out, n, src=ins[0], src_stride=calls * n)
    same_rows(out.download(), again.want(G.T_OVER, src[0][:, :n], src[0][:, :n], n), "after the destroys")
    again.close()
    with pytest.raises(Exception):
        again.bank.process(out, n, src=ins[0])              # a closed bank
