"""mi_noise_generator_bank on the device, the colour filter in the exact mode: every recorded reference case through a bank of one
channel, and banks of 1, 3 and 17 channels with generators and colours mixed, bit for bit in samples, in the state words of all
three sources, in the colour filter's members and memory, against the restatement (tests/noise_generator_ref.py; its sections are
this machine's designer's, which the bank's get_tilt_settings must equal) -- and against the recorded samples wherever those
sections are the recorded ones.  White exponential and Gaussian rows are held by the interval rule of noise_ref.py; a coloured one by
two calls from the same state.  What the bank defines where the reference does not, capture, streams, lifetime."""
import copy
import ctypes
import gc
import os
import subprocess
import sys

import numpy as np
import pytest

import noise_ref as R
import velvet_ref as V
import noise_generator_ref as G
from test_velvet_gpu import words as velvet_words

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_noise_generator_vectors as gen  # noqa: E402

f32, u32, u64 = np.float32, np.uint32, np.uint64
EINVAL, ESTATE = -1, -5
OVERWRITE, ADD, MUL = 0, 1, 2
OP = {G.G_OVER: OVERWRITE, G.G_ADD: ADD, G.G_ADD_IN: ADD, G.G_MUL: MUL, G.G_MUL_IN: MUL, G.G_ADD_NULL: ADD, G.G_MUL_NULL: MUL}
MARK = f32(9.0)


@pytest.fixture(scope="module")
def recorded():
    return [c for c in gen.load() if int(c["ops"][0][0]) >= G.G_OVER]


@pytest.fixture(scope="module")
def restated(recorded):
    """Every recorded case through the restatement on THIS machine's designer, with the neighbouring transcendentals where there are any."""
    out = []
    for c in recorded:
        r = G.run_case(c)
        out.append((r, [G.run_case(c, fn)[0] for fn in R.EXP_NEIGHBOURS + R.GAUSS_NEIGHBOURS] if r[4].any() else []))
    return out


def same_rows(got, want, label=""):
    bad = np.argwhere(~R.same(got, want))
    assert bad.size == 0, (label, bad[:5], np.asarray(got)[tuple(bad[0])], np.asarray(want)[tuple(bad[0])])


class VelvetView:
    """What test_velvet_gpu.words() asks of a bank, over a NoiseGeneratorState."""
    UNSET = 0xFFFFFFFF

    def __init__(self, state):
        self.state = state

    def get_state(self, ch):
        return self.state.velvet


def bank_words(bank, ch=0):
    """The words that the restatement's Generator.words() gives, as far as the bank shows them: the MLS by nBits and nState."""
    s = bank.get_state(ch)
    w = np.zeros(G.WORDS, u64)
    w[0:17] = list(s.lcg.last) + list(s.lcg.mul1) + list(s.lcg.mul2) + list(s.lcg.add) + [s.lcg.buf_id if s.lcg.buf_id != 0xFFFFFFFF else R.UNSET]
    w[17], w[23] = s.mls_n_bits, s.mls_state
    w[25:50] = velvet_words(VelvetView(s))
    w[G.TILT_AT:G.TILT_AT + 11] = G.settings_words(bank.get_tilt_settings(ch))
    w[G.UPDATE_AT] = bank.get_settings(ch).update
    return w, np.array(s.filter, f32).reshape(64, 2)


def shown(words):
    """Generator.words() cut down to what bank_words() shows."""
    w = np.array(words, u64)
    w[18:23], w[24] = 0, 0
    return w


def apply(bank, ch, op, pending):
    what, a, b, c = int(op[0]), op[1], op[2], op[3]
    if what == G.G_INIT_VELVET: pending[:] = [int(a), int(b), int(c)]
    elif what == G.G_INIT: bank.init(ch, int(a), int(b), int(c), *pending)
    elif what == G.G_RATE: bank.set_sample_rate(ch, int(a))
    elif what == G.G_MLS_BITS: bank.set_mls_n_bits(ch, int(a))
    elif what == G.G_MLS_SEED: bank.set_mls_seed(ch, int(a))
    elif what == G.G_DIST: bank.set_lcg_distribution(ch, int(a))
    elif what == G.G_VTYPE: bank.set_velvet_type(ch, int(a))
    elif what == G.G_VWIDTH: bank.set_velvet_window_width(ch, f32(a))
    elif what == G.G_VDELTA: bank.set_velvet_arn_delta(ch, f32(a))
    elif what == G.G_VCRUSH: bank.set_velvet_crush(ch, a != 0)
    elif what == G.G_VPROB: bank.set_velvet_crushing_probability(ch, f32(a))
    elif what == G.G_GEN: bank.set_generator(ch, int(a))
    elif what == G.G_COLOR: bank.set_noise_color(ch, int(a))
    elif what == G.G_ORDER: bank.set_coloring_order(ch, int(a))
    elif what == G.G_SLOPE: bank.set_color_slope(ch, f32(a), int(b))
    elif what == G.G_AMP: bank.set_amplitude(ch, f32(a))
    elif what == G.G_OFF: bank.set_offset(ch, f32(a))
    else: raise ValueError(what)


def through_the_bank(gpu, case):
    """A recorded case on a bank of one channel, the colour filter in the exact mode."""
    bank = gpu.NoiseGeneratorBank(1)
    bank.set_exact(True)
    src = gpu.DeviceBuffer.from_host(case["src"])
    out = gpu.DeviceBuffer.from_host(np.zeros(case["src"].size, f32))
    chart = np.zeros(2 * G.CHART_F.size, f32)
    pending, at = [0, 0, 0], 0
    for op in case["ops"]:
        what, a = int(op[0]), op[1]
        if what in G.G_PROCESS:
            n = int(a)
            dst, s = out.ptr + 4 * at, src.ptr + 4 * at
            if what in (G.G_ADD_IN, G.G_MUL_IN):
                gpu.check(gpu.lib.mi_dspu_copy_d2d(dst, s, 4 * n, None))
                s = dst
            bank.process(dst, n, src=None if what in (G.G_OVER, G.G_ADD_NULL, G.G_MUL_NULL) else s, op=OP[what])
            at += n
        elif what == G.G_CHART:
            c = bank.freq_chart(0, G.CHART_F, packed=a != 0)
            chart[0::2], chart[1::2] = c.real, c.imag
        else:
            apply(bank, 0, op, pending)
    got = out.download()[:at]
    words, memory = bank_words(bank)
    bank.close()
    src.free()
    out.free()
    return got, words, chart, memory


@pytest.mark.gpu
def test_every_recorded_reference_case_through_the_bank_in_the_exact_mode(gpu, recorded, restated):
    on_the_recorded_sections = 0
    for c, ((out, words, chains, chart, trans, unit), others) in zip(recorded, restated):
        got, w, chart_got, memory = through_the_bank(gpu, c)
        bad = R.agree(got, out, out, others, trans)
        assert bad.size == 0, (c["name"], bad[:5], got[bad[:5]], out[bad[:5]])
        assert np.array_equal(w, shown(words)), (c["name"], np.nonzero(w != shown(words))[0])
        same_rows(chart_got, chart, (c["name"], "chart"))
        same_rows(memory, unit.tilt.mem, (c["name"], "filter memory"))
        if G.same_sections(chains, c["chains"]):
            on_the_recorded_sections += 1                   # this machine's libm designs what the recording machine's did
            bad = R.agree(got, c["out"], out, others, trans)
            assert bad.size == 0, (c["name"], "recorded", bad[:5])
            assert np.array_equal(w, shown(c["words"])), c["name"]
            same_rows(chart_got, c["chart"], (c["name"], "recorded chart"))
    print("cases on the recorded sections: %d of %d" % (on_the_recorded_sections, len(recorded)))


PKG = os.path.join(ROOT, "lsp-dsp-units_amd")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """The program that recorded the cases from the reference's classes, compiled against this library's classes instead."""
    d = tmp_path_factory.mktemp("generator_driver")
    src, exe = str(d / "driver.cpp"), str(d / "driver")
    open(src, "w").write(gen.DRIVER)
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-I" + os.path.join(PKG, "include"), "-I" + os.path.join(ROOT, "include"),
                           src, "-o", exe, "-L" + PKG, "-lmi_dspu", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    return exe, str(d)


@pytest.mark.gpu
def test_every_recorded_reference_case_through_the_cpp_class(gpu, driver, recorded, restated, monkeypatch):
    """lsp::dspu::NoiseGenerator on host rows: every sample, every state word of the three sources (all of the MLS's members here),
    the colour filter's members, sections and chart; the FilterBank in the exact mode (the process-wide default, by the environment)."""
    exe, cwd = driver
    monkeypatch.setenv("MI_DSPU_EXACT_IIR", "1")
    got = gen.run(exe, recorded, gen.source_row(), cwd)
    for c, g, ((out, words, chains, chart, trans, _), others) in zip(recorded, got, restated):
        assert G.same_sections(g["chains"], chains), c["name"]
        bad = R.agree(g["out"], out, out, others, trans)
        assert bad.size == 0, (c["name"], bad[:5], g["out"][bad[:5]], out[bad[:5]])
        assert np.array_equal(g["words"], words), (c["name"], np.nonzero(g["words"] != words)[0])
        same_rows(g["chart"], chart, (c["name"], "chart"))
        if G.same_sections(chains, c["chains"]):
            bad = R.agree(g["out"], c["out"], out, others, trans)
            assert bad.size == 0, (c["name"], "recorded", bad[:5])
            assert np.array_equal(g["words"], c["words"]), c["name"]


def source(C, n):
    row = gen.source_row()
    return np.stack([np.roll(np.resize(row, n), 13 * k) for k in range(C)]).astype(f32)


class Bank:
    """A bank of C channels with generators and colours mixed, and the restatement units that say what it has to give."""

    def __init__(self, gpu, C, generators=(G.GEN_MLS, G.GEN_LCG, G.GEN_VELVET), exact=True, seed=0):
        self.gpu, self.C = gpu, C
        self.bank = gpu.NoiseGeneratorBank(C)
        self.bank.set_exact(exact)
        self.units = [G.Generator() for _ in range(C)]
        self.pending = {}
        for k in range(C):
            g = generators[(k + k // 4) % len(generators)]                 # LCG workgroups of four channels: partly on
            ops = [(G.G_INIT_VELVET, 0x5000 + 3 * k + seed, (23, 64, 8)[k % 3], 0x2F + k), (G.G_INIT, (17, 64, 3, 33)[k % 4], 0x1D + k, 0x777 * (k + 1) + seed),
                   (G.G_RATE, (48000, 44100)[k % 2]), (G.G_GEN, g), (G.G_COLOR, k % 6), (G.G_ORDER, (8, 50, 3, 128)[k % 4]), (G.G_SLOPE, -3.0, G.DB_OCT),
                   (G.G_DIST, (R.LCG_UNIFORM, R.LCG_TRIANGULAR)[(k // 2) % 2]), (G.G_VTYPE, k % 4), (G.G_VWIDTH, (0.0005, 0.0002)[k % 2]),
                   (G.G_VCRUSH, k % 5 == 3), (G.G_AMP, 0.5 + 0.25 * (k % 3)), (G.G_OFF, 0.125 * (k % 2))]
            for op in ops:
                self.set(k, op)

    def set(self, k, op):
        """One operation of noise_generator_ref.py's list on channel k of the bank and on its restatement unit."""
        op = tuple(float(v) for v in (list(op) + [0, 0, 0])[:4])
        p = self.pending.setdefault(k, [0, 0, 0])
        apply(self.bank, k, op, p)
        u, what, a, b, c = self.units[k], int(op[0]), op[1], op[2], op[3]
        if what == G.G_INIT_VELVET: pass
        elif what == G.G_INIT: u.init(int(a), int(b), int(c), *p)
        elif what == G.G_RATE: u.set_sample_rate(int(a))
        elif what == G.G_MLS_BITS: u.set_mls_n_bits(int(a))
        elif what == G.G_MLS_SEED: u.set_mls_seed(int(a))
        elif what == G.G_DIST: u.set_lcg_distribution(int(a))
        elif what == G.G_VTYPE: u.set_velvet_type(int(a))
        elif what == G.G_VWIDTH: u.set_velvet_window_width(a)
        elif what == G.G_VDELTA: u.set_velvet_arn_delta(a)
        elif what == G.G_VCRUSH: u.set_velvet_crush(a != 0)
        elif what == G.G_VPROB: u.set_velvet_crushing_probability(a)
        elif what == G.G_GEN: u.set_generator(int(a))
        elif what == G.G_COLOR: u.set_noise_color(int(a))
        elif what == G.G_ORDER: u.set_coloring_order(int(a))
        elif what == G.G_SLOPE: u.set_color_slope(a, int(b))
        elif what == G.G_AMP: u.set_amplitude(a)
        elif what == G.G_OFF: u.set_offset(a)
        else: raise ValueError(what)

    def want(self, what, src, n):
        return np.stack([u.process(what, None if src is None else src[k], n) for k, u in enumerate(self.units)])

    def check_words(self, label=""):
        for k, u in enumerate(self.units):
            w, memory = bank_words(self.bank, k)
            assert np.array_equal(w, shown(u.words())), (label, k, np.nonzero(w != shown(u.words()))[0])
            same_rows(memory, u.tilt.mem, (label, k, "filter memory"))

    def close(self):
        self.bank.close()


@pytest.mark.gpu
@pytest.mark.parametrize("C", [1, 3, 17])
def test_banks_of_one_three_and_seventeen_mixed_channels(gpu, C):
    """Every operation at counts around the segment of 256 and at 1100, on the same bank: the states go on from call to call.  An odd
    stride and one of a multiple of four; the gap behind the rows stays."""
    b = Bank(gpu, C)
    for n, stride in ((1, 5), (255, 260), (256, 256), (257, 261), (1100, 1104)):
        src = source(C, stride)
        s = gpu.DeviceBuffer.from_host(src)
        out = gpu.DeviceBuffer((C, stride))
        for what in (G.G_OVER, G.G_ADD, G.G_MUL, G.G_ADD_NULL, G.G_MUL_NULL, G.G_ADD_IN):
            out.upload(src if what == G.G_ADD_IN else np.full((C, stride), MARK, f32))
            given = None if what in (G.G_OVER, G.G_ADD_NULL, G.G_MUL_NULL) else out if what == G.G_ADD_IN else s
            b.bank.process(out, n, src=given, op=OP[what], dst_stride=stride, src_stride=stride)
            got = out.download()
            same_rows(got[:, :n], b.want(what, src[:, :n], n), (C, n, what))
            same_rows(got[:, n:], src[:, n:] if what == G.G_ADD_IN else np.full((C, stride - n), MARK, f32), (C, n, what, "gap"))
        s.free()
        out.free()
    b.check_words(C)
    b.close()


@pytest.mark.gpu
def test_idle_sources_keep_their_state_and_a_source_bank_without_a_row_is_not_launched(gpu):
    C, n = 17, 300
    b = Bank(gpu, C, generators=(G.GEN_LCG, G.GEN_VELVET))  # no MLS row at all
    out = gpu.DeviceBuffer((C, n))
    b.bank.process(out, n)                                  # (update_settings() gives every source its settings, the idle ones too)
    same_rows(out.download(), b.want(G.G_OVER, None, n), "first call")
    before = [bank_words(b.bank, k)[0] for k in range(C)]
    b.bank.process(out, n)
    same_rows(out.download(), b.want(G.G_OVER, None, n), "no MLS row")
    b.check_words("no MLS row")
    after = [bank_words(b.bank, k)[0] for k in range(C)]
    for k, u in enumerate(b.units):
        idle = [slice(17, 25)] + ([slice(25, 50)] if u.generator == G.GEN_LCG else [slice(0, 17)])
        for sl in idle:
            assert np.array_equal(before[k][sl], after[k][sl]), (k, sl)
        moved = slice(0, 17) if u.generator == G.GEN_LCG else slice(25, 50)
        assert not np.array_equal(before[k][moved], after[k][moved]), k
    # channel 0 to the MLS and back: every source goes on where it stopped (set_generator raises nothing)
    for g in (G.GEN_MLS, b.units[0].generator):
        b.set(0, (G.G_GEN, g))
        b.bank.process(out, n)
        same_rows(out.download(), b.want(G.G_OVER, None, n), ("generator", g))
    b.check_words("to the MLS and back")
    # a white overwrite costs exactly the source bank's launch
    white = gpu.NoiseGeneratorBank(4)
    for k in range(4):
        white.init(k, 23, 5, 100 + k, 7, 23, 9)
    white.process(out, n)
    assert "lcg_kernel" in gpu.last_launch(), gpu.last_launch()
    white.close()
    out.free()
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("dist", [R.LCG_EXPONENTIAL, R.LCG_GAUSSIAN], ids=["exponential", "gaussian"])
def test_a_coloured_transcendental_row_is_the_cascade_of_the_devices_white_row(gpu, dist):
    """Two calls from the same state: a white one that yields the device's row, and the coloured one, which must be the bit-exact
    cascade of that row."""
    n = 1100
    bank = gpu.NoiseGeneratorBank(1)
    bank.set_exact(True)
    unit = G.Generator()
    for u in (bank, unit):
        args = (23, 5, 0xABCDE, 7, 23, 9)
        u.init(0, *args) if u is bank else u.init(*args)
    bank.set_sample_rate(0, 48000), unit.set_sample_rate(48000)
    bank.set_lcg_distribution(0, dist), unit.set_lcg_distribution(dist)
    bank.set_coloring_order(0, 50), unit.set_coloring_order(50)
    out = gpu.DeviceBuffer((1, n))
    bank.process(out, 7)                                    # (the state is one that a call left)
    unit.process(G.G_OVER, None, 7)
    held = bank.get_state(0)
    bank.process(out, n)
    white = out.download()[0]
    star, others = copy.deepcopy(unit), None
    want = star.process(G.G_OVER, None, n)
    fns = R.EXP_NEIGHBOURS if dist == R.LCG_EXPONENTIAL else R.GAUSS_NEIGHBOURS
    others = [copy.deepcopy(unit).process(G.G_OVER, None, n, fn) for fn in fns]
    bad = R.agree(white, want, want, others, np.ones(n, bool))
    assert bad.size == 0, (bad[:5], white[bad[:5]], want[bad[:5]])
    bank.set_state(0, held)
    bank.set_noise_color(0, G.PINK), unit.set_noise_color(G.PINK)
    bank.process(out, n)
    unit.update_settings()
    same_rows(out.download()[0], unit.do_process(n, white=white), "coloured")
    after = bank.get_state(0)
    assert list(after.lcg.last) != list(held.lcg.last)
    out.free()
    bank.close()


@pytest.mark.gpu
def test_what_the_bank_defines_and_every_refusal(gpu):
    C, n = 3, 64
    bank = gpu.NoiseGeneratorBank(C)
    start = np.full((C, n), MARK, f32)
    out, s = gpu.DeviceBuffer.from_host(start), gpu.DeviceBuffer.from_host(start)

    def refused(code, call, text=""):
        with pytest.raises(gpu.MiError) as e:
            call()
        assert e.value.code == code and text in str(e.value), e.value

    refused(ESTATE, lambda: bank.process(out, n), "init")   # process before init
    for k in range(C):
        bank.init(k, 23, 5, 100 + k, 7 + k, 23, 9)
    bank.set_noise_color(1, G.PINK)
    refused(ESTATE, lambda: bank.process(out, n), "sample rate")       # a coloured channel at sample rate 0
    assert np.array_equal(out.download(), start)
    bank.set_sample_rate(1, 48000)
    bank.process(out, 0)                                    # count 0: nothing
    assert np.array_equal(out.download(), start) and bank.get_settings(0).update == G.UPD_ALL
    refused(EINVAL, lambda: bank.process(out, (1 << 24) + 1), "too large")
    refused(EINVAL, lambda: bank.reserve((1 << 24) + 1))
    refused(EINVAL, lambda: bank.process(None, n))
    refused(EINVAL, lambda: bank.process(out, n, op=3))
    refused(EINVAL, lambda: bank.process(out, n, src=s, op=ADD, dst_stride=n - 1))
    refused(EINVAL, lambda: bank.process(out, n, src=out, op=ADD, dst_stride=n, src_stride=n + 4))
    refused(EINVAL, lambda: bank.set_velvet_window_width(0, float("nan")), "finite")
    refused(EINVAL, lambda: bank.set_amplitude(C, 1.0))
    refused(EINVAL, lambda: bank.get_state(C))
    refused(EINVAL, lambda: bank.freq_chart(C, G.CHART_F))
    refused(EINVAL, lambda: gpu.NoiseGeneratorBank(0))
    assert gpu.lib.mi_noise_generator_bank_process(None, None, None, 1, 1, 1, 0, None) == ESTATE
    assert gpu.lib.mi_noise_generator_bank_destroy(None) == 0
    assert np.array_equal(out.download(), start)
    # mul with NULL: zero fill, nothing drawn, and update_settings() has run
    before = bank_words(bank, 0)[0]
    bank.process(out, n, src=None, op=MUL)
    got = out.download()
    assert not got.any() and not np.signbit(got).any()
    after = bank_words(bank, 0)[0]
    assert after[G.UPDATE_AT] == 0 and np.array_equal(before[:17], after[:17]) and np.array_equal(before[25:50], after[25:50])
    # a generator and a colour outside their enums: the default: branches (LCG, white)
    twin = gpu.NoiseGeneratorBank(C)
    for k in range(C):
        twin.init(k, 23, 5, 100 + k, 7 + k, 23, 9)
        twin.set_generator(k, 7)
        twin.set_noise_color(k, 9 if k != 1 else G.WHITE)
        bank.set_noise_color(k, G.WHITE)
    a, b = gpu.DeviceBuffer((C, n)), gpu.DeviceBuffer((C, n))
    bank.process(a, n)
    twin.process(b, n)
    assert np.array_equal(a.download(), b.download())
    assert np.array_equal(twin.freq_chart(0, G.CHART_F), np.ones(G.CHART_F.size, np.complex64))
    for buf in (a, b, out, s):
        buf.free()
    twin.close()
    bank.close()


def _stream(gpu):
    st = ctypes.c_void_p()
    gpu.check(gpu.lib.mi_dspu_stream_create(ctypes.byref(st)))
    return st


@pytest.mark.gpu
def test_one_capture_of_an_add_of_257_replayed_twice_is_three_calls(gpu):
    C, n = 6, 257
    st = _stream(gpu)
    b = Bank(gpu, C, seed=5)
    src = source(C, n)
    s, out = gpu.DeviceBuffer.from_host(src), gpu.DeviceBuffer((C, n))
    gc.collect()
    gc.disable()
    try:
        gpu.check(gpu.lib.mi_dspu_graph_begin_capture(st))
        for call in (lambda: b.bank.process(out, n, src=s, op=ADD, stream=st.value), lambda: b.bank.get_state(0, stream=st.value),
                     lambda: b.bank.update_settings(stream=st.value)):
            with pytest.raises(gpu.MiError) as e:
                call()                                      # scratch rows that are not there, records that have not been sent; a state access
            assert e.value.code == ESTATE
        exe = ctypes.c_void_p()
        gpu.check(gpu.lib.mi_dspu_graph_end_capture(st, ctypes.byref(exe)))
        gpu.lib.mi_dspu_graph_destroy(exe)
        b.bank.reserve(n, stream=st.value)
        b.bank.update_settings(stream=st.value)
        gpu.check(gpu.lib.mi_dspu_graph_begin_capture(st))
        b.bank.process(out, n, src=s, op=ADD, stream=st.value)
        exe = ctypes.c_void_p()
        gpu.check(gpu.lib.mi_dspu_graph_end_capture(st, ctypes.byref(exe)))
    finally:
        gc.enable()
    assert exe.value
    for rep in range(3):
        if rep == 1:
            b.bank.process(out, n, src=s, op=ADD, stream=st.value)      # a plain call between the two replays
        else:
            gpu.check(gpu.lib.mi_dspu_graph_launch(exe, st))
        same_rows(out.download(stream=st.value), b.want(G.G_ADD, src, n), rep)
    gpu.check(gpu.lib.mi_dspu_stream_synchronize(st))
    for k, u in enumerate(b.units):                         # (the host's count of MLS samples does not see replays: nState comes from the device)
        w, memory = bank_words(b.bank, k)
        assert np.array_equal(w, shown(u.words())), (k, np.nonzero(w != shown(u.words()))[0])
    gpu.lib.mi_dspu_graph_destroy(exe)
    b.close()
    s.free()
    out.free()
    gpu.check(gpu.lib.mi_dspu_stream_destroy(st))


@pytest.mark.gpu
def test_two_banks_on_two_streams_and_destroy_with_work_in_flight(gpu):
    n, calls, C = 700, 3, 5
    streams = [_stream(gpu) for _ in range(2)]
    banks = [Bank(gpu, C, seed=10 + i) for i in range(2)]
    outs = [gpu.DeviceBuffer((C, calls * n)) for _ in range(2)]
    wants = [[], []]
    for k in range(calls):
        for i in range(2):
            banks[i].bank.process(outs[i].ptr + 4 * k * n, n, dst_stride=calls * n, stream=streams[i].value)
            wants[i].append(banks[i].want(G.G_OVER, None, n))
    for i in range(2):
        got = outs[i].download(stream=streams[i].value)
        for k in range(calls):
            same_rows(got[:, k * n:(k + 1) * n], wants[i][k], (i, k))
    for k in range(calls):
        for i in range(2):
            banks[i].bank.process(outs[i], n, src=outs[i], op=ADD, dst_stride=calls * n, src_stride=calls * n, stream=streams[i].value)
    for b in banks:
        b.close()                                           # right behind their last launches
    for st in streams:
        gpu.check(gpu.lib.mi_dspu_stream_synchronize(st))
        gpu.check(gpu.lib.mi_dspu_stream_destroy(st))
    again = Bank(gpu, C, seed=10)
    out = gpu.DeviceBuffer((C, n))
    again.bank.process(out, n)
    same_rows(out.download(), again.want(G.G_OVER, None, n), "after the destroys")
    again.close()
    with pytest.raises(Exception):
        again.bank.process(out, n)                          # a closed bank
