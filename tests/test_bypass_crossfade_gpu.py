"""The Bypass and Crossfade banks and the two C++ classes on the device, held to the float32 restatement bit for bit (the samples,
and nState / nCounter, fDelta and fGain from the banks' getters): channels in different states in one launch, counts on both
sides of the kernel's chunk, every variant and NULL combination, in-place and strided rows, special values, calls cut in
pieces, streams, capture, misuse, and every recorded case of the reference through the C-ABI and through the classes."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import bypass_crossfade_ref as bc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "lsp-dsp-units_amd")
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_bypass_crossfade_vectors as gen  # noqa: E402

f32 = np.float32
u32 = np.uint32
EINVAL, ESTATE = -1, -5
COUNTS = [1, 3, 255, 256, 257, 1200]
CHANNELS = [1, 5, 67]
LENGTHS = (1, 240, 300, 5000)
VARIANTS = [(v, dry) for v in (bc.PROCESS, bc.PROCESS_WET, bc.PROCESS_DRYWET) for dry in (True, False)]
COMBOS = [(True, True), (False, True), (True, False), (False, False)]
WET_GAIN, DRY_GAIN = 0.75, -0.5


def _rows(seed, C, n):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((C, n)) * 0.5).astype(f32)


def _init_args(length):
    return (48000, 0.005) if length == 240 else (length, 1.0)


# ---- a bypass bank and its restatement, every channel in another state ---------------------------------------------------

def _bypass(gpu, C, shift=0):
    """Channel by channel: steady off, steady on, ramping down, ramping up (from the start, and from the middle of a ramp),
    never initialised; ramps of 1, 240, 300 and 5000 samples."""
    bank, refs = gpu.BypassBank(C), [bc.Bypass() for _ in range(C)]
    for ch, r in enumerate(refs):
        kind, length = (ch + shift) % 7, LENGTHS[((ch + shift) // 7) % 4]
        if kind == 6:
            continue                                            # as construct() leaves it: fDelta 0
        bank.init(ch, *_init_args(length))
        r.init(*_init_args(length))
        if kind == 1:                                           # steady on: a ramp down that has ended
            r.set_fields(bc.S_ON, -r.delta, 0.0)
            bank.set_state(ch, bc.S_ON, r.delta, 0.0)
        elif kind == 2:
            assert bank.set_bypass(ch, True) is True and r.set_bypass(True)
        elif kind == 3:
            r.set_fields(bc.S_ON, -r.delta, 0.0)
            bank.set_state(ch, bc.S_ON, r.delta, 0.0)
            assert bank.set_bypass(ch, False) is True and r.set_bypass(False)
        elif kind in (4, 5):                                    # in the middle of a ramp
            r.set_fields(bc.S_ACTIVE, r.delta if kind == 4 else -r.delta, 0.37)
            bank.set_state(ch, bc.S_ACTIVE, r.delta, 0.37)
    return bank, refs


def _bypass_states_equal(bank, refs):
    for ch, r in enumerate(refs):
        s = bank.get_state(ch)
        if (s["state"], bc.bits(s["delta"]), bc.bits(s["gain"])) != r.fields():
            return False
    return True


def _bypass_call(bank, variant, dst, dry, wet, n, **kw):
    if variant == bc.PROCESS:
        bank.process(dst, dry, wet, n, **kw)
    elif variant == bc.PROCESS_WET:
        bank.process_wet(dst, dry, wet, WET_GAIN, n, **kw)
    else:
        bank.process_drywet(dst, dry, wet, DRY_GAIN, WET_GAIN, n, **kw)


def _bypass_want(refs, variant, dry, wet):
    got = [r.process(None if dry is None else dry[ch], wet[ch], variant, WET_GAIN, DRY_GAIN) for ch, r in enumerate(refs)]
    return np.array([g[0] for g in got]), np.array([g[1] for g in got])


def _bypass_check(gpu, bank, refs, variant, with_dry, dry, wet, what=""):
    C, n = wet.shape
    d_dry, d_wet, d_out = gpu.DeviceBuffer.from_host(dry), gpu.DeviceBuffer.from_host(wet), gpu.DeviceBuffer((C, n))
    _bypass_call(bank, variant, d_out, d_dry if with_dry else None, d_wet, n)
    want, copied = _bypass_want(refs, variant, dry if with_dry else None, wet)
    got = d_out.download()
    for ch in range(C):
        assert bc.same(got[ch], want[ch], copied[ch]), (what, variant, with_dry, ch)
    assert _bypass_states_equal(bank, refs), (what, variant, with_dry)


@pytest.mark.gpu
@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("C", CHANNELS)
def test_bypass_bit_exact_shapes(gpu, C, count):
    dry, wet = _rows(1, C, 2 * count), _rows(2, C, 2 * count)
    for i, (variant, with_dry) in enumerate(VARIANTS):
        bank, refs = _bypass(gpu, C, shift=i)
        for k in range(2):                                      # the second call goes on where the first one stopped
            _bypass_check(gpu, bank, refs, variant, with_dry, dry[:, k * count:(k + 1) * count], wet[:, k * count:(k + 1) * count], k)
        bank.close()


@pytest.mark.gpu
def test_bypass_across_the_kernels_chunks(gpu):
    """4097 samples: a ramp of 5000 crosses every chunk edge of the call, a ramp of 300 ends inside the first."""
    C, n = 29, 4097
    dry, wet = _rows(3, C, n), _rows(4, C, n)
    for i, (variant, with_dry) in enumerate(VARIANTS):
        bank, refs = _bypass(gpu, C, shift=i)
        _bypass_check(gpu, bank, refs, variant, with_dry, dry, wet)
        bank.close()


# ---- a crossfade bank and its restatement --------------------------------------------------------------------------------

def _crossfade(gpu, C, shift=0):
    """Channel by channel: fresh (fGain 1), fading from its start, in the middle of a fade, after reset() (fGain 0), after a fade."""
    bank, refs = gpu.CrossfadeBank(C), [bc.Crossfade() for _ in range(C)]
    for ch, r in enumerate(refs):
        kind, length = (ch + shift) % 5, LENGTHS[((ch + shift) // 5) % 4]
        bank.init(ch, *_init_args(length))
        r.init(*_init_args(length))
        if kind == 1:
            assert bank.toggle(ch) is True and r.toggle()
        elif kind == 2:
            r.toggle()
            r.set_fields(max(r.counter // 2, 1), r.delta, 0.4)
            bank.set_state(ch, r.counter, r.delta, 0.4)
        elif kind == 3:
            assert bank.toggle(ch) is True and r.toggle()
            bank.reset(ch)
            r.reset()
        elif kind == 4:
            r.toggle()
            r.set_fields(0, r.delta, 1.0000001)
            bank.set_state(ch, 0, r.delta, 1.0000001)
    return bank, refs


def _crossfade_states_equal(bank, refs):
    for ch, r in enumerate(refs):
        s = bank.get_state(ch)
        if (s["counter"], bc.bits(s["delta"]), bc.bits(s["gain"])) != r.fields() or bank.remaining(ch) != r.counter:
            return False
    return True


def _crossfade_check(gpu, bank, refs, fo, fi, a, b, what=""):
    C, n = a.shape
    d_a, d_b, d_out = gpu.DeviceBuffer.from_host(a), gpu.DeviceBuffer.from_host(b), gpu.DeviceBuffer.from_host(np.full((C, n), 7.0, f32))
    bank.process(d_out, d_a if fo else None, d_b if fi else None, n)
    got = d_out.download()
    for ch, r in enumerate(refs):
        want, copied = r.process(a[ch] if fo else None, b[ch] if fi else None, n)
        assert bc.same(got[ch], want, copied), (what, fo, fi, ch)
    assert _crossfade_states_equal(bank, refs), (what, fo, fi)


@pytest.mark.gpu
@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("C", CHANNELS)
def test_crossfade_bit_exact_shapes(gpu, C, count):
    a, b = _rows(5, C, 2 * count), _rows(6, C, 2 * count)
    for i, (fo, fi) in enumerate(COMBOS):
        bank, refs = _crossfade(gpu, C, shift=i)
        for k in range(2):
            _crossfade_check(gpu, bank, refs, fo, fi, a[:, k * count:(k + 1) * count], b[:, k * count:(k + 1) * count], k)
        bank.close()


@pytest.mark.gpu
def test_crossfade_across_the_kernels_chunks(gpu):
    C, n = 23, 4097
    a, b = _rows(7, C, n), _rows(8, C, n)
    for i, (fo, fi) in enumerate(COMBOS):
        bank, refs = _crossfade(gpu, C, shift=i)
        _crossfade_check(gpu, bank, refs, fo, fi, a, b)
        bank.close()


# ---- rows: strides, offsets, in place, special values --------------------------------------------------------------------

@pytest.mark.gpu
def test_strides_that_are_no_multiple_of_four_and_offset_rows(gpu):
    """Rows count + 5, count + 6 and count + 7 floats apart that start one float into their buffers: no 16-byte access fits, and
    nothing outside the rows is written."""
    C, n = 9, 301
    strides = (n + 5, n + 6, n + 7)                             # dst, dry | fade_out, wet | fade_in
    a, b = _rows(9, C, n), _rows(10, C, n)

    def spread(x, stride):
        buf = np.full(1 + C * stride, 99.0, f32)
        buf[1:].reshape(C, stride)[:, :n] = x
        return gpu.DeviceBuffer.from_host(buf)

    for variant, with_dry in VARIANTS[:3]:
        bank, refs = _bypass(gpu, C)
        d_out, d_a, d_b = spread(np.full((C, n), 55.0, f32), strides[0]), spread(a, strides[1]), spread(b, strides[2])
        _bypass_call(bank, variant, d_out.ptr + 4, d_a.ptr + 4 if with_dry else None, d_b.ptr + 4, n, dst_stride=strides[0],
                     dry_stride=strides[1], wet_stride=strides[2])
        want, copied = _bypass_want(refs, variant, a if with_dry else None, b)
        got = d_out.download()
        assert got[0] == 99.0 and np.all(got[1:].reshape(C, strides[0])[:, n:] == 99.0), "written outside the rows"
        for ch in range(C):
            assert bc.same(got[1:].reshape(C, strides[0])[ch, :n], want[ch], copied[ch]), (variant, with_dry, ch)
        assert _bypass_states_equal(bank, refs)
        bank.close()
    for fo, fi in COMBOS:
        bank, refs = _crossfade(gpu, C)
        d_out, d_a, d_b = spread(np.full((C, n), 55.0, f32), strides[0]), spread(a, strides[1]), spread(b, strides[2])
        bank.process(d_out.ptr + 4, d_a.ptr + 4 if fo else None, d_b.ptr + 4 if fi else None, n, dst_stride=strides[0],
                     out_stride=strides[1], in_stride=strides[2])
        got = d_out.download()
        assert got[0] == 99.0 and np.all(got[1:].reshape(C, strides[0])[:, n:] == 99.0), "written outside the rows"
        for ch, r in enumerate(refs):
            want, copied = r.process(a[ch] if fo else None, b[ch] if fi else None, n)
            assert bc.same(got[1:].reshape(C, strides[0])[ch, :n], want, copied), (fo, fi, ch)
        assert _crossfade_states_equal(bank, refs)
        bank.close()


@pytest.mark.gpu
@pytest.mark.parametrize("alias", ["dry", "wet", "fade_out", "fade_in"])
def test_dst_may_be_an_input(gpu, alias):
    C, n = 11, 1300                                             # more than a chunk: ramp, tail and a second chunk in place
    a, b = _rows(11, C, n), _rows(12, C, n)
    if alias in ("dry", "wet"):
        for variant, with_dry in (VARIANTS if alias == "wet" else VARIANTS[::2]):
            bank, refs = _bypass(gpu, C)
            d_a, d_b = gpu.DeviceBuffer.from_host(a), gpu.DeviceBuffer.from_host(b)
            d_out = d_a if alias == "dry" else d_b
            _bypass_call(bank, variant, d_out, d_a if with_dry else None, d_b, n)
            want, copied = _bypass_want(refs, variant, a if with_dry else None, b)
            got = d_out.download()
            for ch in range(C):
                assert bc.same(got[ch], want[ch], copied[ch]), (variant, with_dry, ch)
            other = (d_b if alias == "dry" else d_a).download()
            assert np.array_equal(other.view(u32), (b if alias == "dry" else a).view(u32)), "the other input was written"
            bank.close()
    else:
        for fo, fi in COMBOS[:3]:
            if (alias == "fade_out" and not fo) or (alias == "fade_in" and not fi):
                continue
            bank, refs = _crossfade(gpu, C)
            d_a, d_b = gpu.DeviceBuffer.from_host(a), gpu.DeviceBuffer.from_host(b)
            d_out = d_a if alias == "fade_out" else d_b
            bank.process(d_out, d_a if fo else None, d_b if fi else None, n)
            got = d_out.download()
            for ch, r in enumerate(refs):
                want, copied = r.process(a[ch] if fo else None, b[ch] if fi else None, n)
                assert bc.same(got[ch], want, copied), (fo, fi, ch)
            bank.close()


@pytest.mark.gpu
def test_inf_nan_and_subnormal_rows(gpu):
    """Every pairing of the noise, subnormal and Inf/NaN rows under every state: subnormals are kept, a copied NaN keeps its
    payload, a NaN that went through arithmetic is a NaN."""
    x = gen.signals()
    pairs = [(gen.NOISE_A, gen.SUBNORMAL), (gen.SUBNORMAL, gen.NOISE_B), (gen.SUBNORMAL, gen.SUBNORMAL), (gen.SPECIAL, gen.NOISE_B),
             (gen.NOISE_A, gen.SPECIAL), (gen.SPECIAL, gen.SPECIAL)]
    C = 28
    a = np.array([x[pairs[ch % 6][0]] for ch in range(C)])
    b = np.array([x[pairs[ch % 6][1]] for ch in range(C)])
    for i, (variant, with_dry) in enumerate(VARIANTS):
        bank, refs = _bypass(gpu, C, shift=i)
        _bypass_check(gpu, bank, refs, variant, with_dry, a, b)
        bank.close()
    for i, (fo, fi) in enumerate(COMBOS):
        bank, refs = _crossfade(gpu, C, shift=i)
        _crossfade_check(gpu, bank, refs, fo, fi, a, b)
        bank.close()
    bank = gpu.BypassBank(1)                                    # the tail's copy: bits in, bits out
    bank.init(0, 48000)
    d = gpu.DeviceBuffer.from_host(x[gen.SPECIAL][None])
    out = gpu.DeviceBuffer((1, gen.N))
    bank.process(out, None, d, gen.N)
    assert np.array_equal(out.download().view(u32), x[gen.SPECIAL][None].view(u32))
    bank.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["bypass", "crossfade"])
def test_calls_cut_in_pieces_equal_one_call(gpu, kind):
    C, n = 15, 1200
    a, b = _rows(13, C, n), _rows(14, C, n)
    d_a, d_b = gpu.DeviceBuffer.from_host(a), gpu.DeviceBuffer.from_host(b)
    for which in range(3):
        whole, pieces = gpu.DeviceBuffer((C, n)), gpu.DeviceBuffer((C, n))
        if kind == "bypass":
            variant, with_dry = VARIANTS[2 * which + which % 2]
            (one, refs), (cut, _) = _bypass(gpu, C, which), _bypass(gpu, C, which)
            call = lambda bank, out, at, k: _bypass_call(bank, variant, out.ptr + 4 * at, d_a.ptr + 4 * at if with_dry else None,  # noqa: E731
                                                         d_b.ptr + 4 * at, k, dst_stride=n, dry_stride=n, wet_stride=n)
            same = _bypass_states_equal
        else:
            fo, fi = COMBOS[which]
            (one, refs), (cut, _) = _crossfade(gpu, C, which), _crossfade(gpu, C, which)
            call = lambda bank, out, at, k: bank.process(out.ptr + 4 * at, d_a.ptr + 4 * at if fo else None,  # noqa: E731
                                                         d_b.ptr + 4 * at if fi else None, k, dst_stride=n, out_stride=n, in_stride=n)
            same = _crossfade_states_equal
        call(one, whole, 0, n)
        at = 0
        for k in (1, 7, 113, 256, 1, 300, 522):
            call(cut, pieces, at, k)
            at += k
        assert at == n
        assert np.array_equal(whole.download().view(u32), pieces.download().view(u32)), which
        if kind == "bypass":
            _bypass_want(refs, variant, a if with_dry else None, b)
        else:
            for ch, r in enumerate(refs):
                r.process(a[ch] if fo else None, b[ch] if fi else None, n)
        assert same(one, refs) and same(cut, refs), which
        one.close()
        cut.close()


# ---- the setters' answers ------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_set_bypass_and_toggle_answer_as_the_restatement(gpu):
    """Initialised channels answer from the host (nothing is waited for between the calls); never-initialised ones and states
    set through set_state() that contradict the sign of fDelta answer from the device."""
    C, n = 21, 100
    dry, wet = _rows(15, C, 6 * n), _rows(16, C, 6 * n)
    d_dry, d_wet, out = gpu.DeviceBuffer.from_host(dry), gpu.DeviceBuffer.from_host(wet), gpu.DeviceBuffer((C, n))
    bank, refs = _bypass(gpu, C)
    odd = {3: (bc.S_ON, 0.01, 0.5), 10: (bc.S_OFF, -0.01, 0.5), 17: (7, 0.01, 0.5), 18: (bc.S_ACTIVE, np.nan, 0.5)}
    for ch, fields in odd.items():
        refs[ch].set_fields(*fields)
        bank.set_state(ch, *fields)
    rng = np.random.default_rng(17)
    for k in range(6):
        for ch in range(C):
            want = bool(rng.integers(2))
            assert bank.bypassing(ch) == refs[ch].bypassing(), (k, ch)
            assert bank.set_bypass(ch, want) == refs[ch].set_bypass(want), (k, ch)
            assert bank.bypassing(ch) == refs[ch].bypassing(), (k, ch)
        bank.process(out, d_dry.ptr + 4 * k * n, d_wet.ptr + 4 * k * n, n, dry_stride=6 * n, wet_stride=6 * n)
        want, copied = _bypass_want(refs, bc.PROCESS, dry[:, k * n:(k + 1) * n], wet[:, k * n:(k + 1) * n])
        got = out.download()
        assert all(bc.same(got[ch], want[ch], copied[ch]) for ch in range(C)), k
    assert _bypass_states_equal(bank, refs)
    changed = bank.set_bypass(bank.ALL, True)
    assert changed == sum(int(r.set_bypass(True)) for r in refs) and _bypass_states_equal(bank, refs)
    bank.close()
    bank, refs = _crossfade(gpu, C)
    for k in range(6):
        for ch in range(C):
            if (ch + k) % 3 == 0:
                assert bank.toggle(ch) == refs[ch].toggle(), (k, ch)
            elif (ch + k) % 7 == 0:
                bank.reset(ch)
                refs[ch].reset()
            assert bank.remaining(ch) == refs[ch].counter, (k, ch)
        bank.process(out, d_dry.ptr + 4 * k * n, d_wet.ptr + 4 * k * n, n, out_stride=6 * n, in_stride=6 * n)
        got = out.download()
        for ch, r in enumerate(refs):
            want, copied = r.process(dry[ch, k * n:(k + 1) * n], wet[ch, k * n:(k + 1) * n], n)
            assert bc.same(got[ch], want, copied), (k, ch)
    assert _crossfade_states_equal(bank, refs)
    toggled = bank.toggle(bank.ALL)
    assert toggled == sum(int(r.toggle()) for r in refs) and _crossfade_states_equal(bank, refs)
    bank.close()


# ---- streams, capture, lifetime, arguments -------------------------------------------------------------------------------

def _stream(gpu):
    st = ctypes.c_void_p()
    gpu.check(gpu.lib.mi_dspu_stream_create(ctypes.byref(st)))
    return st


@pytest.mark.gpu
def test_two_banks_on_two_streams_and_destroy_with_work_in_flight(gpu):
    """A bypass bank and a crossfade bank fed alternately on two streams of their own, nothing waited for until the end; then both
    are destroyed right behind their last launches."""
    C, n, calls = 6, 313, 4
    streams = [_stream(gpu) for _ in range(2)]
    (bp, bp_refs), (xf, xf_refs) = _bypass(gpu, C, 2), _crossfade(gpu, C, 1)
    a, b = _rows(18, C, calls * n), _rows(19, C, calls * n)
    d_a, d_b = gpu.DeviceBuffer.from_host(a), gpu.DeviceBuffer.from_host(b)
    outs = [gpu.DeviceBuffer((C, calls * n)) for _ in range(2)]
    for k in range(calls):
        at = 4 * k * n
        bp.process_drywet(outs[0].ptr + at, d_a.ptr + at, d_b.ptr + at, DRY_GAIN, WET_GAIN, n, dst_stride=calls * n, dry_stride=calls * n,
                          wet_stride=calls * n, stream=streams[0].value)
        xf.process(outs[1].ptr + at, d_a.ptr + at, d_b.ptr + at, n, dst_stride=calls * n, out_stride=calls * n, in_stride=calls * n,
                   stream=streams[1].value)
    got = [outs[i].download(stream=streams[i].value) for i in range(2)]
    want, copied = _bypass_want(bp_refs, bc.PROCESS_DRYWET, a, b)
    for ch in range(C):
        assert bc.same(got[0][ch], want[ch], copied[ch]), ch
        w, c = xf_refs[ch].process(a[ch], b[ch], calls * n)
        assert bc.same(got[1][ch], w, c), ch
    assert _bypass_states_equal(bp, bp_refs) and _crossfade_states_equal(xf, xf_refs)
    for k in range(calls):
        bp.process(outs[0], d_a, d_b, n, dst_stride=calls * n, dry_stride=calls * n, wet_stride=calls * n, stream=streams[0].value)
        xf.process(outs[1], d_a, d_b, n, dst_stride=calls * n, out_stride=calls * n, in_stride=calls * n, stream=streams[1].value)
    bp.close()
    xf.close()
    for s in streams:
        gpu.check(gpu.lib.mi_dspu_stream_synchronize(s))
        gpu.check(gpu.lib.mi_dspu_stream_destroy(s))
    again, refs = _bypass(gpu, C)
    _bypass_check(gpu, again, refs, bc.PROCESS, True, a[:, :n], b[:, :n])
    again.close()


@pytest.mark.gpu
def test_zero_and_bad_arguments_on_a_live_bank(gpu):
    """Every bad argument comes back as an error code before any launch; nothing is written."""
    lib, C, n = gpu.lib, 3, 64
    buf = gpu.DeviceBuffer.from_host(np.zeros((C, n), f32))
    p, k = ctypes.c_void_p(buf.ptr), ctypes.c_int()
    bp = gpu.BypassBank(C)
    h = bp.handle
    calls = [lambda *r: lib.mi_bypass_bank_process(h, *r, None),
             lambda d, a, b, *r: lib.mi_bypass_bank_process_wet(h, d, a, b, 0.5, *r, None),
             lambda d, a, b, *r: lib.mi_bypass_bank_process_drywet(h, d, a, b, 0.5, 0.5, *r, None)]
    for fn in calls:
        assert fn(None, None, None, 0, 0, 0, 0) == 0                            # nothing to do
        assert fn(p, p, None, n, n, n, n) == EINVAL and fn(None, p, p, n, n, n, n) == EINVAL     # no wet row, no dst
        assert fn(p, p, p, n, n - 1, n, n) == EINVAL and fn(p, None, p, n, n, n, n - 1) == EINVAL  # a stride shorter than count
        assert fn(p, p, p, n, n, n + 4, n) == EINVAL and fn(p, None, p, n, n, n, n + 4) == EINVAL  # in place with different strides
        assert fn(p, None, p, 1 << 31, 1 << 31, 1 << 31, 1 << 31) == EINVAL
    assert lib.mi_bypass_bank_init(h, C, 48000, 0.005) == EINVAL and lib.mi_bypass_bank_init(h, 0, 48000, float("nan")) == EINVAL
    assert lib.mi_bypass_bank_set_bypass(h, C, 1, ctypes.byref(k)) == EINVAL and lib.mi_bypass_bank_set_bypass(h, 0, 1, None) == EINVAL
    assert lib.mi_bypass_bank_bypassing(h, C, ctypes.byref(k), None) == EINVAL and lib.mi_bypass_bank_bypassing(h, 0, None, None) == EINVAL
    assert lib.mi_bypass_bank_get_state(h, 0, None, None) == EINVAL and lib.mi_bypass_bank_set_state(h, 0, None, None) == EINVAL
    s = bp.get_state(0)
    assert (s["state"], s["delta"], s["gain"]) == (bc.S_OFF, 0, 0)
    assert lib.mi_bypass_bank_set_bypass(h, bp.ALL, 0, None) == 0               # all channels: the count may be left out
    xf = gpu.CrossfadeBank(C)
    g = xf.handle
    fn = lambda *r: lib.mi_crossfade_bank_process(g, *r, None)                  # noqa: E731
    assert fn(None, None, None, 0, 0, 0, 0) == 0
    assert fn(None, p, p, n, n, n, n) == EINVAL
    assert fn(p, p, p, n, n - 1, n, n) == EINVAL and fn(p, p, None, n, n, n - 1, n) == EINVAL
    assert fn(p, p, p, n, n, n + 4, n) == EINVAL and fn(p, None, p, n, n, n, n + 4) == EINVAL
    assert fn(p, None, None, 1 << 31, 1 << 31, 1 << 31, 1 << 31) == EINVAL
    assert lib.mi_crossfade_bank_init(g, C, 48000, 0.005) == EINVAL and lib.mi_crossfade_bank_init(g, 0, 48000, 1e6) == EINVAL
    assert lib.mi_crossfade_bank_toggle(g, C, ctypes.byref(k)) == EINVAL and lib.mi_crossfade_bank_toggle(g, 0, None) == EINVAL
    assert lib.mi_crossfade_bank_reset(g, C) == EINVAL and lib.mi_crossfade_bank_remaining(g, C, None) == EINVAL
    assert lib.mi_crossfade_bank_remaining(g, 0, None) == EINVAL
    assert lib.mi_crossfade_bank_get_state(g, 0, None, None) == EINVAL and lib.mi_crossfade_bank_set_state(g, 0, None, None) == EINVAL
    assert xf.remaining(0) == 0 and xf.get_state(0)["gain"] == 1
    assert np.all(buf.download() == 0.0), "a refused call wrote"
    assert lib.mi_bypass_bank_process(h, p, None, p, n, n, n, n, None) == 0     # and the banks still work
    assert fn(p, None, None, n, n, n, n) == 0
    bp.close()
    xf.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["bypass", "crossfade"])
def test_capture_steady_state_replays_and_pending_setters_are_refused(gpu, kind):
    """On a non-default stream: a setter leaves work to the next call, which a capturing stream refuses (MI_ESTATE), as it refuses
    get_state() and set_state(); with nothing pending a steady-state call is captured, and three replays equal three eager calls."""
    C, n = 7, 300
    st = _stream(gpu)
    a, b = _rows(20, C, n), _rows(21, C, n)
    d_a, d_b, out, direct = gpu.DeviceBuffer.from_host(a), gpu.DeviceBuffer.from_host(b), gpu.DeviceBuffer((C, n)), gpu.DeviceBuffer((C, n))
    if kind == "bypass":
        bank, twin = gpu.BypassBank(C), gpu.BypassBank(C)
        refs = [bc.Bypass() for _ in range(C)]
        for ch, r in enumerate(refs):
            for unit in (bank, twin):
                unit.init(ch, 48000)
            r.init(48000, 0.005)
            if ch % 2:                                          # steady on: switched, and run to the end before the capture
                for unit in (bank, twin):
                    unit.set_bypass(ch, True)
                r.set_bypass(True)
        call = lambda unit, o: unit.process_wet(o, d_a, d_b, WET_GAIN, n, stream=st.value)      # noqa: E731
        step = lambda: _bypass_want(refs, bc.PROCESS_WET, a, b)                                # noqa: E731
        pend = lambda: bank.set_bypass(0, True)                                                # noqa: E731
        ref_pend = lambda: refs[0].set_bypass(True)                                            # noqa: E731
        same = _bypass_states_equal
    else:
        bank, twin = gpu.CrossfadeBank(C), gpu.CrossfadeBank(C)
        refs = [bc.Crossfade() for _ in range(C)]
        for ch, r in enumerate(refs):
            for unit in (bank, twin):
                unit.init(ch, 48000)
            r.init(48000, 0.005)
            if ch % 2:
                for unit in (bank, twin):
                    unit.toggle(ch)
                r.toggle()
        call = lambda unit, o: unit.process(o, d_a, d_b, n, stream=st.value)                   # noqa: E731
        step = lambda: (np.array([r.process(a[ch], b[ch], n)[0] for ch, r in enumerate(refs)]), np.zeros((C, n), bool))  # noqa: E731
        pend = lambda: bank.toggle(0)                                                          # noqa: E731
        ref_pend = lambda: refs[0].toggle()                                                    # noqa: E731
        same = _crossfade_states_equal
    for unit in (bank, twin):
        call(unit, out)                                         # 300 samples: every ramp of 240 has ended
    step()
    assert same(bank, refs)
    pend()
    gpu.check(gpu.lib.mi_dspu_graph_begin_capture(st))
    with pytest.raises(gpu.MiError) as e:
        call(bank, out)
    assert e.value.code == ESTATE
    for refused in (lambda: bank.get_state(2, stream=st.value), lambda: bank.set_state(2, 0, 0.0, 0.0, stream=st.value)):
        with pytest.raises(gpu.MiError) as e:
            refused()
        assert e.value.code == ESTATE
    gpu.check(gpu.lib.mi_dspu_memset(ctypes.c_void_p(out.ptr), 0, 16, st))          # (so that the capture is not empty)
    exe = ctypes.c_void_p()
    gpu.check(gpu.lib.mi_dspu_graph_end_capture(st, ctypes.byref(exe)))
    gpu.lib.mi_dspu_graph_destroy(exe)
    ref_pend()
    twin_pend = twin.set_bypass(0, True) if kind == "bypass" else twin.toggle(0)
    assert twin_pend is True
    for unit in (bank, twin):
        call(unit, out)                                         # eager: the pending setter acts, channel 0 runs its ramp to the end
    want, _ = step()
    assert bc.same(out.download(stream=st.value), want, np.zeros((C, n), bool)) and same(bank, refs)
    gpu.check(gpu.lib.mi_dspu_graph_begin_capture(st))          # every channel steady, nothing pending
    call(bank, out)
    gpu.check(gpu.lib.mi_dspu_graph_end_capture(st, ctypes.byref(exe)))
    assert exe.value
    for rep in range(3):
        gpu.check(gpu.lib.mi_dspu_graph_launch(exe, st))
        call(twin, direct)
        want, _ = step()
        got = out.download(stream=st.value)
        assert np.array_equal(got.view(u32), direct.download(stream=st.value).view(u32)), rep
        assert np.array_equal(got.view(u32), want.view(u32)), rep
    assert same(bank, refs) and same(twin, refs)
    gpu.lib.mi_dspu_graph_destroy(exe)
    bank.close()
    twin.close()
    gpu.check(gpu.lib.mi_dspu_stream_destroy(st))


@pytest.mark.gpu
def test_a_captured_bypass_ramp_goes_on_with_every_replay(gpu):
    """All of the bypass bank's state is on the device: a call captured inside a ramp of 5000 samples replays as the next part
    of that ramp."""
    C, n = 5, 700
    st = _stream(gpu)
    dry, wet = _rows(22, C, n), _rows(23, C, n)
    d_dry, d_wet, out = gpu.DeviceBuffer.from_host(dry), gpu.DeviceBuffer.from_host(wet), gpu.DeviceBuffer((C, n))
    bank, refs = gpu.BypassBank(C), [bc.Bypass() for _ in range(C)]
    for ch, r in enumerate(refs):
        length = (5000, 1500, 240)[ch % 3]
        bank.init(ch, length, 1.0)
        r.init(length, 1.0)
        assert bank.set_bypass(ch, True) and r.set_bypass(True)
    bank.process(None, None, None, 0, stream=st.value)          # what the setters recorded goes out before the capture
    gpu.check(gpu.lib.mi_dspu_graph_begin_capture(st))
    bank.process(out, d_dry, d_wet, n, stream=st.value)
    exe = ctypes.c_void_p()
    gpu.check(gpu.lib.mi_dspu_graph_end_capture(st, ctypes.byref(exe)))
    for rep in range(4):
        gpu.check(gpu.lib.mi_dspu_graph_launch(exe, st))
        want, copied = _bypass_want(refs, bc.PROCESS, dry, wet)
        got = out.download(stream=st.value)
        assert all(bc.same(got[ch], want[ch], copied[ch]) for ch in range(C)), rep
        assert _bypass_states_equal(bank, refs), rep
    assert refs[0].state == bc.S_ACTIVE and refs[1].state == bc.S_ON
    gpu.lib.mi_dspu_graph_destroy(exe)
    bank.close()
    gpu.check(gpu.lib.mi_dspu_stream_destroy(st))


@pytest.mark.gpu
def test_a_capture_across_a_running_crossfade_is_refused_at_its_end(gpu):
    """The counters are positions held on the host: a capture during which they moved cannot replay.  end_capture says so
    (MI_ESTATE) after running the captured calls once, so the device and the host agree as after eager calls."""
    C, n = 4, 100
    st = _stream(gpu)
    a, b = _rows(24, C, n), _rows(25, C, n)
    d_a, d_b, out = gpu.DeviceBuffer.from_host(a), gpu.DeviceBuffer.from_host(b), gpu.DeviceBuffer((C, n))
    bank, refs = gpu.CrossfadeBank(C), [bc.Crossfade() for _ in range(C)]
    bank.init(bank.ALL, 48000)
    for r in refs:
        r.init(48000, 0.005)
    assert bank.toggle(2) is True and refs[2].toggle()
    bank.process(None, None, None, 0, stream=st.value)
    gpu.check(gpu.lib.mi_dspu_graph_begin_capture(st))
    bank.process(out, d_a, d_b, n, stream=st.value)
    exe = ctypes.c_void_p()
    assert gpu.lib.mi_dspu_graph_end_capture(st, ctypes.byref(exe)) == ESTATE and not exe.value
    got = out.download(stream=st.value)
    for ch, r in enumerate(refs):
        want, copied = r.process(a[ch], b[ch], n)
        assert bc.same(got[ch], want, copied), ch
    assert _crossfade_states_equal(bank, refs) and bank.remaining(2) == 140
    bank.close()
    gpu.check(gpu.lib.mi_dspu_stream_destroy(st))


# ---- the reference's recorded cases: through the C-ABI and through the C++ classes ------------------------------------------

class _OnTheBank:
    """One channel of a bank with the restatement's methods, for bypass_crossfade_ref.replay(): the rows stay on the device, a
    call reads them where the case has got to."""

    def __init__(self, gpu, kind, x, signal):
        self.kind, self.at, self.n = kind, 0, x.shape[1]
        self.bank = gpu.BypassBank(1) if kind == bc.BYPASS else gpu.CrossfadeBank(1)
        self.a, self.b = gpu.DeviceBuffer.from_host(x[signal[0]]), gpu.DeviceBuffer.from_host(x[signal[1]])
        self.out = gpu.DeviceBuffer.from_host(np.zeros(self.n, f32))
        self.samples = 0

    def init(self, sample_rate, time):
        self.bank.init(0, sample_rate, time)
        length = bc.ramp_length(sample_rate, time)
        self.samples = int(length)

    def set_bypass(self, bypass):
        return self.bank.set_bypass(0, bypass)

    def set_fields(self, state, delta, gain):
        self.bank.set_state(0, state, delta, gain)

    def toggle(self):
        return self.bank.toggle(0)

    def reset(self):
        self.bank.reset(0)

    def process(self, ra, rb, *more):
        at = 4 * self.at
        pa, pb = (None if ra is None else self.a.ptr + at), (None if rb is None else self.b.ptr + at)
        if self.kind == bc.CROSSFADE:
            count = more[0]
            self.bank.process(self.out.ptr + at, pa, pb, count)
        else:
            count = len(rb)
            variant, wet_gain, dry_gain = (list(more) + [bc.PROCESS, 1.0, 1.0][len(more):])
            if variant == bc.PROCESS:
                self.bank.process(self.out.ptr + at, pa, pb, count)
            elif variant == bc.PROCESS_WET:
                self.bank.process_wet(self.out.ptr + at, pa, pb, wet_gain, count)
            else:
                self.bank.process_drywet(self.out.ptr + at, pa, pb, dry_gain, wet_gain, count)
        self.at += count
        return np.zeros(count, f32)

    def final(self):
        s = self.bank.get_state(0)
        if self.kind == bc.BYPASS:
            return [s["state"], bc.bits(s["delta"]), bc.bits(s["gain"]), 0]
        assert self.bank.remaining(0) == s["counter"]
        return [self.samples, s["counter"], bc.bits(s["delta"]), bc.bits(s["gain"])]


def _copied_in(case, x):
    unit = bc.Bypass() if case["kind"] == bc.BYPASS else bc.Crossfade()
    return bc.replay(case, x, unit)[1]


@pytest.mark.gpu
def test_every_recorded_reference_case_through_the_c_abi(gpu):
    """tests/golden/bypass_crossfade_ref_vectors.npz, operation by operation, through a bank of one channel: the samples, the
    answers of set_bypass() and toggle() and the final state are the reference's."""
    x, cases = gen.load()
    for c in cases:
        unit = _OnTheBank(gpu, c["kind"], x, c["signal"])
        _, _, answers = bc.replay(c, x, unit)
        assert np.array_equal(answers, c["answers"]), c["name"]
        assert bc.same(unit.out.download(), c["out"], _copied_in(c, x)), c["name"]
        assert unit.final() == [int(v) for v in c["state"]], c["name"]
        unit.bank.close()


@pytest.mark.gpu
def test_every_recorded_reference_case_through_the_cpp_classes(gpu, tmp_path):
    """The program that recorded the cases from the reference's classes, compiled against this library's classes instead."""
    src, exe = str(tmp_path / "driver.cpp"), str(tmp_path / "driver")
    open(src, "w").write(gen.DRIVER)
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-I" + os.path.join(PKG, "include"), "-I" + os.path.join(ROOT, "include"), src,
                           "-o", exe, "-L" + PKG, "-lmi_dspu", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    x, cases = gen.load()
    made = [(c["name"], c["kind"], c["signal"], c["ops"]) for c in cases]
    out, state, answers = gen.run(exe, x, made, str(tmp_path))
    at = 0
    for c, o, s in zip(cases, out, state):
        assert bc.same(o, c["out"], _copied_in(c, x)), c["name"]
        assert [int(v) for v in s] == [int(v) for v in c["state"]], c["name"]
        assert np.array_equal(answers[at:at + len(c["ops"])], c["answers"]), c["name"]
        at += len(c["ops"])
    keys = subprocess.check_output([exe, "keys"]).decode().split("\n")
    assert keys[0].split() == ["sizeof", "12", "24"]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["bypass", "crossfade"])
def test_full_size_every_channel(gpu, kind):
    C, n = 1024, 4096
    a, b = _rows(30, C, n), _rows(31, C, n)
    if kind == "bypass":
        bank, refs = gpu.BypassBank(C), [bc.Bypass() for _ in range(C)]
        for ch, r in enumerate(refs):
            length = LENGTHS[ch % 4]
            bank.init(ch, *_init_args(length))
            r.init(*_init_args(length))
            if ch % 3:
                bank.set_bypass(ch, True)
                r.set_bypass(True)
        d_a, d_b, out = gpu.DeviceBuffer.from_host(a), gpu.DeviceBuffer.from_host(b), gpu.DeviceBuffer((C, n))
        bank.process_drywet(out, d_a, d_b, DRY_GAIN, WET_GAIN, n)
        want, copied = _bypass_want(refs, bc.PROCESS_DRYWET, a, b)
        got = out.download()
        assert all(bc.same(got[ch], want[ch], copied[ch]) for ch in range(C))
        for ch in range(0, C, 37):
            s = bank.get_state(ch)
            assert (s["state"], bc.bits(s["delta"]), bc.bits(s["gain"])) == refs[ch].fields(), ch
    else:
        bank, refs = gpu.CrossfadeBank(C), [bc.Crossfade() for _ in range(C)]
        for ch, r in enumerate(refs):
            length = LENGTHS[ch % 4]
            bank.init(ch, *_init_args(length))
            r.init(*_init_args(length))
            if ch % 3:
                bank.toggle(ch)
                r.toggle()
        d_a, d_b, out = gpu.DeviceBuffer.from_host(a), gpu.DeviceBuffer.from_host(b), gpu.DeviceBuffer((C, n))
        bank.process(out, d_a, d_b, n)
        got = out.download()
        for ch, r in enumerate(refs):
            want, copied = r.process(a[ch], b[ch], n)
            assert bc.same(got[ch], want, copied), ch
        for ch in range(0, C, 37):
            s = bank.get_state(ch)
            assert (s["counter"], bc.bits(s["delta"]), bc.bits(s["gain"])) == refs[ch].fields(), ch
    bank.close()
