"""Row enable on the LCG, MLS and Velvet banks, and the Velvet bank's overwrite in segments of 256.

A channel that is switched off is an object on which nobody calls process(): its row keeps what it held, its state words do not move,
and a state (or, for MLS, an update_settings()) that is pending waits for the call that takes the channel in again.  Banks of 17
channels so that LCG workgroups of four are fully on, partly on and fully off.  Samples and state words are compared as
test_noise_gpu.py and test_velvet_gpu.py compare them (the helpers are theirs)."""
import copy

import numpy as np
import pytest

import noise_ref as R
import velvet_ref as V
from test_noise_gpu import ADD, ESTATE, MUL, OVERWRITE, many_channels
from test_velvet_gpu import Bank, configure, same_rows, source, unit_of, words

f32 = np.float32
C = 17
OFF = (1, 4, 5, 6, 7, 16)                                   # one of a workgroup, a whole workgroup, the last workgroup's only channel
MARK = f32(9.0)


def want_of_the_enabled(u, off, n, op=OVERWRITE, src=None):
    """What the restatements make of a call that leaves `off` out: their units stand still."""
    kept = {ch: copy.deepcopy(u.refs[ch]) for ch in off}
    want = u.want(n, op, src)
    for ch in off:
        u.refs[ch] = kept[ch]
    return want


def check_rows(u, got, want, off, start, label):
    star, others, trans = want
    for ch in range(u.C):
        if ch in off:
            assert np.array_equal(got[ch], start[ch]), (label, ch, "a disabled row was written")
            continue
        bad = R.agree(got[ch], star[ch], star[ch], others[ch], trans[ch])
        assert bad.size == 0, (label, ch, bad[:5], got[ch][bad[:5]], star[ch][bad[:5]])


@pytest.mark.gpu
@pytest.mark.parametrize("lcg", [True, False], ids=["lcg", "mls"])
def test_disabled_rows_and_states_stay_and_a_pending_state_waits(gpu, lcg):
    u = many_channels(gpu, C, lcg)
    n, stride = 777, 780
    for ch in OFF:
        u.bank.set_row_enabled(ch, False)
    start = np.full((C, stride), MARK, f32)
    out = gpu.DeviceBuffer.from_host(start)
    for call in range(2):                                   # the second call goes on where the first stopped
        u.bank.process(out, n, dst_stride=stride)
        got = out.download()
        check_rows(u, got[:, :n], want_of_the_enabled(u, OFF, n), OFF, start[:, :n], ("overwrite", call))
        assert (got[:, n:] == MARK).all()
        u.check_states(("overwrite", call))
    # a state given to a disabled channel is pending: get_state shows it, calls pass it by
    for ch in (4, 16):
        if lcg:
            u.set(ch, R.INIT, 0xBEEF00 + ch)
        else:
            u.set(ch, R.SET_N_BITS, 11 + ch)
            u.set(ch, R.SET_STATE, 0x1357 + ch, 0)
            assert u.bank.needs_update(ch)
    src = np.stack([np.linspace(-1.0, 1.0, stride, dtype=f32) * f32(k + 1) for k in range(C)])
    s = gpu.DeviceBuffer.from_host(src)
    for op in (ADD, MUL):
        out.upload(start)
        u.bank.process(out, n, src=s, op=op, dst_stride=stride, src_stride=stride)
        got = out.download()
        check_rows(u, got[:, :n], want_of_the_enabled(u, OFF, n, op, src[:, :n]), OFF, start[:, :n], ("with a source", op))
        u.check_states(("pending", op))
        if not lcg:
            assert u.bank.needs_update(4) and u.bank.needs_update(16) and not u.bank.needs_update(0)
    # in place, some rows off: they keep their source
    out.upload(src)
    u.bank.process(out, n, src=out, op=ADD, dst_stride=stride, src_stride=stride)
    check_rows(u, out.download()[:, :n], want_of_the_enabled(u, OFF, n, ADD, src[:, :n]), OFF, src[:, :n], "in place")
    # taken in again: the pending states are taken, the others go on from where they stood
    for ch in OFF:
        u.bank.set_row_enabled(ch, True)
    for k in (257, n):
        out.upload(start)
        u.bank.process(out, k, dst_stride=stride)
        check_rows(u, out.download()[:, :k], u.want(k), (), start[:, :k], ("enabled again", k))
        u.check_states(("enabled again", k))
    if not lcg:
        assert not any(u.bank.needs_update(ch) for ch in range(C))
    out.free()
    s.free()
    u.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["lcg", "mls", "velvet"])
def test_a_bank_with_no_enabled_row_does_nothing(gpu, kind):
    n = 300
    start = np.full((C, n), MARK, f32)
    out = gpu.DeviceBuffer.from_host(start)
    if kind == "velvet":
        b = Bank(gpu, C)
        bank, states = b.bank, b.check_words
    else:
        u = many_channels(gpu, C, kind == "lcg")
        bank, states = u.bank, u.check_states
    for ch in range(C):
        bank.set_row_enabled(ch, False)
    for op in (OVERWRITE, ADD, MUL):
        bank.process(out, n, src=None if op == OVERWRITE else out, op=op)
        assert np.array_equal(out.download(), start), (kind, op)
    if kind == "velvet":
        bank.process(out, n, src=None, op=MUL)              # the zero fill is a row's process() too
        bank.process_segmented(out, n)
        assert np.array_equal(out.download(), start)
    states(kind)
    bank.close()
    out.free()


@pytest.mark.gpu
def test_a_disabled_channel_need_not_be_inited(gpu):
    out = gpu.DeviceBuffer.from_host(np.full((3, 64), MARK, f32))
    for make in (gpu.LCGBank, gpu.VelvetBank):
        bank = make(3)
        bank.init(0, 1)
        bank.init(2, 2)
        with pytest.raises(gpu.MiError) as e:
            bank.process(out, 64)
        assert e.value.code == ESTATE and "init" in str(e.value)
        bank.set_row_enabled(1, False)
        bank.process(out, 64)
        got = out.download()
        assert (got[1] == MARK).all() and not (got[0] == MARK).all() and not (got[2] == MARK).all()
        bank.set_row_enabled(1, True)
        with pytest.raises(gpu.MiError) as e:
            bank.process(out, 64)
        assert e.value.code == ESTATE
        bank.close()
    out.free()


def velvet_want(b, off, what, src, n):
    kept = {k: copy.deepcopy(b.units[k]) for k in off}
    want = b.want(what, src, n)
    for k in off:
        b.units[k] = kept[k]
    return want


@pytest.mark.gpu
def test_velvet_disabled_rows_and_states_stay_and_a_pending_state_waits(gpu):
    n, stride = 700, 704
    b = Bank(gpu, C)
    src = source(C, stride)
    s = gpu.DeviceBuffer.from_host(src)
    for k in OFF:
        b.bank.set_row_enabled(k, False)
    start = np.full((C, stride), MARK, f32)
    out = gpu.DeviceBuffer.from_host(start)

    def call(what, label, off=OFF):
        out.upload(start)
        null = what in (R.P_OVERWRITE, V.P_ADD_NULL, V.P_MUL_NULL)
        op = {R.P_OVERWRITE: OVERWRITE, R.P_ADD: ADD, R.P_MUL: MUL, V.P_ADD_NULL: ADD, V.P_MUL_NULL: MUL}[what]
        b.bank.process(out, n, src=None if null else s, op=op, dst_stride=stride, src_stride=stride)
        got = out.download()
        want = velvet_want(b, off, what, src[:, :n], n)
        keep = [k for k in range(C) if k not in off]
        same_rows(got[keep, :n], want[keep], label)
        assert (got[list(off)] == MARK).all() and (got[:, n:] == MARK).all(), label
        b.check_words(label)

    for what in (R.P_OVERWRITE, R.P_ADD, R.P_MUL, V.P_ADD_NULL, V.P_MUL_NULL):
        call(what, ("off", what))
    # a pending set_state and a pending init on disabled rows: shown by get_state, passed by, taken when the row runs again
    b.units[4] = unit_of(40, 0x7000)
    configure(b.bank, 4, b.units[4])
    b.units[16].init(0x1234, 17, 0x99)
    b.bank.init(16, 0x1234, 17, 0x99)
    call(R.P_OVERWRITE, "pending")
    call(R.P_ADD, "pending, with a source")
    for k in OFF:
        b.bank.set_row_enabled(k, True)
    call(R.P_OVERWRITE, "enabled again", ())
    call(R.P_MUL, "enabled again, mul", ())
    out.free()
    s.free()
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1100])
def test_velvet_overwrite_in_segments_is_a_loop_of_overwrites_of_256(gpu, n):
    stride = 1104
    whole, cut = Bank(gpu, C, 0x6100), Bank(gpu, C, 0x6100)
    a = gpu.DeviceBuffer.from_host(np.full((C, stride), MARK, f32))
    c = gpu.DeviceBuffer.from_host(np.full((C, stride), MARK, f32))
    whole.bank.process_segmented(a, n, dst_stride=stride)
    want = np.zeros((C, n), f32)
    for at in range(0, n, 256):
        k = min(256, n - at)
        cut.bank.process(c.ptr + 4 * at, k, dst_stride=stride)
        want[:, at:at + k] = whole.want(R.P_OVERWRITE, None, k)
    got = a.download()
    same_rows(got[:, :n], want, ("restatement", n))
    same_rows(got, c.download(), ("loop of calls", n))
    whole.check_words(n)
    for k in range(C):
        assert np.array_equal(words(whole.bank, k), words(cut.bank, k)), k
    if n > 256:                                             # ... and not one overwrite of n: the window scan restarts
        one = Bank(gpu, C, 0x6100)
        o = gpu.DeviceBuffer((C, stride))
        one.bank.process(o, n, dst_stride=stride)
        assert not np.array_equal(o.download()[:, :n], got[:, :n])
        o.free()
        one.close()
    a.free()
    c.free()
    whole.close()
    cut.close()
