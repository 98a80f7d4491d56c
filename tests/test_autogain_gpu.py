"""The AutoGain bank on the device against the float32 restatement of tests/autogain_ref.py, bit for bit: the gain of every
sample and fCurrGain, fOutGain and the surge flags after every call.  The restatement is fed the bank's own parameters."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import autogain_ref as ar

pytestmark = pytest.mark.gpu
f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "lsp-dsp-units_amd")
N = sum(ar.LENGTHS)
CUTS = (1, 3, 255, 256, 257, N - 772)            # the call sizes, and what is left of the signal


def _bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a, f32).view(np.uint32), np.ascontiguousarray(b, f32).view(np.uint32))


class Rig:
    """a bank, its restatement, and the calls on both"""

    def __init__(self, gpu, channels, same=False):
        self.gpu, self.C = gpu, channels
        self.bank = gpu.AutoGainBank(channels)
        for ch in range(channels):
            quick, limit = ar.switches(ch)
            self.bank.configure(ch, quick_amp=quick, limit=limit, **(ar.SETTINGS if same else ar.settings_of(ch)))
        self.bank.update_settings()
        self.ref = ar.AutoGain(self.params())

    def params(self):
        return [self.bank.get_params(ch) for ch in range(self.C)]

    def sync(self):
        self.ref.set_params(self.params())

    def want(self, ll, ls, le):
        return self.ref.process(ll, ls, le)

    def run(self, ll, ls, le, what="", stream=None):
        n = ll.shape[1]
        d = [self.gpu.DeviceBuffer.from_host(x) for x in (ll, ls, le)]
        out = self.gpu.DeviceBuffer((self.C, n))
        self.bank.process(out, d[0], d[1], d[2], n, stream=stream)
        got, want = out.download(stream=stream), self.want(ll, ls, le)
        bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
        assert len(bad) == 0, (what, "first difference at (channel, sample)", bad[0], got[tuple(bad[0])], want[tuple(bad[0])], len(bad))
        self.check_state(what, stream)
        return got

    def check_state(self, what="", stream=None):
        for ch in range(self.C):
            g, o, f = self.bank.get_state(ch, stream=stream)
            assert _bits_equal(g, self.ref.gain[ch]) and _bits_equal(o, self.ref.out[ch]) and f == self.ref.flags(ch), \
                (what, ch, g, self.ref.gain[ch], o, self.ref.out[ch], f, self.ref.flags(ch))

    def assert_every_branch(self, what=""):
        """a condition of the test: the input reached every branch its channel's switches allow"""
        for ch in range(self.C):
            missed = [k for k in ar.expected_counters(*ar.switches(ch)) if self.ref.counters[k][ch] == 0]
            assert not missed, (what, ch, ar.switches(ch), missed)

    def close(self):
        self.bank.close()


def _cut(x, a, b):
    return tuple(v[:, a:b] for v in x)


@pytest.mark.parametrize("channels", [1, 4, 5, 9])
def test_short_calls_equal_one_long_call(gpu, channels):
    """channels: one, a full group, a partial group behind it, several workgroups; calls of 1, 3, 255, 256, 257 samples and the
    rest, then the 1100 samples in one call on a second bank"""
    x = ar.signal(11 + channels, channels)
    rig, whole = Rig(gpu, channels), Rig(gpu, channels)
    parts, at = [], 0
    for n in CUTS:
        parts.append(rig.run(*_cut(x, at, at + n), what="call of %d at %d" % (n, at)))
        at += n
    assert at == N
    one = whole.run(*x, what="one call")
    assert _bits_equal(np.concatenate(parts, axis=1), one)
    for r in (rig, whole):
        r.assert_every_branch()
        r.close()


@pytest.mark.parametrize("first", [255, 256])
def test_a_jump_at_the_tile_edge_and_at_the_end_of_a_call(gpu, first):
    """the surge up begins at the last sample of tile 0 or at the first of tile 1, and is the last sample of a call: the flag is
    carried across the tile and across the call"""
    C = 5
    x = ar.signal(23, C, lengths=(first,) + ar.LENGTHS[1:])
    n = x[0].shape[1]
    rig, whole = Rig(gpu, C), Rig(gpu, C)
    a = rig.run(*_cut(x, 0, first + 1), what="up to the jump")
    assert all(rig.ref.surge == ar.F_SURGE_UP) and all(rig.bank.get_state(ch)[2] & ar.F_SURGE_UP for ch in range(C))
    b = rig.run(*_cut(x, first + 1, n), what="after the jump")
    assert _bits_equal(np.concatenate([a, b], axis=1), whole.run(*x, what="one call"))
    whole.assert_every_branch()
    rig.close()
    whole.close()


@pytest.mark.parametrize("row", [0, 1, 2])
def test_vca_may_be_any_input_row(gpu, row):
    C = 6
    x = ar.signal(31, C)
    rig = Rig(gpu, C)
    d = [gpu.DeviceBuffer.from_host(v) for v in x]
    rig.bank.process(d[row], d[0], d[1], d[2], N)
    assert _bits_equal(d[row].download(), rig.want(*x))
    for k in range(3):
        if k != row:
            assert _bits_equal(d[k].download(), x[k])                   # the other inputs are untouched
    rig.check_state()
    rig.assert_every_branch()
    rig.close()


@pytest.mark.parametrize("strides", [(1101, 1103, 1105, 1107), (1104, 1100, 1112, 1108)])
def test_odd_strides_and_unaligned_rows(gpu, strides):
    """rows that start off 16 bytes and strides that are no multiple of four floats take the lanes' one-by-one loads and stores"""
    C, off = 5, 1
    x = ar.signal(37, C)
    rig = Rig(gpu, C)
    bufs = []
    for v, st in zip((np.zeros_like(x[0]),) + x, strides):
        host = np.full(off + C * st, -7.0, f32)
        host[off:].reshape(C, st)[:, :N] = v
        bufs.append((gpu.DeviceBuffer.from_host(host), host))
    p = [b.ptr + 4 * off for b, _ in bufs]
    rig.bank.process(p[0], p[1], p[2], p[3], N, vca_stride=strides[0], long_stride=strides[1], short_stride=strides[2],
                     exp_stride=strides[3])
    got = bufs[0][0].download()
    assert _bits_equal(got[off:].reshape(C, strides[0])[:, :N], rig.want(*x))
    assert np.all(got[off:].reshape(C, strides[0])[:, N:] == -7.0) and got[0] == -7.0      # nothing written beside the rows
    for (b, host) in bufs[1:]:
        assert _bits_equal(b.download(), host)
    rig.check_state()
    rig.assert_every_branch()
    rig.close()


def test_process_level_is_process_with_constant_rows(gpu):
    C = 5
    ll, ls, le = ar.signal(41, C)
    levels = (ar.LEXP * (1 + 0.125 * np.arange(C))).astype(f32)
    le = np.repeat(levels[:, None], N, axis=1)
    ll[:, 0] = levels                                                   # the crafted sample, for every channel's own level
    rig, twin = Rig(gpu, C), Rig(gpu, C)
    want = rig.run(ll, ls, le, what="rows")
    d = [gpu.DeviceBuffer.from_host(v) for v in (ll, ls, levels)]
    out = gpu.DeviceBuffer((C, N))
    twin.bank.process_level(out, d[0], d[1], d[2], N)
    assert _bits_equal(out.download(), want)
    twin.ref = rig.ref
    twin.check_state()
    rig.assert_every_branch()
    rig.close()
    twin.close()


def test_process_apply_is_process_and_one_multiply(gpu):
    C = 5
    x = ar.signal(43, C)
    audio = np.random.default_rng(47).standard_normal((C, N)).astype(f32)
    rig = Rig(gpu, C)
    d = [gpu.DeviceBuffer.from_host(v) for v in x]
    da = gpu.DeviceBuffer.from_host(audio)
    rig.bank.process_apply(da, da, d[0], d[1], d[2], N)                 # in place on the audio
    assert _bits_equal(da.download(), audio * rig.want(*x))
    rig.check_state()
    rig.assert_every_branch()
    rig.close()


def test_the_setters_without_an_update_reach_the_next_call(gpu):
    """enable_quick_amplifier, set_silence_threshold, set_max_gain and enable_max_gain raise no F_UPDATE and still change the
    next call: channel 0 takes one of them before each call and is held against the restatement and against a bank left alone"""
    C = 4
    x = ar.signal(53, C)
    rig, plain = Rig(gpu, C, same=True), Rig(gpu, C, same=True)
    cuts = [0, 300, 500, 600, 800, N]
    changes = [None, lambda b: b.enable_quick_amplifier(0, False), lambda b: b.set_silence_threshold(0, 0.01),
               lambda b: b.set_max_gain(0, 0.05), lambda b: b.enable_max_gain(0, False)]
    delta = []
    for k in range(5):
        if changes[k] is not None:
            changes[k](rig.bank)
            rig.sync()                                                  # get_params shows the setter's value at once
        part = _cut(x, cuts[k], cuts[k + 1])
        before = [{n: v[0] for n, v in r.ref.counters.items()} for r in (rig, plain)]
        got, other = rig.run(*part, what="call %d" % k), plain.run(*part)
        assert [_bits_equal(got[ch], other[ch]) for ch in range(C)] == [k == 0, True, True, True], k
        delta.append([{n: r.ref.counters[n][0] - c[n] for n in c} for r, c in zip((rig, plain), before)])
    assert delta[1][0]["short_grow"] == 0 and delta[1][1]["short_grow"] > 100      # no quick amplifier after the drop
    assert delta[2][0]["silence"] == 100 and delta[2][1]["silence"] == 50          # 0.004 is silence now
    assert delta[3][0]["max_gain_hit"] == 200 and rig.bank.get_state(0)[1] < 0.5   # fOutGain = 0.05 / fCurrGain
    assert delta[4][0]["creep"] == 300 and 0.4 < rig.bank.get_state(0)[1] < 1      # ... and creeps up by sLong.fKGrow from there
    rig.close()
    plain.close()


def test_all_silence(gpu):
    C = 5
    rig = Rig(gpu, C)
    x = ar.signal(59, C)
    rig.run(*_cut(x, 0, 300), what="sound")                             # so that the gains are not 1
    quiet = (np.zeros((C, 300), f32), np.full((C, 300), 1e-5, f32), x[2][:, :300])
    got = rig.run(*quiet, what="silence")
    assert np.all(rig.ref.counters["silence"] >= 300)
    assert all(np.unique(got[ch]).size <= (1 if ar.switches(ch)[1] else 300) for ch in range(C))
    rig.close()


def test_full_size_every_channel(gpu):
    """1024 channels x 4096 samples in one call, every channel against the restatement"""
    C, n = 1024, 4096
    lengths = ar.LENGTHS * 3 + (150, 200, 200, 100, 146)
    x = ar.signal(61, C, lengths=lengths)
    rig = Rig(gpu, C)
    rig.run(*x, what="full size")
    rig.assert_every_branch()
    rig.close()


def _capture(gpu, st, calls):
    gpu.check(gpu.lib.mi_dspu_graph_begin_capture(st))
    calls()
    exe = ctypes.c_void_p()
    gpu.check(gpu.lib.mi_dspu_graph_end_capture(st, ctypes.byref(exe)))
    return exe


def test_graph_capture_replays_direct_calls(gpu):
    C, n = 9, 550
    st = ctypes.c_void_p()
    gpu.check(gpu.lib.mi_dspu_stream_create(ctypes.byref(st)))
    rig, twin = Rig(gpu, C), Rig(gpu, C)
    x = ar.signal(67, C)
    a, b = _cut(x, 0, n), _cut(x, n, 2 * n)
    levels = gpu.DeviceBuffer.from_host(b[2][:, 0])
    da, db = [gpu.DeviceBuffer.from_host(v) for v in a], [gpu.DeviceBuffer.from_host(v) for v in b]
    g0, g1, t0, t1 = (gpu.DeviceBuffer((C, n)) for _ in range(4))

    def calls(bank, o0, o1):
        bank.process(o0, da[0], da[1], da[2], n, stream=st.value)
        bank.process_level(o1, db[0], db[1], levels, n, stream=st.value)
    exe = _capture(gpu, st, lambda: calls(rig.bank, g0, g1))
    for rep in range(2):
        gpu.check(gpu.lib.mi_dspu_graph_launch(exe, st))
        calls(twin.bank, t0, t1)
        got = [v.download(stream=st.value) for v in (g0, g1)]
        direct = [v.download(stream=st.value) for v in (t0, t1)]
        assert all(_bits_equal(p, q) for p, q in zip(got, direct)), rep
        assert _bits_equal(got[0], rig.want(*a)) and _bits_equal(got[1], rig.want(*b)), rep     # the state advances on every replay
        rig.check_state("replay %d" % rep, stream=st.value)
    rig.assert_every_branch()
    gpu.lib.mi_dspu_graph_destroy(exe)
    rig.close()
    twin.close()
    gpu.check(gpu.lib.mi_dspu_stream_destroy(st))


def test_inside_a_capture_a_settings_change_is_refused(gpu):
    C, n = 4, 550
    st = ctypes.c_void_p()
    gpu.check(gpu.lib.mi_dspu_stream_create(ctypes.byref(st)))
    rig = Rig(gpu, C)
    x = ar.signal(71, C)
    rig.run(*_cut(x, 0, n), what="before", stream=st.value)
    d = [gpu.DeviceBuffer.from_host(v) for v in _cut(x, n, 2 * n)]
    out = gpu.DeviceBuffer((C, n))

    def inside():
        rig.bank.set_deviation(1, 3.0)                                  # raises F_UPDATE
        rig.bank.enable_quick_amplifier(3, True)                        # does not, and is an upload all the same
        for call in (lambda: rig.bank.process(out, d[0], d[1], d[2], n, stream=st.value),
                     lambda: rig.bank.update_settings(stream=st.value)):
            with pytest.raises(gpu.MiError) as e:
                call()
            assert e.value.code == -5 and "update_settings" in str(e.value)
        with pytest.raises(gpu.MiError) as e:
            rig.bank.get_state(0, stream=st.value)
        assert e.value.code == -5 and "captured" in str(e.value)
        gpu.check(gpu.lib.mi_dspu_memset(ctypes.c_void_p(out.ptr), 0, 16, st))      # (so that the capture is not empty)
    exe = _capture(gpu, st, inside)
    assert exe.value
    gpu.lib.mi_dspu_graph_destroy(exe)
    rig.bank.process(out, d[0], d[1], d[2], n, stream=st.value)         # the settings apply now, to the state from before
    rig.sync()
    assert _bits_equal(out.download(stream=st.value), rig.want(*_cut(x, n, 2 * n)))
    rig.check_state(stream=st.value)
    rig.close()
    gpu.check(gpu.lib.mi_dspu_stream_destroy(st))


CPP = r"""
#include <lsp-plug.in/dsp-units/dynamics/AutoGain.h>
#include <cstdio>
#include <vector>
struct Readable: public lsp::dspu::AutoGain
{
    void read(float *dst) const { dst[0] = fCurrGain; dst[1] = fOutGain; dst[2] = float(nFlags); }
};
int main(int argc, char **argv)
{
    const size_t n = 1100, h = 550;
    FILE *f = fopen(argv[1], "rb");
    std::vector<float> x(3 * n), out(n + 6);                    // llong, lshort, lexp; the gain and the state after each call
    if (fread(x.data(), sizeof(float), x.size(), f) != x.size()) return 2;
    fclose(f);
    Readable a;
    a.init();
    a.set_sample_rate(1000);
    a.set_short_speed(160.0f, 320.0f);
    a.set_long_speed(5.0f, 10.0f);
    a.set_silence_threshold(2.5119e-4f);
    a.set_deviation(1.99526f);
    a.set_max_gain(2.0f, true);
    a.enable_quick_amplifier(true);
    if (!a.needs_update()) return 3;
    const float *ll = x.data(), *ls = ll + n, *le = ls + n;
    a.process(out.data(), ll, ls, le, h);                       // rows, then the level
    a.read(out.data() + n);
    a.process(out.data() + h, ll + h, ls + h, le[h], n - h);
    a.read(out.data() + n + 3);
    f = fopen(argv[2], "wb");
    fwrite(out.data(), sizeof(float), out.size(), f);
    fclose(f);
    a.destroy();
    return 0;
}
"""


def test_the_cpp_class_is_a_bank_of_one_channel(gpu, tmp_path):
    src, exe = str(tmp_path / "autogain.cpp"), str(tmp_path / "autogain")
    open(src, "w").write(CPP)
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-I" + os.path.join(PKG, "include"), "-I" + os.path.join(ROOT, "include"), src,
                           "-o", exe, "-L" + PKG, "-lmi_dspu", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    x = ar.signal(73, 1)
    np.concatenate([v[0] for v in x]).tofile(str(tmp_path / "in.bin"))
    out = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out
    r = np.fromfile(str(tmp_path / "out.bin"), f32)
    rig = Rig(gpu, 1, same=True)                                # channel 0: quick amplifier and limiting, as the program sets
    h = 550
    assert _bits_equal(r[:h], rig.run(*_cut(x, 0, h), what="rows")[0])
    assert _bits_equal(r[N:N + 2], [rig.ref.gain[0], rig.ref.out[0]]) and int(r[N + 2]) == rig.ref.flags(0)
    assert _bits_equal(r[h:N], rig.run(*_cut(x, h, N), what="level")[0])
    assert _bits_equal(r[N + 3:N + 5], [rig.ref.gain[0], rig.ref.out[0]]) and int(r[N + 5]) == rig.ref.flags(0)
    rig.assert_every_branch()
    rig.close()
