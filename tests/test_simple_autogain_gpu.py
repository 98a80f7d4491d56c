"""The SimpleAutoGain bank on the device against the float32 restatement of tests/autogain_ref.py, bit for bit: the gain of every
sample and fCurrGain after every call, the limits' setters in their order included."""
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
N = 1100
CUTS = (1, 3, 255, 256, 257, N - 772)
TINY = float(np.finfo(f32).tiny)                # the smallest normal float32


def _bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a, f32).view(np.uint32), np.ascontiguousarray(b, f32).view(np.uint32))


def settings_of(ch):
    """100 dB/s up and 120 dB/s down at 1000 Hz: from one limit to the other within 250 samples"""
    k = ch % 5
    return dict(sample_rate=1000, grow=100.0 + 2 * k, fall=120.0 - 3 * k, threshold=0.1 + 0.005 * k, lo=0.25 - 0.01 * k, hi=4.0 + 0.25 * k)


class Rig:
    def __init__(self, gpu, channels, settings=settings_of):
        self.gpu, self.C = gpu, channels
        self.bank = gpu.SimpleAutoGainBank(channels)
        for ch in range(channels):
            s = settings(ch)
            self.bank.set_sample_rate(ch, s["sample_rate"])
            self.bank.set_speed(ch, s["grow"], s["fall"])
            self.bank.set_threshold(ch, s["threshold"])
            self.bank.set_gain(ch, s["lo"], s["hi"])
        self.bank.update_settings()
        self.ref = ar.SimpleAutoGain([self.bank.get_params(ch) for ch in range(channels)])
        for ch in range(channels):
            self.ref.gain[ch] = ar.lsp_limit(f32(1.0), self.ref.min_gain[ch], self.ref.max_gain[ch])      # what set_gain did

    def set(self, ch, name, *values):
        """one of set_max_gain, set_min_gain, set_gain on both, with the reference's early return"""
        lo, hi = self.ref.min_gain[ch], self.ref.max_gain[ch]
        getattr(self.bank, name)(ch, *values)
        unchanged = {"set_max_gain": lambda: hi == f32(values[0]), "set_min_gain": lambda: lo == f32(values[0]),
                     "set_gain": lambda: lo == f32(values[0]) and hi == f32(values[-1])}[name]()
        if not unchanged:
            getattr(self.ref, name)(ch, *values)

    def run(self, x, what="", stream=None):
        n = x.shape[1]
        d, out = self.gpu.DeviceBuffer.from_host(x), self.gpu.DeviceBuffer((self.C, n))
        self.bank.process(out, d, n, stream=stream)
        got, want = out.download(stream=stream), self.ref.process(x)
        bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
        assert len(bad) == 0, (what, "first difference at (channel, sample)", bad[0], got[tuple(bad[0])], want[tuple(bad[0])], len(bad))
        self.check_state(what, stream)
        return got

    def check_state(self, what="", stream=None):
        got = [self.bank.get_state(ch, stream=stream) for ch in range(self.C)]
        assert _bits_equal(got, self.ref.gain), (what, got, self.ref.gain)

    def assert_reached(self, names, what=""):
        for ch in range(self.C):
            missed = [k for k in names if self.ref.counters[k][ch] == 0]
            assert not missed, (what, ch, missed)

    def close(self):
        self.bank.close()


@pytest.mark.parametrize("channels", [1, 4, 5, 9])
def test_short_calls_equal_one_long_call_and_both_limits_are_reached(gpu, channels):
    x = ar.simple_signal(7 + channels, channels, N)
    rig, whole = Rig(gpu, channels), Rig(gpu, channels)
    parts, at = [], 0
    for n in CUTS:
        parts.append(rig.run(x[:, at:at + n], what="call of %d at %d" % (n, at)))
        at += n
    assert at == N and _bits_equal(np.concatenate(parts, axis=1), whole.run(x, what="one call"))
    for r in (rig, whole):
        r.assert_reached(("grow", "fall", "at_min", "at_max", "inside"))
        r.close()


def test_a_level_exactly_at_the_threshold_leaves_the_gain(gpu):
    """the gain parked at max = 1 and src = threshold: s == threshold, neither factor is taken"""
    C, n = 5, 300
    rig = Rig(gpu, C, settings=lambda ch: dict(sample_rate=1000, grow=50.0, fall=200.0, threshold=0.1 + 0.01 * ch, lo=1e-6, hi=1.0))
    x = np.repeat(rig.ref.threshold[:, None], n, axis=1)
    x[1, 100:] *= f32(4.0)                                              # channel 1 leaves the threshold, falls and comes back up
    x[1, 200:] = f32(0.01)
    got = rig.run(x, what="at the threshold")
    assert np.all(got[[0, 2, 3, 4]] == 1) and np.all(rig.ref.counters["equal"][[0, 2, 3, 4]] == n)
    assert rig.ref.counters["equal"][1] == 100 and got[1].min() < 0.5 and rig.ref.counters["grow"][1] >= 100
    rig.close()


def test_the_gain_decays_into_subnormals(gpu):
    """7 dB per sample down under a subnormal min_gain: the gain and src * gain go through the subnormals and stop at the limit;
    with min_gain = 0 the gain underflows to zero, and 0.75 * 0 is the threshold"""
    C, n = 4, 400
    lows = [1e-40, 3e-42, 1.4e-45, 0.0]
    rig = Rig(gpu, C, settings=lambda ch: dict(sample_rate=1000, grow=10.0, fall=7000.0, threshold=0.0, lo=lows[ch], hi=1.0))
    got = rig.run(np.full((C, n), 0.75, f32), what="decay")
    tiny = (got > 0) & (got < TINY)
    assert np.all(tiny.sum(axis=1) >= 10), tiny.sum(axis=1)
    assert _bits_equal(got[:, -1], np.array(lows, f32)) and np.all(rig.ref.counters["at_min"][:3] > 0), (got[:, -1], rig.ref.counters)
    assert rig.ref.counters["equal"][3] > 0                             # 0.75 * 0 == threshold 0
    rig.close()


def test_the_limits_setters_act_in_their_order(gpu):
    """set_max_gain is lsp_min only, set_min_gain lsp_max only, set_gain lsp_limit, which is no clamp with min > max; the bank
    records them and the next launch applies them ahead of its first sample"""
    C = 6
    rig = Rig(gpu, C, settings=lambda ch: dict(sample_rate=1000, grow=0.0, fall=0.0, threshold=0.1, lo=1e-6, hi=1.0))    # K = 1
    x = np.full((C, 3), 0.5, f32)
    rig.set(0, "set_max_gain", 0.5)
    rig.set(0, "set_max_gain", 2.0)                                     # stays at 0.5
    rig.set(1, "set_min_gain", 3.0)
    rig.set(1, "set_min_gain", 0.5)                                     # stays at 3: above max = 1, and process() limits it to 1
    rig.set(2, "set_gain", 0.75, 0.5)                                   # 1 is not below min: above max, so 0.5
    rig.set(2, "set_gain", 0.75, 0.25)                                  # 0.5 is below min: 0.75, which process() takes to 0.25
    rig.set(3, "set_max_gain", 1.0)                                     # unchanged: nothing
    rig.set(4, "set_gain", 2.0, 8.0)
    rig.set(4, "set_max_gain", 4.0)
    assert [float(v) for v in rig.ref.gain] == [0.5, 3.0, 0.75, 1.0, 2.0, 1.0]
    rig.check_state("before any launch")                                # get_state applies what is recorded
    got = rig.run(x, what="first launch")
    assert [float(v) for v in got[:, 0]] == [0.5, 1.0, 0.25, 1.0, 2.0, 1.0]
    # many of them on several channels, interleaved: more than the table on the device held so far
    rng = np.random.default_rng(5)
    for k in range(150):
        ch = int(rng.integers(0, C))
        name = ("set_max_gain", "set_min_gain", "set_gain")[int(rng.integers(0, 3))]
        rig.set(ch, name, *[float(f32(v)) for v in rng.uniform(0.1, 3.0, 2 if name == "set_gain" else 1)])
    rig.check_state("recorded")
    rig.run(x, what="after 150 setters")
    rig.run(x, what="and again, with nothing recorded")
    rig.close()


@pytest.mark.parametrize("strides", [(1101, 1103), (1104, 1108), (1100, 1100)])
def test_strides_unaligned_rows_and_in_place(gpu, strides):
    C, off = 5, 1
    x = ar.simple_signal(19, C, N)
    rig = Rig(gpu, C)
    if strides[0] == strides[1]:
        d = gpu.DeviceBuffer.from_host(x)
        rig.bank.process(d, d, N)                                       # in place
        assert _bits_equal(d.download(), rig.ref.process(x))
    else:
        hosts = [np.full(off + C * st, -7.0, f32) for st in strides]
        hosts[1][off:].reshape(C, strides[1])[:, :N] = x
        bufs = [gpu.DeviceBuffer.from_host(h) for h in hosts]
        rig.bank.process(bufs[0].ptr + 4 * off, bufs[1].ptr + 4 * off, N, out_stride=strides[0], in_stride=strides[1])
        got = bufs[0].download()
        assert _bits_equal(got[off:].reshape(C, strides[0])[:, :N], rig.ref.process(x))
        assert np.all(got[off:].reshape(C, strides[0])[:, N:] == -7.0) and got[0] == -7.0
        assert _bits_equal(bufs[1].download(), hosts[1])
    rig.check_state()
    rig.close()


def test_full_size_every_channel(gpu):
    C, n = 1024, 4096
    rig = Rig(gpu, C)
    rig.run(ar.simple_signal(23, C, n), what="full size")
    rig.assert_reached(("grow", "fall", "at_min", "at_max", "inside"))
    rig.close()


def test_graph_capture_replays_direct_calls_and_refuses_uploads(gpu):
    C, n = 9, 300
    st = ctypes.c_void_p()
    gpu.check(gpu.lib.mi_dspu_stream_create(ctypes.byref(st)))
    rig = Rig(gpu, C)
    x = ar.simple_signal(29, C, 2 * n)
    d0, d1 = gpu.DeviceBuffer.from_host(x[:, :n]), gpu.DeviceBuffer.from_host(x[:, n:])
    g0, g1 = gpu.DeviceBuffer((C, n)), gpu.DeviceBuffer((C, n))
    rig.set(2, "set_max_gain", 0.5)                                     # recorded; sent by the call before the capture
    rig.run(x[:, :n], what="before", stream=st.value)
    gpu.check(gpu.lib.mi_dspu_graph_begin_capture(st))
    rig.bank.process(g0, d0, n, stream=st.value)
    rig.bank.process(g1, d1, n, stream=st.value)
    rig.bank.set_min_gain(3, 0.3)                                       # a recorded limit is an upload: refused in here
    with pytest.raises(gpu.MiError) as e:
        rig.bank.process(g1, d1, n, stream=st.value)
    assert e.value.code == -5
    with pytest.raises(gpu.MiError) as e:
        rig.bank.get_state(0, stream=st.value)
    assert e.value.code == -5 and "captured" in str(e.value)
    exe = ctypes.c_void_p()
    gpu.check(gpu.lib.mi_dspu_graph_end_capture(st, ctypes.byref(exe)))
    for rep in range(2):                                                # a replay sends nothing: channel 3 runs under the old limit
        gpu.check(gpu.lib.mi_dspu_graph_launch(exe, st))
        got = [v.download(stream=st.value) for v in (g0, g1)]
        assert _bits_equal(got[0], rig.ref.process(x[:, :n])) and _bits_equal(got[1], rig.ref.process(x[:, n:])), rep
    gpu.lib.mi_dspu_graph_destroy(exe)
    rig.ref.set_min_gain(3, 0.3)                                        # the next direct call sends it, ahead of its first sample
    rig.ref.set_params([rig.bank.get_params(ch) for ch in range(C)])
    rig.check_state("after the replays", stream=st.value)
    rig.run(x[:, :n], what="direct", stream=st.value)
    rig.assert_reached(("grow", "fall", "at_min", "inside"))
    rig.close()
    gpu.check(gpu.lib.mi_dspu_stream_destroy(st))


CPP = r"""
#include <lsp-plug.in/dsp-units/dynamics/SimpleAutoGain.h>
#include <cstdio>
#include <vector>
struct Readable: public lsp::dspu::SimpleAutoGain
{
    float curr() const { return fCurrGain; }
};
int main(int argc, char **argv)
{
    const size_t n = 600, h = 300;
    FILE *f = fopen(argv[1], "rb");
    std::vector<float> x(n), out(n + 3);
    if (fread(x.data(), sizeof(float), x.size(), f) != x.size()) return 2;
    fclose(f);
    Readable a;
    a.init();
    a.set_sample_rate(1000);
    a.set_speed(100.0f, 120.0f);
    a.set_threshold(0.1f);
    a.set_gain(0.25f, 4.0f);
    a.process(out.data(), x.data(), h);
    out[n] = a.curr();
    a.set_max_gain(0.5f);                                       // acts on fCurrGain at once; the device takes it over
    a.set_max_gain(2.0f);
    out[n + 1] = a.curr();
    for (size_t i = h; i < h + 10; ++i)                         // sample by sample
        out[i] = a.process(x[i]);
    a.process(out.data() + h + 10, x.data() + h + 10, n - h - 10);
    out[n + 2] = a.curr();
    f = fopen(argv[2], "wb");
    fwrite(out.data(), sizeof(float), out.size(), f);
    fclose(f);
    a.destroy();
    return 0;
}
"""


def test_the_cpp_class_is_a_bank_of_one_channel(gpu, tmp_path):
    src, exe = str(tmp_path / "simple.cpp"), str(tmp_path / "simple")
    open(src, "w").write(CPP)
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-I" + os.path.join(PKG, "include"), "-I" + os.path.join(ROOT, "include"), src,
                           "-o", exe, "-L" + PKG, "-lmi_dspu", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    n, h = 600, 300
    x = ar.simple_signal(31, 1, n)
    x[0, :100] = f32(0.01)                                      # so that the gain is above 0.5 at the first call's end
    x[0].tofile(str(tmp_path / "in.bin"))
    out = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out
    r = np.fromfile(str(tmp_path / "out.bin"), f32)
    rig = Rig(gpu, 1, settings=lambda ch: dict(sample_rate=1000, grow=100.0, fall=120.0, threshold=0.1, lo=0.25, hi=4.0))
    assert _bits_equal(r[:h], rig.run(x[:, :h])[0]) and _bits_equal(r[n], rig.ref.gain[0])
    rig.set(0, "set_max_gain", 0.5)
    rig.set(0, "set_max_gain", 2.0)
    assert _bits_equal(r[n + 1], rig.ref.gain[0]) and r[n + 1] == 0.5
    assert _bits_equal(r[h:n], rig.run(x[:, h:])[0]) and _bits_equal(r[n + 2], rig.ref.gain[0])
    rig.close()
