"""mi_oversampler_bank (lsp::dspu::Oversampler) on the device against the float32 restatement tests/oversampler_ref.py.
Upsampling is compared by bit pattern (a sum starts from +0.0f in both, so the sign of a zero matches too); the filtered
downsample is compared with the oracle's biquad bank (exact mode) and with an independent mi_biquad_bank (default mode)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import oversampler_ref as oref
from oversampler_ref import OversamplerRef

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "lsp-dsp-units_amd")
MODES = list(range(1, 31))
pytestmark = pytest.mark.gpu


def _signal(seed, shape):
    return (np.random.default_rng(seed).standard_normal(shape) * 0.5).astype(np.float32)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _pair(gpu, channels, mode, sr=None, filtering=True):
    bank = gpu.OversamplerBank(channels)
    ref = OversamplerRef(channels, gpu.OversamplerBank.coefficients)
    for o in (bank, ref):
        o.set_mode(mode)
        if sr is not None:
            o.set_sample_rate(sr)
        o.set_filtering(filtering)
        o.update_settings()
    return bank, ref


def _call(gpu, fn, x, n_out, out_stride=None, in_stride=None, **kw):
    """fn(out, inp, count-related args by the caller) on padded rows; checks that nothing is written past the rows."""
    C, n_in = x.shape
    xs, os_ = in_stride or n_in, out_stride or n_out
    host = np.zeros((C, xs), np.float32)
    host[:, :n_in] = x
    din = gpu.DeviceBuffer.from_host(host)
    dout = gpu.DeviceBuffer((C, max(os_, 1)))
    dout.upload(np.full((C, max(os_, 1)), 7.0, np.float32))
    fn(dout, din, out_stride=os_, in_stride=xs, **kw)
    y = dout.download()
    assert np.all(y[:, n_out:] == 7.0), "written past the row"
    return y[:, :n_out]


def _up(gpu, bank, x, **kw):
    n, N = x.shape[1], bank.oversampling()
    return _call(gpu, lambda o, i, **k: bank.upsample(o, i, n, **k), x, N * n, **kw)


def _down(gpu, bank, y, **kw):
    N = bank.oversampling()
    n = y.shape[1] // N
    return _call(gpu, lambda o, i, **k: bank.downsample(o, i, n, **k), y, n, **kw)


def _proc(gpu, bank, x, callback=None, **kw):
    n = x.shape[1]
    return _call(gpu, lambda o, i, **k: bank.process(o, i, n, callback=callback, **k), x, n, **kw)


SHAPES = {"1024x4096": (1024, (4096, 100, 4096)), "2x65536": (2, (65536, 3, 65536)), "5x13": (5, (13, 1, 13, 300)),
          "short": (3, (1, 2, 3, 5, 1, 130, 2))}


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("mode", MODES)
def test_upsample_bit_exact_every_channel_across_calls(gpu, mode, shape):
    C, runs = SHAPES[shape]
    bank, ref = _pair(gpu, C, mode)
    for blk, n in enumerate(runs):
        x = _signal(100 * mode + blk, (C, n))
        y = _up(gpu, bank, x)
        want = ref.upsample(x)
        bad = np.count_nonzero(_bits(y) != _bits(want))
        assert bad == 0, (mode, shape, blk, n, bad)
    bank.close()


@pytest.mark.parametrize("mode", [oref.MODES["4X16BIT"], oref.MODES["3X2"], oref.MODES["8X24BIT"], oref.MODES["6X3"]])
def test_runs_of_calls_equal_one_long_call(gpu, mode):
    C = 64
    runs = (1, 7, 19, 20, 21, 0, 123, 124, 125, 4095, 4097)
    x = _signal(7, (C, sum(runs)))
    one, ref = _pair(gpu, C, mode)
    whole = _up(gpu, one, x)
    assert np.array_equal(_bits(whole), _bits(ref.upsample(x)))
    parts, _ = _pair(gpu, C, mode)
    N, pos, got = one.oversampling(), 0, []
    for r in runs:
        got.append(_up(gpu, parts, np.ascontiguousarray(x[:, pos:pos + r])) if r else np.zeros((C, 0), np.float32))
        if r == 0:                                          # count 0: nothing is touched, NULL buffers are fine
            gpu.check(gpu.lib.mi_oversampler_bank_upsample(parts.handle, None, None, 0, 0, 0, None))
            gpu.check(gpu.lib.mi_oversampler_bank_downsample(parts.handle, None, None, 0, 0, 0, None))
            gpu.check(gpu.lib.mi_oversampler_bank_process(parts.handle, None, None, 0, 0, 0, None, None, None))
        pos += r
    assert np.array_equal(_bits(np.concatenate(got, axis=1)), _bits(whole))
    assert whole.shape[1] == N * sum(runs)
    one.close()
    parts.close()


@pytest.mark.parametrize("mode", [oref.MODES["6X16BIT"], oref.MODES["3X3"], oref.MODES["2X24BIT"]])
def test_strides_and_unaligned_rows(gpu, mode):
    C, n = 33, 1000
    bank, ref = _pair(gpu, C, mode, filtering=False)
    twin, _ = _pair(gpu, C, mode, filtering=False)
    N = bank.oversampling()
    for blk, (os_, is_) in enumerate([(N * n + 37, 1013), (N * n + 1, 1003), (N * n, 1000)]):
        x = _signal(30 + blk, (C, n))
        y = _up(gpu, bank, x, out_stride=os_, in_stride=is_)
        assert np.array_equal(_bits(y), _bits(ref.upsample(x))), blk
        # the decimation from unaligned oversampled rows into unaligned rows, and process() on unaligned rows
        z = _down(gpu, bank, y, out_stride=is_, in_stride=os_)
        assert np.array_equal(_bits(z), _bits(y[:, ::N])), blk
        assert np.array_equal(_bits(_proc(gpu, twin, x, out_stride=is_ + 2, in_stride=is_)), _bits(z)), blk
    bank.close()
    twin.close()


@pytest.mark.parametrize("mode", MODES)
def test_upsample_then_downsample_without_filter_is_a_pure_delay(gpu, mode):
    C, n = 7, 3000
    bank, _ = _pair(gpu, C, mode, filtering=False)
    a = bank.latency()
    assert bank.max_latency() == 62 and a == oref.latency(mode)
    prev = np.zeros((C, a), np.float32)
    for blk in range(2):
        x = _signal(200 + blk, (C, n))
        out = _down(gpu, bank, _up(gpu, bank, x))
        ext = np.concatenate([prev, x], axis=1)
        assert np.array_equal(_bits(out), _bits(ext[:, :n])), (mode, blk)        # out[i] == x[i - a]
        prev = ext[:, -a:]
    bank.close()


@pytest.mark.parametrize("times", [2, 3, 4, 6, 8])
def test_16bit_upsample_is_what_the_true_peak_meter_compares(gpu, times):
    C, n = 16, 5000
    mode = oref.MODES["%dX16BIT" % times]
    rate = {2: 96000, 3: 64000, 4: 48000, 6: 32000, 8: 22050}[times]
    bank, _ = _pair(gpu, C, mode)
    meter = gpu.TruePeakBank(C)
    meter.set_sample_rate(rate)
    for blk in range(2):
        x = _signal(300 + blk, (C, n))
        y = _up(gpu, bank, x)
        din, dout = gpu.DeviceBuffer.from_host(x), gpu.DeviceBuffer((C, n))
        meter.process(dout, din, n)
        assert meter.oversampling() == times
        assert np.array_equal(_bits(np.abs(y).reshape(C, n, times).max(axis=2)), _bits(dout.download())), (times, blk)
    bank.close()
    meter.close()


@pytest.mark.parametrize("sr", [44100, 48000, 96000])
@pytest.mark.parametrize("times", [2, 3, 4, 6, 8])
def test_downsample_filtered_exact_mode_equals_the_oracle(gpu, times, sr):
    C, runs = 6, (1500, 7, 2048)
    mode = oref.MODES["%dX3" % times]
    bank, ref = _pair(gpu, C, mode, sr=sr)
    bank.set_exact(True)
    fp, rate = bank.get_filter()
    want = oref.filter_params(sr)
    assert (fp["nType"], fp["nSlope"]) == (29, 30) and rate == sr * times
    assert np.float32(fp["fFreq"]) == want[2] and np.float32(fp["fFreq2"]) == want[3]
    assert np.float32(fp["fGain"]) == np.float32(1.0) and np.float32(fp["fQuality"]) == np.float32(0.1)
    assert np.float32(fp["fFreq"]) == (np.float32(20000.0) if sr >= 48000 else np.float32(np.float32(sr) * np.float32(0.42)))
    assert len(ref.sections) > 0
    for blk, n in enumerate(runs):
        y = _signal(400 + blk, (C, times * n))
        got = _down(gpu, bank, y)
        assert np.array_equal(_bits(got), _bits(ref.downsample(y))), (times, sr, blk)
    bank.close()


@pytest.mark.parametrize("sr", [44100, 48000, 96000])
@pytest.mark.parametrize("times", [2, 3, 4, 6, 8])
def test_downsample_filtered_default_mode_equals_an_independent_biquad_bank(gpu, times, sr):
    C, runs = 6, (1500, 7, 2048)
    mode = oref.MODES["%dX16BIT" % times]
    bank, ref = _pair(gpu, C, mode, sr=sr)
    S = len(ref.sections)
    _, _, sec = gpu.design_filter(29, 30, ref.params[2], ref.params[3], 1.0, 0.1, sample_rate=sr * times)
    assert np.array_equal(_bits(sec), _bits(ref.sections)) and S > 0
    twin = gpu.BiquadBank(C, S)
    twin.set_all_chains(np.broadcast_to(sec, (C, S, 5)))
    for blk, n in enumerate(runs):
        y = _signal(500 + blk, (C, times * n))
        got = _down(gpu, bank, y)
        din, dout = gpu.DeviceBuffer.from_host(y), gpu.DeviceBuffer((C, times * n))
        twin.process(dout, din, times * n)
        assert np.array_equal(_bits(got), _bits(dout.download()[:, ::times])), (times, sr, blk)
    bank.close()
    twin.close()


def test_a_bank_whose_rate_was_never_set_filters_with_none(gpu):
    bank, ref = _pair(gpu, 3, oref.MODES["4X4"])
    fp, rate = bank.get_filter()
    assert fp["nType"] == 0 and rate == 0 and bank.filtering()
    y = _signal(9, (3, 4 * 500))
    assert np.array_equal(_bits(_down(gpu, bank, y)), _bits(y[:, ::4]))
    assert np.array_equal(_bits(ref.downsample(y)), _bits(y[:, ::4]))
    bank.close()


def _scale_callback(gpu, channels, factor):
    """A device callback without another runtime: a one-section biquad bank y = factor * x in the exact mode (one rounded
    product per sample), enqueued in place on the stream it is given."""
    scaler = gpu.BiquadBank(channels, 1)
    scaler.set_exact(True)
    scaler.set_all_chains(np.broadcast_to(np.array([factor, 0, 0, 0, 0], np.float32), (channels, 1, 5)))

    def cb(buf, samples, stride, ch, stream):
        assert ch == channels
        scaler.process(buf, buf, samples, out_stride=stride, in_stride=stride, stream=stream or None)
    cb.bank = scaler
    return cb


@pytest.mark.parametrize("what", ["null", "scale"])
@pytest.mark.parametrize("mode", [oref.MODES["4X16BIT"], oref.MODES["3X2"], oref.MODES["8X24BIT"], 0])
def test_process_equals_upsample_callback_downsample(gpu, mode, what):
    C, runs = 12, (2000, 33, 2049)
    sr = 48000
    one, ref = _pair(gpu, C, mode, sr=sr)
    parts, _ = _pair(gpu, C, mode, sr=sr)
    inplace, _ = _pair(gpu, C, mode, sr=sr)
    cb = {"null": None, "scale": _scale_callback(gpu, C, 0.75)}[what]
    N = one.oversampling()
    for blk, n in enumerate(runs):
        x = _signal(600 + blk, (C, n))
        got = _proc(gpu, one, x, callback=cb)
        # the same in three calls
        if mode == 0:
            mid = x.copy()
        else:
            mid = _up(gpu, parts, x)
        if cb is not None:
            buf = gpu.DeviceBuffer.from_host(mid)
            cb(buf.ptr, N * n, N * n, C, 0)
            mid = buf.download()
        want = _down(gpu, parts, mid) if mode else mid
        assert np.array_equal(_bits(got), _bits(want)), (mode, what, blk)
        # in place
        buf = gpu.DeviceBuffer.from_host(x)
        inplace.process(buf, buf, n, callback=cb)
        assert np.array_equal(_bits(buf.download()), _bits(got)), (mode, what, blk)
    for b in (one, parts, inplace):
        b.close()


TORCH_CHILD = r'''
import importlib, sys
import numpy as np
import torch                                    # torch first: one HIP runtime per process
sys.path.insert(0, %r)
gpu = importlib.import_module("lsp-dsp-units_amd")
C, mode, runs = 12, gpu.OversamplerBank.MODES["4X16BIT"], (2000, 33, 2049)


def view(ptr, channels, stride):
    class Mem:
        pass
    m = Mem()
    m.__cuda_array_interface__ = {"shape": (channels, stride), "typestr": "<f4", "data": (int(ptr), False), "version": 2}
    return torch.as_tensor(m, device="cuda")


def tanh(buf, samples, stride, channels, stream):
    t = view(buf, channels, stride)[:, :samples]
    with torch.cuda.stream(torch.cuda.ExternalStream(stream) if stream else torch.cuda.default_stream()):
        torch.tanh(t, out=t)


def bank():
    b = gpu.OversamplerBank(C)
    b.set_mode(mode)
    b.set_sample_rate(48000)
    b.update_settings()
    return b


one, parts, inplace = bank(), bank(), bank()
rng = np.random.default_rng(5)
for n in runs:
    x = (rng.standard_normal((C, n)) * 2.0).astype(np.float32)
    din, dout = gpu.DeviceBuffer.from_host(x), gpu.DeviceBuffer((C, n))
    one.process(dout, din, n, callback=tanh)
    got = dout.download()
    mid = gpu.DeviceBuffer((C, 4 * n))
    parts.upsample(mid, din, n)
    tanh(mid.ptr, 4 * n, 4 * n, C, None)
    torch.cuda.synchronize()
    up = mid.download()
    assert 0.9 < np.abs(up).max() <= 1.0, "tanh did not run on the oversampled rows"
    parts.downsample(dout, mid, n)
    assert np.array_equal(dout.download().view(np.uint32), got.view(np.uint32)), n
    inplace.process(din, din, n, callback=tanh)
    assert np.array_equal(din.download().view(np.uint32), got.view(np.uint32)), n
print("TANH OK")
'''


def test_process_with_a_torch_op_on_the_stream(gpu):
    """A callback that launches a tanh on the oversampled rows with torch.  A child process: torch has to be imported
    before the library so that the two share one HIP runtime (bench.py does the same)."""
    import sys
    r = subprocess.run([sys.executable, "-c", TORCH_CHILD % ROOT], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "TANH OK" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])


def test_process_in_the_exact_mode_equals_the_restatement(gpu):
    C, mode = 5, oref.MODES["4X16BIT"]
    bank, ref = _pair(gpu, C, mode, sr=48000)
    bank.set_exact(True)
    for blk, n in enumerate((1000, 3, 2500)):
        x = _signal(650 + blk, (C, n))
        got = _proc(gpu, bank, x, callback=_scale_callback(gpu, C, 0.5))
        assert np.array_equal(_bits(got), _bits(ref.process(x, lambda y: y * np.float32(0.5)))), blk
    bank.close()


def test_a_failing_callback_fails_the_call(gpu):
    bank, _ = _pair(gpu, 2, oref.MODES["2X2"])
    x = gpu.DeviceBuffer.from_host(_signal(1, (2, 64)))
    with pytest.raises(gpu.MiError) as e:
        bank.process(x, x, 64, callback=lambda *a: -1)
    assert e.value.code == -1
    bank.close()


def test_settings_clear_both_states_at_update_and_not_before(gpu):
    C, n = 4, 600
    m4, m12 = oref.MODES["4X4"], oref.MODES["4X12BIT"]
    bank, ref = _pair(gpu, C, m4, sr=48000)
    assert not bank.modified() and bank.mode() == m4 and bank.filtering() and bank.oversampling() == 4 and bank.latency() == 4
    # an unchanged set_* leaves modified() false
    bank.set_mode(m4)
    bank.set_sample_rate(48000)
    bank.set_filtering(True)
    assert not bank.modified()
    x0, x1, x2 = _signal(700, (C, n)), _signal(701, (C, n)), _signal(702, (C, n))
    assert np.array_equal(_bits(_proc(gpu, bank, x0)), _bits(_proc(gpu, _fresh(gpu, C, m4), x0)))
    ref.upsample(x0)

    # a mode change (same kernel, so the bits can be compared): nothing is cleared before update_settings()
    bank.set_mode(m12)
    ref.set_mode(m12)
    assert bank.modified() and bank.mode() == m12
    y1 = _up(gpu, bank, x1)
    assert np.array_equal(_bits(y1), _bits(ref.upsample(x1)))
    assert not np.array_equal(_bits(y1), _bits(_up(gpu, _fresh(gpu, C, m12), x1))), "the upsample state was dropped early"
    f1 = _down(gpu, bank, y1)
    assert not np.array_equal(_bits(f1), _bits(_down(gpu, _fresh(gpu, C, m12), y1))), "the filter state was dropped early"
    bank.update_settings()
    assert not bank.modified()
    assert np.array_equal(_bits(_proc(gpu, bank, x2)), _bits(_proc(gpu, _fresh(gpu, C, m12), x2))), "update_settings() did not clear"

    # a filtering change and a rate change do the same
    changes = (lambda b: b.set_filtering(False), lambda b: b.set_sample_rate(44100))
    for k, change in enumerate(changes):
        _proc(gpu, bank, x0)
        change(bank)
        assert bank.modified()
        y = _up(gpu, bank, x1)
        assert not np.array_equal(_bits(y), _bits(_up(gpu, _fresh(gpu, C, m12), x1)))
        bank.update_settings()
        assert not bank.modified()
        twin = _fresh(gpu, C, m12)                              # a fresh bank with the settings the bank has by now
        for done in changes[:k + 1]:
            done(twin)
        twin.update_settings()
        assert np.array_equal(_bits(_proc(gpu, bank, x2)), _bits(_proc(gpu, twin, x2)))
        twin.close()
    fp, rate = bank.get_filter()
    assert rate == 4 * 44100 and not bank.filtering()
    bank.close()


def _fresh(gpu, C, mode, sr=48000):
    b = gpu.OversamplerBank(C)
    b.set_mode(mode)
    b.set_sample_rate(sr)
    b.update_settings()
    return b


def test_om_none_copies(gpu):
    C, n = 5, 777
    bank = gpu.OversamplerBank(C)
    assert bank.mode() == 0 and bank.modified() and bank.oversampling() == 1 and bank.latency() == 0
    bank.set_sample_rate(48000)
    bank.update_settings()
    x = _signal(800, (C, n))
    for fn in (_up, _down, _proc):
        assert np.array_equal(_bits(fn(gpu, bank, x, out_stride=n + 3, in_stride=n + 1)), _bits(x))
    got = _proc(gpu, bank, x, callback=_scale_callback(gpu, C, 2.0))
    assert np.array_equal(_bits(got), _bits(x * np.float32(2.0)))
    bank.close()


CPP = r'''
#include <lsp-plug.in/dsp-units/util/Oversampler.h>
#include <cstdio>
#include <string>
#include <vector>
using namespace lsp::dspu;

struct halve: public IOversamplerCallback
{
    size_t calls = 0, seen = 0;
    void process(float *out, const float *in, size_t samples) override
    {
        ++calls; seen += samples;
        for (size_t i = 0; i < samples; ++i) out[i] = in[i] * 0.5f;
    }
};

struct names: public IStateDumper
{
    std::vector<std::string> seen;
    int depth = 0;
    void begin_object(const char *n, const void *, size_t) override { if (depth++ == 0) seen.push_back(n); }
    void begin_object(const void *, size_t) override           { ++depth; }
    void end_object() override                                  { --depth; }
    void write(const char *n, const void *) override           { if (!depth) seen.push_back(n); }
    void write(const char *n, bool) override                   { if (!depth) seen.push_back(n); }
    void write(const char *n, size_t) override                 { if (!depth) seen.push_back(n); }
};

static void halve_fn(float *out, const float *in, size_t n, void *arg) { for (size_t i = 0; i < n; ++i) out[i] = in[i] * *(float *)arg; }

int main(int argc, char **argv)
{
    FILE *f = fopen(argv[1], "rb");
    std::vector<float> x(4 * 1500), y(x.size()), up(4 * 1500);
    if (fread(x.data(), sizeof(float), x.size(), f) != x.size()) return 2;
    fclose(f);
    Oversampler o;
    if (!o.init()) return 3;
    o.set_mode(OM_LANCZOS_4X16BIT);
    o.set_sample_rate(48000);
    if (!o.modified()) return 4;
    o.update_settings();
    if (o.modified()) return 5;
    halve h;
    o.process(y.data(), x.data(), 1500, &h);
    o.set_callback(&h);
    o.process(y.data() + 1500, x.data() + 1500, 1500);
    float g = 0.5f;
    o.process(y.data() + 3000, x.data() + 3000, 1500, halve_fn, &g);
    o.process(y.data() + 4500, x.data() + 4500, 1500, static_cast<IOversamplerCallback *>(NULL));
    o.upsample(up.data(), x.data(), 1500);
    f = fopen(argv[2], "wb");
    fwrite(y.data(), sizeof(float), y.size(), f);
    fwrite(up.data(), sizeof(float), up.size(), f);
    fclose(f);
    printf("latency %zu %zu times %zu calls %zu %zu\n", o.latency(), o.max_latency(), o.get_oversampling(), h.calls, h.seen);
    names n;
    o.dump(&n);
    printf("dump");
    for (const std::string &s: n.seen) printf(" %s", s.c_str());
    printf("\n");
    o.destroy();
    return 0;
}
'''


def test_cpp_class_on_the_device(gpu, tmp_path):
    src, exe = str(tmp_path / "os.cpp"), str(tmp_path / "os")
    open(src, "w").write(CPP)
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-I" + os.path.join(PKG, "include"), "-I" + os.path.join(ROOT, "include"), src,
                           "-o", exe, "-L" + PKG, "-lmi_dspu", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    x = _signal(60, (1, 6000))
    x.tofile(str(tmp_path / "in.bin"))
    env = dict(os.environ, MI_DSPU_EXACT_IIR="1")              # the anti-alias filter in the oracle's bits
    out = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=120, env=env)
    assert out.returncode == 0, out
    assert "latency 10 62 times 4 calls 2 12000" in out.stdout, out.stdout
    assert out.stdout.splitlines()[1].split()[1:] == ["pCallback", "fUpBuffer", "fDownBuffer", "pFunc", "nUpHead", "nMode", "nSampleRate",
                                                      "nUpdate", "sFilter", "bData", "bFilter"]
    r = np.fromfile(str(tmp_path / "out.bin"), np.float32)
    ref = OversamplerRef(1, gpu.OversamplerBank.coefficients)
    ref.set_mode(oref.MODES["4X16BIT"])
    ref.set_sample_rate(48000)
    ref.update_settings()
    half = lambda y: y * np.float32(0.5)
    want = [ref.process(x[:, i * 1500:(i + 1) * 1500], cb) for i, cb in enumerate((half, half, half, None))]
    assert np.array_equal(_bits(r[:6000]), _bits(np.concatenate(want, axis=1)[0]))
    assert np.array_equal(_bits(r[6000:]), _bits(ref.upsample(x[:, :1500])[0]))


def test_graph_capture_replays_direct_calls(gpu):
    C, n = 256, 4096
    mode = oref.MODES["4X16BIT"]
    st = ctypes.c_void_p()
    gpu.check(gpu.lib.mi_dspu_stream_create(ctypes.byref(st)))
    bank, _ = _pair(gpu, C, mode, sr=48000)
    twin, _ = _pair(gpu, C, mode, sr=48000)
    x = _signal(70, (C, n))
    din = gpu.DeviceBuffer.from_host(x)
    dout = gpu.DeviceBuffer((C, n))

    # a scratch growth and a changing update are refused during capture, and leave the bank usable
    gpu.check(gpu.lib.mi_dspu_graph_begin_capture(st))
    with pytest.raises(gpu.MiError) as e:
        bank.process(dout, din, n, stream=st.value)
    assert e.value.code == -5
    bank.set_filtering(False)
    with pytest.raises(gpu.MiError) as e:
        bank.update_settings(stream=st.value)
    assert e.value.code == -5
    gpu.check(gpu.lib.mi_dspu_memset(ctypes.c_void_p(dout.ptr), 0, 16, st))        # (so that the capture is not empty)
    exe = ctypes.c_void_p()
    gpu.check(gpu.lib.mi_dspu_graph_end_capture(st, ctypes.byref(exe)))
    gpu.lib.mi_dspu_graph_destroy(exe)
    bank.set_filtering(True)
    bank.update_settings(stream=st.value)
    bank.reserve(n)

    gpu.check(gpu.lib.mi_dspu_graph_begin_capture(st))
    bank.update_settings(stream=st.value)                       # nothing pending: allowed
    bank.process(dout, din, n, stream=st.value)
    exe = ctypes.c_void_p()
    gpu.check(gpu.lib.mi_dspu_graph_end_capture(st, ctypes.byref(exe)))
    tout = gpu.DeviceBuffer((C, n))
    for rep in range(3):
        gpu.check(gpu.lib.mi_dspu_graph_launch(exe, st))
        twin.process(tout, din, n, stream=st.value)
        assert np.array_equal(_bits(dout.download(stream=st.value)), _bits(tout.download(stream=st.value))), rep
    gpu.lib.mi_dspu_graph_destroy(exe)
    bank.close()
    twin.close()
    gpu.check(gpu.lib.mi_dspu_stream_destroy(st))
