"""mi_compressor_bank (lsp::dspu::Compressor) on the device against tests/compressor_ref.py: the envelope, the peak and the hold
counter bit for bit on every channel (the float32 restatement fed the library's own taus, release threshold and nHold), the
gain within the derived bound of the float64 curve on that envelope; across tiles, calls, in place, strides, process_apply,
changed settings, subnormals, the curve, the C++ class and graph capture."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import compressor_ref as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "lsp-dsp-units_amd")
T, G = 256, 4                           # tile_chain_device.h: samples of a tile, channels of a workgroup
f32 = np.float32


def _bank(gpu, C, settings=cr.channel_settings):
    bank = gpu.CompressorBank(C)
    for ch in range(C):
        bank.configure(ch, **settings(ch))
    bank.update_settings()
    return bank, [bank.get_params(ch) for ch in range(C)]


def _follow(x, state, params):
    return cr.follow(x, state, [p["tau_attack"] for p in params], [p["tau_release"] for p in params],
                     [p["release_threshold"] for p in params], [p["hold"] for p in params])


def _state(bank, C):
    s = [bank.get_state(ch) for ch in range(C)]
    return {"e": np.array([v[0] for v in s], f32), "peak": np.array([v[1] for v in s], f32), "hold": np.array([v[2] for v in s], np.uint32)}


def _same_state(a, b):
    return all(np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)) for k in ("e", "peak", "hold"))


def _run(gpu, bank, x, want_env=True):
    C, n = x.shape
    din = gpu.DeviceBuffer.from_host(x)
    dg, de = gpu.DeviceBuffer((C, n)), gpu.DeviceBuffer((C, n))
    de.upload(np.full((C, n), 7.0, f32))
    bank.process(dg, de if want_env else None, din, n)
    return dg.download(), de.download()


def _bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a, f32).view(np.uint32), np.ascontiguousarray(b, f32).view(np.uint32))


def _check_gain(gain, env, params, what, extra=0.0, scale=None):
    g64, bound = cr.gain64(env, params), cr.gain_bound(env, params) + extra
    if scale is not None:
        g64 = g64 * scale
    err = np.abs(gain.astype(np.float64) - g64) / np.abs(g64) / cr.U
    print("%s: gain error at most %.2f u, %.3f of its bound (bound: median %.1f u, max %.1f u)"
          % (what, err.max(), (err / bound).max(), np.median(bound), bound.max()))
    assert np.all(err <= bound), (what, err.max(), (err / bound).max())


SHAPES = [(C, n) for C in sorted({1, G + 1, 5}) for n in (1, 13, T, T + 1, 3 * T + 7)]


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_bit_exact_envelope_and_state_gain_within_bound(gpu, shape):
    C, n = shape
    bank, params = _bank(gpu, C)
    st = cr.fresh_state(C)
    total = dict.fromkeys(cr.BRANCHES, 0)
    for blk in range(2):
        x = cr.sidechain(20 * n + blk, C, n)
        gain, env = _run(gpu, bank, x)
        want, taken = _follow(x, st, params)
        for k in taken:
            total[k] += taken[k]
        assert _bits_equal(env, want), (shape, blk, np.count_nonzero(env.view(np.uint32) != want.view(np.uint32)))
        assert _same_state(_state(bank, C), st), (shape, blk)
        _check_gain(gain, want, params, "%s block %d" % (shape, blk))
    # a condition on the input (the seeds are chosen for it): every branch was taken, at every shape of a tile or more.  Two
    # calls of 1 or 13 samples from a zero state are too short to owe a hold countdown or a fall below the release threshold:
    # those shapes are here for the partial tile, and their bits are checked all the same.
    if n >= T:
        assert all(total[k] > 0 for k in cr.BRANCHES), total
    bank.close()


@pytest.mark.gpu
def test_full_size_every_channel(gpu):
    C, n = 1024, 4096
    bank, params = _bank(gpu, C)
    modes = [cr.channel_settings(ch) for ch in range(8)]
    assert {(s["mode"], s["boost_threshold"] >= 1.0) for s in modes} == {(0, False), (1, False), (2, True), (2, False)}
    x = cr.sidechain(77, C, n)
    st = cr.fresh_state(C)
    gain, env = _run(gpu, bank, x)
    want, taken = _follow(x, st, params)
    assert all(taken[k] > 0 for k in cr.BRANCHES), taken
    assert _bits_equal(env, want), np.count_nonzero(env.view(np.uint32) != want.view(np.uint32))
    assert _same_state(_state(bank, C), st)
    _check_gain(gain, want, params, "1024 x 4096")
    # every branch of the curve was reached somewhere: below both knees, inside a knee, above one
    x32 = np.abs(want)
    k0s, k0e = (np.array([p["k"][0][n_] for p in params], f32)[:, None] for n_ in ("start", "end"))
    assert np.any(x32 <= k0s) and np.any((x32 > k0s) & (x32 < k0e)) and np.any(x32 >= k0e)
    bank.close()


def _hold_settings(hold_ms):
    return lambda ch: dict(sample_rate=48000, mode=cr.CM_DOWNWARD, attack_threshold=0.1, release_threshold=0.01, boost_threshold=0.001,
                           attack=0.2, release=1.0 + ch, hold=hold_ms, knee=0.5, ratio=4.0)


@pytest.mark.gpu
@pytest.mark.parametrize("hold", [(0.0, 0), (0.03, 1), (6.26, 300)])
def test_hold_counts_across_tiles_and_calls(gpu, hold):
    ms, samples = hold
    C, n = 3, 300
    bank, params = _bank(gpu, C, _hold_settings(ms))
    assert [p["hold"] for p in params] == [samples] * C and samples in (0, 1, T + 44)
    x = np.full((C, 2 * n), 1e-3, f32)
    x[:, :200] = 1.0                        # the countdown starts at sample 200: over the tile's end at 256 and the call's at 300
    x[:, 550:560] = 1.0                     # a re-arm in the second call
    st = cr.fresh_state(C)
    for blk in range(2):
        part = np.ascontiguousarray(x[:, blk * n:(blk + 1) * n])
        gain, env = _run(gpu, bank, part)
        want, taken = _follow(part, st, params)
        assert _bits_equal(env, want), (hold, blk)
        got = _state(bank, C)
        assert _same_state(got, st), (hold, blk, got, st)
        if blk == 0:
            assert taken["hold"] == C * min(samples, 100)
            assert np.all(st["hold"] == max(samples - 100, 0))          # the counter crosses the call boundary
        _check_gain(gain, want, params, "hold %d block %d" % (samples, blk))
    bank.close()


@pytest.mark.gpu
def test_runs_of_calls_equal_one_long_call(gpu):
    C = G + 1
    runs = [1, 7, T - 1, T + 1, T + 90]
    x = cr.sidechain(5, C, sum(runs))
    one, params = _bank(gpu, C)
    whole_gain, whole_env = _run(gpu, one, x)
    parts, _ = _bank(gpu, C)
    st = cr.fresh_state(C)
    pos = 0
    for r in runs:
        part = np.ascontiguousarray(x[:, pos:pos + r])
        gain, env = _run(gpu, parts, part)
        want, _ = _follow(part, st, params)
        assert _bits_equal(env, whole_env[:, pos:pos + r]) and _bits_equal(env, want), (pos, r)
        assert _bits_equal(gain, whole_gain[:, pos:pos + r]), (pos, r)
        assert _same_state(_state(parts, C), st), (pos, r)
        pos += r
    assert _same_state(_state(one, C), st)
    one.close()
    parts.close()


@pytest.mark.gpu
def test_without_env_the_gain_is_the_same(gpu):
    C, n = G + 1, 3 * T + 7
    a, _ = _bank(gpu, C)
    b, _ = _bank(gpu, C)
    x = cr.sidechain(6, C, n)
    ga, _ = _run(gpu, a, x)
    gb, untouched = _run(gpu, b, x, want_env=False)
    assert _bits_equal(ga, gb) and np.all(untouched == 7.0)
    assert _same_state(_state(a, C), _state(b, C))
    a.close()
    b.close()


@pytest.mark.gpu
def test_in_place(gpu):
    C, n = G + 1, 3 * T + 7
    ref, _ = _bank(gpu, C)
    x = cr.sidechain(8, C, n)
    gain, env = _run(gpu, ref, x)
    a, _ = _bank(gpu, C)
    buf = gpu.DeviceBuffer.from_host(x)
    a.process(buf, None, buf, n)                                        # gain == in
    assert _bits_equal(buf.download(), gain)
    b, _ = _bank(gpu, C)
    buf, dg = gpu.DeviceBuffer.from_host(x), gpu.DeviceBuffer((C, n))
    b.process(dg, buf, buf, n)                                          # env == in, the gain apart
    assert _bits_equal(buf.download(), env) and _bits_equal(dg.download(), gain)
    c, _ = _bank(gpu, C)
    buf, de = gpu.DeviceBuffer.from_host(x), gpu.DeviceBuffer((C, n))
    c.process(buf, de, buf, n)                                          # gain == in, the envelope apart
    assert _bits_equal(buf.download(), gain) and _bits_equal(de.download(), env)
    for k in (ref, a, b, c):
        k.close()


@pytest.mark.gpu
@pytest.mark.parametrize("strides", [(301, 303, 307), (304, 312, 308), (300, 300, 300), (300, 303, 304)])
def test_strides_and_unaligned_rows(gpu, strides):
    C, n = G + 1, T + 44
    gs, es, xs = strides
    bank, params = _bank(gpu, C)
    x = cr.sidechain(9, C, n)
    host = np.full((C, xs), 3.0, f32)
    host[:, :n] = x
    din = gpu.DeviceBuffer.from_host(host)
    dg, de = gpu.DeviceBuffer((C, gs)), gpu.DeviceBuffer((C, es))
    dg.upload(np.full((C, gs), 7.0, f32))
    de.upload(np.full((C, es), 9.0, f32))
    bank.process(dg, de, din, n, gain_stride=gs, env_stride=es, in_stride=xs)
    gain, env = dg.download(), de.download()
    assert np.all(gain[:, n:] == 7.0) and np.all(env[:, n:] == 9.0), "written past count"
    assert np.array_equal(din.download(), host), "the input was written"
    want, _ = _follow(x, cr.fresh_state(C), params)
    assert _bits_equal(env[:, :n], want)
    twin, _ = _bank(gpu, C)
    tg, _ = _run(gpu, twin, x)
    assert _bits_equal(gain[:, :n], tg)
    bank.close()
    twin.close()


@pytest.mark.gpu
def test_process_apply_is_process_and_a_multiply(gpu):
    C, n = G + 1, 3 * T + 7
    a, _ = _bank(gpu, C)
    x = cr.sidechain(11, C, n)
    audio = (np.random.default_rng(12).standard_normal((C, n)) * 0.5).astype(f32)
    gain, _ = _run(gpu, a, x)
    want = audio * gain                                                 # one float32 multiply
    b, _ = _bank(gpu, C)
    dx, da, dd = gpu.DeviceBuffer.from_host(x), gpu.DeviceBuffer.from_host(audio), gpu.DeviceBuffer((C, n))
    b.process_apply(dd, da, dx, n)
    assert _bits_equal(dd.download(), want)
    assert _same_state(_state(a, C), _state(b, C))
    c, _ = _bank(gpu, C)
    c.process_apply(da, da, dx, n)                                      # dst == audio
    assert _bits_equal(da.download(), want)
    d, _ = _bank(gpu, C)
    da = gpu.DeviceBuffer.from_host(audio)
    d.process_apply(dx, da, dx, n)                                      # dst == sc
    assert _bits_equal(dx.download(), want)
    # rows that are not 16-byte aligned
    e, _ = _bank(gpu, C)
    pad = lambda v, s: np.concatenate([v, np.full((C, s - n), 5.0, f32)], axis=1)
    dx, da, dd = gpu.DeviceBuffer.from_host(pad(x, n + 1)), gpu.DeviceBuffer.from_host(pad(audio, n + 3)), gpu.DeviceBuffer((C, n + 2))
    dd.upload(np.full((C, n + 2), 7.0, f32))
    e.process_apply(dd, da, dx, n, out_stride=n + 2, audio_stride=n + 3, sc_stride=n + 1)
    got = dd.download()
    assert _bits_equal(got[:, :n], want) and np.all(got[:, n:] == 7.0)
    for k in (a, b, c, d, e):
        k.close()


@pytest.mark.gpu
def test_settings_changed_between_calls_and_clear(gpu):
    C, n = G + 1, T + 9
    bank, params = _bank(gpu, C)
    st = cr.fresh_state(C)
    x0, x1, x2 = (cr.sidechain(20 + i, C, n) for i in range(3))
    _, env = _run(gpu, bank, x0)
    assert _bits_equal(env, _follow(x0, st, params)[0])
    bank.set_ratio(0, 2.5)
    bank.set_mode(1, cr.CM_BOOSTING)
    bank.set_timings(3, 0.7, 3.3)
    bank.set_hold(3, 1.0)
    gain, env = _run(gpu, bank, x1)                                     # process() runs update_settings() first
    new = [bank.get_params(ch) for ch in range(C)]
    assert cr.flatten(new[2]) == cr.flatten(params[2]) and new[2]["hold"] == params[2]["hold"]      # an untouched channel
    assert new[0]["k"][0]["tilt"][0] != params[0]["k"][0]["tilt"][0] and new[3]["tau_attack"] != params[3]["tau_attack"]
    assert new[1]["k"][1]["gain"] != params[1]["k"][1]["gain"]
    assert new[3]["hold"] == cr.hold_samples(cr.channel_settings(3)["sample_rate"], 1.0) > 0
    want, _ = _follow(x1, st, new)                                      # the state carried over, the new parameters apply
    assert _bits_equal(env, want)
    assert _same_state(_state(bank, C), st)
    _check_gain(gain, want, new, "changed settings")
    bank.clear()
    z = _state(bank, C)
    assert not z["e"].any() and not z["peak"].any() and not z["hold"].any()
    gain, env = _run(gpu, bank, x2)
    assert _bits_equal(env, _follow(x2, cr.fresh_state(C), new)[0])
    bank.close()


@pytest.mark.gpu
def test_decay_into_subnormals(gpu):
    C, n = 2, 420
    settings = lambda ch: dict(sample_rate=48000, mode=cr.CM_DOWNWARD, attack_threshold=0.1, release_threshold=0.0, boost_threshold=0.001,
                               attack=0.05, release=0.05 + 0.01 * ch, hold=0.0, knee=0.5, ratio=4.0)
    bank, params = _bank(gpu, C, settings)
    x = np.zeros((C, n), f32)
    x[:, :20] = 1.0
    x[1] *= -1.0                                                        # a negative envelope as well
    st = cr.fresh_state(C)
    want, _ = _follow(x, st, params)
    tiny = f32(1.1754944e-38)
    sub = (np.abs(want) > 0) & (np.abs(want) < tiny)
    assert sub[0].sum() > 20 and np.flatnonzero(sub[0])[0] < 400, "the restatement's envelope does not reach the subnormals"
    gain, env = _run(gpu, bank, x)
    assert _bits_equal(env, want), np.flatnonzero(env.view(np.uint32)[0] != want.view(np.uint32)[0])[:4]
    assert _same_state(_state(bank, C), st)
    _check_gain(gain, want, params, "subnormal decay")
    bank.close()


@pytest.mark.gpu
def test_curve_over_a_level_ladder(gpu):
    C = 8
    bank, params = _bank(gpu, C)
    db = np.linspace(-96.0, 12.0, 2 * T + 29)
    x = np.tile((10.0 ** (db / 20.0)).astype(f32), (C, 1))
    x[:, ::5] *= -1.0
    din, dout = gpu.DeviceBuffer.from_host(x), gpu.DeviceBuffer((C, x.shape[1] + 3))
    dout.upload(np.full((C, x.shape[1] + 3), 7.0, f32))
    bank.curve(dout, din, x.shape[1], out_stride=x.shape[1] + 3)
    got = dout.download()
    assert np.all(got[:, x.shape[1]:] == 7.0)
    _check_gain(got[:, :x.shape[1]], x, params, "curve", extra=1.0, scale=np.abs(x).astype(np.float64))    # one more multiply
    bank.curve(din, din, x.shape[1])                                    # in place
    assert _bits_equal(din.download(), got[:, :x.shape[1]])
    bank.close()


CPP = r'''
#include <lsp-plug.in/dsp-units/dynamics/Compressor.h>
#include <cstdio>
#include <vector>
int main(int argc, char **argv)
{
    const size_t n = 700;
    FILE *f = fopen(argv[1], "rb");
    std::vector<float> x(2 * n + 8), out(8 * n + 16);            // gain and env of 2n + 8 each, four curves of n
    if (fread(x.data(), sizeof(float), x.size(), f) != x.size()) return 2;
    fclose(f);
    lsp::dspu::Compressor c;
    c.set_sample_rate(48000);
    c.set_mode(lsp::dspu::CM_UPWARD);
    c.set_threshold(0.2f, 0.05f);
    c.set_boost_threshold(0.004f);
    c.set_timings(0.5f, 4.0f);
    c.set_hold(0.5f);
    c.set_knee(0.6f);
    c.set_ratio(3.0f);
    float *gain = out.data(), *env = gain + 2 * n + 8, *cur = env + 2 * n + 8;
    c.process(gain, env, x.data(), n);                          // with the envelope
    c.process(gain + n, NULL, x.data() + n, n);                 // without it
    for (size_t i = 0; i < 8; ++i)                              // the scalar form: one sample each
        gain[2 * n + i] = c.process(env + 2 * n + i, x[2 * n + i]);
    c.curve(cur, x.data(), n);                                  // array forms ...
    c.reduction(cur + n, x.data(), n);
    for (size_t i = 0; i < n; ++i)                              // ... and scalar ones
    {
        cur[2 * n + i] = c.curve(x[i]);
        cur[3 * n + i] = c.reduction(x[i]);
    }
    f = fopen(argv[2], "wb");
    fwrite(out.data(), sizeof(float), out.size(), f);
    fclose(f);
    c.destroy();
    return 0;
}
'''


@pytest.mark.gpu
def test_cpp_class_on_the_device(gpu, tmp_path):
    src, exe = str(tmp_path / "comp.cpp"), str(tmp_path / "comp")
    open(src, "w").write(CPP)
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-I" + os.path.join(PKG, "include"), "-I" + os.path.join(ROOT, "include"), src,
                           "-o", exe, "-L" + PKG, "-lmi_dspu", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    n = 700
    x = cr.sidechain(60, 1, 2 * n + 8)
    x.tofile(str(tmp_path / "in.bin"))
    out = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out
    r = np.fromfile(str(tmp_path / "out.bin"), f32)
    m = 2 * n + 8
    gain, env, cur = r[:m][None, :], r[m:2 * m][None, :], r[2 * m:]
    s = dict(sample_rate=48000, mode=cr.CM_UPWARD, attack_threshold=0.2, release_threshold=0.05, boost_threshold=0.004,
             attack=0.5, release=4.0, hold=0.5, knee=0.6, ratio=3.0)
    params = [gpu.CompressorBank.compute_params(**s)]
    want, _ = _follow(x, cr.fresh_state(1), params)
    assert _bits_equal(env[:, :n], want[:, :n]) and _bits_equal(env[:, 2 * n:], want[:, 2 * n:])
    assert not env[0, n:2 * n].any()                            # no envelope was asked for in the second call
    _check_gain(gain, want, params, "class process")
    lv = x[:, :n]
    curve, red, curve1, red1 = (cur[i * n:(i + 1) * n][None, :] for i in range(4))
    scale = np.abs(lv).astype(np.float64)
    _check_gain(curve, lv, params, "class curve", extra=1.0, scale=scale)
    assert _bits_equal(red, curve)                              # the array reduction() is the curve, as in the reference
    _check_gain(curve1, lv, params, "class scalar curve", extra=1.0, scale=scale)
    _check_gain(red1, lv, params, "class scalar reduction")     # the scalar reduction() is the gain


CPP_WRITTEN_STATE = r'''
#include <lsp-plug.in/dsp-units/dynamics/Compressor.h>
#include <cstdio>
#include <vector>
struct Written: public lsp::dspu::Compressor                    // the follower's fields are protected: a subclass may write them
{
    void write(float e, float peak, uint32_t hold) { fEnvelope = e; fPeak = peak; nHoldCounter = hold; }
    void read(float *dst) const { dst[0] = fEnvelope; dst[1] = fPeak; dst[2] = float(nHoldCounter); }
};
int main(int argc, char **argv)
{
    const size_t n = 300;
    FILE *f = fopen(argv[1], "rb");
    std::vector<float> x(2 * n), out(4 * n + 3);
    if (fread(x.data(), sizeof(float), x.size(), f) != x.size()) return 2;
    fclose(f);
    Written c;
    c.set_sample_rate(48000);
    c.set_mode(lsp::dspu::CM_DOWNWARD);
    c.set_threshold(0.2f, 0.05f);
    c.set_timings(0.5f, 4.0f);
    c.set_hold(0.5f);
    c.set_knee(0.6f);
    c.set_ratio(3.0f);
    c.process(out.data(), out.data() + n, x.data(), n);
    c.write(1e-5f, 0.75f, 7);                                   // between two calls: the device has to take these
    c.process(out.data() + 2 * n, out.data() + 3 * n, x.data() + n, n);
    c.read(out.data() + 4 * n);
    f = fopen(argv[2], "wb");
    fwrite(out.data(), sizeof(float), out.size(), f);
    fclose(f);
    c.destroy();
    return 0;
}
'''


@pytest.mark.gpu
def test_cpp_class_sends_state_fields_a_subclass_wrote(gpu, tmp_path):
    src, exe = str(tmp_path / "written.cpp"), str(tmp_path / "written")
    open(src, "w").write(CPP_WRITTEN_STATE)
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-I" + os.path.join(PKG, "include"), "-I" + os.path.join(ROOT, "include"), src,
                           "-o", exe, "-L" + PKG, "-lmi_dspu", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    n = 300
    x = cr.sidechain(61, 1, 2 * n)
    x.tofile(str(tmp_path / "in.bin"))
    out = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out
    r = np.fromfile(str(tmp_path / "out.bin"), f32)
    s = dict(sample_rate=48000, mode=cr.CM_DOWNWARD, attack_threshold=0.2, release_threshold=0.05, boost_threshold=2.5119e-4,
             attack=0.5, release=4.0, hold=0.5, knee=0.6, ratio=3.0)
    params = [gpu.CompressorBank.compute_params(**s)]
    st = cr.fresh_state(1)
    assert _bits_equal(r[n:2 * n][None, :], _follow(x[:, :n], st, params)[0])
    st = {"e": np.array([1e-5], f32), "peak": np.array([0.75], f32), "hold": np.array([7], np.uint32)}
    want, taken = _follow(x[:, n:], st, params)
    # a condition on the input: the written counter is counted down, and under the written peak the envelope rises without
    # re-arming the hold, which calls alone never reach (they leave peak <= e)
    assert taken["hold"] >= 7 and taken["attack"] > taken["rearm"], taken
    assert _bits_equal(r[3 * n:4 * n][None, :], want)
    _check_gain(r[2 * n:3 * n][None, :], want, params, "class process after written state")
    assert _bits_equal(r[4 * n:4 * n + 2], [st["e"][0], st["peak"][0]]) and r[4 * n + 2] == float(st["hold"][0])


@pytest.mark.gpu
def test_graph_capture_replays_direct_calls(gpu):
    C, n = 64, T + 100
    st = ctypes.c_void_p()
    gpu.check(gpu.lib.mi_dspu_stream_create(ctypes.byref(st)))
    bank, params = _bank(gpu, C)
    twin, _ = _bank(gpu, C)
    x = cr.sidechain(70, C, 2 * n)
    d0, d1 = gpu.DeviceBuffer.from_host(x[:, :n]), gpu.DeviceBuffer.from_host(x[:, n:])
    g0, g1, e0, e1 = (gpu.DeviceBuffer((C, n)) for _ in range(4))
    gpu.check(gpu.lib.mi_dspu_graph_begin_capture(st))
    bank.process(g0, e0, d0, n, stream=st.value)
    bank.process(g1, e1, d1, n, stream=st.value)
    exe = ctypes.c_void_p()
    gpu.check(gpu.lib.mi_dspu_graph_end_capture(st, ctypes.byref(exe)))
    t = [gpu.DeviceBuffer((C, n)) for _ in range(4)]
    ref = cr.fresh_state(C)
    for rep in range(3):
        gpu.check(gpu.lib.mi_dspu_graph_launch(exe, st))
        twin.process(t[0], t[2], d0, n, stream=st.value)
        twin.process(t[1], t[3], d1, n, stream=st.value)
        got = [b.download(stream=st.value) for b in (g0, g1, e0, e1)]
        direct = [b.download(stream=st.value) for b in t]
        assert all(_bits_equal(a, b) for a, b in zip(got, direct)), rep
        want = np.concatenate([_follow(x[:, :n], ref, params)[0], _follow(x[:, n:], ref, params)[0]], axis=1)
        assert _bits_equal(np.concatenate(got[2:], axis=1), want), rep          # the state advances on every replay
    gpu.lib.mi_dspu_graph_destroy(exe)
    bank.close()
    twin.close()
    gpu.check(gpu.lib.mi_dspu_stream_destroy(st))


@pytest.mark.gpu
def test_changed_setting_inside_a_capture_is_refused(gpu):
    """A setter leaves an upload to the next call.  On a capturing stream that call -- process() or update_settings() -- answers
    MI_ESTATE and names update_settings(), changes nothing on the device and leaves the capture valid; the next eager process()
    applies the setting to the state from before the capture."""
    C, n = 5, T + 100
    st = ctypes.c_void_p()
    gpu.check(gpu.lib.mi_dspu_stream_create(ctypes.byref(st)))
    bank, params = _bank(gpu, C)
    state = cr.fresh_state(C)
    x0, x1 = cr.sidechain(80, C, n), cr.sidechain(81, C, n)
    d0, d1 = gpu.DeviceBuffer.from_host(x0), gpu.DeviceBuffer.from_host(x1)
    dg, de = gpu.DeviceBuffer((C, n)), gpu.DeviceBuffer((C, n))
    bank.process(dg, de, d0, n, stream=st.value)
    env0 = de.download(stream=st.value)
    assert _bits_equal(env0, _follow(x0, state, params)[0])
    before = _state(bank, C)
    gpu.check(gpu.lib.mi_dspu_graph_begin_capture(st))
    bank.set_ratio(0, 2.5)
    bank.set_timings(3, 0.7, 3.3)
    for call in (lambda: bank.process(dg, de, d1, n, stream=st.value), lambda: bank.update_settings(stream=st.value)):
        with pytest.raises(gpu.MiError) as e:
            call()
        assert e.value.code == -5 and "update_settings" in str(e.value)
    gpu.check(gpu.lib.mi_dspu_memset(ctypes.c_void_p(dg.ptr), 0, 16, st))          # (so that the capture is not empty)
    exe = ctypes.c_void_p()
    gpu.check(gpu.lib.mi_dspu_graph_end_capture(st, ctypes.byref(exe)))             # ends and instantiates normally
    assert exe.value
    gpu.lib.mi_dspu_graph_destroy(exe)
    # nothing changed on the device: the state, and the envelope rows no refused call wrote to
    assert _same_state(_state(bank, C), before) and _same_state(before, state)
    assert _bits_equal(de.download(stream=st.value), env0)
    bank.process(dg, de, d1, n, stream=st.value)
    new = [bank.get_params(ch) for ch in range(C)]
    assert new[0]["k"][0]["tilt"][0] != params[0]["k"][0]["tilt"][0] and new[3]["tau_attack"] != params[3]["tau_attack"]
    want, _ = _follow(x1, state, new)                                               # the state carried over, the new parameters apply
    assert _bits_equal(de.download(stream=st.value), want)
    assert _same_state(_state(bank, C), state)
    _check_gain(dg.download(stream=st.value), want, new, "after the refused capture")
    bank.close()
    gpu.check(gpu.lib.mi_dspu_stream_destroy(st))


@pytest.mark.gpu
def test_state_access_inside_a_capture_is_refused(gpu):
    """get_state() ends in a synchronisation, which a capturing stream does not allow: it answers MI_ESTATE with a message and
    leaves the capture valid -- a process() captured after it replays three times with the bits of an eager twin."""
    C, n = 5, T + 100
    st = ctypes.c_void_p()
    gpu.check(gpu.lib.mi_dspu_stream_create(ctypes.byref(st)))
    bank, params = _bank(gpu, C)
    twin, _ = _bank(gpu, C)
    x = cr.sidechain(82, C, n)
    d = gpu.DeviceBuffer.from_host(x)
    g, e, tg, te = (gpu.DeviceBuffer((C, n)) for _ in range(4))
    gpu.check(gpu.lib.mi_dspu_graph_begin_capture(st))
    with pytest.raises(gpu.MiError) as err:
        bank.get_state(2, stream=st.value)
    assert err.value.code == -5 and "captured" in str(err.value)
    bank.process(g, e, d, n, stream=st.value)
    exe = ctypes.c_void_p()
    gpu.check(gpu.lib.mi_dspu_graph_end_capture(st, ctypes.byref(exe)))
    ref = cr.fresh_state(C)
    for rep in range(3):
        gpu.check(gpu.lib.mi_dspu_graph_launch(exe, st))
        twin.process(tg, te, d, n, stream=st.value)
        got = [b.download(stream=st.value) for b in (g, e)]
        direct = [b.download(stream=st.value) for b in (tg, te)]
        assert all(_bits_equal(a, b) for a, b in zip(got, direct)), rep
        assert _bits_equal(got[1], _follow(x, ref, params)[0]), rep                # the state advances on every replay
    assert _same_state(_state(bank, C), ref)                                        # ... and can be read again after the capture
    gpu.lib.mi_dspu_graph_destroy(exe)
    bank.close()
    twin.close()
    gpu.check(gpu.lib.mi_dspu_stream_destroy(st))
