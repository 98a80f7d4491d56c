"""mi_gate_bank (lsp::dspu::Gate) on the device against tests/gate_ref.py: the envelope, the peak, the hold counter and the curve
index bit for bit on every channel (the float32 restatement fed the library's own parameters), the gain within the derived
bound of the float64 curve that the restatement's curve index selects -- open and close curves differ in threshold and zone,
so a sample given the wrong curve is far outside.  Bursts that toggle, crossings placed on the tile's and the call's edges,
the second step while the hold counts, across tiles, calls, in place, strides, process_apply, changed settings, the curves,
the C++ class and graph capture."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import gate_ref as gr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "lsp-dsp-units_amd")
T, G = 256, 4                           # tile_chain_device.h: samples of a tile, channels of a workgroup
f32 = np.float32
KEYS = ("e", "peak", "hold", "curve")


def _bank(gpu, C, settings=gr.channel_settings):
    bank = gpu.GateBank(C)
    for ch in range(C):
        bank.configure(ch, **settings(ch))
    bank.update_settings()
    return bank, [bank.get_params(ch) for ch in range(C)]


def _follow(x, state, params, stats=None):
    """(envelope, curve index of every sample); `stats` gathers toggles, capped, restep_hold, per_channel."""
    stats = gr.fresh_stats() if stats is None else stats
    out = gr.process(x, state, [p["tau_attack"] for p in params], [p["tau_release"] for p in params], [p["hold"] for p in params],
                     [p["k"][0]["end"] for p in params], [p["k"][1]["start"] for p in params], stats)
    assert stats["capped"] == 0, "the restatement reached its cap on a signal with sane settings"
    return out


def _state(bank, C):
    s = [bank.get_state(ch) for ch in range(C)]
    return {"e": np.array([v[0] for v in s], f32), "peak": np.array([v[1] for v in s], f32),
            "hold": np.array([v[2] for v in s], np.uint32), "curve": np.array([v[3] for v in s], np.uint32)}


def _same_state(a, b):
    return all(np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)) for k in KEYS)


def _run(gpu, bank, x, want_env=True):
    C, n = x.shape
    din = gpu.DeviceBuffer.from_host(x)
    dg, de = gpu.DeviceBuffer((C, n)), gpu.DeviceBuffer((C, n))
    de.upload(np.full((C, n), 7.0, f32))
    bank.process(dg, de if want_env else None, din, n)
    return dg.download(), de.download()


def _bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a, f32).view(np.uint32), np.ascontiguousarray(b, f32).view(np.uint32))


def _check_gain(gain, env, which, params, what, extra=0.0, scale=None):
    """Within the bound inside the zone of the curve `which` selects; gain_start / gain_end as stored outside it."""
    g64, bound = gr.gain64(env, which, params), gr.gain_bound(env, which, params)
    const = bound == 0
    bound = bound + extra
    if scale is not None:
        g64 = g64 * scale
    got = gain.astype(np.float64)
    if extra == 0:
        assert np.array_equal(got[const], g64[const]), (what, np.count_nonzero(got[const] != g64[const]))
    err = np.abs(got - g64) / np.abs(g64) / gr.U
    print("%s: gain error at most %.2f u, %.3f of its bound (%d of %d samples inside a zone; bound there: median %.1f u, max %.1f u)"
          % (what, err.max(), (err[~const] / bound[~const]).max() if np.any(~const) else 0.0, np.count_nonzero(~const), const.size,
             np.median(bound[~const]) if np.any(~const) else 0.0, bound.max()))
    assert np.all(err <= bound), (what, err.max(), np.count_nonzero(err > bound))


def _wrong_curve_is_far_outside(env, which, params):
    """A condition on the settings: on samples inside a zone, the other curve's gain is outside this curve's bound."""
    g, other, bound = gr.gain64(env, which, params), gr.gain64(env, 1 - which.astype(np.int64), params), gr.gain_bound(env, which, params)
    differ = np.abs(other - g) > 4 * np.maximum(bound, 1.0) * gr.U * g
    return np.count_nonzero(differ)


SHAPES = [(C, n) for C in sorted({1, G + 1, 5}) for n in (1, 13, T, T + 1, 3 * T + 7)]


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_bit_exact_envelope_state_and_curve_gain_within_bound(gpu, shape):
    C, n = shape
    bank, params = _bank(gpu, C)
    st, stats = gr.fresh_state(C), gr.fresh_stats()
    for blk in range(2):
        x = gr.bursts(20 * n + blk, C, n)
        gain, env = _run(gpu, bank, x)
        want, which = _follow(x, st, params, stats)
        assert _bits_equal(env, want), (shape, blk, np.count_nonzero(env.view(np.uint32) != want.view(np.uint32)))
        assert _same_state(_state(bank, C), st), (shape, blk)
        _check_gain(gain, want, which, params, "%s block %d" % (shape, blk))
    if n >= 3 * T:
        assert stats["per_channel"].min() >= 8, stats["per_channel"]
    bank.close()


@pytest.mark.gpu
def test_bursts_toggle_at_least_eight_times_per_channel(gpu):
    C, n = G + 1, 5 * T + 11
    bank, params = _bank(gpu, C)
    x = gr.bursts(3, C, n)
    st, stats = gr.fresh_state(C), gr.fresh_stats()
    want, which = _follow(x, st, params, stats)
    assert stats["per_channel"].min() >= 8, stats["per_channel"]                # a kernel that never switches cannot pass
    assert np.all(which.min(axis=1) == 0) and np.all(which.max(axis=1) == 1)
    assert _wrong_curve_is_far_outside(want, which, params) > 200
    gain, env = _run(gpu, bank, x)
    assert _bits_equal(env, want)
    assert _same_state(_state(bank, C), st)
    _check_gain(gain, want, which, params, "bursts")
    bank.close()


@pytest.mark.gpu
def test_full_size_every_channel(gpu):
    C, n = 1024, 4096
    bank, params = _bank(gpu, C)
    x = gr.bursts(77, C, n)
    st, stats = gr.fresh_state(C), gr.fresh_stats()
    gain, env = _run(gpu, bank, x)
    want, which = _follow(x, st, params, stats)
    assert stats["per_channel"].min() >= 8 and stats["restep_hold"] == 0
    assert _bits_equal(env, want), np.count_nonzero(env.view(np.uint32) != want.view(np.uint32))
    assert _same_state(_state(bank, C), st)
    _check_gain(gain, want, which, params, "1024 x 4096")
    bank.close()


def _edge_settings(ch):
    """Times of 0 give taus of 1: the envelope is the input, and it crosses where the input steps."""
    return dict(sample_rate=48000, open_threshold=0.1 + 0.01 * ch, close_threshold=0.05, open_zone=0.5, close_zone=0.5, reduction=0.1,
                attack=0.0, release=0.0, hold=0.0)


@pytest.mark.gpu
def test_crossings_on_the_edges_of_tiles_and_calls(gpu):
    C, n = G + 1, 2 * T + 9
    bank, params = _bank(gpu, C, _edge_settings)
    assert all(p["tau_attack"] == 1.0 and p["tau_release"] == 1.0 for p in params)
    flips = [0, T - 1, T, n - 1, n]                                             # n: the first sample of the following call
    level = np.zeros(2 * n, bool)
    for f in flips:
        level[f:] = ~level[f:]
    x = np.where(level, f32(0.5), f32(1e-3)).astype(f32)[None, :].repeat(C, axis=0)
    x[:, 40] = 0.03                                                             # inside the close zone, no crossing
    st, stats = gr.fresh_state(C), gr.fresh_stats()
    both = []
    for blk in range(2):
        part = np.ascontiguousarray(x[:, blk * n:(blk + 1) * n])
        gain, env = _run(gpu, bank, part)
        want, which = _follow(part, st, params, stats)
        both.append(which)
        assert _bits_equal(env, want), blk
        assert _same_state(_state(bank, C), st), (blk, _state(bank, C), st)
        _check_gain(gain, want, which, params, "edges block %d" % blk)
        if blk == 0:
            assert np.all(st["curve"] == 0)                                     # the crossing on the last sample was taken
    which = np.concatenate(both, axis=1)
    changes = np.flatnonzero(np.diff(np.concatenate([[0], which[0]])) != 0).tolist()
    assert changes == flips and stats["toggles"] == C * len(flips)
    bank.close()


def _hold_settings(hold_ms, open_threshold=0.5):
    return lambda ch: dict(sample_rate=48000, open_threshold=open_threshold, close_threshold=open_threshold / 2, open_zone=0.5,
                           close_zone=0.25, reduction=0.05, attack=0.2, release=1.0 + ch, hold=hold_ms)


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
    st = gr.fresh_state(C)
    for blk in range(2):
        part = np.ascontiguousarray(x[:, blk * n:(blk + 1) * n])
        gain, env = _run(gpu, bank, part)
        hold_before = st["hold"].copy()
        want, which = _follow(part, st, params)
        assert _bits_equal(env, want), (hold, blk)
        got = _state(bank, C)
        assert _same_state(got, st), (hold, blk, got, st)
        if blk == 0:
            assert np.all(hold_before == 0) and np.all(st["hold"] == max(samples - 100, 0))     # the counter crosses the call boundary
        _check_gain(gain, want, which, params, "hold %d block %d" % (samples, blk))
    bank.close()


@pytest.mark.gpu
def test_second_step_while_the_hold_counts(gpu):
    """Settings changed between calls put the envelope above the open curve's end while curve 0 is in force and the hold counts:
    the first falling sample is held, crosses, and is held a second time: the counter goes down by two on it."""
    C, n = G + 1, 40
    bank, params = _bank(gpu, C, _hold_settings(0.25))
    assert params[0]["hold"] == 12
    st = gr.fresh_state(C)
    x0 = np.full((C, n), 0.3, f32)
    _, env = _run(gpu, bank, x0)
    want, which = _follow(x0, st, params)
    assert _bits_equal(env, want) and np.all(st["curve"] == 0) and np.all(st["hold"] == 12) and np.all(st["e"] > 0.2)
    for ch in range(C):
        bank.set_threshold(ch, 0.1, 0.05)
    x1 = np.zeros((C, n), f32)
    gain, env = _run(gpu, bank, x1)
    new = [bank.get_params(ch) for ch in range(C)]
    stats = gr.fresh_stats()
    want, which = _follow(x1, st, new, stats)
    assert stats["restep_hold"] == C and stats["toggles"] >= C
    assert np.all(which[:, 0] == 1) and np.all(want[:, 10] == want[:, 0]) and np.all(want[:, 11] < want[:, 0])   # 12 - 2 = 10 more held
    assert _bits_equal(env, want)
    assert _same_state(_state(bank, C), st)
    _check_gain(gain, want, which, new, "second step with hold")
    bank.close()


@pytest.mark.gpu
def test_runs_of_calls_equal_one_long_call(gpu):
    C = G + 1
    runs = [1, 7, T - 1, T + 1, T + 90]
    x = gr.bursts(5, C, sum(runs))
    one, params = _bank(gpu, C)
    whole_gain, whole_env = _run(gpu, one, x)
    parts, _ = _bank(gpu, C)
    st = gr.fresh_state(C)
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
    x = gr.bursts(6, C, n)
    ga, _ = _run(gpu, a, x)
    gb, untouched = _run(gpu, b, x, want_env=False)
    assert _bits_equal(ga, gb) and np.all(untouched == 7.0)
    assert _same_state(_state(a, C), _state(b, C))
    a.close()
    b.close()


@pytest.mark.gpu
def test_in_place(gpu):
    """The second step takes the input sample, not what the first step wrote over it: in place gives the out-of-place bits."""
    C, n = G + 1, 3 * T + 7
    ref, params = _bank(gpu, C)
    x = gr.bursts(8, C, n)
    gain, env = _run(gpu, ref, x)
    stats = gr.fresh_stats()
    _follow(x, gr.fresh_state(C), params, stats)
    assert stats["per_channel"].min() >= 4
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
    x = gr.bursts(9, C, n)
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
    want, _ = _follow(x, gr.fresh_state(C), params)
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
    x = gr.bursts(11, C, n)
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
    e, _ = _bank(gpu, C)                                                # rows that are not 16-byte aligned
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
    st = gr.fresh_state(C)
    x0, x1, x2 = (gr.bursts(20 + i, C, n) for i in range(3))
    _, env = _run(gpu, bank, x0)
    assert _bits_equal(env, _follow(x0, st, params)[0])
    bank.set_reduction(0, 0.5)
    bank.set_zone(1, 0.3, 0.2)
    bank.set_timings(3, 0.3, 0.12)
    bank.set_hold(3, 0.2)
    gain, env = _run(gpu, bank, x1)                                     # the bank's process() applies pending settings first
    new = [bank.get_params(ch) for ch in range(C)]
    assert gr.flatten(new[2]) == gr.flatten(params[2]) and new[2]["hold"] == params[2]["hold"]      # an untouched channel
    assert new[0]["k"][0]["gain_start"] == 0.5 and new[1]["k"][1]["start"] != params[1]["k"][1]["start"]
    assert new[3]["tau_attack"] != params[3]["tau_attack"] and new[3]["hold"] == gr.hold_samples(gr.channel_settings(3)["sample_rate"], 0.2) > 0
    want, which = _follow(x1, st, new)                                  # the state carried over, the new parameters apply
    assert _bits_equal(env, want)
    assert _same_state(_state(bank, C), st)
    _check_gain(gain, want, which, new, "changed settings")
    bank.clear()
    z = _state(bank, C)
    assert not any(z[k].any() for k in KEYS)
    gain, env = _run(gpu, bank, x2)
    assert _bits_equal(env, _follow(x2, gr.fresh_state(C), new)[0])
    bank.close()


@pytest.mark.gpu
@pytest.mark.parametrize("hyst", [False, True])
def test_curve_over_a_level_ladder(gpu, hyst):
    C = 8
    bank, params = _bank(gpu, C)
    db = np.linspace(-96.0, 12.0, 2 * T + 29)
    x = np.tile((10.0 ** (db / 20.0)).astype(f32), (C, 1))
    x[:, ::5] *= -1.0
    din, dout = gpu.DeviceBuffer.from_host(x), gpu.DeviceBuffer((C, x.shape[1] + 3))
    dout.upload(np.full((C, x.shape[1] + 3), 7.0, f32))
    bank.curve(dout, din, x.shape[1], hyst=hyst, out_stride=x.shape[1] + 3)
    got = dout.download()
    assert np.all(got[:, x.shape[1]:] == 7.0)
    which = 1 if hyst else 0
    _check_gain(got[:, :x.shape[1]], x, which, params, "curve %d" % which, extra=1.0, scale=np.abs(x).astype(np.float64))
    inside = gr.gain_bound(x, which, params) > 0
    assert inside.sum() > 100                                           # the ladder has steps inside the zones
    bank.curve(din, din, x.shape[1], hyst=hyst)                         # in place
    assert _bits_equal(din.download(), got[:, :x.shape[1]])
    bank.close()


CPP = r'''
#include <lsp-plug.in/dsp-units/dynamics/Gate.h>
#include <cstdio>
#include <vector>
struct Readable: public lsp::dspu::Gate
{
    void read(float *dst) const { dst[0] = fEnvelope; dst[1] = fPeak; dst[2] = float(nHoldCounter); dst[3] = float(nCurve); }
};
int main(int argc, char **argv)
{
    const size_t n = 700;
    FILE *f = fopen(argv[1], "rb");
    std::vector<float> x(2 * n), out(6 * n + 4);                 // gain and env of 2n each, two curves of n, the state
    if (fread(x.data(), sizeof(float), x.size(), f) != x.size()) return 2;
    fclose(f);
    Readable c;
    c.set_sample_rate(48000);
    c.set_threshold(0.2f, 0.08f);
    c.set_zone(0.5f, 0.3f);
    c.set_reduction(0.02f);
    c.set_timings(0.1f, 0.15f);
    c.set_hold(0.1f);
    c.update_settings();                                        // Gate::process does not call it
    float *gain = out.data(), *env = gain + 2 * n, *cur = env + 2 * n;
    c.process(gain, env, x.data(), n);                          // with the envelope
    c.process(gain + n, NULL, x.data() + n, n);                 // without it
    c.curve(cur, x.data(), n, false);
    c.curve(cur + n, x.data(), n, true);
    c.read(cur + 2 * n);
    f = fopen(argv[2], "wb");
    fwrite(out.data(), sizeof(float), out.size(), f);
    fclose(f);
    c.destroy();
    return 0;
}
'''


@pytest.mark.gpu
def test_cpp_class_on_the_device(gpu, tmp_path):
    src, exe = str(tmp_path / "gate.cpp"), str(tmp_path / "gate")
    open(src, "w").write(CPP)
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-I" + os.path.join(PKG, "include"), "-I" + os.path.join(ROOT, "include"), src,
                           "-o", exe, "-L" + PKG, "-lmi_dspu", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    n = 700
    x = gr.bursts(60, 1, 2 * n)
    x.tofile(str(tmp_path / "in.bin"))
    out = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out
    r = np.fromfile(str(tmp_path / "out.bin"), f32)
    m = 2 * n
    gain, env, cur = r[:m][None, :], r[m:2 * m][None, :], r[2 * m:]
    s = dict(sample_rate=48000, open_threshold=0.2, close_threshold=0.08, open_zone=0.5, close_zone=0.3, reduction=0.02, attack=0.1,
             release=0.15, hold=0.1)
    params = [gpu.GateBank.compute_params(**s)]
    st, stats = gr.fresh_state(1), gr.fresh_stats()
    want, which = _follow(x, st, params, stats)
    assert stats["toggles"] >= 8
    assert _bits_equal(env[:, :n], want[:, :n])
    assert not env[0, n:].any()                                 # no envelope was asked for in the second call
    _check_gain(gain, want, which, params, "class process")
    lv = x[:, :n]
    scale = np.abs(lv).astype(np.float64)
    _check_gain(cur[:n][None, :], lv, 0, params, "class curve open", extra=1.0, scale=scale)
    _check_gain(cur[n:2 * n][None, :], lv, 1, params, "class curve close", extra=1.0, scale=scale)
    assert _bits_equal(cur[2 * n:2 * n + 2], [st["e"][0], st["peak"][0]])
    assert (cur[2 * n + 2], cur[2 * n + 3]) == (float(st["hold"][0]), float(st["curve"][0]))


@pytest.mark.gpu
def test_graph_capture_replays_direct_calls(gpu):
    C, n = 64, T + 100
    st = ctypes.c_void_p()
    gpu.check(gpu.lib.mi_dspu_stream_create(ctypes.byref(st)))
    bank, params = _bank(gpu, C)
    twin, _ = _bank(gpu, C)
    x = gr.bursts(70, C, 2 * n)
    d0, d1 = gpu.DeviceBuffer.from_host(x[:, :n]), gpu.DeviceBuffer.from_host(x[:, n:])
    g0, g1, e0, e1 = (gpu.DeviceBuffer((C, n)) for _ in range(4))
    gpu.check(gpu.lib.mi_dspu_graph_begin_capture(st))
    bank.process(g0, e0, d0, n, stream=st.value)
    bank.process(g1, e1, d1, n, stream=st.value)
    exe = ctypes.c_void_p()
    gpu.check(gpu.lib.mi_dspu_graph_end_capture(st, ctypes.byref(exe)))
    t = [gpu.DeviceBuffer((C, n)) for _ in range(4)]
    ref = gr.fresh_state(C)
    for rep in range(3):
        gpu.check(gpu.lib.mi_dspu_graph_launch(exe, st))
        twin.process(t[0], t[2], d0, n, stream=st.value)
        twin.process(t[1], t[3], d1, n, stream=st.value)
        got = [b.download(stream=st.value) for b in (g0, g1, e0, e1)]
        direct = [b.download(stream=st.value) for b in t]
        assert all(_bits_equal(a, b) for a, b in zip(got, direct)), rep
        want = np.concatenate([_follow(x[:, :n], ref, params)[0], _follow(x[:, n:], ref, params)[0]], axis=1)
        assert _bits_equal(np.concatenate(got[2:], axis=1), want), rep          # the state advances (curve included) on every replay
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
    state = gr.fresh_state(C)
    x0, x1 = gr.bursts(80, C, n), gr.bursts(81, C, n)
    d0, d1 = gpu.DeviceBuffer.from_host(x0), gpu.DeviceBuffer.from_host(x1)
    dg, de = gpu.DeviceBuffer((C, n)), gpu.DeviceBuffer((C, n))
    bank.process(dg, de, d0, n, stream=st.value)
    env0 = de.download(stream=st.value)
    assert _bits_equal(env0, _follow(x0, state, params)[0])
    before = _state(bank, C)
    gpu.check(gpu.lib.mi_dspu_graph_begin_capture(st))
    bank.set_threshold(0, 0.2, 0.08)
    bank.set_timings(3, 0.3, 0.12)
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
    assert new[0]["k"][0]["end"] != params[0]["k"][0]["end"] and new[3]["tau_attack"] != params[3]["tau_attack"]
    want, which = _follow(x1, state, new)                                               # the state carried over, the new parameters apply
    assert _bits_equal(de.download(stream=st.value), want)
    assert _same_state(_state(bank, C), state)
    _check_gain(dg.download(stream=st.value), want, which, new, "after the refused capture")
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
    x = gr.bursts(82, C, n)
    d = gpu.DeviceBuffer.from_host(x)
    g, e, tg, te = (gpu.DeviceBuffer((C, n)) for _ in range(4))
    gpu.check(gpu.lib.mi_dspu_graph_begin_capture(st))
    with pytest.raises(gpu.MiError) as err:
        bank.get_state(2, stream=st.value)
    assert err.value.code == -5 and "captured" in str(err.value)
    bank.process(g, e, d, n, stream=st.value)
    exe = ctypes.c_void_p()
    gpu.check(gpu.lib.mi_dspu_graph_end_capture(st, ctypes.byref(exe)))
    ref = gr.fresh_state(C)
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
