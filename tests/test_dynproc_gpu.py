"""mi_dynproc_bank (lsp::dspu::DynamicProcessor) on the device against tests/dynproc_ref.py: the envelope, the peak and the hold
counter bit for bit on every channel (the float32 restatement fed the library's own tables), the gain within the derived bound
of the float64 curve on that envelope; 1, 3 and 5 reaction ranges and 0, 1, 2 and 4 splines in one workgroup, placed level
crossings, across tiles, calls, in place, strides, process_apply, changed settings, curve and model, the C++ class and graph
capture."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import dynproc_ref as dr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "lsp-dsp-units_amd")
T, G = 256, 4                           # tile_chain_device.h: samples of a tile, channels of a workgroup
f32 = np.float32


def _bank(gpu, C, settings=dr.channel_settings):
    bank = gpu.DynamicProcessorBank(C)
    for ch in range(C):
        bank.configure(ch, **settings(ch))
    bank.update_settings()
    return bank, [bank.get_params(ch) for ch in range(C)]


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


def _check_gain(gain, env, params, what, extra=0.0, scale=None, **kw):
    """Within the bound on every sample; exactly 1 (times the scale) on a channel without splines."""
    g64, bound = dr.gain64(env, params, **kw), dr.gain_bound(env, params, **kw)
    none = np.array([len(p["splines"]) == 0 for p in params])
    bound = np.where(none[:, None], 0.0, bound + extra)
    if scale is not None:
        g64 = g64 * scale
    got = gain.astype(np.float64)
    assert np.array_equal(got[none], g64[none]), what
    ok, err = dr.within(got[~none], g64[~none], bound[~none])
    if err.size:
        print("%s: gain error at most %.2f u, %.3f of its bound (bound: median %.1f u, max %.1f u)"
              % (what, err.max(), (err / np.maximum(bound[~none], 1e-9)).max(), np.median(bound[~none]), bound.max()))
    assert np.all(ok), (what, err.max(), np.count_nonzero(~ok))


SHAPES = [(C, n) for C in (1, G, G + 1) for n in (1, 13, T, T + 1, 3 * T + 7)]


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_bit_exact_envelope_and_state_gain_within_bound(gpu, shape):
    C, n = shape
    bank, params = _bank(gpu, C)
    if C >= G:
        assert [len(p["splines"]) for p in params[:G]] == [0, 1, 2, 4]                      # in one workgroup
        assert [len(p["attack"]) for p in params[:G]] == [1, 3, 5, 2]
    st = dr.fresh_state(C)
    total = dict.fromkeys(dr.BRANCHES, 0)
    for blk in range(2):
        x = dr.sweep(20 * n + blk, C, n)
        gain, env = _run(gpu, bank, x)
        want, taken = dr.follow(x, st, params)
        for k in total:
            total[k] += taken[k]
        assert _bits_equal(env, want), (shape, blk, np.count_nonzero(env.view(np.uint32) != want.view(np.uint32)))
        assert _same_state(_state(bank, C), st), (shape, blk)
        _check_gain(gain, want, params, "%s block %d" % (shape, blk))
    if n >= T:
        assert all(total[k] > 0 for k in ("attack", "release", "rearm")), total
    bank.close()


@pytest.mark.gpu
def test_full_size_every_channel(gpu):
    C, n = 1024, 4096
    bank, params = _bank(gpu, C)
    x = dr.sweep(77, C, n)
    st = dr.fresh_state(C)
    gain, env = _run(gpu, bank, x)
    want, taken = dr.follow(x, st, params)
    assert all(taken[k] > 0 for k in dr.BRANCHES), taken
    # every one of the five attack and five release entries was selected on some sample of some channel
    assert np.all(taken["attack_entry"].sum(axis=0) > 0) and np.all(taken["release_entry"].sum(axis=0) > 0), \
        (taken["attack_entry"].sum(axis=0), taken["release_entry"].sum(axis=0))
    assert _bits_equal(env, want), np.count_nonzero(env.view(np.uint32) != want.view(np.uint32))
    assert _same_state(_state(bank, C), st)
    _check_gain(gain, want, params, "1024 x 4096")
    w = dr.branches(want, params)
    for j in range(4):                                          # every branch of every spline position
        assert {0, 1, 2} <= set(np.unique(w[:, :, j])), (j, np.unique(w[:, :, j]))
    bank.close()


LEVELS = [float(f32(v)) for v in (0.03, 0.1, 0.3, 0.6)]


def _range_settings(ch):
    """Four channels of one workgroup with 1, 3, 5 and 5 entries in both tables and 0, 1, 2, 4 splines.  Every range has a time
    of its own, in both tables, so the entry that a sample selects shows in its envelope; the attacks are short (one to five
    samples), so one loud sample carries the envelope over a level.  No hold."""
    nl = (0, 2, 4, 4)[ch % 4]
    nd = (0, 1, 2, 4)[ch % 4]
    dots = [(0.5, 0.3, 0.5), (0.02, 0.02, 0.7), (0.15, 0.12, 0.6), (0.06, 0.05, 0.8)]
    return dict(sample_rate=48000, hold=0.0, in_ratio=1.5, out_ratio=6.0, dots=[d if i < nd else None for i, d in enumerate(dots)],
                attack_levels=[LEVELS[3 - i] if i < nl else None for i in range(4)],
                release_levels=[LEVELS[(i + 2) % 4] if i < nl else None for i in range(4)],
                attack_times=[0.02, 0.03, 0.045, 0.07, 0.1], release_times=[0.2, 0.35, 0.6, 1.0, 1.7])


@pytest.mark.gpu
def test_reaction_ranges_and_placed_level_crossings(gpu):
    C, n = G, 3 * T + 7
    bank, params = _bank(gpu, C, _range_settings)
    assert [len(p["attack"]) for p in params] == [1, 3, 5, 5] and [len(p["release"]) for p in params] == [1, 3, 5, 5]
    placed = [0, T - 1, T, n - 1]
    x = np.full((C, 2 * n), 1e-3, f32)
    for i in placed + [n]:                                      # n: the first sample of the second call
        x[:, i] = 2.0
    # 255 and n - 1 cross the level 0.3 only; 256 and n, attacks again, take the tau of THAT range from the envelope carried
    # over the tile's or the call's end, and cross 0.6 with it
    x[:, [T - 1, n - 1]] = 0.45
    x[:, 400:420] = np.linspace(0.02, 0.9, 20, dtype=f32)       # attacks from every range
    st = dr.fresh_state(C)
    entries = {"attack_entry": 0, "release_entry": 0}
    envs = []
    for blk in range(2):
        part = np.ascontiguousarray(x[:, blk * n:(blk + 1) * n])
        gain, env = _run(gpu, bank, part)
        before = st["e"].copy()
        want, taken = dr.follow(part, st, params)
        assert _bits_equal(env, want), blk
        assert _same_state(_state(bank, C), st), blk
        _check_gain(gain, want, params, "ranges block %d" % blk)
        for k in entries:
            entries[k] = entries[k] + taken[k]
        envs.append(np.concatenate([before[:, None], want], axis=1))       # envs[b][:, i] is the envelope BEFORE sample i
    for ch in (1, 2, 3):                                        # by construction: a level is crossed upward at each placed sample
        lv = np.array([float(r["level"]) for r in params[ch]["attack"][1:]])
        for b, i in [(0, i) for i in placed] + [(1, 0)]:
            assert np.any((envs[b][ch, i] < lv) & (lv <= envs[b][ch, i + 1])), (ch, b, i)
        # ... and the sample behind 255 and behind n - 1 used another attack entry than the default: the crossing shows
        tab = params[ch]["attack"]
        for b, i in ((0, T), (1, 0)):
            tau, k = dr.solve_reaction(tab, envs[b][ch, i])
            assert k > 0 and tau != tab[0]["tau"] and envs[b][ch, i + 1] == f32(envs[b][ch, i] + f32(f32(2.0 - envs[b][ch, i]) * tau)), (ch, b)
    assert np.all(entries["attack_entry"][2] > 0) and np.all(entries["release_entry"][2] > 0), entries     # all ten entries
    assert np.count_nonzero(entries["attack_entry"][1]) == 3 and np.count_nonzero(entries["release_entry"][1]) == 3
    bank.close()


def _ladder_settings(ch):
    s = _range_settings(ch)
    s.update(attack_times=[0.0] * 5, release_times=[0.0] * 5, attack_levels=[], release_levels=[])      # the envelope IS the input
    return s


@pytest.mark.gpu
def test_spline_counts_in_one_workgroup_and_every_branch(gpu):
    C = G
    bank, params = _bank(gpu, C, _ladder_settings)
    assert [len(p["splines"]) for p in params] == [0, 1, 2, 4]
    db = np.linspace(-150.0, 30.0, T + 45)
    x = np.tile((10.0 ** (db / 20.0)).astype(f32), (C, 1))
    gain, env = _run(gpu, bank, x)
    assert _bits_equal(env, x)                                   # tau = 1 both ways on a rising input
    w = dr.branches(env, params)
    for ch in range(C):
        for j in range(len(params[ch]["splines"])):
            assert {0, 1, 2} <= set(np.unique(w[ch, :, j])), (ch, j)
    _check_gain(gain, env, params, "spline ladder")
    assert np.all(gain[0] == 1.0)                                # no spline: exactly 1
    # the lower limit of process() is 1e-6: every level below it has the gain of 1e-6, not that of 1e-10
    low = np.abs(env[1]) < 1e-6
    assert low.sum() > 20 and len(np.unique(gain[1][low])) == 1
    assert gain[1][low][0] != f32(dr.gain64(np.array([[1e-7]], f32), [params[1]], lo=dr.FLOAT_SAT_M_INF)[0, 0])
    bank.close()


def _hold_settings(hold_ms):
    def settings(ch):
        s = dr.channel_settings(ch)
        s.update(sample_rate=48000, hold=hold_ms)
        return s
    return settings


@pytest.mark.gpu
@pytest.mark.parametrize("hold", [(0.0, 0), (0.03, 1), (6.26, 300)])
def test_hold_counts_across_tiles_and_calls(gpu, hold):
    ms, samples = hold
    C, n = 3, 300
    bank, params = _bank(gpu, C, _hold_settings(ms))
    assert [p["hold"] for p in params] == [samples] * C and samples in (0, 1, T + 44)
    x = np.full((C, 2 * n), 1e-3, f32)
    x[:, :200] = 1.0                        # the countdown starts at sample 200: over the tile's end at 256 and the call's at 300
    x[:, 550:560] = 2.0                     # a re-arm in the second call
    st = dr.fresh_state(C)
    for blk in range(2):
        part = np.ascontiguousarray(x[:, blk * n:(blk + 1) * n])
        gain, env = _run(gpu, bank, part)
        want, taken = dr.follow(part, st, params)
        assert _bits_equal(env, want), (hold, blk)
        assert _same_state(_state(bank, C), st), (hold, blk)
        if blk == 0:
            assert taken["hold"] == C * min(samples, 100)
            assert np.all(st["hold"] == max(samples - 100, 0))          # the counter crosses the call boundary
        else:
            assert taken["rearm"] > 0
        _check_gain(gain, want, params, "hold %d block %d" % (samples, blk))
    bank.close()


@pytest.mark.gpu
def test_runs_of_calls_equal_one_long_call(gpu):
    C = G + 1
    runs = [1, 7, T - 1, T + 1, T + 90]
    x = dr.sweep(5, C, sum(runs))
    one, params = _bank(gpu, C)
    whole_gain, whole_env = _run(gpu, one, x)
    parts, _ = _bank(gpu, C)
    st = dr.fresh_state(C)
    pos = 0
    for r in runs:
        part = np.ascontiguousarray(x[:, pos:pos + r])
        gain, env = _run(gpu, parts, part)
        want, _ = dr.follow(part, st, params)
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
    x = dr.sweep(6, C, n)
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
    x = dr.sweep(8, C, n)
    gain, env = _run(gpu, ref, x)
    a, _ = _bank(gpu, C)
    buf = gpu.DeviceBuffer.from_host(x)
    a.process(buf, None, buf, n)                                        # gain == in
    assert _bits_equal(buf.download(), gain)
    b, _ = _bank(gpu, C)
    buf, dg = gpu.DeviceBuffer.from_host(x), gpu.DeviceBuffer((C, n))
    b.process(dg, buf, buf, n)                                          # env == in, the gain apart
    assert _bits_equal(buf.download(), env) and _bits_equal(dg.download(), gain)
    for k in (ref, a, b):
        k.close()


@pytest.mark.gpu
@pytest.mark.parametrize("strides", [(301, 303, 307), (304, 312, 308), (300, 300, 300)])
def test_strides_and_unaligned_rows(gpu, strides):
    C, n = G + 1, T + 44
    gs, es, xs = strides
    bank, params = _bank(gpu, C)
    x = dr.sweep(9, C, n)
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
    want, _ = dr.follow(x, dr.fresh_state(C), params)
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
    x = dr.sweep(11, C, n)
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
    e, _ = _bank(gpu, C)                                                # rows that are not 16-byte aligned
    pad = lambda v, s: np.concatenate([v, np.full((C, s - n), 5.0, f32)], axis=1)
    dx, da, dd = gpu.DeviceBuffer.from_host(pad(x, n + 1)), gpu.DeviceBuffer.from_host(pad(audio, n + 3)), gpu.DeviceBuffer((C, n + 2))
    dd.upload(np.full((C, n + 2), 7.0, f32))
    e.process_apply(dd, da, dx, n, out_stride=n + 2, audio_stride=n + 3, sc_stride=n + 1)
    got = dd.download()
    assert _bits_equal(got[:, :n], want) and np.all(got[:, n:] == 7.0)
    for k in (a, b, c, e):
        k.close()


@pytest.mark.gpu
def test_settings_changed_between_calls_and_clear(gpu):
    C, n = G + 1, T + 9
    bank, params = _bank(gpu, C)
    fresh = gpu.DynamicProcessorBank(1)
    fresh.update_settings()                                             # four dots at (0, 0, 0): returns without error
    fresh.close()
    st = dr.fresh_state(C)
    x0, x1, x2 = (dr.sweep(20 + i, C, n) for i in range(3))
    _, env = _run(gpu, bank, x0)
    assert _bits_equal(env, dr.follow(x0, st, params)[0])
    bank.set_out_ratio(1, 2.5)
    bank.set_dot(2, [i for i, d in enumerate(dr.channel_settings(2)["dots"]) if d is not None][0], None)
    bank.set_attack_time(3, 0, 0.7)
    bank.set_release_level(0, 0, 0.2)
    bank.set_hold(3, 1.0)
    gain, env = _run(gpu, bank, x1)                                     # process() runs update_settings() first
    new = [bank.get_params(ch) for ch in range(C)]
    assert dr.flatten(new[4]) == dr.flatten(params[4]) and new[4]["hold"] == params[4]["hold"]      # an untouched channel
    assert new[1]["splines"][-1]["post_ratio"] != params[1]["splines"][-1]["post_ratio"]
    assert len(new[2]["splines"]) == len(params[2]["splines"]) - 1 and len(new[0]["release"]) == len(params[0]["release"]) + 1
    assert new[3]["attack"][0]["tau"] != params[3]["attack"][0]["tau"]
    assert new[3]["hold"] == dr.hold_samples(dr.channel_settings(3)["sample_rate"], 1.0) > 0
    want, _ = dr.follow(x1, st, new)                                    # the state carried over, the new parameters apply
    assert _bits_equal(env, want)
    assert _same_state(_state(bank, C), st)
    _check_gain(gain, want, new, "changed settings")
    bank.clear()
    z = _state(bank, C)
    assert not z["e"].any() and not z["peak"].any() and not z["hold"].any()
    gain, env = _run(gpu, bank, x2)
    assert _bits_equal(env, dr.follow(x2, dr.fresh_state(C), new)[0])
    bank.close()


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["curve", "model"])
def test_curve_and_model_over_a_level_ladder(gpu, what):
    C = 8
    bank, params = _bank(gpu, C)
    db = np.linspace(-240.0, 240.0, 2 * T + 29)
    x = np.tile((10.0 ** (db / 20.0)).astype(f32), (C, 1))
    x[:, ::5] *= -1.0
    n = x.shape[1]
    din, dout = gpu.DeviceBuffer.from_host(x), gpu.DeviceBuffer((C, n + 3))
    dout.upload(np.full((C, n + 3), 7.0, f32))
    call = bank.curve if what == "curve" else bank.model
    call(dout, din, n, out_stride=n + 3)
    got = dout.download()
    assert np.all(got[:, n:] == 7.0)
    kw = dict(lo=dr.FLOAT_SAT_M_INF, model=what == "model")
    _check_gain(got[:, :n], x, params, what, extra=1.0, scale=dr.limited(x, dr.FLOAT_SAT_M_INF).astype(np.float64), **kw)
    call(din, din, n)                                                   # in place
    assert _bits_equal(din.download(), got[:, :n])
    bank.close()


CPP = r'''
#include <lsp-plug.in/dsp-units/dynamics/DynamicProcessor.h>
#include <cstdio>
#include <vector>
int main(int argc, char **argv)
{
    const size_t n = 700;
    FILE *f = fopen(argv[1], "rb");
    std::vector<float> x(2 * n + 8), out(6 * n + 16);            // gain and env of 2n + 8 each, curve and model of n
    if (fread(x.data(), sizeof(float), x.size(), f) != x.size()) return 2;
    fclose(f);
    lsp::dspu::DynamicProcessor c;
    c.set_sample_rate(48000);
    c.set_in_ratio(1.5f);
    c.set_out_ratio(4.0f);
    c.set_hold(0.5f);
    c.set_dot(0, 0.25f, 0.2f, 0.5f);
    c.set_dot(1, NULL);
    c.set_dot(2, 0.01f, 0.02f, 0.7f);
    c.set_dot(3, NULL);
    for (size_t i = 0; i < 4; ++i) { c.set_attack_level(i, -1.0f); c.set_release_level(i, -1.0f); }
    c.set_attack_level(2, 0.3f);
    c.set_release_level(0, 0.05f);
    c.set_attack_time(0, 0.5f); c.set_attack_time(3, 0.1f);
    c.set_release_time(0, 4.0f); c.set_release_time(1, 1.5f);
    if (c.modified())
        c.update_settings();
    float *gain = out.data(), *env = gain + 2 * n + 8, *cur = env + 2 * n + 8;
    c.process(gain, env, x.data(), n);                          // with the envelope
    c.process(gain + n, NULL, x.data() + n, n);                 // without it
    for (size_t i = 0; i < 8; ++i)                              // the scalar form on the host, from the device's state
        gain[2 * n + i] = c.process(env + 2 * n + i, x[2 * n + i]);
    c.curve(cur, x.data(), n);
    c.model(cur + n, x.data(), n);
    f = fopen(argv[2], "wb");
    fwrite(out.data(), sizeof(float), out.size(), f);
    fclose(f);
    c.destroy();
    return 0;
}
'''


@pytest.mark.gpu
def test_cpp_class_on_the_device(gpu, tmp_path):
    src, exe = str(tmp_path / "dyn.cpp"), str(tmp_path / "dyn")
    open(src, "w").write(CPP)
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-I" + os.path.join(PKG, "include"), "-I" + os.path.join(ROOT, "include"), src,
                           "-o", exe, "-L" + PKG, "-lmi_dspu", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    n = 700
    x = dr.sweep(60, 1, 2 * n + 8)
    x.tofile(str(tmp_path / "in.bin"))
    out = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out
    r = np.fromfile(str(tmp_path / "out.bin"), f32)
    m = 2 * n + 8
    gain, env, cur = r[:m][None, :], r[m:2 * m][None, :], r[2 * m:]
    params = [gpu.DynamicProcessorBank.compute_params(
        sample_rate=48000, hold=0.5, in_ratio=1.5, out_ratio=4.0, dots=[(0.25, 0.2, 0.5), None, (0.01, 0.02, 0.7)],
        attack_levels=[None, None, 0.3], release_levels=[0.05], attack_times=[0.5, 0.0, 0.0, 0.1], release_times=[4.0, 1.5])]
    want, _ = dr.follow(x, dr.fresh_state(1), params)
    assert _bits_equal(env[:, :n], want[:, :n]) and _bits_equal(env[:, 2 * n:], want[:, 2 * n:])
    assert not env[0, n:2 * n].any()                            # no envelope was asked for in the second call
    _check_gain(gain[:, :2 * n], want[:, :2 * n], params, "class process")
    _check_gain(gain[:, 2 * n:], want[:, 2 * n:], params, "class scalar process", lo=dr.FLOAT_SAT_M_INF)
    lv = x[:, :n]
    scale = dr.limited(lv, dr.FLOAT_SAT_M_INF).astype(np.float64)
    _check_gain(cur[:n][None, :], lv, params, "class curve", extra=1.0, scale=scale, lo=dr.FLOAT_SAT_M_INF)
    _check_gain(cur[n:2 * n][None, :], lv, params, "class model", extra=1.0, scale=scale, lo=dr.FLOAT_SAT_M_INF, model=True)


@pytest.mark.gpu
def test_graph_capture_replays_direct_calls(gpu):
    C, n = 64, T + 100
    st = ctypes.c_void_p()
    gpu.check(gpu.lib.mi_dspu_stream_create(ctypes.byref(st)))
    bank, params = _bank(gpu, C)
    twin, _ = _bank(gpu, C)
    x = dr.sweep(70, C, 2 * n)
    d0, d1 = gpu.DeviceBuffer.from_host(x[:, :n]), gpu.DeviceBuffer.from_host(x[:, n:])
    g0, g1, e0, e1 = (gpu.DeviceBuffer((C, n)) for _ in range(4))
    gpu.check(gpu.lib.mi_dspu_graph_begin_capture(st))
    bank.process(g0, e0, d0, n, stream=st.value)
    bank.process(g1, e1, d1, n, stream=st.value)
    exe = ctypes.c_void_p()
    gpu.check(gpu.lib.mi_dspu_graph_end_capture(st, ctypes.byref(exe)))
    t = [gpu.DeviceBuffer((C, n)) for _ in range(4)]
    ref = dr.fresh_state(C)
    for rep in range(3):
        gpu.check(gpu.lib.mi_dspu_graph_launch(exe, st))
        twin.process(t[0], t[2], d0, n, stream=st.value)
        twin.process(t[1], t[3], d1, n, stream=st.value)
        got = [b.download(stream=st.value) for b in (g0, g1, e0, e1)]
        direct = [b.download(stream=st.value) for b in t]
        assert all(_bits_equal(a, b) for a, b in zip(got, direct)), rep
        want = np.concatenate([dr.follow(x[:, :n], ref, params)[0], dr.follow(x[:, n:], ref, params)[0]], axis=1)
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
    state = dr.fresh_state(C)
    x0, x1 = dr.sweep(80, C, n), dr.sweep(81, C, n)
    d0, d1 = gpu.DeviceBuffer.from_host(x0), gpu.DeviceBuffer.from_host(x1)
    dg, de = gpu.DeviceBuffer((C, n)), gpu.DeviceBuffer((C, n))
    bank.process(dg, de, d0, n, stream=st.value)
    env0 = de.download(stream=st.value)
    assert _bits_equal(env0, dr.follow(x0, state, params)[0])
    before = _state(bank, C)
    gpu.check(gpu.lib.mi_dspu_graph_begin_capture(st))
    bank.set_dot(2, [i for i, d in enumerate(dr.channel_settings(2)["dots"]) if d is not None][0], None)
    bank.set_attack_time(3, 0, 0.7)
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
    assert len(new[2]["splines"]) == len(params[2]["splines"]) - 1 and new[3]["attack"][0]["tau"] != params[3]["attack"][0]["tau"]
    want, _ = dr.follow(x1, state, new)                                               # the state carried over, the new parameters apply
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
    x = dr.sweep(82, C, n)
    d = gpu.DeviceBuffer.from_host(x)
    g, e, tg, te = (gpu.DeviceBuffer((C, n)) for _ in range(4))
    gpu.check(gpu.lib.mi_dspu_graph_begin_capture(st))
    with pytest.raises(gpu.MiError) as err:
        bank.get_state(2, stream=st.value)
    assert err.value.code == -5 and "captured" in str(err.value)
    bank.process(g, e, d, n, stream=st.value)
    exe = ctypes.c_void_p()
    gpu.check(gpu.lib.mi_dspu_graph_end_capture(st, ctypes.byref(exe)))
    ref = dr.fresh_state(C)
    for rep in range(3):
        gpu.check(gpu.lib.mi_dspu_graph_launch(exe, st))
        twin.process(tg, te, d, n, stream=st.value)
        got = [b.download(stream=st.value) for b in (g, e)]
        direct = [b.download(stream=st.value) for b in (tg, te)]
        assert all(_bits_equal(a, b) for a, b in zip(got, direct)), rep
        assert _bits_equal(got[1], dr.follow(x, ref, params)[0]), rep                # the state advances on every replay
    assert _same_state(_state(bank, C), ref)                                        # ... and can be read again after the capture
    gpu.lib.mi_dspu_graph_destroy(exe)
    bank.close()
    twin.close()
    gpu.check(gpu.lib.mi_dspu_stream_destroy(st))
