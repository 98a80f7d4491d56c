"""lsp::dspu::Depopper without a device: tests/depopper_ref.py against every recorded case of the reference's own class (env, gain,
state words and both buffers bit for bit), the library's designer (mi_depopper_compute_params) against the recorded integers and
polynomials bit for bit and against the recorded fade tables (polynomial modes bit for bit; sine and Gaussian by the interval rule
of DESIGN 3.24), the refusals that need no device, the generator's own invariants, and the output's independence of how a
stream is cut into calls."""
import ctypes
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import depopper_ref as dr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, GOLDEN)
import make_depopper_vectors as gen  # noqa: E402

f32, u32 = np.float32, np.uint32
REFERENCE = os.path.join(os.path.dirname(ROOT), "reference")
SETTERS = {gen.IN_MODE: "set_fade_in_mode", gen.OUT_MODE: "set_fade_out_mode", gen.IN_TIME: "set_fade_in_time", gen.OUT_TIME: "set_fade_out_time",
           gen.IN_THRESH: "set_fade_in_threshold", gen.OUT_THRESH: "set_fade_out_threshold", gen.IN_DELAY: "set_fade_in_delay",
           gen.OUT_DELAY: "set_fade_out_delay", gen.RMS_LENGTH: "set_rms_length"}


@pytest.fixture(scope="module")
def recorded():
    return gen.load()


def _same(a, b):
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    return a.shape == b.shape and np.array_equal(a.view(u32), b.view(u32))


def replay(x, c, cut=None):
    """The case's operations on the restatement -> (object, env, gain); cut: other call lengths for the same samples."""
    d, env, gain, at = dr.Depopper(), [], [], 0
    for op in c["ops"]:
        w = int(op[0])
        if w == gen.INIT:
            d.init(int(op[1]), op[2], op[3])
        elif w == gen.PROCESS:
            m, k = int(op[1]), 0
            while m > 0:
                step = m if cut is None else min(m, cut[k % len(cut)])
                e, g = d.process(x[c["signal"], at:at + step])
                env.append(e), gain.append(g)
                at, m, k = at + step, m - step, k + 1
        elif w == gen.RECONFIGURE:
            d.reconfigure()
        else:
            getattr(d, SETTERS[w])(int(op[1]) if w in (gen.IN_MODE, gen.OUT_MODE) else op[1])
    return d, np.concatenate(env), np.concatenate(gain)


def test_restatement_equals_every_recorded_case(recorded):
    x, cases = recorded
    assert len(cases) >= 20
    for c in cases:
        d, env, gain = replay(x, c)
        assert d.accepted(), c["name"]
        assert _same(env, c["env"]) and _same(gain, c["gain"]), c["name"]
        assert np.array_equal(d.state_words(), c["state"]), (c["name"], d.state_words(), c["state"])
        assert np.array_equal(d.design_words(), c["design"]), c["name"]
        rb, gb = d.buffers()
        assert _same(rb, c["rms_buf"]) and _same(gb, c["gain_buf"]), c["name"]
        assert _same(dr.fade_table(d.sFadeIn), c["tab_in"]) and _same(dr.fade_table(d.sFadeOut), c["tab_out"]), c["name"]


def test_output_does_not_depend_on_how_the_stream_is_cut(recorded):
    x, cases = recorded
    by = {c["name"]: c for c in cases}
    a, b = by["one call"], by["the same in uneven calls"]
    assert _same(a["env"], b["env"]) and _same(a["gain"], b["gain"]) and np.array_equal(a["state"], b["state"])
    assert _same(a["rms_buf"], b["rms_buf"]) and _same(a["gain_buf"], b["gain_buf"])
    for name, cut in (("both wraps max_rms 1", (1, 999, 17)), ("setters between calls", (64,)), ("NaN and Inf with delays", (3, 700))):
        d, env, gain = replay(x, by[name], cut)
        assert _same(env, by[name]["env"]) and _same(gain, by[name]["gain"]) and np.array_equal(d.state_words(), by[name]["state"]), name


def _final_settings(c):
    """The setters' fields as the case's operations leave them (the restatement's setters are the reference's)."""
    d = dr.Depopper()
    for op in c["ops"]:
        w = int(op[0])
        if w == gen.INIT:
            d.init(int(op[1]), op[2], op[3])
        elif w in SETTERS:
            getattr(d, SETTERS[w])(int(op[1]) if w in (gen.IN_MODE, gen.OUT_MODE) else op[1])
    return d


def _compute(mi, d, tables=True):
    capi = importlib.import_module("lsp-dsp-units_amd.capi")
    s, out = capi.DepopperParams(), capi.DepopperParams()
    s.sample_rate, s.look_max, s.rms_max, s.rms_length = d.nSampleRate & (2 ** 64 - 1), d.fLookMax, d.fRmsMax, d.fRmsLength
    for to, fade in ((s.fade_in, d.sFadeIn), (s.fade_out, d.sFadeOut)):
        to.mode, to.threshold, to.time, to.delay = fade.enMode, fade.fThresh, fade.fTime, fade.fDelay
    tin, tout = np.full(1 << 12, 7.0, f32), np.full(1 << 12, 7.0, f32)
    r = mi.lib.mi_depopper_compute_params(ctypes.byref(s), ctypes.byref(out), ctypes.c_void_p(tin.ctypes.data), tin.size,
                                          ctypes.c_void_p(tout.ctypes.data), tout.size)
    return r, out, tin, tout


def _design_words(p):
    def fade(f):
        return [f.samples, f.delay_samples] + [int(v) for v in np.array(list(f.poly), f32).view(u32)]
    return np.array(fade(p.fade_in) + fade(p.fade_out) + [p.rms_len, p.look_count, int(f32(p.rms_norm).view(u32)), p.look_min_off, p.look_max_off,
                                                          p.rms_min_off, p.rms_max_off], np.int64)


def _within_interval(table, fade, fn64):
    """DESIGN 3.24, "Sinusoids": every recorded entry lies within the span of the restatement evaluated with the float64 function
    rounded once, its float32 predecessor and its successor.  -> the number of entries that are not the once-rounded value"""
    once = dr.once(fn64)
    differ = 0
    for x, got in enumerate(table):
        vals = []
        for nudge in (None, -np.inf, np.inf):
            f = once if nudge is None else (lambda v, n=nudge: np.nextafter(once(v), f32(n)))
            vals.append(dr.crossfade(fade, x, sin=f, exp=f))
        assert min(vals) <= got <= max(vals), (x, got, vals)
        differ += int(f32(got).view(u32) != f32(vals[0]).view(u32))
    return differ


def test_designer_integers_polynomials_and_tables_against_the_recordings(mi, recorded):
    x, cases = recorded
    differ = total = 0
    for c in cases:
        d = _final_settings(c)
        r, p, tin, tout = _compute(mi, d)
        assert r == 0, (c["name"], mi.lib.mi_dspu_last_error())
        assert np.array_equal(_design_words(p), c["design"]), (c["name"], _design_words(p), c["design"])
        d.reconfigure()
        for fade, mine, rec in ((d.sFadeIn, tin, c["tab_in"]), (d.sFadeOut, tout, c["tab_out"])):
            assert rec.size == max(fade.nSamples, 0) and np.all(mine[rec.size:] == 7.0), c["name"]
            if fade.enMode in (dr.LINEAR, dr.CUBIC, dr.PARABOLIC):
                assert _same(mine[:rec.size], rec), (c["name"], fade.enMode)
            else:
                fn = np.sin if fade.enMode == dr.SINE else np.exp
                _within_interval(mine[:rec.size], fade, fn)                 # this host's tables obey the rule as well
                differ, total = differ + _within_interval(rec, fade, fn), total + rec.size
    assert total > 2000
    print("sine and Gaussian table entries that are not the once-rounded value: %d of %d" % (differ, total))


def test_square_thresholds_decide_as_the_roots_do(mi):
    """The bank compares fRms * fRmsNorm with the threshold taken to the domain of squares.  mi_depopper_square_threshold is the
    search that update_settings() runs: its Q against the root itself (numpy's float32 sqrt is correctly rounded, as sqrtf is) at
    Q - 3 .. Q + 3 ulp, at 0, at +Inf and at NaN; for thresholds that are not above 0 and for NaN neither compare ever holds."""
    def square(t):
        q = ctypes.c_float(7.0)
        assert mi.lib.mi_depopper_square_threshold(ctypes.c_float(float(t)), ctypes.byref(q)) == 0
        return f32(q.value)

    ends = np.array([0.0, np.inf, np.nan], f32)
    rng = np.random.default_rng(5)
    tiny, huge = u32(1).view(f32), u32(0x7f7fffff).view(f32)
    some = [f32(v) for v in (0.0001, 0.05, 0.1, 0.25, 0.125, 1.0, 3e-20, 1e-30, 2e19, np.inf)] + [tiny, huge, u32(0x00800000).view(f32)]
    for t in some + list(rng.random(40).astype(f32)) + list(np.exp(rng.uniform(-80, 80, 40)).astype(f32)):
        q = square(t)
        bits = int(q.view(u32))
        assert q >= 0 and np.sqrt(q) >= t and (bits == 0 or np.sqrt(u32(bits - 1).view(f32)) < t), (t, q)
        around = np.concatenate([u32(np.clip(np.arange(bits - 3, bits + 4), 0, 0x7f800000)).view(f32), ends])
        with np.errstate(invalid="ignore"):
            assert np.array_equal(np.sqrt(around) < t, around < q), (t, q)
    probe = np.concatenate([np.array([0.0, tiny, 1e-30, 0.5, huge], f32), ends])
    for t in (0.0, -0.0, -1.0, -np.inf, np.nan):
        q = square(f32(t))
        with np.errstate(invalid="ignore"):
            assert not np.any(np.sqrt(probe) < f32(t)) and not np.any(probe < q), (t, q)
    assert mi.lib.mi_depopper_square_threshold(ctypes.c_float(1.0), None) == -1


def test_refusals_that_need_no_device(mi):
    lib = mi.lib
    good = dr.Depopper()
    good.init(48000, 10.0, 1.0)
    good.set_rms_length(1.0)
    assert _compute(mi, good)[0] == 0

    def refused(change, text):
        d = dr.Depopper()
        d.init(48000, 10.0, 1.0)
        d.set_rms_length(1.0)
        change(d)
        r = _compute(mi, d)[0]
        assert r == -1 and text in lib.mi_dspu_last_error(), (text, lib.mi_dspu_last_error())

    refused(lambda d: d.set_rms_length(0.0), b"nRmsLen == 0")
    refused(lambda d: d.set_rms_length(0.02), b"nRmsLen == 0")                             # 0.96 of a sample
    refused(lambda d: d.set_fade_out_time(10.001), b"fade-out")
    refused(lambda d: d.set_fade_out_time(-0.5), b"fade-out")
    refused(lambda d: d.set_fade_in_time(float("nan")), b"not a number")
    refused(lambda d: d.set_fade_out_delay(float("inf")), b"not a number")
    refused(lambda d: d.set_fade_in_time(30000.0), b"2^20")
    # what a refused design leaves in *designed: the reference's values where it defines them (reconfigure 0), nothing (1)
    d = dr.Depopper()
    d.init(48000, 10.0, 1.0)
    d.set_fade_out_time(10.001)
    r, p, _, _ = _compute(mi, d)
    d.reconfigure()
    assert r == -1 and p.reconfigure == 0 and np.array_equal(_design_words(p), d.design_words()) and p.rms_len == 0
    d.set_fade_in_time(float("nan"))
    r, p, _, _ = _compute(mi, d)
    assert r == -1 and p.reconfigure == 1
    # init() alone
    capi = importlib.import_module("lsp-dsp-units_amd.capi")
    e = capi.DepopperParams()
    assert lib.mi_depopper_compute_extents(48000, 10.0, 1.0, ctypes.byref(e)) == 0 and e.sample_rate == 48000 and e.look_max == f32(10.0)
    assert (e.look_min_off, e.look_max_off, e.rms_min_off, e.rms_max_off) == (good.nLookMin, good.nLookMax, good.nRmsMin, good.nRmsMax)
    assert (e.look_min_off, e.rms_min_off) == (512 + 64, 64)
    for bad in ((48000, -1.0, 1.0), (48000, float("nan"), 1.0), (48000, 10.0, 1e9)):
        assert lib.mi_depopper_compute_extents(*bad, ctypes.byref(e)) == -1, bad
    assert lib.mi_depopper_compute_extents(48000, 10.0, 1.0, None) == -1
    fresh = dr.Depopper()
    fresh.nSampleRate = 2 ** 64 - 1
    assert _compute(mi, fresh)[0] == -1 and b"init" in lib.mi_dspu_last_error()             # never init()ed
    for bad in ((48000, -1.0, 1.0), (48000, float("nan"), 1.0), (48000, 10.0, 1e9)):
        d = dr.Depopper()
        d.nSampleRate, d.fLookMax, d.fRmsMax = bad[0], f32(bad[1]), f32(bad[2])
        assert _compute(mi, d)[0] == -1
    clamp = dr.Depopper()                                                                   # an RMS length outside [0, max_rms] is clamped
    clamp.init(48000, 10.0, 1.0)
    clamp.fRmsLength = f32(5.0)
    r, p, _, _ = _compute(mi, clamp)
    assert r == 0 and p.rms_len == 48 and p.rms_length == f32(1.0)
    # NULL handles are refused, never followed
    byref, h = ctypes.byref, ctypes.c_void_p()
    assert lib.mi_depopper_bank_init(None, 0, 48000, 10.0, 1.0) == -5 and lib.mi_depopper_bank_update_settings(None, None) == -5
    for what in ("set_fade_in_time", "set_fade_out_time", "set_fade_in_threshold", "set_fade_out_threshold", "set_fade_in_delay",
                 "set_fade_out_delay", "set_rms_length"):
        assert getattr(lib, "mi_depopper_bank_" + what)(None, 0, 1.0, None) == -5, what
    assert lib.mi_depopper_bank_set_fade_in_mode(None, 0, 0, None) == -5 and lib.mi_depopper_bank_set_fade_out_mode(None, 0, 0, None) == -5
    assert lib.mi_depopper_bank_get_params(None, 0, None) == -5 and lib.mi_depopper_bank_get_state(None, 0, None, None, None, None) == -5
    assert lib.mi_depopper_bank_set_state(None, 0, None, None, None, None) == -5 and lib.mi_depopper_bank_set_settings(None, 0, None) == -5
    assert lib.mi_depopper_bank_get_fade_table(None, 0, 0, None, 0, None) == -5 and lib.mi_depopper_bank_latency(None, 0, None) == -5
    assert lib.mi_depopper_bank_process(None, None, None, None, 4, 4, 4, 4, None) == -5
    assert lib.mi_depopper_bank_destroy(None) == 0
    assert lib.mi_depopper_bank_create(None, 1) == -1 and lib.mi_depopper_bank_create(byref(h), 0) == -1 and not h.value
    assert lib.mi_depopper_compute_params(None, None, None, 0, None, 0) == -1


def test_recorded_inventories(recorded):
    x, cases = recorded
    dump = json.load(open(os.path.join(GOLDEN, "depopper_dump_keys.json")))
    names = json.load(open(os.path.join(GOLDEN, "depopper_public_names.json")))
    assert dump["sizeof"] == [248, 48] and len(dump["Depopper"]) == 37 and dump["Depopper"][0] == "0:nSampleRate" and dump["Depopper"][-1] == "0:bReconfigure"
    assert "set_release" in names["util/Depopper.h"] and "latency" in names["util/Depopper.h"]
    assert os.path.getsize(gen.OUT) < 400 * 1024 and x.shape == (3, gen.N)
    modes = {(int(c["ops"][1][1]), int(c["ops"][2][1])) for c in cases}
    assert {m for m, _ in modes} == set(range(5)) and {m for _, m in modes} == set(range(5))
    assert {int(c["design"][12]) for c in cases} >= {1, 31, 32, 33, 48, 96} and {int(c["design"][6]) for c in cases} >= {0, 1, 255, 257, 480}


@pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE, "src", "main", "util")), reason="the reference tree is not here")
def test_generator_reproduces_the_stored_file():
    data, dump, names = gen.build(REFERENCE)
    assert data == open(gen.OUT, "rb").read()
    assert dump == json.load(open(os.path.join(GOLDEN, "depopper_dump_keys.json")))
    assert names == json.load(open(os.path.join(GOLDEN, "depopper_public_names.json")))


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_chain_keeps_its_two_roundings(tmp_path):
    """(fRms + x) - g is two dependent roundings and fRms * fRmsNorm a product of its own: no fused multiply-add in the chain's
    body under the Makefile's -ffp-contract=on."""
    pkg = os.path.join(ROOT, "lsp-dsp-units_amd")
    asm = str(tmp_path / "depopper.s")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(pkg, "csrc"), "-I" + os.path.join(pkg, "include"), "-ffp-contract=on", "--cuda-device-only", "-S",
                           os.path.join(pkg, "csrc", "depopper.hip"), "-o", asm])
    text = open(asm).read()
    start = text.index("depopper_chain_tile")
    body = text[text.index(":", start):text.index("s_setpc_b64", start)]
    assert "v_add_f32" in body and "v_sub_f32" in body and "v_mul_f32" in body
    assert "fma" not in body and "v_mad" not in body and "v_mac" not in body
