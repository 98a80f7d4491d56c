"""Oscillator without a device: the numpy restatement against the reference's recorded outputs and settings words (bit for bit;
sinusoid samples by the interval rule), what the recorded cases are there for, the closed-form phase against the serial
accumulator, what the bank defines where the reference does not, the C-ABI's settings arithmetic against the restatement on
every recorded case, and refusals that need no device."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import oscillator_ref as R
from oversampler_ref import OversamplerRef

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_oscillator_vectors as gen  # noqa: E402

f32, u32 = np.float32, np.uint32
PKG = os.path.join(ROOT, "lsp-dsp-units_amd")
REFERENCE = os.path.join(os.path.dirname(ROOT), "reference")


def oversampler():
    return OversamplerRef(1, None)


@pytest.fixture(scope="module")
def recorded():
    return gen.load()


@pytest.fixture(scope="module")
def restated(recorded):
    """Every recorded case through the restatement with S*, its predecessor and its successor: computed once."""
    return [tuple(R.run_case(c, sine=s, oversampler=oversampler) for s in (R.sine_star, R.sine_prev, R.sine_next)) for c in recorded]


def restated_periods(c):
    return R.run_case(c, oversampler=oversampler)[1]


def test_restatement_equals_the_references_recorded_outputs(recorded, restated):
    assert len(recorded) >= 100
    for c, ((out, _, osc, sinus), (lo, _, _, _), (hi, _, _, _)) in zip(recorded, restated):
        assert R.same(out[~sinus], c["out"][~sinus]), c["name"]
        assert R.inside(c["out"], out, lo, hi)[sinus].all(), c["name"]
        assert np.array_equal(osc.words(), c["words"]), (c["name"], [R.WORDS[i] for i in np.nonzero(osc.words() != c["words"])[0]])
        assert osc.double_writes == 0, c["name"]
        assert R.same(restated_periods(c), c["periods"]), c["name"]


def test_recorded_sinusoids_obey_the_interval_rule(recorded, restated):
    """glibc's sinf against S*: within the interval everywhere, and not equal everywhere (else the rule would be idle)."""
    seen = differ = 0
    for c, ((out, _, _, sinus), (lo, _, _, _), (hi, _, _, _)) in zip(recorded, restated):
        if not sinus.any():
            continue
        assert R.inside(c["out"], out, lo, hi)[sinus].all(), c["name"]
        seen += int(sinus.sum())
        differ += int(np.count_nonzero(R.bits(out)[sinus] != R.bits(c["out"])[sinus]))
        if "plain" in c["name"] and c["name"].startswith(("sine", "cosine")):   # amplitude 1, DC 0: within one ulp of S*
            star = out.astype(np.float64)
            assert np.all(np.abs(c["out"].astype(np.float64) - star) <= np.spacing(np.abs(out)).astype(np.float64)), c["name"]
    assert seen > 20000 and 0 < differ < seen // 10


@pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE, "src", "main", "util")), reason="the reference tree is not here")
def test_the_generator_still_makes_the_recorded_cases(recorded):
    cs, src, got, keys, names = gen.run_reference(REFERENCE)
    assert [c["name"] for c in cs] == [c["name"] for c in recorded]
    for m, g, c in zip(cs, got, recorded):
        assert np.array_equal(m["ops"], c["ops"]) and np.array_equal(R.bits(src), R.bits(c["src"])), m["name"]
        assert R.same(g["out"], c["out"]) and np.array_equal(g["words"], c["words"]) and R.same(g["periods"], c["periods"]), m["name"]
    gen.check_branches(cs, src, got)
    assert keys["sinsize"] == ["4"]                                         # :372 resolves to the float overload of sin
    golden = os.path.join(ROOT, "tests", "golden")
    stored = json.load(open(os.path.join(golden, "oscillator_dump_keys.json")))
    assert stored["keys"] == keys["oscillator"] and [str(stored["sizeof"])] == keys["sizeof"][:1]
    assert json.load(open(os.path.join(golden, "oscillator_public_names.json"))) == names


def test_the_committed_operation_lists_are_the_generators(recorded):
    made, src = gen.cases(), gen.source_row()
    assert [m["name"] for m in made] == [c["name"] for c in recorded]
    for m, c in zip(made, recorded):
        assert np.array_equal(m["ops"], c["ops"]) and np.array_equal(R.bits(src), R.bits(c["src"])), m["name"]


def test_recorded_cases_cover_what_the_issue_lists(recorded, restated):
    fns, calls, whats, bits, modes, refs = set(), set(), set(), set(), set(), set()
    for c in recorded:
        assert c["out"].size == 1100
        for what, a, b, _ in c["ops"].tolist():
            whats.add(int(what))
            if what in R.PROCESS_OPS:
                calls.add(int(a))
            sets = {R.SET_FUNCTION: fns, R.SET_BITS: bits, R.SET_OVER_MODE: modes, R.SET_DC_REFERENCE: refs}
            if int(what) in sets:
                sets[int(what)].add(int(a))
    assert fns == set(range(14)) and calls >= {1100, 1, 7, 256, 1023} and bits >= {32, 24, 8} and refs == {0, 1}
    assert {R.times_of(m) for m in modes} == {1, 2, 3, 4, 6, 8}
    assert whats >= set(R.PROCESS_OPS) | {R.SET_PHASE, R.SET_FREQUENCY, R.SET_AMPLITUDE, R.SET_DC_OFFSET, R.RESET_PHASE,
                                         R.SET_SQUARED_INVERSION, R.SET_PARABOLIC_INVERSION, R.SET_DUTY, R.SET_WIDTH, R.SET_TRAPEZOID,
                                         R.SET_PULSETRAIN, R.SET_PARABOLIC_WIDTH}
    # get_periods for a plain and a BL function, behind skipped periods (the calls the reference defines: one fill, no refill)
    asked = {(int(op[1]), int(op[2]), int(op[3])) for c in recorded for op in c["ops"] if int(op[0]) == R.GET_PERIODS}
    assert asked == {(3, 5, 64), (2, 4, 50), (1, 1, 17)} and all(gen.single_fill(48000.0 / 1000.5, *a) for a in asked)
    assert not gen.single_fill(48000.0 / 1000.5, 2, 0, 100), "a call without skipped periods refills: undefined in the reference"
    with_periods = [c["name"] for c in recorded if c["periods"].size]
    assert any(n.startswith("BL") for n in with_periods) and any(not n.startswith("BL") for n in with_periods)
    assert all(c["periods"].size in (0, 131) and np.isfinite(c["periods"]).all() for c in recorded)
    by = {c["name"]: (c, r[0][2]) for c, r in zip(recorded, restated)}
    c, osc = by["sawtooth width 1 at phase == mask"]        # +-Inf coefficients, NaN at phase == mask
    assert np.isinf(osc.saw_coeffs[2]) and np.isinf(osc.saw_coeffs[3]) and np.isnan(c["out"][:301]).all() and np.isfinite(c["out"][301:]).all()
    c, osc = by["sine wraps 32 bits"]
    assert osc.freq_word * 2 > 1 << 32
    c, osc = by["sawtooth, 8 bits"]
    assert osc.mask == 255 and osc.freq_word * 6 > 256                      # wraps within a few samples
    c, osc = by["sine frequency 0"]
    assert osc.freq_word == 0 and len(set(R.bits(c["out"]).tolist())) == 1
    for name, lo, hi in (("rectangular duty", 0, 1), ("sawtooth width", 0, 1), ("parabolic width", 0, 1)):
        vals = {float(n.split()[2]) for n in by if n.startswith(name + " ") and len(n.split()) == 3}
        assert {0.0, 1.0} <= vals and any(0 < v < 1 for v in vals), name
    c, _ = by["rectangular amplitude 0 mul without a source"]               # 0.0f * -2.0f: the sign of a zero
    assert (R.bits(c["out"]) == 0x80000000).all()
    c, _ = by["sawtooth add without a source"]
    assert not (R.bits(c["out"]) == 0x80000000).any()
    src = recorded[0]["src"]
    assert np.isnan(src).any() and np.isinf(src).any() and (R.bits(src) == 0x80000000).any() and (R.bits(src) == 0).any()
    for name in ("sawtooth add in place", "sine mul in place", "BL pulsetrain mul", "oversampler mode changed on the way",
                 "bits changed on the way", "reset_phase_accumulator on the way", "phase beyond a turn and negative"):
        assert name in by, name


@pytest.mark.parametrize("bits", [32, 24, 8])
def test_closed_form_phase_is_the_serial_accumulator(bits):
    mask = (1 << bits) - 1
    rng = np.random.default_rng(bits)
    for w in (0, 1, mask, (mask >> 1) + 1, int(rng.integers(0, 1 << 32)) & mask, 0xFFFFFFF1 & mask, 89543210 & mask):
        for p0 in (0, mask, int(rng.integers(0, 1 << 32)) & mask):
            for step in (w, w // 3, w // 8):                                # ... and the oversampled step
                serial, end = R.serial_phases(p0, step, mask, 3000)
                closed = R.closed_phases(p0, step, mask, 3001)
                assert np.array_equal(serial, closed[:3000]) and end == int(closed[3000]), (bits, w, p0, step)
                if step * 3000 > mask:
                    assert (np.diff(serial.astype(np.int64)) < 0).any(), "no wrap in this row"


def test_trapezoid_writes_one_value_per_sample_the_first_branch_that_holds(mi):
    """fFallRatio == 0: nPoints[1] == nPoints[2], and a phase exactly there satisfies :433 and :439."""
    o = R.Oscillator()
    o.set_sample_rate(48000)
    o.set_frequency(12000.0)                                # a word of 2^30: the phases are 0, 2^30, 2^31, 3 2^30
    o.set_function(R.FG_TRAPEZOID)
    o.set_trapezoid_ratios(0.5, 0.0)
    out = o.process(8)
    assert o.points[1] == o.points[2] == 1 << 31 and o.double_writes == 2
    ph = R.closed_phases(0, 1 << 30, 0xFFFFFFFF, 8)
    assert [[bool(b[i]) for b in o.trapezoid_branches(ph)] for i in (2,)] == [[False, True, False, True, False]]
    assert out.size == 8 and out[2] == f32(1) and out[6] == f32(1)                   # :434, amplitude + DC, and not :440
    assert out[3] == f32(-1)
    # the C-ABI's words put the two points on the same phase too (the kernel's branch order is held to this on the GPU)
    from importlib import import_module
    s = import_module(mi.__name__ + ".capi").OscillatorSettings()
    lib = mi.lib
    lib.mi_oscillator_settings_init(ctypes.byref(s))
    for setter, a, b in ((2, 48000.0, 0.0), (1, 12000.0, 0.0), (0, float(R.FG_TRAPEZOID), 0.0), (10, 0.5, 0.0)):
        assert lib.mi_oscillator_settings_set(ctypes.byref(s), setter, a, b) == 0
    assert lib.mi_oscillator_settings_update(ctypes.byref(s)) == 0
    assert list(s.points) == o.points and s.points[1] == s.points[2] == 1 << 31 and s.freq_word == 1 << 30
    assert [f32(v) for v in s.trap_coeffs][:2] == o.trap_coeffs[:2] and np.isinf(s.trap_coeffs[2]) and np.isinf(o.trap_coeffs[2])


def test_a_frequency_out_of_range_converts_through_int64(mi):
    assert R.to_u32(-1.0) == 0xFFFFFFFF and R.to_u32(-0.5) == 0 and R.to_u32(4294967296.0 + 7.9) == 7 and R.to_u32(float("nan")) == 0
    assert R.to_u32(1e30) == 0 and R.to_u32(-1e30) == 0 and R.to_u32(float("inf")) == 0 and R.to_u32(-(2.0 ** 40) - 3) == 0xFFFFFFFD
    for freq, word in ((-12000.0, 0xC0000000), (60000.0, 0x40000000), (float("nan"), 0), (3e38, 0)):
        o = R.Oscillator()
        o.set_sample_rate(48000)
        o.set_frequency(freq)
        o.update_settings()
        assert o.freq_word == word, freq
        # ... and the C-ABI's conversion is the same one, on every word it forms (here: phases far outside a turn, NaN and Inf)
        from importlib import import_module
        s = import_module(mi.__name__ + ".capi").OscillatorSettings()
        mi.lib.mi_oscillator_settings_init(ctypes.byref(s))
        for setter, a in ((2, 48000.0), (1, freq), (3, -1e30 if word else float("inf"))):
            mi.lib.mi_oscillator_settings_set(ctypes.byref(s), setter, a, 0.0)
        o.set_phase(-1e30 if word else float("inf"))
        o.update_settings()
        assert mi.lib.mi_oscillator_settings_update(ctypes.byref(s)) == 0
        assert (s.freq_word, s.init_word) == (o.freq_word, o.init_word) == (word, o.init_word), freq


def test_an_unset_sample_rate_is_size_t_minus_one_in_the_arithmetic(mi):
    o = R.Oscillator()
    o.set_frequency(1000.0)
    o.set_phase(1.0)
    o.update_settings()
    assert o.sample_rate == (1 << 64) - 1 and o.freq_word == 0          # 2^32 * 1000 / 1.8e19 truncates to 0
    from importlib import import_module
    s = import_module(mi.__name__ + ".capi").OscillatorSettings()
    mi.lib.mi_oscillator_settings_init(ctypes.byref(s))
    mi.lib.mi_oscillator_settings_set(ctypes.byref(s), 1, 1000.0, 0.0)
    mi.lib.mi_oscillator_settings_set(ctypes.byref(s), 3, 1.0, 0.0)
    assert mi.lib.mi_oscillator_settings_update(ctypes.byref(s)) == 0
    assert s.sample_rate == (1 << 64) - 1 and s.unset_rate_ok == 0 and np.array_equal(abi_words(s), o.words())


# ---- the C-ABI's settings arithmetic, no device ----------------------------------------------------------------------------
SETTER_OF = {R.SET_FUNCTION: 0, R.SET_FREQUENCY: 1, R.SET_SAMPLE_RATE: 2, R.SET_PHASE: 3, R.SET_BITS: 4, R.SET_DC_OFFSET: 5, R.SET_DC_REFERENCE: 6,
             R.SET_AMPLITUDE: 7, R.SET_DUTY: 8, R.SET_WIDTH: 9, R.SET_TRAPEZOID: 10, R.SET_PULSETRAIN: 11, R.SET_PARABOLIC_WIDTH: 12,
             R.SET_SQUARED_INVERSION: 13, R.SET_PARABOLIC_INVERSION: 14, R.SET_OVER_MODE: 15, R.RESET_PHASE: 16}


def abi_words(s):
    fb = lambda v: int(np.array([v], f32).view(u32)[0])     # noqa: E731
    return np.array([s.phase, s.mask, fb(s.acc2phase), s.freq_word, s.init_word, fb(s.referenced_dc), fb(s.sq_amplitude), fb(s.sq_wave_dc),
                     s.duty_word, fb(s.rect_wave_dc), fb(s.rect_atten), s.width_word] + [fb(v) for v in s.saw_coeffs] + [fb(s.saw_atten)] +
                    list(s.points) + [fb(v) for v in s.trap_coeffs] + [fb(s.trap_atten)] + list(s.train) +
                    [fb(s.pulse_wave_dc), fb(s.pulse_atten), fb(s.par_amplitude), s.par_word, fb(s.par_wave_dc), fb(s.par_atten),
                     s.oversampling, s.freq_word_over], u32)


def test_abi_settings_words_equal_the_restatements_on_every_recorded_case(mi, recorded):
    from importlib import import_module
    capi = import_module(mi.__name__ + ".capi")
    lib = mi.lib
    for c in recorded:
        s = capi.OscillatorSettings()
        assert lib.mi_oscillator_settings_init(ctypes.byref(s)) == 0
        o = R.Oscillator()
        for op in c["ops"]:
            what = int(op[0])
            if what in R.PROCESS_OPS or what == R.UPDATE:   # process_* call update_settings first; the phase then runs on
                assert lib.mi_oscillator_settings_update(ctypes.byref(s)) == 0
                o.update_settings()
                assert s.phase_known == 1 and s.phase == o.acc, c["name"]       # no device here: nothing has advanced it
            elif what == R.GET_PERIODS:                     # changes no setting and leaves the phase
                continue
            else:
                assert lib.mi_oscillator_settings_set(ctypes.byref(s), SETTER_OF[what], float(op[1]), float(op[2])) == 0
                R.apply(o, op)
            assert bool(s.sync) == o.sync, (c["name"], what)
        got, want = abi_words(s), o.words()
        assert np.array_equal(got, want), (c["name"], [R.WORDS[i] for i in np.nonzero(got != want)[0]])
        assert np.array_equal(got[1:], c["words"][1:]), c["name"]               # ... which are the reference's


def test_abi_settings_define_what_the_reference_does_not(mi):
    from importlib import import_module
    capi = import_module(mi.__name__ + ".capi")
    lib = mi.lib
    for freq, word in ((-12000.0, 0xC0000000), (60000.0, 0x40000000), (float("nan"), 0), (3e38, 0)):
        s = capi.OscillatorSettings()
        lib.mi_oscillator_settings_init(ctypes.byref(s))
        lib.mi_oscillator_settings_set(ctypes.byref(s), 2, 48000.0, 0.0)
        lib.mi_oscillator_settings_set(ctypes.byref(s), 1, freq, 0.0)
        assert lib.mi_oscillator_settings_update(ctypes.byref(s)) == 0 and s.freq_word == word, freq
    s = capi.OscillatorSettings()
    lib.mi_oscillator_settings_init(ctypes.byref(s))
    assert s.sample_rate == (1 << 64) - 1 and s.sync == 1 and s.bits == 32 and s.mask == 0 and s.duty == 0.5 and s.width == 1.0


def test_setters_clamp_and_refuse_as_the_reference_does(mi):
    from importlib import import_module
    capi = import_module(mi.__name__ + ".capi")
    lib = mi.lib
    s = capi.OscillatorSettings()
    lib.mi_oscillator_settings_init(ctypes.byref(s))
    o = R.Oscillator()
    tries = [(R.SET_DUTY, 1.5, 0), (R.SET_DUTY, -0.1, 0), (R.SET_DUTY, 1.0, 0), (R.SET_WIDTH, 7.0, 0), (R.SET_WIDTH, -1.0, 0), (R.SET_TRAPEZOID, 0.7, 0.9),
             (R.SET_TRAPEZOID, -1.0, -1.0), (R.SET_TRAPEZOID, 2.0, 2.0), (R.SET_PULSETRAIN, 3.0, -3.0), (R.SET_PARABOLIC_WIDTH, 1.5, 0),
             (R.SET_BITS, 33, 0), (R.SET_BITS, 0, 0), (R.SET_BITS, 12, 0), (R.SET_DC_OFFSET, -0.0, 0), (R.SET_PHASE, -0.0, 0)]
    for what, a, b in tries:
        assert lib.mi_oscillator_settings_set(ctypes.byref(s), SETTER_OF[what], a, b) == 0
        R.apply(o, (what, a, b, 0))
        got = (s.duty, s.width, s.raise_ratio, s.fall_ratio, s.pos_ratio, s.neg_ratio, s.par_width, s.bits)
        want = (o.duty, o.width, o.raise_ratio, o.fall_ratio, o.pos_ratio, o.neg_ratio, o.par_width, o.bits)
        assert [float(f32(v)) for v in got] == [float(v) for v in want], (what, a, b)
    assert np.signbit(f32(s.dc_offset)) == np.signbit(o.dc_offset) == False  # noqa: E712  -0 == 0: not stored
    # the sync flag: set_dc_offset leaves it alone, set_function always raises it
    lib.mi_oscillator_settings_update(ctypes.byref(s))
    lib.mi_oscillator_settings_set(ctypes.byref(s), SETTER_OF[R.SET_DC_OFFSET], 0.5, 0)
    assert s.sync == 0
    lib.mi_oscillator_settings_set(ctypes.byref(s), SETTER_OF[R.SET_FUNCTION], float(s.function), 0)
    assert s.sync == 1


def test_refusals_that_need_no_device(mi):
    from importlib import import_module
    capi = import_module(mi.__name__ + ".capi")
    lib, byref = mi.lib, ctypes.byref
    s = capi.OscillatorSettings()
    assert lib.mi_oscillator_settings_init(None) == -1 and lib.mi_oscillator_settings_update(None) == -1
    assert lib.mi_oscillator_settings_set(None, 0, 0.0, 0.0) == -1
    lib.mi_oscillator_settings_init(byref(s))
    for setter, a in ((0, 14.0), (0, -1.0), (0, 1.5), (6, 2.0), (15, 31.0), (4, 256.0), (2, -1.0), (17, 0.0), (99, 0.0)):
        assert lib.mi_oscillator_settings_set(byref(s), setter, a, 0.0) == -1, (setter, a)
    h, n, v = ctypes.c_void_p(), ctypes.c_int(), ctypes.c_float()
    assert lib.mi_oscillator_bank_create(None, 1) == -1
    assert lib.mi_oscillator_bank_create(byref(h), 0) == -1 and lib.mi_oscillator_bank_create(byref(h), 65536) == -1 and not h.value
    assert lib.mi_oscillator_bank_destroy(None) == 0
    assert lib.mi_oscillator_bank_set(None, 0, 0, 0.0, 0.0) == -5 and lib.mi_oscillator_bank_set_function(None, 0, 0) == -5
    assert lib.mi_oscillator_bank_set_frequency(None, 0, 1.0) == -5 and lib.mi_oscillator_bank_reset_phase_accumulator(None, 0) == -5
    assert lib.mi_oscillator_bank_needs_update(None, 0, byref(n)) == -5 and lib.mi_oscillator_bank_update_settings(None, None) == -5
    assert lib.mi_oscillator_bank_set_settings(None, 0, byref(s)) == -5
    assert lib.mi_oscillator_bank_get_settings(None, 0, byref(s)) == -5 and lib.mi_oscillator_bank_get_exact_frequency(None, 0, byref(v)) == -5
    assert lib.mi_oscillator_bank_get_exact_phase(None, 0, byref(v)) == -5
    assert lib.mi_oscillator_bank_process(None, None, None, 4, 4, 4, 0, None) == -5
    assert lib.mi_oscillator_bank_reserve(None, 4) == -5 and lib.mi_oscillator_bank_set_exact(None, 1) == -5
    assert lib.mi_oscillator_bank_get_state(None, 0, None, None) == -5 and lib.mi_oscillator_bank_set_state(None, 0, None, None) == -5
    assert lib.mi_oscillator_bank_synth_rows(None, None, None) == -5
    assert lib.mi_oscillator_bank_get_periods(None, 0, None, 1, 0, 4, None) == -5


def test_the_header_declares_the_banks_entries(mi):
    text = open(os.path.join(ROOT, "include", "mi_dspu.h")).read()
    declared = set(re.findall(r"\b(mi_oscillator_\w+)\s*\(", text))
    setters = ["set_" + n for n in mi.OscillatorBank.SETTERS]
    want = {"mi_oscillator_settings_" + n for n in ("init", "set", "update")} | {"mi_oscillator_bank_" + n for n in [
        "create", "destroy", "set", "reset_phase_accumulator", "needs_update", "update_settings", "get_settings", "set_settings", "get_exact_frequency",
        "get_exact_phase", "process", "reserve", "set_exact", "get_state", "set_state", "get_periods", "synth_rows"] + setters}
    assert declared == want
    for name in want:
        assert hasattr(mi.lib, name), name
    for text_of in ("first branch, in source order, that holds", "converts through int64_t", "never set refuses process with MI_ESTATE"):
        assert text_of in text, text_of


# ---- the C++ class -----------------------------------------------------------------------------------------------------------
PROBE = r'''
#define private public
#define protected public
#include <lsp-plug.in/dsp-units/util/Oscillator.h>
#undef private
#undef protected
#include <cstdio>
#include <cstdlib>
#include <cstring>
using namespace lsp::dspu;
struct keys: public IStateDumper
{
    int depth = 0;
    void note(const char *n) { if (depth == 0) printf(" %s", n); }
    void begin_object(const char *n, const void *, size_t) override { note(n); ++depth; }
    void begin_object(const void *, size_t) override    { ++depth; }
    void end_object() override                          { --depth; }
    void begin_array(const char *n, const void *, size_t) override { note(n); ++depth; }
    void begin_array(const void *, size_t) override     { ++depth; }
    void end_array() override                           { --depth; }
    void write(const char *n, const void *) override    { note(n); }
    void write(const char *n, bool) override            { note(n); }
    void write(const char *n, unsigned char) override   { note(n); }
    void write(const char *n, signed int) override      { note(n); }
    void write(const char *n, unsigned int) override    { note(n); }
    void write(const char *n, unsigned long) override   { note(n); }
    void write(const char *n, float) override           { note(n); }
    void writev(const char *n, const float *, size_t) override          { note(n); }
    void writev(const char *n, const unsigned int *, size_t) override   { note(n); }
};
int main()
{
    printf("sizeof %zu %zu\n", sizeof(Oscillator), sizeof(Oversampler));
    void *raw = malloc(sizeof(Oscillator));
    memset(raw, 0xa5, sizeof(Oscillator));
    Oscillator *o = reinterpret_cast<Oscillator *>(raw);
    o->construct();
    printf("fresh %d %g %g %g %d %zu %u %u %u %u %g %g %g %g %g %g %zu %d %d %d %d\n", int(o->enFunction), o->fAmplitude, o->fFrequency, o->fDCOffset,
           int(o->enDCReference), o->nSampleRate + 1, o->nPhaseAcc, unsigned(o->nPhaseAccBits), unsigned(o->nPhaseAccMaxBits), o->nPhaseAccMask,
           o->sRectangular.fDutyRatio, o->sSawtooth.fWidth, o->sTrapezoid.fRaiseRatio, o->sTrapezoid.fFallRatio, o->sParabolic.fAmplitude,
           o->sParabolic.fWidth, o->nOversampling, int(o->enOverMode), int(o->bSync), o->pData == NULL, o->vSynthBuffer == NULL);
    o->set_frequency(1000.0f);                  // the setters and update_settings() need no device
    o->set_sample_rate(48000);
    o->set_function(FG_SAWTOOTH);
    o->set_width(7.0f);
    o->set_duty_ratio(1.5f);
    o->set_trapezoid_ratios(0.7f, 0.9f);
    o->set_phase_accumulator_bits(24);
    o->update_settings();
    printf("words %u %u %u %g %g %g %d %zu %g\n", o->nPhaseAccMask, o->nFreqCtrlWord, o->sSawtooth.nWidthWord, o->sSawtooth.fWidth,
           o->sRectangular.fDutyRatio, o->sTrapezoid.fFallRatio, int(o->needs_update()), o->nOversampling, o->get_exact_frequency());
    float y[4] = { 9, 9, 9, 9 };
    o->process_overwrite(y, 4);                 // no bank yet: nothing happens
    printf("untouched %g %u\n", y[0], o->nPhaseAcc);
    printf("dump");
    keys k;
    o->dump(&k);
    printf("\n");
    o->destroy();
    free(raw);
    return 0;
}
'''


@pytest.fixture(scope="module")
def probe(mi, tmp_path_factory):
    d = tmp_path_factory.mktemp("oscillator_probe")
    src, exe = str(d / "osc_probe.cpp"), str(d / "osc_probe")
    with open(src, "w") as f:
        f.write(PROBE)
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-I" + os.path.join(PKG, "include"), "-I" + os.path.join(ROOT, "include"),
                           src, "-o", exe, "-L" + PKG, "-lmi_dspu", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.check_output([exe]).decode().splitlines()
    return {l.split()[0]: l.split()[1:] for l in out if l.strip()}


def test_mirror_size_and_fresh_object_are_the_references(probe):
    stored = json.load(open(os.path.join(ROOT, "tests", "golden", "oscillator_dump_keys.json")))
    assert probe["sizeof"] == [str(stored["sizeof"]), "168"] == ["608", "168"]
    assert probe["fresh"] == ["0", "1", "0", "0", "0", "0", "0", "32", "32", "0", "0.5", "1", "0.25", "0.25", "1", "0", "0", "0", "1", "1", "1"]
    o = R.Oscillator()
    for what, a, b in ((R.SET_FREQUENCY, 1000.0, 0), (R.SET_SAMPLE_RATE, 48000, 0), (R.SET_FUNCTION, R.FG_SAWTOOTH, 0), (R.SET_WIDTH, 7.0, 0),
                       (R.SET_DUTY, 1.5, 0), (R.SET_TRAPEZOID, 0.7, 0.9), (R.SET_BITS, 24, 0)):
        R.apply(o, (what, a, b, 0))
    o.update_settings()
    assert probe["words"] == [str(o.mask), str(o.freq_word), str(o.width_word), "1", "0.5", "%g" % o.fall_ratio, "0", "1", "%g" % o.get_exact_frequency()]
    assert probe["untouched"] == ["9", "0"]


def test_dump_writes_the_references_keys_in_order(probe):
    keys = json.load(open(os.path.join(ROOT, "tests", "golden", "oscillator_dump_keys.json")))
    assert len(keys["keys"]) == 30 and probe["dump"] == keys["keys"] and keys["closes"] == []


def test_mirror_declares_the_references_public_names():
    names = json.load(open(os.path.join(ROOT, "tests", "golden", "oscillator_public_names.json")))
    assert set(names) == {"util/Oscillator.h"}
    listed = names["util/Oscillator.h"]
    path = os.path.join(PKG, "include", "lsp-plug.in", "dsp-units", "util", "Oscillator.h")
    text = re.sub(r"//.*", "", open(path).read())
    assert len(listed) >= 30 and gen.public_names(path, "Oscillator") == listed
    for deleted in ("Oscillator(const Oscillator &) = delete", "Oscillator(Oscillator &&) = delete",
                    "operator = (const Oscillator &) = delete", "operator = (Oscillator &&) = delete"):
        assert deleted in text, deleted
    fields = json.load(open(os.path.join(ROOT, "tests", "golden", "oscillator_dump_keys.json")))["keys"]
    members = text[text.index("private:"):]                 # behind the nested structs, which have fields of the same names
    pos = [re.search(r"\b%s;" % n, members).start() for n in fields]
    assert pos == sorted(pos), "the fields are not in the reference's order"
    assert re.search(r"Oversampler\s+sOver;\s*Oversampler\s+sOverGetPeriods;", text), "the two oversamplers are embedded by value"


def test_mirror_exports_the_references_symbols(mi):
    out = subprocess.check_output(["nm", "-D", "--defined-only", "-C", mi.LIB_PATH]).decode()
    for sym in ("Oscillator()", "~Oscillator()", "construct()", "init()", "destroy()", "update_settings()", "set_phase(float)", "get_exact_phase() const",
                "set_dc_offset(float)", "set_dc_reference(lsp::dspu::dc_reference_t)", "set_squared_sinusoid_inversion(bool)",
                "set_parabolic_inversion(bool)", "set_duty_ratio(float)", "set_width(float)", "set_trapezoid_ratios(float, float)",
                "set_pulsetrain_ratios(float, float)", "set_parabolic_width(float)", "set_oversampler_mode(lsp::dspu::over_mode_t)",
                "set_amplitude(float)", "get_periods(float*, unsigned long, unsigned long, unsigned long)",
                "process_add(float*, float const*, unsigned long)", "process_mul(float*, float const*, unsigned long)",
                "process_overwrite(float*, unsigned long)", "dump(lsp::dspu::IStateDumper*) const",
                "do_process(lsp::dspu::Oversampler*, float*, unsigned long)"):
        assert re.search(r" T lsp::dspu::Oscillator::%s$" % re.escape(sym), out, re.M), sym
