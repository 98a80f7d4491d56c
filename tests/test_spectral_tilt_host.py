"""The SpectralTilt designer and restatement against the reference's recordings (tests/golden/noise_generator_ref_vectors.npz), no device:
the restatement -- the library's host designer, the cascade of oracle/biquad_oracle.c, the process rules of noise_generator_ref.py --
gives the recorded samples, members, sections and charts bit for bit; the recordings cover what they are there for; the designer's
own entry points refuse what they must."""
import ctypes
import os
import sys

import numpy as np
import pytest

import noise_ref as R
import noise_generator_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_noise_generator_vectors as gen  # noqa: E402

f32, u32 = np.float32, np.uint32
EINVAL = -1


@pytest.fixture(scope="module")
def recorded():
    return [c for c in gen.load() if int(c["ops"][0][0]) < G.G_OVER]


@pytest.fixture(scope="module")
def restated(recorded):
    return [G.run_case(c) for c in recorded]


def test_the_restatement_equals_the_recordings_bit_for_bit(recorded, restated):
    assert len(recorded) >= 50
    for c, (out, words, chains, chart, _, _) in zip(recorded, restated):
        assert out.size == c["out"].size and R.same(out, c["out"]).all(), c["name"]
        assert np.array_equal(words, c["words"]), (c["name"], words[G.TILT_AT:G.TILT_AT + 11], c["words"][G.TILT_AT:G.TILT_AT + 11])
        assert R.same(chart, c["chart"]).all(), c["name"]


def test_the_designers_sections_equal_the_recorded_ones_bit_for_bit(recorded, restated):
    designed = 0
    for c, (_, _, chains, _, _, _) in zip(recorded, restated):
        assert G.same_sections(chains, c["chains"]), c["name"]
        designed += chains.shape[0] != 0
    assert designed >= 40


def by_name(recorded):
    return {c["name"]: c for c in recorded}


def test_the_recordings_cover_the_orders_slopes_norms_and_quirks(recorded):
    by = by_name(recorded)
    sections = {o: by["tilt order %d" % o]["chains"].shape[0] for o in (0, 1, 2, 7, 50, 128, 200)}
    assert sections == {0: 0, 1: 1, 2: 1, 7: 4, 50: 25, 128: 64, 200: 64}       # odd orders raised, clamped to 128
    assert by["tilt order 7"]["words"][G.TILT_AT] == 8 and by["tilt order 200"]["words"][G.TILT_AT] == 128
    src = by["tilt order 0"]["src"]
    assert np.isfinite(src).all() and not np.isfinite(by["tilt with a non-finite source"]["src"]).all()
    assert np.isnan(by["tilt with a non-finite source"]["out"][12:]).all()
    # the reference's own NaN designs: the gain at DC of a section whose numerator and denominator both vanish there, and the
    # sample rate of size_t(-1) that construct() leaves
    nan_designs = {"tilt with a non-finite source", "tilt norm 0 at 44100 Hz", "tilt norm 0 at 48000 Hz", "tilt as constructed"}
    assert {c["name"] for c in recorded if not np.isfinite(c["out"]).all()} == nan_designs
    assert np.array_equal(by["tilt order 0"]["out"][:600], src[:600])           # no section: a copy
    bypass = G.TILT_AT + 8
    for name in ("tilt slope 0 unit 0", "tilt slope -0.5 unit 3"):
        assert by[name]["words"][bypass] == 1 and np.array_equal(by[name]["out"][:400], src[:400]), name
    for name in ("tilt slope -3 unit 1", "tilt slope 10 unit 2", "tilt slope 0.5 unit 0"):
        assert by[name]["words"][bypass] == 0, name
    # all seven norms at three rates, and they differ where they should
    for rate in (44100, 48000, 30000):
        gains = {n: by["tilt norm %d at %d Hz" % (n, rate)]["chains"][0, 0] for n in range(7)}
        assert len({v.tobytes() for v in gains.values()}) >= 4, (rate, gains)      # the auto norm is one of the others by definition
    a, b = by["tilt norm 3 at 30000 Hz"], by["tilt norm 3 at 48000 Hz"]
    assert a["words"][G.TILT_AT + 6] == G.fbits(20000.0) and b["words"][G.TILT_AT + 6] == G.fbits(20000.0)
    # the range quirks: what was given the right way round is swapped, and update_settings() falls back to the defaults
    lower, upper = G.TILT_AT + 5, G.TILT_AT + 6
    w = by["tilt range the right way round"]["words"]
    assert (w[lower], w[upper]) == (G.fbits(0.1), G.fbits(20000.0))
    w = by["tilt range given backwards"]["words"]             # ... and what was given backwards is not swapped: the defaults again
    assert (w[lower], w[upper]) == (G.fbits(0.1), G.fbits(20000.0))
    assert by["tilt upper at Nyquist"]["words"][upper] == G.fbits(20000.0)
    assert by["tilt lower above Nyquist"]["words"][lower] == G.fbits(0.1)
    w = by["tilt lower above upper"]["words"]
    assert (w[lower], w[upper]) == (G.fbits(0.1), G.fbits(20000.0))
    # the stale chart of a bypassed tilt: the sections of the design before, not a flat response
    c = by["tilt bypass keeps the stale cascade"]
    assert c["words"][bypass] == 1 and c["chains"].shape[0] == 4 and not np.allclose(c["chart"][0::2], 1.0)
    # a re-design clears the memory: the samples behind it are those of a fresh filter on that stretch of the source
    c = by["tilt re-design in mid-stream"]
    t = G.Tilt()
    t.given = c["chains"]
    t.s.bypass, t.s.sync = 0, 0
    assert R.same(t.process(G.T_OVER, None, src[300:600], 300), c["out"][300:600]).all()
    ops = {int(o[0]) for c in recorded for o in c["ops"]}
    assert set(G.T_PROCESS) <= ops and {G.T_CHART, G.T_RANGE, G.T_NORM} <= ops
    assert {int(o[1]) for c in recorded for o in c["ops"] if int(o[0]) == G.T_CHART} == {0, 1}


def test_the_generator_script_still_makes_the_recorded_cases():
    reference = os.path.join(os.path.dirname(ROOT), "reference")
    if not os.path.isdir(os.path.join(reference, "src", "main", "noise")):
        pytest.skip("no reference tree beside the repository")
    cs, _, got = gen.run_reference(reference, sanitized=False)
    stored = gen.load()
    assert [c["name"] for c in cs] == [c["name"] for c in stored]
    for c, made, g in zip(stored, cs, got):
        assert np.array_equal(c["ops"], made["ops"]), c["name"]
        assert R.same(g["out"], c["out"]).all() and np.array_equal(g["words"], c["words"]), c["name"]
        assert G.same_sections(g["chains"], c["chains"]) and R.same(g["chart"], c["chart"]).all(), c["name"]


def test_the_setters_rules_and_the_refusals_that_need_no_device(mi):
    from importlib import import_module
    capi = import_module("lsp-dsp-units_amd.capi")
    lib = mi.lib
    t = G.Tilt()
    assert (t.s.order, t.s.sync, t.s.bypass, t.s.sample_rate) == (1, 1, 0, 2 ** 64 - 1) and t.s.norm == G.NORM_AUTO
    t.set_sample_rate(48000)
    t.update_settings()
    assert t.s.sync == 0 and t.s.order == 2 and t.s.n_sections == 1
    for call in (lambda: t.set_order(2), lambda: t.set_slope(0.5, G.NEPER), lambda: t.set_lower_frequency(0.1), lambda: t.set_upper_frequency(20000.0),
                 lambda: t.set_sample_rate(48000)):
        call()
        assert t.s.sync == 0                                # the value it has: nothing happens
    t.set_frequency_range(0.1, 20000.0)                     # swapped to (20000, 0.1): never what update_settings() leaves
    assert t.s.sync == 1 and (t.s.lower_frequency, t.s.upper_frequency) == (20000.0, f32(0.1))
    t.update_settings()
    assert (t.s.lower_frequency, t.s.upper_frequency) == (f32(0.1), 20000.0)
    t.set_norm(G.NORM_AUTO)
    assert t.s.sync == 1                                    # set_norm does not compare
    assert t.update_settings() is True                      # a new design, though nothing changed
    t.set_order(999)
    t.update_settings()
    assert t.s.order == 128 and t.s.n_sections == 64
    for fn, args in ((lib.mi_spectral_tilt_settings_init, (None,)), (lib.mi_spectral_tilt_settings_update, (None, None)),
                     (lib.mi_spectral_tilt_settings_set_order, (None, 2)), (lib.mi_spectral_tilt_settings_freq_chart, (None, None, None, None, None, 0))):
        assert fn(*args) == EINVAL
    f = np.zeros(4, f32)
    assert lib.mi_spectral_tilt_settings_freq_chart(ctypes.byref(t.s), None, None, None, f.ctypes.data_as(ctypes.c_void_p), 4) == EINVAL
    assert "NULL" in (lib.mi_dspu_last_error() or b"").decode()
    assert ctypes.sizeof(capi.SpectralTiltSettings) == 56 + 64 * 32
    # both chart forms give the same numbers
    re, im, c = np.zeros(4, f32), np.zeros(4, f32), np.zeros(8, f32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    f[:] = (20.0, 1000.0, 20000.0, 30000.0)
    assert lib.mi_spectral_tilt_settings_freq_chart(ctypes.byref(t.s), p(re), p(im), p(c), p(f), 4) == 0
    assert np.array_equal(c[0::2], re) and np.array_equal(c[1::2], im) and np.isfinite(c).all()
    if mi.device_count() <= 0:                              # no bank without a device: no quiet fall-back
        with pytest.raises(mi.MiError):
            mi.SpectralTiltBank(1)
        with pytest.raises(mi.MiError):
            mi.NoiseGeneratorBank(1)
