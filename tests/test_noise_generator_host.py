"""The NoiseGenerator restatement against the reference's recordings (tests/golden/noise_generator_ref_vectors.npz), no device: every
sample, every state word of the three sources, the colour filter's members and sections and the chart, bit for bit (exponential
and Gaussian samples by the interval rule of noise_ref.py); and the recordings cover what they are there for."""
import os
import sys

import numpy as np
import pytest

import noise_ref as R
import velvet_ref as V
import noise_generator_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_noise_generator_vectors as gen  # noqa: E402

f32, u32 = np.float32, np.uint32


@pytest.fixture(scope="module")
def recorded():
    return [c for c in gen.load() if int(c["ops"][0][0]) >= G.G_OVER]


@pytest.fixture(scope="module")
def restated(recorded):
    return [G.run_case(c) for c in recorded]


def neighbours(c, trans):
    if not trans.any():
        return []
    return [G.run_case(c, fn)[0] for fn in R.EXP_NEIGHBOURS + R.GAUSS_NEIGHBOURS]


def test_the_restatement_equals_the_recordings_bit_for_bit(recorded, restated):
    assert len(recorded) >= 80
    for c, (out, words, chains, chart, trans, _) in zip(recorded, restated):
        assert out.size == c["out"].size, c["name"]
        bad = R.agree(c["out"], out, out, neighbours(c, trans), trans)
        assert bad.size == 0, (c["name"], bad[:5], out[bad[:5]], c["out"][bad[:5]])
        assert np.array_equal(words, c["words"]), (c["name"], np.nonzero(words != c["words"])[0])
        assert G.same_sections(chains, c["chains"]), c["name"]
        assert R.same(chart, c["chart"]).all(), c["name"]


def test_the_recordings_cover_generators_colours_counts_and_setters(recorded):
    by = {c["name"]: c for c in recorded}
    src = recorded[0]["src"]
    for g in range(3):
        for color in range(6):
            c = by["generator %d colour %d" % (g, color)]
            assert c["out"].size == 1100 and (c["chains"].shape[0] != 0) == (color != G.WHITE), c["name"]
            assert np.array_equal(c["chart"][0::2], np.ones(G.CHART_F.size, f32)) == (color == G.WHITE), c["name"]
        for what in (G.G_OVER, G.G_ADD, G.G_MUL, G.G_ADD_IN, G.G_ADD_NULL):
            c = by["generator %d op %d counts" % (g, what)]
            assert [int(o[1]) for o in c["ops"] if int(o[0]) == what] == [1, 255, 256, 257, 331]
    # the third call of LCG, MLS, LCG goes on where the first stopped
    a, b = by["LCG, MLS, LCG"], by["LCG alone"]
    assert np.array_equal(a["out"][600:900], b["out"][300:600]) and not np.array_equal(a["out"][300:600], b["out"][300:600])
    assert np.array_equal(a["words"][:17], b["words"][:17])
    # Velvet: an add of 1100 with a source is five segments, with NULL it is one: the sources' states differ
    a, b = by["generator 2 add of 1100"], by["generator 2 add of 1100 with NULL"]
    assert not np.array_equal(a["words"][25:50], b["words"][25:50])
    a, b = by["generator 1 add of 1100"], by["generator 1 add of 1100 with NULL"]
    assert np.array_equal(a["words"][:17], b["words"][:17])        # ... and the LCG cannot tell
    # every setter, with and without its effect: the second identical call raises nothing (nUpdate is 0 at the end)
    seen = {int(o[0]) for c in recorded for o in c["ops"]}
    assert set(range(G.G_OVER, G.G_MUL_NULL + 1)) <= seen and set(range(G.G_INIT_VELVET, G.G_CHART + 1)) <= seen
    assert all(c["words"][G.UPDATE_AT] == 0 for c in recorded if "setter" in c["name"])
    # mul with NULL: zeros, nothing drawn
    c = by["mul with NULL between two calls"]
    assert not c["out"][300:700].any() and not np.signbit(c["out"][300:700]).any()
    # white keeps the colour filter's update_settings() pending
    c = by["colour white keeps the filter's update pending"]
    assert c["words"][G.TILT_AT + 9] == 1 and c["chains"].shape[0] == 0
    # special levels
    levels = {(float(c["ops"][i][1])) for c in recorded if "amplitude" in c["name"] for i in range(len(c["ops"])) if int(c["ops"][i][0]) == G.G_AMP}
    assert {0.0, -2.0, np.inf} <= levels
    assert any(np.signbit(c["ops"][i][1]) and c["ops"][i][1] == 0 for c in recorded for i in range(len(c["ops"])) if int(c["ops"][i][0]) in (G.G_AMP, G.G_OFF))
    assert src.size == 1100


def test_the_restatement_takes_the_default_branches_outside_the_enums():
    def run(generator, color):
        g = G.Generator()
        g.init(23, 5, 77, 99, 23, 0x2F)
        g.set_sample_rate(48000)
        g.set_generator(generator)
        g.set_noise_color(color)
        return g.process(G.G_OVER, None, 200)
    assert np.array_equal(run(7, 9), run(G.GEN_LCG, G.WHITE))
    assert not np.array_equal(run(G.GEN_LCG, G.PINK), run(G.GEN_LCG, G.WHITE))
    assert V.BUF_LIM_SIZE == 256
