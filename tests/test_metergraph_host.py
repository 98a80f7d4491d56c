"""tests/metergraph_ref.py, the numpy restatement of lsp::dspu::MeterGraph, against what the reference's own class recorded into
tests/golden/metergraph_ref_vectors.npz: every ring word, nHead, fCurrent and nCount after every operation, and every read() and
level(), bit for bit.  No GPU.

The restatement also shows what a test may and may not rest on: for finite input the rings do not depend on how a stream is cut,
except with MM_ABS_MAXIMUM, whose block form folds a partial frame with > where the single-sample form has <."""
import os
import sys

import numpy as np
import pytest

import metergraph_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_metergraph_vectors as gen  # noqa: E402

f32, u32 = np.float32, np.uint32
X, CASES = gen.load()


def test_the_stored_file_is_the_generators_case_list():
    want = gen.cases()
    assert [c["name"] for c in CASES] == [c["name"] for c in want]
    assert np.array_equal(X.view(u32), gen.rows().view(u32))
    for a, b in zip(CASES, want):
        assert a["frames"] == b["frames"] and a["period"] == b["period"] and np.array_equal(a["ops"], b["ops"]), a["name"]
    assert os.path.getsize(gen.OUT) < 400 * 1000


def test_the_cases_cover_what_they_must():
    codes = {int(op[0]) for c in CASES for op in c["ops"]}
    assert codes == set(range(10))
    assert {int(op[3]) for c in CASES for op in c["ops"] if int(op[0]) == M.SET_METHOD} >= set(range(5))
    assert {float(op[4]) for c in CASES for op in c["ops"] if int(op[0]) == M.PROCESS_GAIN} == {1.0, 0.5, -2.0, 0.0}
    assert {c["frames"] for c in CASES} == {1, 2, 16, 333}
    assert {int(op[3]) for c in CASES if c["name"] == "read and level" for op in c["ops"] if int(op[0]) == M.READ} == {0, 1, 16, 21}
    # nCount == nPeriod and nCount > nPeriod at a set_period, seen in the recorded nCount
    eq = gt = 0
    for c in CASES:
        for k, op in enumerate(c["ops"]):
            if int(op[0]) == M.SET_PERIOD:
                count = int(c["state"][k, -1])
                eq += count == int(op[3]) and count != 0
                gt += count > int(op[3])
    assert eq >= 5 and gt >= 5
    # a ring overrun several times in one call
    assert any(int(op[0]) == M.PROCESS and int(op[3]) // c["period"] > 3 * c["frames"] for c in CASES for op in c["ops"])
    # the input rows: NaN in first and in later place of a chunk, Inf, subnormals, zeros of both signs
    nan = np.flatnonzero(np.isnan(X[gen.ROW_NAN]))
    assert (nan % 7 == 0).any() and (nan % 7 != 0).any() and (nan % 64 == 0).any() and (nan % 64 != 0).any()
    sp = X[gen.ROW_SPECIAL]
    assert np.isinf(sp).sum() == 2 and ((sp != 0) & (np.abs(sp) < 1e-38)).any() and (sp.view(u32) == 0x80000000).any() and (sp.view(u32) == 0).any()
    assert not np.isnan(X[[gen.ROW_RANDOM, gen.ROW_TIES, gen.ROW_SPECIAL]]).any()


@pytest.mark.parametrize("index", range(len(CASES)), ids=[c["name"].replace(" ", "_") for c in CASES])
def test_restatement_is_the_reference_in_every_bit(index):
    c = CASES[index]
    state, answers = M.run_case(X, c)
    assert state.shape == c["state"].shape
    bad = np.argwhere(state != c["state"])
    assert bad.size == 0, (c["name"], "operation %d, word %d of %d" % (bad[0][0], bad[0][1], state.shape[1]), c["ops"][bad[0][0]])
    assert np.array_equal(answers, c["answers"]), c["name"]


def test_primitives_first_of_equals_and_nan():
    a = np.array([1.0, -2.0, 2.0, -2.0, 0.5, -0.5], f32)
    assert M.sign_max(a) == -2.0 and M.abs_max(a) == 2.0
    assert M.sign_min(a).view(u32) == f32(0.5).view(u32) and M.abs_min(a) == 0.5
    assert M.sign_min(np.array([-0.0, 0.0], f32)).view(u32) == 0x80000000 and M.abs_min(np.array([-0.0, 0.0], f32)).view(u32) == 0
    n = np.array([np.nan, 5.0, -7.0], f32)
    for fn in (M.abs_max, M.abs_min, M.sign_max, M.sign_min):
        assert np.isnan(fn(n)), fn.__name__                           # in first place it is the result
    m = np.array([1.0, np.nan, -7.0, np.nan, 0.25], f32)
    assert M.abs_max(m) == 7.0 and M.sign_max(m) == -7.0 and M.abs_min(m) == 0.25 and M.sign_min(m) == 0.25   # elsewhere it is ignored
    for fn in (M.abs_max, M.abs_min, M.sign_max, M.sign_min):
        assert fn(np.zeros(0, f32)) == 0.0


def _rings(method, x, cuts, period=20, frames=16, gain=None):
    g = M.MeterGraph(frames, period)
    g.set_method(method)
    at = 0
    for n in cuts:
        g.process(x[at:at + n], gain)
        at += n
    return g.state_words()


CUTS = ([520], [1] * 520, [7] * 74 + [2], [256, 256, 8], [19, 1, 20, 21, 459])


@pytest.mark.parametrize("method", (M.ABS_MINIMUM, M.SIGN_MAXIMUM, M.SIGN_MINIMUM, M.PEAK))
@pytest.mark.parametrize("row", (gen.ROW_RANDOM, gen.ROW_TIES, gen.ROW_SPECIAL))
def test_rings_do_not_depend_on_the_cut_for_finite_input(method, row):
    for gain in (None, 0.5):
        want = _rings(method, X[row], CUTS[0], gain=gain)
        for cuts in CUTS[1:]:
            assert np.array_equal(_rings(method, X[row], cuts, gain=gain), want), (method, row, cuts[:3])


def test_a_negative_gain_makes_abs_minimum_depend_on_the_cut():
    """:210: the chunk's minimum times a negative gain is compared as it is, fCurrent > sample, so an open frame takes the chunk
    of the LARGER magnitude: with a gain below 0 MM_ABS_MINIMUM is cut-dependent too (the sign methods compare magnitudes)."""
    x = np.array([1.0, 3.0, 2.0, 0.5], f32)
    whole = _rings(M.ABS_MINIMUM, x, [4], period=4, frames=2, gain=-2.0)
    halves = _rings(M.ABS_MINIMUM, x, [2, 2], period=4, frames=2, gain=-2.0)
    assert whole[0] == f32(-1.0).view(u32) and halves[0] == f32(-2.0).view(u32)


def test_abs_maximum_depends_on_the_cut():
    """MeterGraph.cpp:158: the block form folds the open frame with fCurrent > sample: a frame that two calls share holds the
    smaller of the two partial maxima."""
    x = np.array([1.0, 3.0, 2.0, 0.5], f32)
    whole = _rings(M.ABS_MAXIMUM, x, [4], period=4, frames=2)
    halves = _rings(M.ABS_MAXIMUM, x, [2, 2], period=4, frames=2)
    assert whole[0] == f32(3.0).view(u32) and halves[0] == f32(2.0).view(u32)
    assert any(not np.array_equal(_rings(M.ABS_MAXIMUM, X[gen.ROW_RANDOM], cuts), _rings(M.ABS_MAXIMUM, X[gen.ROW_RANDOM], CUTS[0])) for cuts in CUTS[1:])
    # ... while calls that end on frame boundaries agree with one call
    assert np.array_equal(_rings(M.ABS_MAXIMUM, X[gen.ROW_RANDOM], [20] * 26), _rings(M.ABS_MAXIMUM, X[gen.ROW_RANDOM], [520]))
    # the single-sample form has < (:99): there the frame holds the maximum
    g = M.MeterGraph(2, 4)
    for v in x:
        g.process_single(v)
    assert g.buffer.data[0] == 3.0


def test_chunk_length_is_uint32_arithmetic():
    g = M.MeterGraph(4, 10)
    g.process(np.arange(1, 8, dtype=f32))
    g.set_period(7)                                                 # nCount == nPeriod: a frame before any sample is read
    g.process(np.array([9.0], f32))
    assert g.buffer.data[0] == 7.0 and g.buffer.head == 1 and g.count == 1 and g.current == 9.0
    g.set_period(10)
    g.process(np.arange(1, 6, dtype=f32))
    g.set_period(3)                                                 # nCount > nPeriod: the rest of the call is one chunk
    g.process(np.arange(20, 40, dtype=f32))
    assert g.buffer.head == 2 and g.count == 0
    with pytest.raises(AssertionError):
        M.MeterGraph(4, 0)
