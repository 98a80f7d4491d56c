"""tests/scaled_metergraph_ref.py, the numpy restatement of lsp::dspu::ScaledMeterGraph, against what the reference's own class
recorded into tests/golden/scaled_metergraph_ref_vectors.npz: every word of both rings, both heads, both samplers' fCurrent, nCount
and nPeriod after every operation, and every read() and level(), bit for bit.  No GPU.

Every quirk that the bank and the class keep is shown to matter: with it taken out of the restatement some recorded case differs.
The closed form of update_period()'s frame boundaries (csrc/scaled_metergraph_bank.h) is checked against the counted loop."""
import os
import sys

import numpy as np
import pytest

import scaled_metergraph_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_scaled_metergraph_vectors as gen  # noqa: E402

f32, u32 = np.float32, np.uint32
X, CASES = gen.load()


def test_the_stored_file_is_the_generators_case_list():
    want = gen.cases()
    assert [c["name"] for c in CASES] == [c["name"] for c in want]
    assert np.array_equal(X.view(u32), gen.rows().view(u32))
    for a, b in zip(CASES, want):
        assert all(a[k] == b[k] for k in ("frames", "subsampling", "max_period")) and np.array_equal(a["ops"], b["ops"]), a["name"]
    golden = os.path.dirname(gen.OUT)
    largest = max(os.path.getsize(os.path.join(golden, n)) for n in os.listdir(golden) if n != os.path.basename(gen.OUT))
    assert os.path.getsize(gen.OUT) <= largest


class Watched(M.ScaledMeterGraph):
    """Notes how every re-decimation was entered: (sHistory.nCount > 0, sFrames.nCount > 0, from period, to period, method,
    history words it folded)."""

    def __init__(self, *a):
        super().__init__(*a)
        self.seen = []

    def update_period(self):
        h, fr = self.history, self.frames
        before = (h.count > 0, fr.count > 0, fr.period, self.period, self.method)
        done = super().update_period()
        if done:
            sub = (fr.period * fr.frames + h.period - 1) // h.period
            self.seen.append(before + (np.array([h.buffer.read(sub - i) for i in range(sub)], f32), h.period, fr.frames))
        return done


def watched(c):
    g = Watched(c["frames"], c["subsampling"], c["max_period"])
    for code, row, off, n, value in c["ops"]:
        code, row, off, n = int(code), int(row), int(off), int(n)
        if code == M.SET_METHOD:
            g.set_method(n)
        elif code == M.SET_PERIOD:
            g.set_period(n)
        elif code == M.FILL:
            g.fill(value)
        elif code in (M.PROCESS, M.PROCESS_GAIN):
            g.process(X[row, off:off + n], value if code == M.PROCESS_GAIN else None)
        elif code == M.PROCESS_SINGLE:
            for v in X[row, off:off + n]:
                g.process_single(v)
    return g.seen


def test_the_cases_cover_what_they_must():
    codes = {int(op[0]) for c in CASES for op in c["ops"]}
    assert codes == set(range(8))
    assert {int(op[3]) for c in CASES for op in c["ops"] if int(op[0]) == M.SET_METHOD} >= set(range(5))
    assert {float(op[4]) for c in CASES for op in c["ops"] if int(op[0]) == M.PROCESS_GAIN} == {1.0, 0.5, -2.0, 0.0}
    assert {c["frames"] for c in CASES} == {1, 2, 16, 333}
    assert {c["subsampling"] for c in CASES} >= {1, 3, 4, 64}
    assert any(c["max_period"] == c["subsampling"] for c in CASES)
    # no case is one where the reference is undefined
    assert all(c["subsampling"] >= 1 and c["frames"] >= 1 and c["max_period"] >= c["subsampling"] for c in CASES)
    for c in CASES:
        target = 0
        for k, op in enumerate(c["ops"]):
            assert int(op[0]) not in (M.PROCESS, M.PROCESS_GAIN, M.PROCESS_SINGLE) or target != 0, c["name"]
            target = int(c["state"][k, -1])
    # periods: equal to the subsampling, multiples, no multiples; clamped below and above; the same again
    sets = [(c, int(op[3]), int(c["state"][k, -1])) for c in CASES for k, op in enumerate(c["ops"]) if int(op[0]) == M.SET_PERIOD]
    assert any(p == c["subsampling"] for c, p, t in sets) and any(p % c["subsampling"] == 0 and p > c["subsampling"] for c, p, t in sets)
    assert any(p % c["subsampling"] != 0 and c["subsampling"] < p < c["max_period"] for c, p, t in sets)
    assert any(p < c["subsampling"] and t == c["subsampling"] for c, p, t in sets) and any(p > c["max_period"] and t == c["max_period"] for c, p, t in sets)
    assert {(4, 7), (4, 10), (4, 64)} <= {(c["subsampling"], p) for c, p, t in sets}
    # how update_period() was entered, per method: history frame open; only the frames' frame open (the else if); both closed
    seen = [s for c in CASES for s in watched(c)]
    for m in range(5):
        mine = [s for s in seen if s[4] == m]
        assert any(s[0] for s in mine) and any(not s[0] and s[1] for s in mine) and any(not s[0] and not s[1] and s[2] != 0 for s in mine), m
        assert any(s[3] > s[2] > 0 for s in mine) and any(s[3] < s[2] for s in mine), m
    # the sentinel's cases: a SIGN method over words that are negative, -1.0f and -0.0f; an ABS method over negative words; NaN as
    # a group's first sub-sample and elsewhere
    for m in (M.SIGN_MAXIMUM, M.SIGN_MINIMUM):
        words = np.concatenate([s[5] for s in seen if s[4] == m])
        assert (words == -1.0).any() and (words.view(u32) == 0x80000000).any() and ((words < 0) & (words != -1.0)).any()
    for m in (M.ABS_MAXIMUM, M.ABS_MINIMUM, M.PEAK):
        assert any((s[5] < 0).any() for s in seen if s[4] == m), m
    first = later = 0
    for s in seen:
        hp_words = s[5]
        if np.isnan(hp_words).any():
            for a, b in M.group_bounds(s[6], s[3], s[7])[1]:
                first += bool(np.isnan(hp_words[a - 1]))
                later += bool(np.isnan(hp_words[a:b]).any())
    assert first and later
    # both rings overrun several times in one call
    assert any(int(op[0]) == M.PROCESS and int(op[3]) > 3 * gen.capacities(c)[0] * c["subsampling"] and
               int(op[3]) > 3 * gen.capacities(c)[1] * max(1, int(c["state"][k, -2])) for c in CASES for k, op in enumerate(c["ops"]))
    # read of 0, 1, frames and more than frames
    assert {int(op[3]) for c in CASES if c["name"] == "read and level" for op in c["ops"] if int(op[0]) == M.READ} == {0, 1, 16, 21}
    # the input rows
    nan = np.flatnonzero(np.isnan(X[gen.ROW_NAN]))
    assert (nan % 7 == 0).any() and (nan % 7 != 0).any() and (nan % 64 == 0).any() and (nan % 64 != 0).any()
    assert not np.isnan(X[[gen.ROW_RANDOM, gen.ROW_TIES, gen.ROW_SPECIAL, gen.ROW_SENTINEL]]).any()


@pytest.mark.parametrize("index", range(len(CASES)), ids=[c["name"].replace(" ", "_") for c in CASES])
def test_restatement_is_the_reference_in_every_bit(index):
    c = CASES[index]
    state, answers = M.run_case(X, c)
    assert state.shape == c["state"].shape
    bad = np.argwhere(state != c["state"])
    assert bad.size == 0, (c["name"], "operation %d, word %d of %d" % (bad[0][0], bad[0][1], state.shape[1]), c["ops"][bad[0][0]])
    assert np.array_equal(answers, c["answers"]), c["name"]


@pytest.mark.parametrize("quirk", ("carry", "push", "else_if", "sentinel", "reset"))
def test_every_quirk_matters(quirk):
    """With the quirk taken out of the restatement at least one recorded case comes out differently."""
    differ = []
    for c in CASES:
        state, answers = M.run_case(X, c, without=(quirk,))
        if not np.array_equal(state, c["state"]) or not np.array_equal(answers, c["answers"]):
            differ.append(c["name"])
            if len(differ) >= 3:
                break
    assert differ, quirk


def test_abs_maximum_carries_with_the_natural_sense():
    """:189: a frame that two calls share holds the LARGER of the two partial maxima, where MeterGraph's holds the smaller."""
    x = np.array([1.0, 3.0, 2.0, 0.5], f32)
    for cuts in ([4], [2, 2], [1, 3], [3, 1]):
        g = M.ScaledMeterGraph(2, 4, 4)
        g.set_period(4)
        g.process(np.zeros(4, f32))                                     # the first call re-decimates, which closes an open frame
        at = 0
        for n in cuts:
            g.process(x[at:at + n])
            at += n
        assert g.history.buffer.data[1] == 3.0 and g.frames.buffer.data[2] == 3.0 and g.history.buffer.head == 2, cuts


def test_the_single_sample_form_pushes_the_sample():
    g = M.ScaledMeterGraph(2, 4, 4)
    g.set_period(4)
    g.process(np.zeros(4, f32))                                         # the first call re-decimates, which closes an open frame
    for v in (5.0, -3.0, 1.0, -0.5):
        g.process_single(v)
    assert g.history.buffer.data[1] == 0.5 and g.history.current == 5.0       # :142: fabsf of the LAST sample, not fCurrent


def test_a_negative_sign_winner_counts_as_unset():
    g = M.ScaledMeterGraph(1, 1, 4)
    g.set_method(M.SIGN_MAXIMUM)
    g.set_period(1)
    g.process(np.array([-3.0, 0.5, -1.0, 0.25], f32))
    g.set_period(4)
    g.process(np.array([-9.0], f32))
    # the fold of 0.5 -1.0 0.25 -9.0: -1.0 wins over 0.5, is negative, so 0.25 replaces it; -9.0 wins
    assert g.frames.buffer.data[0] == -9.0 and g.frames.buffer.head == 1 and g.frames.current == -1.0 and g.frames.count == 0
    g.set_period(2)
    g.process(np.array([0.125], f32))
    assert list(g.frames.buffer.data[:1]) == [0.125]                            # 0.25 -9.0 | -9.0 0.125 -> the last frame: -9 unset, 0.125


@pytest.mark.parametrize("hp", range(1, 65))
def test_closed_form_group_boundaries_are_the_counted_loop(hp):
    for P in range(hp, 65):
        for frames in range(1, 9):
            sub, groups, left = M.group_bounds(hp, P, frames)
            csub, cgroups, ccount, start = M.counted_bounds(hp, P, frames)
            assert (sub, groups, left) == (csub, cgroups, ccount), (hp, P, frames)
            assert len(groups) == frames and start == sub + 1 and 0 <= left < hp


@pytest.mark.parametrize("hp,P,frames", ((32, 2400, 320), (32, 64, 320), (1, 4099, 333), (64, 65, 1000), (7, 4800, 640), (3, 1 << 20, 7),
                                         (48000, 48001, 50), (64, 64, 4096)))
def test_closed_form_group_boundaries_at_large_sizes(hp, P, frames):
    sub, groups, left = M.group_bounds(hp, P, frames)
    csub, cgroups, ccount, start = M.counted_bounds(hp, P, frames)
    assert (sub, groups, left) == (csub, cgroups, ccount) and len(groups) == frames and start == sub + 1 and 0 <= left < hp
