"""The restatement of DynamicFilters (oracle/dynamic_filters.py) and the product's host builders (mi.dynfilter_sections) against the
REFERENCE'S OWN DynamicFilters class: tests/golden/dynfilter_ref_*.npz, recorded from oracle/_ref/dynfilter_ref (DynamicFilters.cpp
compiled unmodified) by tests/golden/make_dynfilter_vectors.py.  No GPU.

What the recording pins is the class's own text: set_params' swap and transform of the second frequency, kf, the cascade builders of
every type, the groups of 8 / 4 / 2 / 1 and bClearMem.  The per-sample transform and the section arithmetic are stand-ins there
(oracle/ref_overlay/filters) and stay pinned by properties only.

Distances.  The restatement takes tan, exp, log, cos and sin from numpy, the reference from the C library; how far apart they were
when the files were written is in tests/dynfilter_reference.py (CASCADE_ULP_SEEN, PARAM_ULP_SEEN), and the bounds here are twice
that.  The types whose builders take nothing from libm (the pass filters, the notch and the amplifiers) are equal in every bit.
The product's host code calls the same C library as the reference's program, so it is held to the recorded bits."""
import os
import sys

import numpy as np
import pytest

import dynfilter_reference as R
from conftest import TOL
from oracle import dynamic_filters as df
from oracle import filter_design as fd

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_dynfilter_vectors as gv  # noqa: E402

f32 = np.float32
bits = R.bits
HAVE_REF = os.path.exists(gv.DF_REF) and os.path.exists(gv.DF_SAN)
CASCADE_ULP_SEEN, PARAM_ULP_SEEN, ulps, check, coef_tol = R.CASCADE_ULP_SEEN, R.PARAM_ULP_SEEN, R.ulps, R.check, R.coef_tol
NO_LIBM = ("AMPLIFIER", "LOPASS", "HIPASS", "NOTCH")       # builders of plain arithmetic (and sqrtf, which IEEE 754 rounds correctly)
SWAPPED = ("LADDERPASS", "LADDERREJ", "BANDPASS")


@pytest.fixture(scope="module")
def short():
    return [c for k in ("rlc", "bwc", "lrx") for c in R.load(k)]


@pytest.fixture(scope="module")
def streams():
    return R.load("streams")


def _fp(c, fid=0):
    """The parameters a filter was last given ahead of the first call."""
    return [e[3] for e in c["events"] if e[1] == R.SET_PARAMS and e[2] == fid and e[0] == 0][-1]


def test_stored_vectors_are_what_the_reference_gives_today():
    """Freshness: where the reference binary exists the generator runs again (the sanitizer run and the margin of the all-filters
    clear included) and must give the committed bytes."""
    if not HAVE_REF:
        pytest.skip("no oracle/_ref/dynfilter_ref: the reference tree is not on this machine")
    for which, data in gv.build_bytes().items():
        with open(R.FILES[which], "rb") as f:
            assert data == f.read(), "dynfilter_ref_%s.npz is stale: python tests/golden/make_dynfilter_vectors.py" % which


def test_stored_vectors_hold_every_branch_and_edge(short, streams):
    assert all(os.path.getsize(p) < 400 * 1000 for p in R.FILES.values())
    types = {t for t in range(1, len(fd.FILTER_TYPES)) if df.cascade_count(t, 1) > 0}
    assert len(types) == 54 and not any("ENVELOPE" in fd.FILTER_TYPES[t] for t in types)
    # short cases: every type at slopes 1, 2 and 3, 40 samples, the gains 1.0, below, above and 1e-3; the reference's groups
    assert {(_fp(c)[0], _fp(c)[1]) for c in short} == {(t, s) for t in types for s in (1, 2, 3)}
    sizes = set()
    for c in short:
        g = c["gain"]
        assert len(g) == 40 and c["calls"] == [(0, 0, 40)] and c["record"] == 1
        assert g[0] == 1.0 and f32(1e-3) in g and g.min() < 0.1 and g.max() > 10.0
        T, B, groups = R.cascades_of(c, 0)
        assert groups == R.group_sizes(df.cascade_count(_fp(c)[0], _fp(c)[1])), c["name"]
        sizes |= set(groups)
    assert sizes == {8, 4, 2, 1}
    # one stream per type: 600 samples in two calls, at the slope of tests/test_dynfilter_gpu.py::test_every_type_matches_the_oracle
    per_type = [c for c in streams if c["name"].startswith("stream")]
    assert {_fp(c, 1)[0] for c in per_type} == types and len(per_type) == 54
    for c in per_type:
        t, slope = _fp(c, 1)[:2]
        assert slope == (2 if df.cascade_count(t, 2) <= 16 else 1) and [call[2] for call in c["calls"]] == [257, 343]
    # six longer cases: 2148 samples through filter 0, 1 / 2 / 4 / 8 / 12 / 15 cascades, every event
    long_ = [c for c in streams if c["name"].startswith("long")]
    assert sorted(df.cascade_count(*_fp(c)[:2]) for c in long_) == [1, 2, 4, 8, 12, 15]
    seen = set()
    for c in long_:
        assert sum(call[2] for call in c["calls"] if call[0] == 0) == 2148
        if max(call[2] for call in c["calls"]) > R.BUF_SIZE:
            seen.add("a call across BUF_SIZE")
        if any(call[1] < 2048 < call[1] + call[2] for call in c["calls"] if call[0] == 0):
            seen.add("a call across a super-block of 2048")
        else:
            assert [call[2] for call in c["calls"] if call[0] == 0] == [1024, 1024, 100]
            seen.add("1024 + 1024 + 100")
        cur = {}
        for i, call in enumerate(c["calls"]):
            for before, kind, fid, fp in c["events"]:
                if before == i and kind == R.SET_PARAMS:
                    if i > 0:
                        seen.add("same type" if cur[fid][0] == fp[0] else "new type for filter %d" % fid)
                        if fp[3] < fp[2] and any(k in fd.FILTER_TYPES[fp[0]] for k in SWAPPED):
                            got = R.fp_tuple(c["params"][i])
                            assert got[2] == f32(fp[3])                      # the recorded fFreq is the lower of the two
                            seen.add("swap")
                    cur[fid] = fp
            if call[0] not in cur:
                at = sum(k[2] for k in c["calls"][:i])
                assert np.array_equal(bits(c["out"][at:at + call[2]]), bits(c["x"][call[1]:call[1] + call[2]]))
                seen.add("inactive filter copies")
    assert seen == {"a call across BUF_SIZE", "a call across a super-block of 2048", "1024 + 1024 + 100", "same type", "new type for filter 0", "new type for filter 1", "swap", "inactive filter copies"}, seen


def _restated(c, fid=0):
    o = df.DynamicFilters(c["filters"])
    o.set_sample_rate(c["sample_rate"])
    o.set_params(fid, *_fp(c, fid))
    o.set_filter_active(fid, True)
    return o


def test_restated_set_params_and_kf_are_the_references(short):
    """fFreq and fFreq2 of get_params() (swapped, transformed) and kf against the recorded ones: the matched types (a division and a
    constant) in every bit, the bilinear ones within twice the distance seen."""
    worst = 0
    for c in short:
        fp = _fp(c)
        o = _restated(c)
        p, want = o.get_params(0), R.fp_tuple(c["params"][0])
        assert (p["nType"], p["nSlope"]) == want[:2] and p["fGain"] == want[4] and p["fQuality"] == want[5]
        kf = o.kf(0)                                               # what coefficients() hands the transform
        d = int(max(ulps(p["fFreq"], want[2]).max(), ulps(p["fFreq2"], want[3]).max(), ulps(kf, c["kf"][0]).max()))
        if not (fp[0] & 1):
            assert d == 0, (c["name"], d)
        worst = max(worst, d)
        assert d <= 2 * PARAM_ULP_SEEN, (c["name"], d)
    print("set_params and kf: at most %d ulp from the recording (seen when written: %d)" % (worst, PARAM_ULP_SEEN))


def test_restated_cascades_are_the_references(short):
    """cascades() fed the RECORDED fFreq2 against the recorded cascades of all 40 samples."""
    worst, exact = {}, set()
    for c in short:
        fp = _fp(c)
        name = fd.FILTER_TYPES[fp[0]]
        T, B, _ = R.cascades_of(c, 0)
        with np.errstate(all="ignore"):
            oT, oB = df.cascades(fp[0], fp[1], R.fp_tuple(c["params"][0])[3], fp[5], c["gain"])
        assert oT.shape == T.shape, c["name"]
        worst[name] = max(worst.get(name, 0), int(ulps(oT, T).max()), int(ulps(oB, B).max()))
    exact = {n for n, d in worst.items() if d == 0}
    print("bit-equal: %s" % " ".join(sorted(exact)))
    print("cascades: at most %d ulp from the recording (seen when written: %d)" % (max(worst.values()), CASCADE_ULP_SEEN))
    assert {n for n in worst if any(k in n for k in NO_LIBM)} <= exact, sorted(set(worst) - exact)
    assert max(worst.values()) <= 2 * CASCADE_ULP_SEEN, {n: d for n, d in worst.items() if d > 2 * CASCADE_ULP_SEEN}


def _coefficients_close(name, got, want):
    """tests/test_dynfilter_gpu.py::check's coefficient distances, for a machine whose libm is not the recording's: one part in 1e6
    of a section's coefficients for the bilinear types, 1e-3 of its numerator for matched-Z."""
    g, w = got.astype(np.float64), want.astype(np.float64)
    scale = np.abs(w).max(axis=-1, keepdims=True)
    if "_MT_" not in name:
        return bool(np.all(np.abs(g - w) <= 1e-6 * scale))
    num = np.abs(w[..., :3]).max(axis=-1, keepdims=True)
    return bool(np.all(np.abs(g[..., :3] - w[..., :3]) <= 1e-3 * num) and np.all(np.abs(g[..., 3:] - w[..., 3:]) <= 1e-6 * scale))


def test_recorded_sections_are_the_transform_of_the_recorded_cascades(short):
    """The sections recorded beside the cascades are the stand-in transform of them: for the bilinear types, plain float arithmetic,
    oracle/dynamic_filters.py's bilinear gives them in every bit; for matched-Z (expf and cosf of two libms) its matched is near."""
    for c in short:
        fp = _fp(c)
        T, B, _ = R.cascades_of(c, 0)
        with np.errstate(all="ignore"):
            mine = df.bilinear(T, B, c["kf"][0]) if fp[0] & 1 else df.matched(T, B, R.fp_tuple(c["params"][0])[2], c["kf"][0])
        if fp[0] & 1:
            assert np.array_equal(bits(mine), bits(R.sections_of(c, 0))), c["name"]
        else:
            assert _coefficients_close(fd.FILTER_TYPES[fp[0]], mine, R.sections_of(c, 0)), c["name"]


def test_product_builders_give_the_references_sections(mi, short):
    """mi.dynfilter_sections (the product's C++ set_params, kf, builders and transform) at every recorded gain against the RECORDED
    sections: what the reference's own builders made, through the stand-in transform, in the reference's program.  Bilinear and
    matched-Z alike: every case in every bit on the recording machine, three quarters of each elsewhere, and a case that is not
    within check's coefficient distance."""
    direct, total = {0: 0, 1: 0}, {0: 0, 1: 0}
    for c in short:
        fp = _fp(c)
        name = fd.FILTER_TYPES[fp[0]]
        want = R.sections_of(c, 0)
        got = np.stack([mi.dynfilter_sections(fp[0], fp[1], float(fp[2]), float(fp[3]), float(fp[5]), float(g), c["sample_rate"]) for g in c["gain"]], 1)
        assert got.shape == want.shape, c["name"]
        same = np.array_equal(bits(got), bits(want))
        total[fp[0] & 1] += 1
        direct[fp[0] & 1] += int(same)
        assert same or _coefficients_close(name, got, want), c["name"]
    for kind, what in ((1, "bilinear"), (0, "matched-Z")):
        print("mi.dynfilter_sections: %d of %d %s cases bit-equal to the recorded sections" % (direct[kind], total[kind], what))
        assert total[kind] == 81
        if HAVE_REF:
            assert direct[kind] == total[kind], what                  # same machine, same libm as the recording
        assert 4 * direct[kind] >= 3 * total[kind], what


def test_restated_process_gives_the_recorded_streams(streams):
    """oracle.dynamic_filters.DynamicFilters.process over every recorded stream and the six longer cases, events included, under
    check's rule; and the all-filters clear is visible: without it the other filter's next call is more than 100 x TOL away."""
    for c in streams + R.load("rlc")[:6]:
        y, y64 = R.replay(c, df, exact=True)
        check(y, c["out"], y64, c["name"], coef_tol(c))
    for c in streams:
        if c["name"].startswith("long"):
            keep, new, other = R.long_boundaries(c)
            assert R.margin(c, df, keep, clear_at=keep) > 100 * TOL and R.margin(c, df, other, no_clear_at=new) > 100 * TOL, c["name"]
