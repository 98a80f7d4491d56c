"""The filter designer (the oracle's restatement and the product's C++ one) and the oracle's static recurrence against the REFERENCE'S
OWN Filter and FilterBank classes: tests/golden/filter_ref_designs.npz and filter_ref_streams.npz, recorded from oracle/_ref/filter_ref
(Filter.cpp and FilterBank.cpp compiled unmodified) by tests/golden/make_filter_vectors.py.  No GPU.

What the recording pins is what the reference's own text decides: the sections of every design, Filter::limit, how FilterBank::end
packs and when it clears, impulse_response()'s backup.  The arithmetic inside a section is a stand-in there (oracle/ref_overlay/
filters) and stays pinned by properties only (oracle/biquad_oracle.c's header)."""
import json
import os
import sys

import numpy as np
import pytest

import filter_reference as R
import oracle
from oracle import filter_design as fd

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_filter_vectors as gv  # noqa: E402

f32 = np.float32
bits = R.bits
HAVE_REF = os.path.exists(gv.FLT_REF) and os.path.exists(gv.FLT_SAN)


@pytest.fixture(scope="module")
def designs():
    return R.load_designs()


@pytest.fixture(scope="module")
def streams():
    return R.load_streams()


def test_stored_vectors_are_what_the_reference_gives_today():
    """Freshness: where the reference binary exists the generator runs again (the sanitizer run, the oracle replay and the
    kept-against-cleared margins included) and must give the committed bytes."""
    if not HAVE_REF:
        pytest.skip("no oracle/_ref/filter_ref: the reference tree is not on this machine")
    d, s = gv.build_bytes()
    with open(R.DESIGNS, "rb") as f:
        assert d == f.read(), "filter_ref_designs.npz is stale: python tests/golden/make_filter_vectors.py"
    with open(R.STREAMS, "rb") as f:
        assert s == f.read(), "filter_ref_streams.npz is stale: python tests/golden/make_filter_vectors.py"


def test_stored_vectors_hold_every_branch_and_edge(designs, streams):
    assert os.path.getsize(R.DESIGNS) < 400 * 1000 and os.path.getsize(R.STREAMS) < 400 * 1000
    # designs: every type at slopes 1-4, three settings at 48 kHz and one at 44.1 kHz; slope 8 in every family
    seen = {}
    for d in designs:
        seen.setdefault((d["fp"][0], d["fp"][1]), []).append(d["sample_rate"])
    for t in range(len(fd.FILTER_TYPES)):
        for slope in (1, 2, 3, 4):
            assert seen[(t, slope)].count(48000) >= 3 and seen[(t, slope)].count(44100) >= 1, (fd.FILTER_TYPES[t], slope)
    assert {gv.family(fd.FILTER_TYPES[t]) for (t, slope) in seen if slope == 8} >= {"RLC", "BWC", "LRX", "APO", "WEIGHTED", "AMPLIFIER"}
    # Filter::limit: a frequency above 0.49 sr, a negative one, slope 0 and slope 1000, each visible in get_params()
    lim = [(d["fp"], R.fp_tuple(d["limited"]), d["sample_rate"]) for d in designs]
    top = f32(0.49) * f32(48000)
    assert any(fp[2] > top and got[2] == top for fp, got, sr in lim if sr == 48000)
    assert any(fp[3] > top and got[3] == top for fp, got, sr in lim if sr == 48000)
    assert any(fp[2] < 0 and got[2] == 0 for fp, got, sr in lim) and any(fp[3] < 0 and got[3] == 0 for fp, got, sr in lim)
    assert any(fp[1] == 0 and got[1] == 1 for fp, got, sr in lim) and any(fp[1] == 1000 and got[1] == R.FILTER_CHAINS_MAX for fp, got, sr in lim)
    assert max(len(d["sections"]) for d in designs) == R.FILTER_CHAINS_MAX
    assert any(d["inactive"] for d in designs) and not all(d["inactive"] for d in designs)
    for fp, got, sr in lim:
        assert got == R.limit(sr, fp), (fp, got)
    # freq_chart: recorded for every APO design (all eleven types, both rates) and for no other; past half the sample rate too
    apo = {t for name, t in fd.T.items() if "_APO_" in name}
    assert len(apo) == 11 and all((d["chart"] is not None) == (d["fp"][0] in apo) for d in designs)
    charted = [d for d in designs if d["chart"] is not None]
    assert {d["fp"][0] for d in charted} == apo and {d["sample_rate"] for d in charted} == {44100, 48000}
    assert all(len(d["chart"]) == 16 and np.isfinite(d["chart"]).all() for d in charted)
    assert all(R.chart_frequencies(sr)[-1] > 0.5 * sr > R.chart_frequencies(sr)[-3] for sr in (44100, 48000))
    # streams
    assert 25 <= len(streams) <= 45 and max(len(c["x"]) for c in streams) <= 4200
    assert {c["shared"] for c in streams} == {0, 1, 2, 3}
    counts = {len(s) for c in streams for s in c["sections"]}
    assert counts >= {0, 1, 2, 3, 4, 7, 8, 9, 15}, counts
    kinds = set()
    for c in streams:
        own = c["shared"] == 0
        bounds = R.boundaries(c)
        cur = R.limit(c["sample_rate"], c["fp"])
        for i in range(1, len(c["calls"])):
            ups = [e for e in c["events"] if e[0] == i and e[1] == R.UPDATE]
            same_count = len(c["sections"][i]) == len(c["sections"][i - 1])
            if ups:
                new = R.limit(ups[-1][2], ups[-1][3])
                if len(ups) == 1:
                    changed = {k for k, (a, b) in zip(("type", "slope", "freq", "freq2", "gain", "q"), zip(cur, new)) if a != b}
                    if changed and changed <= {"gain", "freq", "q"} and len(changed) == 1:
                        assert not bounds[i][1]
                        kinds.add("only " + changed.pop())
                    if "type" in changed and same_count and new[0] != R.FLT_NONE:
                        assert bounds[i][1] == own
                        kinds.add("type, own" if own else "type, shared")
                    if changed == {"slope"}:
                        assert bounds[i][1] == (own or not same_count)
                        kinds.add("slope, count %s, %s" % ("kept" if same_count else "changed", "own" if own else "shared"))
                    if new[0] == R.FLT_NONE or cur[0] == R.FLT_NONE:
                        assert bounds[i][1]
                        kinds.add("to none" if new[0] == R.FLT_NONE else "from none")
                else:
                    kinds.add("two updates ahead of one call")
                cur = new
            if any(e[0] == i and e[1] == R.CLEAR for e in c["events"]):
                assert bounds[i][1]
                kinds.add("clear()")
            if any(e[0] == i and e[1] == R.IMPULSE for e in c["events"]):
                kinds.add("impulse response")
            if c["shared"] in (1, 2) and bounds[i][0]:
                kinds.add("neighbour, %s" % ("cleared" if bounds[i][1] else "kept"))
    assert kinds >= {"only gain", "only freq", "only q", "type, own", "type, shared", "slope, count kept, own", "slope, count kept, shared",
                     "slope, count changed, own", "slope, count changed, shared", "to none", "from none", "two updates ahead of one call",
                     "clear()", "impulse response", "neighbour, kept", "neighbour, cleared"}, kinds
    assert sum(len(c["irs"]) for c in streams) >= 2


def _distance_ok(name, got, want):
    """The coefficient distance the project allows between two libms (tests/test_dynfilter_gpu.py::check): one part in 1e6 of the
    design's coefficients for the bilinear and APO families; for matched-Z 1e-3 of a section's numerator."""
    if got.shape != want.shape or not np.array_equal(np.isfinite(got), np.isfinite(want)):
        return False
    ok = np.isfinite(want)
    g, w = np.where(ok, got, 0).astype(np.float64), np.where(ok, want, 0).astype(np.float64)
    scale = max(float(np.abs(w).max()), 1e-30) if w.size else 1.0
    if "_MT_" not in name:
        return bool(np.all(np.abs(g - w) <= 1e-6 * scale))
    num = np.abs(w[:, :3]).max(axis=1, keepdims=True)
    return bool(np.all(np.abs(g[:, :3] - w[:, :3]) <= 1e-3 * num) and np.all(np.abs(g[:, 3:] - w[:, 3:]) <= 1e-6 * scale))


def _hold(what, designs, design):
    direct = 0
    for d in designs:
        name = fd.FILTER_TYPES[d["fp"][0]]
        got = R.canon(design(d))
        if got.shape == d["sections"].shape and np.array_equal(bits(got), bits(d["sections"])):
            direct += 1
        else:
            assert _distance_ok(name, got, d["sections"]), (what, name, d["fp"], d["sample_rate"], got, d["sections"])
    print("%s: %d of %d recorded designs bit-equal to the reference's" % (what, direct, len(designs)))
    if HAVE_REF:
        assert direct == len(designs), (what, direct, len(designs))         # same machine, same libm as the recording
    assert 4 * direct >= 3 * len(designs), (what, direct, len(designs))


def _oracle_design(d):
    with np.errstate(all="ignore"):
        return fd.design(fd.Params(*d["fp"]), d["sample_rate"])[2]


def _product_design(mi):
    def design(d):
        fp = d["fp"]
        return mi.design_filter(fp[0], fp[1], float(fp[2]), float(fp[3]), float(fp[4]), float(fp[5]), sample_rate=d["sample_rate"])[2]
    return design


def test_restated_designer_gives_the_recorded_sections(designs):
    _hold("oracle.filter_design.design", designs, _oracle_design)


def test_product_designer_gives_the_recorded_sections(mi, designs):
    _hold("mi.design_filter", designs, _product_design(mi))


def test_designers_report_what_the_reference_reports(mi, designs):
    """inactive() and the section count, from the recorded data: a design is inactive exactly where its mode is FM_BYPASS."""
    for d in designs:
        with np.errstate(all="ignore"):
            mode = fd.design(fd.Params(*d["fp"]), d["sample_rate"])[0]
        fp = d["fp"]
        pmode = mi.design_filter(fp[0], fp[1], float(fp[2]), float(fp[3]), float(fp[4]), float(fp[5]), sample_rate=d["sample_rate"])[0]
        assert (mode == fd.FM_BYPASS) == bool(d["inactive"]) == (pmode == fd.FM_BYPASS), (fd.FILTER_TYPES[fp[0]], fp)
        assert d["latency"] == 0


def _charts_hold(what, designs, chart):
    """freq_chart of the APO designs (Filter.cpp:405-498 is the reference's own text for it) against the recorded charts: bit-equal on
    the recording machine, three quarters elsewhere, and never further than one part in 1e6 of the chart's largest magnitude."""
    charted = [d for d in designs if d["chart"] is not None]
    direct = 0
    for d in charted:
        got, want = np.asarray(chart(d), np.complex64), d["chart"]
        if np.array_equal(got.view(f32).view(np.uint32), want.view(f32).view(np.uint32)):
            direct += 1
        else:
            assert float(np.abs(got - want).max()) <= 1e-6 * float(np.abs(want).max()), (what, fd.FILTER_TYPES[d["fp"][0]], d["fp"])
    print("%s: %d of %d recorded APO charts bit-equal to the reference's" % (what, direct, len(charted)))
    if HAVE_REF:
        assert direct == len(charted), (what, direct, len(charted))
    assert 4 * direct >= 3 * len(charted), (what, direct, len(charted))


def test_restated_freq_chart_gives_the_recorded_apo_charts(designs):
    _charts_hold("oracle.filter_design.freq_chart", designs,
                 lambda d: fd.freq_chart(fd.Params(*d["fp"]), d["sample_rate"], R.chart_frequencies(d["sample_rate"]))[0])


def test_product_freq_chart_gives_the_recorded_apo_charts(mi, designs):
    def chart(d):
        fp = d["fp"]
        return mi.filter_freq_chart(R.chart_frequencies(d["sample_rate"]), fp[0], fp[1], float(fp[2]), float(fp[3]), float(fp[4]), float(fp[5]),
                                    sample_rate=d["sample_rate"])
    _charts_hold("mi.filter_freq_chart", designs, chart)


def test_full_grid_against_the_reference_binary(mi):
    """29 160 designs (81 types, slopes 1-5 and 8, 100 Hz to 23 kHz, gains 0.1 to 15.8, Q 0 to 3, three rates) through the reference
    binary, live: both designers give its sections in every bit.  Runs wherever oracle/_ref/filter_ref is."""
    if not HAVE_REF:
        pytest.skip("no oracle/_ref/filter_ref: the reference tree is not on this machine")
    grid = gv.grid()
    assert len(grid) == 29160
    cs = [R.design_case(sr, fp) for sr, fp in grid]
    res = R.parse_results(gv.run_driver(gv.FLT_REF, cs), cs)
    product = _product_design(mi)
    bad = []
    for (sr, fp), r in zip(grid, res):
        d = dict(fp=fp, sample_rate=sr)
        want = r["sections"][0]
        for what, got in (("oracle", R.canon(_oracle_design(d))), ("product", R.canon(product(d)))):
            if got.shape != want.shape or not np.array_equal(bits(got), bits(want)):
                bad.append((what, sr, fd.FILTER_TYPES[fp[0]], fp[1:]))
    assert not bad, (len(bad), bad[:10])


def test_oracle_recurrence_gives_the_recorded_streams(streams):
    """The oracle's static recurrence over the recorded sections with the clear / keep rule restated in filter_reference.boundaries
    gives the recorded output and impulse responses in every bit; with any rebuilt boundary decided the other way it does not."""
    for c in streams:
        out, irs = R.replay(c, oracle)
        assert np.array_equal(bits(out), bits(c["out"])), c["name"]
        assert len(irs) == len(c["irs"]) and all(np.array_equal(bits(a), bits(b)) for a, b in zip(irs, c["irs"])), c["name"]
        bounds = R.boundaries(c)
        for i in range(1, len(c["calls"])):
            if bounds[i][0] and len(c["sections"][i]) == len(c["sections"][i - 1]) and len(c["sections"][i]):
                assert gv.margin(c, oracle, i) > 100 * gv.TOL, (c["name"], i)


def test_designers_give_the_sections_of_every_stream_call(mi, streams):
    """The sections in force per call (both filters of a shared bank, in the bank's order) from both designers."""
    product = _product_design(mi)
    for c in streams:
        cur = c["fp"]
        for i in range(len(c["calls"])):
            for e in c["events"]:
                if e[0] == i and e[1] == R.UPDATE:
                    cur = e[3]
            mine = dict(fp=cur, sample_rate=c["sample_rate"])
            other = dict(fp=c["other"], sample_rate=c["sample_rate"])
            order = {0: [mine], 3: [mine], 1: [other, mine], 2: [mine, other]}[c["shared"]]
            for what, design in (("oracle", _oracle_design), ("product", product)):
                got = np.concatenate([design(d).reshape(-1, 5) for d in order])
                if HAVE_REF:
                    assert np.array_equal(bits(got), bits(c["sections"][i])), (what, c["name"], i)
                else:
                    assert _distance_ok(fd.FILTER_TYPES[cur[0]], got, c["sections"][i]), (what, c["name"], i)


def test_anchors_follow_from_the_recorded_file(designs, streams):
    """tests/golden/filter_anchors.json (two sections and eight impulse-response samples of one filter, recorded earlier by a probe
    and printed with nine digits) is what the reference binary gives for that filter today."""
    with open(os.path.join(R.GOLDEN, "filter_anchors.json")) as f:
        anchors = json.load(f)
    want = np.array(anchors["c1_hishelf_sections"], f32)
    fp = (fd.FLT_BT_BWC_HISHELF, 2, f32(1000.0), f32(1000.0), f32(gv.PLUS_6_DB), f32(0.0))
    hit = [d for d in designs if d["fp"] == fp and d["sample_rate"] == 48000]
    assert len(hit) == 1
    np.testing.assert_allclose(hit[0]["sections"], want, rtol=0, atol=3e-7)
    case = [c for c in streams if c["fp"] == fp and c["irs"]]
    assert len(case) == 1 and np.array_equal(bits(case[0]["sections"][0]), bits(hit[0]["sections"]))
    np.testing.assert_allclose(case[0]["irs"][0], np.array(anchors["c1_impulse_response_head"], f32), rtol=0, atol=3e-7)
