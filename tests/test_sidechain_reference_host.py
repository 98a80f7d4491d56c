"""The numpy restatement (sidechain_ref) and the host code of update_settings() (mi_sidechain_compute_params) against the
REFERENCE'S OWN Sidechain: Sidechain.cpp and RawRingBuffer.cpp compiled unmodified (oracle/Makefile -> oracle/_ref/sidechain_ref)
and run by tests/golden/make_sidechain_vectors.py, whose results are stored in tests/golden/sidechain_ref_vectors.npz.  A reading
of the reference that the restatement and the kernel share is caught here; tests/test_sidechain_reference_gpu.py holds the kernel
and the C++ class to the same file.

Not pinned by any of this: dsp::h_abs_sum / h_sqr_sum (the order of the refresh sums), dsp::ssqrt1 and the result type of a
mixed lsp_max, which the reference tree does not carry and oracle/ref_shim states by this project's reading."""
import os
import sys

import numpy as np
import pytest

import sidechain_ref as ref
import sidechain_reference as R

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_sidechain_vectors as gv  # noqa: E402

f32 = np.float32
bits = R.bits


@pytest.fixture(scope="module")
def data():
    return R.load()


@pytest.fixture(scope="module")
def restated(data):
    """Every case through the restatement fed the reference's recorded parameters: computed once."""
    return [R.replay(c, R.single_params(c) if c["single"] else R.recorded_params(c)) for c in data]


def test_stored_vectors_are_what_the_reference_gives_today():
    """Freshness: where the reference binary exists the generator runs again (the sanitizer run and the scalar preprocess()
    comparison included) and must give the committed bytes."""
    if not os.path.exists(gv.SC_REF):
        pytest.skip("no oracle/_ref/sidechain_ref: the reference tree is not on this machine")
    with open(gv.OUT, "rb") as f:
        assert gv.build_bytes() == f.read(), "sidechain_ref_vectors.npz is stale: python tests/golden/make_sidechain_vectors.py"


def test_stored_vectors_hold_every_branch_and_edge(data):
    assert os.path.getsize(R.PATH) < 400 * 1000
    by = {c["name"]: c for c in data}
    # at most a quarter of the cases depend on libm (fTau): the others are direct on any machine
    lpf = [c for c in data if c["lpf"]]
    assert 4 * len(lpf) <= len(data) and len(lpf) >= 8
    # four modes x one and two inputs x both stereo modes x six sources
    seen = {(c["mode"], c["inputs"], c["stereo"], c["source"]) for c in data}
    for mode in ref.MODES:
        assert (mode, 1, 0, ref.SCS_MIDDLE) in seen
        assert all((mode, 2, st, s) in seen for st in (0, 1) for s in ref.SOURCES)
    gains = {float(c["gain"]) for c in data} | {float(a) for c in data for _, s, a in c["events"] if s == "set_gain"}
    assert {1.0, -1.5, 0.0} <= gains
    windows = {int(v) for c in data for v in R.column(c, "reactivity")}
    assert {1, 2, 457, 480} <= windows and max(windows) == 960            # 480: the maximum at 48 kHz; 960 after the rate change
    lens = {v for c in data for v in c["calls"]}
    assert {1, 511, 512, 513, 8193} <= lens
    # past 0x2000 samples without any event
    quiet = [c for c in data if not c["events"] and not c["single"] and c["n"] >= 2 * 0x2000 + 700]
    assert len(quiet) >= 2 and any(c["calls"] == [8192, 8192, 700] for c in quiet)
    # the places the driver saw the class go through, per mode of the refresh
    places = 0
    for c in data:
        places |= int(np.bitwise_or.reduce(R.column(c, "places")))
    for p in (R.P_RMS_WHOLE, R.P_RMS_WRAPPED, R.P_UNI_WHOLE, R.P_UNI_WRAPPED, R.P_SPLIT, R.P_OTHER_REFRESH, R.P_COUNTED, R.P_AT_START,
              R.P_HEAD_AT_END):
        assert places & p, p
    quiet_places = 0
    for c in quiet:
        quiet_places |= int(np.bitwise_or.reduce(R.column(c, "places")[1:]))          # not the first call's forced refresh
    assert quiet_places & R.P_COUNTED and quiet_places & R.P_AT_START
    assert quiet_places & R.P_RMS_WHOLE and quiet_places & R.P_RMS_WRAPPED and quiet_places & R.P_UNI_WHOLE and quiet_places & R.P_UNI_WRAPPED
    # every setter between calls; the three set_reactivity calls that return early change nothing
    setters = {s for c in data for _, s, _ in c["events"]}
    assert setters == set(R.EVENTS)
    w = by["window 457 mode 1"]
    early = [float(a) for b, s, a in w["events"] if b == 3]
    assert early[0] == float([a for b, s, a in w["events"] if b == 1][0]) and early[1] < 0 and early[2] > w["max_reactivity"]
    assert R.column(w, "reactivity")[3] == R.column(w, "reactivity")[2] == 457 and R.column(w, "refresh")[3] == 511 + 512 + 513
    # set_mode: the same mode changes nothing; a new one zeroes the sum, so the output sits on the clamp until a refresh
    m = by["mode RMS UNIFORM RMS"]
    assert [(b, int(a)) for b, s, a in m["events"]] == [(2, ref.SCM_UNIFORM), (3, ref.SCM_UNIFORM), (4, ref.SCM_RMS)]
    assert any(m["out"].whole[512:1024] == 0.0) and not any(m["out"].whole[64:512] == 0.0)
    # clear, a rate change (new capacity, the mid-side flag dropped), in == NULL, the subnormals
    assert R.column(by["clear uniform"], "refresh")[3] == 513
    r = by["sample rate midside"]
    assert list(R.column(r, "capacity")) == [992, 992, 1472, 1472, 1472] and list(R.column(r, "flags")) == [1, 1, 0, 0, 0]
    assert list(R.column(r, "head")[:3]) == [1, 512, 512]
    assert any(any(c["null"]) for c in data if c["inputs"] == 1) and any(any(c["null"]) for c in data if c["inputs"] == 2)
    d = by["lpf decay"]["out"].whole
    tiny = np.finfo(f32).tiny
    assert np.any((d > 0) & (d < tiny)) and d[-1] == 0.0
    for c in data:
        assert np.isfinite(c["in0"]).all() and (c["in1"] is None or np.isfinite(c["in1"]).all())
    # the single-sample overload on short cases of every mode, and on one that runs past 0x2000 samples
    singles = [c for c in data if c["single"]]
    assert {c["mode"] for c in singles} == set(ref.MODES) and any(c["n"] > 0x2000 for c in singles)


def test_the_head_rests_at_the_capacity_after_a_block_that_ends_there(data):
    """RawRingBuffer::push(data, count) wraps only where nHead + count > nCapacity: a recorded call leaves position() == capacity."""
    hit = [(c["name"], i) for c in data for i in range(len(c["state"])) if R.column(c, "head")[i] == R.column(c, "capacity")[i]]
    assert hit
    assert all(R.column(c, "places")[i] & R.P_HEAD_AT_END for c in data for n, i in hit if c["name"] == n)
    assert not any(R.column(c, "head")[i] == 0 for c in data for i in range(len(c["state"])))


def test_restatement_gives_the_references_output_state_and_ring(data, restated):
    for c, (out, rows, ring, _) in zip(data, restated):
        assert c["out"].mismatch(out) is None, (c["name"], c["out"].mismatch(out))
        want = c["state"][:, :8]
        got = rows[-1:] if c["single"] else rows
        for k, name in enumerate(R.STATE[:8]):
            assert np.array_equal(got[:, k], want[:, k]), (c["name"], name, got[:, k], want[:, k])
        assert np.array_equal(bits(ring), bits(c["ring"])), c["name"]


def test_single_sample_overload_differs_from_length_one_calls_as_documented(data):
    """Sidechain.h of this project documents that process(const float *) is one sample through the block path, and names where the
    reference's own text for it differs from its block overload.  R.one_by_one has each arithmetic difference as a switch: with
    all of them on it gives the recorded single-sample results bit for bit, with all of them off the recorded calls of length 1,
    and with any one of them off it misses a recorded single-sample result.  The remaining documented difference (no equalizer
    for LEFT and RIGHT in stereo mode) needs a pre-equalizer, which no recorded case has."""
    missed = {"early": 0, "divide": 0, "left_first": 0}
    for c in data:
        if not c["single"]:
            continue
        params = R.single_params(c)
        on = dict(early=True, divide=True, left_first=True)
        assert c["single_out"].mismatch(R.one_by_one(c, params, **on)) is None, (c["name"], c["single_out"].mismatch(R.one_by_one(c, params, **on)))
        assert c["out"].mismatch(R.one_by_one(c, params, False, False, False)) is None, c["name"]
        if c["mode"] in (ref.SCM_PEAK, ref.SCM_LPF) and c["n"] < ref.REFRESH_RATE:
            assert c["out"].mismatch(np.array([c["single_out"].at(i) for i in range(c["n"])], f32)) is None      # nothing to differ in
        for which in missed:
            miss = c["single_out"].mismatch(R.one_by_one(c, params, **dict(on, **{which: False})))
            missed[which] += miss is not None
            if which == "early" and miss is not None:
                # not before the sample that brings the single-sample overload's counter to 0x2000
                assert c["n"] > ref.REFRESH_RATE and int(miss.split()[1].rstrip(":")) >= ref.REFRESH_RATE - 1 - R.WINDOW, miss
    assert missed["early"] >= 1 and missed["divide"] >= 2 and missed["left_first"] >= 2, missed


def test_host_parameters_are_the_references(mi, data):
    """mi_sidechain_compute_params against the recorded nReactivity, capacity and 1 / nReactivity in every bit, and against fTau
    where this machine's libm rounds as the recording machine's did: at least three quarters of the distinct windows."""
    seen = {}
    for c in data:
        if c["single"]:
            continue
        st = R.Settings(c)
        for i in range(len(c["calls"])):
            for setter, a in R.events_before(c, i):
                st.apply(setter, a)
            p = mi.SidechainBank.compute_params(st.rate, float(st.max), float(st.reactivity))
            want = R.recorded_params(c)[i]
            assert (p["reactivity"], p["capacity"]) == (want["reactivity"], want["capacity"]), (c["name"], i)
            assert bits(p["interval"]) == bits(want["interval"])
            assert (p["reactivity"], p["capacity"]) == (ref.reactivity_samples(st.rate, st.reactivity), ref.capacity(st.rate, st.max))
            seen[(st.rate, want["reactivity"])] = bool(bits(p["tau"]) == bits(want["tau"]))
    assert len(seen) >= 12
    agree = sum(seen.values())
    assert 4 * agree >= 3 * len(seen), "fTau agrees on %d of %d windows: %r" % (agree, len(seen), [k for k, v in seen.items() if not v])
