"""The numpy restatement of the TruePeakMeter (truepeak_ref) against the REFERENCE'S OWN class: TruePeakMeter.cpp compiled
unmodified (oracle/Makefile -> oracle/_ref/truepeak_ref) and run by tests/golden/make_resampler_vectors.py, whose results are stored
in tests/golden/truepeak_ref_vectors.npz.  tests/test_resampler_reference_gpu.py holds the kernel and the C++ class to the same
file.  Not pinned by any of this: the tap values (the stand-in resampler takes mi_truepeak_coefficients' table) and dsp::abs2 /
abs_max, which the reference tree does not carry.  The second half does the same for the Oversampler
(oversampler_ref, oracle/_ref/oversampler_ref, oversampler_ref_vectors.npz)."""
import os
import sys

import numpy as np
import pytest

import resampler_reference as R
import truepeak_ref as tp

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_resampler_vectors as gv  # noqa: E402

f32 = np.float32
bits = R.bits


@pytest.fixture(scope="module")
def data():
    return R.load()


def replay(case, table):
    """The restatement through the case's calls and events -> (out [n], per call (latency, maximum of process_max, times))."""
    ref = tp.TruePeakRef(1, table)
    ref.set_sample_rate(case["sample_rate"])
    out, rows, pos = np.zeros(len(case["x"]), f32), [], 0
    for i, (n, kind) in enumerate(case["calls"]):
        for before, setter, a in case["events"]:
            if before == i:
                ref.set_sample_rate(a) if setter == "set_sample_rate" else ref.clear()
        x = case["x"][None, pos:pos + n]
        peak = None
        if kind == "process_max":
            twin_state = ref.state.copy()
            peak = ref.process_max(x)[0]
            ref.state = twin_state                  # ... and the same samples once more for the stream's output
        out[pos:pos + n] = ref.process(x)[0]
        rows.append((ref.latency(), peak, ref.times))
        pos += n
    return out, rows


def test_stored_vectors_are_what_the_reference_gives_today():
    """Freshness: where the reference binary exists the generator runs again (the sanitizer run included) and must give the
    committed bytes."""
    if not os.path.exists(gv.TP_REF):
        pytest.skip("no oracle/_ref/truepeak_ref: the reference tree is not on this machine")
    with open(gv.OUT, "rb") as f:
        assert gv.build_bytes() == f.read(), "truepeak_ref_vectors.npz is stale: python tests/golden/make_resampler_vectors.py"


def test_stored_vectors_hold_every_branch_and_edge(data):
    assert os.path.getsize(R.PATH) < 400 * 1000
    by = {c["name"]: c for c in data}
    # rates for the factors 8, 6, 4, 3, 2 and none, four signals each, 5000 samples cut at 1, 511, 512, 513 and 2048
    plain = [c for c in data if not c["events"]]
    assert sorted({int(R.column(c, "times")[0]) for c in plain}) == [0, 2, 3, 4, 6, 8] and len(plain) == 24
    for c in plain:
        assert len(c["x"]) == 5000 and [n for n, _ in c["calls"]][:5] == [1, 511, 512, 513, 2048]
        assert {k for _, k in c["calls"]} == set(R.KINDS)
        times = int(R.column(c, "times")[0])
        assert list(R.column(c, "latency")) == [10 if times else 0] * len(c["calls"])
        if times:
            # two compactions at least, each from where the buffer cannot take another input: 4096 - (4096 mod N)
            assert R.column(c, "compactions").sum() >= 2
            froms = {int(f) for f, k in zip(R.column(c, "from"), R.column(c, "compactions")) if k}
            assert froms == {R.BUFFER_SIZE - R.BUFFER_SIZE % times}, (c["name"], froms)
            # a call straddles a compaction: it starts with room in the buffer and compacts inside
            heads = [0] + [int(h) for h in R.column(c, "head")[:-1]]
            assert any(k and h < R.BUFFER_SIZE - times for h, k in zip(heads, R.column(c, "compactions")))
        else:
            assert R.column(c, "compactions").sum() == 0 and not R.column(c, "head").any()
    assert {int(f) for c in plain for f in R.column(c, "from") if f} == {4096, 4095, 4092}      # 3x and 6x start from 4095, 4092
    assert 4095 in {int(f) for f in R.column(by["3x noise"], "from")}
    sine, zeros = by["4x sine"], by["4x zeros"]
    assert np.allclose(np.abs(sine["x"]), np.sqrt(0.5), atol=1e-6) and sine["out"][100:].max() > 0.99
    assert np.signbit(zeros["x"][zeros["x"] == 0]).any() and not np.signbit(zeros["x"][zeros["x"] == 0]).all()
    # a rate change that keeps the factor does not clear; one that changes it does; clear() in mid-stream
    keep, change = by["rate keeps factor"], by["rate changes factor"]
    assert list(R.column(keep, "times")) == [4] * 6 and list(R.column(keep, "update")) == [1, 0, 1, 0, 0, 0]
    assert np.array_equal(bits(keep["out"]), bits(by["4x noise"]["out"]))
    assert list(R.column(change, "times")) == [4, 4, 2, 2, 4, 4] and R.column(change, "head")[2] == 2 * 512
    assert not np.array_equal(bits(change["out"][1024:1100]), bits(by["4x noise"]["out"][1024:1100]))
    assert list(R.column(by["rate to none and back"], "times")) == [4, 0, 0, 8, 8, 8]
    assert list(R.column(by["rate to none and back"], "latency")) == [10, 0, 0, 10, 10, 10]
    assert R.column(by["clear 3x"], "head")[3] == 3 * 513 and {s for c in data for _, s, _ in c["events"]} == set(R.EVENTS)


def test_factor_per_rate_is_the_recorded_one(data):
    seen = set()
    for c in data:
        rate = c["sample_rate"]
        for i in range(len(c["calls"])):
            for before, setter, a in c["events"]:
                if before == i and setter == "set_sample_rate":
                    rate = a
            assert tp.oversampling(rate) == R.column(c, "times")[i], (c["name"], i, rate)
            seen.add(rate)
    assert seen == {22050, 32000, 44100, 48000, 64000, 96000, 192000}


def test_restatement_gives_the_references_output_and_latency(mi, data):
    for c in data:
        out, rows = replay(c, mi.TruePeakBank.coefficients)
        bad = np.flatnonzero(bits(out) != bits(c["out"]))
        assert len(bad) == 0, (c["name"], bad[:4], out[bad[:4]], c["out"][bad[:4]])
        assert [r[0] for r in rows] == list(R.column(c, "latency")) and [r[2] for r in rows] == list(R.column(c, "times"))
        # process_max as this project documents it: the largest value process() writes for the block
        for (lat, peak, _), want, (n, kind) in zip(rows, R.call_maxima(c), c["calls"]):
            assert kind != "process_max" or bits(peak) == bits(want), (c["name"], peak, want)


def test_the_references_process_max_returns_zero(data):
    """TruePeakMeter.cpp:271 returns 0.0f whatever it found (and :264 looks at to_process of the nTimes * to_process values).  The
    product's header documents that it returns the block's maximum instead: the record and the decision, side by side."""
    calls = [(c, i) for c in data for i, (n, kind) in enumerate(c["calls"]) if kind == "process_max"]
    assert len(calls) >= 50
    oversampled = [(c, i) for c, i in calls if R.column(c, "times")[i]]
    assert all(bits(R.column(c, "returned")[i]) == 0 for c, i in oversampled)
    assert sum(R.call_maxima(c)[i] > 0 for c, i in oversampled) >= 40           # ... where the block's true peak is not zero
    # without oversampling it returns dsp::abs_max of the input, which is what process() writes there
    plain = [(c, i) for c, i in calls if not R.column(c, "times")[i]]
    assert plain and all(bits(R.column(c, "returned")[i]) == bits(R.call_maxima(c)[i]) for c, i in plain)


# ---- Oversampler ------------------------------------------------------------------------------------------------------------
import oversampler_ref as osr  # noqa: E402


@pytest.fixture(scope="module")
def os_data():
    return R.os_load()


def os_replay(case, table):
    """The restatement through the case's steps -> (up, down, per step (oversampling, latency, modified, the filter calls it owes)).
    The recorded filter copies, so the restatement's own filter is taken out: what it is ASKED is compared instead."""
    ref = osr.OversamplerRef(1, table)
    ref._filtered = lambda y: y
    fbits = lambda p: (0,) * 6 if p is None else (int(p[0]), int(p[1])) + tuple(int(bits(v)[0]) for v in p[2:])
    up, down, rows, pos, last = [], [], [], 0, None
    for op, a in case["steps"]:
        calls = []
        if op == "set_mode":
            ref.set_mode(a)
        elif op == "set_sample_rate":
            changed = a != ref.sample_rate
            ref.set_sample_rate(a)
            if changed:
                calls.append((False, ref.design_rate, fbits(ref.params)))
        elif op == "set_filtering":
            ref.set_filtering(a)
        elif op == "update_settings":
            if ref.update & (osr.UP_MODE | osr.UP_SAMPLE_RATE):
                calls.append((True, 0, fbits(ref.params)))
            ref.update_settings()
            calls.append((False, ref.design_rate, fbits(ref.params)))
        elif op == "upsample":
            last = ref.upsample(case["x"][None, pos:pos + a])
            up.append(last[0])
            pos += a
        elif op == "downsample":
            down.append(ref.downsample(last)[0])
        else:
            with np.errstate(all="ignore"):
                down.append(ref.process(case["x"][None, pos:pos + a], lambda y: (y * f32(-0.5) + f32(0.0)).astype(f32))[0])
            pos += a
        rows.append((ref.oversampling(), ref.latency(), int(ref.modified()), calls))
    cat = lambda v: np.concatenate(v) if v else np.zeros(0, f32)
    return cat(up), cat(down), rows


def test_oversampler_vectors_are_what_the_reference_gives_today():
    if not os.path.exists(gv.OS_REF):
        pytest.skip("no oracle/_ref/oversampler_ref: the reference tree is not on this machine")
    with open(gv.OS_OUT, "rb") as f:
        assert gv.os_build_bytes() == f.read(), "oversampler_ref_vectors.npz is stale: python tests/golden/make_resampler_vectors.py"


def test_oversampler_vectors_hold_every_branch_and_edge(mi, os_data):
    assert os.path.getsize(R.OS_PATH) < 400 * 1000
    by = {c["name"]: c for c in os_data}
    modes = {a for c in os_data for op, a in c["steps"] if op == "set_mode"}
    assert modes == set(range(31))                                                  # all 30 modes and OM_NONE
    for name, mode in osr.MODES.items():
        c = by["mode " + name]
        times = osr.oversampling(mode)
        ups = [a for op, a in c["steps"] if op == "upsample"]
        assert ups[:5] == [1, 61, 62, 63, R.OS_UP_BUFFER_SIZE // times] and sum(ups) * times >= 26000
        # two compactions of the buffer: nUpHead falls short of what the calls added by the buffer's length each time
        head = [0] + [int(h) for (op, _), h in zip(c["steps"], c["state"][:, 3]) if op == "upsample"]
        short = [h0 + times * a - h1 for h0, h1, a in zip(head, head[1:], ups)]
        assert all(v % R.OS_UP_BUFFER_SIZE == 0 for v in short) and sum(short) // R.OS_UP_BUFFER_SIZE >= 2, (name, head)
        assert any(v and h0 for v, h0 in zip(short, head)), name                     # ... inside a call that began with room
        assert [a for op, a in c["steps"] if op == "downsample"] == ups and c["down"].n == sum(ups)
        # no pending sum reaches past the stand-in's RSV_SAMPLES
        h = mi.OversamplerBank.coefficients(mode)
        assert h.size - h.shape[0] <= R.RSV_SAMPLES
    assert max(mi.OversamplerBank.coefficients(m).size for m in range(1, 31)) == 8 * 2 * 62
    f = by["filter requests"]
    rates = {a for op, a in f["steps"] if op == "set_sample_rate"}
    assert rates == {20000, 44100, 48000, 96000}
    assert sum(1 for r in f["log"] if r[0]) >= 5 and sum(1 for r in f["log"] if not r[0]) >= 12
    # same-value setters ask nothing and clear nothing: the update_settings() after them has one update and no clear
    i = f["steps"].index(("set_filtering", 1))
    assert f["steps"][i - 2:i + 2] == [("set_mode", osr.MODES["4X16BIT"]), ("set_sample_rate", 44100), ("set_filtering", 1), ("update_settings", 0)]
    assert [R.os_calls(f, k) for k in (i - 2, i - 1, i)] == [[], [], []] and [c[0] for c in R.os_calls(f, i + 1)] == [False]
    # 20000 Hz: 0.42 sr = 8400 is the smaller limit
    k = f["steps"].index(("set_sample_rate", 20000))
    assert np.array([R.os_calls(f, k)[0][2][2]], np.uint32).view(f32)[0] == f32(8400.0) and R.os_calls(f, k)[0][1] == 8 * 20000
    p = by["process 8X16BIT"]
    assert [a for op, a in p["steps"] if op == "process"] == [1, 1535, 1536, 1537, 4097]
    assert ("set_filtering", 1) in p["steps"] and {c["name"] for c in os_data} >= {"process 3X4", "process 2X24BIT", "process NONE", "mode NONE"}


def test_oversampler_restatement_gives_the_references_samples_and_requests(mi, os_data):
    for c in os_data:
        up, down, rows = os_replay(c, mi.OversamplerBank.coefficients)
        assert c["up"].mismatch(up) is None, (c["name"], "up", c["up"].mismatch(up))
        assert c["down"].mismatch(down) is None, (c["name"], "down", c["down"].mismatch(down))
        for k, (times, lat, mod, calls) in enumerate(rows):
            assert (times, lat, mod) == tuple(int(v) for v in c["state"][k, :3]), (c["name"], k, c["steps"][k])
            assert calls == R.os_calls(c, k), (c["name"], k, c["steps"][k], calls, R.os_calls(c, k))


def test_oversampler_tables_of_oversampling_and_latency_are_the_recorded_ones(os_data):
    seen = {}
    for c in os_data:
        mode = 0
        for (op, a), st in zip(c["steps"], c["state"]):
            mode = a if op == "set_mode" else mode
            seen[mode] = (int(st[0]), int(st[1]))
            assert (osr.oversampling(mode), osr.latency(mode)) == seen[mode], (c["name"], mode)
    assert sorted(seen) == list(range(31)) and seen[0] == (1, 0) and seen[osr.MODES["8X24BIT"]] == (8, 62)
