"""LoudnessMeter and ILUFSMeter against the REFERENCE'S OWN classes, host side: the results stored in
tests/golden/loudness_ref_vectors.npz and ilufs_ref_vectors.npz (tests/golden/make_loudness_vectors.py) are fresh, hold every branch
and edge they were made for, and the restatements oracle.loudness.LoudnessMeter and oracle.ilufs.ILUFSMeter give every recorded output
and every recorded state value after every call bit for bit.  The GPU side is tests/test_loudness_reference_gpu.py.

The product's own settings arithmetic (period, latency, block size, nMSInt, history size) lives behind mi_loudness_bank_create /
mi_ilufs_bank_create, which need a device: it is held to the recorded integers there."""
import os
import sys

import numpy as np
import pytest

import loudness_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
bits = R.bits
OP = R.OP
GATING_ABS_THRESH = f32(1.17246530458e-07)


@pytest.fixture(scope="module")
def loudness():
    return R.load(R.LOUDNESS)


@pytest.fixture(scope="module")
def ilufs():
    return R.load(R.ILUFS)


def _generator():
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_loudness_vectors as gen
    return gen


def test_stored_vectors_are_fresh():
    gen = _generator()
    if not (os.path.exists(gen.LD_REF) and os.path.exists(gen.LD_SAN)):
        pytest.skip("oracle/_ref/loudness_ref is built only where the reference tree is")
    for kind in (R.LOUDNESS, R.ILUFS):
        with open(R.FILES[kind], "rb") as f:
            assert gen.build_bytes(kind) == f.read(), os.path.basename(R.FILES[kind])
        assert os.path.getsize(R.FILES[kind]) < 400 * 1000


def _ops(c, name):
    return [s for s in c["steps"] if s[0] == OP[name]]


def _process(c):
    return _ops(c, "process")


def test_stored_loudness_vectors_hold_every_branch_and_edge(loudness):
    cs = [c for c in loudness if "bare_clear" not in c]
    assert {c["channels"] for c in cs} >= {1, 2, 3, 6} and {c["sample_rate"] for c in cs} >= {44100, 48000}
    states = [R.lstate(r, c["channels"]) for c in cs for r in c["calls"]]
    assert {s["size"] for s in states} == {2048}
    places = 0
    for s in states:
        places |= s["places"]
    for bit in (R.P_START_WHOLE, R.P_START_WRAPPED, R.P_COUNTED_WHOLE, R.P_COUNTED_WRAPPED, R.P_RING_WRAPPED):
        assert places & bit, "no case goes through place %d" % bit
    # streams of 9000 to 14000 samples: the ring wrapped several times, calls with a counted refresh more often than there are cases
    assert all(9000 <= c["n"] <= 14000 for c in cs)
    assert sum(1 for s in states if s["places"] & (R.P_COUNTED_WHOLE | R.P_COUNTED_WRAPPED)) > len(cs)
    # designations: the defaults of mono and stereo, NONE beyond, the +1.5 dB group, both LFE
    des = {(c["channels"], int(d)) for c in cs for r in c["calls"] for d in r["designation"]}
    assert {(1, 1), (2, 4), (2, 5), (3, 0), (6, 32), (6, 33)} <= des and any(6 <= d <= 11 for _, d in des)
    # links 0, 1, in between, and out of range either way (recorded as the class clamps them)
    asked = [float(s[2]) for c in cs for s in _ops(c, "set_link")]
    assert 0.0 in asked and any(0 < v < 1 for v in asked) and any(v > 1 for v in asked) and any(v < 0 for v in asked)
    got = {float(R.from_bits(v)) for c in cs for r in c["calls"] for v in r["link"]}
    assert 0.0 in got and 1.0 in got and min(got) >= 0.0 and max(got) <= 1.0
    assert {r["weighting"] for c in cs for r in c["calls"]} == set(range(6))
    # periods: one sample (0 ms), the maximum, above it, shorter and longer mid-stream, the same value again without a flag
    per = [c for c in cs if c["name"] == "periods"][0]
    seq = [R.lstate(r, 2)["period"] for r in per["calls"]]
    assert 1 in seq and 960 in seq and any(b < a for a, b in zip(seq, seq[1:])) and any(b > a for a, b in zip(seq, seq[1:]))
    assert any(float(s[2]) > float(per["a"]) for s in _ops(per, "set_period"))
    pend = {(int(s[0]), float(s[2])): int(r[0]) for s, r in zip(per["steps"], per["step_results"])}
    assert any(o == OP["set_period"] and p == 0 for (o, _), p in pend.items()) and any(o == OP["set_period"] and p == 1 for (o, _), p in pend.items())
    # set_active either way, the same state again; unbound and bound again; every channel off, every channel unbound
    for c in cs:
        for call, r in zip(R.walk(c), c["calls"]):
            assert [int(v) for v in r["active"]] == [int(v) for v in call["active"]], c["name"]
    walks = [call for c in cs for call in R.walk(c)]
    assert any(not any(w["active"]) for w in walks) and any(all(v is None for v in w["in_at"]) and all(w["active"]) for w in walks)
    ab = [c for c in cs if c["name"] == "active and bound"][0]
    acts = [(s[1], float(s[2])) for s in _ops(ab, "set_active")]
    assert acts[:4] == [(1, 0.0), (2, 1.0), (1, 0.0), (1, 1.0)]                 # off, on -> on, off -> off, on
    # out == NULL, per-channel outputs absent, both forms, a call of no samples, the call lengths, binding with a position and
    # calls without rebinding
    calls = [s for c in cs for s in _process(c)]
    assert any(s[4] & R.PF_NULL for s in calls) and any(s[4] & R.PF_GAIN for s in calls) and any(not s[4] & R.PF_GAIN for s in calls)
    assert {1, 1023, 1024, 1025, 4096, 4097, 9000, 0} <= {s[3] for s in calls}
    assert any(s[4] & R.PF_KEEP for s in calls) and any(s[3] > 0 for c in cs for s in _ops(c, "bind"))
    assert any(w["in_at"][k] is not None and not w["have"][k] and w["active"][k] for w in walks for k in range(len(w["have"])))
    zero = [(c, i) for c in cs for i, s in enumerate(c["steps"]) if s[0] == OP["process"] and s[3] == 0]
    assert all(c["step_results"][i - 1][0] == 1 and c["step_results"][i][0] == 0 for c, i in zero) and zero
    # only the plain form records fLoudness
    for c in cs:
        last = 0
        for s, r in zip(c["steps"], c["step_results"]):
            if s[0] == OP["process"] and s[4] & R.PF_GAIN:
                assert int(r[2]) == last, c["name"]
            last = int(r[2])
    # set_sample_rate to the same rate and to another one
    sr = [c for c in cs if c["name"] == "sample rate"][0]
    assert {s[3] for s in _ops(sr, "set_sample_rate")} == {44100, 48000} and {r["sample_rate"] for r in sr["calls"]} == {44100, 48000}
    # the inputs: a stretch 100 dB down, subnormals, a full-scale step
    x = R.rows([c for c in cs if c["name"] == "levels"][0])
    tiny = np.abs(x[0]) < np.finfo(f32).tiny
    assert (tiny & (x[0] != 0)).sum() > 1000 and np.abs(x[0]).max() == 1.0 and ((np.abs(x[0]) < 4e-6) & ~tiny).sum() > 2000
    # the bare clear(): the reference's bank takes the cascades a second time and computes something else from there
    bare = [c for c in loudness if "bare_clear" in c]
    assert len(bare) == 1 and bare[0]["bare_clear"] == (2, 4, 1)
    good = [c for c in cs if c["name"] == "clear defined"][0]
    assert [s for s in good["steps"] if s[0] != OP["set_weighting"]] == bare[0]["steps"] and good["segments"] == bare[0]["segments"]
    assert all(R.lstate(r, 2)["items"] == 2 for r in good["calls"])


def test_stored_ilufs_vectors_hold_every_branch_and_edge(ilufs):
    cs = ilufs
    assert {c["channels"] for c in cs} == {1, 2, 3} and all(12000 <= c["n"] <= 14000 for c in cs)
    first = {c["name"]: R.istate(c["calls"][0], c["channels"]) for c in cs}
    assert {s["block_size"] for s in first.values()} >= {48, 96} and all(48 <= s["block_size"] <= 96 for s in first.values())
    sizes = {s["ms_size"] for s in first.values()}
    assert 64 in sizes and 96 in sizes                                  # int_count below 64, and 90 rounded up to 16 floats
    assert any(s["ms_int"] == 0 for s in first.values())                # infinite mode
    wrapped = halved = dropped = lost = False
    ms_ints = set()
    for c in cs:
        prev = None
        evaluated = 0
        for call, r in zip(R.walk(c), c["calls"]):
            s = R.istate(r, c["channels"])
            ms_ints.add(s["ms_int"])
            if s["ms_int"] > 0:
                live = [(s["ms_head"] + s["ms_size"] - 1 - j) % s["ms_size"] for j in range(s["ms_count"])]
                dropped = dropped or any(s["hist"][i] <= GATING_ABS_THRESH for i in live)
                wrapped = wrapped or (prev is not None and prev["ms_size"] == s["ms_size"] and s["ms_head"] < prev["ms_head"] and s["ms_count"] >= prev["ms_count"] > 0)
            elif prev is not None and prev["ms_int"] == 0:
                halved = halved or (0 < s["ms_count"] < prev["ms_count"] and prev["ms_count"] > 0x80)
            # a call of fewer than four quarters that started with quarters done: F_BLK_FULL was wiped, nothing is evaluated
            if prev is not None and call["len"] < 4 * s["block_size"] and s["flags"] == 0 and call["len"] >= s["block_size"]:
                lost = lost or (np.array_equal(bits(prev["hist"]), bits(s["hist"])) and prev["ms_head"] == s["ms_head"] and evaluated > 0)
            evaluated += int(s["flags"] == 4)
            prev = s
    assert wrapped and halved and dropped and lost
    assert 1 in ms_ints and len(ms_ints) >= 5
    for name in ("set_period", "set_weighting", "set_active", "clear", "set_sample_rate", "bind", "set_designation", "update_settings"):
        assert any(_ops(c, name) for c in cs), name
    calls = [s for c in cs for s in _process(c)]
    assert any(s[4] & R.PF_NULL for s in calls)
    assert {1.0, 0.0} <= {float(s[2]) for s in calls if s[4] & R.PF_GAIN} and any(not s[4] & R.PF_GAIN for s in calls)
    # calls that end on, one before and one after a quarter block's end; a clear() and a weighting change inside a block
    offs = {R.istate(r, c["channels"])["block_offset"] for c in cs if c["name"] == "mono finite 50" for r in c["calls"]}
    assert {0, 47, 1} <= offs
    wc = [c for c in cs if c["name"] == "weighting clear rate"][0]
    seen, k = set(), 0
    for i, s in enumerate(wc["steps"]):
        if s[0] == OP["process"]:
            k += 1
        elif k and s[0] in (OP["clear"], OP["set_weighting"]):
            st = R.istate(wc["calls"][k - 1], 2)
            if st["block_offset"] or st["block_part"]:
                seen.add(s[0])
    assert seen == {OP["clear"], OP["set_weighting"]}
    # needs_update() is nFlags != 0 and F_BLK_FULL is one of nFlags' bits: a call that completed a gating block leaves it pending
    assert any(int(r[0]) == 1 and s[0] == OP["process"] for c in cs for s, r in zip(c["steps"], c["step_results"]))
    # the condition on the inputs: no stored gating block within 5 % of the absolute gate
    for c in cs:
        for r in c["calls"]:
            s = R.istate(r, c["channels"])
            if s["ms_int"] > 0:
                live = [(s["ms_head"] + s["ms_size"] - 1 - j) % s["ms_size"] for j in range(s["ms_count"])]
                assert all(abs(float(s["hist"][i]) - float(GATING_ABS_THRESH)) >= 0.05 * float(GATING_ABS_THRESH) for i in live), c["name"]


def _held(c):
    """The restatement over one case against the recording: every step's needs_update / latency / loudness, every call's output (the
    CRC of all of it, and the stored samples themselves), every state value."""
    K = c["channels"]
    steps, calls = R.replay(c)
    assert np.array_equal(steps, c["step_results"]), (c["name"], np.flatnonzero((steps != c["step_results"]).any(axis=1))[:4])
    for i, (got, want) in enumerate(zip(calls, c["calls"])):
        what = (c["name"], "call %d" % i)
        assert R.crc(got["out"]) == want["crc"], what
        assert [None if v is None else R.crc(v) for v in got["ch_out"]] == want["ch_crc"], what
        w = [int(v) for v in want["state"]]
        g = [wv if gv is None else int(gv) for gv, wv in zip(got["state"], w)]
        assert g == w, what + ([(k, a, b) for k, (a, b) in enumerate(zip(g, w)) if a != b][:6],)
    out = np.concatenate([q["out"] for q in calls])
    if c["kind"] == R.ILUFS:
        assert np.array_equal(bits(out), bits(c["out"])), c["name"]
    else:
        rows_ = [out] + [np.concatenate([v if v is not None else np.full(len(q["out"]), R.SENTINEL, f32) for q in calls for v in [q["ch_out"][k]]])
                         for k in range(K)]
        assert np.array_equal(bits(np.stack([v[c["index"]] for v in rows_])), bits(c["samples"])), c["name"]
    return len(calls)


def test_loudness_restatement_gives_the_references_bits(loudness):
    n = sum(_held(c) for c in loudness if "bare_clear" not in c)
    assert n >= 50


def test_ilufs_restatement_gives_the_references_bits(ilufs):
    n = sum(_held(c) for c in ilufs)
    assert n >= 40
