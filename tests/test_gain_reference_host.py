"""The numpy restatements (limiter_ref, autogain_ref) and the host code of update_settings() / update()
(mi_limiter_compute_params, mi_limiter_compute_patch, mi_autogain_compute_params, mi_simple_autogain_compute_params) against the
REFERENCE'S OWN Limiter, AutoGain and SimpleAutoGain: their .cpp text compiled unmodified (oracle/Makefile -> oracle/_ref/gain_ref)
and run by tests/golden/make_gain_vectors.py, whose results are stored in tests/golden/limiter_ref_vectors.npz and
autogain_ref_vectors.npz.  A reading of the reference that the restatement and the kernel share is caught here;
tests/test_gain_reference_gpu.py holds the kernels and the C++ classes to the same files.

Not pinned by any of this: dsp::abs_mul3 and dsp::max_index, which the reference tree does not carry and
oracle/ref_shim states by this project's reading."""
import os

import numpy as np
import pytest

import gain_reference as R
from gain_reference import ar, gv, lr

f32 = np.float32


@pytest.fixture(scope="module")
def data():
    return R.load()


@pytest.fixture(scope="module")
def restated(data):
    """Every case through its restatement fed the reference's recorded parameters: computed once."""
    out = {"limiter": [R.run_limiter(c, R.recorded_limiter(c)) for c in data["limiter"]],
           "autogain": [R.run_autogain(c, lambda k, c=c: R.autogain_params(c, k)) for c in data["autogain"]],
           "autogain_level": [R.run_autogain(c, lambda k, c=c: R.autogain_params(c, k), scalar=True) for c in data["autogain"]],
           "simple": [R.run_simple(c, lambda k, c=c: R.simple_params(c, k)) for c in data["simple"]]}
    return out


def test_stored_vectors_are_what_the_reference_gives_today():
    """Freshness: where the reference binary exists the generator runs again (the sanitizer run included) and must give the
    committed bytes."""
    if not os.path.exists(gv.GAIN_REF):
        pytest.skip("no oracle/_ref/gain_ref: the reference tree is not on this machine")
    fresh = gv.build_bytes()
    for which, path in gv.OUT.items():
        with open(path, "rb") as f:
            assert fresh[which] == f.read(), "%s is stale: python tests/golden/make_gain_vectors.py" % os.path.relpath(path, gv.ROOT)


def test_stored_vectors_are_small_and_complete(data):
    for path in gv.OUT.values():
        assert os.path.getsize(path) < 400 * 1024
    lim = data["limiter"]
    assert len(lim) == gv.LIM_GENERAL + 1 + len(gv.LONG_CUTS)
    assert all(len(c["inputs"][0]) == gv.LIM_N and len(c["calls"]) >= 3 for c in lim[:gv.LIM_GENERAL])
    assert len({int(c["settings"][2]) for c in lim[:gv.LIM_GENERAL]}) >= 3                          # sample rates
    one, cuts = lim[gv.LIM_GENERAL], lim[gv.LIM_GENERAL + 1:]
    assert one["calls"] == [gv.LONG_N] and gv.LONG_N == 8192 + 300 and gv.LONG_CUTS == (5000, 4096, 8191)
    for at, cut in zip(gv.LONG_CUTS, cuts):
        assert cut["calls"] == [at, gv.LONG_N - at]
        assert R.same(one["inputs"][0], cut["inputs"][0]) and np.array_equal(one["settings"], cut["settings"])
    assert np.isfinite(np.concatenate([c["inputs"][0] for c in lim])).all(), "no NaN and no infinity goes into the Limiter"
    for c in lim:
        # the reference writes outside its allocation with ML < 8, and below 8 samples of look-ahead lsp_limit's order decides
        assert all(R.row("limiter", c, k)["max_lookahead"] >= 8 and R.row("limiter", c, k)["lookahead"] >= 8 for k in range(len(c["calls"])))
        assert 8 <= R.row("limiter", c, 0)["max_lookahead"] <= 400
        # every cut falls inside a burst: the samples on both sides of it are far above the threshold
        x, thr = np.abs(c["inputs"][0]), max(R.row("limiter", c, k)["threshold"] for k in range(len(c["calls"])))
        if "a peak at" not in c["name"]:
            assert all(x[e - 1] > thr and x[e] > thr for e in np.cumsum(c["calls"])[:-1]), c["name"]
    names = [c["name"] for c in lim]
    for special in ("second sample", "last sample", "dense", "two equal peaks", "threshold, look-ahead and mode change", "sample rate and ALR"):
        assert sum(special in n for n in names) == 1, special
    assert sum(int(c["settings"][9]) for c in lim) >= 4                                              # ALR on
    ev = {gv.event_call("limiter", e)[0] for c in lim for e in c["events"]}
    assert ev == {name for name, _, _ in gv.EVENTS["limiter"]}
    eq = [c for c in lim if "two equal peaks" in c["name"]][0]["inputs"][0]
    top = np.flatnonzero(eq[:eq.size // 4] == eq[:120].max())
    assert len(top) == 2 and not eq[:120][np.setdiff1d(np.arange(120), top)].any()

    ag = data["autogain"]
    assert len({int(c["settings"][0]) for c in ag[:gv.AG_GENERAL]}) == 3
    assert {(bool(c["settings"][8]), bool(c["settings"][9])) for c in ag[:gv.AG_GENERAL]} == {(a, b) for a in (False, True) for b in (False, True)}
    assert all(len(c["inputs"][0]) == sum(ar.LENGTHS) for c in ag[:gv.AG_GENERAL])
    for special in ("setters between the calls", "all silence", "subnormal gain", "one NaN", "one +Inf"):
        assert [c["name"] for c in ag].count(special) == 1, special
    ev = {gv.event_call("autogain", e)[0] for c in ag for e in c["events"]}
    assert ev >= {"set_deviation", "enable_quick_amplifier", "enable_max_gain", "set_max_gain", "set_short_speed", "set_long_speed",
                  "set_silence_threshold"}
    sg = data["simple"]
    assert len({int(c["settings"][0]) for c in sg[:gv.SAG_GENERAL]}) == 3
    for special in ("a level at the threshold", "limit setters: min, max, both", "limit setters: max, min, both", "decay into subnormals",
                    "one NaN", "one +Inf"):
        assert [c["name"] for c in sg].count(special) == 1, special


# ---- conditions on the inputs, read from the reference's recorded results -------------------------------------------------
def test_limiter_cases_reach_what_they_are_for(data):
    lim = data["limiter"]
    assert {R.row("limiter", c, k)["mode"] for c in lim for k in range(len(c["calls"]))} == set(range(12))
    inside = at_end = passed = met = 0
    for c in lim:
        ml8 = 8 * R.row("limiter", c, 0)["max_lookahead"]
        before = 0
        for k, n in enumerate(c["calls"]):
            head = R.row("limiter", c, k)["head"]
            if n <= lr.BUF_GRANULARITY:
                assert head == (before + n if before + n < ml8 else 0), (c["name"], k)
                at_end += head == 0
                passed += before + n > ml8
                met += before + n == ml8
            else:                                   # a call of several chunks that ends on another count than it would without a move
                inside += head < before + n and head != 0
            before = head
    # `inside` rests on one case: only a call of more than 8192 samples has a chunk end, and with it a move, inside itself,
    # and "long, one call" is the only such call recorded
    assert inside >= 1 and at_end >= 1 and passed >= 1 and met >= 1, (inside, at_end, passed, met)
    for c in lim:
        assert all(R.row("limiter", c, k)["latency"] == R.row("limiter", c, k)["lookahead"] for k in range(len(c["calls"]))), c["name"]
    # ALR really acts where it is on, and the gain really is a limiter's
    for c in lim:
        on = [R.row("limiter", c, k)["envelope"] for k in range(len(c["calls"]))]
        if int(c["settings"][9]) and not c["events"]:
            assert all(e > 0 for e in on), c["name"]
        g = c["out"][0]
        assert np.isfinite(g).all() and g.min() < 0.9 and g.max() <= 1.0, c["name"]
    # chunks are counted from a call's first sample: the same input in other cuts is another result, so each cut is recorded
    one, cuts = lim[gv.LIM_GENERAL], lim[gv.LIM_GENERAL + 1:]
    differ = [int(np.count_nonzero(R.bits(one["out"][0]) != R.bits(cut["out"][0]))) for cut in cuts]
    print("long case: samples that differ from the single call's, per cut %s: %s" % (gv.LONG_CUTS, differ))
    assert differ[0] > 0 and differ[1] > 0 and differ[2] == 0, differ


def test_limiter_cases_meet_every_limit_of_attack_and_release(data):
    """init_sat / init_exp / init_line (Limiter.cpp:278-394) limit attack to [8, nLookahead] and release to [8, 2 nLookahead]
    (init_sat takes release from the limited attack, :284).  From the recorded settings and events the times in samples, from
    the recorded fields what became of them: per family each limit is met from just outside (within 5 samples of the
    look-ahead, within one look-ahead of twice it) and from far outside, and a look-ahead lowered under the attack as well."""
    met = {}
    for c in data["limiter"]:
        s = R.settings(c)
        sr, att, rel = int(s["sample_rate"]), s["attack"], s["release"]
        for k in range(len(c["calls"])):
            for name, a in R.events_before(c, k):
                sr = a[0] if name == "set_sample_rate" else sr
                att = f32(a[0]) if name == "set_attack" else att
                rel = f32(a[0]) if name == "set_release" else rel
            r = R.row("limiter", c, k)
            la, family = r["lookahead"], ("hermite", "exp", "line")[r["mode"] // 4]
            raw_a, raw_r = int(lr.millis_to_samples(sr, att)), int(lr.millis_to_samples(sr, rel))
            got_a, got_r = r["middle"], r["release"] - r["middle"] - 1
            lowered = any(name == "set_lookahead" for j in range(k + 1) for name, _ in R.events_before(c, j))
            assert got_a == min(max(raw_a, 8), la), (c["name"], k, raw_a, got_a, la)
            assert got_r == (got_a if family == "hermite" else min(max(raw_r, 8), 2 * la)), (c["name"], k, raw_r, got_r, la)
            for what, hit in (("attack just above", la < raw_a <= la + 5), ("attack far above", raw_a >= 2 * la), ("attack under 8", raw_a < 8),
                              ("attack inside", 8 < raw_a < la), ("release just above", 2 * la < raw_r <= 3 * la),
                              ("release far above", raw_r >= 4 * la), ("release under 8", raw_r < 8), ("release inside", 8 < raw_r < 2 * la),
                              ("release is not attack", raw_r != got_a), ("look-ahead lowered under the attack", lowered and raw_a > la)):
                if hit:
                    met.setdefault(family, set()).add(what)
    print({k: sorted(v) for k, v in met.items()})
    every = {"attack just above", "attack far above", "attack under 8", "attack inside"}
    assert met["hermite"] >= every | {"release is not attack"}, met["hermite"]
    for family in ("exp", "line"):
        assert met[family] >= every | {"release just above", "release far above", "release under 8", "release inside"}, (family, met[family])
    assert "look-ahead lowered under the attack" in met["line"]


def test_autogain_and_simple_cases_reach_what_they_are_for(data, restated):
    tiny = f32(1.1754944e-38)
    for c, (vca, states, counters) in zip(data["autogain"][:gv.AG_GENERAL], restated["autogain"]):
        quick, limit = bool(c["settings"][8]), bool(c["settings"][9])
        missed = [k for k in ar.expected_counters(quick, limit) if counters[k] == 0]
        assert not missed, (c["name"], missed)
    by = {c["name"]: c for c in data["autogain"]}
    assert np.all(by["all silence"]["out"] == 1.0)
    g = by["subnormal gain"]["callf"][:, gv.CALLF["autogain"].index("curr_gain")]
    assert np.all((g > 0) & (g < tiny)), g
    assert np.isnan(by["one NaN"]["inputs"][1]).sum() == 1 and np.isnan(by["one NaN"]["out"]).any()
    assert np.isposinf(by["one +Inf"]["inputs"][1]).sum() == 1
    # both switches on, the quick amplifier off, both off, both on again
    flags = [int(by["setters between the calls"]["calli"][k][0]) & (ar.F_QUICK_AMP | ar.F_MAX_GAIN) for k in range(4)]
    assert flags == [6, 4, 0, 6], flags
    # the surge flags are up at a cut: a call ends inside a surge
    assert any(int(c["calli"][k][1]) & (ar.F_SURGE_UP | ar.F_SURGE_DOWN) for c in data["autogain"][:gv.AG_GENERAL] for k in range(len(c["calls"]) - 1))

    for c in data["simple"][:gv.SAG_GENERAL]:
        lo, hi = c["settings"][4], c["settings"][5]
        assert (c["out"][0] == lo).any() and (c["out"][0] == hi).any(), c["name"]
    by = {c["name"]: c for c in data["simple"]}
    c = by["a level at the threshold"]
    assert np.all(c["inputs"][0][150:160] * c["out"][0][149:159] == c["settings"][3]) and np.all(c["out"][0][150:160] == c["out"][0][149])
    a, b = by["limit setters: min, max, both"], by["limit setters: max, min, both"]
    assert R.same(a["inputs"][0], b["inputs"][0]) and a["after"][0] != b["after"][0] and a["after"][2] != b["after"][2]
    d = by["decay into subnormals"]["out"][0]
    assert np.count_nonzero((d > 0) & (d < tiny)) > 20
    assert np.isnan(by["one NaN"]["inputs"][0]).sum() == 1 and np.isposinf(by["one +Inf"]["inputs"][0]).sum() == 1


# ---- the restatements fed the reference's parameters ------------------------------------------------------------------------
def test_limiter_restatement_gives_the_references_gain_and_state(data, restated):
    most = 0
    for c, (gain, heads, envs, patches, _) in zip(data["limiter"], restated["limiter"]):
        bad = np.flatnonzero(R.bits(gain) != R.bits(c["out"][0]))
        assert bad.size == 0, (c["name"], "first difference at", int(bad[0]), gain[bad[0]], c["out"][0][bad[0]], bad.size)
        for k in range(len(c["calls"])):
            r = R.row("limiter", c, k)
            assert heads[k] == r["head"], (c["name"], k, heads[k], r["head"])
            assert R.same(envs[k], r["envelope"]), (c["name"], k, envs[k], r["envelope"])
        if "dense" in c["name"]:
            most = max(max(p) for p in patches)
    print("most patches in a chunk of the dense case: %d" % most)
    assert most > lr.PEAKS_MAX, most


@pytest.mark.parametrize("scalar", [False, True])
def test_autogain_restatement_gives_the_references_gain_and_state(data, restated, scalar):
    for c, (vca, states, _) in zip(data["autogain"], restated["autogain_level" if scalar else "autogain"]):
        want = c["out"][1 if scalar else 0]
        assert R.same(vca, want), (c["name"], np.flatnonzero(R.bits(vca) != R.bits(want))[:4])
        if scalar:
            continue                                # the second object's state is not recorded
        for k in range(len(c["calls"])):
            r = R.row("autogain", c, k)
            assert R.same(states[k][0], r["curr_gain"]) and R.same(states[k][1], r["out_gain"]) and states[k][2] == r["flags"], \
                (c["name"], k, states[k], r["curr_gain"], r["out_gain"], r["flags"])


def test_simple_autogain_restatement_gives_the_references_gain_and_state(data, restated):
    for c, (dst, states, after) in zip(data["simple"], restated["simple"]):
        assert R.same(dst, c["out"][0]), (c["name"], np.flatnonzero(R.bits(dst) != R.bits(c["out"][0]))[:4])
        for k in range(len(c["calls"])):
            assert R.same(states[k], R.row("simple", c, k)["curr_gain"]), (c["name"], k)
        assert R.same(after, c["after"]), (c["name"], after, c["after"])


# ---- update_settings() / update() -----------------------------------------------------------------------------------------
def test_host_limiter_parameters_and_table_are_the_references(mi, data):
    """mi_limiter_compute_params on the settings ahead of every call: integer fields equal, float fields bit for bit; and
    mi_limiter_compute_patch the float32 formula of apply_*_patch on the RECORDED coefficients, bit for bit."""
    LB = mi.LimiterBank
    sets = 0
    for c in data["limiter"]:
        seen = R.run_limiter(dict(c, inputs=[np.zeros_like(c["inputs"][0])]), R.recorded_limiter(c))[4]
        for k, s in seen:
            want = R.limiter_params(c, k)
            got = LB.compute_params(**{n: (v.item() if hasattr(v, "item") else v) for n, v in s.items()})
            assert R.all_same(got, want), (c["name"], k, got, want)
            assert got["lookahead"] == R.row("limiter", c, k)["latency"]
            table = R.limiter_table(want)
            patch = LB.compute_patch(got)
            assert np.array_equal(R.bits(patch), R.bits(table)), (c["name"], k, np.flatnonzero(R.bits(patch) != R.bits(table))[:4])
            sets += 1
    print("limiter: %d parameter sets and tables bit-identical to the reference's over %d cases" % (sets, len(data["limiter"])))
    assert sets >= len(data["limiter"])


def test_host_autogain_parameters_are_the_references(mi, data):
    n = 0
    for c in data["autogain"]:
        for k, s in enumerate(R.autogain_settings_at(c)):
            got, want = mi.AutoGainBank.compute_params(**s), R.autogain_params(c, k)
            assert R.all_same(got, want), (c["name"], k, got, want)
            n += 1
    print("autogain: %d parameter sets bit-identical to the reference's" % n)


def test_host_simple_autogain_parameters_are_the_references(mi, data):
    n = 0
    for c in data["simple"]:
        for k, s in enumerate(R.simple_settings_at(c)):
            got, want = mi.SimpleAutoGainBank.compute_params(**s), R.simple_params(c, k)
            assert R.all_same(got, want), (c["name"], k, got, want)
            n += 1
    print("simple autogain: %d parameter sets bit-identical to the reference's" % n)
