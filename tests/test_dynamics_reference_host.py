"""The numpy restatements (compressor_ref, expander_ref, gate_ref, dynproc_ref) and the host code of update_settings()
(mi_*_compute_params) against the REFERENCE'S OWN Compressor, Expander, Gate and DynamicProcessor: their .cpp text compiled
unmodified (oracle/Makefile -> oracle/_ref/dyn_ref) and run by tests/golden/make_dynamics_vectors.py, whose results are stored in
tests/golden/dynamics_ref_vectors.npz.  A reading of the reference that the restatement and the kernel share is caught here;
tests/test_dynamics_reference_gpu.py holds the kernels and the C++ classes to the same file."""
import os

import numpy as np
import pytest

import dynamics_reference as R
from dynamics_reference import mv

f32 = np.float32
T = mv.T


@pytest.fixture(scope="module")
def data():
    return R.load()


@pytest.fixture(scope="module")
def followed(data):
    """Every case with its restatement's follower fed the reference's recorded parameters: computed once."""
    out = {}
    for cls in R.CLASSES:
        out[cls] = [R.follow(c, R.params_dict(cls, c["paramf"], c["parami"])) for c in data[cls]]
    return out


def test_stored_vectors_are_what_the_reference_gives_today():
    """Freshness: where the reference binary exists the generator runs again and must give the committed bytes."""
    if not os.path.exists(mv.DYN_REF):
        pytest.skip("no oracle/_ref/dyn_ref: the reference tree is not on this machine")
    with open(mv.OUT, "rb") as f:
        stored = f.read()
    assert mv.build_bytes() == stored, "tests/golden/dynamics_ref_vectors.npz is stale: python tests/golden/make_dynamics_vectors.py"


def test_stored_vectors_are_small_and_complete(data):
    assert os.path.getsize(mv.OUT) < 400 * 1024
    for cls in R.CLASSES:
        names = [c["name"] for c in data[cls]]
        assert names[:mv.GENERAL] == ["channel %d" % (mv.FIRST[cls] + ch) for ch in range(mv.GENERAL)]
        assert all(c["calls"] == list(mv.CALLS) and len(c["x"]) == 3 * T + 7 for c in data[cls][:mv.GENERAL])
        assert len({int(c["settings"][0]) for c in data[cls][:mv.GENERAL]}) == 3                    # sample rates
        for special in ("subnormals", "one +Inf", "one NaN", "written state", "re-arm on equality"):
            assert names.count(special) == 1, (cls, special)
        lad = data[cls][0]["ladder"]
        assert lad.min() < 0 and (lad == 0).any() and np.abs(lad[lad != 0]).min() <= 1.01e-6 and lad.max() >= 15.8      # -120 .. +24 dB
    modes = lambda cls, k: {int(c["settings"][mv.SETTINGS[cls].index(k)]) for c in data[cls][:mv.GENERAL]}
    assert modes("compressor", "mode") == {0, 1, 2} and modes("expander", "mode") == {0, 1}
    boost = [c["settings"][4] for c in data["compressor"][:mv.GENERAL] if int(c["settings"][1]) == 2]
    assert min(boost) < 1.0 <= max(boost)
    assert {int(c["parami"][0] > 0) for c in data["gate"][:mv.GENERAL]} == {0, 1}                   # with and without hold
    assert {int(c["parami"][1]) for c in data["dynproc"][:mv.GENERAL]} >= {0, 1, 4}                 # splines
    assert {int(c["parami"][2]) for c in data["dynproc"][:mv.GENERAL]} >= {1, 3}                    # reaction ranges


# ---- conditions on the inputs, read from the reference's recorded results -------------------------------------------------
def test_gate_cases_cross_where_they_are_meant_to(data):
    where = {0: set(), 1: set()}                    # direction -> crossing samples, over the cases of two calls of 300 / 475
    held_crossings = twice = 0
    for c in data["gate"]:
        w = R.written(c)
        before = np.concatenate([[0], c["which"][:-1]])
        hold_before = np.concatenate([[0], c["holds"][:-1]]).astype(np.int64)
        if w is not None:
            before[c["calls"][0]], hold_before[c["calls"][0]] = w[3], w[2]
        at = np.flatnonzero(c["which"] != before)
        if c["calls"] == list(mv.CALLS):
            for i in at:
                where[int(c["which"][i])].add(int(i))
        held_crossings += int(np.count_nonzero(hold_before[at] > 0))
        twice += int(np.count_nonzero(hold_before[at] - c["holds"][at].astype(np.int64) == 2))     # a held sample stepped twice
    for direction in (0, 1):
        assert where[direction] & {T - 1, T}, (direction, sorted(where[direction]))
    assert (where[0] | where[1]) & {mv.CALLS[0] - 1}
    assert held_crossings > 0 and twice > 0, (held_crossings, twice)


def test_special_cases_reach_what_they_are_for(data):
    tiny = f32(1.1754944e-38)
    for cls in R.CLASSES:
        by = {c["name"]: c for c in data[cls]}
        e = np.abs(by["subnormals"]["env"])
        assert np.count_nonzero((e > 0) & (e < tiny)) > 20, cls
        assert np.isposinf(by["one +Inf"]["x"]).sum() == 1 and np.isnan(by["one NaN"]["x"]).sum() == 1
        assert len(by["one +Inf"]["x"]) - int(np.flatnonzero(np.isposinf(by["one +Inf"]["x"]))[0]) == 201
        assert not np.isfinite(by["one +Inf"]["env"]).all() and np.isnan(by["one NaN"]["env"]).any(), cls
        assert R.written(by["written state"]) is not None
        # the re-arm on equality: the envelope stands still over the returning sample, which is not below it, and the counter
        # that five held samples had taken from 24 to 19 is 0 only after 24 more, at the first call's end, the envelope unmoved
        c = by["re-arm on equality"]
        e = R.bits(c["env"])
        assert c["parami"][0] == 24 and c["calls"][0] == 150
        assert e[119] == e[125] == e[149] and c["x"][125] >= c["env"][124] and np.all(c["x"][126:150] < c["env"][125])
        assert c["states"][0][2] == 0 and c["states"][0][0] == e[149] and e[150] != e[149]


# ---- the followers ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", R.CLASSES)
def test_follower_fed_the_references_parameters_gives_its_envelope_and_state(data, followed, cls):
    total = {}
    for c, (env, which, states, taken) in zip(data[cls], followed[cls]):
        what = (cls, c["name"])
        assert R.same(env, c["env"]), what + (np.flatnonzero(R.bits(env) != R.bits(c["env"]))[:4],)
        assert np.array_equal(states, c["states"]), what + (states, c["states"])
        if cls == "gate":
            assert np.array_equal(which, c["which"]), what + (np.flatnonzero(which != c["which"])[:4],)
        for k, v in taken.items():
            total[k] = total.get(k, 0) + v
    print(cls, total)
    if cls == "gate":
        assert total["toggles"] > 0 and total["restep_hold"] > 0 and total["capped"] == 0, total
    else:
        assert all(total[k] > 0 for k in (R.dr.BRANCHES if cls == "dynproc" else R.cr.BRANCHES)), total


def test_gate_transcription_agrees_too(data):
    """gate_ref.process_transcribed (the reference's loops statement for statement) on the recorded cases."""
    for c in data["gate"]:
        p = R.params_dict("gate", c["paramf"], c["parami"])
        st, pos = (f32(0), f32(0), 0, 0), 0
        with np.errstate(all="ignore"):
            for ci, n in enumerate(c["calls"]):
                env, which, st = R.gr.process_transcribed(c["x"][pos:pos + n], st, p["tau_attack"], p["tau_release"], p["hold"],
                                                          p["k"][0]["end"], p["k"][1]["start"])
                assert R.same(env, c["env"][pos:pos + n]) and np.array_equal(which, c["which"][pos:pos + n]), (c["name"], ci)
                assert [int(R.bits(st[0])[0]), int(R.bits(st[1])[0]), st[2], st[3]] == [int(v) for v in c["states"][ci]], (c["name"], ci)
                pos += n
                if ci == 0 and R.written(c) is not None:
                    st = R.written(c)


# ---- the gains ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", R.CLASSES)
def test_references_gain_lies_within_the_derived_bound(data, cls):
    """What the reference's process() wrote, and its scalar overload on the same envelope, against the restatement's float64
    curve under the restatement's derived bound: the bound was derived for the kernel and meets here the arithmetic it models."""
    worst = 0.0
    for c in data[cls]:
        p = R.params_dict(cls, c["paramf"], c["parami"])
        finite = np.isfinite(c["env"])
        for got, scalar in ((c["out"], False), (c["sgain"], True)):
            kind = "gain" if not scalar else R.GAIN_KIND[cls]
            g64, bound, exact = R.expected(cls, kind, c["env"], p, which=c.get("which"), scalar=scalar)
            ok, err = R.judge(got, g64, bound, exact)
            assert np.all(ok[finite]), (cls, c["name"], scalar, int(np.count_nonzero(~ok[finite])), float(err[finite].max()))
            with np.errstate(all="ignore"):
                worst = max(worst, float(np.max(np.where(finite & (bound > 0), err / np.maximum(bound, 1e-9), 0.0))))
        # a NaN or infinite envelope: the float32 restatement gives NaN where the reference does and its bits elsewhere
        if not finite.all():
            mod = {"compressor": R.cr, "expander": R.er, "gate": R.gr, "dynproc": R.dr}[cls]
            with np.errstate(all="ignore"):
                args = (c["env"][None, :], c["which"][None, :], [p]) if cls == "gate" else (c["env"][None, :], [p])
                g32 = np.asarray(mod.gain32(*args), f32)[0]
            assert R.same(g32[~finite], c["out"][~finite]), (cls, c["name"], g32[~finite][:4], c["out"][~finite][:4])
    print("%s: the reference's gain uses at most %.3f of the bound" % (cls, worst))
    assert worst > 0.0 or cls == "gate"


@pytest.mark.parametrize("cls", R.CLASSES)
def test_references_curves_lie_within_the_derived_bound(data, cls):
    """curve(), reduction() / amplification() and model() over the level ladder, array and scalar forms."""
    worst = 0.0
    for c in data[cls][:mv.GENERAL]:
        p = R.params_dict(cls, c["paramf"], c["parami"])
        for k, name in enumerate(mv.CURVES[cls]):
            for scalar in (False, True):
                g64, bound, exact = R.expected(cls, name, c["ladder"], p, scalar=scalar)
                ok, err = R.judge(c["curves"][k, int(scalar)], g64, bound, exact)
                assert np.all(ok), (cls, c["name"], name, scalar, c["ladder"][~ok][:4], float(err.max()))
                worst = max(worst, float(np.max(np.where(bound > 0, err / np.maximum(bound, 1e-9), 0.0))))
    print("%s: the reference's curves use at most %.3f of the bound" % (cls, worst))
    assert worst > 0.0


# ---- update_settings() --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", R.CLASSES)
def test_host_update_settings_gives_the_references_parameters(mi, data, cls):
    """mi_*_compute_params on the recorded settings: integer fields equal, float fields bit for bit (both are float32 code on
    this machine's libm: a difference is an operation-order difference of csrc/host/*.cpp)."""
    bank = {"compressor": mi.CompressorBank, "expander": mi.ExpanderBank, "gate": mi.GateBank, "dynproc": mi.DynamicProcessorBank}[cls]
    identical = fields = 0
    differing = []
    for c in data[cls]:
        f, i = R.flat(cls, bank.compute_params(**R.settings(c)))
        assert np.array_equal(i, c["parami"]), (cls, c["name"], i, c["parami"])
        eq = R.bits(f) == R.bits(c["paramf"])
        identical, fields = identical + int(eq.sum()), fields + eq.size
        differing += [(c["name"], mv.PARAMF[cls][j], float(f[j]), float(c["paramf"][j])) for j in np.flatnonzero(~eq)]
    print("%s: %d of %d float fields bit-identical to the reference's over %d cases" % (cls, identical, fields, len(data[cls])))
    assert not differing, differing
