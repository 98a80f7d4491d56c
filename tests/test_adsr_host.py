"""lsp::dspu::ADSREnvelope without a device: tests/adsr_ref.py against every recorded case of the reference's own class (bit for bit
outside EXP segments; inside them with the float64 exp rounded once or one of its two float32 neighbours, and the share of samples
that need a neighbour capped), the library's designer (mi_adsr_settings_*) against the recorded record, nFlags and clamped times,
the host evaluation of the scalar process(float), the refusals, what the recorded cases cover, and the six mutations of the
restatement that the recording has to catch."""
import ctypes
import importlib
import json
import os
import sys

import numpy as np
import pytest

import adsr_ref as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, GOLDEN)
import make_adsr_vectors as gen  # noqa: E402

f32, u32 = np.float32, np.uint32
REFERENCE = os.path.join(os.path.dirname(ROOT), "reference")
NEIGHBOUR_CAP = 0.005                                       # ten times the 0.046 % measured on the reference alone


@pytest.fixture(scope="module")
def recorded():
    return gen.load()


def same_bits(a, b):
    """Bit for bit; a NaN counts as a NaN."""
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    return (a.view(u32) == b.view(u32)) | (np.isnan(a) & np.isnan(b))


def run_case(x, c, shift=0, env=None):
    """The restatement on a recorded case: (out, EXP mask, stages, the designed Envelope)."""
    e = A.design(c["ops"]) if env is None else env
    src = x[c["tsig"], :c["n"]] if c["tsig"] >= 0 else None
    data = x[c["dsig"], :c["n"]] if c["dsig"] >= 0 else None
    out, exp, stage = e.run(c["kind"], n=c["n"], src=src if c["kind"] in (A.PROCESS, A.PROCESS_MUL) else data, dst=data,
                            start=c["start"], step=c["step"], first=c["first"], shift=shift)
    return out, exp, stage, e


def matches(x, c):
    """(every sample agrees by the rule, EXP samples, EXP samples that need a neighbour)"""
    out, exp, stage, e = run_case(x, c)
    ok = same_bits(out, c["out"])
    if not np.all(ok | exp):
        return False, int(exp.sum()), 0
    need = exp & ~ok
    if need.any():
        near = np.zeros_like(ok)
        for shift in (-1, 1):
            near |= same_bits(run_case(x, c, shift, e)[0], c["out"])
        if not np.all(near[need]):
            return False, int(exp.sum()), int(need.sum())
    return True, int(exp.sum()), int(need.sum())


def test_restatement_equals_every_recorded_case(recorded):
    x, cases = recorded
    assert len(cases) >= 200
    total = needing = 0
    for c in cases:
        ok, n_exp, n_need = matches(x, c)
        assert ok, c["name"]
        total, needing = total + n_exp, needing + n_need
    share = needing / total
    print("EXP samples: %d, of which %d (%.4f %%) match with a float32 neighbour of the rounded-once exp" % (total, needing, 100 * share))
    assert total > 10000 and share <= NEIGHBOUR_CAP


def used_slots(record):
    """Which of the 40 recorded words a comparison looks at: everything but the parameters of empty segments (a segment of zero
    length designs to Inf, NaN or whatever the elimination leaves, and is never evaluated) and the union's undesigned floats."""
    e = A.Envelope()
    keep = np.ones(40, bool)
    as_float = np.asarray(record, np.int64).astype(u32).view(f32)
    t, hold = [as_float[9 * p] for p in range(4)], as_float[36]
    flags = int(record[39])
    ends = {A.ATTACK: (f32(0), t[A.ATTACK]), A.DECAY: (hold if flags & A.USE_HOLD else t[A.ATTACK], t[A.DECAY]),
            A.SLOPE: (t[A.DECAY], t[A.SLOPE]) if flags & A.USE_BREAK else None, A.RELEASE: (t[A.RELEASE], f32(1))}
    for p in range(4):
        e.fn[p] = int(record[9 * p + 2])
        used = e.used_params(p) if ends[p] is not None and ends[p][0] < ends[p][1] else 0
        keep[9 * p + 3 + used:9 * p + 9] = False
    return keep


def test_restatement_designs_the_recorded_record(recorded):
    x, cases = recorded
    for c in cases:
        e = A.design(c["ops"])
        assert e.flags == c["flags_before"], c["name"]
        e.update_settings()
        keep = used_slots(c["record"])
        assert np.array_equal(e.record()[keep], c["record"][keep]), (c["name"], e.record(), c["record"])


def c_design(mi, ops):
    capi = importlib.import_module("lsp-dsp-units_amd.capi")
    s = capi.AdsrSettings()
    assert mi.lib.mi_adsr_settings_init(ctypes.byref(s)) == 0
    for op in ops:
        if int(op[0]) == A.UPDATE:
            assert mi.lib.mi_adsr_settings_update(ctypes.byref(s)) == 0
        else:
            assert mi.lib.mi_adsr_settings_set(ctypes.byref(s), int(op[0]), op[1], op[2], op[3]) == 0, mi.lib.mi_dspu_last_error()
    return s


def c_record(s):
    out = []
    for k in range(4):
        cv = s.curve[k]
        out += [int(f32(cv.time).view(u32)), int(f32(cv.curve).view(u32)), int(cv.function)] + [int(f32(v).view(u32)) for v in cv.params]
    return np.array(out + [int(f32(v).view(u32)) for v in (s.hold_time, s.break_level, s.sustain_level)] + [int(s.flags)], np.int64)


def test_c_designer_equals_the_recorded_record(mi, recorded):
    x, cases = recorded
    for c in cases:
        s = c_design(mi, c["ops"])
        assert s.flags == c["flags_before"], c["name"]
        assert mi.lib.mi_adsr_settings_update(ctypes.byref(s)) == 0
        keep = used_slots(c["record"])
        assert np.array_equal(c_record(s)[keep], c["record"][keep]), (c["name"], c_record(s), c["record"])
        assert not s.flags & A.RECONFIGURE


def test_host_process_is_the_restatement(mi, recorded):
    """mi_adsr_settings_process, the class's scalar process(float): the restatement's bits, EXP included (the same rounded-once exp)."""
    x, cases = recorded
    v = ctypes.c_float()
    done = 0
    for c in cases:
        if c["kind"] != A.PROCESS or c["n"] > 700:
            continue
        s = c_design(mi, c["ops"])
        if s.flags & A.RECONFIGURE:                             # MI_ESTATE: not updated yet
            assert mi.lib.mi_adsr_settings_process(ctypes.byref(s), 0.5, ctypes.byref(v)) == -5
        mi.lib.mi_adsr_settings_update(ctypes.byref(s))
        t = x[c["tsig"], :c["n"]]
        want = run_case(x, c)[0]
        got = np.zeros(c["n"], f32)
        for i in range(0, c["n"], 3):
            assert mi.lib.mi_adsr_settings_process(ctypes.byref(s), ctypes.c_float(float(t[i])), ctypes.byref(v)) == 0
            got[i] = v.value
        assert np.all(same_bits(got[::3], want[::3])), c["name"]
        done += 1
    assert done > 50


def test_hermite_designs(mi):
    rng = np.random.default_rng(7)
    p = np.zeros(5, f32)
    for _ in range(200):
        a = rng.uniform(-1, 1, 8).astype(f32)
        a[3] = a[0] + abs(a[3]) + f32(0.01)
        a[6] = (a[0] + a[3]) * f32(0.5)
        assert mi.lib.mi_interpolation_hermite_cubic(p.ctypes.data, *[ctypes.c_float(float(v)) for v in a[:6]]) == 0
        assert np.all(same_bits(p[:4], A.hermite_cubic(*a[:6])))
        assert mi.lib.mi_interpolation_hermite_quadro(p.ctypes.data, *[ctypes.c_float(float(v)) for v in a]) == 0
        assert np.all(same_bits(p, A.hermite_quadro(*a)))
    assert mi.lib.mi_interpolation_hermite_cubic(None, *[ctypes.c_float(0)] * 6) == -1


def test_refusals_and_getters_after_a_refusal(mi):
    capi = importlib.import_module("lsp-dsp-units_amd.capi")
    lib = mi.lib
    s = c_design(mi, gen.op_rows(gen.base(A.CUBIC, 0.3)))
    before = bytes(s)
    nan = float("nan")
    for setter in range(A.SET_RELEASE + 1):
        assert lib.mi_adsr_settings_set(ctypes.byref(s), setter, nan, 0.0, 0.0) == -1, setter
    for setter in (A.SET_ATTACK, A.SET_DECAY, A.SET_SLOPE, A.SET_RELEASE):
        assert lib.mi_adsr_settings_set(ctypes.byref(s), setter, 0.5, nan, 0.0) == -1
        assert lib.mi_adsr_settings_set(ctypes.byref(s), setter, 0.5, 0.5, nan) == -1
        assert lib.mi_adsr_settings_set(ctypes.byref(s), setter, 0.5, 0.5, 1.5) == -1         # no integer
        assert lib.mi_adsr_settings_set(ctypes.byref(s), setter, 0.5, 0.5, -1.0) == -1
    for setter in (A.SET_HOLD, A.SET_BREAK):
        assert lib.mi_adsr_settings_set(ctypes.byref(s), setter, 0.5, nan, 0.0) == -1
    assert lib.mi_adsr_settings_set(ctypes.byref(s), A.SET_RELEASE + 1, 0.5, 0.0, 0.0) == -1
    assert lib.mi_adsr_settings_set(ctypes.byref(s), A.SET_ATTACK_FUNCTION, 0.5, 0.0, 0.0) == -1
    assert bytes(s) == before, "a refused setter changed the settings"
    assert lib.mi_adsr_settings_init(None) == -1 and lib.mi_adsr_settings_update(None) == -1
    assert lib.mi_adsr_settings_set(None, 0, 0.0, 0.0, 0.0) == -1
    v = ctypes.c_float()
    assert lib.mi_adsr_settings_process(None, 0.5, ctypes.byref(v)) == -1 and lib.mi_adsr_settings_process(ctypes.byref(s), 0.5, None) == -1
    # +-Inf are values like any other: clamped
    assert lib.mi_adsr_settings_set(ctypes.byref(s), A.SET_SUSTAIN_LEVEL, float("inf"), 0.0, 0.0) == 0 and s.sustain_level == 1.0
    assert lib.mi_adsr_settings_set(ctypes.byref(s), A.SET_SUSTAIN_LEVEL, float("-inf"), 0.0, 0.0) == 0 and s.sustain_level == 0.0
    # a function outside the enum is taken and designs as NONE does
    t = c_design(mi, gen.op_rows(gen.base(77, 0.3)))
    u = c_design(mi, gen.op_rows(gen.base(A.NONE, 0.3)))
    lib.mi_adsr_settings_update(ctypes.byref(t)), lib.mi_adsr_settings_update(ctypes.byref(u))
    for k in range(4):
        assert t.curve[k].function == 77 and list(t.curve[k].params)[:3] == list(u.curve[k].params)[:3]
    for tv in (0.05, 0.3, 0.5, 0.9):
        a, b = ctypes.c_float(), ctypes.c_float()
        lib.mi_adsr_settings_process(ctypes.byref(t), tv, ctypes.byref(a)), lib.mi_adsr_settings_process(ctypes.byref(u), tv, ctypes.byref(b))
        assert a.value == b.value
    assert ctypes.sizeof(capi.AdsrSettings) == 160


def test_the_recorded_cases_cover_what_they_are_for(recorded):
    x, cases = recorded
    seen_fn = set()                                         # (part, function) evaluated in a non-empty segment
    seen_stage = {k: set() for k in range(5)}
    special_t, special_d = gen.special_times(), gen.special_data()
    seen_t, seen_d = set(), set()
    kt_signs = set()
    for c in cases:
        out, exp, stage, e = run_case(x, c)
        for st, part in ((A.ST_ATTACK, A.ATTACK), (A.ST_DECAY, A.DECAY), (A.ST_SLOPE, A.SLOPE), (A.ST_RELEASE, A.RELEASE)):
            if np.any(stage == st):
                seen_fn.add((part, e.fn[part]))
                if e.fn[part] == A.EXP:
                    kt_signs.add((float(np.sign(f32(0.5) - e.curve[part])), float(e.params[part][1]) == 0.0))
        seen_stage[c["kind"]] |= set(np.unique(stage).tolist())
        if c["tsig"] == gen.ROW_SPECIAL:
            seen_t |= set(x[c["tsig"], :c["n"]].view(u32).tolist())
            if c["dsig"] >= 0:
                seen_d |= set(zip(x[c["tsig"], :c["n"]].view(u32).tolist(), x[c["dsig"], :c["n"]].view(u32).tolist()))
    assert seen_fn == {(p, f) for p in range(4) for f in range(6)}
    for kind in range(5):
        assert seen_stage[kind] == set(range(8)), (kind, seen_stage[kind])
    assert set(special_t.view(u32).tolist()) <= seen_t
    outside = [t for t in special_t if not (t > 0 and t < 1)]
    assert len(outside) >= 10
    for t in outside:                                       # every special datum against every time outside (0, 1)
        for d in special_d:
            assert (int(f32(t).view(u32)), int(f32(d).view(u32))) in seen_d
    assert kt_signs >= {(1.0, False), (-1.0, False), (0.0, True)}
    by = {c["name"]: c for c in cases}
    assert by["the same values again"]["flags_before"] & A.RECONFIGURE == 0, "a setter that changes nothing raised F_RECONFIGURE"
    assert by["constructed"]["flags_before"] == A.RECONFIGURE
    pushed = by["times out of order"]["record"]
    times = np.array([pushed[0], pushed[36], pushed[9], pushed[18], pushed[27]], np.int64).astype(u32).view(f32)
    assert np.all(np.diff(times) >= 0) and times[1] == f32(0.5)
    long = by["generate long"]
    assert long["first"] == 1 << 24 and long["n"] == gen.N and len(np.unique(long["out"])) > 1000
    neg = [c for c in cases if c["kind"] >= A.GENERATE and c["step"] < 0]
    assert len(neg) >= 20
    assert os.path.getsize(gen.OUT) <= 329 * 1024


@pytest.mark.parametrize("mutation", A.MUTATIONS)
def test_the_recording_catches_a_mutation_of_the_restatement(recorded, mutation):
    x, cases = recorded
    try:
        A.MUTATION = mutation
        caught = [c["name"] for c in cases if not matches(x, c)[0]]
    finally:
        A.MUTATION = None
    assert caught, mutation


@pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE, "src", "main", "util")), reason="the reference tree is not here")
def test_generator_reproduces_the_stored_file():
    data, dump, names = gen.build(REFERENCE)
    assert data == open(gen.OUT, "rb").read()
    assert dump == json.load(open(os.path.join(GOLDEN, "adsr_dump_keys.json")))
    assert names == json.load(open(os.path.join(GOLDEN, "adsr_public_names.json")))
