"""Velvet without a device: the numpy restatement (tests/velvet_ref.py) against the reference's recorded outputs and state words, bit
for bit; the generator against the recorded cases where the reference tree exists; the 256-sample segmentation of a call with a
source; the setters' clamps and the refusals of the C ABI that need no device."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

import noise_ref as R
import velvet_ref as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_velvet_vectors as gen  # noqa: E402

f32, u32, u64 = np.float32, np.uint32, np.uint64
REFERENCE = os.path.join(os.path.dirname(ROOT), "reference")
EINVAL, ENODEV, ESTATE = -1, -3, -5
GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def recorded():
    return gen.load()


@pytest.fixture(scope="module")
def restated(recorded):
    """Every recorded case through the restatement: once."""
    return [V.run_case(c) for c in recorded]


def test_restatement_equals_the_references_recorded_outputs(recorded, restated):
    assert len(recorded) >= 150
    for c, (out, unit) in zip(recorded, restated):
        bad = np.nonzero(~R.same(c["out"], out))[0]
        assert bad.size == 0, (c["name"], bad[:5], c["out"][bad[:5]], out[bad[:5]])
        assert np.array_equal(unit.words(), c["words"]), (c["name"], unit.words(), c["words"])


@pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE, "src", "main", "noise")), reason="the reference tree is not here")
def test_the_generator_still_makes_the_recorded_cases(recorded):
    cs, src, got, keys, names = gen.run_reference(REFERENCE)
    assert [c["name"] for c in cs] == [c["name"] for c in recorded]
    for m, g, c in zip(cs, got, recorded):
        assert np.array_equal(m["ops"], c["ops"]) and np.array_equal(R.bits(src), R.bits(c["src"])), m["name"]
        assert R.same(g["out"], c["out"]).all() and np.array_equal(g["words"], c["words"]), m["name"]
    gen.check_branches(cs, src, got)
    dump, names = gen.inventories(keys, names)
    assert json.load(open(os.path.join(GOLDEN, "velvet_dump_keys.json"))) == dump
    assert json.load(open(os.path.join(GOLDEN, "velvet_public_names.json"))) == names


def test_the_committed_operation_lists_are_the_generators(recorded):
    made, src = gen.cases(), gen.source_row()
    assert [m["name"] for m in made] == [c["name"] for c in recorded]
    for m, c in zip(made, recorded):
        assert np.array_equal(m["ops"], c["ops"]) and np.array_equal(R.bits(src), R.bits(c["src"])), m["name"]


def test_recorded_cases_cover_what_the_issue_lists(recorded):
    combos, widths, deltas, bits, calls, whats, amps, offs, probs = set(), set(), set(), set(), set(), set(), set(), set(), set()
    for c in recorded:
        unit = V.Velvet()
        for op in c["ops"]:
            what = int(op[0])
            if what in V.PROCESS_OPS:
                calls.add(int(op[1]))
                whats.add(what)
                combos.add((unit.type, unit.core, unit.crush))
                widths.add(float(unit.width))
                if unit.crush:
                    probs.add(float(unit.prob))
                if unit.type == V.ARN:
                    deltas.add(float(unit.delta))
            else:
                if what == V.SET_WIDTH: widths.add(("asked", float(op[1])))
                elif what == V.SET_DELTA: deltas.add(("asked", float(op[1])))
                elif what == V.INIT: bits.add(int(op[2]))
                elif what == R.SET_AMPLITUDE: amps.add(float(op[1]))
                elif what == R.SET_OFFSET: offs.add((float(op[1]), bool(np.signbit(op[1]))))
                V.apply(unit, op)
    assert combos >= {(t, c, k) for t in range(4) for c in (0, 1) for k in (False, True)}
    assert probs >= {0.0, 0.5, 1.0}
    assert widths >= {2.0, 2.5, 10.0, float(f32(10.7)), 64.0, 256.0, 257.0, 1000.0, ("asked", 1.0)}
    assert deltas >= {0.0, 0.5, 1.0, ("asked", -0.5), ("asked", 1.5)}
    assert bits >= {1, 2, 23, 64}
    assert calls >= {1100, 1, 3, 7, 255, 256, 257, 1023}
    assert whats == set(V.PROCESS_OPS)
    assert 0.0 in amps and np.inf in amps and any(a < 0 for a in amps)
    assert (0.0, True) in offs and any(o == (0.0, False) or o[0] > 0 for o in offs)
    src = recorded[0]["src"]
    assert np.isnan(src).any() and np.isinf(src).any() and (src == 0).any() and np.signbit(src[src == 0]).any()


@pytest.mark.parametrize("type_", range(4))
@pytest.mark.parametrize("what", [R.P_ADD, R.P_MUL])
def test_a_call_with_a_source_is_calls_of_256(type_, what):
    """process_add / process_mul with a source over n equals the same object called with 256 samples at a time -- and an overwrite
    of n does not equal overwrites of 256."""
    src = gen.source_row()

    def unit():
        u = V.Velvet()
        u.init(0x77 + type_, 23, 0x55)
        u.type, u.core, u.crush = type_, type_ % 2, type_ == V.ARN
        u.set_width(7.3)
        return u

    whole, cut, over, over_cut = unit(), unit(), unit(), unit()
    n = 1100
    a = whole.process(what, src[:n], n)
    b = np.concatenate([cut.process(what, src[at:at + 256], min(256, n - at)) for at in range(0, n, 256)])
    assert R.same(a, b).all() and np.array_equal(whole.words(), cut.words())
    c = over.process(R.P_OVERWRITE, None, n)
    d = np.concatenate([over_cut.process(R.P_OVERWRITE, None, min(256, n - at)) for at in range(0, n, 256)])
    same = R.same(c, d).all() and np.array_equal(over.words(), over_cut.words())
    assert same == (type_ == V.TRN and not over.crush)              # uncrushed TRN is one draw per sample: there alone it is the same


def test_setter_clamps_of_the_restatement_are_the_references(recorded):
    u = V.Velvet()
    for asked, want in ((1.0, 2.0), (2.0, 2.0), (-5.0, 2.0), (2.5, 2.5), (1000.0, 1000.0)):
        u.set_width(asked)
        assert u.width == f32(want)
    for asked, want in ((-0.5, 0.0), (0.0, 0.0), (0.25, 0.25), (1.0, 1.0), (1.5, 1.0)):
        u.set_delta(asked)
        u.set_crush_prob(asked)
        assert u.delta == f32(want) and u.prob == f32(want)


def test_refusals_that_need_no_device(mi):
    capi = sys.modules[mi.__name__ + ".capi"]
    lib = mi.lib
    assert ctypes.sizeof(capi.VelvetState) == 144 and capi.VelvetState.mls.offset == 72
    h = ctypes.c_void_p(1)
    assert lib.mi_velvet_bank_create(None, 1) == EINVAL
    assert lib.mi_velvet_bank_create(ctypes.byref(h), 0) == EINVAL and not h.value
    s = capi.VelvetState()
    for entry, args in ((lib.mi_velvet_bank_init, (None, 0, 1, 23, 1)), (lib.mi_velvet_bank_init_time, (None, 0)),
                        (lib.mi_velvet_bank_set_core_type, (None, 0, 1)), (lib.mi_velvet_bank_set_velvet_type, (None, 0, 1)),
                        (lib.mi_velvet_bank_set_velvet_window_width, (None, 0, 10.0)), (lib.mi_velvet_bank_set_delta_value, (None, 0, 0.5)),
                        (lib.mi_velvet_bank_set_crush_probability, (None, 0, 0.5)), (lib.mi_velvet_bank_set_amplitude, (None, 0, 1.0)),
                        (lib.mi_velvet_bank_set_offset, (None, 0, 0.0)), (lib.mi_velvet_bank_set_crush, (None, 0, 1)),
                        (lib.mi_velvet_bank_process, (None, None, None, 1, 1, 1, 0, None)), (lib.mi_velvet_bank_reserve, (None, 1)),
                        (lib.mi_velvet_bank_get_state, (None, 0, ctypes.byref(s), None)), (lib.mi_velvet_bank_set_state, (None, 0, ctypes.byref(s), None))):
        assert entry(*args) == ESTATE, entry                                        # no bank
    assert lib.mi_velvet_bank_destroy(None) == 0
    if mi.device_count() <= 0:                                                      # no device: no bank, loudly
        with pytest.raises(mi.MiError) as e:
            mi.VelvetBank(2)
        assert e.value.code == ENODEV


def test_the_golden_inventories_name_the_references_members():
    keys = json.load(open(os.path.join(GOLDEN, "velvet_dump_keys.json")))["Velvet"]
    top = [k[2:] for k in keys["keys"] if k.startswith("0:")]
    assert top == list(gen.MEMBERS)
    assert "1:bCrush" in keys["keys"] and "1:fCrushProb" in keys["keys"] and "1:nState" in keys["keys"] and "1:nBufID" in keys["keys"]
    assert keys["sizeof"] == 176 and keys["offsetof"][:2] == [0, 72]
    names = json.load(open(os.path.join(GOLDEN, "velvet_public_names.json")))["noise/Velvet.h"]
    assert {"init", "set_core_type", "set_velvet_type", "set_velvet_window_width", "set_delta_value", "set_amplitude", "set_offset", "set_crush",
            "set_crush_probability", "process_add", "process_mul", "process_overwrite", "dump"} <= set(names)
