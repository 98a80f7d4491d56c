"""LCG and MLS without a device: the numpy restatement against the reference's recorded outputs and state words (bit for bit;
samples that expf, logf or cosf made by the interval rule), the MLS closed form over GF(2) against the serial register for every
register width, the C-ABI's word arithmetic (init(seed), the MLS masks, the tables of the closed form) against the restatement, and
the refusals that need no device."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

import noise_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_noise_vectors as gen  # noqa: E402

f32, u32, u64 = np.float32, np.uint32, np.uint64
REFERENCE = os.path.join(os.path.dirname(ROOT), "reference")
EINVAL, ENODEV = -1, -3
TILE, POWERS = 1024, 27


@pytest.fixture(scope="module")
def recorded():
    return gen.load()


@pytest.fixture(scope="module")
def restated(recorded):
    """Every recorded case through the restatement with S* and, where a transcendental made samples, with its neighbours: once."""
    out = []
    for c in recorded:
        star, trans, unit = R.run_case(c)
        out.append((star, trans, unit, R.neighbours(c, trans)))
    return out


def test_restatement_equals_the_references_recorded_outputs(recorded, restated):
    assert sum(c["kind"] == R.KIND_LCG for c in recorded) >= 36 and sum(c["kind"] == R.KIND_MLS for c in recorded) >= 40
    for c, (star, trans, unit, others) in zip(recorded, restated):
        bad = R.agree(c["out"], star, star, others, trans)
        assert bad.size == 0, (c["name"], bad[:5], c["out"][bad[:5]], star[bad[:5]])
        w = unit.words()
        assert np.array_equal(w, c["words"][:w.size]) and not c["words"][w.size:].any(), (c["name"], w, c["words"])
        if c["kind"] == R.KIND_MLS:
            assert not trans.any(), c["name"]


def test_recorded_transcendental_samples_obey_the_interval_rule(recorded, restated):
    """The reference's C library against S*: inside the interval everywhere.  How many samples differ from S* is printed, not
    asserted: a C library may match S* on every recorded sample."""
    seen = differ = 0
    for c, (star, trans, _, others) in zip(recorded, restated):
        if not trans.any():
            continue
        assert len(others) in (2, 8, 10), c["name"]
        assert R.inside(c["out"], star, others)[trans].all(), c["name"]
        seen += int(trans.sum())
        differ += int(np.count_nonzero(~R.same(c["out"], star) & trans))
    print("recorded samples that expf, logf or cosf made: %d; they differ from S* in %d" % (seen, differ))
    assert seen > 15000 and differ < seen // 10


@pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE, "src", "main", "noise")), reason="the reference tree is not here")
def test_the_generator_still_makes_the_recorded_cases(recorded):
    cs, src, got, keys, names = gen.run_reference(REFERENCE)
    assert [c["name"] for c in cs] == [c["name"] for c in recorded]
    for m, g, c in zip(cs, got, recorded):
        assert np.array_equal(m["ops"], c["ops"]) and np.array_equal(R.bits(src), R.bits(c["src"])) and m["kind"] == c["kind"], m["name"]
        assert R.same(g["out"], c["out"]).all() and np.array_equal(g["words"], c["words"]), m["name"]
    gen.check_branches(cs, src, got)
    golden = os.path.join(ROOT, "tests", "golden")
    stored = json.load(open(os.path.join(golden, "noise_dump_keys.json")))
    for k, cls in enumerate(("Randomizer", "LCG", "MLS")):                      # dump keys in order, object sizes
        assert stored[cls]["keys"] == keys[cls] and str(stored[cls]["sizeof"]) == keys["sizeof"][k], cls
    assert json.load(open(os.path.join(golden, "noise_public_names.json"))) == names


def test_the_committed_operation_lists_are_the_generators(recorded):
    made, src = gen.cases(), gen.source_row()
    assert [m["name"] for m in made] == [c["name"] for c in recorded]
    for m, c in zip(made, recorded):
        assert np.array_equal(m["ops"], c["ops"]) and np.array_equal(R.bits(src), R.bits(c["src"])), m["name"]


def test_recorded_cases_cover_what_the_issue_lists(recorded):
    dists, seeds, calls, whats, widths, amps = set(), set(), set(), set(), set(), set()
    for c in recorded:
        for op in c["ops"]:
            what = int(op[0])
            if what in R.PROCESS_OPS:
                calls.add(int(op[1]))
                whats.add((c["kind"], what))
            elif what == R.SET_DISTRIBUTION: dists.add(int(op[1]))
            elif what == R.INIT: seeds.add(int(op[1]))
            elif what == R.SET_N_BITS: widths.add(int(op[1]))
            elif what == R.SET_AMPLITUDE: amps.add((c["kind"], float(op[1])))
    assert dists == {0, 1, 2, 3} and {0, 1, 0x12345678, 0xFFFFFFFF} <= seeds
    assert {1, 3, 7, 255, 257, 1023} <= calls
    assert whats == {(k, w) for k in (R.KIND_LCG, R.KIND_MLS) for w in R.PROCESS_OPS}
    assert {0, 1, 2, 3, 8, 23, 32, 33, 63, 64, 200} <= widths
    lcg = {a for k, a in amps if k == R.KIND_LCG}
    assert 0.0 in lcg and np.inf in lcg and any(a < 0 for a in lcg) and any(0 < a < 1.2e-38 for a in lcg)
    assert {0.0, np.inf} <= {a for k, a in amps if k == R.KIND_MLS}


# ---- the MLS closed form ------------------------------------------------------------------------------------------------------
def serial_states(n_bits, s0, n):
    """states[i]: the register i samples on; bits[i]: sample i."""
    m = R.MLS()
    m.set_n_bits(n_bits)
    m.set_state(s0)
    m.update_settings()
    states, bits = [m.state], []
    for _ in range(n):
        bits.append(m.progress())
        states.append(m.state)
    return states, bits


def np_parity(v):
    v = np.asarray(v, u64).copy()
    for s in (32, 16, 8, 4, 2, 1):
        v ^= v >> u64(s)
    return (v & u64(1)).astype(np.uint8)


def np_matvec(A, v):
    return int(np.sum(np_parity(A & u64(v)).astype(u64) << np.arange(64, dtype=u64)))


SEED = 0xDEADBEEFCAFEF00D


@pytest.mark.parametrize("n_bits", range(1, 65))
def test_the_closed_form_of_the_restatement_is_the_serial_register(n_bits):
    states, bits = serial_states(n_bits, SEED, 160)
    rows = R.rows(n_bits, 160)
    assert [R.parity(r & states[0]) for r in rows] == bits
    assert R.TAPS[n_bits - 1] & ~((1 << n_bits) - 1) == 0 and R.TAPS[n_bits - 1] & 1       # the taps lie inside the register; M is invertible
    pw = R.powers(n_bits, 8)
    for p in range(8):
        assert R.matvec(pw[p], states[0]) == states[1 << p], p
    for n in (0, 1, 63, 64, 65, 127, 160):
        assert R.advance(pw, states[0], n) == states[n], n


@pytest.fixture(scope="module")
def tables(mi):
    out = {}
    for n_bits in range(1, 65):
        rows, powers = np.zeros(TILE, u64), np.zeros((POWERS, 64), u64)
        mi.check(mi.lib.mi_mls_tables(n_bits, rows.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), powers.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))))
        out[n_bits] = (rows, powers)
    return out


def abi_advance(mi, n_bits, state, count):
    v = ctypes.c_uint64()
    mi.check(mi.lib.mi_mls_advance(n_bits, state, count, ctypes.byref(v)))
    return v.value


@pytest.mark.parametrize("n_bits", range(1, 65))
def test_the_librarys_tables_are_the_serial_register(mi, tables, n_bits):
    """rows over one whole tile, the powers M^(2^p) up to the tile against the register itself, the higher ones by squaring, and
    M^count for counts around the tile and beyond the table."""
    rows, powers = tables[n_bits]
    states, bits = serial_states(n_bits, SEED, TILE + 70)
    assert np.array_equal(np_parity(rows & u64(states[0])), np.array(bits[:TILE], np.uint8))
    for p in range(11):
        assert np_matvec(powers[p], states[0]) == states[1 << p], p
    rng = np.random.default_rng(n_bits)
    for p in range(10, POWERS - 1):
        v = int(rng.integers(0, 1 << 63)) * 2 + 1
        assert np_matvec(powers[p + 1], v) == np_matvec(powers[p], np_matvec(powers[p], v)), p
    for n in (0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1, TILE + 70):
        assert abi_advance(mi, n_bits, states[0], n) == states[n], n
    a, b = (1 << 27) - 5, (1 << 33) + 12345                                    # M^(a + b) = M^b M^a, beyond the 27 powers too
    assert abi_advance(mi, n_bits, states[0], a + b) == abi_advance(mi, n_bits, abi_advance(mi, n_bits, states[0], a), b)
    if n_bits <= 20:                                                            # a whole period is the identity
        assert abi_advance(mi, n_bits, states[0], (1 << n_bits) - 1) == states[0]
        assert n_bits == 1 or all(abi_advance(mi, n_bits, states[0], k) != states[0] for k in (1, (1 << n_bits) - 2))


def test_the_restatements_tables_are_the_librarys(tables):
    for n_bits in (1, 2, 3, 8, 23, 33, 64):
        rows, powers = tables[n_bits]
        assert [int(r) for r in rows[:200]] == R.rows(n_bits, 200)
        assert [[int(w) for w in P] for P in powers[:12]] == R.powers(n_bits, 12)


# ---- the C-ABI's word arithmetic --------------------------------------------------------------------------------------------
def test_abi_init_words_are_the_restatements(mi):
    capi = sys.modules[mi.__name__ + ".capi"]
    for seed in (0, 1, 0x12345678, 0xFFFFFFFF, 0x80000000, 0xABCDEF01, 0x00F0F00F, 77):
        s = capi.LcgState()
        mi.check(mi.lib.mi_lcg_seed_words(seed, ctypes.byref(s)))
        want = R.seed_words(seed)
        assert [tuple(f[k] for f in (s.last, s.mul1, s.mul2, s.add)) for k in range(4)] == want and s.buf_id == 0, hex(seed)
    unit = R.LCG()
    unit.init(1)
    assert (unit.mul1[0], unit.mul2[0], unit.add[0]) == (R.MUL1[0], R.MUL2[0], R.ADDERS[1])    # the generator the edge draws were searched for
    assert ctypes.sizeof(capi.LcgState) == 68 and ctypes.sizeof(capi.MlsSettings) == 72


def test_abi_mls_settings_are_the_restatements(mi):
    capi = sys.modules[mi.__name__ + ".capi"]
    s = capi.MlsSettings()
    mi.check(mi.lib.mi_mls_settings_init(ctypes.byref(s)))
    fresh = R.MLS()
    assert (s.n_bits, s.output_mask, s.state, s.amplitude, s.offset, s.sync) == (64, 1, 0, 1.0, 0.0, 1)
    assert (fresh.n_bits, fresh.output_mask, fresh.state, bool(fresh.sync)) == (64, 1, 0, True)
    for n_bits in list(range(0, 70)) + [200, (1 << 64) - 1]:
        for state in (0, 1, SEED, R.M64, 1 << 63, 1 << max(min(n_bits, 63), 0)):
            s = capi.MlsSettings()
            mi.lib.mi_mls_settings_init(ctypes.byref(s))
            s.n_bits, s.state = n_bits, state
            mi.check(mi.lib.mi_mls_settings_update(ctypes.byref(s)))
            m = R.MLS()
            m.n_bits, m.state, m.sync = n_bits, state, True
            m.update_settings()
            got = [s.n_bits, s.feedback_bit, s.feedback_mask, s.active_mask, s.taps_mask, s.output_mask, s.state, s.sync]
            assert got == [int(w) for w in m.words()[:8]], (n_bits, hex(state))
            before = bytes(s)
            mi.check(mi.lib.mi_mls_settings_update(ctypes.byref(s)))            # nothing pending: nothing happens
            assert bytes(s) == before


def test_refusals_that_need_no_device(mi):
    capi = sys.modules[mi.__name__ + ".capi"]
    assert mi.lib.mi_lcg_seed_words(1, None) == EINVAL
    assert mi.lib.mi_mls_settings_init(None) == EINVAL and mi.lib.mi_mls_settings_update(None) == EINVAL
    v = ctypes.c_uint64()
    for bad in (0, 65, 200):
        assert mi.lib.mi_mls_tables(bad, None, None) == EINVAL
        assert mi.lib.mi_mls_advance(bad, 1, 1, ctypes.byref(v)) == EINVAL
    assert mi.lib.mi_mls_advance(8, 1, 1, None) == EINVAL
    assert mi.lib.mi_mls_tables(8, None, None) == 0
    h = ctypes.c_void_p(1)
    for create in (mi.lib.mi_lcg_bank_create, mi.lib.mi_mls_bank_create):
        assert create(None, 1) == EINVAL
        assert create(ctypes.byref(h), 0) == EINVAL and not h.value
    assert mi.lib.mi_mls_bank_create(ctypes.byref(h), 65536) == EINVAL              # a channel is a row of the grid
    s = capi.LcgState()
    for entry, args in ((mi.lib.mi_lcg_bank_init, (None, 0, 1)), (mi.lib.mi_lcg_bank_process, (None, None, None, 1, 1, 1, 0, None)),
                        (mi.lib.mi_lcg_bank_get_state, (None, 0, ctypes.byref(s), None)), (mi.lib.mi_mls_bank_set_n_bits, (None, 0, 8)),
                        (mi.lib.mi_mls_bank_process, (None, None, None, 1, 1, 1, 0, None)), (mi.lib.mi_mls_bank_update_settings, (None, None)),
                        (mi.lib.mi_mls_bank_reserve, (None, 1))):
        assert entry(*args) == -5, entry                                            # MI_ESTATE: no bank
    assert mi.lib.mi_lcg_bank_destroy(None) == 0 and mi.lib.mi_mls_bank_destroy(None) == 0
    if mi.device_count() <= 0:                                                      # no device: no bank, loudly
        for cls in (mi.LCGBank, mi.MLSBank):
            with pytest.raises(mi.MiError) as e:
                cls(2)
            assert e.value.code == ENODEV


def test_the_golden_inventories_name_the_references_members():
    golden = os.path.join(ROOT, "tests", "golden")
    keys = json.load(open(os.path.join(golden, "noise_dump_keys.json")))
    assert [k for k in keys["MLS"]["keys"]] == ["0:" + n for n in ("vTapsMaskTable", "nMaxBits", "nBits", "nFeedbackBit", "nFeedbackMask", "nActiveMask",
                                                                    "nTapsMask", "nOutputMask", "nState", "fAmplitude", "fOffset", "bSync")]
    assert keys["LCG"]["keys"][0] == "0:sRand" and keys["LCG"]["keys"][-3:] == ["0:enDistribution", "0:fAmplitude", "0:fOffset"]
    assert keys["Randomizer"]["keys"][0] == "0:vRandom" and keys["Randomizer"]["keys"][-1] == "0:nBufID" and len(keys["Randomizer"]["keys"]) == 18
    names = json.load(open(os.path.join(golden, "noise_public_names.json")))
    assert {"init", "random", "dump"} <= set(names["util/Randomizer.h"])
    assert {"init", "set_distribution", "set_amplitude", "set_offset", "process_single", "process_add", "process_mul", "process_overwrite",
            "dump"} <= set(names["noise/LCG.h"])
    assert {"maximum_number_of_bits", "needs_update", "set_n_bits", "set_state", "set_amplitude", "set_offset", "get_period", "process_single",
            "process_add", "process_mul", "process_overwrite", "dump"} <= set(names["noise/MLS.h"])
