"""The C++ class lsp::dspu::ADSREnvelope without a device: tests/cpp/adsr_layout.cpp, a stand-alone program, gives sizeof and
offsetof of the class (those that the reference's driver printed into tests/golden/adsr_dump_keys.json; where the reference tree
exists the same program compiled against the reference's own headers and sources prints the same lines, EXP samples by the
neighbour rule) and what its host side does: a fresh object, the setters' flags, update_settings(), the generator that every
function gets, the scalar process(float) against the restatement bit for bit, dump()'s keys, and the public names."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import adsr_ref as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_adsr_vectors as gen  # noqa: E402
from make_bypass_crossfade_vectors import public_names  # noqa: E402

f32, u32 = np.float32, np.uint32
PKG = os.path.join(ROOT, "lsp-dsp-units_amd")
REFERENCE = os.path.join(os.path.dirname(ROOT), "reference")
PROGRAM = os.path.join(ROOT, "tests", "cpp", "adsr_layout.cpp")
GOLDEN = os.path.join(ROOT, "tests", "golden")
HEADER = os.path.join(PKG, "include", "lsp-plug.in", "dsp-units", "util", "ADSREnvelope.h")
USED = (3, 5, 5, 5, 6, 6)
GENERATOR = (0, 1, 1, 3, 4, 5)                              # LINE2 takes the line generator


def lines(text):
    return {l.split()[0]: l.split()[1:] for l in text.splitlines() if l.strip()}


def bits(*values):
    return [str(int(np.array(v, f32).view(u32))) for v in values]


@pytest.fixture(scope="module")
def program(mi, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("adsr_layout") / "adsr_layout")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-I" + os.path.join(PKG, "include"), "-I" + os.path.join(ROOT, "include"),
                           PROGRAM, "-o", exe, "-L" + PKG, "-lmi_dspu", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


@pytest.fixture(scope="module")
def behaviour(program):
    return lines(subprocess.check_output([program, "behaviour"]).decode())


@pytest.fixture(scope="module")
def stored():
    return json.load(open(os.path.join(GOLDEN, "adsr_dump_keys.json")))


def test_sizeof_and_offsetof_are_those_the_reference_driver_printed(program, stored):
    got = lines(subprocess.check_output([program]).decode())
    assert [int(v) for v in got["sizeof"]] == stored["sizeof"] == [208, 48, 24]
    assert [int(v) for v in got["offsetof"]] == stored["offsetof"] == [0, 192, 196, 200, 204, 4, 8, 16, 24]


@pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE, "src", "main", "util")), reason="the reference tree is not here")
def test_the_same_program_against_the_references_headers_says_the_same(program, tmp_path):
    exe = gen.compile_driver(REFERENCE, str(tmp_path), PROGRAM, str(tmp_path / "ref_layout"))
    assert subprocess.check_output([exe]) == subprocess.check_output([program])
    ref, mine = lines(subprocess.check_output([exe, "behaviour"]).decode()), lines(subprocess.check_output([program, "behaviour"]).decode())
    assert ref.keys() == mine.keys()
    for key in ref:
        if key == "fresh":                                  # the reference's constructor leaves most of the union unset
            continue
        if key == "process5":                               # EXP: the C library's expf against the float64 exp rounded once
            a, b = np.array(ref[key], np.int64), np.array(mine[key], np.int64)
            assert np.all(np.abs(a - b) <= 4) and np.mean(a != b) <= 0.05, key
        else:
            assert ref[key] == mine[key], key


def test_fresh_object_and_the_setters_flags(behaviour):
    curve = bits(0.0, 0.5) + ["0", "0"]                         # construct(), :40-58
    assert behaviour["fresh"] == curve * 4 + bits(0.0, 0.0, 0.0) + [str(A.RECONFIGURE)]
    assert behaviour["fresh_getters"] == bits(0.0, 0.0, 0.0, 0.5, 0.0) + ["0"] + bits(0.0, 0.0)
    # update_settings() clears F_RECONFIGURE; the same values again ask for nothing; a clamped value, a new value and a flag do
    assert behaviour["flags"] == ["0", "0", "4", "0", "6", "2", "6"] + bits(1.0)
    assert behaviour["pushed"] == bits(0.5, 0.5, 0.5, 0.7, 0.7)


@pytest.mark.parametrize("fn", range(6))
def test_update_settings_and_scalar_process_are_the_restatement(behaviour, fn):
    e = A.design(gen.op_rows(gen.base(fn, 0.25))).update_settings()
    want = []
    for p in range(4):
        want += bits(e.time[p], e.curve[p]) + [str(fn), str(GENERATOR[fn])] + [str(int(v)) for v in e.params[p][:USED[fn]].view(u32)]
    want += bits(e.hold_time, e.break_level, e.sustain_level) + [str(A.USE_HOLD | A.USE_BREAK)]
    assert behaviour["designed%d" % fn] == want
    t = (np.arange(-2, 67).astype(f32) / f32(64)).astype(f32)
    out = e.run(A.PROCESS, src=t)[0]
    assert behaviour["process%d" % fn] == [str(int(v)) for v in out.view(u32)]
    assert np.count_nonzero(out) >= 60 and out[0] == 0 and out[2] == 0 and out[-1] == 0


def test_dump_writes_the_references_keys_in_the_references_order(behaviour, stored):
    for fn, name in enumerate(gen.FN_NAMES):
        assert behaviour["dump%d" % fn] == stored[name], name
        assert stored[name][0] == "0:vCurve" and stored[name][-1].endswith(":nFlags")


def test_interpolation_entries(behaviour):
    assert behaviour["cubic"] == [str(int(v)) for v in A.hermite_cubic(0.0, 1.0, -2.5, 0.2, 0.5, -1.0).view(u32)]
    assert behaviour["quadro"] == [str(int(v)) for v in A.hermite_quadro(0.0, 1.0, 0.0, 0.2, 0.5, 0.0, 0.1, 0.8).view(u32)]


def test_public_names_are_the_references():
    stored = json.load(open(os.path.join(GOLDEN, "adsr_public_names.json")))
    assert public_names(HEADER, "ADSREnvelope") == stored["util/ADSREnvelope.h"]
    assert "set_relese_time" in stored["util/ADSREnvelope.h"] and len(stored["util/ADSREnvelope.h"]) >= 45
