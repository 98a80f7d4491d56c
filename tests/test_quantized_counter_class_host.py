"""The C++ class lsp::dspu::QuantizedCounter without a device: tests/cpp/quantized_counter_layout.cpp, a stand-alone program, gives
sizeof and offsetof of the class (those that the reference's driver printed into tests/golden/quantized_counter_dump_keys.json;
where the reference tree exists the same program compiled against the reference's own headers and sources prints the same lines)
and what its host side does: a fresh object, init(), the setters' limits and their bUpdate rule against the restatement,
update_settings() and clear() on an empty window, dump()'s keys, and the public names."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import quantized_counter_ref as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_quantized_counter_vectors as gen  # noqa: E402

f32, u32 = np.float32, np.uint32
PKG = os.path.join(ROOT, "lsp-dsp-units_amd")
REFERENCE = os.path.join(os.path.dirname(ROOT), "reference")
PROGRAM = os.path.join(ROOT, "tests", "cpp", "quantized_counter_layout.cpp")
GOLDEN = os.path.join(ROOT, "tests", "golden")
HEADER = os.path.join(PKG, "include", "lsp-plug.in", "dsp-units", "stat", "QuantizedCounter.h")


def lines(text):
    return {l.split()[0]: l.split()[1:] for l in text.splitlines() if l.strip()}


def compile_program(exe):
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-I" + os.path.join(PKG, "include"), "-I" + os.path.join(ROOT, "include"),
                           PROGRAM, "-o", exe, "-L" + PKG, "-lmi_dspu", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


@pytest.fixture(scope="module")
def program(mi, tmp_path_factory):
    return compile_program(str(tmp_path_factory.mktemp("quantized_counter_layout") / "quantized_counter_layout"))


@pytest.fixture(scope="module")
def behaviour(program):
    return lines(subprocess.check_output([program, "behaviour"]).decode())


@pytest.fixture(scope="module")
def stored():
    return json.load(open(os.path.join(GOLDEN, "quantized_counter_dump_keys.json")))


def test_sizeof_and_offsetof_are_those_the_reference_driver_printed(program, stored):
    got = lines(subprocess.check_output([program]).decode())
    assert [int(v) for v in got["sizeof"]] == stored["sizeof"] == [72]
    assert [int(v) for v in got["offsetof"]] == stored["offsetof"] == [0, 4, 8, 12, 16, 20, 24, 28, 32, 36, 40, 48, 56, 64]


@pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE, "src", "main", "stat")), reason="the reference tree is not here")
def test_the_same_program_against_the_references_headers_says_the_same(program, tmp_path):
    exe = gen.compile_driver(REFERENCE, str(tmp_path), PROGRAM, str(tmp_path / "ref_layout"))
    assert subprocess.check_output([exe]) == subprocess.check_output([program])
    assert subprocess.check_output([exe, "behaviour"]) == subprocess.check_output([program, "behaviour"])


def line_of(q):
    """What the program's line() prints for the restatement's object."""
    w = q.settings_words()[-8:]
    return [str(v) for v in (q.period, q.levels, q.head, q.capacity, q.count, q.max_period, q.max_levels, w[4], w[5], w[6], int(q.update),
                             q.period, q.max_period, q.levels, q.count, int(q.update))]


def test_the_host_side_is_the_restatement(behaviour):
    # construct(), :42-62: everything 0, bUpdate set
    assert behaviour["fresh"] == ["0"] * 10 + ["1", "0", "0", "0", "0", "1"]
    assert behaviour["init"] == ["0", "1", "1"]                             # STATUS_OK; a 64-byte aligned ring with the counters behind it
    q = Q.QuantizedCounter(40, 16)
    assert q.capacity == 1072
    assert behaviour["inited"] == line_of(q)
    q.set_period(1000), q.set_levels(100)
    assert behaviour["limited_high"] == line_of(q) and q.period == 40 and q.levels == 16
    q.set_period(0), q.set_levels(0)
    assert behaviour["limited_low"] == line_of(q) and q.period == 1 and q.levels == 1
    q.update_settings()
    assert behaviour["updated"] == line_of(q) and np.isinf(q.rstep) and not q.update
    assert behaviour["counters"] == ["0"] * 4
    q.set_levels(1), q.set_min_value(0.0), q.set_max_value(0.0), q.set_value_range(0.0, 0.0), q.set_range(0.0, 0.0, 1)
    assert behaviour["unchanged"] == line_of(q) and not q.update            # unchanged values: no bUpdate
    q.set_range(-1.0, 1.0, 8)
    assert behaviour["set_range"] == line_of(q) and q.update
    q.update_settings()
    assert behaviour["updated_range"] == line_of(q) and q.rstep == f32(4.0)
    q.set_min_value(-2.0)
    assert behaviour["set_min"] == line_of(q) and q.update and q.rstep == f32(4.0)     # fRStep is that of the last update
    q.update_settings(), q.set_max_value(2.0)
    assert behaviour["set_max"] == line_of(q) and q.update
    q.update_settings(), q.set_value_range(-2.0, 2.0)
    assert behaviour["same_value_range"] == line_of(q) and not q.update
    q.set_value_range(1.0, -1.0), q.update_settings()
    assert behaviour["reversed"] == line_of(q) and q.rstep == f32(-4.0)
    q.set_period(7), q.clear()
    assert behaviour["cleared"] == line_of(q)
    assert behaviour["destroyed"] == ["1"]


def test_dump_writes_the_references_keys_in_the_references_order(behaviour, stored):
    assert behaviour["dump"] == stored["dump"]
    assert stored["dump"][0] == "0:nPeriod" and stored["dump"][-1] == "0:pData" and len(stored["dump"]) == 14


def test_public_names_are_the_references():
    stored = json.load(open(os.path.join(GOLDEN, "quantized_counter_public_names.json")))
    assert gen.public_names(HEADER, "QuantizedCounter") == stored["stat/QuantizedCounter.h"]
    assert "needs_update" in stored["stat/QuantizedCounter.h"] and len(stored["stat/QuantizedCounter.h"]) >= 22
