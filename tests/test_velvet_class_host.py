"""The C++ class lsp::dspu::Velvet without a device: tests/cpp/velvet_layout.cpp, a stand-alone program, gives sizeof and offsetof of
the class (those that the reference's driver printed into tests/golden/velvet_dump_keys.json, and where the reference tree exists
the same program compiled against the reference's own headers says the same) and what its host side does: a fresh object, the
setters' clamps, init() and dump().  Public names and dump keys are held to the recorded inventories."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import noise_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_velvet_vectors as gen  # noqa: E402

f32, u32 = np.float32, np.uint32
PKG = os.path.join(ROOT, "lsp-dsp-units_amd")
REFERENCE = os.path.join(os.path.dirname(ROOT), "reference")
PROGRAM = os.path.join(ROOT, "tests", "cpp", "velvet_layout.cpp")
GOLDEN = os.path.join(ROOT, "tests", "golden")
HEADER = os.path.join(PKG, "include", "lsp-plug.in", "dsp-units", "noise", "Velvet.h")


def lines(text):
    return {l.split()[0]: l.split()[1:] for l in text.splitlines() if l.strip()}


def bits(*values):
    return [str(int(np.array(v, f32).view(u32))) for v in values]


@pytest.fixture(scope="module")
def program(mi, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("velvet_layout") / "velvet_layout")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-I" + os.path.join(PKG, "include"), "-I" + os.path.join(ROOT, "include"),
                           PROGRAM, "-o", exe, "-L" + PKG, "-lmi_dspu", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


@pytest.fixture(scope="module")
def behaviour(program):
    return lines(subprocess.check_output([program, "behaviour"]).decode())


@pytest.fixture(scope="module")
def stored():
    return json.load(open(os.path.join(GOLDEN, "velvet_dump_keys.json")))["Velvet"]


def test_sizeof_and_offsetof_are_those_the_reference_driver_printed(program, stored):
    got = lines(subprocess.check_output([program]).decode())
    assert [int(v) for v in got["sizeof"]] == [stored["sizeof"]] == [176]
    assert [int(v) for v in got["offsetof"]] == stored["offsetof"] == [0, 72, 144, 148, 152, 160, 164, 168, 172, 8, 0, 4]


@pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE, "src", "main", "noise")), reason="the reference tree is not here")
def test_the_same_program_against_the_references_headers_says_the_same(program, tmp_path):
    exe = gen.compile_driver(REFERENCE, str(tmp_path), PROGRAM, str(tmp_path / "ref_layout"))
    assert subprocess.check_output([exe]) == subprocess.check_output([program])
    assert subprocess.check_output([exe, "behaviour"]) == subprocess.check_output([program, "behaviour"])


def test_fresh_object_and_setter_clamps(behaviour):
    assert behaviour["fresh"] == ["0", "0", "0"] + bits(0.5, 10.0, 0.5, 1.0, 0.0)                   # construct(), Velvet.cpp:48-63
    assert behaviour["freshstate"] == ["1", "64", "0", "1"]
    assert behaviour["clamped"] == ["1", "2", "1"] + bits(1.0, 2.0, 0.0, -2.0, -0.0)
    assert behaviour["clamped2"] == ["1", "2", "1"] + bits(0.0, 10.7, 1.0, -2.0, -0.0)
    assert behaviour["kept"] == ["1", "2", "1"] + bits(0.25, 2.0, 0.75, -2.0, -0.0)


def test_init_gives_the_randomizers_words_and_tells_the_mls(behaviour):
    want = [w for g in R.seed_words(0x12345678) for w in g] + [0]
    assert [int(v) for v in behaviour["init"]] == want
    assert behaviour["mls"] == ["23", str(0x55), "1"] + bits(1.0, 0.0)                              # told, not yet updated
    assert behaviour["same"] == ["0"] and behaviour["other"] == ["1", "24"]


def test_dump_writes_the_references_keys_in_order(behaviour, stored):
    assert behaviour["Velvet"] == stored["keys"]
    nested = stored["keys"][stored["keys"].index("0:sCrushParams") + 1:][:2]
    assert nested == ["1:bCrush", "1:fCrushProb"]


def test_the_mirror_declares_the_references_public_names_and_members(stored):
    names = json.load(open(os.path.join(GOLDEN, "velvet_public_names.json")))
    assert set(names) == {"noise/Velvet.h"}
    assert gen.public_names(HEADER, "Velvet") == names["noise/Velvet.h"]
    text = re.sub(r"//.*", "", open(HEADER).read())
    for deleted in ("Velvet(const Velvet &) = delete", "Velvet(Velvet &&) = delete"):
        assert deleted in text, deleted
    fields = [k[2:] for k in stored["keys"] if k.startswith("0:")]
    members = text[text.index("private:"):]
    assert fields == list(gen.MEMBERS) and all(re.search(r"\b%s;" % n, members) for n in fields)
    assert [members.index(n + ";") for n in fields] == sorted(members.index(n + ";") for n in fields)     # in the reference's order
    for enum in ("VN_CORE_MLS", "VN_CORE_LCG", "VN_VELVET_OVN", "VN_VELVET_OVNA", "VN_VELVET_ARN", "VN_VELVET_TRN"):
        assert re.search(r"\b%s\b" % enum, text), enum


def test_the_library_exports_the_class(mi):
    out = subprocess.check_output(["nm", "-D", "--defined-only", "-C", mi.LIB_PATH]).decode()
    for sym in ("lsp::dspu::Velvet::Velvet()", "lsp::dspu::Velvet::init(unsigned int, unsigned char, unsigned long)", "lsp::dspu::Velvet::init()",
                "lsp::dspu::Velvet::set_core_type(lsp::dspu::vn_core_t)", "lsp::dspu::Velvet::set_velvet_type(lsp::dspu::vn_velvet_type_t)",
                "lsp::dspu::Velvet::set_velvet_window_width(float)", "lsp::dspu::Velvet::set_delta_value(float)", "lsp::dspu::Velvet::set_crush(bool)",
                "lsp::dspu::Velvet::set_crush_probability(float)", "lsp::dspu::Velvet::process_add(float*, float const*, unsigned long)",
                "lsp::dspu::Velvet::process_mul(float*, float const*, unsigned long)", "lsp::dspu::Velvet::process_overwrite(float*, unsigned long)",
                "lsp::dspu::Velvet::dump(lsp::dspu::IStateDumper*) const", "mi_velvet_bank_create", "mi_velvet_bank_process"):
        assert sym in out, sym
