"""The C++ class lsp::dspu::Depopper without a device: tests/cpp/depopper_layout.cpp, a stand-alone program, gives sizeof and offsetof
of the class (those that the reference's driver printed into tests/golden/depopper_dump_keys.json; where the reference tree exists
the same program compiled against the reference's own headers and sources prints the same lines) and what its host side does: a
fresh object, the setters' returns and quirks, init()'s extents, reconfigure() in every mode, dump()."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import depopper_ref as dr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_depopper_vectors as gen  # noqa: E402

f32, u32 = np.float32, np.uint32
PKG = os.path.join(ROOT, "lsp-dsp-units_amd")
REFERENCE = os.path.join(os.path.dirname(ROOT), "reference")
PROGRAM = os.path.join(ROOT, "tests", "cpp", "depopper_layout.cpp")
GOLDEN = os.path.join(ROOT, "tests", "golden")
HEADER = os.path.join(PKG, "include", "lsp-plug.in", "dsp-units", "util", "Depopper.h")


def lines(text):
    return {l.split()[0]: l.split()[1:] for l in text.splitlines() if l.strip()}


def bits(*values):
    return [str(int(np.array(v, f32).view(u32))) for v in values]


@pytest.fixture(scope="module")
def program(mi, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("depopper_layout") / "depopper_layout")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-I" + os.path.join(PKG, "include"), "-I" + os.path.join(ROOT, "include"),
                           PROGRAM, "-o", exe, "-L" + PKG, "-lmi_dspu", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


@pytest.fixture(scope="module")
def behaviour(program):
    return lines(subprocess.check_output([program, "behaviour"]).decode())


@pytest.fixture(scope="module")
def stored():
    return json.load(open(os.path.join(GOLDEN, "depopper_dump_keys.json")))


def test_sizeof_and_offsetof_are_those_the_reference_driver_printed(program, stored):
    got = lines(subprocess.check_output([program]).decode())
    assert [int(v) for v in got["sizeof"]] == stored["sizeof"] == [248, 48]
    assert [int(v) for v in got["offsetof"]] == stored["offsetof"] == [0, 8, 12, 48, 96, 112, 120, 168, 216, 240]


@pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE, "src", "main", "util")), reason="the reference tree is not here")
def test_the_same_program_against_the_references_headers_says_the_same(program, tmp_path):
    exe = gen.compile_driver(REFERENCE, str(tmp_path), PROGRAM, str(tmp_path / "ref_layout"))
    assert subprocess.check_output([exe]) == subprocess.check_output([program])
    assert subprocess.check_output([exe, "behaviour"]) == subprocess.check_output([program, "behaviour"])


def test_fresh_object_and_init(behaviour):
    assert behaviour["fresh"] == ["-1"] + ["0"] * 17 + ["1"]                                # construct(), Depopper.cpp:44-94
    assert behaviour["fresh_in"] == ["0"] + bits(0.0001, 50.0, 0.0) + ["0"] * 6
    assert behaviour["fresh_out"] == ["0"] + bits(0.0001, 0.0, 0.0) + ["0"] * 6
    # 480 -> 512 and 96 -> 128 by DEFAULT_ALIGN 0x40; nLookMin = 640, nLookMax = 640 + max(2048, 0x1000); nRmsMax = 128 + 0x1000
    assert behaviour["init"] == ["1"] and behaviour["same"] == ["1"] and behaviour["buffers"] == ["1", "1"]
    assert behaviour["inited"] == ["48000", "0"] + bits(10.0) + ["640", "4736", "640", "0"] + bits(2.0, 0.0) + ["128", "4224", "128"] + ["0"] * 5 + ["1", "1"]
    assert behaviour["inited2"][:7] == ["44100", "0"] + bits(5.0) + ["320", "4416", "320", "288"]      # the designed values stay until reconfigure()
    assert behaviour["inited2"][9:12] == ["64", "4160", "64"] and behaviour["inited2"][-2:] == ["1", "1"]
    assert behaviour["destroyed"][-2:] == ["0", "1"]


def test_setters_return_the_clamped_old_value_and_store_the_new_one_as_given(behaviour):
    assert behaviour["olds"] == bits(50.0, 0.0, 0.0, 10.0, 0.0001, 0.0, 0.0)
    assert behaviour["kept"] == bits(-3.0, 25.0, -1.0, 2.0) + ["1"]                        # 0, 10 and 0 were "unchanged"; 7 ms is clamped
    assert behaviour["delay"] == bits(0.25) + ["0"] + bits(0.25) + ["1"] + bits(1.0)      # set_fade_out_delay compares with fThresh
    assert behaviour["modes"] == ["0", "2", "0"]


def test_reconfigure_designs_what_the_restatement_designs(behaviour):
    for m in range(5):
        d = dr.Depopper()
        d.init(48000, 10.0, 2.0)
        d.set_fade_in_time(6.25), d.set_fade_out_time(5.0), d.set_fade_in_delay(0.5), d.set_fade_in_threshold(0.1), d.set_rms_length(1.0)
        d.set_fade_out_threshold(0.25), d.set_fade_out_delay(1.0)
        d.set_fade_in_mode(m), d.set_fade_out_mode(m)
        d.reconfigure()
        for key, fade in (("in%d" % m, d.sFadeIn), ("out%d" % m, d.sFadeOut)):
            got = behaviour[key]
            assert got[:4] == [str(m)] + bits(fade.fThresh, fade.fTime, fade.fDelay), key
            assert [int(v) for v in got[4:]] == fade.words(), key
    assert behaviour["designed"][6] == "288" and behaviour["designed"][12:14] == ["48"] + bits(f32(1.0) / f32(48.0)) and behaviour["latency"] == ["240"]


def test_dump_writes_the_references_keys_in_order(behaviour, stored):
    assert behaviour["Depopper"] == stored["Depopper"]
    at = stored["Depopper"].index("0:sFadeOut")
    assert stored["Depopper"][at + 1:at + 8] == ["1:enMode", "1:fThresh", "1:fTime", "1:fDelay", "1:nSamples", "1:nDelay", "1:fPoly"]


def test_the_mirror_declares_the_references_public_names_and_members(stored):
    names = json.load(open(os.path.join(GOLDEN, "depopper_public_names.json")))
    assert set(names) == {"util/Depopper.h"}
    assert gen.public_names(HEADER, "Depopper") == names["util/Depopper.h"] and len(names["util/Depopper.h"]) == 29
    text = re.sub(r"//.*", "", open(HEADER).read())
    fields = [k[2:] for k in stored["Depopper"] if k.startswith("0:")]
    members = text[text.index("size_t          nSampleRate"):]
    assert len(fields) == 23 and all(re.search(r"\b%s;" % n, members) for n in fields)
    assert [members.index(n + ";") for n in fields] == sorted(members.index(n + ";") for n in fields)     # in the reference's order
    for enum in ("DPM_LINEAR", "DPM_CUBIC", "DPM_SINE", "DPM_GAUSSIAN", "DPM_PARABOLIC", "ST_CLOSED", "ST_FADE", "ST_OPENED", "ST_WAIT"):
        assert re.search(r"\b%s\b" % enum, text), enum
    order = [text.index(n) for n in ("DPM_LINEAR", "DPM_CUBIC", "DPM_SINE", "DPM_GAUSSIAN", "DPM_PARABOLIC")]
    assert order == sorted(order)


def test_the_library_exports_the_class(mi):
    out = subprocess.check_output(["nm", "-D", "--defined-only", "-C", mi.LIB_PATH]).decode()
    for sym in ("lsp::dspu::Depopper::Depopper()", "lsp::dspu::Depopper::~Depopper()", "lsp::dspu::Depopper::construct()", "lsp::dspu::Depopper::destroy()",
                "lsp::dspu::Depopper::init(unsigned long, float, float)", "lsp::dspu::Depopper::reconfigure()",
                "lsp::dspu::Depopper::set_fade_in_time(float)", "lsp::dspu::Depopper::set_fade_out_time(float)",
                "lsp::dspu::Depopper::set_fade_in_delay(float)", "lsp::dspu::Depopper::set_fade_out_delay(float)",
                "lsp::dspu::Depopper::set_fade_in_threshold(float)", "lsp::dspu::Depopper::set_fade_out_threshold(float)",
                "lsp::dspu::Depopper::set_rms_length(float)", "lsp::dspu::Depopper::set_fade_in_mode(lsp::dspu::depopper_mode_t)",
                "lsp::dspu::Depopper::set_fade_out_mode(lsp::dspu::depopper_mode_t)",
                "lsp::dspu::Depopper::process(float*, float*, float const*, unsigned long)",
                "lsp::dspu::Depopper::dump(lsp::dspu::IStateDumper*) const", "mi_depopper_bank_create", "mi_depopper_bank_process"):
        assert sym in out, sym
    assert "Depopper::set_release" not in out              # declared by the reference, defined nowhere
