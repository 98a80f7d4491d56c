"""The C++ classes lsp::dspu::SpectralTilt and lsp::dspu::NoiseGenerator without a device: tests/cpp/noise_generator_layout.cpp, a
stand-alone program, gives sizeof and offsetof of both classes (those that the same program printed against the reference's headers
into tests/golden/noise_generator_dump_keys.json; where the reference tree exists it is compiled against it again and says the same)
and what their host side does: fresh objects, which setter raises which UPD_* bit, the range quirk, dump().  Public names and dump keys
are held to the recorded inventories, and the library exports the reference's out-of-line signatures."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_noise_generator_vectors as gen  # noqa: E402

f32, u32 = np.float32, np.uint32
PKG = os.path.join(ROOT, "lsp-dsp-units_amd")
REFERENCE = os.path.join(os.path.dirname(ROOT), "reference")
GOLDEN = os.path.join(ROOT, "tests", "golden")
INCLUDE = os.path.join(PKG, "include", "lsp-plug.in", "dsp-units")


def bits(*values):
    return [str(int(np.array(v, f32).view(u32))) for v in values]


@pytest.fixture(scope="module")
def program(mi, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("noise_generator_layout") / "layout")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-I" + os.path.join(PKG, "include"), "-I" + os.path.join(ROOT, "include"),
                           gen.LAYOUT, "-o", exe, "-L" + PKG, "-lmi_dspu", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


@pytest.fixture(scope="module")
def printed(program):
    return gen.layout_lines(program)


@pytest.fixture(scope="module")
def stored():
    return json.load(open(os.path.join(GOLDEN, "noise_generator_dump_keys.json")))


def test_sizeof_and_offsetof_are_those_of_the_references_classes(printed, stored):
    assert [int(v) for v in printed["sizeof"]] == stored["sizeof"]
    assert [int(v) for v in printed["offsetof_tilt"]] == stored["SpectralTilt"]["offsetof"] == [0, 8, 12, 16, 20, 24, 28, 32, 40, 41, 48]
    assert [int(v) for v in printed["offsetof_generator"]] == stored["NoiseGenerator"]["offsetof"]
    assert [int(v) for v in printed["offsetof_params"]] == stored["NoiseGenerator"]["offsetof_params"]
    assert stored["NoiseGenerator"]["offsetof"][:4] == [0, 72, 160, 336]       # MLS, LCG, Velvet and SpectralTilt by value


@pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE, "src", "main", "noise")), reason="the reference tree is not here")
def test_the_same_program_against_the_references_headers_says_the_same(program, tmp_path):
    exe = gen.compile_driver(REFERENCE, str(tmp_path), gen.LAYOUT, str(tmp_path / "ref_layout"))
    assert subprocess.check_output([exe]) == subprocess.check_output([program])
    assert subprocess.check_output([exe, "behaviour"]) == subprocess.check_output([program, "behaviour"])


def test_fresh_objects_setters_and_the_bits_they_raise(printed):
    none = str(2 ** 64 - 1)
    assert printed["tilt_fresh"] == ["1", "0", "5"] + bits(0.5, 0.5, 0.1, 20000.0) + [none, "0", "1"]           # construct(), SpectralTilt.cpp:52-71
    assert printed["tilt_same"][-1] == "0" and printed["tilt_norm"][-1] == "1"
    assert printed["tilt_range"][5:7] == bits(18000.0, 20.0) and printed["tilt_range"][-1] == "1"               # swapped the wrong way round
    assert printed["tilt_range_again"][5:7] == bits(18000.0, 20.0) and printed["tilt_range_again"][-1] == "0"
    assert printed["tilt_set"][:4] == ["7", "1", "5"] + bits(-3.0) and printed["tilt_set"][7] == "48000"        # order 7 until update_settings()
    fresh = ["0", "0", "0", "0", "0", "0", "0", "1", "0"] + bits(0.1, 0.5) + ["0"] + bits(0.5) + ["0", "50"] + bits(0.0) + ["0", "0", "1"] + bits(1.0, 0.0)
    assert printed["generator_fresh"] == fresh + ["31"]                                                         # construct(), Generator.cpp:44-78: UPD_ALL
    assert printed["generator_same"] == fresh[:18] + ["2"] + fresh[19:] + ["0"]                                 # nothing raised; the generator is set
    # sample rate: colour and velvet; the MLS, LCG, velvet and colour setters their own bit; amplitude UPD_OTHER; an offset of -0.0f
    # compares equal to the 0.0f it has; set_generator nothing
    assert printed["raised"] == ["12", "1", "1", "2", "4", "4", "4", "4", "4", "8", "8", "8", "16", "0", "0"]
    assert printed["generator_set"][:4] == ["9", "5", "0", "3"] and printed["generator_set"][-1] == "0"


def test_dump_writes_the_references_keys_in_order(printed, stored):
    assert printed["SpectralTilt"] == stored["SpectralTilt"]["keys"]
    assert printed["NoiseGenerator"] == stored["NoiseGenerator"]["keys"]
    top = [k[2:] for k in stored["NoiseGenerator"]["keys"] if k.startswith("0:")]
    assert top == ["nSampleRate", "sMLS", "sLCG", "sVelvetNoise", "sMLSParams", "sLCGParams", "sVelvetParams", "sColorParams", "enGenerator", "fAmplitude", "fOffset"]
    assert [k[2:] for k in stored["SpectralTilt"]["keys"] if k.startswith("0:")][:3] == ["nOrder", "enSlopeType", "enNorm"]


def test_the_mirrors_declare_the_references_public_names_and_members():
    names = json.load(open(os.path.join(GOLDEN, "noise_generator_public_names.json")))
    assert set(names) == set(gen.HEADERS)
    members = {"SpectralTilt": ("nOrder", "enSlopeUnit", "enNorm", "fSlopeVal", "fSlopeNepNep", "fLowerFrequency", "fUpperFrequency", "nSampleRate", "bBypass",
                                "bSync", "sFilter"),
               "NoiseGenerator": ("sMLS", "sLCG", "sVelvetNoise", "sColorFilter", "sMLSParams", "sLCGParams", "sVelvetParams", "sColorParams", "nSampleRate",
                                  "enGenerator", "fAmplitude", "fOffset", "nUpdate")}
    for header, cls in gen.HEADERS.items():
        path = os.path.join(INCLUDE, header)
        assert gen.public_names(path, cls) == names[header], header
        text = re.sub(r"//.*", "", open(path).read())
        for deleted in ("%s(const %s &) = delete" % (cls, cls), "%s(%s &&) = delete" % (cls, cls)):
            assert deleted in text, deleted
        body = text[text.index("private:"):]
        at = [re.search(r"\b%s;" % n, body).start() for n in members[cls]]
        assert at == sorted(at), cls                        # in the reference's order
    text = open(os.path.join(INCLUDE, "filters", "SpectralTilt.h")).read() + open(os.path.join(INCLUDE, "noise", "Generator.h")).read()
    for enum in ("STLT_SLOPE_UNIT_NEPER_PER_NEPER", "STLT_SLOPE_UNIT_DB_PER_OCTAVE", "STLT_SLOPE_UNIT_DB_PER_DECADE", "STLT_SLOPE_UNIT_NONE", "STLT_SLOPE_UNIT_MAX",
                 "STLT_NORM_AT_DC", "STLT_NORM_AT_20_HZ", "STLT_NORM_AT_1_KHZ", "STLT_NORM_AT_20_KHZ", "STLT_NORM_AT_NYQUIST", "STLT_NORM_AUTO", "STLT_NORM_NONE",
                 "STLT_NORM_MAX", "NG_GEN_MLS", "NG_GEN_LCG", "NG_GEN_VELVET", "NG_COLOR_WHITE", "NG_COLOR_PINK", "NG_COLOR_RED", "NG_COLOR_BLUE", "NG_COLOR_VIOLET",
                 "NG_COLOR_ARBITRARY", "NG_COLOR_BROWN", "NG_COLOR_BROWNIAN"):
        assert re.search(r"\b%s\b" % enum, text), enum


def test_the_library_exports_the_classes(mi):
    out = subprocess.check_output(["nm", "-D", "--defined-only", "-C", mi.LIB_PATH]).decode()
    T, N = "lsp::dspu::SpectralTilt::", "lsp::dspu::NoiseGenerator::"
    for sym in (T + "SpectralTilt()", T + "construct()", T + "destroy()", T + "init()", T + "set_order(unsigned long)",
                T + "set_slope(float, lsp::dspu::stlt_slope_unit_t)", T + "set_norm(lsp::dspu::stlt_norm_t)", T + "set_lower_frequency(float)",
                T + "set_upper_frequency(float)", T + "set_frequency_range(float, float)", T + "set_sample_rate(unsigned long)",
                T + "process_add(float*, float const*, unsigned long)", T + "process_mul(float*, float const*, unsigned long)",
                T + "process_overwrite(float*, float const*, unsigned long)", T + "freq_chart(float*, float*, float const*, unsigned long)",
                T + "freq_chart(float*, float const*, unsigned long)", T + "dump(lsp::dspu::IStateDumper*) const", T + "update_settings()",
                T + "bilinear_coefficient(float, float)", T + "compute_bilinear_element(float, float)", T + "normalise_digital_biquad(lsp::dsp::biquad_x1_t*)",
                T + "complex_transfer_calc(float*, float*, float)",
                N + "NoiseGenerator()", N + "construct()", N + "destroy()", N + "init(unsigned char, unsigned long, unsigned int, unsigned int, unsigned char, unsigned long)",
                N + "init()", N + "set_sample_rate(unsigned long)", N + "set_mls_n_bits(unsigned char)", N + "set_mls_seed(unsigned long)",
                N + "set_lcg_distribution(lsp::dspu::lcg_dist_t)", N + "set_velvet_type(lsp::dspu::vn_velvet_type_t)", N + "set_velvet_window_width(float)",
                N + "set_velvet_arn_delta(float)", N + "set_velvet_crush(bool)", N + "set_velvet_crushing_probability(float)",
                N + "set_generator(lsp::dspu::ng_generator_t)", N + "set_noise_color(lsp::dspu::ng_color_t)", N + "set_coloring_order(unsigned long)",
                N + "set_color_slope(float, lsp::dspu::stlt_slope_unit_t)", N + "set_amplitude(float)", N + "set_offset(float)",
                N + "process_add(float*, float const*, unsigned long)", N + "process_mul(float*, float const*, unsigned long)",
                N + "process_overwrite(float*, unsigned long)", N + "freq_chart(float*, float*, float const*, unsigned long)",
                N + "freq_chart(float*, float const*, unsigned long)", N + "dump(lsp::dspu::IStateDumper*) const", N + "do_process(float*, unsigned long)",
                N + "update_settings()", "mi_noise_generator_bank_process", "mi_spectral_tilt_bank_process"):
        assert sym in out, sym
