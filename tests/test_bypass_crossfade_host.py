"""Bypass and Crossfade without a device: the float32 restatement against the reference's recorded outputs, answers and final
state bit for bit (every case), what the recorded cases are there for, init()'s refusals, the mirror headers (sizes, names, field
order, dump keys, the host-side members' rules) and refusals that need no device."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import bypass_crossfade_ref as bc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "lsp-dsp-units_amd")
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_bypass_crossfade_vectors as gen  # noqa: E402

f32 = np.float32
u32 = np.uint32


@pytest.fixture(scope="module")
def recorded():
    return gen.load()


def _final(unit, kind):
    return list(unit.fields()) + [0] if kind == bc.BYPASS else [unit.samples] + list(unit.fields())


def test_restatement_equals_the_references_recorded_outputs(recorded):
    x, cases = recorded
    assert len(cases) >= 70 and {c["kind"] for c in cases} == {bc.BYPASS, bc.CROSSFADE}
    for c in cases:
        unit = bc.Bypass() if c["kind"] == bc.BYPASS else bc.Crossfade()
        out, copied, answers = bc.replay(c, x, unit)
        assert bc.same(out, c["out"], copied), c["name"]
        assert np.array_equal(answers, c["answers"]), c["name"]
        assert [int(v) for v in _final(unit, c["kind"])] == [int(v) for v in c["state"]], c["name"]


def test_the_generator_still_makes_the_recorded_cases(recorded):
    """The committed operation lists and signals are the generator's (the outputs need the reference tree)."""
    x, cases = recorded
    assert np.array_equal(x.view(u32), gen.signals().view(u32))
    made = gen.cases()
    assert [c[0] for c in made] == [c["name"] for c in cases]
    for m, c in zip(made, cases):
        assert np.array_equal(m[3], c["ops"]) and tuple(m[2]) == tuple(c["signal"]) and m[1] == c["kind"], m[0]
    gen.check_branches(made, np.array([c["out"] for c in cases]), np.array([c["state"] for c in cases]),
                       np.concatenate([c["answers"] for c in cases]))


def test_recorded_cases_cover_what_the_issue_lists(recorded):
    x, cases = recorded
    lengths, variants, calls, gains, combos = set(), set(), set(), set(), set()
    for c in cases:
        for what, arg, flags, u, v in c["ops"]:
            if c["kind"] == bc.BYPASS and what == bc.B_INIT:
                lengths.add(int(bc.ramp_length(int(arg), bc.flt(u))))
            elif c["kind"] == bc.BYPASS and what >= bc.B_PROCESS:
                variants.add((int(what), bool(flags & bc.HAS_A)))
                calls.add(int(arg))
                gains.update((float(bc.flt(u)), float(bc.flt(v))))
            elif c["kind"] == bc.CROSSFADE and what == bc.X_PROCESS:
                combos.add(int(flags))
    assert lengths >= {1, 2, 7, 240, 300, 5000}
    assert len(variants) == 6 and calls >= {1, 7, 256, 936} and combos == {0, 1, 2, 3}
    assert gains >= {0.0, 1.0, -0.5, float(f32(1e-30))}
    sub = np.abs(x[gen.SUBNORMAL])
    assert sub[sub > 0].min() == f32(1.4e-45) and sub.max() < np.finfo(f32).tiny
    assert np.isnan(x[gen.SPECIAL]).any() and np.isposinf(x[gen.SPECIAL]).any() and np.isneginf(x[gen.SPECIAL]).any()


def test_a_ramp_is_as_long_as_the_running_sum_says():
    """g0 + k * delta is not the gain: the number of ramp samples is known only by walking."""
    differs = 0
    for length in (7, 240, 300, 5000, 1000, 48000 * 0.005, 44100 * 0.005):
        b = bc.Bypass()
        b.init(1, length)
        b.set_bypass(True)
        n = int(length) + 8
        out, _ = b.process(None, np.ones(n, f32))
        steps = int(np.count_nonzero(out))
        closed = f32(1.0) + np.arange(n, dtype=f32) * b.delta
        differs += int(not np.array_equal(out[:steps], closed[:steps])) + int(steps != int(length))
        assert b.state == bc.S_ON and b.gain == 0 and abs(steps - length) <= 1
    assert differs > 0


def test_init_refuses_what_the_reference_cannot_convert(mi):
    lib = mi.lib
    for fn in (lib.mi_bypass_bank_init, lib.mi_crossfade_bank_init):
        for sr, time in ((48000, float("nan")), (48000, 1e6), (1 << 30, 4.0), (48000, float("inf")), (0, float("inf")), (-48000, float("-inf"))):
            assert bc.ramp_length(sr, time) is None
            assert fn(None, 0, sr, time) == -1, (sr, time)          # refused with or without a bank
        for sr, time in ((48000, 0.005), (0, 1.0), (-5, 1.0), (48000, float("-inf")), (65536, 65535.0)):
            assert bc.ramp_length(sr, time) is not None
            assert fn(None, 0, sr, time) == -5, (sr, time)          # nothing wrong with the length: the NULL bank is what is wrong
    assert bc.ramp_length(48000, 0.005) == 240 and bc.ramp_length(0, 1.0) == 1 and bc.ramp_length(-5, 1.0) == 1


def test_refusals(mi):
    """NULL handles are refused, never followed."""
    lib = mi.lib
    byref, h, n = ctypes.byref, ctypes.c_void_p(), ctypes.c_int()
    assert lib.mi_bypass_bank_set_bypass(None, 0, 1, byref(n)) == -5 and lib.mi_bypass_bank_bypassing(None, 0, byref(n), None) == -5
    assert lib.mi_bypass_bank_get_state(None, 0, None, None) == -5 and lib.mi_bypass_bank_set_state(None, 0, None, None) == -5
    assert lib.mi_bypass_bank_process(None, None, None, None, 4, 4, 4, 4, None) == -5
    assert lib.mi_bypass_bank_process_wet(None, None, None, None, 1.0, 4, 4, 4, 4, None) == -5
    assert lib.mi_bypass_bank_process_drywet(None, None, None, None, 1.0, 1.0, 4, 4, 4, 4, None) == -5
    assert lib.mi_bypass_bank_destroy(None) == 0
    assert lib.mi_bypass_bank_create(None, 1) == -1 and lib.mi_dspu_last_error()
    assert lib.mi_bypass_bank_create(byref(h), 0) == -1 and not h.value
    assert lib.mi_crossfade_bank_toggle(None, 0, byref(n)) == -5 and lib.mi_crossfade_bank_reset(None, 0) == -5
    assert lib.mi_crossfade_bank_remaining(None, 0, None) == -5
    assert lib.mi_crossfade_bank_get_state(None, 0, None, None) == -5 and lib.mi_crossfade_bank_set_state(None, 0, None, None) == -5
    assert lib.mi_crossfade_bank_process(None, None, None, None, 4, 4, 4, 4, None) == -5
    assert lib.mi_crossfade_bank_destroy(None) == 0
    assert lib.mi_crossfade_bank_create(None, 1) == -1 and lib.mi_crossfade_bank_create(byref(h), 0) == -1 and not h.value


PROBE = r'''
#include <lsp-plug.in/dsp-units/ctl/Bypass.h>
#include <lsp-plug.in/dsp-units/ctl/Crossfade.h>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using lsp::dspu::Bypass;
using lsp::dspu::Crossfade;

struct names: public lsp::dspu::IStateDumper                       // the keys in order, and the values by key
{
    std::vector<std::string> seen, closes;
    std::string values;
    void note(const char *n, double v)                                 { char b[96]; snprintf(b, sizeof(b), " %s=%.9g", n, v); values += b; seen.push_back(n); }
    void end_object() override                                         { closes.push_back("end_object"); }
    void end_array() override                                          { closes.push_back("end_array"); }
    void write(const char *n, signed int v) override                   { note(n, v); }
    void write(const char *n, unsigned int v) override                 { note(n, v); }
    void write(const char *n, unsigned long v) override                { note(n, double(v)); }
    void write(const char *n, float v) override                        { note(n, v); }
};

template <class M> static void show(const char *label, const M &m)
{
    names n;
    m.dump(&n);
    printf("%s%s\n", label, n.values.c_str());
}

template <class M> static void keys(const char *label, const M &m)
{
    names n;
    m.dump(&n);
    printf("%s_dump", label);
    for (const std::string &s: n.seen)
        printf(" %s", s.c_str());
    printf("\n%s_closes", label);
    for (const std::string &s: n.closes)
        printf(" %s", s.c_str());
    printf("\n");
}

int main()
{
    // the public surface, by address
    void (Bypass::*b1)(int, float) = &Bypass::init;
    void (Bypass::*b2)(float *, const float *, const float *, size_t) = &Bypass::process;
    void (Bypass::*b3)(float *, const float *, const float *, float, size_t) = &Bypass::process_wet;
    void (Bypass::*b4)(float *, const float *, const float *, float, float, size_t) = &Bypass::process_drywet;
    bool (Bypass::*b5)(bool) = &Bypass::set_bypass;
    bool (Bypass::*b6)(float) = &Bypass::set_bypass;
    bool (Bypass::*b7)() const = &Bypass::bypassing;
    void (Crossfade::*c1)(int, float) = &Crossfade::init;
    void (Crossfade::*c2)(float *, const float *, const float *, size_t) = &Crossfade::process;
    size_t (Crossfade::*c3)() const = &Crossfade::remaining;
    bool (Crossfade::*c4)() = &Crossfade::toggle;
    (void)b1; (void)b2; (void)b3; (void)b4; (void)b5; (void)b6; (void)b7; (void)c1; (void)c2; (void)c3; (void)c4;

    printf("sizeof %zu %zu\n", sizeof(Bypass), sizeof(Crossfade));

    // construct() on raw memory and the host-side members' rules, no device involved
    void *raw = malloc(sizeof(Bypass));
    memset(raw, 0xa5, sizeof(Bypass));
    Bypass *b = reinterpret_cast<Bypass *>(raw);
    b->construct();
    show("b_fresh", *b);
    printf("b_fresh_is %d %d %d %d\n", b->on(), b->active(), b->off(), b->bypassing());
    b->init(48000);
    show("b_init", *b);
    const int a0 = b->set_bypass(false), a1 = b->set_bypass(true), a2 = b->set_bypass(0.75f), a3 = b->bypassing(), a4 = b->active(),
              a5 = b->set_bypass(0.25f), a6 = b->bypassing();
    printf("b_answers %d %d %d %d %d %d %d\n", a0, a1, a2, a3, a4, a5, a6);
    show("b_switched", *b);
    b->init(48000, 0.0f);
    show("b_short", *b);
    b->init(48000, NAN);
    show("b_nan", *b);
    keys("b", *b);
    b->destroy();
    show("b_destroyed", *b);
    free(raw);

    raw = malloc(sizeof(Crossfade));
    memset(raw, 0xa5, sizeof(Crossfade));
    Crossfade *c = reinterpret_cast<Crossfade *>(raw);
    c->construct();
    show("c_fresh", *c);
    c->init(48000);
    show("c_init", *c);
    const int t0 = c->toggle(), t1 = c->toggle();
    printf("c_answers %d %d %zu %d\n", t0, t1, c->remaining(), int(c->active()));
    show("c_toggled", *c);
    c->reset();
    show("c_reset", *c);
    printf("c_after_reset %zu %d\n", c->remaining(), c->active());
    c->init(48000, -1.0f);
    show("c_short", *c);
    c->init(48000, NAN);
    show("c_nan", *c);
    c->init(1 << 30, 1e30f);
    show("c_huge", *c);
    keys("c", *c);
    c->destroy();
    free(raw);
    return 0;
}
'''


@pytest.fixture(scope="module")
def probe(mi, tmp_path_factory):
    d = tmp_path_factory.mktemp("bypass_crossfade_probe")
    src, exe = str(d / "bc_probe.cpp"), str(d / "bc_probe")
    with open(src, "w") as f:
        f.write(PROBE)
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-I" + os.path.join(PKG, "include"), "-I" + os.path.join(ROOT, "include"),
                           src, "-o", exe, "-L" + PKG, "-lmi_dspu", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.check_output([exe]).decode().splitlines()
    return {l.split()[0]: l.split()[1:] for l in out if l.strip()}


def _fields(words):
    return {w.split("=")[0]: float(w.split("=")[1]) for w in words}


def test_mirror_sizes_are_the_references(probe):
    # an enum and two floats; two size_t and two floats
    assert probe["sizeof"] == ["12", "24"]


def test_mirror_host_members_follow_the_references_rules(probe):
    assert _fields(probe["b_fresh"]) == {"nState": bc.S_OFF, "fDelta": 0, "fGain": 0}
    assert probe["b_fresh_is"] == ["0", "0", "1", "0"]
    want = bc.Bypass()
    want.init(48000, 0.005)
    f = _fields(probe["b_init"])
    assert (f["nState"], f32(f["fDelta"]), f["fGain"]) == (bc.S_OFF, want.delta, 1)
    # off: switching off changes nothing; on: changed; on again: nothing; now bypassing and active; off again: changed
    assert probe["b_answers"] == ["0", "1", "0", "1", "1", "1", "0"]
    f = _fields(probe["b_switched"])
    assert (f["nState"], f32(f["fDelta"]), f["fGain"]) == (bc.S_ACTIVE, want.delta, 1)
    assert _fields(probe["b_short"])["fDelta"] == 1
    assert np.isnan(_fields(probe["b_nan"])["fDelta"])
    assert _fields(probe["b_destroyed"]) == {"nState": bc.S_OFF, "fDelta": 0, "fGain": 0}
    assert _fields(probe["c_fresh"]) == {"nSamples": 0, "nCounter": 0, "fDelta": 0, "fGain": 1}
    assert _fields(probe["c_init"]) == {"nSamples": 240, "nCounter": 0, "fDelta": 0, "fGain": 1}
    assert probe["c_answers"] == ["1", "0", "240", "1"]
    f = _fields(probe["c_toggled"])
    assert (f["nSamples"], f["nCounter"], f32(f["fDelta"]), f["fGain"]) == (240, 240, f32(1.0) / f32(240.0), 0)
    assert _fields(probe["c_reset"]) == {"nSamples": 240, "nCounter": 0, "fDelta": 0, "fGain": 0}
    assert probe["c_after_reset"] == ["0", "0"]
    assert _fields(probe["c_short"])["nSamples"] == 1 and _fields(probe["c_nan"])["nSamples"] == 1
    assert abs(_fields(probe["c_huge"])["nSamples"] - (2 ** 32 - 1)) < 8             # (printed with nine digits)


def test_dump_writes_the_references_keys_in_order(probe):
    for cls, tag in (("bypass", "b"), ("crossfade", "c")):
        keys = json.load(open(os.path.join(ROOT, "tests", "golden", cls + "_dump_keys.json")))
        assert len(keys["keys"]) >= 3
        assert probe[tag + "_dump"] == keys["keys"], cls
        assert probe.get(tag + "_closes", []) == keys["closes"], cls


def test_mirrors_declare_the_references_public_names():
    names = json.load(open(os.path.join(ROOT, "tests", "golden", "bypass_crossfade_public_names.json")))
    assert set(names) == {"ctl/Bypass.h", "ctl/Crossfade.h"}
    for header, listed in names.items():
        text = re.sub(r"//.*", "", open(os.path.join(PKG, "include", "lsp-plug.in", "dsp-units", header)).read())
        assert len(listed) >= 10
        for name in listed:
            assert re.search(r"\b%s\b" % name, text), (header, name)
        # the generator's own reading of the mirror header gives the same list: nothing public is missing or added
        assert gen.public_names(os.path.join(PKG, "include", "lsp-plug.in", "dsp-units", header), os.path.basename(header)[:-2]) == listed
        cls = os.path.basename(header)[:-2]
        for deleted in ("%s(const %s &) = delete" % (cls, cls), "%s(%s &&) = delete" % (cls, cls), "operator = (const %s &) = delete" % cls,
                        "operator = (%s &&) = delete" % cls):
            assert deleted in text, (header, deleted)
    order = {"ctl/Bypass.h": ("nState", "fDelta", "fGain"), "ctl/Crossfade.h": ("nSamples", "nCounter", "fDelta", "fGain")}
    for header, fields in order.items():
        text = re.sub(r"//.*", "", open(os.path.join(PKG, "include", "lsp-plug.in", "dsp-units", header)).read())
        pos = [re.search(r"\b%s;" % n, text).start() for n in fields]
        assert pos == sorted(pos), "%s: the fields are not in the reference's order" % header
    text = open(os.path.join(PKG, "include", "lsp-plug.in", "dsp-units", "ctl", "Bypass.h")).read()
    assert re.search(r"private:\s*enum state_t\s*\{\s*S_ON,[^}]*S_ACTIVE,[^}]*S_OFF[^}]*\}", re.sub(r"//.*", "", text)), "the enum's order and access"
    assert re.search(r"protected:\s*size_t\s+nSamples;", re.sub(r"//.*", "", open(os.path.join(PKG, "include", "lsp-plug.in", "dsp-units", "ctl",
                                                                                              "Crossfade.h")).read()))


def test_mirrors_export_the_references_symbols(mi):
    out = subprocess.check_output(["nm", "-D", "--defined-only", mi.LIB_PATH]).decode()
    for sym in ("_ZN3lsp4dspu6BypassC1Ev", "_ZN3lsp4dspu6BypassD1Ev", "_ZN3lsp4dspu6Bypass9constructEv", "_ZN3lsp4dspu6Bypass7destroyEv",
                "_ZN3lsp4dspu6Bypass4initEif", "_ZN3lsp4dspu6Bypass7processEPfPKfS4_m", "_ZN3lsp4dspu6Bypass11process_wetEPfPKfS4_fm",
                "_ZN3lsp4dspu6Bypass14process_drywetEPfPKfS4_ffm", "_ZN3lsp4dspu6Bypass10set_bypassEb", "_ZNK3lsp4dspu6Bypass9bypassingEv",
                "_ZNK3lsp4dspu6Bypass4dumpEPNS0_12IStateDumperE",
                "_ZN3lsp4dspu9CrossfadeC1Ev", "_ZN3lsp4dspu9CrossfadeD1Ev", "_ZN3lsp4dspu9Crossfade9constructEv", "_ZN3lsp4dspu9Crossfade7destroyEv",
                "_ZN3lsp4dspu9Crossfade4initEif", "_ZN3lsp4dspu9Crossfade7processEPfPKfS4_m", "_ZN3lsp4dspu9Crossfade5resetEv",
                "_ZN3lsp4dspu9Crossfade6toggleEv", "_ZNK3lsp4dspu9Crossfade4dumpEPNS0_12IStateDumperE"):
        assert re.search(r" T %s$" % re.escape(sym), out, re.M), sym
