"""PeakMeter and SurgeProtector without a device: the float32 restatement against the reference's recorded outputs and final state
bit for bit (every case), the host designer's fTau and nHold against the recorded ones and against this machine's expf and logf,
the gain's closed form against the branches, the mirror headers (size, names, dump order, setters' rules), refusals that need no
device and the rounding of the PeakMeter's chain function."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import isa_rounding
import peak_surge_ref as ps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "lsp-dsp-units_amd")
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_peak_surge_vectors as gen  # noqa: E402

f32 = np.float32
u32 = np.uint32


def _f(word):
    return u32(word).view(f32)


def _settings(case):
    """(sample rate, hold ms, release ms) as the case's setters leave them -- a fresh meter's where there are none."""
    sr, hold, rel = 0, f32(5.0), f32(0.0)
    for what, arg in case["ops"]:
        what, arg = int(what), int(arg)
        if what == gen.P_SET_SR:
            sr = arg
        elif what == gen.P_SET_HOLD:
            hold = _f(arg)
        elif what == gen.P_SET_RELEASE:
            rel = _f(arg)
    return sr, hold, rel


def replay_peakmeter(case, x, design):
    """A recorded PeakMeter case through the restatement; design(sr, hold, release) -> (tau, hold in samples) stands for
    update_settings().  Returns (out, [fPeak bits, nCounter, fTau bits, nHold])."""
    m = ps.PeakMeters([f32(1.0)], [0])
    sr, hold, rel, stale = 0, f32(5.0), f32(0.0), True
    out, at = np.zeros(gen.N, f32), 0

    def settle():
        nonlocal stale
        if stale:
            tau, h = design(sr, hold, rel)
            m.tau[0], m.hold[0] = tau, h
            stale = False

    for what, arg in case["ops"]:
        what, arg = int(what), int(arg)
        if what == gen.P_SET_SR:
            sr, stale = arg, stale or arg != sr
        elif what == gen.P_SET_HOLD:
            stale, hold = stale or _f(arg) != hold, _f(arg)
        elif what == gen.P_SET_RELEASE:
            stale, rel = stale or _f(arg) != rel, _f(arg)
        elif what == gen.P_CLEAR:
            m.clear()
        elif what in (gen.P_PROCESS, gen.P_PROCESS_STATE):
            settle()
            o = m.process(x[None, at:at + arg])[0]
            if what == gen.P_PROCESS:
                out[at:at + arg] = o
            else:
                out[at + arg - 1] = o[-1]
            at += arg
        elif what == gen.P_PROCESS_VALUE:
            settle()
            out[at] = m.process_value(x[at:at + 1], arg)[0]
            at += 1
    assert at == gen.N
    return out, [int(m.peak.view(u32)[0]), int(m.counter[0]), int(m.tau.view(u32)[0]), int(m.hold[0])]


def replay_surge(case, x, audio):
    """A recorded SurgeProtector case through the restatement: (out, [fGain bits, nTransitionTime, nShutdownTime, bOn])."""
    m = ps.SurgeProtectors(1)
    out, at = np.zeros(gen.N, f32), 0
    for what, arg in case["ops"]:
        what, arg = int(what), int(arg)
        if what == gen.S_SET_TRANSITION:
            m.set_transition_time(0, arg)
        elif what == gen.S_SET_SHUTDOWN:
            m.set_shutdown_time(0, arg)
        elif what == gen.S_SET_ON:
            m.on_thr[0] = _f(arg)
        elif what == gen.S_SET_OFF:
            m.off_thr[0] = _f(arg)
        elif what == gen.S_RESET:
            m.reset()
        else:
            g = m.process(x[None, at:at + arg])[0]
            if what == gen.S_PROCESS:
                out[at:at + arg] = g
            elif what == gen.S_PROCESS_MUL:
                out[at:at + arg] = audio[at:at + arg] * g
            at += arg
    assert at == gen.N
    return out, [int(m.gain.view(u32)[0]), int(m.t[0]), int(m.sd[0]), int(m.on[0])]


def _same(got, want):
    """bit for bit, NaN at the same positions counting as equal whatever its payload"""
    got, want = np.asarray(got, f32), np.asarray(want, f32)
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(u32)[~nan], want.view(u32)[~nan])


def test_restatement_equals_the_references_recorded_outputs():
    """tests/golden/peak_surge_ref_vectors.npz: the reference's two .cpp files compiled unmodified, 40 cases, none left out."""
    x, cases = gen.load()
    assert len(cases) == 40 and {c["kind"] for c in cases} == {gen.PEAKMETER, gen.SURGE}
    holds, transitions, shutdowns = set(), set(), set()
    for c in cases:
        if c["kind"] == gen.PEAKMETER:
            out, words = replay_peakmeter(c, x[c["signal"]], ps.design)
            holds.add(int(c["state"][3]))
            nan_state = np.isnan(_f(c["state"][0]))
            assert nan_state == bool(np.isnan(_f(words[0]))), c["name"]
            if nan_state:
                words[0] = int(c["state"][0])
        else:
            out, words = replay_surge(c, x[c["signal"]], x[gen.AUDIO])
            transitions |= {int(a) for w, a in c["ops"] if w == gen.S_SET_TRANSITION}
            shutdowns |= {int(a) for w, a in c["ops"] if w == gen.S_SET_SHUTDOWN}
        assert _same(out, c["out"]), (c["name"], np.flatnonzero(out.view(u32) != c["out"].view(u32))[:4].tolist())
        assert words == [int(v) for v in c["state"]], (c["name"], words, c["state"])
    assert holds >= set(gen.HOLDS) | {40} and transitions >= set(gen.TRANSITIONS) | {5, 100} and shutdowns >= set(gen.SHUTDOWNS) | {20}


def test_recorded_cases_reach_what_they_are_there_for():
    x, cases = gen.load()
    by = {c["name"]: c for c in cases}
    tiny = f32(np.finfo(f32).tiny)
    o = by["peakmeter hold 1 release 0.0369"]["out"]
    assert np.any((o > 0) & (o < tiny)) and np.all(o[900:1000] == 0.0)              # through the subnormals to 0
    assert np.all(by["peakmeter hold 0 tau above half"]["out"][900:1000].view(u32) == 1)    # ... or stuck at the smallest one
    c = by["peakmeter fresh (5 ms at rate 0, release 0)"]
    assert c["state"][2] == 0 and c["state"][3] == 0                                # tau = expf(-inf) = 0
    o = by["peakmeter NaN and Inf tau 0"]["out"]
    assert np.isnan(o).any() and np.isposinf(o).any()                               # inf * 0
    c = by["peakmeter clear()"]
    assert np.all(c["out"][300:330] == f32(0.75)) and c["out"][270] < f32(0.1)      # the plateau, s == peak, after a clear() at 270
    o = by["surge transition 255, then 5 and 100 at a counter of 50"]["out"]
    assert o[139] == np.sqrt(f32(49) / f32(255)) and o[140] == np.sqrt(f32(5) / f32(100))
    o = by["surge NaN level"]["out"]
    assert not np.isnan(o).any() and o[50] == 0.0                                   # NaN never passes a >=


def _compute(mi, sr, hold, release):
    from importlib import import_module
    capi = import_module("lsp-dsp-units_amd.capi")
    p = capi.PeakMeterParams()
    code = mi.lib.mi_peakmeter_compute_params(sr, float(hold), float(release), ctypes.byref(p))
    return code, p


def test_host_designer_against_the_reference_and_this_machines_libm(mi):
    """nHold is the recorded one.  fTau is, bit for bit, what this machine's expf and logf give for the same float32 expression
    (peak_surge_ref.design calls them through ctypes), and within 1 ulp of the recorded value: glibc documents both functions to
    under 1 ulp, and the logarithm's error, divided by the sample count, is far below the ulp of a result near 1."""
    x, cases = gen.load()
    seen = set()
    for c in cases:
        if c["kind"] != gen.PEAKMETER:
            continue
        sr, hold, rel = _settings(c)
        code, p = _compute(mi, sr, hold, rel)
        assert code == 0, c["name"]
        assert p.hold == int(c["state"][3]), c["name"]
        tau, h = ps.design(sr, hold, rel)
        assert h == p.hold and int(f32(p.tau).view(u32)) == int(tau.view(u32)), c["name"]
        assert abs(int(f32(p.tau).view(u32)) - int(c["state"][2])) <= 1, (c["name"], p.tau, _f(c["state"][2]))
        seen.add((sr, float(hold), float(rel)))
    assert len(seen) >= 12


def test_hold_times_the_reference_cannot_convert_are_refused(mi):
    """uint32_t(float) is undefined below 0, for NaN and from 2^32 on: MI_EINVAL."""
    for sr, hold in ((48000, -1.0), (48000, float("nan")), (48000, 1e8), (48000, float("inf")), (4000000000, 2000.0)):
        code, _ = _compute(mi, sr, hold, 1.0)
        assert code == -1 and b"hold" in mi.lib.mi_dspu_last_error(), (sr, hold)
    assert _compute(mi, 48000, 89478.0, 1.0)[0] == 0                                # 4294944000 samples: still below 2^32
    assert _compute(mi, 0, -1.0, 1.0)[0] == 0                                       # -0.0 samples are 0
    assert mi.lib.mi_peakmeter_compute_params(48000, 5.0, 1.0, None) == -1


def test_gain_is_a_function_of_the_counter_before_the_step():
    """While nTransitionTime <= nTransitionMax the branches of the reference (SurgeProtector.cpp:126-145, written out below) give
    sqrtf(float(t) / float(max)) for max != 0 and on ? 1 : 0 for max == 0, t the counter BEFORE the step -- what the kernel's helper
    waves compute from the chain's integers.  Random levels around both thresholds with NaN among them, setters and resets on
    the way: 24 configurations, 48000 samples."""
    rng = np.random.default_rng(3)
    toggles = 0
    for cfg in range(24):
        tmax, sdmax = int(rng.choice([0, 1, 2, 7, 100, 300])), int(rng.choice([0, 1, 5, 60]))
        t = sd = 0
        on = False
        level = (rng.random(2000) * (np.repeat(rng.random(40), 50) < 0.6)).astype(f32)
        level[rng.random(2000) < 0.01] = np.nan
        for i, v in enumerate(level):
            if i % 500 == 499:
                tmax = int(rng.choice([0, 3, 50, 300]))
                t = min(t, tmax)                                                    # set_transition_time's clamp
            if i % 700 == 699:
                on, t = False, 0                                                    # reset()
            was = on
            if on:
                sd = 0 if v >= f32(0.25) else sd + 1
                if sd >= sdmax:
                    on = False
            elif v >= f32(0.5):
                on, sd = True, 0
            toggles += was != on
            before = t
            with np.errstate(invalid="ignore", divide="ignore"):
                ramp = np.sqrt(f32(t) / f32(tmax))
            if on:
                if t < tmax:
                    gain, t = ramp, t + 1
                else:
                    gain = f32(1.0)
            elif t > 0:
                gain, t = ramp, t - 1
            else:
                gain = f32(0.0)
            with np.errstate(invalid="ignore", divide="ignore"):
                closed = np.sqrt(f32(before) / f32(tmax)) if tmax != 0 else f32(1.0 if on else 0.0)
            assert f32(gain).view(u32) == f32(closed).view(u32), (cfg, i, before, tmax, on)
    assert toggles > 500


PROBE = r'''
#include <lsp-plug.in/dsp-units/meters/PeakMeter.h>
#include <lsp-plug.in/dsp-units/dynamics/SurgeProtector.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using lsp::dspu::PeakMeter;
using lsp::dspu::SurgeProtector;

struct names: public lsp::dspu::IStateDumper                       // the keys in order, and the values by key
{
    std::vector<std::string> seen, closes;
    std::string values;
    void note(const char *n, double v)                                 { char b[96]; snprintf(b, sizeof(b), " %s=%.9g", n, v); values += b; seen.push_back(n); }
    void end_object() override                                         { closes.push_back("end_object"); }
    void end_array() override                                          { closes.push_back("end_array"); }
    void write(const char *n, bool v) override                         { note(n, v ? 1 : 0); }
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
    float (PeakMeter::*m1)(const float *, size_t) = &PeakMeter::process;
    float (PeakMeter::*m2)(float *, const float *, size_t) = &PeakMeter::process;
    float (PeakMeter::*m3)(float, size_t) = &PeakMeter::process;
    void (PeakMeter::*m4)(float, float) = &PeakMeter::set_time;
    size_t (PeakMeter::*m5)() const = &PeakMeter::sample_rate;
    float (SurgeProtector::*s1)(float) = &SurgeProtector::process;
    void (SurgeProtector::*s2)(const float *, size_t) = &SurgeProtector::process;
    void (SurgeProtector::*s3)(float *, const float *, size_t) = &SurgeProtector::process;
    void (SurgeProtector::*s4)(float *, const float *, size_t) = &SurgeProtector::process_mul;
    void (SurgeProtector::*s5)(size_t) = &SurgeProtector::set_transition_time;
    (void)m1; (void)m2; (void)m3; (void)m4; (void)m5; (void)s1; (void)s2; (void)s3; (void)s4; (void)s5;

    printf("sizeof %zu %zu\n", sizeof(PeakMeter), sizeof(SurgeProtector));

    // construct() on raw memory and the setters' rules, no device involved
    void *raw = malloc(sizeof(PeakMeter));
    memset(raw, 0xa5, sizeof(PeakMeter));
    PeakMeter *p = reinterpret_cast<PeakMeter *>(raw);
    p->construct();
    show("p_fresh", *p);
    p->set_sample_rate(48000);
    p->set_hold_time(10.0f);
    p->set_release_time(20.0f);
    printf("p_get %zu %.9g %.9g %.9g\n", p->sample_rate(), p->hold_time(), p->release_time(), p->value());
    p->set_time(1.0f, 2.0f);
    show("p_set", *p);                                              // lazy: fTau and nHold wait for process()
    p->clear();
    show("p_cleared", *p);
    keys("p", *p);
    p->destroy();
    free(raw);

    raw = malloc(sizeof(SurgeProtector));
    memset(raw, 0xa5, sizeof(SurgeProtector));
    SurgeProtector *s = reinterpret_cast<SurgeProtector *>(raw);
    s->construct();
    show("s_fresh", *s);
    s->set_transition_time(100);
    s->set_shutdown_time(300);
    s->set_on_threshold(0.5f);
    s->set_off_threshold(0.25f);
    show("s_set", *s);
    s->set_threshold(0.75f, 0.125f);
    s->reset();
    show("s_reset", *s);
    keys("s", *s);
    s->destroy();
    show("s_destroyed", *s);
    free(raw);
    return 0;
}
'''


@pytest.fixture(scope="module")
def probe(mi, tmp_path_factory):
    d = tmp_path_factory.mktemp("peak_surge_probe")
    src, exe = str(d / "ps_probe.cpp"), str(d / "ps_probe")
    with open(src, "w") as f:
        f.write(PROBE)
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-I" + os.path.join(PKG, "include"), "-I" + os.path.join(ROOT, "include"),
                           src, "-o", exe, "-L" + PKG, "-lmi_dspu", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.check_output([exe]).decode().splitlines()
    return {l.split()[0]: l.split()[1:] for l in out if l.strip()}


def _fields(words):
    return {w.split("=")[0]: float(w.split("=")[1]) for w in words}


def test_mirror_sizes_are_the_references(probe):
    # four floats, three uint32_t, a bool; a float, four size_t, two floats, a bool
    assert probe["sizeof"] == ["32", "56"]


def test_mirror_setters_follow_the_references_rules(probe):
    f = _fields(probe["p_fresh"])
    assert f == {"fPeak": 0, "fTau": 1, "fHold": 5, "fRelease": 0, "nHold": 0, "nCounter": 0, "nSampleRate": 0, "bUpdate": 1}
    assert probe["p_get"] == ["48000", "10", "20", "0"]
    f = _fields(probe["p_set"])
    assert (f["fHold"], f["fRelease"], f["nSampleRate"], f["bUpdate"], f["fTau"], f["nHold"]) == (1, 2, 48000, 1, 1, 0)
    f = _fields(probe["p_cleared"])
    assert (f["fPeak"], f["nCounter"], f["bUpdate"]) == (0, 0, 1)
    f = _fields(probe["s_fresh"])
    assert all(v == 0 for v in f.values()) and len(f) == 8
    f = _fields(probe["s_set"])
    assert (f["nTransitionMax"], f["nShutdownMax"], f["fOnThreshold"], f["fOffThreshold"]) == (100, 300, 0.5, 0.25)
    f = _fields(probe["s_reset"])
    assert (f["fOnThreshold"], f["fOffThreshold"], f["bOn"], f["nTransitionTime"], f["nTransitionMax"]) == (0.75, 0.125, 0, 0, 100)
    assert all(v == 0 for v in _fields(probe["s_destroyed"]).values())


def test_dump_writes_the_references_keys_in_order(probe):
    for cls, tag in (("peakmeter", "p"), ("surgeprotector", "s")):
        keys = json.load(open(os.path.join(ROOT, "tests", "golden", cls + "_dump_keys.json")))
        assert probe[tag + "_dump"] == keys["keys"], cls
        assert probe.get(tag + "_closes", []) == keys["closes"], cls


def test_mirrors_declare_the_references_public_names():
    names = json.load(open(os.path.join(ROOT, "tests", "golden", "peak_surge_public_names.json")))
    assert set(names) == {"meters/PeakMeter.h", "dynamics/SurgeProtector.h"}
    for header, listed in names.items():
        text = re.sub(r"//.*", "", open(os.path.join(PKG, "include", "lsp-plug.in", "dsp-units", header)).read())
        assert len(listed) >= 10
        for name in listed:
            assert re.search(r"\b%s\b" % name, text), (header, name)
    order = {"meters/PeakMeter.h": ("fPeak", "fTau", "fHold", "fRelease", "nHold", "nCounter", "nSampleRate", "bUpdate"),
             "dynamics/SurgeProtector.h": ("fGain", "nTransitionTime", "nTransitionMax", "nShutdownTime", "nShutdownMax", "fOnThreshold",
                                           "fOffThreshold", "bOn")}
    for header, fields in order.items():
        text = re.sub(r"//.*", "", open(os.path.join(PKG, "include", "lsp-plug.in", "dsp-units", header)).read())
        pos = [re.search(r"\b%s;" % n, text).start() for n in fields]
        assert pos == sorted(pos), "%s: the fields are not in the reference's order" % header


def test_mirrors_export_the_references_symbols(mi):
    out = subprocess.check_output(["nm", "-D", "--defined-only", mi.LIB_PATH]).decode()
    for sym in ("_ZN3lsp4dspu9PeakMeterC1Ev", "_ZN3lsp4dspu9PeakMeterD1Ev", "_ZN3lsp4dspu9PeakMeter9constructEv", "_ZN3lsp4dspu9PeakMeter7destroyEv",
                "_ZN3lsp4dspu9PeakMeter15set_sample_rateEm", "_ZNK3lsp4dspu9PeakMeter11sample_rateEv", "_ZN3lsp4dspu9PeakMeter7processEPKfm",
                "_ZN3lsp4dspu9PeakMeter7processEPfPKfm", "_ZN3lsp4dspu9PeakMeter7processEfm", "_ZN3lsp4dspu9PeakMeter13set_hold_timeEf",
                "_ZN3lsp4dspu9PeakMeter16set_release_timeEf", "_ZN3lsp4dspu9PeakMeter8set_timeEff", "_ZNK3lsp4dspu9PeakMeter5valueEv",
                "_ZN3lsp4dspu9PeakMeter5clearEv", "_ZN3lsp4dspu9PeakMeter15update_settingsEv", "_ZNK3lsp4dspu9PeakMeter4dumpEPNS0_12IStateDumperE",
                "_ZN3lsp4dspu14SurgeProtectorC1Ev", "_ZN3lsp4dspu14SurgeProtectorD1Ev", "_ZN3lsp4dspu14SurgeProtector9constructEv",
                "_ZN3lsp4dspu14SurgeProtector7destroyEv", "_ZN3lsp4dspu14SurgeProtector5resetEv", "_ZN3lsp4dspu14SurgeProtector19set_transition_timeEm",
                "_ZN3lsp4dspu14SurgeProtector17set_shutdown_timeEm", "_ZN3lsp4dspu14SurgeProtector16set_on_thresholdEf",
                "_ZN3lsp4dspu14SurgeProtector17set_off_thresholdEf", "_ZN3lsp4dspu14SurgeProtector13set_thresholdEff",
                "_ZN3lsp4dspu14SurgeProtector7processEf", "_ZN3lsp4dspu14SurgeProtector7processEPKfm", "_ZN3lsp4dspu14SurgeProtector7processEPfPKfm",
                "_ZN3lsp4dspu14SurgeProtector11process_mulEPfPKfm", "_ZNK3lsp4dspu14SurgeProtector4dumpEPNS0_12IStateDumperE"):
        assert re.search(r" T %s$" % re.escape(sym), out, re.M), sym


def test_refusals(mi):
    """NULL handles are refused, never followed."""
    lib = mi.lib
    byref, h = ctypes.byref, ctypes.c_void_p()
    assert lib.mi_peakmeter_bank_set_sample_rate(None, 0, 48000) == -5 and lib.mi_peakmeter_bank_set_hold_time(None, 0, 1.0) == -5
    assert lib.mi_peakmeter_bank_set_release_time(None, 0, 1.0) == -5 and lib.mi_peakmeter_bank_set_time(None, 0, 1.0, 1.0) == -5
    assert lib.mi_peakmeter_bank_clear(None, 0) == -5 and lib.mi_peakmeter_bank_update_settings(None, None) == -5
    assert lib.mi_peakmeter_bank_get_params(None, 0, None) == -5 and lib.mi_peakmeter_bank_set_params(None, 0, None) == -1
    assert lib.mi_peakmeter_bank_get_state(None, 0, None, None) == -5 and lib.mi_peakmeter_bank_set_state(None, 0, None, None) == -5
    assert lib.mi_peakmeter_bank_process(None, None, None, None, 4, 4, 4, None) == -5
    assert lib.mi_peakmeter_bank_process_value(None, None, None, 4, None) == -5
    assert lib.mi_peakmeter_bank_destroy(None) == 0
    assert lib.mi_peakmeter_bank_create(None, 1) == -1 and lib.mi_dspu_last_error()
    assert lib.mi_peakmeter_bank_create(byref(h), 0) == -1 and not h.value
    for what in ("set_transition_time", "set_shutdown_time"):
        assert getattr(lib, "mi_surge_bank_" + what)(None, 0, 5) == -5
    for what in ("set_on_threshold", "set_off_threshold"):
        assert getattr(lib, "mi_surge_bank_" + what)(None, 0, 0.5) == -5
    assert lib.mi_surge_bank_set_threshold(None, 0, 0.5, 0.25) == -5 and lib.mi_surge_bank_reset(None, 0) == -5
    assert lib.mi_surge_bank_get_params(None, 0, None) == -5 and lib.mi_surge_bank_get_state(None, 0, None, None) == -5
    assert lib.mi_surge_bank_set_state(None, 0, None, None) == -5
    assert lib.mi_surge_bank_process(None, None, None, 4, 4, 4, None) == -5 and lib.mi_surge_bank_process_mul(None, None, None, 4, 4, 4, None) == -5
    assert lib.mi_surge_bank_destroy(None) == 0
    assert lib.mi_surge_bank_create(None, 1) == -1 and lib.mi_surge_bank_create(byref(h), 0) == -1 and not h.value


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_peakmeter_chain_keeps_its_multiply(tmp_path):
    """The decay is one product rounded once: no fused multiply-add in the chain's body under the Makefile's -ffp-contract=on."""
    isa_rounding.assert_separate_multiplies_and_adds(tmp_path, "peakmeter.hip", "peakmeter_chain_tile")
