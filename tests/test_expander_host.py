"""Expander without a device: update_settings() (mi_expander_compute_params) against float64 over a grid of settings, the
float32 restatement of the curve inside the derived gain bound, the follower restatement on a hand-checked vector, the mirror
header (layout, names, dump order, setters) and the rounding contract of the follower's ISA."""
import itertools
import json
import os
import re
import subprocess

import numpy as np
import pytest

import expander_ref as er
import isa_rounding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "lsp-dsp-units_amd")
f32 = np.float32


def _cases():
    """Thresholds -60 .. -6 dB, knees 0.063 .. 1, ratios 1 .. 20, both modes; then the channels of the device tests."""
    base = dict(sample_rate=48000, release_threshold=0.05, attack=1.5, release=40.0, hold=2.7)
    out = [dict(base, mode=m, attack_threshold=float(f32(10.0 ** (db / 20.0))), knee=kn, ratio=ra)
           for m, db, kn, ra in itertools.product((er.EM_DOWNWARD, er.EM_UPWARD), (-60.0, -36.0, -18.0, -6.0),
                                                  (0.063, 0.25, 0.7, 1.0), (1.0, 1.5, 4.0, 20.0))]
    return out + [er.channel_settings(ch) for ch in range(16)]


CASES = _cases()


@pytest.mark.parametrize("case", range(len(CASES)))
def test_update_settings_against_float64(mi, case):
    s = CASES[case]
    got = mi.ExpanderBank.compute_params(**s)
    assert got["hold"] == er.hold_samples(s["sample_rate"], s["hold"])                  # nHold: exact
    assert got["upward"] == (1 if s["mode"] == er.EM_UPWARD else 0)
    want = er.params64(**s)
    flat = er.flatten(got)
    knee_open = flat["start"] < flat["end"]
    for name, q in want.items():
        if "herm" in name and not knee_open:
            continue                    # start == end: no sample reaches the knee polynomial (it divides by zero there)
        if name == "threshold" and np.isnan(q.v):
            # knee 1 and the threshold taken from the roots of that polynomial: NaN, which the reference's lsp_min / lsp_max
            # turn into the limit
            assert flat[name] == (er.MAX_UPPER_THRESHOLD if s["mode"] == er.EM_UPWARD else er.MIN_LOWER_THRESHOLD), (s, flat[name])
            continue
        assert np.isfinite(q.v), (name, q.v)
        assert abs(flat[name] - q.v) <= q.err, (s, name, flat[name], q.v, abs(flat[name] - q.v) / er.U / max(abs(q.v), 1e-300), q.err)


def test_threshold_takes_both_formulas_and_both_limits(mi):
    """The grid reaches the tilt line's crossing, the knee's roots, and the two limits (the conditions of :224 and :235)."""
    kinds = set()
    for s in CASES:
        p = mi.ExpanderBank.compute_params(**s)["k"]
        t0 = max(float(p["tilt"][0]), er.MINIMUM_TILT)
        with np.errstate(all="ignore"):
            if s["mode"] == er.EM_UPWARD:
                line = np.exp((np.float64(er.UPPER_THRESHOLD) - p["tilt"][1]) / t0)
                kinds.add(("up", "limit" if p["threshold"] == f32(1e6) else "roots" if line < p["end"] else "line"))
            else:
                line = np.exp((np.float64(er.LOWER_THRESHOLD) - p["tilt"][1]) / t0)
                kinds.add(("down", "limit" if p["threshold"] == f32(1e-7) else "roots" if line > p["start"] else "line"))
    assert {("up", "line"), ("up", "limit"), ("down", "line"), ("down", "roots"), ("down", "limit")} <= kinds, kinds


def test_fresh_parameters(mi):
    p = mi.ExpanderBank.compute_params()                        # as constructed: upward, rate 0, times 0 -> tau 1
    assert p["tau_attack"] == 1.0 and p["tau_release"] == 1.0 and p["hold"] == 0 and p["upward"] == 1


def _level_ladder(C):
    db = np.linspace(-140.0, 12.0, 1729)
    x = (10.0 ** (db / 20.0)).astype(f32)
    x[::7] *= -1.0
    return np.tile(x, (C, 1))


def test_float32_curve_is_inside_the_gain_bound(mi):
    params = [mi.ExpanderBank.compute_params(**s) for s in CASES if s["knee"] < 1.0 or s["ratio"] > 1.0]
    x = _level_ladder(len(params))
    for c, p in enumerate(params):      # the limits of the branches and their float32 neighbours
        for i, v in enumerate(p["k"][n] for n in ("start", "end", "threshold")):
            for d, w in enumerate((np.nextafter(f32(v), f32(0)), f32(v), np.nextafter(f32(v), f32(np.inf)))):
                x[c, 3 * i + d] = w
    g32, g64, bound = er.gain32(x, params), er.gain64(x, params), er.gain_bound(x, params)
    assert np.all(np.isfinite(g64)) and np.all(g64 >= 0)
    exact = bound == 0
    assert np.array_equal(g32[exact].astype(np.float64), g64[exact]) and set(np.unique(g64[exact])) <= {0.0, 1.0}
    err = np.abs(g32.astype(np.float64) - g64)[~exact] / g64[~exact] / er.U
    assert np.all(err <= bound[~exact]), (err.max(), (err / bound[~exact]).max())
    assert (err / bound[~exact]).max() > 0.02                   # the bound is of the error's order, not a blanket
    down = np.array([not p["upward"] for p in params])
    assert np.any(g64[down] == 0.0) and np.any(g64[~down] > 1.0) and np.any(g64[down] < 1.0)
    print("gain bound in u: median %.1f, max %.1f; float32 restatement at most %.2f of it"
          % (np.median(bound[~exact]), bound.max(), (err / bound[~exact]).max()))


def test_follower_restatement_on_a_hand_checked_vector():
    """ta = 0.5, tr = 0.25, release threshold 0.5, nHold = 2; every value is exact in float32 and was worked out by hand
    (Expander.cpp:258-278 reads as Compressor.cpp:231-256 does):
       s     d      branch                               e      hold
       1     1      attack, e >= peak: re-arm            0.5    2
       1     0.5    attack, re-arm                       0.75   2
       0.25  -0.5   hold countdown                       0.75   1
       0.25  -0.5   hold countdown                       0.75   0
       0.25  -0.5   release, e > 0.5: tau release        0.625  0
       0.125 -0.5   release, e > 0.5: tau release        0.5    0
       0     -0.5   release, e = 0.5 not above: tau att  0.25   0
       0.25  0      d = 0 is an attack; e >= peak        0.25   2"""
    x = np.array([[1, 1, 0.25, 0.25, 0.25, 0.125, 0, 0.25]], f32)
    st = er.fresh_state(1)
    got, taken = er.follow(x, st, 0.5, 0.25, 0.5, 2)
    assert got[0].tolist() == [0.5, 0.75, 0.75, 0.75, 0.625, 0.5, 0.25, 0.25]
    assert taken == {"attack": 3, "rearm": 3, "hold": 2, "release_above": 2, "release_below": 1}
    assert (st["e"][0], st["peak"][0], st["hold"][0]) == (0.25, 0.25, 2)
    # the product rounds before the sum (see tests/test_compressor_host.py for the numbers)
    t = f32(1.0 + 2.0 ** -12)
    st = {"e": np.array([-1.0], f32), "peak": np.array([-1.0], f32), "hold": np.zeros(1, np.uint32)}
    e, _ = er.follow(np.array([[f32(2.0 ** -12)]], f32), st, t, t, 0.0, 0)
    assert e[0, 0] == f32(2.0 ** -11)


PROBE = r'''
#include <lsp-plug.in/dsp-units/dynamics/Expander.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using lsp::dspu::Expander;

struct names: public lsp::dspu::IStateDumper
{
    std::vector<std::string> seen, closes;
    void begin_object(const char *n, const void *, size_t) override    { seen.push_back(n); }
    void begin_array(const char *n, const void *, size_t) override     { seen.push_back(n); }
    void end_object() override                                         { closes.push_back("end_object"); }
    void end_array() override                                          { closes.push_back("end_array"); }
    void write(const char *n, bool) override                           { seen.push_back(n); }
    void write(const char *n, unsigned int) override                   { seen.push_back(n); }
    void write(const char *n, float) override                          { seen.push_back(n); }
    void writev(const char *n, const float *, size_t) override         { seen.push_back(n); }
};

struct probe: public Expander
{
    static size_t knee_size()   { return sizeof(sExp); }
    float tau_attack() const    { return fTauAttack; }
    unsigned hold_samples() const { return nHold; }
    float start() const         { return sExp.start; }
    float threshold() const     { return sExp.threshold; }
};

#define SETTER(label, a, b) \
    do { m->a; int s1 = m->modified(); m->update_settings(); int s0 = m->modified(); m->a; int s2 = m->modified(); m->b; \
         printf("setter_%s %d %d %d %d\n", label, s1, s0, s2, int(m->modified())); m->update_settings(); } while (0)

int main()
{
    void (Expander::*p1)(float *, float *, const float *, size_t) = &Expander::process;
    float (Expander::*p2)(float *, float) = &Expander::process;
    void (Expander::*c1)(float *, const float *, size_t) = &Expander::curve;
    float (Expander::*c2)(float) = &Expander::curve;
    void (Expander::*a1)(float *, const float *, size_t) = &Expander::amplification;
    float (Expander::*a2)(float) = &Expander::amplification;
    void (Expander::*pv)(lsp::dspu::IStateDumper *) const = &Expander::dump;
    (void)p1; (void)p2; (void)c1; (void)c2; (void)a1; (void)a2; (void)pv;

    printf("sizeof %zu %zu %zu\n", sizeof(Expander), probe::knee_size(), sizeof(lsp::dsp::expander_knee_t));
    printf("modes %d %d\n", int(lsp::dspu::EM_DOWNWARD), int(lsp::dspu::EM_UPWARD));

    void *raw = malloc(sizeof(Expander));
    memset(raw, 0xa5, sizeof(Expander));
    probe *m = reinterpret_cast<probe *>(raw);
    m->construct();
    printf("fresh %d %g %g %g %g %g %g %g %zu %zu %d %d\n", int(m->modified()), m->attack_threshold(), m->release_threshold(),
           m->attack(), m->release(), m->knee(), m->ratio(), m->hold(), m->sample_rate(), m->mode(), int(m->is_upward()),
           int(m->is_downward()));

    SETTER("sample_rate", set_sample_rate(48000), set_sample_rate(44100));
    SETTER("mode", set_mode(lsp::dspu::EM_DOWNWARD), set_mode(lsp::dspu::EM_UPWARD));
    SETTER("attack_threshold", set_attack_threshold(0.25f), set_attack_threshold(0.125f));
    SETTER("release_threshold", set_release_threshold(0.25f), set_release_threshold(0.0625f));
    SETTER("threshold", set_threshold(0.5f, 0.25f), set_threshold(0.5f, 0.125f));
    SETTER("timings", set_timings(10.0f, 100.0f), set_timings(10.0f, 50.0f));
    SETTER("attack", set_attack(5.0f), set_attack(6.0f));
    SETTER("release", set_release(70.0f), set_release(80.0f));
    SETTER("knee", set_knee(0.5f), set_knee(0.25f));
    SETTER("ratio", set_ratio(4.0f), set_ratio(8.0f));
    SETTER("hold", set_hold(3.0f), set_hold(4.0f));
    // set_mode compares "upward or not": 7 is downward, as 0 is
    m->set_mode(lsp::dspu::EM_DOWNWARD); m->update_settings(); m->set_mode(7);
    printf("mode_other %d %zu\n", int(m->modified()), m->mode());
    // the limits: hold to >= 0; the knee is NOT limited
    m->set_knee(1.0f); m->update_settings(); m->set_knee(7.0f);
    printf("limits %d %g", int(m->modified()), m->knee());
    m->set_hold(0.0f); m->update_settings(); m->set_hold(-2.0f);
    printf(" %d %g\n", int(m->modified()), m->hold());

    m->set_sample_rate(48000); m->set_mode(lsp::dspu::EM_DOWNWARD); m->set_threshold(0.25f, 0.125f); m->set_timings(1.0f, 10.0f);
    m->set_knee(0.5f); m->set_ratio(4.0f); m->set_hold(2.0f);
    m->update_settings();
    printf("amplification %.9g %.9g %.9g %.9g\n", m->amplification(0.01f), m->amplification(1.0f), m->amplification(-0.25f),
           m->amplification(0.1f));
    printf("curve %.9g %.9g %.9g %.9g\n", m->curve(0.01f), m->curve(1.0f), m->curve(-0.25f), m->curve(0.1f));
    float in[4] = { 0.01f, 1.0f, -0.25f, 0.1f }, out[4];
    m->amplification(out, in, 4);
    printf("amplification_array %.9g %.9g %.9g %.9g\n", out[0], out[1], out[2], out[3]);
    printf("computed %.9g %u %.9g %.9g\n", m->tau_attack(), m->hold_samples(), m->start(), m->threshold());

    names n;
    m->dump(&n);
    printf("dump");
    for (const std::string &s: n.seen)
        printf(" %s", s.c_str());
    printf("\ncloses");
    for (const std::string &s: n.closes)
        printf(" %s", s.c_str());
    printf("\n");
    m->destroy();
    free(raw);
    return 0;
}
'''


def _probe(tmp_path):
    src = os.path.join(str(tmp_path), "exp_probe.cpp")
    exe = os.path.join(str(tmp_path), "exp_probe")
    with open(src, "w") as f:
        f.write(PROBE)
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-I" + os.path.join(PKG, "include"), "-I" + os.path.join(ROOT, "include"),
                           src, "-o", exe, "-L" + PKG, "-lmi_dspu", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.check_output([exe]).decode().splitlines()
    return {l.split()[0]: l.split()[1:] for l in out}


def test_mirror_header_layout_dump_order_and_setters(mi, tmp_path):
    r = _probe(tmp_path)
    # 11 floats, sExp (8 floats), three uint32_t and two bool: 44 + 32 + 12 + 2, padded to a multiple of 4
    assert r["sizeof"] == ["92", "32", "32"]
    assert r["modes"] == ["0", "1"]
    assert r["fresh"] == ["1", "0", "0", "0", "0", "0", "1", "0", "0", "1", "1", "0"]       # a fresh expander is UPWARD
    for name in ("sample_rate", "mode", "attack_threshold", "release_threshold", "threshold", "timings", "attack", "release",
                 "knee", "ratio", "hold"):
        assert r["setter_" + name] == ["1", "0", "0", "1"], name
    assert r["mode_other"] == ["0", "0"]
    assert r["limits"] == ["1", "7", "0", "0"]                  # set_knee(7) is taken as it is; set_hold(-2) is 0
    keys = json.load(open(os.path.join(ROOT, "tests", "golden", "expander_dump_keys.json")))
    assert r["dump"] == keys["keys"]
    assert r["closes"] == keys["closes"]
    s = dict(sample_rate=48000, mode=er.EM_DOWNWARD, attack_threshold=0.25, release_threshold=0.125, attack=1.0, release=10.0,
             hold=2.0, knee=0.5, ratio=4.0)
    p = mi.ExpanderBank.compute_params(**s)
    assert [f32(v) for v in r["computed"]] == [f32(p["tau_attack"]), f32(p["hold"]), f32(p["k"]["start"]), f32(p["k"]["threshold"])]
    x = np.array([[0.01, 1.0, -0.25, 0.1]], f32)
    g64, bound = er.gain64(x, [p])[0], er.gain_bound(x, [p])[0]
    amp = np.array([float(v) for v in r["amplification"]])
    cur = np.array([float(v) for v in r["curve"]])
    assert np.all(np.abs(amp - g64) <= bound * er.U * g64)
    assert np.all(np.abs(cur - g64 * np.abs(x[0])) <= (bound + 1) * er.U * g64 * np.abs(x[0]))
    assert r["amplification_array"] == r["amplification"]
    # downward, ratio 4, threshold 0.25: 1 at and above the knee's end, (0.1 / 0.25) ^ 3 = 0.064 on the line, 0 under the floor
    assert amp[1] == 1.0 and abs(amp[3] - 0.064) < 1e-4 and 0 < amp[0] < 1e-4
    q = mi.ExpanderBank.compute_params(**dict(s, ratio=20.0))
    assert er.gain64(np.array([[1e-3]], f32), [q])[0, 0] == 0.0 and q["k"]["threshold"] > 1e-3


def test_mirror_header_declares_the_reference_names():
    names = json.load(open(os.path.join(ROOT, "tests", "golden", "expander_public_names.json")))
    assert set(names) == {"dynamics/Expander.h"}
    text = open(os.path.join(PKG, "include", "lsp-plug.in", "dsp-units", "dynamics", "Expander.h")).read()
    text = re.sub(r"//.*", "", text)
    assert len(names["dynamics/Expander.h"]) >= 30
    for name in names["dynamics/Expander.h"]:
        assert re.search(r"\b%s\b" % name, text), name
    fields = ("fAttackThresh", "fReleaseThresh", "fAttack", "fRelease", "fKnee", "fRatio", "fEnvelope", "fHold", "fPeak",
              "fTauAttack", "fTauRelease", "sExp", "nHold", "nHoldCounter", "nSampleRate", "bUpdate", "bUpward")
    prot = text[text.index("protected:"):text.index("public:")]
    pos = [prot.index(" " + n + ";") for n in fields]
    assert pos == sorted(pos), "the protected fields are not in the reference's order"


def test_mirror_exports_the_reference_symbols(mi):
    out = subprocess.check_output(["nm", "-D", "--defined-only", mi.LIB_PATH]).decode()
    for sym in ("_ZN3lsp4dspu8ExpanderC1Ev", "_ZN3lsp4dspu8ExpanderD1Ev", "_ZN3lsp4dspu8Expander9constructEv",
                "_ZN3lsp4dspu8Expander7destroyEv", "_ZN3lsp4dspu8Expander15update_settingsEv",
                "_ZN3lsp4dspu8Expander7processEPfS2_PKfm", "_ZN3lsp4dspu8Expander7processEPff",
                "_ZN3lsp4dspu8Expander5curveEPfPKfm", "_ZN3lsp4dspu8Expander5curveEf",
                "_ZN3lsp4dspu8Expander13amplificationEPfPKfm", "_ZN3lsp4dspu8Expander13amplificationEf",
                "_ZN3lsp4dspu8Expander13set_thresholdEff", "_ZN3lsp4dspu8Expander11set_timingsEff",
                "_ZN3lsp4dspu8Expander15set_sample_rateEm", "_ZN3lsp4dspu8Expander8set_modeEm",
                "_ZN3lsp4dspu8Expander8set_kneeEf", "_ZN3lsp4dspu8Expander9set_ratioEf", "_ZN3lsp4dspu8Expander8set_holdEf",
                "_ZNK3lsp4dspu8Expander4dumpEPNS0_12IStateDumperE"):
        assert re.search(r" T %s$" % re.escape(sym), out, re.M), sym


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_follower_keeps_separate_multiplies_and_adds(tmp_path):
    """The bits of the restatement need tau * d and e + ... rounded on their own: no fused multiply-add in any form in the
    follower's body, under the Makefile's -ffp-contract=on."""
    isa_rounding.assert_separate_multiplies_and_adds(tmp_path, "expander.hip", "expander_follow_tile")
