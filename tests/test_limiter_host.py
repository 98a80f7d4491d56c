"""Limiter on the host (no GPU): mi_limiter_compute_params and mi_limiter_compute_patch against limiter_ref.py for all twelve
modes, the setter quirks that need no device, and the numpy restatement of process() on the reference's own unit test."""
import importlib
import itertools
import json
import os
import subprocess

import numpy as np
import pytest

import limiter_ref as lr

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "lsp-dsp-units_amd")


@pytest.fixture(scope="module")
def LB():
    return importlib.import_module("lsp-dsp-units_amd").LimiterBank


# (sample rate, look-ahead ms, attack ms, release ms): look-aheads of 0, 3, 8 and 240 .. 960 samples, attack under 8 samples,
# attack above the look-ahead, release clamped at twice the look-ahead and free of it
LADDER = [(48000, 0.0, 1.5, 1.5), (48000, 0.0625, 1.5, 1.5), (48000, 0.17, 0.1, 0.1), (48000, 5.0, 1.5, 1.5),
          (48000, 5.0, 0.1, 20.0), (48000, 5.0, 7.0, 3.0), (44100, 2.0, 1.0, 9.0), (96000, 10.0, 4.0, 30.0),
          (192000, 5.0, 2.5, 3.0), (48000, 1.0, 0.5, 1.25)]


def _check(got, s):
    ints, floats = lr.params_ref(**s)
    gi, gf = lr.flatten(got)
    assert gi == ints, (s, gi, ints)
    for name, (v, bound) in floats.items():
        if not np.isfinite(v):
            assert not np.isfinite(gf[name]) or np.isnan(v), (s, name, gf[name], v)
            continue
        assert abs(gf[name] - v) <= bound + 1e-45, (s, name, gf[name], v, bound)


@pytest.mark.parametrize("mode", range(12), ids=lr.MODES)
def test_parameters_and_tables(LB, mode):
    seen = set()
    for sr, la, att, rel in LADDER:
        s = dict(sample_rate=sr, mode=mode, threshold=0.5, lookahead=la, attack=att, release=rel, knee=0.7, alr_attack=3.0,
                 alr_release=40.0, alr_knee=0.6)
        s = dict((k, float(f32(v)) if isinstance(v, float) else v) for k, v in s.items())
        p = LB.compute_params(**s)
        _check(p, s)
        seen.add(p["lookahead"])
        if 4 <= mode < 8 and p["lookahead"] == 0:
            continue                # 2.0f / attack with attack 0: the reference's coefficients are not numbers (:351-352)
        table = LB.compute_patch(p)
        want, bound = lr.shape64(p)
        assert table.dtype == np.float32 and len(table) == p["release"]
        assert np.all(np.abs(table.astype(np.float64) - want) <= bound), (s, np.abs(table - want).max())
        assert np.all(table[p["attack"]:p["plane"]] == f32(1.0))
        assert np.isfinite(table).all()
    assert {0, 3, 8, 240}.issubset(seen), seen


def test_widths_and_limits(LB):
    """attack < 8 samples is raised to 8 (the lower limit wins in init_sat; in init_exp / init_line the upper one does);
    release is clamped at twice the look-ahead; init_sat takes release from ATTACK."""
    base = dict(sample_rate=48000, threshold=0.5, lookahead=5.0)
    p = LB.compute_params(mode=0, attack=0.1, release=20.0, **base)                 # 4 samples -> 8; release = limit(8, 8, 480)
    assert (p["attack"], p["plane"], p["middle"], p["release"]) == (8, 8, 8, 17)
    p = LB.compute_params(mode=8, attack=0.1, release=20.0, **base)                 # LINE_THIN: release 960 -> 480
    assert (p["attack"], p["plane"], p["middle"], p["release"]) == (8, 8, 8, 8 + 480 + 1)
    for mode, width in itertools.product((0, 8), range(4)):
        p = LB.compute_params(mode=mode + width, attack=2.0, release=4.0, **base)  # 96 and 192 samples
        rel = 96 if mode == 0 else 192                                              # THE QUIRK, :284
        att, plane = [(96, 96), (48, 96 + rel // 2), (48, 96), (96, 96 + rel // 2)][width]
        assert (p["attack"], p["plane"], p["middle"], p["release"]) == (att, plane, 96, 96 + rel + 1), (mode, width)
    for width in range(4):                                                          # init_exp tests for LM_HERM_*: always WIDE
        p = LB.compute_params(mode=4 + width, attack=2.0, release=4.0, **base)
        assert (p["attack"], p["plane"], p["middle"], p["release"]) == (48, 96 + 96, 96, 96 + 192 + 1)
    # a look-ahead under 8 samples.  lsp_limit(x, 8, la): x below 8 becomes 8 (beyond the look-ahead), x above la becomes la
    p = LB.compute_params(mode=1, sample_rate=48000, lookahead=0.0625, attack=1.0, release=1.0)
    assert (p["lookahead"], p["middle"], p["release"]) == (3, 3, 3 + 8 + 1)        # release = lsp_limit(3, 8, 6) = 8
    p = LB.compute_params(mode=1, sample_rate=48000, lookahead=0.0625, attack=0.1, release=1.0)
    assert (p["lookahead"], p["middle"], p["release"]) == (3, 8, 8 + 6 + 1)        # attack 4 -> 8; release = lsp_limit(8, 8, 6) = 6
    p = LB.compute_params(mode=9, sample_rate=48000, lookahead=0.0625, attack=1.0, release=1.0)
    assert (p["lookahead"], p["middle"], p["release"]) == (3, 3, 3 + 6 + 1)
    p = LB.compute_params(mode=0, sample_rate=48000, lookahead=0.0, attack=0.1, release=1.0)
    assert (p["lookahead"], p["middle"], p["release"]) == (0, 8, 8 + 0 + 1)


def test_alr_knee_is_stored_inverted():
    assert lr.stored_alr_knee(2.0) == f32(0.5) and lr.stored_alr_knee(0.25) == f32(0.25)


def test_bad_arguments(LB):
    mi = importlib.import_module("lsp-dsp-units_amd")
    with pytest.raises(mi.MiError):
        LB.compute_params(mode=12)
    p = LB.compute_params(sample_rate=48000, lookahead=5.0, attack=1.5, release=1.5)
    from ctypes import byref, c_void_p
    units = importlib.import_module("lsp-dsp-units_amd.units")
    out = np.zeros(10, np.float32)
    assert mi.lib.mi_limiter_compute_patch(byref(units._limiter_params(p)), out.ctypes.data_as(c_void_p), out.size) < 0


def triangle():
    """src/test/utest/dynamics/limiter.cpp:43-52."""
    x = np.zeros(4096, f32)
    s, step, i = f32(0.0), f32(0.05), 0
    while s < f32(0.999):
        x[i] = s
        i += 1
        s = f32(s + step)
    while s > f32(0.001):
        x[i] = s
        i += 1
        s = f32(s - step)
    return x


TRIANGLE = dict(sample_rate=48000, mode=0, knee=1.0, threshold=0.5, attack=1.5, release=1.5, lookahead=5.0)


def check_triangle(x, gain, out, latency):
    """The assertions of the reference's test_triangle_peak (:71-107)."""
    assert latency == int(f32(5.0) * f32(48000) * f32(0.001)) == 240
    assert out.max() < 0.6 and out.min() >= 0.0
    assert gain.max() >= 1.0 and gain.min() >= 0.0
    assert gain[0] == 1.0 and gain[4095] == 1.0
    assert int(np.argmax(out)) - int(np.argmax(x)) == latency


def test_restatement_meets_the_reference_unit_test(LB):
    """What ties the restatement to the reference: its own test (src/test/utest/dynamics/limiter.cpp:37-110) at its own sizes,
    init(192000, 20) -> ML = 3840."""
    p = LB.compute_params(**TRIANGLE)
    table = LB.compute_patch(p)
    ml = int(lr.millis_to_samples(192000, 20.0))
    assert ml == 3840
    lim = lr.Limiter(ml)
    lim.refill()
    x = triangle()
    gain = lim.process(x, p, table)
    out = lr.delayed(x, 0, 4096, p["lookahead"]) * gain
    check_triangle(x, gain, out, p["lookahead"])
    assert lim.patches == 1 and lim.overrun == 0 and lim.outside == 0
    assert lim.head == 4096                                                        # under 8 ML: no move


def test_restatement_stays_inside_the_reference_allocation_from_ml_8(LB):
    """The reference multiplies floats outside its allocation only with ML < 8; the guard floats are for that case alone."""
    rng = np.random.default_rng(5)
    for ml_ms, la_ms, expect_outside in ((8 / 48.0, 0.0, False), (8 / 48.0, 8 / 48.0, False), (3 / 48.0, 3 / 48.0, True)):
        ml = int(lr.millis_to_samples(48000, f32(ml_ms) + f32(1e-4)))
        p = LB.compute_params(sample_rate=48000, mode=0, threshold=0.25, lookahead=float(f32(la_ms) + f32(1e-4)), attack=0.1, release=0.1)
        table = LB.compute_patch(p)
        lim = lr.Limiter(ml)
        for _ in range(40):
            lim.process(rng.standard_normal(1 + ml).astype(f32), p, table)
        assert lim.patches_per_chunk and (lim.outside > 0) == expect_outside, (ml, lim.outside)


PROBE = r"""
#include <lsp-plug.in/dsp-units/dynamics/Limiter.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace lsp::dspu;

struct names: public IStateDumper
{
    std::vector<std::string> seen, closes;
    void begin_object(const char *n, const void *, size_t) override    { seen.push_back(n); }
    void end_object() override                                         { closes.push_back("end_object"); }
    void write(const char *n, const void *) override                   { seen.push_back(n); }
    void write(const char *n, bool) override                           { seen.push_back(n); }
    void write(const char *n, signed int) override                     { seen.push_back(n); }
    void write(const char *n, unsigned long) override                  { seen.push_back(n); }
    void write(const char *n, float) override                          { seen.push_back(n); }
    void writev(const char *n, const float *, size_t) override         { seen.push_back(n); }
};

struct probe: public Limiter
{
    static size_t alr_size()    { return sizeof(alr_t); }
    static size_t sat_size()    { return sizeof(sat_t); }
    static size_t line_size()   { return sizeof(line_t); }
    float threshold() const     { return fThreshold; }
    void set_max(float ms)      { fMaxLookahead = ms; }
    void show(const char *label) const
    {
        printf("%s %zu %d %d %d %d", label, nLookahead, sSat.nAttack, sSat.nPlane, sSat.nRelease, sSat.nMiddle);
        for (int i = 0; i < 4; ++i) printf(" %.9g", sSat.vAttack[i]);
        for (int i = 0; i < 4; ++i) printf(" %.9g", sSat.vRelease[i]);
        printf(" %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g\n", fThreshold, sALR.fKS, sALR.fKE, sALR.fGain, sALR.vHermite[0],
               sALR.vHermite[1], sALR.vHermite[2], sALR.fTauAttack, sALR.fTauRelease);
    }
};

int main()
{
    printf("sizeof %zu %zu %zu %zu\n", sizeof(Limiter), probe::alr_size(), probe::sat_size(), probe::line_size());
    void *raw = malloc(sizeof(Limiter));
    memset(raw, 0xa5, sizeof(Limiter));
    probe *m = reinterpret_cast<probe *>(raw);
    m->construct();
    printf("fresh %d %d %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g %d %zu %zu\n", int(m->modified()), int(m->get_mode()), m->get_threshold(),
           m->threshold(), m->get_lookahead(), m->get_attack(), m->get_release(), m->get_knee(), m->get_alr_attack(), m->get_alr_release(),
           int(m->get_alr()), m->get_latency(), m->max_latency());
    printf("alr_knee %.9g", m->alr_knee());
    m->update_settings();
    m->set_alr_knee(2.0f);  printf(" %.9g %d", m->alr_knee(), int(m->modified()));
    m->update_settings();
    m->set_alr_knee(0.5f);  printf(" %.9g %d", m->alr_knee(), int(m->modified()));     // 0.5 is what is stored: no change
    m->set_alr_knee(0.25f); printf(" %.9g %d\n", m->alr_knee(), int(m->modified()));
    m->update_settings();
    m->set_sample_rate(48000);
    m->set_max(5.0f);
    m->set_lookahead(7.0f); printf("lookahead %.9g %zu", m->get_lookahead(), m->get_latency());
    m->set_lookahead(2.0f); printf(" %.9g %zu\n", m->get_lookahead(), m->get_latency());
    m->update_settings();
    m->set_threshold(0.5f, false); printf("threshold %.9g %.9g %d", m->get_threshold(), m->threshold(), int(m->modified()));
    m->update_settings();          printf(" %.9g %d", m->threshold(), int(m->modified()));
    m->set_threshold(0.25f, true); printf(" %.9g %.9g %d", m->get_threshold(), m->threshold(), int(m->modified()));
    m->update_settings();
    m->set_threshold(0.25f, true); printf(" %d\n", int(m->modified()));
    m->set_alr(true);
    m->set_alr(false);             printf("alr %d %d\n", int(m->get_alr()), int(m->modified()));

    m->set_threshold(0.5f, true); m->set_knee(0.7f); m->set_attack(1.5f); m->set_release(3.0f); m->set_lookahead(5.0f);
    m->set_alr_attack(3.0f); m->set_alr_release(40.0f); m->set_alr_knee(0.6f);
    const limiter_mode_t modes[3] = { LM_HERM_DUCK, LM_EXP_TAIL, LM_LINE_WIDE };
    for (int k = 0; k < 3; ++k)
    {
        m->set_mode(modes[k]);
        m->update_settings();
        char label[16];
        snprintf(label, sizeof(label), "computed%d", int(modes[k]));
        m->show(label);
        names n;
        m->dump(&n);
        printf("dump%d", int(modes[k]));
        for (const std::string &s: n.seen)
            printf(" %s", s.c_str());
        printf("\ncloses%d", int(modes[k]));
        for (const std::string &s: n.closes)
            printf(" %s", s.c_str());
        printf("\n");
    }
    m->destroy();
    free(raw);
    return 0;
}
"""


def test_mirror_header_layout_setter_quirks_and_dump_order(LB, tmp_path):
    src, exe = os.path.join(str(tmp_path), "limiter_probe.cpp"), os.path.join(str(tmp_path), "limiter_probe")
    with open(src, "w") as f:
        f.write(PROBE)
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-I" + os.path.join(PKG, "include"), "-I" + os.path.join(ROOT, "include"),
                           src, "-o", exe, "-L" + PKG, "-lmi_dspu", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.check_output([exe]).decode().splitlines()
    r = {l.split()[0]: l.split()[1:] for l in out}
    # seven floats, seven size_t, alr_t (twelve floats and a bool), three pointers, the union of 48 bytes
    assert r["sizeof"] == ["216", "52", "48", "32"]
    assert r["fresh"] == ["1", "0", "1", "1", "0", "0", "0", "%.9g" % f32(0.50118), "10", "50", "0", "0", "0"]
    assert r["alr_knee"] == ["%.9g" % f32(0.56234), "0.5", "1", "0.5", "0", "0.25", "1"]
    assert r["lookahead"] == ["5", "240", "2", "96"]                                # above the maximum: clamped
    # without `immediate` fThreshold waits for update_settings(); with it, it is set at once; an unchanged value marks nothing
    assert r["threshold"] == ["0.5", "1", "1", "0.5", "0", "0.25", "0.25", "1", "0"]
    assert r["alr"] == ["0", "0"]
    keys = json.load(open(os.path.join(ROOT, "tests", "golden", "limiter_dump_keys.json")))
    for mode in (3, 6, 9):
        want = [keys["shape"]["LM_" + lr.MODES[mode]] if k == "<shape>" else k for k in keys["keys"]]
        assert r["dump%d" % mode] == want, mode
        assert r["closes%d" % mode] == keys["closes"]
        p = LB.compute_params(sample_rate=48000, mode=mode, threshold=0.5, lookahead=5.0, attack=1.5, release=3.0,
                              knee=float(f32(0.7)), alr_attack=3.0, alr_release=40.0, alr_knee=float(f32(0.6)))
        got = r["computed%d" % mode]
        assert [int(v) for v in got[:5]] == [p[k] for k in ("lookahead", "attack", "plane", "release", "middle")]
        shape = list(p["v_attack"]) + list(p["v_release"])
        if mode >= 8:                           # line_t: two coefficients each, side by side where sat_t has vAttack
            shape = list(p["v_attack"][:2]) + list(p["v_release"][:2]) + [f32(0)] * 4
        floats = shape + [p[k] for k in ("threshold", "ks", "ke", "gain")] + list(p["hermite"]) + \
            [p["tau_attack"], p["tau_release"]]
        assert got[5:] == ["%.9g" % v for v in floats], mode
