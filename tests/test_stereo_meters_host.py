"""Correlometer and Panometer without a device: the float32 restatement against the reference's recorded outputs bit for bit and
against float64 window sums inside a stated bound, known answers, the refresh's split on a hand-computed ring, the mirror headers
(size, names, dump order, setters' rules), refusals and the rounding of both chain functions."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import isa_rounding
import stereo_meters_ref as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "lsp-dsp-units_amd")
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_stereo_meter_vectors as gen  # noqa: E402

f32 = np.float32
MAX_PERIOD = 480
CAP = sm.capacity(MAX_PERIOD)


def _corr(periods, max_period=MAX_PERIOD):
    return sm.Correlometers([dict(period=p, capacity=sm.capacity(max_period)) for p in periods])


def _pan(periods, law=sm.PAN_LAW_EQUAL_POWER, dflt=0.5, max_period=MAX_PERIOD):
    return sm.Panometers([dict(period=p, capacity=sm.capacity(max_period), law=law, norm=f32(1.0) / f32(p), default_pan=dflt)
                          for p in periods])


def test_capacity_is_the_references():
    assert CAP == 1536 and sm.capacity(257) == 1344 and sm.capacity(2400) == 3456 and sm.capacity(1) == 1088


def _replay(case, a, b):
    """A recorded case through the restatement: (out, the five state words)."""
    mp = case["max_period"]
    if case["kind"] == gen.CORRELOMETER:
        m = sm.Correlometers([dict(period=0, capacity=sm.capacity(mp))])
    else:
        m = sm.Panometers([dict(period=0, capacity=sm.capacity(mp), law=sm.PAN_LAW_EQUAL_POWER, norm=f32(0.0), default_pan=0.5)])
    out, at = [], 0
    for what, arg in case["ops"]:
        what, arg = int(what), int(arg)
        if what == gen.OP_SET_PERIOD:
            m.set_period(0, arg, mp)
        elif what == gen.OP_CLEAR:
            m.clear(0)
        elif what == gen.OP_PROCESS:
            out.append(m.process(a[None, at:at + arg], b[None, at:at + arg])[0][0])
            at += arg
        elif what == gen.OP_SET_LAW:
            m.law[0] = arg
        elif what == gen.OP_SET_DEFAULT:
            m.dflt[0] = np.uint32(arg).view(f32)
    s = m.state()
    keys = ("v", "a", "b") if case["kind"] == gen.CORRELOMETER else ("value_a", "value_b")
    words = [int(s[k].view(np.uint32)[0]) for k in keys] + [0] * (3 - len(keys)) + [int(s["head"][0]), int(s["window"][0])]
    return np.concatenate(out), words, m


def test_restatement_equals_the_references_recorded_outputs():
    """tests/golden/stereo_meter_ref_vectors.npz: the reference's two .cpp files compiled unmodified on 24 cases."""
    a, b, cases = gen.load()
    assert len(cases) == 24 and {c["kind"] for c in cases} == {gen.CORRELOMETER, gen.PANOMETER}
    periods = set()
    for c in cases:
        out, words, m = _replay(c, a, b)
        bad = np.flatnonzero(out.view(np.uint32) != c["out"].view(np.uint32))
        assert bad.size == 0, (c["name"], len(bad), bad[:4].tolist())
        assert words == [int(v) for v in c["state"]], c["name"]
        assert {w for _, w in m.refreshes} == {False, True}, c["name"]
        periods |= {int(arg) for what, arg in c["ops"] if what == gen.OP_SET_PERIOD}
        rest = c["out"][gen.SILENCE[1] - 50:gen.SILENCE[1]]             # the zero branch and the default branch, taken and not
        assert len(set(rest.tolist())) == 1 and np.any(c["out"][:gen.SILENCE[0]] != rest[0]), c["name"]
    assert periods >= {1, 7, 255, 256, 257, 480, 100}


@pytest.fixture(scope="module")
def window_run():
    """The generator's signal without its silences (a correlated pair whose level steps between 1 and 1e-3) through both
    restatements at periods 1, 40 and 480, computed once."""
    n = 3000
    rng = np.random.default_rng(2024)
    level = np.where((np.arange(n) // 700) % 2 == 0, 1.0, 1e-3)
    a = (rng.standard_normal(n) * level).astype(f32)
    b = (0.6 * a + 0.8 * rng.standard_normal(n) * level).astype(f32)
    periods = (1, 40, 480)
    A, B = np.tile(a, (3, 1)), np.tile(b, (3, 1))
    corr = _corr(periods)
    pan = _pan(periods)
    return a, b, periods, corr.process(A, B), pan.process(A, B)


def _window_sums(term, n, N):
    cs = np.concatenate([[0.0], np.cumsum(term)])
    t = np.arange(n)
    return cs[t + 1] - cs[np.maximum(t + 1 - N, 0)]


def test_restatement_against_float64_window_sums(window_run):
    """|trace - exact window sum| <= 1.01 (N + r k) 2^-24 S_max, k the samples since the last refresh (one at the first sample,
    then every N) and S_max the running maximum of the exact window sum of the terms' MAGNITUDES (for v: of |a b|).  The refresh
    is N terms added serially: at most N roundings of sums no larger than S_max, the products' own roundings among them (a sum of
    one term is exact).  Every sample after it adds r roundings of values no larger than S_max: r = 4 for the Correlometer
    (product, product, difference, sum), r = 2 for the Panometer ((v + head) - tail over the stored squares, which are the terms
    as they are, so no product rounds)."""
    a, b, periods, (c_out, c_trace), (p_out, p_trace) = window_run
    n = a.size
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    sq_a, sq_b = (a * a).astype(np.float64), (b * b).astype(np.float64)         # what the Panometer's rings hold
    t = np.arange(n)
    for ch, N in enumerate(periods):
        k = t % N + 1
        cases = [("v", c_trace[0, ch], a64 * b64, np.abs(a64 * b64), 4), ("a", c_trace[1, ch], a64 * a64, a64 * a64, 4),
                 ("b", c_trace[2, ch], b64 * b64, b64 * b64, 4), ("va", p_trace[0, ch], sq_a, sq_a, 2), ("vb", p_trace[1, ch], sq_b, sq_b, 2)]
        for name, trace, term, mag, r in cases:
            exact = _window_sums(term, n, N)
            smax = np.maximum.accumulate(_window_sums(mag, n, N))
            bound = 1.01 * (N + r * k) * sm.U * smax
            err = np.abs(trace.astype(np.float64) - exact)
            ratio = (err / np.maximum(bound, 1e-300)).max()
            print("%s N %d: at most %.3f of the bound" % (name, N, ratio))
            assert np.all(err <= bound), (name, N, ratio)
    # the correlation is not clamped (no more than in the reference): what cancellation leaves in v, a and b after a loud stretch
    # takes it past 1 here; the pan is a quotient of non-negative numbers
    print("largest |correlation| %.6f" % np.abs(c_out).max())
    assert np.all((p_out >= 0.0) & (p_out <= 1.0))


def test_known_answers():
    n, periods = 700, (1, 7, 100, 257)
    rng = np.random.default_rng(7)
    a = np.tile((rng.standard_normal(n) * 0.5).astype(f32), (4, 1))
    silence = np.zeros((4, n), f32)
    # b = a: v, a, b are the same sums, so v == sqrt(a * b) to a rounding or two and the correlation is 1 to as much
    out, trace = _corr(periods).process(a, a)
    assert np.array_equal(trace[0], trace[1]) and np.array_equal(trace[1], trace[2])
    root = np.sqrt(trace[1] * trace[2])
    live = trace[1] * trace[2] >= sm.CORR_THRESHOLD
    assert np.all(np.abs(trace[0] - root)[live] <= 2 * 2 * sm.U * root[live])          # the product and the root, one unit each
    assert live.sum() > 2000 and np.all(np.abs(out[live] - 1.0) <= 4 * sm.U * 2)
    out, _ = _corr(periods).process(a, -a)
    assert np.all(np.abs(out[live] + 1.0) <= 4 * sm.U * 2)
    out, trace = _corr(periods).process(silence, silence)
    assert np.all(out == 0.0) and not np.any(np.signbit(out)) and np.all(trace == 0.0)
    for law in (sm.PAN_LAW_LINEAR, sm.PAN_LAW_EQUAL_POWER):
        left, _ = _pan(periods, law).process(a, silence)                                # hard left: nothing in b
        right, _ = _pan(periods, law).process(silence, a)
        both, _ = _pan(periods, law).process(a, a)
        none, _ = _pan(periods, law, dflt=0.125).process(silence, silence)
        sounding = np.abs(a) > 1e-2
        assert np.all(left[sounding] == 0.0) and np.all(right[sounding] == 1.0) and np.all(both[sounding] == 0.5)
        assert np.all(none == f32(0.125))


def test_refresh_split_on_a_hand_computed_ring():
    """Rings of 1536.  Refreshes fall on multiples of the period; nHead there is the sample index modulo 1536.  Period 257 wraps
    first at sample 1542 (nHead 6: the ring's last 251 samples, then its first 6), period 480 at 1920 (nHead 384: 96, then 384),
    period 256 at 1536 (nHead 0: the last 256, then nothing)."""
    n = 1925
    rng = np.random.default_rng(5)
    a = np.tile((rng.standard_normal(n) * 0.5).astype(f32), (3, 1))
    b = np.tile((rng.standard_normal(n) * 0.5).astype(f32), (3, 1))
    periods = (257, 480, 256)
    corr, pan = _corr(periods), _pan(periods)
    _, ct = corr.process(a, b)
    _, pt = pan.process(a, b)
    for ref in (corr, pan):
        for ch, (p, first) in enumerate(zip(periods, (1542, 1920, 1536))):
            wrapped = [w for c, w in ref.refreshes if c == ch]
            # (the very first refresh finds nHead 0 and an empty ring: wrapped as well, over zeros)
            assert len(wrapped) == -(-n // p) and wrapped[0] and wrapped[1:].index(True) + 1 == first // p and first % p == 0, (p, wrapped)
    for ch, (p, at, head) in enumerate(zip(periods, (1542, 1920, 1536), (6, 384, 0))):
        assert at % CAP == head
        x, y = a[ch, at - p:at], b[ch, at - p:at]
        cut = p - head
        two = lambda t: sm.serial_sum(t[:cut]) + sm.serial_sum(t[cut:])
        ah, bh, at_, bt = a[ch, at], b[ch, at], a[ch, at - p], b[ch, at - p]
        assert ct[0, ch, at] == two(x * y) + (ah * bh - at_ * bt)
        assert ct[1, ch, at] == two(x * x) + (ah * ah - at_ * at_)
        assert pt[0, ch, at] == (two(x * x) + ah * ah) - at_ * at_
        assert pt[1, ch, at] == (two(y * y) + bh * bh) - bt * bt
    # ... and the one serial sum is another number somewhere: the split is not a matter of taste
    x = a[1, 1920 - 480:1920]
    assert any(sm.serial_sum((v * v)[:cut]) + sm.serial_sum((v * v)[cut:]) != sm.serial_sum(v * v)
               for v, cut in ((x, 96), (a[0, 1542 - 257:1542], 251)))


PROBE = r'''
#include <lsp-plug.in/dsp-units/meters/Correlometer.h>
#include <lsp-plug.in/dsp-units/meters/Panometer.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using lsp::dspu::Correlometer;
using lsp::dspu::Panometer;

struct names: public lsp::dspu::IStateDumper                       // the keys in order, and the values by key
{
    std::vector<std::string> seen, closes;
    std::string values;
    void note(const char *n, double v)                                 { char b[96]; snprintf(b, sizeof(b), " %s=%g", n, v); values += b; seen.push_back(n); }
    void begin_object(const char *n, const void *, size_t) override    { seen.push_back(n); }
    void end_object() override                                         { closes.push_back("end_object"); }
    void end_array() override                                          { closes.push_back("end_array"); }
    void write(const char *n, const void *p) override                  { note(n, p == NULL ? 0.0 : 1.0); }
    void write(const char *n, unsigned int v) override                 { note(n, v); }
    void write(const char *n, int v) override                          { note(n, v); }
    void write(const char *n, float v) override                        { note(n, v); }
};

template <class M> static void show(const char *label, const M &m)
{
    names n;
    m.dump(&n);
    printf("%s%s\n", label, n.values.c_str());
}

int main()
{
    // the public surface, by address
    void (Correlometer::*c1)(float *, const float *, const float *, size_t) = &Correlometer::process;
    lsp::status_t (Correlometer::*c2)(size_t) = &Correlometer::init;
    void (Correlometer::*c3)(size_t) = &Correlometer::set_period;
    size_t (Correlometer::*c4)() const = &Correlometer::period;
    bool (Correlometer::*c5)() const = &Correlometer::needs_update;
    void (Correlometer::*c6)(lsp::dspu::IStateDumper *) const = &Correlometer::dump;
    void (Panometer::*p1)(float *, const float *, const float *, size_t) = &Panometer::process;
    void (Panometer::*p2)(lsp::dspu::pan_law_t) = &Panometer::set_pan_law;
    lsp::dspu::pan_law_t (Panometer::*p3)() const = &Panometer::pan_law;
    void (Panometer::*p4)(float) = &Panometer::set_default_pan;
    float (Panometer::*p5)() const = &Panometer::default_pan;
    (void)c1; (void)c2; (void)c3; (void)c4; (void)c5; (void)c6; (void)p1; (void)p2; (void)p3; (void)p4; (void)p5;

    printf("sizeof %zu %zu %zu\n", sizeof(Correlometer), sizeof(Panometer), sizeof(lsp::dsp::correlation_t));
    printf("enums %d %d\n", int(lsp::dspu::PAN_LAW_LINEAR), int(lsp::dspu::PAN_LAW_EQUAL_POWER));

    // construct() on raw memory and the setters' rules, no device involved
    void *raw = malloc(sizeof(Correlometer));
    memset(raw, 0xa5, sizeof(Correlometer));
    Correlometer *c = reinterpret_cast<Correlometer *>(raw);
    c->construct();
    show("c_fresh", *c);
    printf("c_init %d\n", int(c->init(480)));
    show("c_inited", *c);
    c->set_period(257);
    printf("c_needs %d", int(c->needs_update()));
    c->update_settings();
    printf(" %d", int(c->needs_update()));
    c->set_period(257);                                             // unchanged: ignored
    printf(" %d", int(c->needs_update()));
    show("\nc_settled", *c);
    c->set_period(9999);                                            // clamped to the maximum
    printf("c_clamped %zu %d\n", c->period(), int(c->needs_update()));
    c->clear();                                                     // nHead = nPeriod; nWindow and the flag stay
    show("c_cleared", *c);
    float out[4] = { 7.0f, 7.0f, 7.0f, 7.0f }, in[4] = { 1.0f, 1.0f, 1.0f, 1.0f };
    Correlometer z;
    z.init(480);
    z.process(out, in, in, 4);                                      // a period of 0: returns, dst untouched
    printf("c_zero %g %g\n", out[0], out[3]);
    names n;
    c->dump(&n);
    printf("c_dump");
    for (const std::string &s: n.seen)
        printf(" %s", s.c_str());
    printf("\nc_closes");
    for (const std::string &s: n.closes)
        printf(" %s", s.c_str());
    printf("\n");
    c->destroy();
    free(raw);

    raw = malloc(sizeof(Panometer));
    memset(raw, 0xa5, sizeof(Panometer));
    Panometer *p = reinterpret_cast<Panometer *>(raw);
    p->construct();
    show("p_fresh", *p);
    printf("p_init %d\n", int(p->init(480)));
    p->set_period(100);                                             // at once: nWindow, fNorm
    show("p_period", *p);
    p->set_period(9999);
    p->set_pan_law(lsp::dspu::PAN_LAW_LINEAR);
    p->set_default_pan(0.25f);
    printf("p_set %zu %d %g\n", p->period(), int(p->pan_law()), p->default_pan());
    p->clear();
    show("p_cleared", *p);
    Panometer pz;
    pz.init(480);
    pz.process(out, in, in, 4);
    printf("p_zero %g %g\n", out[0], out[3]);
    names pn;
    p->dump(&pn);
    printf("p_dump");
    for (const std::string &s: pn.seen)
        printf(" %s", s.c_str());
    printf("\np_closes");
    for (const std::string &s: pn.closes)
        printf(" %s", s.c_str());
    printf("\n");
    p->destroy();
    free(raw);
    return 0;
}
'''


@pytest.fixture(scope="module")
def probe(mi, tmp_path_factory):
    d = tmp_path_factory.mktemp("stereo_meter_probe")
    src, exe = str(d / "sm_probe.cpp"), str(d / "sm_probe")
    with open(src, "w") as f:
        f.write(PROBE)
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-I" + os.path.join(PKG, "include"), "-I" + os.path.join(ROOT, "include"),
                           src, "-o", exe, "-L" + PKG, "-lmi_dspu", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.check_output([exe]).decode().splitlines()
    return {l.split()[0]: l.split()[1:] for l in out if l.strip()}


def _fields(words):
    return {w.split("=")[0]: float(w.split("=")[1]) for w in words}


def test_mirror_sizes_are_the_references(probe):
    # a correlation_t (12, padded to 16), two pointers, six uint32_t, a pointer; two pointers, an enum, four floats, five uint32_t,
    # a pointer
    assert probe["sizeof"] == ["64", "64", "12"]
    assert probe["enums"] == ["0", "1"]


def test_mirror_setters_follow_the_references_rules(probe):
    f = _fields(probe["c_fresh"])
    assert f["nFlags"] == 1 and all(f[k] == 0 for k in f if k != "nFlags")                 # CF_UPDATE; no rings on the host
    assert probe["c_init"] == ["0"]
    f = _fields(probe["c_inited"])
    assert (f["nCapacity"], f["nMaxPeriod"], f["nPeriod"], f["nHead"], f["nFlags"]) == (1536, 480, 0, 0, 0)
    assert probe["c_needs"] == ["1", "0", "0"]                                              # set, settled, unchanged: ignored
    f = _fields(probe["c_settled"])
    assert (f["nPeriod"], f["nWindow"], f["nFlags"]) == (257, 257, 0)
    assert probe["c_clamped"] == ["480", "1"]
    f = _fields(probe["c_cleared"])
    assert (f["nHead"], f["nPeriod"], f["nWindow"], f["nFlags"]) == (480, 480, 257, 1)
    assert probe["c_zero"] == ["7", "7"] and probe["p_zero"] == ["7", "7"]
    f = _fields(probe["p_fresh"])
    assert f["enPanLaw"] == 1 and f["fDefault"] == 0.5 and all(f[k] == 0 for k in f if k not in ("enPanLaw", "fDefault"))
    assert probe["p_init"] == ["0"]
    f = _fields(probe["p_period"])
    assert (f["nPeriod"], f["nWindow"], f["nCapacity"], f["nMaxPeriod"]) == (100, 100, 1536, 480)
    assert f["fNorm"] == 0.01
    assert probe["p_set"] == ["480", "0", "0.25"]
    f = _fields(probe["p_cleared"])
    assert (f["nHead"], f["nPeriod"], f["nWindow"], f["enPanLaw"], f["fDefault"]) == (480, 480, 480, 0, 0.25)


def test_dump_writes_the_references_keys_in_order(probe):
    for cls in ("correlometer", "panometer"):
        keys = json.load(open(os.path.join(ROOT, "tests", "golden", cls + "_dump_keys.json")))
        assert probe[cls[0] + "_dump"] == keys["keys"], cls
        assert probe.get(cls[0] + "_closes", []) == keys["closes"], cls


def test_mirrors_declare_the_references_public_names():
    names = json.load(open(os.path.join(ROOT, "tests", "golden", "stereo_meter_public_names.json")))
    assert set(names) == {"meters/Correlometer.h", "meters/Panometer.h"}
    for header, listed in names.items():
        text = re.sub(r"//.*", "", open(os.path.join(PKG, "include", "lsp-plug.in", "dsp-units", header)).read())
        assert len(listed) >= 10
        for name in listed:
            assert re.search(r"\b%s\b" % name, text), (header, name)
    order = {"meters/Correlometer.h": ("sCorr", "vInA", "vInB", "nCapacity", "nHead", "nMaxPeriod", "nPeriod", "nWindow", "nFlags", "pData"),
             "meters/Panometer.h": ("vInA", "vInB", "enPanLaw", "fValueA", "fValueB", "fNorm", "fDefault", "nCapacity", "nHead", "nMaxPeriod",
                                    "nPeriod", "nWindow", "pData")}
    for header, fields in order.items():
        text = re.sub(r"//.*", "", open(os.path.join(PKG, "include", "lsp-plug.in", "dsp-units", header)).read())
        pos = [re.search(r"\b%s;" % n, text).start() for n in fields]
        assert pos == sorted(pos), "%s: the private fields are not in the reference's order" % header
    dsp = open(os.path.join(PKG, "include", "lsp-plug.in", "dsp", "dsp.h")).read()
    assert re.search(r"struct correlation_t\s*\{\s*float v;\s*float a;\s*float b;", dsp)


def test_mirrors_export_the_references_symbols(mi):
    out = subprocess.check_output(["nm", "-D", "--defined-only", mi.LIB_PATH]).decode()
    for sym in ("_ZN3lsp4dspu12CorrelometerC1Ev", "_ZN3lsp4dspu12CorrelometerD1Ev", "_ZN3lsp4dspu12Correlometer9constructEv",
                "_ZN3lsp4dspu12Correlometer7destroyEv", "_ZN3lsp4dspu12Correlometer4initEm", "_ZN3lsp4dspu12Correlometer10set_periodEm",
                "_ZN3lsp4dspu12Correlometer15update_settingsEv", "_ZN3lsp4dspu12Correlometer5clearEv",
                "_ZN3lsp4dspu12Correlometer7processEPfPKfS4_m", "_ZNK3lsp4dspu12Correlometer4dumpEPNS0_12IStateDumperE",
                "_ZN3lsp4dspu9PanometerC1Ev", "_ZN3lsp4dspu9PanometerD1Ev", "_ZN3lsp4dspu9Panometer9constructEv",
                "_ZN3lsp4dspu9Panometer7destroyEv", "_ZN3lsp4dspu9Panometer4initEm", "_ZN3lsp4dspu9Panometer11set_pan_lawENS0_9pan_law_tE",
                "_ZN3lsp4dspu9Panometer15set_default_panEf", "_ZN3lsp4dspu9Panometer10set_periodEm", "_ZN3lsp4dspu9Panometer5clearEv",
                "_ZN3lsp4dspu9Panometer7processEPfPKfS4_m", "_ZNK3lsp4dspu9Panometer4dumpEPNS0_12IStateDumperE"):
        assert re.search(r" T %s$" % re.escape(sym), out, re.M), sym


def test_refusals(mi):
    """NULL handles are refused, never followed; a period of 0 is MI_EINVAL wherever it can be told without a bank."""
    lib = mi.lib
    for kind in ("correlometer", "panometer"):
        fn = lambda what: getattr(lib, "mi_%s_bank_%s" % (kind, what))
        assert fn("set_period")(None, 0, 10) == -5 and fn("clear")(None, 0) == -5 and fn("update_settings")(None, None) == -5
        assert fn("process")(None, None, None, None, 4, 4, 4, 4, None) == -5
        assert fn("get_params")(None, 0, None) == -5 and fn("get_state")(None, 0, None, None) == -5
        assert fn("set_state")(None, 0, None, 0, None) == -5
        assert fn("destroy")(None) == 0
        assert fn("create")(None, 1, 480) == -1 and lib.mi_dspu_last_error()
        h = __import__("ctypes").c_void_p()
        assert fn("create")(__import__("ctypes").byref(h), 0, 480) == -1 and not h.value           # no channels
        assert fn("create")(__import__("ctypes").byref(h), 1, 0) == -1 and not h.value             # no period could ever be set
    assert lib.mi_panometer_bank_set_pan_law(None, 0, 0) == -5 and lib.mi_panometer_bank_set_default_pan(None, 0, 0.5) == -5
    if mi.device_count() > 0:
        bank = mi.CorrelometerBank(1, 480)
        assert lib.mi_correlometer_bank_set_period(bank.handle, 0, 0) == -1 and b"period of 0" in lib.mi_dspu_last_error()
        bank.close()


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
@pytest.mark.parametrize("source,function", [("correlometer.hip", "correlometer_chain_tile"), ("panometer.hip", "panometer_chain_tile")])
def test_chains_keep_separate_multiplies_and_adds(tmp_path, source, function):
    """The bits of the restatement need every sum of the chains rounded on its own: no fused multiply-add in any form in the
    chain's body, under the Makefile's -ffp-contract=on."""
    isa_rounding.assert_separate_multiplies_and_adds(tmp_path, source, function)
