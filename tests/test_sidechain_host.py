"""Sidechain without a device: update_settings() (mi_sidechain_compute_params) against exact and float64 values, the float32
restatement of the window detectors against float64 window sums inside a stated bound, the mirror headers (layout, names,
dump order, setters' flags) and RawRingBuffer on known answers."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import isa_rounding
import sidechain_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "lsp-dsp-units_amd")
f32 = np.float32

RATES = (8000, 11025, 44100, 48000, 88200, 96000, 192000)
MAX_MS = 50.0


@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("react", [0.0, 13.7, MAX_MS])
def test_compute_params_exact_counts_and_tau_against_float64(mi, rate, react):
    p = mi.SidechainBank.compute_params(rate, MAX_MS, react)
    n = sr.reactivity_samples(rate, react)
    assert p["reactivity"] == n and p["capacity"] == sr.capacity(rate, MAX_MS)     # exact
    assert p["capacity"] >= p["reactivity"] + sr.RING_EXTRA
    assert p["interval"] == f32(1.0) / f32(n)
    tau, bound = sr.tau64(n)
    assert abs(float(p["tau"]) - tau) <= bound, (rate, react, p["tau"], tau, abs(float(p["tau"]) - tau) / bound)
    assert (p["mode"], p["source"], p["flags"], p["gain"]) == (0, 0, 0, 1.0)


def test_compute_params_known_values_and_refusals(mi):
    assert mi.SidechainBank.compute_params(48000, 50.0, 50.0)["reactivity"] == 2400
    assert mi.SidechainBank.compute_params(48000, 50.0, 50.0)["capacity"] == 2912
    assert mi.SidechainBank.compute_params(8000, 5.0, 5.0)["reactivity"] == 40
    assert mi.SidechainBank.compute_params(8000, 5.0, 5.0)["capacity"] == 552
    p = mi.SidechainBank.compute_params(0, 0.0, 0.0)                # as constructed: one sample, tau = sqrt(1/2)
    assert (p["reactivity"], p["capacity"]) == (1, 513) and abs(float(p["tau"]) - np.sqrt(0.5)) < 1e-6
    for bad in (-1.0, 50.5):
        with pytest.raises(mi.MiError) as e:
            mi.SidechainBank.compute_params(48000, 50.0, bad)
        assert e.value.code == -1
    assert mi.lib.mi_sidechain_compute_params(48000, 50.0, 1.0, None) == -1
    # null handles are refused, never followed
    assert mi.lib.mi_sidechain_bank_set_mode(None, 0, 1) < 0 and mi.lib.mi_sidechain_bank_clear(None, 0) < 0
    assert mi.lib.mi_sidechain_bank_process(None, None, None, None, 4, 4, 4, 4, None) < 0
    assert mi.lib.mi_sidechain_bank_update_settings(None, None) < 0 and mi.lib.mi_sidechain_bank_destroy(None) == 0


def _window_params(mi, mode):
    out = []
    for rate, mx, ms in ((8000, 0.0, 0.0), (8000, 5.0, 5.0), (48000, 50.0, 50.0)):
        p = mi.SidechainBank.compute_params(rate, mx, ms)
        p.update(mode=mode)
        out.append(p)
    return out


@pytest.fixture(scope="module")
def window_run(mi):
    """Gaussian magnitudes alternating between level 1 and 1e-3 every 3000 samples through the restatement, RMS and UNIFORM,
    computed once."""
    n = 3 * sr.REFRESH_RATE + 17
    level = np.where((np.arange(n) // 3000) % 2 == 0, 1.0, 1e-3)
    x = (np.random.default_rng(2024).standard_normal((1, n)) * level).astype(f32)
    runs = {}
    for mode in (sr.SCM_RMS, sr.SCM_UNIFORM):
        params = _window_params(mi, mode)
        ref = sr.Sidechains(params)
        out, trace = ref.process(np.tile(x, (3, 1)))
        runs[mode] = (params, out, trace, ref)
    return x[0], runs


@pytest.mark.parametrize("mode", [sr.SCM_RMS, sr.SCM_UNIFORM])
def test_restatement_against_float64_window_sums(window_run, mode):
    """|trace - exact window sum| <= 1.01 (N + 4 k) 2^-24 S_max: the refresh sum is N terms added serially (at most N roundings of
    sums no larger than S_max, the terms' own roundings within the 1 %), every sample since then adds at most four roundings
    (two squares, their difference, the sum) of values no larger than S_max."""
    x, runs = window_run
    params, out, trace, ref = runs[mode]
    assert [(p["reactivity"], p["capacity"]) for p in params] == [(1, 513), (40, 552), (2400, 2912)]
    n = x.size
    term = np.abs(x).astype(np.float64)
    term = term * term if mode == sr.SCM_RMS else term
    cs = np.concatenate([[0.0], np.cumsum(term)])
    t = np.arange(n)
    k = np.where(t >= sr.REFRESH_RATE, t % sr.REFRESH_RATE, t) + 1             # samples since the last refresh (or the start)
    for ch, p in enumerate(params):
        N = p["reactivity"]
        exact = cs[t + 1] - cs[np.maximum(t + 1 - N, 0)]
        smax = np.maximum.accumulate(exact)
        bound = 1.01 * (N + 4 * k) * sr.U * smax
        err = np.abs(trace[ch].astype(np.float64) - exact)
        ratio = (err / bound).max()
        negative = int((trace[ch] < 0).sum())
        print("mode %d N %d: at most %.3f of the bound, the running sum negative at %d samples" % (mode, N, ratio, negative))
        assert np.all(err <= bound), (mode, N, ratio)
        # the clamps are exercised: after a loud stretch the rounding left in the sum of squares exceeds the quiet window's
        # 1e-6 N (the sum of magnitudes keeps 1e-3 N, above its rounding)
        assert negative > 0 or mode == sr.SCM_UNIFORM, (mode, N)
        assert np.all(out[ch][trace[ch] < 0] == 0.0) and np.all(out[ch] >= 0.0)
        pos = trace[ch] > 0
        want = trace[ch] * p["interval"]
        want = np.sqrt(want[pos]) if mode == sr.SCM_RMS else want[pos]
        assert np.array_equal(out[ch][pos], want.astype(f32))
    assert all(int(v) == 17 for v in ref.refresh) and [int(h) for h in ref.head] == [n % p["capacity"] for p in params]
    # three refreshes per channel; whether the window was wrapped in the ring follows from position and length
    assert len(ref.refreshes) == 9
    for ch, wrapped in ref.refreshes:
        assert params[ch]["reactivity"] <= params[ch]["capacity"] - sr.RING_EXTRA and isinstance(wrapped, (bool, np.bool_))


def test_restatement_refresh_split_on_a_hand_checked_ring(mi):
    """After 0x2000 samples a ring of 513 stands at 0x2000 % 513 = 497 and one of 552 at 464: the windows of 1 and 40 samples lie
    in one piece.  The ring of 2912 stands at 2368 < 2400: the window wraps, and the refresh is the sum of the oldest 32 samples
    plus the sum of the newest 2368, each taken serially -- not the one serial sum."""
    params = _window_params(mi, sr.SCM_RMS)
    ref = sr.Sidechains(params)
    x = np.tile((np.random.default_rng(5).standard_normal((1, sr.REFRESH_RATE + 1)) * 0.5).astype(f32), (3, 1))
    out, trace = ref.process(x)
    assert sorted(ref.refreshes) == [(0, False), (1, False), (2, True)]
    sq = (x[2, sr.REFRESH_RATE - 2400:sr.REFRESH_RATE] ** 2).astype(f32)
    first = 2400 - 2368
    two = sr.serial_sum(sq[:first]) + sr.serial_sum(sq[first:])
    last, new = x[2, sr.REFRESH_RATE - 2400], x[2, sr.REFRESH_RATE]
    assert trace[2, sr.REFRESH_RATE] == f32(two + (new * new - last * last))


PROBE = r'''
#include <lsp-plug.in/dsp-units/util/Sidechain.h>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using lsp::dspu::Sidechain;
using lsp::dspu::RawRingBuffer;

struct names: public lsp::dspu::IStateDumper
{
    std::vector<std::string> seen, closes;
    void begin_object(const char *n, const void *, size_t) override    { seen.push_back(n); }
    void end_object() override                                         { closes.push_back("end_object"); }
    void end_array() override                                          { closes.push_back("end_array"); }
    void write(const char *n, const void *) override                   { seen.push_back(n); }
    void write(const char *n, unsigned char) override                  { seen.push_back(n); }
    void write(const char *n, unsigned int) override                   { seen.push_back(n); }
    void write(const char *n, unsigned long) override                  { seen.push_back(n); }
    void write(const char *n, float) override                          { seen.push_back(n); }
};

struct probe: public Sidechain
{
    static void offsets()
    {
        printf("offsets %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", offsetof(probe, sBuffer), offsetof(probe, nReactivity),
               offsetof(probe, nSampleRate), offsetof(probe, pPreEq), offsetof(probe, fReactivity), offsetof(probe, fTau),
               offsetof(probe, fRmsValue), offsetof(probe, fMaxReactivity), offsetof(probe, fGain), offsetof(probe, nRefresh),
               offsetof(probe, nSource), offsetof(probe, nMode), offsetof(probe, nChannels), offsetof(probe, nFlags));
        printf("flagbits %d %d %d\n", int(SCF_MIDSIDE), int(SCF_UPDATE), int(SCF_CLEAR));
    }
    void show(const char *label) const
    {
        printf("%s %d %zu %g %g %u %d %d %d %zu %zu\n", label, int(nFlags), nReactivity, fReactivity, fRmsValue, nRefresh, int(nMode),
               int(nSource), int(nChannels), sBuffer.size(), sBuffer.position());
    }
    void settle()           { update_settings(); }
    void poke_rms(float v)  { fRmsValue = v; }
};

struct ring_probe: public RawRingBuffer
{
    static void offsets() { printf("ringoffsets %zu %zu %zu\n", offsetof(ring_probe, pData), offsetof(ring_probe, nCapacity), offsetof(ring_probe, nHead)); }
};

int main()
{
    // the public surface, by address
    void (Sidechain::*p1)(float *, const float **, size_t) = &Sidechain::process;
    float (Sidechain::*p2)(const float *) = &Sidechain::process;
    bool (Sidechain::*pi)(size_t, float) = &Sidechain::init;
    void (Sidechain::*ps)(lsp::dspu::sidechain_stereo_mode_t) = &Sidechain::set_stereo_mode;
    void (Sidechain::*pe)(lsp::dspu::Equalizer *) = &Sidechain::set_pre_equalizer;
    void (Sidechain::*pv)(lsp::dspu::IStateDumper *) const = &Sidechain::dump;
    size_t (RawRingBuffer::*r1)(const float *, size_t) = &RawRingBuffer::push;
    void (RawRingBuffer::*r2)(float) = &RawRingBuffer::push;
    size_t (RawRingBuffer::*r3)(float *, size_t, size_t) = &RawRingBuffer::read;
    float (RawRingBuffer::*r4)(size_t) const = &RawRingBuffer::read;
    const float *(RawRingBuffer::*r5)(size_t) const = &RawRingBuffer::tail;
    (void)p1; (void)p2; (void)pi; (void)ps; (void)pe; (void)pv; (void)r1; (void)r2; (void)r3; (void)r4; (void)r5;

    printf("sizeof %zu %zu\n", sizeof(Sidechain), sizeof(RawRingBuffer));
    probe::offsets();
    ring_probe::offsets();
    printf("enums %d %d %d %d %d %d | %d %d %d %d | %d %d\n", int(lsp::dspu::SCS_MIDDLE), int(lsp::dspu::SCS_SIDE), int(lsp::dspu::SCS_LEFT),
           int(lsp::dspu::SCS_RIGHT), int(lsp::dspu::SCS_AMIN), int(lsp::dspu::SCS_AMAX), int(lsp::dspu::SCM_PEAK), int(lsp::dspu::SCM_RMS),
           int(lsp::dspu::SCM_LPF), int(lsp::dspu::SCM_UNIFORM), int(lsp::dspu::SCSM_STEREO), int(lsp::dspu::SCSM_MIDSIDE));

    // construct() on raw memory and the setters' rules, no device involved
    void *raw = malloc(sizeof(Sidechain));
    memset(raw, 0xa5, sizeof(Sidechain));
    probe *m = reinterpret_cast<probe *>(raw);
    m->construct();
    m->show("fresh");
    printf("init %d %d %d\n", int(m->init(3, 50.0f)), int(m->init(0, 50.0f)), int(m->init(2, 50.0f)));
    m->set_sample_rate(48000);
    m->show("rate");
    m->set_reactivity(50.0f);
    m->settle();
    m->show("settled");                     // nReactivity 2400; UPDATE set nRefresh to 0x2000, CLEAR after it to 0
    m->set_reactivity(50.5f);               // above the maximum: ignored
    m->set_reactivity(-1.0f);               // negative: ignored
    m->set_reactivity(50.0f);               // unchanged: ignored
    m->show("ignored");
    m->set_reactivity(10.0f);
    m->show("reactivity");
    m->settle();
    m->show("forced");                      // nRefresh 0x2000: a refresh at the next sample
    m->poke_rms(3.0f);
    m->set_mode(lsp::dspu::SCM_RMS);        // unchanged: fRmsValue stays
    m->show("samemode");
    m->set_mode(lsp::dspu::SCM_UNIFORM);    // changed: fRmsValue = 0, no flag
    m->show("mode");
    m->set_stereo_mode(lsp::dspu::SCSM_STEREO);     // unchanged
    m->show("samestereo");
    m->set_stereo_mode(lsp::dspu::SCSM_MIDSIDE);    // MIDSIDE and CLEAR
    m->show("stereo");
    m->settle();
    m->clear();
    m->show("clear");
    m->set_source(lsp::dspu::SCS_AMAX);
    m->set_gain(-2.0f);
    printf("gain %g\n", m->get_gain());
    m->show("source");

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

    // RawRingBuffer on known answers: 5 samples
    RawRingBuffer rb;
    const bool made = rb.init(5);
    printf("ring_init %d %zu %zu\n", int(made), rb.size(), rb.position());
    const float a[4] = { 1, 2, 3, 4 }, b[3] = { 5, 6, 7 };
    printf("ring_push %zu", rb.push(a, 4));
    printf(" %zu", rb.position());
    printf(" %zu", rb.push(b, 3));                              // wraps: 5 at [4], 6 7 at [0] [1]
    printf(" %zu\n", rb.position());
    printf("ring_data");
    for (const float *p = rb.begin(); p != rb.end(); ++p)
        printf(" %g", *p);
    printf("\n");
    float got[5] = { 0, 0, 0, 0, 0 };
    printf("ring_read %g %g %g %zu", rb.read(1), rb.read(2), rb.read(5), rb.read(got, 4, 4));     // 7, 6, 3; 4 5 6 7
    printf(" %g %g %g %g\n", got[0], got[1], got[2], got[3]);
    printf("ring_tail %td %td %zu %zu %zu %zu\n", rb.tail(1) - rb.begin(), rb.tail(3) - rb.begin(), rb.head_remaining(), rb.tail_remaining(3),
           rb.remaining(3), rb.remaining(1));
    rb.push(8.0f);
    rb.write(9.0f);                                             // at the head, which stays
    printf("ring_single %zu %g %g", rb.position(), rb.read(1), *rb.head());
    printf(" %td\n", rb.advance(3) - rb.begin());
    const float c[7] = { 1, 2, 3, 4, 5, 6, 7 };
    printf("ring_long %zu %zu", rb.write(c, 7), rb.position());  // five of seven, from the head on, the head stays
    for (const float *p = rb.begin(); p != rb.end(); ++p)
        printf(" %g", *p);
    rb.fill(2.5f);
    printf(" %g %zu", rb.read(3), rb.position());
    rb.reset();
    printf(" %zu", rb.position());
    rb.advance(2);
    rb.clear();
    printf(" %zu %g\n", rb.position(), *rb.begin());
    // a block that ends at the ring's end leaves the position AT the capacity; a single sample then goes to the start
    printf("ring_end %zu", rb.push(a, 4));
    rb.push(b, 1);
    printf(" %zu %td", rb.position(), rb.head() - rb.begin());
    rb.push(8.0f);
    printf(" %zu %g", rb.position(), *rb.begin());
    rb.advance(3);
    rb.push(b, 3);                                              // 1 + 3 + 3 = 7 > 5: wraps to 2
    printf(" %zu\n", rb.position());
    names rn;
    rb.dump(&rn);
    printf("ring_dump");
    for (const std::string &s: rn.seen)
        printf(" %s", s.c_str());
    printf("\n");
    rb.destroy();
    printf("ring_gone %zu %d\n", rb.size(), int(rb.begin() == NULL));
    return 0;
}
'''


@pytest.fixture(scope="module")
def probe(mi, tmp_path_factory):
    d = tmp_path_factory.mktemp("sidechain_probe")
    src, exe = str(d / "sc_probe.cpp"), str(d / "sc_probe")
    with open(src, "w") as f:
        f.write(PROBE)
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-Wno-invalid-offsetof", "-I" + os.path.join(PKG, "include"),
                           "-I" + os.path.join(ROOT, "include"), src, "-o", exe, "-L" + PKG, "-lmi_dspu", "-Wl,-rpath," + PKG,
                           "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.check_output([exe]).decode().splitlines()
    return {l.split()[0]: l.split()[1:] for l in out}


def test_mirror_layout_is_the_references(probe):
    # RawRingBuffer (a pointer, two size_t), two size_t, a pointer, five floats, a uint32_t, four uint8_t: 76, padded to 80
    assert probe["sizeof"] == ["80", "24"]
    assert [int(v) for v in probe["offsets"]] == [0, 24, 32, 40, 48, 52, 56, 60, 64, 68, 72, 73, 74, 75]
    assert probe["ringoffsets"] == ["0", "8", "16"]
    assert probe["flagbits"] == ["1", "2", "4"]
    assert probe["enums"] == "0 1 2 3 4 5 | 0 1 2 3 | 0 1".split()


def test_mirror_setters_follow_the_references_rules(probe):
    # label: nFlags nReactivity fReactivity fRmsValue nRefresh nMode nSource nChannels capacity position
    assert probe["fresh"] == ["6", "0", "0", "0", "0", "1", "0", "0", "0", "0"]        # UPDATE | CLEAR, RMS, MIDDLE
    assert probe["init"] == ["0", "0", "1"]
    assert probe["rate"] == ["6", "0", "0", "0", "0", "1", "0", "2", "2912", "0"]      # the ring: 2400 + 0x200
    assert probe["settled"] == ["0", "2400", "50", "0", "0", "1", "0", "2", "2912", "0"]
    assert probe["ignored"] == probe["settled"]
    assert probe["reactivity"][:3] == ["2", "2400", "10"]                              # UPDATE pending, not yet computed
    assert probe["forced"][:5] == ["0", "480", "10", "0", "8192"]                      # a refresh is due
    assert probe["samemode"][3] == "3" and probe["samemode"][5] == "1"
    assert probe["mode"][0] == "0" and probe["mode"][3] == "0" and probe["mode"][5] == "3"     # zeroed, no flag, no refresh
    assert probe["mode"][4] == "8192"
    assert probe["samestereo"][0] == "0"
    assert probe["stereo"][0] == "5"                                                   # MIDSIDE | CLEAR
    assert probe["clear"][0] == "5" and probe["clear"][4] == "0"                       # settled (nRefresh 0), then CLEAR again
    assert probe["gain"] == ["-2"] and probe["source"][6] == "5"


def test_dump_writes_the_references_keys_in_order(probe):
    keys = json.load(open(os.path.join(ROOT, "tests", "golden", "sidechain_dump_keys.json")))
    assert probe["dump"] == keys["keys"]
    assert probe["closes"] == keys["closes"]
    assert probe["ring_dump"] == keys["keys"][1:4]


def test_raw_ring_buffer_known_answers(probe):
    assert probe["ring_init"] == ["1", "5", "0"]
    assert probe["ring_push"] == ["4", "4", "3", "2"]
    assert probe["ring_data"] == ["6", "7", "3", "4", "5"]
    assert probe["ring_read"] == ["7", "6", "3", "4", "4", "5", "6", "7"]
    # tail(1) is index 1, tail(3) index 4; 3 samples from the head to the end, 1 from tail(3), the nearer of the two
    assert probe["ring_tail"] == ["1", "4", "3", "1", "1", "3"]
    assert probe["ring_single"] == ["3", "8", "9", "1"]                                # push(8) at [2]; write(9) at [3]; advance(3): 6 % 5
    # write of 7 keeps 5: 1..4 at [1..4], 5 at [0]; the head stays at 1
    assert probe["ring_long"] == ["5", "1", "5", "1", "2", "3", "4", "2.5", "1", "0", "0", "0"]
    assert probe["ring_end"] == ["4", "5", "5", "1", "8", "2"]
    assert probe["ring_gone"] == ["0", "1"]


def test_mirrors_declare_the_references_public_names():
    names = json.load(open(os.path.join(ROOT, "tests", "golden", "sidechain_public_names.json")))
    assert set(names) == {"util/Sidechain.h", "util/RawRingBuffer.h"}
    for header, listed in names.items():
        text = open(os.path.join(PKG, "include", "lsp-plug.in", "dsp-units", header)).read()
        text = re.sub(r"//.*", "", text)
        assert len(listed) >= 20
        for name in listed:
            assert re.search(r"\b%s\b" % name, text), (header, name)
    text = re.sub(r"//.*", "", open(os.path.join(PKG, "include", "lsp-plug.in", "dsp-units", "util", "Sidechain.h")).read())
    fields = ("sBuffer", "nReactivity", "nSampleRate", "pPreEq", "fReactivity", "fTau", "fRmsValue", "fMaxReactivity", "fGain",
              "nRefresh", "nSource", "nMode", "nChannels", "nFlags")
    pos = [re.search(r"\b%s;" % n, text).start() for n in fields]
    assert pos == sorted(pos), "the protected fields are not in the reference's order"


def test_mirrors_export_the_references_symbols(mi):
    out = subprocess.check_output(["nm", "-D", "--defined-only", mi.LIB_PATH]).decode()
    for sym in ("_ZN3lsp4dspu9SidechainC1Ev", "_ZN3lsp4dspu9SidechainD1Ev", "_ZN3lsp4dspu9Sidechain9constructEv",
                "_ZN3lsp4dspu9Sidechain4initEmf", "_ZN3lsp4dspu9Sidechain7destroyEv", "_ZN3lsp4dspu9Sidechain15set_sample_rateEm",
                "_ZN3lsp4dspu9Sidechain14set_reactivityEf", "_ZN3lsp4dspu9Sidechain15set_stereo_modeENS0_23sidechain_stereo_mode_tE",
                "_ZN3lsp4dspu9Sidechain5clearEv", "_ZN3lsp4dspu9Sidechain7processEPfPPKfm", "_ZN3lsp4dspu9Sidechain7processEPKf",
                "_ZNK3lsp4dspu9Sidechain4dumpEPNS0_12IStateDumperE", "_ZN3lsp4dspu13RawRingBufferC1Ev", "_ZN3lsp4dspu13RawRingBuffer4initEm",
                "_ZN3lsp4dspu13RawRingBuffer4pushEPKfm", "_ZN3lsp4dspu13RawRingBuffer4pushEf", "_ZN3lsp4dspu13RawRingBuffer4readEPfmm",
                "_ZNK3lsp4dspu13RawRingBuffer4readEm", "_ZN3lsp4dspu13RawRingBuffer4tailEm", "_ZNK3lsp4dspu13RawRingBuffer4tailEm",
                "_ZN3lsp4dspu13RawRingBuffer7advanceEm", "_ZNK3lsp4dspu13RawRingBuffer14tail_remainingEm",
                "_ZNK3lsp4dspu13RawRingBuffer9remainingEm", "_ZN3lsp4dspu13RawRingBuffer4fillEf",
                "_ZNK3lsp4dspu13RawRingBuffer4dumpEPNS0_12IStateDumperE"):
        assert re.search(r" T %s$" % re.escape(sym), out, re.M), sym


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_chain_keeps_separate_multiplies_and_adds(tmp_path):
    """The bits of the restatement need the low-pass's tau * (x - rms) and rms + ... rounded on their own: no fused multiply-add
    in any form in the chain's body, under the Makefile's -ffp-contract=on."""
    isa_rounding.assert_separate_multiplies_and_adds(tmp_path, "sidechain.hip", "sidechain_chain_tile")
