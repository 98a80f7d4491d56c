"""Oversampler without a device: the coefficient tables of mi_oversampler_coefficients, the mode tables, the float32
restatement against float64, the mirror header (layout, names, enum, dump order) and the rounding contract of the
upsample kernels' ISA."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import oversampler_ref as oref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "lsp-dsp-units_amd")
CSRC = os.path.join(PKG, "csrc")

# Oversampler::get_oversampling (Oversampler.cpp:146-195) and latency (:955-1006), the two switch statements as data
NAMES = ["OM_NONE"] + ["OM_LANCZOS_%dX%s" % (n, k) for n in (2, 3, 4, 6, 8) for k in ("2", "3", "4", "12BIT", "16BIT", "24BIT")]
TIMES = {"OM_NONE": 1}
LATENCY = {"OM_NONE": 0}
for _n in (2, 3, 4, 6, 8):
    for _k, _a in (("2", 2), ("3", 3), ("4", 4), ("12BIT", 4), ("16BIT", 10), ("24BIT", 62)):
        TIMES["OM_LANCZOS_%dX%s" % (_n, _k)] = _n
        LATENCY["OM_LANCZOS_%dX%s" % (_n, _k)] = _a
MODES = list(range(1, 31))


def _table(mi, mode):
    n = ctypes.c_size_t()
    mi.check(mi.lib.mi_oversampler_coefficients(mode, None, ctypes.byref(n)))
    h = np.zeros(n.value, np.float32)
    mi.check(mi.lib.mi_oversampler_coefficients(mode, h.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), ctypes.byref(n)))
    return h


@pytest.mark.parametrize("mode", MODES)
def test_coefficient_table(mi, mode):
    N, a = TIMES[NAMES[mode]], LATENCY[NAMES[mode]]
    h = _table(mi, mode)
    assert h.size == N * 2 * a
    h = h.reshape(N, 2 * a)
    assert np.array_equal(h, mi.OversamplerBank.coefficients(mode))
    unit = np.zeros(2 * a, np.float32)
    unit[a] = 1.0
    assert np.array_equal(h[0], unit)
    for k in range(1, N):
        x = np.arange(2 * a) - a + k / N
        want = (np.sinc(x) * np.sinc(x / a)).astype(np.float32)
        ulps = np.abs(h[k].view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
        assert ulps.max() <= 1, (mode, k, ulps)
        assert np.array_equal(h[k].view(np.uint32), h[N - k][::-1].view(np.uint32)), (mode, k)    # h_k[t] == h_{N-k}[2a-1-t]


@pytest.mark.parametrize("times", (2, 3, 4, 6, 8))
def test_16bit_tables_are_the_true_peak_tables_and_12bit_are_x4(mi, times):
    g = (2, 3, 4, 6, 8).index(times)
    m16, m12, m4 = 1 + 6 * g + 4, 1 + 6 * g + 3, 1 + 6 * g + 2
    n = ctypes.c_size_t()
    mi.check(mi.lib.mi_truepeak_coefficients(times, None, ctypes.byref(n)))
    tp = np.zeros(n.value, np.float32)
    mi.check(mi.lib.mi_truepeak_coefficients(times, tp.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), ctypes.byref(n)))
    assert np.array_equal(_table(mi, m16).view(np.uint32), tp.view(np.uint32))
    assert np.array_equal(_table(mi, m12).view(np.uint32), _table(mi, m4).view(np.uint32))


def test_coefficients_of_none_and_bad_modes(mi):
    n = ctypes.c_size_t(7)
    assert mi.lib.mi_oversampler_coefficients(0, None, ctypes.byref(n)) == 0 and n.value == 0
    assert mi.OversamplerBank.coefficients(0).size == 0
    for bad in (31, 32, 1000):
        assert mi.lib.mi_oversampler_coefficients(bad, None, ctypes.byref(n)) < 0
    assert mi.lib.mi_oversampler_coefficients(17, None, None) < 0


def test_mode_tables_of_the_restatement_and_the_wrapper(mi):
    assert mi.OversamplerBank.OM_NONE == 0
    for mode, name in enumerate(NAMES):
        assert oref.oversampling(mode) == TIMES[name], name
        assert oref.latency(mode) == LATENCY[name], name
        if mode:
            assert mi.OversamplerBank.MODES[name[len("OM_LANCZOS_"):]] == mode
            assert oref.MODES[name[len("OM_LANCZOS_"):]] == mode
    assert max(LATENCY.values()) == 62


def test_header_mode_constants_have_the_reference_values():
    text = open(os.path.join(ROOT, "include", "mi_dspu.h")).read()
    found = dict((k, int(v)) for k, v in re.findall(r"\bMI_(OM_[A-Z0-9_]+)\s*=\s*(\d+)", text))
    assert found == {name: i for i, name in enumerate(NAMES)}


@pytest.mark.parametrize("mode", MODES)
def test_restatement_is_within_the_a_priori_bound_of_float64(mi, mode):
    """A sum of 2a rounded products, started from zero: every partial sum and product carries one rounding of at most
    2^-24 relative, so |float32 - exact| <= (2a + 1) 2^-24 sum_t |h_k[t]| |x[i - t]| to first order."""
    N, a = TIMES[NAMES[mode]], LATENCY[NAMES[mode]]
    C, n = 4, 4096
    h = mi.OversamplerBank.coefficients(mode)
    ref = oref.OversamplerRef(C, mi.OversamplerBank.coefficients)
    ref.set_mode(mode)
    ref.update_settings()
    rng = np.random.default_rng(1000 + mode)
    worst = 0.0
    prev = np.zeros((C, 2 * a), np.float32)
    for blk in range(2):
        x = rng.standard_normal((C, n)).astype(np.float32)
        y = ref.upsample(x)
        ext = np.concatenate([prev, x], axis=1)
        exact = oref.gather(ext, h, n, np.float64)
        bound = (2 * a + 1) * 2.0 ** -24 * oref.gather(np.abs(ext), np.abs(h), n, np.float64)
        assert y.shape == (C, N * n) and y.dtype == np.float32
        err = np.abs(y.astype(np.float64) - exact)
        assert np.all(err <= bound), (mode, blk, float((err / np.maximum(bound, 1e-300)).max()))
        worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max()))
        # phase 0 is the input a samples back, copied
        assert np.array_equal(y[:, ::N].view(np.uint32), ext[:, a:a + n].view(np.uint32))
        prev = ext[:, -2 * a:]
    print("mode %d (N %d, a %d): worst error / bound %.3f" % (mode, N, a, worst))


def test_restatement_zero_sign_and_settings(mi):
    """A sum starts from +0.0f: negative zeros sum to +0, only the copied phase 0 keeps a -0.  The pending flags follow
    the reference (:108-144, :1055-1063)."""
    ref = oref.OversamplerRef(1, mi.OversamplerBank.coefficients)
    assert ref.modified()
    ref.update_settings()
    assert not ref.modified()
    ref.set_mode(0)
    ref.set_filtering(True)
    ref.set_sample_rate(0)
    assert not ref.modified()
    ref.set_mode(oref.MODES["4X2"])
    assert ref.modified() and ref.oversampling() == 4 and ref.latency() == 2
    ref.update_settings()
    y = ref.upsample(np.full((1, 16), -0.0, np.float32))
    assert np.all(y == 0)
    sign = np.signbit(y).reshape(16, 4)
    assert not sign[:, 1:].any() and sign[2:, 0].all() and not sign[:2, 0].any()
    ref.set_sample_rate(44100)
    assert ref.params[2] == np.float32(np.float32(44100) * np.float32(0.42)) and ref.design_rate == 4 * 44100
    ref.set_sample_rate(48000)
    assert ref.params[2] == np.float32(20000.0) and ref.params[:2] == (29, 30)
    assert ref.params[4:] == (np.float32(1.0), np.float32(0.1))


PROBE = r'''
#include <lsp-plug.in/dsp-units/util/Oversampler.h>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

using namespace lsp::dspu;

struct probe: public Oversampler
{
    static void layout()
    {
        #define OFF(m) printf("off_" #m " %zu %zu\n", offsetof(probe, m), sizeof(((probe *)0)->m))
        OFF(pCallback); OFF(fUpBuffer); OFF(fDownBuffer); OFF(pFunc); OFF(nUpHead); OFF(nMode); OFF(nSampleRate); OFF(nUpdate);
        OFF(sFilter); OFF(bData); OFF(bFilter);
        #undef OFF
        static_assert(std::is_same<decltype(probe::pCallback), IOversamplerCallback *>::value, "pCallback");
        static_assert(std::is_same<decltype(probe::fUpBuffer), float *>::value, "fUpBuffer");
        static_assert(std::is_same<decltype(probe::fDownBuffer), float *>::value, "fDownBuffer");
        static_assert(std::is_same<decltype(probe::pFunc), void (*)(float *, const float *, size_t)>::value, "pFunc");
        static_assert(std::is_same<decltype(probe::nUpHead), size_t>::value, "nUpHead");
        static_assert(std::is_same<decltype(probe::nMode), size_t>::value, "nMode");
        static_assert(std::is_same<decltype(probe::nSampleRate), size_t>::value, "nSampleRate");
        static_assert(std::is_same<decltype(probe::nUpdate), size_t>::value, "nUpdate");
        static_assert(std::is_same<decltype(probe::sFilter), Filter>::value, "sFilter");
        static_assert(std::is_same<decltype(probe::bData), uint8_t *>::value, "bData");
        static_assert(std::is_same<decltype(probe::bFilter), bool>::value, "bFilter");
        printf("flags %d %d %d %d\n", int(UP_MODE), int(UP_SAMPLE_RATE), int(UP_OTHER), int(UP_ALL));
        resample_func_t f = get_function(OM_LANCZOS_4X16BIT);
        (void)f;
    }
};

struct names: public IStateDumper
{
    std::vector<std::string> seen;
    int depth = 0;
    void begin_object(const char *n, const void *, size_t) override { if (depth++ == 0) seen.push_back(n); }
    void begin_object(const void *, size_t) override           { ++depth; }
    void end_object() override                                  { --depth; }
    void write(const char *n, const void *) override           { if (!depth) seen.push_back(n); }
    void write(const char *n, bool) override                   { if (!depth) seen.push_back(n); }
    void write(const char *n, size_t) override                 { if (!depth) seen.push_back(n); }
};

static void twice(float *out, const float *in, size_t n, void *arg) { for (size_t i = 0; i < n; ++i) out[i] = in[i] * *(float *)arg; }

int main()
{
    void (Oversampler::*p1)(float *, const float *, size_t, IOversamplerCallback *) = &Oversampler::process;
    void (Oversampler::*p2)(float *, const float *, size_t, oversampler_callback_t, void *) = &Oversampler::process;
    void (Oversampler::*p3)(float *, const float *, size_t) = &Oversampler::process;
    void (Oversampler::*pu)(float *, const float *, size_t) = &Oversampler::upsample;
    void (Oversampler::*pd)(float *, const float *, size_t) = &Oversampler::downsample;
    bool (Oversampler::*pi)() = &Oversampler::init;
    void (Oversampler::*pc)() = &Oversampler::construct;
    void (Oversampler::*px)() = &Oversampler::destroy;
    void (Oversampler::*ps)(size_t) = &Oversampler::set_sample_rate;
    void (Oversampler::*pb)(IOversamplerCallback *) = &Oversampler::set_callback;
    void (Oversampler::*pm)(over_mode_t) = &Oversampler::set_mode;
    over_mode_t (Oversampler::*pg)() const = &Oversampler::mode;
    void (Oversampler::*pf)(bool) = &Oversampler::set_filtering;
    bool (Oversampler::*ph)() const = &Oversampler::filtering;
    bool (Oversampler::*pq)() const = &Oversampler::modified;
    size_t (Oversampler::*po)() const = &Oversampler::get_oversampling;
    void (Oversampler::*pt)() = &Oversampler::update_settings;
    size_t (Oversampler::*pl)() const = &Oversampler::latency;
    size_t (Oversampler::*pn)() const = &Oversampler::max_latency;
    void (Oversampler::*pv)(IStateDumper *) const = &Oversampler::dump;
    (void)p1; (void)p2; (void)p3; (void)pu; (void)pd; (void)pi; (void)pc; (void)px; (void)ps; (void)pb; (void)pm; (void)pg; (void)pf;
    (void)ph; (void)pq; (void)po; (void)pt; (void)pl; (void)pn; (void)pv;

    printf("sizeof %zu %zu %zu\n", sizeof(Oversampler), sizeof(Filter), alignof(Oversampler));
    printf("max %zu\n", size_t(OVERSAMPLER_MAX_LATENCY));
    probe::layout();
    printf("enum");
    for (int m = OM_NONE; m <= OM_LANCZOS_8X24BIT; ++m)
        printf(" %d", m);
    printf(" %d %d %d %d\n", int(OM_LANCZOS_2X2), int(OM_LANCZOS_4X16BIT), int(OM_LANCZOS_6X12BIT), int(OM_LANCZOS_8X24BIT));

    // construct() on raw memory, no device involved
    void *raw = malloc(sizeof(Oversampler));
    memset(raw, 0xa5, sizeof(Oversampler));
    Oversampler *o = reinterpret_cast<Oversampler *>(raw);
    o->construct();
    printf("fresh %d %d %d %zu %zu %zu\n", int(o->mode()), int(o->filtering()), int(o->modified()), o->get_oversampling(), o->latency(),
           o->max_latency());
    printf("modes");
    for (int m = OM_NONE; m <= OM_LANCZOS_8X24BIT; ++m)
    {
        o->set_mode(over_mode_t(m));
        printf(" %zu:%zu", o->get_oversampling(), o->latency());
    }
    printf("\n");
    names n;
    o->dump(&n);
    printf("dump");
    for (const std::string &s: n.seen)
        printf(" %s", s.c_str());
    printf("\n");

    // OM_NONE needs no device: a copy, or the callback alone (:731-737, :945-951)
    o->set_mode(OM_NONE);
    float x[4] = { 1, 2, 3, 4 }, y[4] = { 0, 0, 0, 0 }, g = 2.0f;
    IOversamplerCallback plain;
    o->process(y, x, 4, &plain);
    printf("none %g %g", y[0], y[3]);
    o->process(y, x, 4, twice, &g);
    printf(" %g %g\n", y[0], y[3]);
    o->destroy();
    free(raw);
    return 0;
}
'''


def _probe(tmp_path):
    src = os.path.join(str(tmp_path), "os_probe.cpp")
    exe = os.path.join(str(tmp_path), "os_probe")
    with open(src, "w") as f:
        f.write(PROBE)
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-Wno-invalid-offsetof", "-I" + os.path.join(PKG, "include"),
                           "-I" + os.path.join(ROOT, "include"), src, "-o", exe, "-L" + PKG, "-lmi_dspu", "-Wl,-rpath," + PKG,
                           "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.check_output([exe]).decode().splitlines()
    return {l.split()[0]: l.split()[1:] for l in out}


def test_mirror_header_layout_enum_and_dump_order(tmp_path):
    r = _probe(tmp_path)
    # the reference's layout (Oversampler.h:123-133) from the declared member types, LP64
    members = [("pCallback", 8, 8), ("fUpBuffer", 8, 8), ("fDownBuffer", 8, 8), ("pFunc", 8, 8), ("nUpHead", 8, 8), ("nMode", 8, 8),
               ("nSampleRate", 8, 8), ("nUpdate", 8, 8), ("sFilter", int(r["sizeof"][1]), 8), ("bData", 8, 8), ("bFilter", 1, 1)]
    off = 0
    for name, size, align in members:
        off = (off + align - 1) // align * align
        assert r["off_" + name] == [str(off), str(size)], (name, r["off_" + name], off, size)
        off += size
    assert r["sizeof"] == [str((off + 7) // 8 * 8), "88", "8"]
    assert r["sizeof"][0] == "168"
    assert r["max"] == ["62"]
    assert r["flags"] == ["1", "4", "8", "13"]
    assert r["enum"] == [str(i) for i in range(31)] + ["1", "17", "22", "30"]
    assert r["fresh"] == ["0", "1", "1", "1", "0", "62"]
    assert r["modes"] == ["%d:%d" % (TIMES[n], LATENCY[n]) for n in NAMES]
    # Oversampler.cpp:1075-1088
    assert r["dump"] == ["pCallback", "fUpBuffer", "fDownBuffer", "pFunc", "nUpHead", "nMode", "nSampleRate", "nUpdate", "sFilter",
                         "bData", "bFilter"]
    assert r["none"] == ["1", "4", "2", "8"]


def test_mirror_header_declares_the_reference_names():
    text = open(os.path.join(PKG, "include", "lsp-plug.in", "dsp-units", "util", "Oversampler.h")).read()
    text = re.sub(r"//.*", "", text)
    for name in ("IOversamplerCallback", "oversampler_callback_t", "over_mode_t", "OVERSAMPLER_MAX_LATENCY", "resample_func_t",
                 "update_t", "UP_MODE", "UP_SAMPLE_RATE", "UP_OTHER", "UP_ALL", "pCallback", "fUpBuffer", "fDownBuffer", "pFunc",
                 "nUpHead", "nMode", "nSampleRate", "nUpdate", "sFilter", "bData", "bFilter", "get_function", "construct", "init",
                 "destroy", "set_sample_rate", "set_callback", "set_mode", "mode", "set_filtering", "filtering", "modified",
                 "get_oversampling", "update_settings", "upsample", "downsample", "process", "latency", "max_latency", "dump"):
        assert re.search(r"\b%s\b" % name, text), name
    for name in NAMES:
        assert re.search(r"\b%s\b" % name, text), name
    assert re.search(r"Filter\s+sFilter;", text)


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_upsample_kernels_keep_separate_multiplies_and_adds(tmp_path):
    """The bits of the restatement need every product and every sum rounded on its own: no fused multiply-add in any
    form in any upsample kernel, under the Makefile's -ffp-contract=on; packed multiplies and adds where a <= 10."""
    out = os.path.join(str(tmp_path), "oversampler.s")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=on", "-w",
                           "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-I" + os.path.join(PKG, "include"),
                           "-S", "--offload-device-only", os.path.join(CSRC, "oversampler.hip"), "-o", out])
    lines = open(out).read().split("\n")
    bodies, cur = {}, None
    for l in lines:
        m = re.match(r"^(_Z\w+):", l)
        if m:
            cur = m.group(1)
            bodies[cur] = []
        elif cur and (l.startswith(".Lfunc_end") or ".amdhsa_kernel" in l):
            cur = None
        elif cur:
            bodies[cur].append(l.strip())
    seen = set()
    for times in (2, 3, 4, 6, 8):
        for a in (2, 3, 4, 10, 62):
            names = [n for n in bodies if "oversampler_up_kernelILi%dELi%dEE" % (times, a) in n]
            assert len(names) == 1, (times, a, names)
            ops = [l.split()[0] for l in bodies[names[0]] if l and not l.startswith((";", "."))]
            fused = [o for o in ops if o.startswith(("v_fma", "v_fmac", "v_pk_fma", "v_mac_f", "v_mad_f", "v_mad_legacy_f"))]
            assert not fused, (times, a, fused)
            if a <= 10:
                assert "v_pk_mul_f32" in ops and "v_pk_add_f32" in ops, (times, a)
            else:
                assert ("v_mul_f32" in ops or "v_mul_f32_e32" in ops or "v_pk_mul_f32" in ops), (times, a)
            seen.add((times, a))
    assert len(seen) == 25
