"""DynamicDelay without a device: the serial numpy restatement against the reference's recorded outputs, lines and heads bit for
bit (every case), what the recorded cases are there for, the rule that lets steps run side by side (a numpy model of the kernel's
runs against the serial loop), the mirror header (size, names, field order, dump keys) and refusals that need no device."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import dyndelay_ref as dd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "lsp-dsp-units_amd")
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_dyndelay_vectors as gen  # noqa: E402

f32 = np.float32
u32 = np.uint32


@pytest.fixture(scope="module")
def recorded():
    return gen.load()


def test_restatement_equals_the_references_recorded_outputs(recorded):
    assert len(recorded) >= 60
    for c in recorded:
        out, a, b, _ = dd.run_case(c)
        assert np.array_equal(dd.bits(out), dd.bits(c["out"])), c["name"]
        assert [a.head, b.head] == [int(v) for v in c["head"]], c["name"]
        assert np.array_equal(dd.bits(a.ring()), dd.bits(c["ring_a"])), c["name"]
        assert np.array_equal(dd.bits(b.ring()), dd.bits(c["ring_b"])), c["name"]


def test_the_generator_still_makes_the_recorded_cases(recorded):
    """The committed operation lists and rows are the generator's (the outputs need the reference tree)."""
    made = gen.cases()
    assert [m["name"] for m in made] == [c["name"] for c in recorded]
    for m, c in zip(made, recorded):
        assert np.array_equal(m["ops"], c["ops"]) and np.array_equal(dd.bits(m["rows"]), dd.bits(c["rows"])), m["name"]
        assert (m["max_size"], m["other_size"]) == (c["max_size"], c["other_size"]), m["name"]
    gen.check_branches(made, recorded)


def test_recorded_cases_cover_what_the_issue_lists(recorded):
    sizes, calls, fdelays, whats = set(), set(), set(), set()
    for c in recorded:
        sizes.add(c["max_size"])
        assert np.isfinite(c["rows"][1]).all() and np.isfinite(c["rows"][3]).all(), "undefined in the reference: not to be recorded"
        for what, arg in c["ops"].tolist():
            whats.add(what)
            if what in (dd.P_A, dd.P_B):
                calls.add(arg)
        if len(set(c["rows"][3].tolist())) == 1:
            fdelays.add(float(c["rows"][3][0]))
        assert c["ring_a"].size == (dd.capacity_of(c["max_size"]) if dd.capacity_of(c["max_size"]) <= dd.RING_WHOLE else dd.RING_BEHIND)
    assert sizes >= {0, 5, 1000, 40000} and calls >= {1, 7, 256, 1023} and whats == set(range(7))
    assert fdelays >= {0.0, float(f32(0.99)), 1.0, 7.0, 63.0, 64.0, 300.0, 39000.0}
    gains = np.concatenate([c["rows"][2] for c in recorded])
    assert np.isnan(gains).any() and np.isinf(gains).any() and (gains == 1).any() and (np.abs(gains) > 1).any()
    assert (dd.bits(gains) == 0x80000000).any() and (dd.bits(gains) == 0).any()
    assert ((np.abs(gains) > 0) & (np.abs(gains) < np.finfo(f32).tiny)).any()
    ins = np.concatenate([c["rows"][0] for c in recorded])
    assert np.isnan(ins).any() and np.isposinf(ins).any() and np.isneginf(ins).any()
    delays = np.concatenate([c["rows"][1] for c in recorded])
    assert (delays < 0).any() and (delays > 40000).any()


def test_what_the_bank_defines_where_the_reference_does_not():
    """NaN and out-of-range delays convert with saturation, a NaN fdelay counts as 0."""
    cap = dd.capacity_of(1000)
    delay = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, 3e9, 9.3e18, 0.5, -0.5, 999.5, 1000.5], f32)
    fdelay = np.array([5, np.nan, 5, np.nan, 5, np.inf, -np.inf, np.nan, 1, 1e30, np.nan], f32)
    shift, tail, feed = dd.indices(100, cap, 1000, delay, fdelay)
    assert shift.tolist() == [0, 1000, 0, 1000, 0, 1000, 1000, 0, 0, 999, 1000]
    back = (feed - tail) % cap
    assert back.tolist() == [0, 0, 0, 0, 0, 1000, 0, 0, 0, 999, 0]


def model(head, max_size, line, inp, delay, fgain, fdelay, run=256):
    """The kernel's plan in numpy: stretches of 0x400 samples with their inputs placed at once, cut into runs in front of the
    first step whose feed is an earlier step's feed or tail or whose tail is an earlier step's feed; a run's steps all read, all
    add, all select.  Returns out, the share of steps in runs longer than one."""
    cap = line.size
    out, n, side = np.empty(inp.size, f32), inp.size, 0
    with np.errstate(all="ignore"):
        for pos in range(0, n, 0x400):
            m = min(0x400, n - pos)
            shift, tail, feed = dd.indices(head, cap, max_size, delay[pos:pos + m], fdelay[pos:pos + m])
            h = (head + np.arange(m)) % cap
            assert np.all((h - feed) % cap <= shift), "a feed ahead of its head: the kernel walks such a stretch as the reference does"
            line[h] = inp[pos:pos + m]
            a = 0
            while a < m:
                b = a + 1
                feeds, tails = {int(feed[a])}, {int(tail[a])}
                while b < min(a + run, m) and int(feed[b]) not in feeds and int(feed[b]) not in tails and int(tail[b]) not in feeds:
                    feeds.add(int(feed[b]))
                    tails.add(int(tail[b]))
                    b += 1
                t, f = tail[a:b], feed[a:b]
                s = line[t]
                v = (line[f] + (s * fgain[pos + a:pos + b]).astype(f32)).astype(f32)
                line[f] = v
                out[pos + a:pos + b] = np.where(f == t, v, s)
                side += (b - a) if b - a > 1 else 0
                a = b
            head = (head + m) % cap
    return out, head, side / n


@pytest.mark.parametrize("max_size", [1000, 40000])
def test_runs_of_steps_side_by_side_give_the_serial_loops_bits(max_size):
    rng = np.random.default_rng(99)
    n = 2500
    inp, gains = rng.standard_normal(n).astype(f32), rng.uniform(-0.95, 0.95, n).astype(f32)
    d = float(max_size) * 0.9
    shares = {}
    rows = {"echo": (np.full(n, d, f32), np.full(n, d, f32)), "fdelay 0": (np.full(n, d, f32), np.zeros(n, f32)),
            "fdelay 7": (np.full(n, d, f32), np.full(n, 7, f32)), "fdelay 64": (np.full(n, d, f32), np.full(n, 64, f32)),
            "chorus": ((d / 2 + d / 2.2 * np.sin(np.arange(n) / 83.0)).astype(f32), (d / 4 + d / 4.4 * np.sin(np.arange(n) / 47.0)).astype(f32)),
            "random": (rng.uniform(-50, max_size + 50, n).astype(f32), rng.uniform(-50, max_size + 50, n).astype(f32))}
    for name, (delay, fdelay) in rows.items():
        ref = dd.DynamicDelay(max_size)
        ref.head = ref.capacity - 700
        ref.line[:] = rng.standard_normal(ref.capacity).astype(f32)
        line = ref.line.copy()
        want = ref.process(inp, delay, gains, fdelay)
        got, head, shares[name] = model(ref.capacity - 700, max_size, line, inp, delay, gains, fdelay)
        assert np.array_equal(dd.bits(got), dd.bits(want)) and np.array_equal(dd.bits(line), dd.bits(ref.line)) and head == ref.head, name
    assert shares["echo"] == 1 and shares["fdelay 0"] == 1 and shares["fdelay 64"] == 1 and shares["fdelay 7"] == 1
    assert 0 < shares["random"] <= 1


def test_refusals(mi):
    """NULL handles are refused, never followed; a line longer than 2^24 floats is refused with or without a device."""
    lib = mi.lib
    byref, h, n = ctypes.byref, ctypes.c_void_p(), ctypes.c_uint32()
    assert lib.mi_dyndelay_bank_create(None, 1, 100) == -1 and lib.mi_dspu_last_error().decode().startswith("mi_dyndelay_bank_create")
    assert lib.mi_dyndelay_bank_create(byref(h), 0, 100) == -1 and not h.value
    for max_size in ((1 << 24) - 1025, 1 << 24, 1 << 40):
        assert dd.capacity_of(max_size) > 1 << 24
        assert lib.mi_dyndelay_bank_create(byref(h), 1, max_size) == -1 and not h.value, max_size
        assert "2^24" in lib.mi_dspu_last_error().decode()
    assert dd.capacity_of((1 << 24) - 1026) == 1 << 24                      # the longest line there is
    assert lib.mi_dyndelay_bank_destroy(None) == 0
    assert lib.mi_dyndelay_bank_get(None, 0, byref(n), byref(n), byref(n)) == -5
    assert lib.mi_dyndelay_bank_get_state(None, 0, None, None) == -5 and lib.mi_dyndelay_bank_set_state(None, 0, None, None) == -5
    assert lib.mi_dyndelay_bank_clear(None, None) == -5
    assert lib.mi_dyndelay_bank_process(None, None, None, None, None, None, 4, 4, 4, 4, 4, 4, None) == -5
    assert lib.mi_dyndelay_bank_copy(None, 0, None, 0, None) == -5
    assert lib.mi_dyndelay_bank_read_line(None, 0, None, 0, 4, None) == -5 and lib.mi_dyndelay_bank_write_line(None, 0, None, 0, 4, None) == -5
    assert lib.mi_dyndelay_bank_count_steps(None, 1, None) == -5 and lib.mi_dyndelay_bank_steps(None, None, None, None) == -5


def test_the_prefix_is_not_the_delay_banks(mi):
    names = [n for n in dir(mi.lib) if n.startswith("mi_dyndelay_bank_")]
    assert not any(n.startswith("mi_delay_bank_") for n in names)
    text = open(os.path.join(ROOT, "include", "mi_dspu.h")).read()
    declared = set(re.findall(r"\b(mi_dyndelay_bank_\w+)\s*\(", text))
    assert declared == {"mi_dyndelay_bank_" + n for n in ("create", "destroy", "get", "get_state", "set_state", "clear", "process", "copy",
                                                          "read_line", "write_line", "count_steps", "steps")}


PROBE = r'''
#define protected public
#include <lsp-plug.in/dsp-units/util/DynamicDelay.h>
#undef protected
#include <cstdio>
#include <cstdlib>
#include <cstring>
using namespace lsp::dspu;
struct keys: public IStateDumper
{
    void write(const char *n, const void *) override    { printf(" %s", n); }
    void write(const char *n, signed int) override      { printf(" %s", n); }
    void write(const char *n, unsigned int) override    { printf(" %s", n); }
};
int main()
{
    printf("sizeof %zu\n", sizeof(DynamicDelay));
    void *raw = malloc(sizeof(DynamicDelay));
    memset(raw, 0xa5, sizeof(DynamicDelay));
    DynamicDelay *d = reinterpret_cast<DynamicDelay *>(raw);
    d->construct();
    printf("fresh %d %u %u %d %d %zu %zu\n", d->vDelay == NULL, d->nHead, d->nCapacity, d->nMaxDelay, d->pData == NULL, d->max_delay(), d->capacity());
    float x[4] = { 1, 2, 3, 4 }, y[4] = { 9, 9, 9, 9 };
    d->process(y, x, x, x, x, 4);           // no line yet: nothing happens
    d->clear();
    d->copy(d);
    printf("untouched %g %u\n", y[0], d->nHead);
    printf("dump");
    keys k;
    d->dump(&k);
    printf("\n");
    d->destroy();
    free(raw);
    return 0;
}
'''


@pytest.fixture(scope="module")
def probe(mi, tmp_path_factory):
    d = tmp_path_factory.mktemp("dyndelay_probe")
    src, exe = str(d / "dd_probe.cpp"), str(d / "dd_probe")
    with open(src, "w") as f:
        f.write(PROBE)
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-I" + os.path.join(PKG, "include"), "-I" + os.path.join(ROOT, "include"),
                           src, "-o", exe, "-L" + PKG, "-lmi_dspu", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.check_output([exe]).decode().splitlines()
    return {l.split()[0]: l.split()[1:] for l in out if l.strip()}


def test_mirror_size_and_fresh_object_are_the_references(probe):
    assert probe["sizeof"] == ["32"]
    assert probe["fresh"] == ["1", "0", "0", "0", "1", "0", "0"]
    assert probe["untouched"] == ["9", "0"]


def test_dump_writes_the_references_keys_in_order(probe):
    keys = json.load(open(os.path.join(ROOT, "tests", "golden", "dyndelay_dump_keys.json")))
    assert keys["keys"] == ["vDelay", "nHead", "nCapacity", "nMaxDelay", "pData"] and probe["dump"] == keys["keys"] and keys["closes"] == []


def test_mirror_declares_the_references_public_names():
    names = json.load(open(os.path.join(ROOT, "tests", "golden", "dyndelay_public_names.json")))
    assert set(names) == {"util/DynamicDelay.h"}
    listed = names["util/DynamicDelay.h"]
    path = os.path.join(PKG, "include", "lsp-plug.in", "dsp-units", "util", "DynamicDelay.h")
    text = re.sub(r"//.*", "", open(path).read())
    assert len(listed) >= 11 and gen.public_names(path, "DynamicDelay") == listed
    for deleted in ("DynamicDelay(const DynamicDelay &) = delete", "DynamicDelay(DynamicDelay &&) = delete",
                    "operator = (const DynamicDelay &) = delete", "operator = (DynamicDelay &&) = delete"):
        assert deleted in text, deleted
    pos = [re.search(r"\b%s;" % n, text).start() for n in ("vDelay", "nHead", "nCapacity", "nMaxDelay", "pData")]
    assert pos == sorted(pos), "the fields are not in the reference's order"
    assert re.search(r"protected:\s*float\s*\*vDelay;", text)


def test_mirror_exports_the_references_symbols(mi):
    out = subprocess.check_output(["nm", "-D", "--defined-only", mi.LIB_PATH]).decode()
    for sym in ("_ZN3lsp4dspu12DynamicDelayC1Ev", "_ZN3lsp4dspu12DynamicDelayD1Ev", "_ZN3lsp4dspu12DynamicDelay9constructEv",
                "_ZN3lsp4dspu12DynamicDelay7destroyEv", "_ZN3lsp4dspu12DynamicDelay4initEm", "_ZN3lsp4dspu12DynamicDelay7processEPfPKfS4_S4_S4_m",
                "_ZN3lsp4dspu12DynamicDelay5clearEv", "_ZN3lsp4dspu12DynamicDelay4copyEPS1_", "_ZN3lsp4dspu12DynamicDelay4swapEPS1_",
                "_ZNK3lsp4dspu12DynamicDelay4dumpEPNS0_12IStateDumperE"):
        assert re.search(r" T %s$" % re.escape(sym), out, re.M), sym
