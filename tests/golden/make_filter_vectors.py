"""Writes tests/golden/filter_ref_designs.npz and filter_ref_streams.npz: what the reference's own Filter and FilterBank classes
(oracle/_ref/filter_ref: Filter.cpp and FilterBank.cpp compiled unmodified, see oracle/Makefile) compute on a list of designs and of
stream cases.  Data only: parameters, calls, events, one shared input row, the sections the reference's bank held, what the filter
reported and its outputs.  Run where the reference tree exists, after the build:

    python tests/golden/make_filter_vectors.py

Every case first runs through oracle/_ref/filter_ref_san, the same program with the address and undefined-behaviour sanitizers (a
stand-alone host program); nothing is written unless that run is clean and gives the same bytes.  The section arithmetic under the
reference's classes is a stand-in (oracle/ref_overlay/filters): nothing is written unless every recorded output is
oracle.biquad_cascade on the recorded sections bit for bit, and unless every boundary at which the reference keeps (or clears) the
delays is one where keeping and clearing give clearly different outputs.  tests/test_filter_reference_host.py regenerates the files
with build_bytes() and requires the committed bytes, so they are written without time stamps.  The layout is
tests/filter_reference.py's, which reads them.
"""
import io
import os
import subprocess
import sys
import tempfile
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import filter_reference as fr  # noqa: E402

f32 = np.float32
FLT_REF = os.path.join(ROOT, "oracle", "_ref", "filter_ref")
FLT_SAN = os.path.join(ROOT, "oracle", "_ref", "filter_ref_san")
TOL = 1e-5                                      # tests/conftest.py's TOL: the margin below is 100 x this
NTYPES = 81


def types():
    from oracle import filter_design as fd
    assert len(fd.FILTER_TYPES) == NTYPES
    return fd.T


def family(name):
    for key in ("_RLC_", "_BWC_", "_LRX_", "_APO_", "_WEIGHTED", "AMPLIFIER", "NONE"):
        if key in name:
            return key.strip("_")
    raise ValueError(name)


# ---- designs -------------------------------------------------------------------------------------------------------------
TRIPLES_48K = [(100.0, 400.0, 0.5, 0.0), (1000.0, 250.0, 2.0, 0.7), (9000.0, 15000.0, 4.0, 2.5)]     # fFreq, fFreq2, fGain, fQuality
TRIPLE_44K = (3000.0, 7000.0, 0.25, 1.2)
PLUS_6_DB = 1.9952623844146729                  # float32 of 10^(6/20): the gain of tests/golden/filter_anchors.json's high-shelf
SLOPE8 = ("FLT_BT_RLC_LOPASS", "FLT_MT_BWC_BELL", "FLT_BT_LRX_HISHELF", "FLT_DR_APO_PEAKING", "FLT_K_WEIGHTED", "FLT_MT_AMPLIFIER")


def designs():
    """(sample rate, fp): every type at slopes 1-4 with three triples at 48 kHz and one at 44.1 kHz, slope 8 for one type per family,
    and the edges of Filter::limit."""
    T = types()
    out = []
    for t in range(NTYPES):
        for slope in (1, 2, 3, 4):
            for q in TRIPLES_48K:
                out.append((48000, (t, slope) + q))
            out.append((44100, (t, slope) + TRIPLE_44K))
    for name in SLOPE8:
        out.append((48000, (T[name], 8) + TRIPLES_48K[1]))
    out.append((48000, (T["FLT_BT_BWC_HISHELF"], 2, 1000.0, 1000.0, PLUS_6_DB, 0.0)))      # the design of filter_anchors.json
    for name in ("FLT_BT_RLC_LOPASS", "FLT_MT_RLC_BELL", "FLT_BT_BWC_HISHELF", "FLT_BT_LRX_BANDPASS", "FLT_DR_APO_LADDERPASS"):
        t = T[name]
        out.append((48000, (t, 2, 30000.0, 1000.0, 2.0, 0.5)))          # fFreq above 0.49 sr
        out.append((48000, (t, 2, 1000.0, 24000.0, 2.0, 0.5)))          # fFreq2 above 0.49 sr
        out.append((48000, (t, 2, -100.0, 1000.0, 2.0, 0.5)))           # negative frequencies are limited to 0
        out.append((48000, (t, 2, 1000.0, -5.0, 2.0, 0.5)))
        out.append((48000, (t, 0, 1000.0, 3000.0, 2.0, 0.5)))           # slope 0 -> 1
        out.append((48000, (t, 1000, 1000.0, 3000.0, 2.0, 0.5)))        # slope 1000 -> FILTER_CHAINS_MAX
    return out


def grid():
    """The full grid of tests/test_filter_reference_host.py: 81 types x 6 slopes x 5 frequencies x 4 (gain, Q) x 3 rates = 29 160."""
    out = []
    for sr in (44100, 48000, 96000):
        for t in range(NTYPES):
            for slope in (1, 2, 3, 4, 5, 8):
                for freq in (100.0, 440.0, 2500.0, 9000.0, 23000.0):
                    for gain, q in ((0.1, 0.0), (0.5, 0.7), (2.0, 1.5), (15.8, 3.0)):
                        out.append((sr, (t, slope, freq, 2.5 * freq if freq < 5000 else 0.3 * freq, gain, q)))
    return out


# ---- streams -------------------------------------------------------------------------------------------------------------
CUTS = [257, 300, 443]                          # 1000 samples in three calls
NX = 6000


def signal():
    return np.random.default_rng(20241019).uniform(-1.0, 1.0, NX).astype(f32)


def stream_cases():
    T = types()
    P = lambda name, slope, freq=1000.0, freq2=3000.0, gain=2.0, q=0.5: (T[name], slope, freq, freq2, gain, q)
    up = lambda before, fp, sr=48000: (before, fr.UPDATE, sr, fp)
    none = P("FLT_NONE", 1)
    out = []

    def add(name, fp, events, shared=(0, 3), calls=CUTS, other=none):
        for s in shared:
            out.append(dict(name="%s, %s" % (name, ("own bank", "neighbour ahead", "neighbour behind", "bank of one")[s]), shared=s,
                            sample_rate=48000, fp=fp, other=other, calls=list(calls), events=list(events)))

    bell = lambda slope, gain=2.0, freq=1000.0, q=0.5: P("FLT_BT_RLC_BELL", slope, freq, 3000.0, gain, q)
    # only the gain, the frequency or the quality changes: no FF_CLEAR (Filter.cpp:154-158), the delays are kept
    add("gain only", bell(2), [up(1, bell(2, 0.5)), up(2, bell(2, 4.0))])
    add("frequency only", P("FLT_BT_RLC_LOPASS", 4, 300.0), [up(1, P("FLT_BT_RLC_LOPASS", 4, 2000.0)), up(2, P("FLT_BT_RLC_LOPASS", 4, 700.0))])
    add("quality only", P("FLT_MT_RLC_BELL", 3, q=0.5), [up(1, P("FLT_MT_RLC_BELL", 3, q=3.0)), up(2, P("FLT_MT_RLC_BELL", 3, q=0.0))])
    # the type changes, the number of sections does not: a filter with its own bank clears, a shared bank keeps
    add("type changed", P("FLT_BT_RLC_LOPASS", 2), [up(1, P("FLT_BT_BWC_LOPASS", 2)), up(2, P("FLT_DR_APO_PEAKING", 2))])
    # the slope changes, the number of sections does not (RLC low-pass: slopes 1 and 2 are one section)
    add("slope changed, count kept", P("FLT_BT_RLC_LOPASS", 1, 500.0), [up(1, P("FLT_BT_RLC_LOPASS", 2, 500.0)), up(2, P("FLT_BT_RLC_LOPASS", 1, 500.0))])
    # the slope and the number of sections change: FilterBank::end clears on nItems != nLastItems
    add("slope changed, count changed", bell(2), [up(1, bell(3)), up(2, bell(2))])
    add("to FLT_NONE and back", bell(2), [up(1, none), up(2, bell(2))])
    # two updates ahead of one call, the second back to the first type: the flag of the first stays
    add("type there and back ahead of one call", bell(2), [up(1, P("FLT_BT_RLC_NOTCH", 2)), up(1, bell(2, 0.5)), up(2, bell(2, 0.5))])
    # clear() without any update
    add("clear() alone", bell(3), [(2, fr.CLEAR, 0, none)], shared=(0,))
    # next to another filter on a shared bank: a gain update keeps the delays of both, a changed count clears those of both
    add("beside a shelf", bell(3), [up(1, bell(3, 0.5)), up(2, bell(4, 0.5))], shared=(1, 2), other=P("FLT_BT_RLC_HISHELF", 2, 4000.0))
    # 1, 2, 3, 4, 7, 8, 9 and 15 sections: every x8 / x4 / x2 / x1 packing of FilterBank::end, the delays kept over a gain update
    for k in (1, 2, 3, 4, 7, 8, 9, 15):
        add("%d sections" % k, bell(k, 2.0, 800.0 + 150.0 * k), [up(1, bell(k, 0.6, 800.0 + 150.0 * k))], calls=[300, 333])
    # impulse_response() between two calls: the delays are saved and put back (FilterBank.cpp:293-330)
    add("impulse response between calls", bell(9), [(1, fr.IMPULSE, 64, none), up(2, bell(9, 0.5)), (2, fr.IMPULSE, 48, none)], shared=(0,))
    # the filter of tests/golden/filter_anchors.json: its sections and the head of its impulse response
    add("anchor high-shelf", P("FLT_BT_BWC_HISHELF", 2, 1000.0, 1000.0, PLUS_6_DB, 0.0), [(0, fr.IMPULSE, 8, none)], shared=(0,), calls=[16])
    # long: past the bank kernel's tiles, with retunes that keep the delays
    add("long low-pass of 8 sections", P("FLT_BT_LRX_LOPASS", 4, 1500.0), [up(1, P("FLT_BT_LRX_LOPASS", 4, 900.0)), up(2, P("FLT_BT_LRX_LOPASS", 4, 2500.0))],
        shared=(3,), calls=[2049, 2047, 104])
    add("long bell of 15 sections", bell(15, 1.5, 3000.0), [up(1, bell(15, 0.7, 3000.0)), up(2, bell(15, 0.7, 5000.0))], shared=(0,), calls=[1023, 3072, 105])
    return out


def run_driver(exe, cs, timeout=900, case_bytes=fr.case_bytes):
    """Runs a driver over the cases under a time limit; its standard error must stay empty (a sanitizer writes there)."""
    with tempfile.TemporaryDirectory() as d:
        src, dst = os.path.join(d, "cases.bin"), os.path.join(d, "results.bin")
        with open(src, "wb") as f:
            f.write(case_bytes(cs))
        p = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=timeout)
        if exe.endswith("_san") and "LeakSanitizer has encountered a fatal error" in p.stderr:
            # the sanitizer twin's leak check needs ptrace, which a build machine may withhold: there, and only there, the run
            # is repeated for the bounds and the undefined arithmetic alone
            p = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=timeout,
                               env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
        if p.returncode != 0 or p.stderr.strip():
            raise RuntimeError("%s: exit status %d\n%s" % (exe, p.returncode, p.stderr[-4000:]))
        with open(dst, "rb") as f:
            return f.read()


def run_both(cs):
    san = fr.parse_results(run_driver(FLT_SAN, cs), cs)
    res = fr.parse_results(run_driver(FLT_REF, cs), cs)
    for c, a, b in zip(cs, san, res):                                   # (parse_results makes every NaN the canonical one)
        same = all(np.array_equal(fr.bits(u), fr.bits(v)) for u, v in zip(a["sections"] + a["irs"] + [a["out"]] + [ch["packed"].view(f32) for ch in a["charts"]],
                                                                          b["sections"] + b["irs"] + [b["out"]] + [ch["packed"].view(f32) for ch in b["charts"]]))
        assert same and all(np.array_equal(a[k], b[k]) for k in ("inactive", "latency", "limited")), "the sanitizer build computes something else: %s" % (c["fp"],)
    return res


def run_designs():
    T = types()
    apo = {t for name, t in T.items() if "_APO_" in name}
    ds = designs()
    # freq_chart is recorded for the APO designs alone: their evaluation is Filter.cpp's own text (:405-498); every other chart goes
    # through lsp-dsp-lib's filter_transfer_*, whose stand-ins end the program
    cs = [fr.design_case(sr, fp, chart=fp[0] in apo) for sr, fp in ds]
    res = run_both(cs)
    for c, r in zip(cs, res):
        for ch in r["charts"]:                                          # the two overloads of freq_chart agree in every bit
            assert np.array_equal(ch["packed"].view(f32).view(np.uint32), ch["split"].view(f32).view(np.uint32)) and np.isfinite(ch["packed"]).all(), c["fp"]
    return ds, res


def margin(c, oracle, i):
    """How far apart keeping and clearing the delays at the start of call i are, over the 64 samples after it, against the peak."""
    base = [b[1] for b in fr.boundaries(c)]
    other = list(base)
    other[i] = not other[i]
    a, b = fr.replay(c, oracle, base)[0], fr.replay(c, oracle, other)[0]
    at = sum(c["calls"][:i])
    w = slice(at, at + 64)
    return float(np.max(np.abs(a[w].astype(np.float64) - b[w]))) / max(float(np.max(np.abs(a[w]))), 1e-30)


def run_streams():
    import oracle
    x = signal()
    cs = stream_cases()
    for k, c in enumerate(cs):
        n = sum(c["calls"])
        for at in range(37 * k, NX - n, 101):                       # the input is chosen until every boundary proves something
            c["at"], c["x"] = at, x[at:at + n]
            c.update(run_both([c])[0])
            bounds = fr.boundaries(c)
            worst = min([margin(c, oracle, i) for i in range(1, len(c["calls"]))
                         if bounds[i][0] and len(c["sections"][i]) == len(c["sections"][i - 1]) and len(c["sections"][i])] or [1.0])
            if worst > 100 * TOL:
                break
        else:
            raise AssertionError("%s: no input at which keeping and clearing differ" % c["name"])
        # the stand-in's packing has no arithmetic effect: the output is the oracle's recurrence on the recorded sections
        out, irs = fr.replay(c, oracle)
        assert np.array_equal(fr.bits(out), fr.bits(c["out"])), c["name"]
        assert len(irs) == len(c["irs"]) and all(np.array_equal(fr.bits(a), fr.bits(b)) for a, b in zip(irs, c["irs"])), c["name"]
    return cs, x


def design_arrays(ds, res):
    return {
        "sample_rate": np.array([sr for sr, _ in ds], np.uint32),
        "fp": np.stack([fr.fp_words(fp) for _, fp in ds]),
        "nsec": np.array([len(r["sections"][0]) for r in res], np.uint32),
        "sections": np.concatenate([r["sections"][0] for r in res]).astype(f32),
        "inactive": np.array([r["inactive"][0] for r in res], np.uint8),
        "latency": np.array([r["latency"][0] for r in res], np.uint32),
        "limited": np.stack([r["limited"][0] for r in res]).astype(np.uint32),
        "chart_of": np.array([i for i, r in enumerate(res) if r["charts"]], np.uint32),
        "chart": np.stack([r["charts"][0]["packed"] for r in res if r["charts"]]).astype(np.complex64),
    }


def stream_arrays(cs, x):
    a = {"names": np.array([c["name"] for c in cs]), "x": x}
    for k in ("shared", "sample_rate", "at"):
        a[k] = np.array([c[k] for c in cs], np.uint32)
    a["n"] = np.array([len(c["x"]) for c in cs], np.uint32)
    a["fp"] = np.stack([fr.fp_words(c["fp"]) for c in cs])
    a["other"] = np.stack([fr.fp_words(c["other"]) for c in cs])
    a["ncalls"] = np.array([len(c["calls"]) for c in cs], np.uint32)
    a["calls"] = np.array([v for c in cs for v in c["calls"]], np.uint32)
    a["nevents"] = np.array([len(c["events"]) for c in cs], np.uint32)
    a["events"] = np.array([np.concatenate([np.array(e[:3], np.uint32), fr.fp_words(e[3])]) for c in cs for e in c["events"]], np.uint32).reshape(-1, 9)
    a["nsec"] = np.array([len(s) for c in cs for s in c["sections"]], np.uint32)
    a["sections"] = np.concatenate([s for c in cs for s in c["sections"]]).astype(f32)
    a["inactive"] = np.array([v for c in cs for v in c["inactive"]], np.uint8)
    a["latency"] = np.array([v for c in cs for v in c["latency"]], np.uint32)
    a["limited"] = np.stack([w for c in cs for w in c["limited"]]).astype(np.uint32)
    a["out"] = np.concatenate([c["out"] for c in cs]).astype(f32)
    a["ir_len"] = np.array([len(r) for c in cs for r in c["irs"]], np.uint32)
    a["ir"] = np.concatenate([r for c in cs for r in c["irs"]] or [np.zeros(0, f32)]).astype(f32)
    return a


def npz_bytes(arrs):
    """An .npz without time stamps: the same arrays give the same bytes."""
    b = io.BytesIO()
    with zipfile.ZipFile(b, "w") as z:
        for name in sorted(arrs):
            a = io.BytesIO()
            np.lib.format.write_array(a, np.ascontiguousarray(arrs[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, a.getvalue(), compresslevel=9)
    return b.getvalue()


def build_bytes():
    """-> (the bytes of filter_ref_designs.npz, the bytes of filter_ref_streams.npz)"""
    d = npz_bytes(design_arrays(*run_designs()))
    s = npz_bytes(stream_arrays(*run_streams()))
    assert len(d) < 400 * 1000 and len(s) < 400 * 1000, (len(d), len(s))
    return d, s


if __name__ == "__main__":
    d, s = build_bytes()
    for path, data in ((fr.DESIGNS, d), (fr.STREAMS, s)):
        with open(path, "wb") as f:
            f.write(data)
    print(len(fr.load_designs()), "designs,", len(d), "bytes;", len(fr.load_streams()), "stream cases,", len(s), "bytes")
