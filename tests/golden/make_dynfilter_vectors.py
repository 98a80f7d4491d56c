"""Writes tests/golden/dynfilter_ref_rlc.npz, _bwc.npz, _lrx.npz and _streams.npz: what the reference's own DynamicFilters class
(oracle/_ref/dynfilter_ref: DynamicFilters.cpp compiled unmodified, see oracle/Makefile) does on a list of cases.  Data only:
settings, events, calls, shared input and gain rows, the reference's get_params(), the analog cascades it built for every sample (as
its transform was handed them) and its outputs.  Run where the reference tree exists, after the build:

    python tests/golden/make_dynfilter_vectors.py

Every case first runs through oracle/_ref/dynfilter_ref_san, the same program with the address and undefined-behaviour sanitizers (a
stand-alone host program); nothing is written unless that run is clean and gives the same bytes.  The per-sample transform and the
section arithmetic under the class are stand-ins (oracle/ref_overlay/filters); what the files pin is the class's own text: the
cascade builders of every type, the groups of 8 / 4 / 2 / 1, kf, the swap of the two frequencies and bClearMem.
tests/test_dynfilter_reference_host.py regenerates the files with build_bytes() and requires the committed bytes, so they are written
without time stamps.  The layout is tests/dynfilter_reference.py's, which reads them.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import dynfilter_reference as dr  # noqa: E402
from make_filter_vectors import npz_bytes, run_driver as _run  # noqa: E402

f32 = np.float32
DF_REF = os.path.join(ROOT, "oracle", "_ref", "dynfilter_ref")
DF_SAN = os.path.join(ROOT, "oracle", "_ref", "dynfilter_ref_san")
SR = 48000
TOL = 1e-5                                      # tests/conftest.py's TOL
SHORT = 40
NX = 4000


def modules():
    from oracle import dynamic_filters as df
    from oracle import filter_design as fd
    return df, fd


def types():
    """Every type that DynamicFilters builds cascades for; the RLC_ENVELOPE pair is left out (oracle/dynamic_filters.py says why)."""
    df, fd = modules()
    return [t for t in range(1, len(fd.FILTER_TYPES)) if df.cascade_count(t, 1) > 0]


def rows():
    """The shared rows: x, and gain = the 40 gains of the short cases (1.0, values below and above it, 1e-3), then a slow envelope
    between 0.3 and 3, then sample-to-sample changes."""
    rng = np.random.default_rng(20241020)
    x = rng.uniform(-0.5, 0.5, NX).astype(f32)
    short = np.concatenate([[1.0, 0.5, 2.0, 1e-3, 1.0, 0.25, 4.0, 16.0], np.exp(rng.uniform(np.log(0.05), np.log(16.0), SHORT - 8))])
    t = np.arange(3000) / float(SR)
    sweep = np.exp(np.log(3.0) * np.sin(2 * np.pi * 5.0 * t + 0.7))
    jumps = np.exp(rng.uniform(-1.0, 1.0, NX - SHORT - 3000))
    return x, np.concatenate([short, sweep, jumps]).astype(f32)


def family(name):
    return "bwc" if "_BWC_" in name else "lrx" if "_LRX_" in name else "rlc"


def case(name, filters, record, events, calls, at_x, at_gain, n):
    return dict(name=name, filters=filters, sample_rate=SR, record=record, events=events, calls=calls, at_x=at_x, at_gain=at_gain, n=n)


def setup(fid, fp, before=0):
    return [(before, dr.SET_PARAMS, fid, fp), (before, dr.SET_ACTIVE, fid, fp)]


def cases():
    """-> {file: [cases]}"""
    df, fd = modules()
    T = fd.T
    out = {k: [] for k in dr.FILES}
    for k, t in enumerate(types()):
        name = fd.FILTER_TYPES[t]
        for slope in (1, 2, 3):
            out[family(name)].append(case("%s slope %d" % (name, slope), 1, 1, setup(0, (t, slope, 1200.0, 5000.0, 1.0, 0.6)), [(0, 0, SHORT)],
                                          17 * k + slope, 0, SHORT))
        slope = 2 if df.cascade_count(t, 2) <= 16 else 1                # the rule of tests/test_dynfilter_gpu.py::test_every_type_matches_the_oracle
        out["streams"].append(case("stream %s" % name, 2, 0, setup(1, (t, slope, 1200.0, 5000.0, 1.0, 0.6)), [(1, 0, 257), (1, 257, 343)],
                                   31 * k, SHORT + 29 * k, 600))
    # six longer cases of 2148 samples through filter 0: 1, 2, 4, 8, 12 and 15 cascades, so every group size and every mix
    bell2 = (T["FLT_BT_RLC_BELL"], 2, 900.0, 900.0, 1.0, 0.4)
    long_ = [
        (1, (T["FLT_BT_RLC_NOTCH"], 1, 1500.0, 1500.0, 1.0, 0.5), (T["FLT_BT_RLC_NOTCH"], 1, 2500.0, 2500.0, 1.0, 0.5), (T["FLT_BT_RLC_BELL"], 1, 2500.0, 2500.0, 1.0, 0.5)),
        (2, (T["FLT_MT_RLC_BANDPASS"], 2, 800.0, 3000.0, 1.0, 0.3), (T["FLT_MT_RLC_BANDPASS"], 2, 4000.0, 600.0, 1.0, 0.3), None),
        (4, (T["FLT_BT_RLC_LOSHELF"], 4, 700.0, 700.0, 1.0, 0.2), (T["FLT_BT_RLC_LOSHELF"], 4, 700.0, 700.0, 1.0, 0.9), (T["FLT_BT_RLC_HISHELF"], 4, 700.0, 700.0, 1.0, 0.9)),
        (8, (T["FLT_BT_LRX_LOPASS"], 4, 2000.0, 2000.0, 1.0, 0.0), (T["FLT_BT_LRX_LOPASS"], 4, 1000.0, 1000.0, 1.0, 0.0), None),
        (12, (T["FLT_MT_BWC_BELL"], 6, 1800.0, 1800.0, 1.0, 0.5), (T["FLT_MT_BWC_BELL"], 6, 1800.0, 1800.0, 1.0, 1.5), (T["FLT_BT_BWC_BELL"], 6, 1800.0, 1800.0, 1.0, 1.5)),
        (15, (T["FLT_BT_RLC_BELL"], 15, 3000.0, 3000.0, 1.0, 0.7), (T["FLT_BT_RLC_BELL"], 15, 5000.0, 5000.0, 1.0, 0.7), None),
    ]
    for k, (nc, first, same_type, new_type) in enumerate(long_):
        assert df.cascade_count(first[0], first[1]) == nc
        ev = setup(0, first) + setup(1, bell2)
        if new_type is not None:
            # 1024 + 1024 + 100: the same type keeps the memory; a new type sets bClearMem, which clears the memory of ALL filters
            # (:215-219), filter 1's too; filter 2 was never made active: its call copies
            calls = [(0, 0, 1024), (1, 0, 300), (0, 1024, 1024), (1, 300, 300), (0, 2048, 100), (1, 600, 100), (2, 0, 64)]
            ev += [(2, dr.SET_PARAMS, 0, same_type), (4, dr.SET_PARAMS, 0, new_type)]
        else:
            # 2100 + 24 + 24: one call across the reference's BUF_SIZE (twice) and from one of the kernel's super-blocks of 2048 samples
            # into the next; the same type (a band type with freq2 < freq: swapped) keeps the memory; a new type for filter 1 clears
            # filter 0's memory as well
            calls = [(0, 0, 2100), (1, 0, 300), (0, 2100, 24), (1, 300, 100), (0, 2124, 24), (1, 400, 100), (2, 0, 64)]
            ev += [(2, dr.SET_PARAMS, 0, same_type), (4, dr.SET_PARAMS, 1, (T["FLT_BT_RLC_RESONANCE"], 2, 900.0, 900.0, 1.0, 0.4))]
        out["streams"].append(case("long, %d cascades" % nc, 3, 0, ev, calls, 200 * k, SHORT + 150 * k, 2148))
    return out


def run_both(cs):
    san = _run(DF_SAN, cs, case_bytes=dr.case_bytes)
    raw = _run(DF_REF, cs, case_bytes=dr.case_bytes)
    assert san == raw, "the sanitizer build computes something else"
    return dr.parse_results(raw, cs)


def run_reference():
    df, fd = modules()
    x, gain = rows()
    files = cases()
    for which, cs in files.items():
        for c in cs:
            c["x"], c["gain"] = x[c["at_x"]:c["at_x"] + c["n"]], gain[c["at_gain"]:c["at_gain"] + c["n"]]
            assert len(c["x"]) == c["n"] == len(c["gain"])
        for c, r in zip(cs, run_both(cs)):
            assert np.isfinite(r["out"]).all(), c["name"]
            c.update(r)
        for c in cs:
            if not c["name"].startswith("long"):
                continue
            # both events prove something: the call after the same-type set_params is clearly different with the memory cleared, and
            # the call of the OTHER filter after the new type clearly different without the all-filters clear
            keep, new, other = dr.long_boundaries(c)
            assert dr.margin(c, df, keep, clear_at=keep) > 100 * TOL, (c["name"], "keep")
            assert dr.margin(c, df, other, no_clear_at=new) > 100 * TOL, (c["name"], "clear")
    return files, x, gain


def build_bytes():
    """-> {file: bytes}"""
    files, x, gain = run_reference()
    out = {}
    for which, cs in files.items():
        used_x = max(c["at_x"] + c["n"] for c in cs)
        used_g = max(c["at_gain"] + c["n"] for c in cs)
        out[which] = npz_bytes(dr.arrays(cs, x[:used_x], gain[:used_g]))
        assert len(out[which]) < 400 * 1000, (which, len(out[which]))
    return out


if __name__ == "__main__":
    for which, data in build_bytes().items():
        with open(dr.FILES[which], "wb") as f:
            f.write(data)
        print(which, len(dr.load(which)), "cases,", len(data), "bytes")
