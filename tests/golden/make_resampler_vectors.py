"""Writes tests/golden/truepeak_ref_vectors.npz: what the reference's own TruePeakMeter class (oracle/_ref/truepeak_ref: its
TruePeakMeter.cpp compiled unmodified, see oracle/Makefile) computes on a list of cases.  Data only: rates, calls, events, shared
input rows, the reference's outputs and its counters after every call.  Run where the reference tree exists, after the build:

    python tests/golden/make_resampler_vectors.py

The resampling functions of lsp-dsp-lib are not in the reference tree.  The stand-in (oracle/ref_overlay/resampler) is one scatter
loop whose taps this script takes from mi_truepeak_coefficients, a host function held to the float64 formula by its own tests: the
tap values are UNPINNED, what is pinned is everything the class does around them.  Every case first runs through
oracle/_ref/truepeak_ref_san (address and undefined-behaviour sanitizers, a stand-alone host program); nothing is written unless that
run is clean and gives the same bytes.  tests/test_resampler_reference_host.py regenerates the file with build_bytes() and requires
the committed bytes, so it is written without time stamps.  The Oversampler's file is made by the second half of this script."""
import importlib
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

import resampler_reference as rr  # noqa: E402

f32 = np.float32
TP_REF = os.path.join(ROOT, "oracle", "_ref", "truepeak_ref")
TP_SAN = os.path.join(ROOT, "oracle", "_ref", "truepeak_ref_san")
OUT = os.path.join(HERE, "truepeak_ref_vectors.npz")
N = 5000                                        # two compactions of the buffer of 0x1000 even at 2x
RATES = {8: 22050, 6: 32000, 4: 44100, 3: 64000, 2: 96000, 0: 192000}
CUTS = (1, 511, 512, 513, 2048, 1415)           # a call straddles the compaction at every factor
KINDS = ("process", "in_place", "process", "process_max", "in_place", "process_max")
NOISE, IMPULSES, SINE, ZEROS = range(4)


def tables():
    mi = importlib.import_module("lsp-dsp-units_amd")
    return {t: mi.TruePeakBank.coefficients(t) for t in rr.FACTORS}


def signals():
    rng = np.random.default_rng(1770)
    noise = rng.uniform(-1.0, 1.0, N).astype(f32)
    # an impulse train at the compaction points: the inputs on either side of every place where a buffer fills, for every factor
    imp = np.zeros(N, f32)
    for t in rr.FACTORS:
        per = rr.BUFFER_SIZE // t
        for k in range(1, N // per + 1):
            for d in (-11, -1, 0, 1):
                if 0 <= k * per + d < N:
                    imp[k * per + d] = (1.0, -0.5, 0.75, -1.0)[(k + d) % 4]
    # full scale at fs / 4 with 45 degrees of phase: every sample +-sqrt(1/2), the true peak between them 1
    sine = np.sin(2 * np.pi * (np.arange(N) / 4.0 + 0.125)).astype(f32)
    # signed zeros among sparse values
    zeros = np.where(np.arange(N) % 2 == 0, f32(0.0), f32(-0.0)).astype(f32)
    zeros[::97] = noise[::97]
    return np.stack([noise, imp, sine, zeros])


def case(name, rate, row, events=(), calls=None, off=0, n=N):
    calls = list(zip(CUTS, KINDS)) if calls is None else calls
    assert sum(m for m, _ in calls) == n
    return dict(name=name, sample_rate=rate, row=row, off=off, calls=calls, events=sorted(events, key=lambda e: e[0]))


def cases():
    out = []
    for times, rate in RATES.items():
        for row, what in enumerate(("noise", "impulses", "sine", "zeros")):
            out.append(case("%dx %s" % (times, what), rate, row))
    # a rate change that keeps the factor (no clear), one that changes it (clear), back again, and the same rate set again
    out.append(case("rate keeps factor", 44100, NOISE, [(2, "set_sample_rate", 48000), (4, "set_sample_rate", 48000)]))
    out.append(case("rate changes factor", 44100, NOISE, [(2, "set_sample_rate", 96000), (4, "set_sample_rate", 44100)]))
    out.append(case("rate to none and back", 48000, SINE, [(1, "set_sample_rate", 192000), (3, "set_sample_rate", 22050)]))
    # clear() in mid-stream, with pending sums in the buffer
    out.append(case("clear 3x", 64000, NOISE, [(3, "clear", 0)]))
    out.append(case("clear 8x", 22050, IMPULSES, [(2, "clear", 0), (5, "clear", 0)]))
    return out


def run_driver(exe, cs, tabs, timeout=300):
    """Runs a driver over the cases under a time limit; its standard error must stay empty (a sanitizer writes there)."""
    with tempfile.TemporaryDirectory() as d:
        src, dst = os.path.join(d, "cases.bin"), os.path.join(d, "results.bin")
        with open(src, "wb") as f:
            f.write(rr.case_bytes(cs, tabs))
        p = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=timeout)
        if exe == TP_SAN and "LeakSanitizer has encountered a fatal error" in p.stderr:
            # the sanitizer twin's leak check needs ptrace, which a build machine may withhold: there, and only there, the run
            # is repeated for the bounds and the undefined arithmetic alone
            p = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=timeout,
                               env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
        if p.returncode != 0 or p.stderr.strip():
            raise RuntimeError("%s: exit status %d\n%s" % (exe, p.returncode, p.stderr[-4000:]))
        with open(dst, "rb") as f:
            return f.read()


def run_reference():
    x, cs, tabs = signals(), cases(), tables()
    for c in cs:
        c["x"] = x[c["row"], c["off"]:c["off"] + sum(m for m, _ in c["calls"])]
    san = run_driver(TP_SAN, cs, tabs)
    raw = run_driver(TP_REF, cs, tabs)
    assert san == raw, "the sanitizer build computes something else"
    for c, r in zip(cs, rr.parse_results(raw, cs)):
        c.update(r)
        # what the first object wrote with process(), out of place and in place, is the whole stream's
        pos = 0
        for m, kind in c["calls"]:
            if kind != "process_max":
                assert np.array_equal(rr.bits(c["own"][pos:pos + m]), rr.bits(c["out"][pos:pos + m])), c["name"]
            pos += m
    return cs, x


def arrays(cs, x):
    a = {"names": np.array([c["name"] for c in cs]), "x": x}
    a["sample_rate"] = np.array([c["sample_rate"] for c in cs], np.uint32)
    a["n"] = np.array([len(c["x"]) for c in cs], np.uint32)
    a["rows"] = np.array([[c["row"], c["off"]] for c in cs], np.uint32)
    a["ncalls"] = np.array([len(c["calls"]) for c in cs], np.uint32)
    a["calls"] = np.array([[m, rr.KINDS.index(k)] for c in cs for m, k in c["calls"]], np.uint32)
    a["nevents"] = np.array([len(c["events"]) for c in cs], np.uint32)
    a["events"] = np.array([[b, rr.EVENTS.index(s), v] for c in cs for b, s, v in c["events"]], np.uint32).reshape(-1, 3)
    a["state"] = np.concatenate([c["state"] for c in cs]).astype(np.uint32)
    a["out"] = np.concatenate([c["out"] for c in cs]).astype(f32)
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
    data = npz_bytes(arrays(*run_reference()))
    assert len(data) < 400 * 1000, len(data)
    return data




# ---- Oversampler -> oversampler_ref_vectors.npz ------------------------------------------------------------------------------
# What the reference's own Oversampler class (oracle/_ref/oversampler_ref: Oversampler.cpp compiled unmodified, with the stand-in
# resamplers fed mi_oversampler_coefficients' tables and a RECORDING stand-in Filter) computes and asks of its filter.
import zlib  # noqa: E402

import sidechain_reference as sr  # noqa: E402

OS_REF = os.path.join(ROOT, "oracle", "_ref", "oversampler_ref")
OS_SAN = os.path.join(ROOT, "oracle", "_ref", "oversampler_ref_san")
OS_OUT = os.path.join(HERE, "oversampler_ref_vectors.npz")
OS_N = 13000
TIMES = (2, 3, 4, 6, 8)
MODE = {"%dX%s" % (n, k): 1 + 6 * g + j for g, n in enumerate(TIMES) for j, k in enumerate(("2", "3", "4", "12BIT", "16BIT", "24BIT"))}


def os_tables():
    mi = importlib.import_module("lsp-dsp-units_amd")
    return {m: mi.OversamplerBank.coefficients(m) for m in range(1, 31)}


def os_cases():
    out = []
    setup = lambda mode, rate, filt: [("set_mode", mode), ("set_sample_rate", rate), ("set_filtering", filt), ("update_settings", 0)]
    # all 30 modes: 26000 oversampled samples (two compactions of the buffer of 12288), cut at 1, 61, 62, 63 and at the buffer's own
    # length in inputs; every upsample followed by the downsample of what it wrote, without filter
    for name, mode in MODE.items():
        times = TIMES[(mode - 1) // 6]
        total = -(-2 * OS_N // times)
        cuts = [1, 61, 62, 63, rr.OS_UP_BUFFER_SIZE // times]
        cuts.append(total - sum(cuts))
        steps = setup(mode, 48000, 0)
        for m in cuts:
            steps += [("upsample", m), ("downsample", m)]
        out.append(dict(name="mode " + name, steps=steps))
    out.append(dict(name="mode NONE", steps=setup(0, 48000, 0) + [("upsample", 700), ("downsample", 700), ("upsample", 1), ("downsample", 1)]))
    # what the filter is asked and when it is cleared: mode change, rate change, same-value setters, set_filtering, the rates 44100,
    # 48000 and 96000, and 20000, where 0.42 sr is the smaller limit; 100 samples in between show what was cleared
    up = [("upsample", 100), ("downsample", 100)]
    out.append(dict(name="filter requests", steps=[
        ("set_sample_rate", 44100), ("update_settings", 0), ("set_mode", MODE["4X16BIT"]), ("update_settings", 0)] + up + [
        ("set_mode", MODE["4X16BIT"]), ("set_sample_rate", 44100), ("set_filtering", 1), ("update_settings", 0)] + up + [
        ("set_sample_rate", 48000), ("update_settings", 0)] + up + [
        ("set_filtering", 0), ("update_settings", 0)] + up + [("set_filtering", 0), ("update_settings", 0)] + up + [
        ("set_sample_rate", 96000), ("set_mode", MODE["8X2"]), ("update_settings", 0)] + up + [
        ("set_sample_rate", 20000), ("update_settings", 0)] + up + [("set_mode", 0), ("update_settings", 0)] + up))
    # process() with the callback, the recording filter on (it copies, so filtering equals the unfiltered path): the counts stand
    # around OS_UP_BUFFER_SIZE / 8
    out.append(dict(name="process 8X16BIT", steps=setup(MODE["8X16BIT"], 48000, 1) + [("process", m) for m in (1, 1535, 1536, 1537, 4097)]))
    out.append(dict(name="process 3X4", steps=setup(MODE["3X4"], 44100, 1) + [("process", m) for m in (1, 4095, 4096, 4097, 500)]))
    out.append(dict(name="process 2X24BIT", steps=setup(MODE["2X24BIT"], 96000, 1) + [("process", m) for m in (61, 6144, 6145)]))
    out.append(dict(name="process NONE", steps=setup(0, 48000, 1) + [("process", 300)]))
    return out


def os_run_driver(exe, cs, tabs, timeout=600):
    with tempfile.TemporaryDirectory() as d:
        src, dst = os.path.join(d, "cases.bin"), os.path.join(d, "results.bin")
        with open(src, "wb") as f:
            f.write(rr.os_case_bytes(cs, tabs))
        p = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=timeout)
        if exe == OS_SAN and "LeakSanitizer has encountered a fatal error" in p.stderr:
            # as in run_driver(): only the leak check is given up, and only where ptrace is withheld
            p = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=timeout,
                               env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
        if p.returncode != 0 or p.stderr.strip():
            raise RuntimeError("%s: exit status %d\n%s" % (exe, p.returncode, p.stderr[-4000:]))
        with open(dst, "rb") as f:
            return f.read()


def os_run_reference():
    x = np.random.default_rng(30).uniform(-1.0, 1.0, OS_N).astype(f32)
    cs, tabs = os_cases(), os_tables()
    # no mode's pending sums reach past the stand-in's RSV_SAMPLES: the tail a compaction carries holds all of them
    for mode, h in tabs.items():
        assert h.size - h.shape[0] <= rr.RSV_SAMPLES, (mode, h.shape)
    for c in cs:
        c["x"] = x[:sum(a for op, a in c["steps"] if op in ("upsample", "process"))]
    san = os_run_driver(OS_SAN, cs, tabs)
    raw = os_run_driver(OS_REF, cs, tabs)
    assert san == raw, "the sanitizer build computes something else"
    for c, r in zip(cs, rr.os_parse_results(raw, cs)):
        c.update(r)
    return cs, x


def os_stored(v, points):
    n = len(v)
    if n <= sr.WHOLE:
        return v, np.zeros(0, np.uint32), np.zeros((0, sr.WINDOW), f32), np.zeros(0, np.uint32)
    starts = sorted({min(max(0, p - sr.WINDOW // 2), n - sr.WINDOW) for p in points})
    wins = np.stack([v[s:s + sr.WINDOW] for s in starts])
    crc = [zlib.crc32(rr.bits(v[s:s + sr.BLOCK]).tobytes()) for s in range(0, n, sr.BLOCK)]
    return np.zeros(0, f32), np.array(starts, np.uint32), wins, np.array(crc, np.uint32)


def os_arrays(cs, x):
    a = {"names": np.array([c["name"] for c in cs]), "x": x, "n": np.array([len(c["x"]) for c in cs], np.uint32)}
    a["nsteps"] = np.array([len(c["steps"]) for c in cs], np.uint32)
    a["steps"] = np.array([[rr.OPS.index(op), v] for c in cs for op, v in c["steps"]], np.uint32)
    a["state"] = np.concatenate([c["state"] for c in cs]).astype(np.uint32)
    a["log"] = np.concatenate([c["log"] for c in cs]).astype(np.uint32)
    for key in ("up", "down"):
        parts, counts = [[], [], [], []], []
        for c in cs:
            # windows at every call's end in this stream and at the multiples of the up-buffer's length
            times, ends, pos = 1, [], 0
            for (op, v), st in zip(c["steps"], c["state"]):
                times = int(st[0])
                if (key == "up" and op == "upsample") or (key == "down" and op in ("downsample", "process")):
                    pos += v * (times if key == "up" else 1)
                    ends.append(pos)
            points = [0, len(c[key])] + ends + list(range(rr.OS_UP_BUFFER_SIZE // (times if key == "down" else 1), len(c[key]),
                                                          rr.OS_UP_BUFFER_SIZE // (times if key == "down" else 1)))
            got = os_stored(c[key], points)
            for p, g in zip(parts, got):
                p.append(g)
            counts.append([len(c[key])] + [len(g) for g in got[:2]] + [len(got[3])])
        a[key + "_whole"] = np.concatenate(parts[0]).astype(f32)
        a[key + "_starts"] = np.concatenate(parts[1]).astype(np.uint32)
        a[key + "_windows"] = np.concatenate(parts[2]).astype(f32)
        a[key + "_crc"] = np.concatenate(parts[3]).astype(np.uint32)
        a[key + "_counts"] = np.array(counts, np.uint32)
    return a


def os_build_bytes():
    data = npz_bytes(os_arrays(*os_run_reference()))
    assert len(data) < 400 * 1000, len(data)
    return data


if __name__ == "__main__":
    for path, build, load in ((OUT, build_bytes, rr.load), (OS_OUT, os_build_bytes, rr.os_load)):
        data = build()
        with open(path, "wb") as f:
            f.write(data)
        print(os.path.basename(path), len(load()), "cases,", len(data), "bytes")
