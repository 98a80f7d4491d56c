"""Writes tests/golden/sidechain_ref_vectors.npz: what the reference's own Sidechain class (oracle/_ref/sidechain_ref: its
Sidechain.cpp and RawRingBuffer.cpp compiled unmodified, see oracle/Makefile) computes on a list of cases.  Data only: settings,
calls, setter events, shared input rows, the reference's outputs and its state after every call.  Run where the reference tree
exists, after the build:

    python tests/golden/make_sidechain_vectors.py

Every case first runs through oracle/_ref/sidechain_ref_san, the same program with the address and undefined-behaviour
sanitizers (a stand-alone host program); nothing is written unless that run is clean and gives the same bytes.  The driver also
runs both preprocess() overloads on every sample; nothing is written unless the array stand-ins of oracle/ref_shim return the bits
of the class's scalar overload.  tests/test_sidechain_reference_host.py regenerates the file with build_bytes() and requires the
committed bytes, so it is written without time stamps.  The layout is tests/sidechain_reference.py's, which reads it.
"""
import io
import os
import subprocess
import sys
import tempfile
import zipfile
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import sidechain_reference as sr  # noqa: E402

f32 = np.float32
SC_REF = os.path.join(ROOT, "oracle", "_ref", "sidechain_ref")
SC_SAN = os.path.join(ROOT, "oracle", "_ref", "sidechain_ref_san")
OUT = os.path.join(HERE, "sidechain_ref_vectors.npz")
MAGIC = 0x53434844
RATE, MAX_MS = 48000, 10.0                      # a ring of 480 + 512 = 992 samples
PEAK, RMS, LPF, UNIFORM = range(4)
MIDDLE, SIDE, LEFT, RIGHT, AMIN, AMAX = range(6)
CUTS = [1, 511, 512, 513, 163]                  # heads 1, 512, 32 (wrapped once), 545, 708 of the ring of 992


def millis_to_samples(sr_, ms):
    return (f32(ms) * f32(0.001)) * f32(sr_)


def ms_of(samples, rate=RATE):
    """A time that millis_to_samples() turns into that many samples at the rate."""
    ms = float(f32((samples + 0.5) * 1000.0 / rate))
    assert int(millis_to_samples(rate, ms)) == samples and ms <= MAX_MS, (samples, rate)
    return ms


MS_MAX = float(f32(MAX_MS))                      # 480 samples at 48 kHz


def signals():
    """The shared input rows."""
    rng = np.random.default_rng(20240917)
    a = rng.uniform(-1.0, 1.0, 18084).astype(f32)
    b = rng.uniform(-1.0, 1.0, 2100).astype(f32)
    decay = np.zeros(300, f32)
    decay[0] = 1.0
    # equal magnitudes with either combination of signs, and zeros, beside row `a`: where AMIN and AMAX have to choose.  No
    # negative zero: the class's scalar text, (s < 0.0f) ? -s : s, keeps its sign, and whether dsp::abs1 / abs2 of lsp-dsp-lib do
    # is not pinned by anything in the reference tree (the bank gives +0)
    ties = b.copy()
    ties[::3] = a[:2100:3]
    ties[1::6] = -a[1:2100:6]
    a[40:42] = 0.0
    ties[40:42] = [0.0, 0.25]
    assert not any(np.any((r == 0) & np.signbit(r)) for r in (a, b, ties))
    return [a, b, decay, ties]


A, B, DECAY, TIES = range(4)


def ev(before, setter, a=0.0):
    assert setter in sr.EVENTS
    return (int(before), setter, f32(a))


def case(name, n, calls, mode, react_ms, inputs=1, source=MIDDLE, stereo=0, gain=1.0, in0=(A, 0), in1=(B, 0), events=(), null=(),
         single=False, rate=RATE):
    calls = [1] * n if single else [int(c) for c in calls]
    assert sum(calls) == n, name
    return dict(name=name, n=n, calls=calls, null=[int(i in null) for i in range(len(calls))], mode=mode, reactivity=f32(react_ms),
                inputs=inputs, source=source, stereo=stereo, gain=f32(gain), at0=in0, at1=in1 if inputs == 2 else (-1, 0),
                events=sorted(events, key=lambda e: e[0]), single=int(single), sample_rate=rate, max_reactivity=f32(MAX_MS))


def cases():
    out = []
    # the four modes x (one input, two inputs x both stereo modes x the six sources); AMIN / AMAX against the row of ties
    k = 0
    for mode in range(4):
        for inputs, stereo, source in [(1, 0, MIDDLE)] + [(2, st, s) for st in (0, 1) for s in range(6)]:
            second = (TIES, 0) if source in (AMIN, AMAX) or (stereo == 1 and source in (LEFT, RIGHT)) else (B, 7 * k)
            out.append(case("matrix mode %d inputs %d stereo %d source %d" % (mode, inputs, stereo, source), 300, [1, 255, 44], mode,
                            ms_of(37), inputs, source, stereo, (1.0, -1.5, 1.0, 0.75)[k % 4], (A, 0 if second[0] == TIES else 11 * k),
                            second))
            k += 1
    # (a negative gain makes UNIFORM's sums negative and its output the clamp's zero: the matrix above has that, the cases below
    # do not)
    # window lengths 1, 2, 457 and the maximum: set ahead of call 1 (a refresh at head 1), left alone by three setters that
    # return early ahead of call 3, changed again ahead of call 4 (a refresh at head 545: the window in one piece)
    for mode in (RMS, UNIFORM):
        for i, (win, ms) in enumerate(((1, ms_of(1)), (2, ms_of(2)), (457, ms_of(457)), (480, MS_MAX))):
            out.append(case("window %d mode %d" % (win, mode), 1700, CUTS, mode, ms_of(100), gain=((1.0, -1.5) if mode == RMS else (1.0, 0.75))[i % 2],
                            in0=(A, 500 * i + mode),
                            events=[ev(1, "set_reactivity", ms), ev(3, "set_reactivity", ms), ev(3, "set_reactivity", -1.0),
                                    ev(3, "set_reactivity", 10.5), ev(4, "set_reactivity", ms_of(100 + win % 200))]))
    # a refresh with the window wrapped: the reactivity changed at head 32
    for mode in (RMS, UNIFORM):
        out.append(case("refresh wrapped mode %d" % mode, 1700, CUTS, mode, ms_of(300), in0=(A, 3000 + mode),
                        events=[ev(3, "set_reactivity", ms_of(457))]))
    # set_mode: the same mode is a no-op, a new one zeroes the sum without a refresh
    out.append(case("mode RMS UNIFORM RMS", 1700, CUTS, RMS, ms_of(457), in0=(A, 4000),
                    events=[ev(2, "set_mode", UNIFORM), ev(3, "set_mode", UNIFORM), ev(4, "set_mode", RMS)]))
    out.append(case("mode PEAK RMS LPF", 1700, CUTS, PEAK, ms_of(200), in0=(A, 4100), gain=-1.5,
                    events=[ev(2, "set_mode", RMS), ev(4, "set_mode", LPF)]))
    out.append(case("mode LPF UNIFORM PEAK", 1700, CUTS, LPF, ms_of(50), in0=(A, 4200),
                    events=[ev(1, "set_mode", UNIFORM), ev(3, "set_mode", PEAK), ev(4, "set_mode", UNIFORM)]))
    # source, gain and stereo mode between calls; a stereo mode that changes clears, the same one does not
    out.append(case("source gain stereo", 1700, CUTS, RMS, ms_of(200), 2, LEFT, 0, 1.0, (A, 5000), (B, 3),
                    events=[ev(2, "set_source", AMAX), ev(2, "set_gain", 0.0), ev(3, "set_stereo_mode", 1), ev(3, "set_gain", -1.5),
                            ev(4, "set_stereo_mode", 1), ev(4, "set_source", SIDE)]))
    out.append(case("source gain stereo uniform", 1700, CUTS, UNIFORM, ms_of(457), 2, AMIN, 1, 0.75, (A, 5100), (TIES, 0),
                    events=[ev(1, "set_stereo_mode", 0), ev(2, "set_source", MIDDLE), ev(3, "set_gain", 1.0), ev(4, "set_stereo_mode", 0)]))
    # clear(), alone and together with a changed reactivity (the forced refresh is then cancelled by the zeroed counter)
    out.append(case("clear uniform", 1700, CUTS, UNIFORM, MS_MAX, in0=(A, 5200), events=[ev(3, "clear")]))
    out.append(case("clear and reactivity rms", 1700, CUTS, RMS, ms_of(457), in0=(A, 5300), gain=-1.5,
                    events=[ev(2, "clear"), ev(2, "set_reactivity", ms_of(300)), ev(4, "clear")]))
    # set_sample_rate to a higher rate: a new ring at position 0; the class also drops the mid-side flag there (Sidechain.cpp:91)
    out.append(case("sample rate midside", 1700, CUTS, RMS, ms_of(200), 2, LEFT, 1, 1.0, (A, 5400), (TIES, 0),
                    events=[ev(2, "set_sample_rate", 96000)]))
    out.append(case("sample rate uniform", 1700, CUTS, UNIFORM, MS_MAX, in0=(A, 5500), events=[ev(3, "set_sample_rate", 96000)]))
    # in == NULL: silence through gain, ring and detector
    out.append(case("null rms", 1700, CUTS, RMS, ms_of(100), in0=(A, 5600), null=(2,)))
    out.append(case("null lpf two inputs", 1700, CUTS, LPF, ms_of(100), 2, AMAX, 0, -1.5, (A, 5700), (B, 0), null=(0, 3)))
    out.append(case("gain zero uniform", 1700, CUTS, UNIFORM, ms_of(2), gain=0.0, in0=(A, 5800)))
    # a call that ends at the ring's end: push() leaves the position AT the capacity there (RawRingBuffer.cpp:118-122)
    out.append(case("head at the end", 1700, [1, 511, 480, 513, 195], UNIFORM, MS_MAX, in0=(A, 6500), events=[ev(3, "set_reactivity", ms_of(457))]))
    # LPF: a decay into the subnormals and down to zero (a window of one sample: tau = sqrt(1/2)), and a long window
    out.append(case("lpf decay", 300, [1, 150, 149], LPF, ms_of(1), in0=(DECAY, 0)))
    out.append(case("lpf window 480", 1700, CUTS, LPF, MS_MAX, in0=(A, 5900), gain=-1.5))
    # past 0x2000 samples without any event: the counted refresh at a call's start (8192 + 8192 + 700) and inside a call
    out.append(case("long rms", 17084, [8192, 8192, 700], RMS, MS_MAX, in0=(A, 0)))
    out.append(case("long uniform", 17084, [5000, 8193, 3891], UNIFORM, MS_MAX, in0=(A, 1000), gain=0.75))
    out.append(case("long rms two inputs", 17084, [8193, 8191, 700], RMS, ms_of(457), 2, SIDE, 0, 1.0, (A, 0), (A, 1000)))
    out.append(case("long peak", 17084, [8192, 8192, 700], PEAK, ms_of(100), in0=(A, 500)))
    # the single-sample overload beside the same samples as block calls of length 1
    out.append(case("single rms", 300, None, RMS, ms_of(37), in0=(A, 6000), single=True, events=[ev(150, "set_reactivity", ms_of(5))]))
    out.append(case("single uniform", 300, None, UNIFORM, ms_of(37), in0=(A, 6100), gain=0.75, single=True))
    out.append(case("single lpf", 300, None, LPF, ms_of(37), in0=(A, 6200), single=True))
    out.append(case("single peak two inputs", 300, None, PEAK, ms_of(37), 2, AMIN, 1, 1.0, (A, 6300), (TIES, 0), single=True))
    out.append(case("single rms long", 8300, None, RMS, ms_of(37), in0=(A, 7000), single=True))
    return out


def run_driver(exe, cs, timeout=300, raw=False):
    """Runs a driver over the cases under a time limit; its standard error must stay empty (a sanitizer writes there)."""
    with tempfile.TemporaryDirectory() as d:
        src, dst = os.path.join(d, "cases.bin"), os.path.join(d, "results.bin")
        with open(src, "wb") as f:
            f.write(sr.case_bytes(cs))
        p = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=timeout)
        if exe == SC_SAN and "LeakSanitizer has encountered a fatal error" in p.stderr:
            # the sanitizer twin's leak check needs ptrace, which a build machine may withhold: there, and only there, the run
            # is repeated for the bounds and the undefined arithmetic alone
            p = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=timeout,
                               env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
        if p.returncode != 0 or p.stderr.strip():
            raise RuntimeError("%s: exit status %d\n%s" % (exe, p.returncode, p.stderr[-4000:]))
        with open(dst, "rb") as f:
            data = f.read()
    return data if raw else sr.parse_results(data, cs)


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def run_reference():
    x = signals()
    cs = cases()
    for c in cs:
        c["in0"], c["in1"] = (x[r][o:o + c["n"]] if r >= 0 else None for r, o in (c["at0"], c["at1"]))
        assert all(v is None or (len(v) == c["n"] and np.isfinite(v).all()) for v in (c["in0"], c["in1"])), c["name"]
    san = run_driver(SC_SAN, cs, raw=True)
    raw = run_driver(SC_REF, cs, raw=True)
    assert san == raw, "the sanitizer build computes something else"
    res = sr.parse_results(raw, cs)
    places = 0
    for c, r in zip(cs, res):
        keep = np.repeat(np.array(c["null"]) == 0, c["calls"])
        # the array stand-ins against the class's own scalar preprocess(), on every sample
        assert np.array_equal(bits(r["pre_array"])[keep], bits(r["pre_scalar"])[keep]), c["name"]
        for call in ([len(c["calls"]) - 1] if c["single"] else range(len(c["calls"]))):         # the rows that are kept
            places |= int(r["state"][call, 8])
        # the recorded ring check sums are those of zlib
        assert int(r["state"][-1, 7]) == zlib.crc32(bits(r["ring"]).tobytes()), c["name"]
        c.update(r)
    for bit in (sr.P_RMS_WHOLE, sr.P_RMS_WRAPPED, sr.P_UNI_WHOLE, sr.P_UNI_WRAPPED, sr.P_SPLIT, sr.P_OTHER_REFRESH, sr.P_COUNTED,
                sr.P_AT_START, sr.P_HEAD_AT_END):
        assert places & bit, "no case goes through place %d" % bit
    lpf = sum(1 for c in cs if c["mode"] == LPF or any(e[1] == "set_mode" and int(e[2]) == LPF for e in c["events"]))
    assert 4 * lpf <= len(cs), (lpf, len(cs))
    return cs, x


def stored(v, n, points):
    """A row as it is stored: whole up to sr.WHOLE samples; else windows of sr.WINDOW samples around the points and a CRC-32 of
    every block of sr.BLOCK samples' bits."""
    if n <= sr.WHOLE:
        return v, np.zeros(0, np.uint32), np.zeros((0, sr.WINDOW), f32), np.zeros(0, np.uint32)
    starts = sorted({min(max(0, p - sr.WINDOW // 2), n - sr.WINDOW) for p in points})
    wins = np.stack([v[s:s + sr.WINDOW] for s in starts])
    crc = [zlib.crc32(bits(v[s:s + sr.BLOCK]).tobytes()) for s in range(0, n, sr.BLOCK)]
    return np.zeros(0, f32), np.array(starts, np.uint32), wins, np.array(crc, np.uint32)


def arrays(cs, x):
    a = {"names": np.array([c["name"] for c in cs])}
    for k in ("n", "inputs", "sample_rate", "mode", "source", "stereo", "single"):
        a[k] = np.array([c[k] for c in cs], np.uint32)
    for k in ("max_reactivity", "reactivity", "gain"):
        a[k] = np.array([c[k] for c in cs], f32)
    a["rows"] = np.array([[c["at0"][0], c["at0"][1], c["at1"][0], c["at1"][1]] for c in cs], np.int32)
    a["x"] = np.concatenate(x)
    a["x_len"] = np.array([len(r) for r in x], np.uint32)
    # a single-sample case is n calls of one sample: its calls are not listed, and only the last call's state is kept
    a["ncalls"] = np.array([0 if c["single"] else len(c["calls"]) for c in cs], np.uint32)
    a["calls"] = np.array([v for c in cs if not c["single"] for v in c["calls"]], np.uint32)
    a["null"] = np.array([v for c in cs if not c["single"] for v in c["null"]], np.uint8)
    a["state"] = np.concatenate([c["state"][-1:] if c["single"] else c["state"] for c in cs]).astype(np.uint32)
    a["nevents"] = np.array([len(c["events"]) for c in cs], np.uint32)
    a["events"] = np.array([[e[0], sr.EVENTS.index(e[1]), int(bits(e[2])[0])] for c in cs for e in c["events"]], np.uint32).reshape(-1, 3)
    a["ring"] = np.concatenate([c["ring"] for c in cs])
    a["nring"] = np.array([len(c["ring"]) for c in cs], np.uint32)
    for key in ("out", "single"):
        parts = [[], [], [], []]
        counts = []
        for c in cs:
            if key == "single" and not c["single"]:
                continue
            cuts = np.cumsum(c["calls"])[:-1] if not c["single"] else []
            points = [0, c["n"]] + [int(v) for v in cuts] + list(range(0x2000, c["n"], 0x2000))
            got = stored(c["out" if key == "out" else "single_out"], c["n"], points)
            for p, g in zip(parts, got):
                p.append(g)
            counts.append([len(g) for g in got])
        a[key + "_whole"] = np.concatenate(parts[0]).astype(f32)
        a[key + "_starts"] = np.concatenate(parts[1]).astype(np.uint32)
        a[key + "_windows"] = np.concatenate(parts[2]).astype(f32)
        a[key + "_crc"] = np.concatenate(parts[3]).astype(np.uint32)
        a[key + "_counts"] = np.array(counts, np.uint32)
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
    cs, x = run_reference()
    data = npz_bytes(arrays(cs, x))
    assert len(data) < 400 * 1000, len(data)
    return data


if __name__ == "__main__":
    data = build_bytes()
    with open(OUT, "wb") as f:
        f.write(data)
    got = sr.load()
    print(len(got), "cases,", len(data), "bytes,", sum(1 for c in got if c["lpf"]), "with LPF")
