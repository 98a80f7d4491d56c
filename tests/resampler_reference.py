"""Reads tests/golden/truepeak_ref_vectors.npz (written by tests/golden/make_resampler_vectors.py from the reference's own
compiled TruePeakMeter class), and writes and reads the files of oracle/truepeak_driver.cpp.  Never reads the reference tree or
oracle/_ref/.

A case: name, sample_rate, calls [(length, kind)], events [(ahead of which call, setter, argument)], x (a row of the shared
signals), out (the true peaks of the whole stream, float32 [n]), state uint32 [calls, 7] (STATE)."""
import io
import os

import numpy as np

f32 = np.float32
PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "truepeak_ref_vectors.npz")
MAGIC = 0x5450454B
KINDS = ("process", "in_place", "process_max")
EVENTS = ("set_sample_rate", "clear")
STATE = ("latency", "returned", "times", "head", "compactions", "from", "update")
FACTORS = (2, 3, 4, 6, 8)
BUFFER_SIZE = 0x1000


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def scatter_taps(table):
    """The [times][20] table of mi_truepeak_coefficients as the taps of one scatter loop: phase k, tap t at [times * t + k]."""
    return np.ascontiguousarray(np.asarray(table, f32).T).reshape(-1)


def case_bytes(cases, tables):
    """The case file of oracle/truepeak_driver.cpp (its head comment has the layout); tables: {times: [times][20]}."""
    b = io.BytesIO()
    u32 = lambda *v: b.write(np.array(v, np.uint32).tobytes())
    u32(MAGIC, len(tables))
    for times in sorted(tables):
        taps = scatter_taps(tables[times])
        u32(times, len(taps))
        b.write(taps.tobytes())
    u32(len(cases))
    for c in cases:
        u32(c["sample_rate"], len(c["calls"]))
        for n, kind in c["calls"]:
            u32(n, KINDS.index(kind))
        u32(len(c["events"]))
        for before, setter, a in c["events"]:
            u32(before, EVENTS.index(setter), a)
        u32(len(c["x"]))
        b.write(np.ascontiguousarray(c["x"], f32).tobytes())
    return b.getvalue()


def parse_results(raw, cases):
    """What a driver wrote: per case a dict of state uint32 [calls, 7], out and own float32 [n]."""
    w = np.frombuffer(raw, np.uint32)
    pos, out = 0, []

    def take(n):
        nonlocal pos
        v = w[pos:pos + n]
        assert len(v) == n, "short result file"
        pos += n
        return v

    for c in cases:
        ncalls = int(take(1)[0])
        assert ncalls == len(c["calls"])
        r = {"state": take(7 * ncalls).reshape(ncalls, 7).copy()}
        for key in ("out", "own"):
            r[key] = take(int(take(1)[0])).view(f32).copy()
            assert len(r[key]) == len(c["x"])
        out.append(r)
    assert pos == len(w), "result file longer than its cases"
    return out


def load(path=PATH):
    z = np.load(path)
    cases = []
    pc = pe = po = 0
    for i, name in enumerate(z["names"]):
        n, nc, ne = int(z["n"][i]), int(z["ncalls"][i]), int(z["nevents"][i])
        row, off = (int(v) for v in z["rows"][i])
        cases.append(dict(name=str(name), sample_rate=int(z["sample_rate"][i]), x=z["x"][row, off:off + n],
                          calls=[(int(m), KINDS[int(k)]) for m, k in z["calls"][pc:pc + nc]],
                          events=[(int(b), EVENTS[int(k)], int(a)) for b, k, a in z["events"][pe:pe + ne]],
                          state=z["state"][pc:pc + nc], out=z["out"][po:po + n]))
        pc, pe, po = pc + nc, pe + ne, po + n
    return cases


def column(case, name):
    v = case["state"][:, STATE.index(name)]
    return v.view(f32) if name == "returned" else v


def call_maxima(case):
    """Per call the largest recorded true peak of its samples: what process() wrote for the block."""
    out, pos = [], 0
    for n, _ in case["calls"]:
        out.append(case["out"][pos:pos + n].max() if n else f32(0.0))
        pos += n
    return np.array(out, f32)


# ---- Oversampler ------------------------------------------------------------------------------------------------------------
OS_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "oversampler_ref_vectors.npz")
OS_MAGIC = 0x4F565253
OPS = ("set_mode", "set_sample_rate", "set_filtering", "update_settings", "upsample", "downsample", "process")
OS_STATE = ("oversampling", "latency", "modified", "head", "calls")
FILTER_CALL = ("clear", "rate", "type", "slope", "freq", "freq2", "gain", "quality")
OS_UP_BUFFER_SIZE = 12 * 1024
RSV_SAMPLES = 1024                              # the stand-in's LSP_DSP_RESAMPLING_RSV_SAMPLES (oracle/ref_overlay/oversampler)


def os_case_bytes(cases, tables):
    """The case file of oracle/oversampler_driver.cpp (its head comment has the layout); tables: {mode: [N][2a]}."""
    b = io.BytesIO()
    u32 = lambda *v: b.write(np.array(v, np.uint32).tobytes())
    u32(OS_MAGIC, len(tables))
    for mode in sorted(tables):
        taps = scatter_taps(tables[mode])
        u32(mode, len(taps))
        b.write(taps.tobytes())
    u32(len(cases))
    for c in cases:
        u32(len(c["steps"]))
        for op, a in c["steps"]:
            u32(OPS.index(op), a)
        u32(len(c["x"]))
        b.write(np.ascontiguousarray(c["x"], f32).tobytes())
    return b.getvalue()


def os_parse_results(raw, cases):
    """What a driver wrote: per case a dict of state uint32 [steps, 5], log uint32 [calls, 8], up and down float32."""
    w = np.frombuffer(raw, np.uint32)
    pos, out = 0, []

    def take(n):
        nonlocal pos
        v = w[pos:pos + n]
        assert len(v) == n, "short result file"
        pos += n
        return v

    for c in cases:
        state, log = [], []
        for _ in c["steps"]:
            state.append(take(5).copy())
            for _ in range(int(state[-1][4])):
                log.append(take(8).copy())
        r = {"state": np.array(state, np.uint32).reshape(-1, 5), "log": np.array(log, np.uint32).reshape(-1, 8)}
        for key in ("up", "down"):
            r[key] = take(int(take(1)[0])).view(f32).copy()
        out.append(r)
    assert pos == len(w), "result file longer than its cases"
    return out


def os_load(path=OS_PATH):
    """The Oversampler's cases: name, steps [(op, argument)], x, state [steps, 5] (OS_STATE), log [calls, 8] (FILTER_CALL; freq ..
    quality as float32 bits), up and down (sidechain_reference.Stored)."""
    from sidechain_reference import Stored
    z = np.load(path)
    cases = []
    ps = pl = 0
    pos = {"up": [0, 0, 0], "down": [0, 0, 0]}
    for i, name in enumerate(z["names"]):
        ns = int(z["nsteps"][i])
        c = dict(name=str(name), steps=[(OPS[int(o)], int(a)) for o, a in z["steps"][ps:ps + ns]], x=z["x"][:int(z["n"][i])],
                 state=z["state"][ps:ps + ns])
        nl = int(c["state"][:, 4].sum())
        c["log"] = z["log"][pl:pl + nl]
        ps, pl = ps + ns, pl + nl
        for key in ("up", "down"):
            n, nw, nst, ncrc = (int(v) for v in z[key + "_counts"][i])
            p = pos[key]
            c[key] = Stored(n, z[key + "_whole"][p[0]:p[0] + nw], z[key + "_starts"][p[1]:p[1] + nst], z[key + "_windows"][p[1]:p[1] + nst],
                            z[key + "_crc"][p[2]:p[2] + ncrc])
            p[0], p[1], p[2] = p[0] + nw, p[1] + nst, p[2] + ncrc
        cases.append(c)
    return cases


def os_calls(case, step):
    """The filter calls inside a step: [(is clear, rate, (type, slope, freq, freq2, gain, quality) with the floats as bits)]."""
    first = int(case["state"][:step, 4].sum())
    return [(bool(r[0]), int(r[1]), tuple(int(v) for v in r[2:])) for r in case["log"][first:first + int(case["state"][step, 4])]]
