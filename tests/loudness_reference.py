"""The layout of tests/golden/loudness_ref_vectors.npz and ilufs_ref_vectors.npz (written by tests/golden/make_loudness_vectors.py
from the reference's own LoudnessMeter and ILUFSMeter classes), the protocol of oracle/loudness_driver.cpp, and the replay of a
recorded case on the restatements of oracle/loudness.py and oracle/ilufs.py.  Data only; nothing here reads the reference tree.

A case is a list of steps in the order the driver applies them: setters, bind() and process() calls.  Inputs are not stored: a row is
a list of segments (length, kind, amplitude, seed) and rows() makes the samples again, from a counter-based generator written out
here so that no library's random stream is relied on.  Outputs: an ILUFSMeter's is constant between gating blocks and is stored as its
steps; a LoudnessMeter's rows are stored at sample_index(): every sample around a call's start and end, around every event and every
4096th sample, and a thinned grid elsewhere, plus a CRC-32 of every call's whole rows, which holds the restatement to all of them."""
import os
import struct
import zlib

import numpy as np

f32 = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
FILES = {0: os.path.join(HERE, "golden", "loudness_ref_vectors.npz"), 1: os.path.join(HERE, "golden", "ilufs_ref_vectors.npz")}
MAGIC = 0x4C444E53
LOUDNESS, ILUFS = 0, 1
OPS = ["process", "bind", "set_designation", "set_link", "set_active", "set_weighting", "set_period", "clear", "update_settings",
       "set_sample_rate"]
OP = {name: i for i, name in enumerate(OPS)}
PF_NULL, PF_GAIN, PF_KEEP = 1, 2, 4
BF_IN, BF_OUT = 1, 2
P_START_WHOLE, P_START_WRAPPED, P_COUNTED_WHOLE, P_COUNTED_WRAPPED, P_RING_WRAPPED = 1, 2, 4, 8, 16
SENTINEL = f32(-77.0)
SLACK = 0x4000
NOISE, CONST = 0, 1
WINDOW, GRID = 64, 5
L_STATE = ["period", "size", "head", "refresh", "items", "places"]              # then fMS per channel
I_STATE = ["block_size", "block_offset", "block_part", "ms_size", "ms_int", "ms_count", "ms_head", "flags"]   # then vBlock, vLoudness
DEFAULT_GAIN = f32(0.923527857225)              # bs::DBFS_TO_LUFS_SHIFT_GAIN


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def fbits(v):
    return int(bits(f32(v)).reshape(-1)[0])


def from_bits(v):
    return np.array([v], np.uint32).view(f32)[0]


def crc(a):
    return zlib.crc32(bits(a).tobytes())


def noise(seed, n):
    """n values in [-1, 1): splitmix64 of the sample's index, the top 24 bits."""
    with np.errstate(over="ignore"):
        z = np.arange(n, dtype=np.uint64) + np.uint64(seed) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return ((z >> np.uint64(40)).astype(np.float64) / 2.0 ** 23 - 1.0).astype(f32)


def rows(c):
    """The case's input rows [channels][n]."""
    x = np.zeros((c["channels"], c["n"]), f32)
    for ch, segs in enumerate(c["segments"]):
        at = 0
        for length, kind, amp, seed in segs:
            x[ch, at:at + length] = (noise(seed, length) * f32(amp)).astype(f32) if kind == NOISE else f32(amp)
            at += length
        assert at == c["n"], (c["name"], ch, at)
    return x


def walk(c):
    """The process() calls of a case as the driver makes them -> per call a dict: step, pos, len, flags, a, in_at[ch] (where the
    channel's input starts in its row, None: no input), have[ch] (the call writes the channel's output), active[ch]."""
    K = c["channels"]
    has_in, has_out, active = [True] * K, [True] * K, [True] * K
    in_at, pos, calls = [0] * K, 0, []
    for si, (op, ch, a, length, flags) in enumerate(c["steps"]):
        if op == OP["process"]:
            if not flags & PF_KEEP:
                in_at = [pos] * K
            calls.append(dict(step=si, pos=pos, len=length, flags=flags, a=f32(a), in_at=[in_at[k] if has_in[k] else None for k in range(K)],
                              have=[bool(has_out[k] and has_in[k] and active[k]) for k in range(K)], active=list(active)))
            pos += length
        elif op == OP["bind"]:
            has_in[ch], has_out[ch] = bool(flags & BF_IN), bool(flags & BF_OUT) and c["kind"] == LOUDNESS
            in_at[ch] = pos
        elif op == OP["set_active"]:
            active[ch] = bool(a != 0)
    assert pos == c["n"], c["name"]
    return calls


def call_input(c, x, call):
    """[channels][len] as the call reads it (zeros where a channel has no input: it is left out anyway)."""
    xp = np.concatenate([x, np.zeros((c["channels"], SLACK), f32)], axis=1)
    return np.stack([xp[k, at:at + call["len"]] if at is not None else np.zeros(call["len"], f32) for k, at in enumerate(call["in_at"])])


def sample_index(c):
    """The samples of a LoudnessMeter case whose outputs are stored."""
    n = c["n"]
    keep = np.zeros(n, bool)
    keep[::GRID] = True
    points = list(range(0, n, 4096))
    for call in walk(c):
        points += [call["pos"], call["pos"] + call["len"]]
    for p in points:
        keep[max(0, p - WINDOW):min(n, p + WINDOW)] = True
    return np.flatnonzero(keep)


def case_bytes(cases):
    out = [struct.pack("<II", MAGIC, len(cases))]
    for c in cases:
        x = rows(c)
        out.append(struct.pack("<IIIIII", c["kind"], c["channels"], fbits(c["a"]), fbits(c["b"]), c["sample_rate"], c["n"]))
        out.append(np.ascontiguousarray(x, f32).tobytes())
        out.append(struct.pack("<I", len(c["steps"])))
        for op, ch, a, length, flags in c["steps"]:
            out.append(struct.pack("<IIIII", op, ch, fbits(a), length, flags))
    return b"".join(out)


def parse_results(data, cases, reference=True):
    """-> per case: steps [nsteps][3] (needs_update, latency, loudness bits) and per call: out, ch_out (None where not written),
    getters, state words."""
    at = 0

    def words(count, dtype=np.uint32):
        nonlocal at
        v = np.frombuffer(data, dtype, count, at)
        at += 4 * count
        return v

    res = []
    for c in cases:
        K = c["channels"]
        steps, calls = [], []
        for op, ch, a, length, flags in c["steps"]:
            steps.append(words(3).copy())
            if op != OP["process"]:
                continue
            n = int(words(1)[0])
            assert n == length, (c["name"], n, length)
            r = dict(out=words(n, f32).copy(), ch_out=[None] * K)
            if c["kind"] == LOUDNESS:
                for k in range(K):
                    if words(1)[0]:
                        r["ch_out"][k] = words(n, f32).copy()
            g = words(3 * K).reshape(K, 3)
            r["designation"], r["link"], r["active"] = g[:, 0].copy(), g[:, 1].copy(), g[:, 2].copy()
            r["weighting"], r["period"], r["sample_rate"] = (int(v) for v in words(3))
            ns = int(words(1)[0])
            assert (ns > 0) == reference, (c["name"], ns)
            r["state"] = words(ns).copy()
            calls.append(r)
        res.append(dict(steps=np.array(steps, np.uint32).reshape(-1, 3), calls=calls))
    assert at == len(data), (at, len(data))
    return res


# ---- the stored files ---------------------------------------------------------------------------------------------------------
def steps_of(out):
    """A row that is constant between a few points -> (positions, values): the row's first sample and every sample that differs in
    its bits from the one before."""
    b = bits(out)
    at = np.concatenate([[0], np.flatnonzero(b[1:] != b[:-1]) + 1]) if len(b) else np.zeros(0, np.int64)
    return at.astype(np.uint32), np.asarray(out, f32)[at]


def from_steps(at, values, n):
    out = np.zeros(n, f32)
    for i, p in enumerate(at):
        out[int(p):] = values[i]
    return out


def arrays(cases):
    """The cases with their results -> the arrays of one file (all cases of one kind)."""
    a = {"names": np.array([c["name"] for c in cases])}
    a["head"] = np.array([[c["kind"], c["channels"], fbits(c["a"]), fbits(c["b"]), c["sample_rate"], c["n"], len(c["steps"]), len(c["calls"])]
                          for c in cases], np.uint32)
    a["steps"] = np.array([[op, ch, fbits(v), length, flags] for c in cases for op, ch, v, length, flags in c["steps"]], np.uint32).reshape(-1, 5)
    a["segments"] = np.array([[i, ch, length, kind, fbits(amp), seed] for i, c in enumerate(cases) for ch, segs in enumerate(c["segments"])
                              for length, kind, amp, seed in segs], np.uint32).reshape(-1, 6)
    a["step_results"] = np.concatenate([c["step_results"] for c in cases]).astype(np.uint32)
    a["bare_clear"] = np.array([[i] + list(c["bare_clear"]) for i, c in enumerate(cases) if c.get("bare_clear")], np.uint32).reshape(-1, 4)
    getters, state, nstate, crcs, have = [], [], [], [], []
    for c in cases:
        for r in c["calls"]:
            getters.append(np.concatenate([r["designation"], r["link"], r["active"], [r["weighting"], r["period"], r["sample_rate"]]]))
            state.append(r["state"])
            nstate.append(len(r["state"]))
            crcs.append([r["crc"]] + [0 if v is None else v for v in r["ch_crc"]])
            have.append([0 if v is None else 1 for v in r["ch_crc"]])
    a["getters"] = np.concatenate(getters).astype(np.uint32) if getters else np.zeros(0, np.uint32)
    a["state"] = np.concatenate(state).astype(np.uint32) if state else np.zeros(0, np.uint32)
    a["nstate"] = np.array(nstate, np.uint32)
    a["crc"] = np.concatenate([np.array(v, np.uint32) for v in crcs]) if crcs else np.zeros(0, np.uint32)
    a["have"] = np.concatenate([np.array(v, np.uint8) for v in have]) if have else np.zeros(0, np.uint8)
    if cases and cases[0]["kind"] == ILUFS:
        a["out_at"] = np.concatenate([c["out_steps"][0] for c in cases])
        a["out_values"] = np.concatenate([c["out_steps"][1] for c in cases])
        a["out_count"] = np.array([len(c["out_steps"][0]) for c in cases], np.uint32)
    else:
        a["samples"] = np.concatenate([c["samples"].reshape(-1) for c in cases if not c.get("bare_clear")]).astype(f32)
    return a


def load(kind):
    """The stored cases of one kind, as make_loudness_vectors.py had them: settings, steps, segments and, from the reference, per step
    needs_update / latency / loudness, per call getters, state and CRCs, and the outputs (ILUFSMeter: `out` whole; LoudnessMeter:
    `index` and `samples` [1 + channels][len(index)], a channel's row holding SENTINEL where no call wrote it).  The case with the bare
    clear() has no outputs: `bare_clear` = (sBank.nItems before, after, 1 if its outputs differ from the well-defined sequence's)."""
    z = np.load(FILES[kind])
    cases = []
    s_at = r_at = g_at = st_at = c_at = h_at = call_at = o_at = smp_at = 0
    bare = {int(r[0]): tuple(int(v) for v in r[1:]) for r in z["bare_clear"]}
    for i, name in enumerate(z["names"]):
        k, K, a, b, sr, n, nsteps, ncalls = (int(v) for v in z["head"][i])
        c = dict(name=str(name), kind=k, channels=K, a=from_bits(a), b=from_bits(b), sample_rate=sr, n=n)
        c["steps"] = [(int(op), int(ch), from_bits(v), int(length), int(flags)) for op, ch, v, length, flags in z["steps"][s_at:s_at + nsteps]]
        s_at += nsteps
        c["segments"] = [[(int(r[2]), int(r[3]), from_bits(r[4]), int(r[5])) for r in z["segments"] if r[0] == i and r[1] == ch] for ch in range(K)]
        c["step_results"] = z["step_results"][r_at:r_at + nsteps]
        r_at += nsteps
        c["calls"] = []
        for _ in range(ncalls):
            g = z["getters"][g_at:g_at + 3 * K + 3]
            g_at += 3 * K + 3
            ns = int(z["nstate"][call_at])
            r = dict(designation=g[:K], link=g[K:2 * K], active=g[2 * K:3 * K], weighting=int(g[3 * K]), period=int(g[3 * K + 1]),
                     sample_rate=int(g[3 * K + 2]), state=z["state"][st_at:st_at + ns])
            st_at += ns
            row = z["crc"][c_at:c_at + 1 + K]
            hv = z["have"][h_at:h_at + K]
            c_at += 1 + K
            h_at += K
            call_at += 1
            r["crc"], r["ch_crc"] = int(row[0]), [int(v) if h else None for v, h in zip(row[1:], hv)]
            c["calls"].append(r)
        if i in bare:
            c["bare_clear"] = bare[i]
        elif k == ILUFS:
            m = int(z["out_count"][i])
            c["out"] = from_steps(z["out_at"][o_at:o_at + m], z["out_values"][o_at:o_at + m], n)
            o_at += m
        else:
            c["index"] = sample_index(c)
            m = (1 + K) * len(c["index"])
            c["samples"] = z["samples"][smp_at:smp_at + m].reshape(1 + K, -1)
            smp_at += m
        cases.append(c)
    return cases


def lstate(r, K):
    """A LoudnessMeter call's recorded state -> dict (ms: the fMS bits per channel)."""
    d = {k: int(v) for k, v in zip(L_STATE, r["state"])}
    d["ms"] = [int(v) for v in r["state"][len(L_STATE):len(L_STATE) + K]]
    return d


def istate(r, K):
    d = {k: int(v) for k, v in zip(I_STATE, r["state"])}
    base = len(I_STATE)
    d["block"] = r["state"][base:base + 4 * K].copy().view(f32).reshape(K, 4)
    d["hist"] = r["state"][base + 4 * K:].copy().view(f32)
    assert len(d["hist"]) == d["ms_size"]
    return d


# ---- the restatements over a recorded case -----------------------------------------------------------------------------------------
def replay(c, x=None, on_call=None):
    """The case on oracle.loudness.LoudnessMeter / oracle.ilufs.ILUFSMeter -> (step results [nsteps][3], per call a dict with out,
    ch_out and the state in the recording's own words).  on_call(meter, call index) runs after every process() call."""
    from oracle import ilufs as oi, loudness as ol
    K = c["channels"]
    x = rows(c) if x is None else x
    calls = {call["step"]: call for call in walk(c)}
    m = ol.LoudnessMeter(K, c["a"]) if c["kind"] == LOUDNESS else oi.ILUFSMeter(K, c["a"], c["b"])
    m.set_sample_rate(c["sample_rate"])
    steps, out = [], []
    for si, (op, ch, a, length, flags) in enumerate(c["steps"]):
        name = OPS[op]
        if name == "process":
            call = calls[si]
            for k in range(K):
                m.set_bound(k, call["in_at"][k] is not None)
            xin = call_input(c, x, call)
            if c["kind"] == LOUDNESS:
                o, cho = m.process(xin, gain=f32(a) if flags & PF_GAIN else None)
                st = [m.period, m.size, m.head, m.refresh, None, None] + [fbits(q["ms"]) for q in m.ch]
                r = dict(out=o, ch_out=[cho[k] if call["have"][k] else None for k in range(K)], state=st)
            else:
                o = m.process(xin, gain=f32(a) if flags & PF_GAIN else DEFAULT_GAIN)
                st = [m.block_size, m.block_offset, m.block_part, m.ms_size, m.ms_int, m.ms_count, m.ms_head, 4 if m.blk_full else 0]
                st += [int(v) for q in m.ch for v in bits(q["block"])] + [int(v) for v in bits(m.hist)]
                r = dict(out=o, ch_out=[None] * K, state=st)
            if flags & PF_NULL:
                r["out"] = np.full(length, SENTINEL, f32)
            out.append(r)
            if on_call is not None:
                on_call(m, len(out) - 1)
        elif name == "bind":
            pass                                            # walk() has it
        elif name == "set_designation":
            m.set_designation(ch, int(a))
        elif name == "set_link":
            m.set_link(ch, f32(a))
        elif name == "set_active":
            m.set_active(ch, a != 0)
        elif name == "set_weighting":
            m.set_weighting(int(a))
        elif name == "set_period":
            (m.set_period if c["kind"] == LOUDNESS else m.set_integration_period)(f32(a))
        elif name == "clear":
            m.clear()
        elif name == "update_settings":
            m.update_settings()
        elif name == "set_sample_rate":
            m.set_sample_rate(length)
        steps.append([int(m.needs_update()), m.latency() if c["kind"] == LOUDNESS else 0, fbits(m.loud)])
    return np.array(steps, np.uint32).reshape(-1, 3), out
