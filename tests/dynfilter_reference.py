"""Reads tests/golden/dynfilter_ref_*.npz (written by tests/golden/make_dynfilter_vectors.py from the reference's own compiled
DynamicFilters class) and replays the cases on the numpy restatement (oracle/dynamic_filters.py).  Never reads the reference tree.

A case: name, filters, sample_rate, record, events [(ahead of which call, kind, fid, fp)] with kind 0 set_params(fid, fp) and 1
set_filter_active(fid), fp = (nType, nSlope, fFreq, fFreq2, fGain, fQuality) as given; calls [(fid, offset, len)]: process(fid, out,
x + offset, gain + offset, len); x, gain; and what the reference did: params (get_params(fid) after every call, six 32-bit words: the
swapped frequencies and the transformed fFreq2), kf (what the transform was handed), groups (per call the cascade arrays in the
reference's groups of 8 / 4 / 2 / 1, float32 [lanes, samples, 11] = t[0..2], b[0..2] and the section b0 b1 b2 a1 a2 that the
transform's stand-in made of them, out of their diagonal layout; recorded cases only), out (the outputs of the calls one after another)."""
import io
import os

import numpy as np

from conftest import IIR_EXACT_FACTOR, IIR_REF_FACTOR, NOISE_FLOOR, TOL

f32 = np.float32
# how far the numpy restatement (numpy's tan, exp, log, cos) was from the recording (glibc's) when it was written, in units in the
# last place: the cascades (RLC bell and resonance at a gain of 1e-3; 6 elsewhere), and the transformed fFreq2 and kf.  The tests
# allow twice that, because a second host libm may round the other way.
CASCADE_ULP_SEEN, PARAM_ULP_SEEN = 15, 2
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FILES = {k: os.path.join(GOLDEN, "dynfilter_ref_%s.npz" % k) for k in ("rlc", "bwc", "lrx", "streams")}
MAGIC = 0x44594e46
SET_PARAMS, SET_ACTIVE = 0, 1
BUF_SIZE = 0x400


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def fp_words(fp):
    return np.concatenate([np.array(fp[:2], np.uint32), bits(np.array(fp[2:], f32))])


def fp_tuple(words):
    w = np.ascontiguousarray(words, np.uint32)
    f = w[2:].view(f32)
    return (int(w[0]), int(w[1]), f[0], f[1], f[2], f[3])


def ulps(a, b):
    """The distance of two float32 arrays in units in the last place (on the number line of the float32 values)."""
    def key(v):
        w = np.ascontiguousarray(v, f32).view(np.int32).astype(np.int64)
        return np.where(w < 0, -(w & 0x7fffffff), w)
    return np.abs(key(a) - key(b))


def check(y, ref, exact, what, coef_tol=0.0):
    """conftest.assert_iir_parity's rule (the recursion's own float32 noise is the yardstick).
    coef_tol: how far the coefficient sets of the device and of the oracle may differ (matched-Z types: the float
    amplitude normalisation next to z = 1, Filter.cpp:2369-2411, turns the last bits of expf into 1e-4 of a numerator --
    tests/test_oracle_dynamic_filters.py::test_product_builders_match_the_oracle shows the same between two host libms)."""
    peak = max(float(np.abs(exact).max()), 1e-30)
    noise = float(np.abs(ref - exact).max()) / peak
    e32 = float(np.abs(y - ref).max()) / peak
    e64 = float(np.abs(y - exact).max()) / peak
    msg = "%s: vs oracle %.2e, vs float64 %.2e, oracle's own noise %.2e" % (what, e32, e64, noise)
    assert np.all(np.isfinite(y)), msg
    # the coefficients themselves come from two libms (device / numpy): one part in 1e6 of the coefficients on top of the
    # recursion's noise
    if noise <= NOISE_FLOOR:
        assert e32 <= 2 * TOL + coef_tol, msg
    else:
        assert e64 <= max(2 * TOL, IIR_EXACT_FACTOR * noise) + coef_tol and e32 <= max(2 * TOL, IIR_REF_FACTOR * noise) + coef_tol, msg
    return e32, noise


def coef_tol(case):
    """check's coef_tol for a case: 1e-3 where a matched-Z type is in it, else 0 (as tests/test_dynfilter_gpu.py has it)."""
    return 1e-3 if any(e[1] == SET_PARAMS and not (e[3][0] & 1) for e in case["events"]) else 0.0


def case_bytes(cases):
    """The case file of oracle/dynfilter_driver.cpp (its head comment has the layout)."""
    b = io.BytesIO()
    u32 = lambda *v: b.write(np.array(v, np.uint32).tobytes())
    u32(MAGIC, len(cases))
    for c in cases:
        u32(c["filters"], c["sample_rate"], c["record"], len(c["events"]))
        for before, kind, fid, fp in c["events"]:
            u32(before, kind, fid)
            b.write(fp_words(fp).tobytes())
        u32(len(c["calls"]))
        for call in c["calls"]:
            u32(*call)
        assert len(c["x"]) == len(c["gain"])
        u32(len(c["x"]))
        b.write(np.ascontiguousarray(c["x"], f32).tobytes())
        b.write(np.ascontiguousarray(c["gain"], f32).tobytes())
    return b.getvalue()


def parse_results(raw, cases):
    """What a driver wrote: per case a dict of params [calls, 6] uint32, kf [calls], groups (a list per call) and out."""
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
        r = dict(params=np.zeros((ncalls, 6), np.uint32), kf=np.zeros(ncalls, f32), groups=[])
        for i in range(ncalls):
            r["params"][i] = take(6)
            r["kf"][i] = take(1).view(f32)[0]
            gs = []
            for _ in range(int(take(1)[0])):
                lanes, samples = (int(v) for v in take(2))
                gs.append(take(lanes * samples * 11).view(f32).reshape(lanes, samples, 11).copy())
            r["groups"].append(gs)
        r["out"] = take(int(take(1)[0])).view(f32).copy()
        assert len(r["out"]) == sum(call[2] for call in c["calls"])
        out.append(r)
    assert pos == len(w), "result file longer than its cases"
    return out


def arrays(cases, x, gain):
    """The cases as the arrays of one file; x and gain are the shared rows that every case's input is a stretch of."""
    a = {"names": np.array([c["name"] for c in cases]), "x": x, "gain": gain}
    for k in ("filters", "sample_rate", "record", "at_x", "at_gain"):
        a[k] = np.array([c[k] for c in cases], np.uint32)
    a["n"] = np.array([len(c["x"]) for c in cases], np.uint32)
    a["nevents"] = np.array([len(c["events"]) for c in cases], np.uint32)
    a["events"] = np.array([np.concatenate([np.array(e[:3], np.uint32), fp_words(e[3])]) for c in cases for e in c["events"]], np.uint32).reshape(-1, 9)
    a["ncalls"] = np.array([len(c["calls"]) for c in cases], np.uint32)
    a["calls"] = np.array([call for c in cases for call in c["calls"]], np.uint32).reshape(-1, 3)
    a["params"] = np.concatenate([c["params"] for c in cases]).astype(np.uint32)
    a["kf"] = np.concatenate([c["kf"] for c in cases]).astype(f32)
    a["ngroups"] = np.array([len(g) for c in cases for g in c["groups"]], np.uint32)
    a["group_shape"] = np.array([g.shape[:2] for c in cases for gs in c["groups"] for g in gs], np.uint32).reshape(-1, 2)
    a["cascades"] = np.concatenate([g.reshape(-1) for c in cases for gs in c["groups"] for g in gs] or [np.zeros(0, f32)]).astype(f32)
    a["out"] = np.concatenate([c["out"] for c in cases]).astype(f32)
    return a


def load(which):
    z = np.load(FILES[which])
    cases = []
    pe = pc = pg = pv = po = 0
    for i, name in enumerate(z["names"]):
        n, ne, nc = int(z["n"][i]), int(z["nevents"][i]), int(z["ncalls"][i])
        c = dict(name=str(name), filters=int(z["filters"][i]), sample_rate=int(z["sample_rate"][i]), record=int(z["record"][i]),
                 events=[(int(e[0]), int(e[1]), int(e[2]), fp_tuple(e[3:])) for e in z["events"][pe:pe + ne]],
                 calls=[tuple(int(v) for v in call) for call in z["calls"][pc:pc + nc]],
                 x=z["x"][int(z["at_x"][i]):int(z["at_x"][i]) + n], gain=z["gain"][int(z["at_gain"][i]):int(z["at_gain"][i]) + n],
                 params=z["params"][pc:pc + nc], kf=z["kf"][pc:pc + nc], groups=[])
        for k in z["ngroups"][pc:pc + nc]:
            gs = []
            for lanes, samples in z["group_shape"][pg:pg + int(k)]:
                m = int(lanes) * int(samples) * 11
                gs.append(z["cascades"][pv:pv + m].reshape(int(lanes), int(samples), 11))
                pv += m
            pg += int(k)
            c["groups"].append(gs)
        total = sum(call[2] for call in c["calls"])
        c["out"] = z["out"][po:po + total]
        pe, pc, po = pe + ne, pc + nc, po + total
        cases.append(c)
    return cases


def cascades_of(case, call):
    """The cascades of a recorded call of at most BUF_SIZE samples, the groups put together: (T, B) float32 [nc, samples, 3], and the
    group sizes."""
    gs = case["groups"][call]
    assert case["calls"][call][2] <= BUF_SIZE and gs
    all_ = np.concatenate(gs)
    return all_[..., :3], all_[..., 3:6], [len(g) for g in gs]


def sections_of(case, call):
    """The sections that the transform's stand-in (glibc's expf and cosf for matched-Z) made of those cascades: [nc, samples, 5]."""
    return np.concatenate(case["groups"][call])[..., 6:]


def margin(case, df, call, **wrong):
    """How far the restatement's output over the 64 samples from the start of `call` moves, against its peak there, when the memory
    is handled the wrong way (replay's no_clear_at / clear_at)."""
    at = sum(k[2] for k in case["calls"][:call])
    w = slice(at, at + 64)
    a, b = replay(case, df), replay(case, df, **wrong)
    return float(np.max(np.abs(a[w].astype(np.float64) - b[w]))) / max(float(np.max(np.abs(a[w]))), 1e-30)


def long_boundaries(case):
    """The two events of a longer case: (the call of filter 0 after the same-type set_params, which keeps the memory; the call ahead
    of which the new type stands; the first call of the OTHER filter after it, whose memory is cleared as well)."""
    keep = [e[0] for e in case["events"] if e[0] > 0 and e[1] == SET_PARAMS][0]
    new, fid = [(e[0], e[2]) for e in case["events"] if e[0] > keep and e[1] == SET_PARAMS][0]
    other = [i for i, k in enumerate(case["calls"]) if i >= new and k[0] == 1 - fid][0]
    assert case["calls"][keep][0] == 0
    return keep, new, other


def group_sizes(nc):
    """DynamicFilters::quantify (DynamicFilters.cpp:191-202) over nc cascades: 8 while 8 are left, then 4, 2, 1."""
    out = []
    while nc > 0:
        k = 8 if nc >= 8 else 4 if nc >= 4 else 2 if nc >= 2 else 1
        out.append(k)
        nc -= k
    return out


def replay(case, df, exact=False, no_clear_at=None, clear_at=None):
    """The restatement (oracle.dynamic_filters.DynamicFilters) through the case's events and calls -> out, or (out, float64 out).
    no_clear_at: the call ahead of which a pending clear of the memory is dropped; clear_at: the call ahead of which the memory is
    cleared although nothing asks for it (what a wrong implementation would do, either way)."""
    obj = df.DynamicFilters(case["filters"])
    obj.set_sample_rate(case["sample_rate"])
    out, out64 = [], []
    for i, (fid, offset, n) in enumerate(case["calls"]):
        for before, kind, efid, fp in case["events"]:
            if before == i:
                if kind == SET_PARAMS:
                    obj.set_params(efid, *fp)
                else:
                    obj.set_filter_active(efid, True)
        if no_clear_at == i:
            obj.clear_mem = False
        if clear_at == i:
            obj.clear_mem = True
        y = obj.process(fid, case["x"][offset:offset + n], case["gain"][offset:offset + n], exact=True) if fid < case["filters"] else \
            (case["x"][offset:offset + n].copy(), case["x"][offset:offset + n].astype(np.float64))
        out.append(y[0])
        out64.append(y[1])
    out, out64 = np.concatenate(out), np.concatenate(out64)
    return (out, out64) if exact else out
