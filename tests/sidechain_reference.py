"""Reads tests/golden/sidechain_ref_vectors.npz (written by tests/golden/make_sidechain_vectors.py from the reference's own
compiled Sidechain class) and replays its cases: on the numpy restatement (replay) and, in the GPU tests, on the bank.  Never
reads the reference tree or oracle/_ref/.

A case: name, n, inputs, sample_rate, max_reactivity, reactivity, mode, source, stereo, gain, single, calls, null (per call: the
call passes in == NULL), events [(ahead of which call, setter, float32 argument)], in0, in1 (rows of x), state uint32 [calls, 9]
(STATE; a single-sample case is n calls of one sample and keeps the last call's row only), out and single_out (Stored), ring (the last
nReactivity ring values after the last call, oldest first), lpf (the case is in LPF mode at some time)."""
import io
import os
import zlib

import numpy as np

import sidechain_ref as ref

f32 = np.float32
PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sidechain_ref_vectors.npz")
EVENTS = ("set_reactivity", "set_mode", "set_source", "set_gain", "set_stereo_mode", "clear", "set_sample_rate")
STATE = ("reactivity", "tau", "refresh", "rms", "flags", "capacity", "head", "ring_crc", "places")
# the places a call went through, as the driver saw them on the class's own counters and ring
P_RMS_WHOLE, P_RMS_WRAPPED, P_UNI_WHOLE, P_UNI_WRAPPED, P_SPLIT, P_OTHER_REFRESH, P_COUNTED, P_AT_START, P_HEAD_AT_END = (1 << i for i in range(9))
WHOLE, WINDOW, BLOCK = 2000, 64, 1024           # rows longer than WHOLE are stored as windows and block check sums
SCF_MIDSIDE, SCF_UPDATE, SCF_CLEAR = 1, 2, 4


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


MAGIC = 0x53434844


def case_bytes(cases):
    """The case file of oracle/sidechain_driver.cpp (its head comment has the layout)."""
    b = io.BytesIO()
    u32 = lambda *v: b.write(np.array(v, np.uint32).tobytes())
    fl = lambda *v: b.write(np.array(v, f32).tobytes())
    u32(MAGIC, len(cases))
    for c in cases:
        u32(c["inputs"]); fl(c["max_reactivity"]); u32(c["sample_rate"]); fl(c["reactivity"])
        u32(c["mode"], c["source"], c["stereo"]); fl(c["gain"]); u32(int(bool(c["single"])))
        u32(len(c["calls"]))
        b.write(np.stack([c["calls"], c["null"]], 1).astype(np.uint32).tobytes())
        u32(len(c["events"]))
        for before, setter, a in c["events"]:
            u32(before, EVENTS.index(setter)); fl(a)
        u32(c["n"])
        for r in ([c["in0"]] if c["inputs"] == 1 else [c["in0"], c["in1"]]):
            assert len(r) == c["n"]
            b.write(np.ascontiguousarray(r, f32).tobytes())
    return b.getvalue()


def parse_results(raw, cases, reference=True):
    """What a driver wrote: per case a dict of state uint32 [calls, 9], out, pre_array, pre_scalar, single_out, ring (float32); the
    product's class (reference=False) writes no preprocess() rows and no ring."""
    w = np.frombuffer(raw, np.uint32)
    pos, out = 0, []

    def take(n):
        nonlocal pos
        v = w[pos:pos + n]
        assert len(v) == n, "short result file"
        pos += n
        return v

    def vec():
        return take(int(take(1)[0])).view(f32).copy()

    for c in cases:
        ncalls = int(take(1)[0])
        assert ncalls == len(c["calls"])
        r = {"state": take(9 * ncalls).reshape(ncalls, 9).copy(), "out": vec()}
        npre = int(take(1)[0])
        r["pre_array"], r["pre_scalar"] = take(npre).view(f32).copy(), take(npre).view(f32).copy()
        r["single_out"], r["ring"] = vec(), vec()
        assert len(r["out"]) == c["n"] and npre == (c["n"] if reference else 0) and len(r["single_out"]) == (c["n"] if c["single"] else 0)
        out.append(r)
    assert pos == len(w), "result file longer than its cases"
    return out


class Stored:
    """A row of n float32: whole, or windows of WINDOW samples and a CRC-32 of the bits of every block of BLOCK samples."""

    def __init__(self, n, whole, starts, windows, crc):
        self.n, self.whole, self.starts, self.windows, self.crc = n, whole, starts, windows, crc

    def mismatch(self, got):
        """None where `got` has the stored bits, else where it first differs."""
        got = np.ascontiguousarray(got, f32)
        assert got.shape == (self.n,), got.shape
        if self.n <= WHOLE:
            bad = np.flatnonzero(bits(got) != bits(self.whole))
            return None if len(bad) == 0 else "sample %d: %r for %r (%d differ)" % (bad[0], got[bad[0]], self.whole[bad[0]], len(bad))
        for s, w in zip(self.starts, self.windows):
            bad = np.flatnonzero(bits(got[s:s + WINDOW]) != bits(w))
            if len(bad):
                return "sample %d: %r for %r" % (s + bad[0], got[s + bad[0]], w[bad[0]])
        for k, c in enumerate(self.crc):
            if zlib.crc32(bits(got[k * BLOCK:(k + 1) * BLOCK]).tobytes()) != int(c):
                return "block of %d samples at %d" % (BLOCK, k * BLOCK)
        return None

    def at(self, i):
        """The stored sample i (which has to be a stored one)."""
        if self.n <= WHOLE:
            return self.whole[i]
        k = [j for j, s in enumerate(self.starts) if s <= i < s + WINDOW][0]
        return self.windows[k][i - self.starts[k]]


def load(path=PATH):
    z = np.load(path)
    x = np.split(z["x"], np.cumsum(z["x_len"])[:-1])
    cases = []
    pc = pe = pr = 0
    pos = {"out": [0, 0, 0], "single": [0, 0, 0]}
    nsingle = 0
    for i, name in enumerate(z["names"]):
        n, single = int(z["n"][i]), bool(z["single"][i])
        c = dict(name=str(name), n=n, single=single, ring=z["ring"][pr:pr + int(z["nring"][i])])
        pr += int(z["nring"][i])
        for k in ("inputs", "sample_rate", "mode", "source", "stereo"):
            c[k] = int(z[k][i])
        for k in ("max_reactivity", "reactivity", "gain"):
            c[k] = f32(z[k][i])
        r0, o0, r1, o1 = (int(v) for v in z["rows"][i])
        c["in0"] = x[r0][o0:o0 + n]
        c["in1"] = x[r1][o1:o1 + n] if r1 >= 0 else None
        nc = int(z["ncalls"][i])
        c["calls"] = [1] * n if single else [int(v) for v in z["calls"][pc:pc + nc]]
        c["null"] = [0] * n if single else [int(v) for v in z["null"][pc:pc + nc]]
        rows = 1 if single else nc
        c["state"] = z["state"][pc + nsingle:pc + nsingle + rows]
        pc += nc
        nsingle += 1 if single else 0
        ne = int(z["nevents"][i])
        c["events"] = [(int(b), EVENTS[int(k)], np.array([a], np.uint32).view(f32)[0]) for b, k, a in z["events"][pe:pe + ne]]
        pe += ne
        for key in (("out", "single") if single else ("out",)):
            row = i if key == "out" else nsingle - 1
            nw, ns, _, ncrc = (int(v) for v in z[key + "_counts"][row])
            p = pos[key]
            c["out" if key == "out" else "single_out"] = Stored(n, z[key + "_whole"][p[0]:p[0] + nw], z[key + "_starts"][p[1]:p[1] + ns], z[key + "_windows"][p[1]:p[1] + ns],
                            z[key + "_crc"][p[2]:p[2] + ncrc])
            p[0], p[1], p[2] = p[0] + nw, p[1] + ns, p[2] + ncrc
        c["lpf"] = c["mode"] == ref.SCM_LPF or any(s == "set_mode" and int(a) == ref.SCM_LPF for _, s, a in c["events"])
        cases.append(c)
    return cases


def column(case, name):
    """A column of the case's state rows; tau and rms as float32."""
    v = case["state"][:, STATE.index(name)]
    return v.view(f32) if name in ("tau", "rms") else v


class Settings:
    """The setters' side of the class as Sidechain.cpp:67-142 and Sidechain.h:146-175 state it: what every setter does to
    fReactivity, nMode, nSource, fGain and nFlags, and what update_settings() then owes the state."""

    def __init__(self, case):
        self.max, self.reactivity = f32(case["max_reactivity"]), f32(0.0)
        self.mode, self.source, self.gain = ref.SCM_RMS, ref.SCS_MIDDLE, f32(1.0)
        self.flags, self.rate, self.new_ring, self.zeroed = SCF_UPDATE | SCF_CLEAR, 0, False, False
        for setter, a in (("set_sample_rate", case["sample_rate"]), ("set_reactivity", case["reactivity"]), ("set_mode", case["mode"]),
                          ("set_source", case["source"]), ("set_stereo_mode", case["stereo"]), ("set_gain", case["gain"])):
            self.apply(setter, a)

    def apply(self, setter, a):
        a = f32(a)
        if setter == "set_sample_rate":
            self.rate, self.flags, self.new_ring = int(a), SCF_UPDATE | SCF_CLEAR, True         # the mid-side flag goes too (:91)
        elif setter == "set_reactivity":
            if not (self.reactivity == a or a < 0 or a > self.max):
                self.reactivity = a
                self.flags |= SCF_UPDATE
        elif setter == "set_stereo_mode":
            if bool(self.flags & SCF_MIDSIDE) != bool(int(a)):
                self.flags = (self.flags & ~SCF_MIDSIDE) | (SCF_MIDSIDE if int(a) else 0) | SCF_CLEAR
        elif setter == "clear":
            self.flags |= SCF_CLEAR
        elif setter == "set_mode":
            if self.mode != int(a):
                self.mode, self.zeroed = int(a), True
        elif setter == "set_source":
            self.source = int(a)
        elif setter == "set_gain":
            self.gain = a
        else:
            raise ValueError(setter)

    def settle(self):
        """update_settings(): -> (an update was pending, a clear was pending, a new ring was made)."""
        got = bool(self.flags & SCF_UPDATE), bool(self.flags & SCF_CLEAR), self.new_ring
        self.flags &= SCF_MIDSIDE
        self.new_ring = False
        return got


def events_before(case, call):
    return [(s, a) for b, s, a in case["events"] if b == call]


def recorded_params(case):
    """Per call the parameters the reference had in force: nReactivity, fTau, 1 / nReactivity, the capacity."""
    rows = case["state"]
    assert not case["single"]
    return [dict(reactivity=int(r[0]), tau=r[1:2].view(f32)[0], interval=f32(1.0) / f32(int(r[0])), capacity=int(r[5])) for r in rows]


def single_params(case, tau=None):
    """Per call the parameters of a single-sample case, whose per-call rows are not stored: the window from the restatement's
    integer arithmetic, tau the last call's recorded one (such a case in LPF mode has no event)."""
    st = Settings(case)
    out = []
    for i in range(case["n"]):
        for setter, a in events_before(case, i):
            st.apply(setter, a)
        n = ref.reactivity_samples(st.rate, st.reactivity)
        out.append(dict(reactivity=n, tau=column(case, "tau")[-1] if tau is None else tau, interval=f32(1.0) / f32(n),
                        capacity=ref.capacity(st.rate, st.max)))
    return out


def replay(case, params, early_refresh=False):
    """The restatement (sidechain_ref.Sidechains, one channel) through the case's calls and events with the given per-call
    parameters -> (out [n], state uint32 [calls, 8] as STATE without the places, the last ring values, fRmsValue after every
    sample).  early_refresh: the counter runs one sample ahead after the first call, as the single-sample overload's does."""
    st = Settings(case)
    sc = None
    out, trace = np.zeros(case["n"], f32), np.zeros(case["n"], f32)
    rows = []
    pos = 0
    for i, n in enumerate(case["calls"]):
        if early_refresh and i == 1:
            sc.refresh += 1
        for setter, a in events_before(case, i):
            if setter == "set_mode" and sc is not None:
                sc.set_mode(0, int(a))
            st.apply(setter, a)
        updated, cleared, new_ring = st.settle()
        p = dict(params[i], mode=st.mode, source=st.source, flags=st.flags & SCF_MIDSIDE, gain=st.gain)
        if sc is None or new_ring:
            sc = ref.Sidechains([p], case["inputs"])
        else:
            sc.set_params([p])
        if updated:
            sc.updated(0)
        if cleared:
            sc.clear(0)
        if case["null"][i]:
            got = sc.process(None, count=n)
        else:
            in1 = None if case["in1"] is None else case["in1"][None, pos:pos + n]
            got = sc.process(case["in0"][None, pos:pos + n], in1)
        out[pos:pos + n], trace[pos:pos + n] = got[0][0], got[1][0]
        pos += n
        s = sc.state()
        ring = ring_tail(sc, 0)
        rows.append([p["reactivity"], int(bits(p["tau"])[0]), int(s["refresh"][0]), int(bits(s["rms"][0])[0]), st.flags, p["capacity"],
                     int(s["head"][0]), zlib.crc32(bits(ring).tobytes())])
    return out, np.array(rows, np.uint32), ring, trace


def ring_tail(sc, ch):
    n, cap, head = int(sc.N[ch]), int(sc.cap[ch]), int(sc.head[ch])
    return sc.ring[ch][(head - n + np.arange(n)) % cap]


def one_by_one(case, params, early, divide, left_first):
    """The single-sample overload, Sidechain.cpp:556-624, on every sample of a case with one call per sample, with each of its
    differences from the block overload as a switch: early (++nRefresh BEFORE the comparison with 0x2000, :569), divide
    (rms / float(nReactivity), :601, :614, for rms * (1.0f / nReactivity)) and left_first ((fRmsValue + new) - last, :600, :613, for
    rms += new - last).  All three off is the block overload on calls of one sample.  -> out [n]"""
    st = Settings(case)
    two = case["inputs"] == 2
    ring, head, rms, refresh = None, 0, f32(0.0), 0
    out = np.zeros(case["n"], f32)
    zero = f32(0.0)
    with np.errstate(under="ignore"):
        for t in range(case["n"]):
            for setter, a in events_before(case, t):
                if setter == "set_mode" and st.mode != int(a):
                    rms = zero
                st.apply(setter, a)
            updated, cleared, new_ring = st.settle()
            p = params[t]
            n, cap, mode = p["reactivity"], p["capacity"], st.mode
            if ring is None or new_ring:
                ring, head = np.zeros(cap, f32), 0
            if updated:
                refresh = ref.REFRESH_RATE
            if cleared:
                rms, refresh = zero, 0
                ring[:] = 0
            b = None if case["in1"] is None else case["in1"][t:t + 1]
            s = ref.pick_source(case["in0"][t:t + 1], b, st.source, bool(st.flags & SCF_MIDSIDE), two)[0]
            x = f32(np.abs(s) * st.gain)
            refresh += 1 if early else 0
            if refresh >= ref.REFRESH_RATE:
                if mode == ref.SCM_PEAK:
                    rms = zero
                elif mode != ref.SCM_LPF:
                    term = (lambda v: v * v) if mode == ref.SCM_RMS else np.abs
                    tail = (head + cap - n) % cap
                    rms = ref.serial_sum(term(ring[tail:tail + n])) if tail < head else \
                        f32(ref.serial_sum(term(ring[tail:])) + ref.serial_sum(term(ring[:head])))
                refresh %= ref.REFRESH_RATE
            refresh += 0 if early else 1
            ring[head] = x
            head = (head + 1) % cap
            last = ring[(head + cap - (n + 1)) % cap]
            if mode == ref.SCM_PEAK:
                out[t] = x
            elif mode == ref.SCM_LPF:
                rms = f32(rms + p["tau"] * f32(x - rms))
                out[t] = max(rms, zero)
            else:
                new, old = (f32(x * x), f32(last * last)) if mode == ref.SCM_RMS else (x, last)
                rms = f32(f32(rms + new) - old) if left_first else f32(rms + f32(new - old))
                q = f32(rms / f32(n)) if divide else f32(rms * p["interval"])
                if mode == ref.SCM_UNIFORM:
                    out[t] = zero if rms < zero else q
                elif divide:
                    out[t] = zero if rms < zero else np.sqrt(q)
                else:
                    out[t] = np.sqrt(q) if q > zero else zero
    return out
