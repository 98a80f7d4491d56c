"""Writes tests/golden/loudness_ref_vectors.npz and ilufs_ref_vectors.npz: what the reference's own LoudnessMeter and ILUFSMeter
classes (oracle/_ref/loudness_ref: LoudnessMeter.cpp, ILUFSMeter.cpp, broadcast.cpp, Filter.cpp and FilterBank.cpp compiled
unmodified, see oracle/Makefile) compute on a list of cases.  Data only: settings, steps, the segments the input rows are made of,
the reference's outputs and its state after every call.  Run where the reference tree exists, after the build:

    python tests/golden/make_loudness_vectors.py

Every case first runs through oracle/_ref/loudness_ref_san, the same program with the address and undefined-behaviour sanitizers
(a stand-alone host program); nothing is written unless that run is clean and gives the same bytes.  The one exception is recorded
as a fact: the case "clear bare" calls LoudnessMeter::clear() with nothing else between two calls, which leaves the reference's
filter bank with its cascades added twice and its packed sections stale; the two builds need not agree on it, and only
sBank.nItems before and after and whether its outputs differ from "clear defined" are kept.  No gating block of an ILUFSMeter case
may lie within 5 % of the absolute gate: asserted from the reference's own vLoudness after every call and, for the blocks that leave no
trace there, from the restatement, which tests/test_loudness_reference_host.py holds to the same recording bit for bit.  That test
also regenerates the files with build_bytes() and requires the committed bytes, so they are written without time stamps.  The layout
is tests/loudness_reference.py's, which reads it.
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

import loudness_reference as R  # noqa: E402

f32 = np.float32
LD_REF = os.path.join(ROOT, "oracle", "_ref", "loudness_ref")
LD_SAN = os.path.join(ROOT, "oracle", "_ref", "loudness_ref_san")
NONE, A, B, C, D, K = range(6)                                     # bs::weighting_t
CH_NONE, CENTER, LEFT, RIGHT, LFE1, LFE2 = 0, 1, 4, 5, 32, 33       # bs::channel_t; 6..11 the +1.5 dB group
GATING_ABS_THRESH = f32(1.17246530458e-07)
OP = R.OP


def P(n, gain=None, null=False, keep=False):
    return (OP["process"], 0, 0.0 if gain is None else gain, n, (R.PF_NULL if null else 0) | (R.PF_GAIN if gain is not None else 0) | (R.PF_KEEP if keep else 0))


def BIND(ch, inp=True, out=True, pos=0):
    return (OP["bind"], ch, 0.0, pos, (R.BF_IN if inp else 0) | (R.BF_OUT if out else 0))


def DES(ch, d):     return (OP["set_designation"], ch, float(d), 0, 0)
def LINK(ch, v):    return (OP["set_link"], ch, v, 0, 0)
def ACT(ch, on):    return (OP["set_active"], ch, 1.0 if on else 0.0, 0, 0)
def W(w):           return (OP["set_weighting"], 0, float(w), 0, 0)
def PER(v):         return (OP["set_period"], 0, v, 0, 0)
def CLR():          return (OP["clear"], 0, 0.0, 0, 0)
def UPD():          return (OP["update_settings"], 0, 0.0, 0, 0)
def SR(rate):       return (OP["set_sample_rate"], 0, 0.0, rate, 0)


_SEED = [1000]


def case(name, kind, channels, a, b, rate, steps, segments=None, amp=0.2):
    n = sum(s[3] for s in steps if s[0] == OP["process"])
    segs = []
    for ch in range(channels):
        _SEED[0] += 1
        spec = (segments or {}).get(ch, [(n, R.NOISE, amp * (1.0 - 0.15 * ch))])
        rest = n - sum(s[0] for s in spec)
        assert rest >= 0, name
        spec = list(spec) + ([(rest, R.NOISE, amp)] if rest else [])
        segs.append([(length, kind_, f32(v), _SEED[0] * 8 + i) for i, (length, kind_, v) in enumerate(spec)])
    return dict(name=name, kind=kind, channels=channels, a=f32(a), b=f32(b), sample_rate=rate, n=n, steps=[(o, c, f32(v), int(l), int(g)) for o, c, v, l, g in steps],
                segments=segs)


def loudness_cases():
    """LoudnessMeter: max_period 20 ms, a ring of 2048 cells at 44100 and 48000 Hz; the counted refresh every 4096 samples."""
    L = lambda name, channels, steps, rate=48000, mp=20.0, **kw: case(name, R.LOUDNESS, channels, mp, 0.0, rate, steps, **kw)
    out = []
    # mono, the default designation; the call lengths; both forms alternating (only the plain one records fLoudness); a call of 0
    # samples after a setter still runs update_settings(); the refresh set at head 0: the counted one finds the window wrapped
    out.append(L("mono lengths forms", 1, [P(1), P(1023, gain=0.5), P(1024), P(1025, gain=2.0), P(4096), PER(10.0), P(0), P(4097, gain=1.0),
                                           P(734)]))
    # stereo, the defaults, one call of 9000 samples, links 0 and in between
    out.append(L("stereo one long call", 2, [LINK(0, 0.0), LINK(1, 0.25), P(9000), P(1000, gain=0.5)], rate=44100))
    # three channels: NONE weighs nothing (the first call reads zero while channels are mixed), then LEFT, the +1.5 dB group, LFE;
    # links 1, in between, 0, and out of range either way
    out.append(L("three designations links", 3, [P(700), DES(0, LEFT), DES(1, 7), DES(2, LFE1), LINK(0, 0.0), LINK(1, 0.5), P(4500, gain=0.5),
                                                 LINK(0, 1.5), LINK(1, -0.5), LINK(2, 0.75), P(2000), DES(2, CENTER), DES(0, CH_NONE), P(2800)]))
    # (the same configuration over other rows: the two run as the meters of one bank)
    out.append(L("three designations links, other rows", 3, list(out[-1]["steps"]), amp=0.05))
    out.append(L("six channels", 6, [DES(0, LEFT), DES(1, RIGHT), DES(2, CENTER), DES(3, LFE1), DES(4, 10), DES(5, 11), LINK(4, 0.0),
                                     LINK(5, 0.3), P(4097), DES(3, 6), DES(0, LFE2), P(4903, gain=0.25)], rate=44100))
    # all six weightings, each one a rebuilt filter with cleared memory; the same one again sets no flag
    out.append(L("weightings", 2, [W(K), P(1500), W(NONE), P(1500), W(A), P(2000, gain=0.5), W(B), P(2000), W(C), P(2000), W(C), P(500),
                                   W(D), P(2000), W(K), P(1500)]))
    # periods: shorter and longer mid-stream (the longer window takes in older squares of the ring), the same value again, 0 (one
    # sample), above the maximum (= the maximum); a period set at head 1500: its counted refresh finds the window in one piece
    out.append(L("periods", 2, [P(1500), PER(5.0), P(4597), PER(20.0), P(1200), PER(20.0), P(300), PER(0.0), P(700, gain=0.5), PER(1000.0),
                                P(5003), PER(7.5), UPD(), P(700)]))
    # set_active off -> on (the line is cleared), on -> on and off -> off (nothing); a channel unbound and bound again (it goes on
    # from where it was); all channels disabled, all unbound (mixed == 0)
    out.append(L("active and bound", 3, [DES(0, LEFT), DES(1, RIGHT), DES(2, 8), LINK(1, 0.0), P(1300), ACT(1, False), ACT(2, True), P(1100),
                                         ACT(1, False), ACT(1, True), P(1025), BIND(0, False, False), P(900, gain=0.5), BIND(0), P(1700),
                                         ACT(0, False), ACT(1, False), ACT(2, False), P(600), ACT(0, True), ACT(1, True), ACT(2, True),
                                         BIND(0, False, False), BIND(1, False, False), BIND(2, False, False), P(500), BIND(0), BIND(1), BIND(2),
                                         P(2875)]))
    # out == NULL; per-channel outputs absent; bind with a position, and calls without rebinding (the inputs are read from where
    # they were bound, the outputs go on from nOffset)
    out.append(L("null out and bind", 2, [LINK(0, 0.0), P(1000, null=True), BIND(1, True, False), P(1200), P(800, gain=0.5, null=True), BIND(1),
                                          BIND(0, True, True, 5), BIND(1, True, True, 0), P(700, keep=True), P(700, keep=True),
                                          P(300, gain=0.5, keep=True), P(4300)]))
    # set_sample_rate to the same rate (nothing) and to another one (new lines, everything cleared, both flags)
    out.append(L("sample rate", 2, [P(2500), SR(48000), P(1500), SR(44100), P(5000), PER(12.0), SR(48000), P(1000)]))
    # noise, a stretch 100 dB down, subnormals, a full-scale step
    quiet = [(2500, R.NOISE, 0.2), (2500, R.NOISE, 2e-6), (1500, R.NOISE, 1e-39), (500, R.CONST, 0.0), (2000, R.CONST, 1.0), (1000, R.CONST, -1.0)]
    out.append(L("levels", 2, [LINK(1, 0.0), P(3000), P(3000, gain=0.5), P(4000)], segments={0: quiet, 1: quiet[:3] + [(3500, R.NOISE, 0.5)]}))
    # clear(): the well-defined sequence (clear, then a forced filter update) and the bare one, of which only nItems is kept
    clr = lambda forced: [LINK(1, 0.0), P(3000), CLR()] + ([W(NONE), W(K)] if forced else []) + [P(1500), P(1500, gain=0.5), ACT(1, False), CLR(), ] + \
                         ([W(A), W(K)] if forced else []) + [P(3000)]
    seed = _SEED[0]
    out.append(L("clear defined", 2, clr(True)))
    _SEED[0] = seed                                                 # the same rows
    out.append(L("clear bare", 2, clr(False)))
    return out


def ilufs_cases():
    """ILUFSMeter: block periods of 4 to 8 ms, quarter blocks of 48 to 96 samples."""
    I = lambda name, channels, steps, max_int=0.05, block=4.0, rate=48000, **kw: case(name, R.ILUFS, channels, max_int, block, rate, steps, **kw)
    out = []
    # mono, 50 gating blocks (a history of 64); calls that end on, one before and one after a quarter block's end
    out.append(I("mono finite 50", 1, [P(48), P(47), P(1), P(49), P(47), P(192), P(191), P(193), P(1024), P(1025), P(4097), P(5086)]))
    # stereo, 90 gating blocks: a history of 96 that is no multiple of 64, wrapped more than twice
    out.append(I("stereo finite 90", 2, [P(4000), P(4097, gain=1.0), P(3903), P(2000, gain=0.0)], max_int=0.09))
    out.append(I("stereo finite 90, other rows", 2, list(out[-1]["steps"]), max_int=0.09, amp=0.03))
    # three channels with an LFE, infinite mode: past 0x100 gating blocks the sums are halved
    out.append(I("three lfe infinite", 3, [DES(0, LEFT), DES(1, 9), DES(2, LFE1), P(5000), P(4097), DES(2, RIGHT), P(4903, gain=1.0)], max_int=0.0))
    out.append(I("three lfe infinite, other rows", 3, list(out[-1]["steps"]), max_int=0.0, amp=0.5))
    out.append(I("mono infinite quiet", 1, [P(3000), P(3000), P(3000, null=True), P(5000)], max_int=0.0, block=5.0,
                 segments={0: [(2500, R.NOISE, 0.15), (3000, R.NOISE, 2e-6), (2000, R.CONST, 0.0), (6500, R.NOISE, 0.1)]}))
    # the integration period: below the block period, above the maximum, shorter and longer mid-stream, the same again
    out.append(I("integration periods", 2, [P(3000), PER(0.001), P(2000), PER(5.0), P(2500), PER(0.03), P(1500, gain=1.0), PER(0.03), P(700),
                                            PER(0.06), UPD(), P(2300)], max_int=0.09))
    # a weighting change mid-block: update_settings() wipes F_BLK_FULL with the other flags, so no block is evaluated until four
    # more quarters have passed; calls shorter than that in a row; a clear() mid-block; set_sample_rate
    out.append(I("weighting clear rate", 2, [P(1000), W(A), P(100), P(100), P(100), P(700), W(K), P(1011), CLR(), P(2000), W(K), P(989),
                                             SR(48000), P(1500), SR(44100), P(4500)], block=8.0, max_int=0.08))
    # set_active, channels without an input, all of them off; stretches below the absolute gate; out == NULL
    out.append(I("active bound gate", 3, [DES(0, LEFT), DES(1, RIGHT), DES(2, 10), P(2000), ACT(1, False), P(1500, null=True), ACT(1, True),
                                          BIND(2, False), P(1500), BIND(2), ACT(0, False), ACT(0, False), P(1000), BIND(0, False), BIND(1, False),
                                          BIND(2, False), P(1000), BIND(0), BIND(1), BIND(2), ACT(0, True), P(5000)],
                 segments={0: [(6000, R.NOISE, 0.2), (2500, R.NOISE, 2e-6), (3500, R.NOISE, 0.2)],
                           1: [(6000, R.NOISE, 0.2), (2500, R.CONST, 0.0), (3500, R.NOISE, 0.1)],
                           2: [(6000, R.NOISE, 0.1), (2500, R.NOISE, 1e-39), (3500, R.NOISE, 0.2)]}))
    return out


def run_driver(exe, cs, timeout=600, may_fail=False):
    """Runs a driver over the cases under a time limit; its standard error must stay empty (a sanitizer writes there)."""
    with tempfile.TemporaryDirectory() as d:
        src, dst = os.path.join(d, "cases.bin"), os.path.join(d, "results.bin")
        with open(src, "wb") as f:
            f.write(R.case_bytes(cs))
        p = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=timeout)
        if exe == LD_SAN and "LeakSanitizer has encountered a fatal error" in p.stderr:
            # the sanitizer twin's leak check needs ptrace, which a build machine may withhold: there, and only there, the run
            # is repeated for the bounds and the undefined arithmetic alone
            p = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=timeout, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
        if p.returncode != 0 or p.stderr.strip():
            if may_fail:
                return None
            raise RuntimeError("%s: exit status %d\n%s" % (exe, p.returncode, p.stderr[-4000:]))
        with open(dst, "rb") as f:
            return f.read()


def gate_margin(loudness):
    return abs(float(loudness) - float(GATING_ABS_THRESH)) / float(GATING_ABS_THRESH)


def run_reference(kind):
    cs = loudness_cases() if kind == R.LOUDNESS else ilufs_cases()
    defined = [c for c in cs if c["name"] != "clear bare"]
    san = run_driver(LD_SAN, defined)
    raw = run_driver(LD_REF, defined)
    assert san == raw, "the sanitizer build computes something else"
    for c, r in zip(defined, R.parse_results(raw, defined)):
        calls = R.walk(c)
        c["step_results"] = r["steps"]
        c["calls"] = r["calls"]
        out = np.concatenate([q["out"] for q in r["calls"]]) if r["calls"] else np.zeros(0, f32)
        for q, call in zip(r["calls"], calls):
            assert [v is not None for v in q["ch_out"]] == (call["have"] if kind == R.LOUDNESS else [False] * c["channels"]), c["name"]
            assert bool(call["flags"] & R.PF_NULL) == bool(len(q["out"]) and np.all(q["out"] == R.SENTINEL)), c["name"]
            q["crc"], q["ch_crc"] = R.crc(q["out"]), [None if v is None else R.crc(v) for v in q["ch_out"]]
        assert np.isfinite(out).all(), c["name"]
        if kind == R.ILUFS:
            c["out_steps"] = R.steps_of(out)
            assert np.array_equal(R.bits(R.from_steps(*c["out_steps"], c["n"])), R.bits(out)), c["name"]
            for q in r["calls"]:                                    # the condition on the inputs, from the reference's own history
                st = R.istate(q, c["channels"])
                live = [(st["ms_head"] + st["ms_size"] - 1 - j) % st["ms_size"] for j in range(st["ms_count"])] if st["ms_int"] > 0 else []
                assert all(gate_margin(st["hist"][i]) >= 0.05 for i in live), (c["name"], "a gating block at the absolute gate")
            margins = []
            R.replay(c, on_call=lambda m, i: margins.append(m.gate_margin))
            assert min(margins) >= 0.05, (c["name"], "a gating block at the absolute gate", min(margins))
        else:
            idx = R.sample_index(c)
            rows_ = [out] + [np.concatenate([v if v is not None else np.full(len(q["out"]), R.SENTINEL, f32) for q in r["calls"] for v in [q["ch_out"][k]]])
                             for k in range(c["channels"])]
            c["samples"] = np.stack([v[idx] for v in rows_]).astype(f32)
    if kind == R.LOUDNESS:
        # the bare clear(): what the plain build gives, if it ends at all; only the facts are kept
        bare, good = [c for c in cs if c["name"] == "clear bare"][0], [c for c in cs if c["name"] == "clear defined"][0]
        got = run_driver(LD_REF, [bare], may_fail=True)
        assert got is not None, "the plain build does not get through the bare clear()"
        r = R.parse_results(got, [bare])[0]
        k_clear = [i for i, s in enumerate([s for s in bare["steps"]]) if s[0] == OP["clear"]][0]
        n_before = sum(1 for s in bare["steps"][:k_clear] if s[0] == OP["process"])
        items = [R.lstate(q, 2)["items"] for q in r["calls"]]
        want = np.concatenate([q["out"] for q in good["calls"]])
        have = np.concatenate([q["out"] for q in r["calls"]])
        differs = int(not np.array_equal(R.bits(want), R.bits(have)))
        bare["bare_clear"] = (items[n_before - 1], items[n_before], differs)
        bare["step_results"] = np.zeros((len(bare["steps"]), 3), np.uint32)
        bare["calls"] = []
    return cs


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


def build_bytes(kind):
    _SEED[0] = 1000 if kind == R.LOUDNESS else 5000
    data = npz_bytes(R.arrays(run_reference(kind)))
    assert len(data) < 400 * 1000, len(data)
    return data


if __name__ == "__main__":
    for kind in (R.LOUDNESS, R.ILUFS):
        data = build_bytes(kind)
        with open(R.FILES[kind], "wb") as f:
            f.write(data)
        print(os.path.basename(R.FILES[kind]), len(R.load(kind)), "cases,", len(data), "bytes")
