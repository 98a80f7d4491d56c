"""The LoudnessMeter and ILUFSMeter banks and the drop-in C++ classes on the device against the REFERENCE'S OWN classes: the results
stored in tests/golden/loudness_ref_vectors.npz and ilufs_ref_vectors.npz (tests/golden/make_loudness_vectors.py; the host side is
tests/test_loudness_reference_host.py).  Nothing here reads the reference tree or oracle/_ref/.

Cases that share a configuration (the same steps over other rows) run as the meters of one bank, the rest have a bank each; the calls
are cut as recorded.  Integers are exact: latency, needs_update, the ILUFS history's size, head and count, the samples at which the
ILUFS output steps.  Floats follow the rules of tests/test_loudness_gpu.py and tests/test_ilufs_gpu.py with the recorded output in
the oracle's place: TOL = 1e-5 of the level (5e-5 under the A, B, C and D curves, whose poles sit at 20 Hz), and for the momentary
meter the mean-square rule of test_random_operation_sequences where the output is small; loudness() to twice (LoudnessMeter) and three
times (ILUFSMeter) that tolerance and the ILUFS history to three times, as those tests have them.

The floats are held with the banks' weighting filters in their exact mode (mi_loudness_bank_set_exact, mi_ilufs_bank_set_exact; the
classes through the process-wide default, MI_DSPU_EXACT_IIR=1): the reference's serial recurrence.  In the default mode, the
time-parallel kernels, every case runs as well: the integers are held exactly, the floats are measured and printed, not held --
three cases miss the bound there by the weighting filter's own round-off, which a meter does not always average away (DESIGN.md
3.6; measured on an MI355X): "periods" (a window of one sample reads |the filter's output| itself) 5.7 times the bound, "levels"
(loudness() behind a full-scale step through the K curve's 38 Hz high-pass, coherent over the window) 9.5 times, "active bound gate"
(gating blocks of the filter's decaying memory after a 100 dB drop) 2.6 times.  The default kernels' floats are held to the oracle
by tests/test_loudness_gpu.py and tests/test_ilufs_gpu.py under the rules they have there.

The samples at which the ILUFS output steps: every step of either row is at a sample the recorded integers allow (a call's start, a
quarter block's end).  A step may be on one side only where each row's own change at that sample is at most one ulp: a gated mean that
moves by an ulp in one arithmetic and by none in the other.  That is an exception to "exact", and the count is printed.

clear(): the reference's LoudnessMeter::clear() leaves its filter bank ill-defined; the product zeroes the filter memory
and the lines and keeps the filter, which is what the reference computes for clear() followed by a forced filter update.  The steps
of the recorded case "clear bare" run here against the recorded results of "clear defined"."""
import ctypes
import os
import subprocess
import time

import numpy as np
import pytest

import loudness_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "lsp-dsp-units_amd")
f32 = np.float32
bits = R.bits
OP, OPS = R.OP, R.OPS
TOL, MS_TOL = 1e-5, 2e-5
pytestmark = pytest.mark.gpu


def _tol(weighting):
    return TOL if weighting in (0, 5) else 5e-5                   # NONE and K; the A, B, C and D curves as the existing tests have them


def _cases(kind):
    """The stored cases; the bare clear() takes the expected values of the well-defined sequence."""
    cs = R.load(kind)
    for c in cs:
        if "bare_clear" in c:
            good = [g for g in cs if g["name"] == "clear defined"][0]
            assert c["bare_clear"][2] == 1                          # the reference itself computes something else there
            c.update(index=good["index"], samples=good["samples"])
            steps = iter(good["step_results"][i] for i, s in enumerate(good["steps"]) if s[0] != OP["set_weighting"])
            calls = iter(good["calls"])
            c["step_results"] = np.array([next(steps) for _ in c["steps"]], np.uint32)
            c["calls"] = [next(calls) for s in c["steps"] if s[0] == OP["process"]]
            # (needs_update differs between the two sequences by the forced update alone: it is compared on the other cases)
            c["skip_pending"] = True
    return cs


@pytest.fixture(scope="module")
def loudness():
    return _cases(R.LOUDNESS)


@pytest.fixture(scope="module")
def ilufs():
    return _cases(R.ILUFS)


def _groups(cases):
    groups = {}
    for c in cases:
        key = (c["channels"], float(c["a"]), float(c["b"]), c["sample_rate"], tuple((s[0], s[1], R.fbits(s[2]), s[3], s[4]) for s in c["steps"]))
        groups.setdefault(key, []).append(c)
    return list(groups.values())


def _judge_loudness(c, got, what, hold=True):
    """got [1 + channels][n] (SENTINEL where nothing was written) against the stored samples, call by call: rule A, the amplitude,
    |got - want| <= tol x the loudest level so far; or rule B, the mean square, |got^2 - want^2| <= (the running sum's floor, or 2e-5
    where the output is below 3 % of that level) x the level's square.  -> the worst ratio to the bound."""
    idx, want = c["index"], c["samples"]
    level, worst, where = 0.0, 0.0, ()
    for call, r in zip(R.walk(c), c["calls"]):
        sel = (idx >= call["pos"]) & (idx < call["pos"] + call["len"])
        if not sel.any():
            continue
        g = float(call["a"]) if call["flags"] & R.PF_GAIN else 1.0
        assert g != 0.0
        judged = ([] if call["flags"] & R.PF_NULL else [0]) + [1 + k for k, h in enumerate(call["have"]) if h]
        for row in range(want.shape[0]):
            if row not in judged:
                assert np.all(want[row][sel] == R.SENTINEL) and np.all(got[row][idx[sel]] == R.SENTINEL), what + (row, "written")
        for row in judged:
            level = max(level, float(np.abs(want[row][sel]).max()) / abs(g))
        tol = _tol(r["weighting"])
        ms_floor = 2.0 ** -24 * np.sqrt(max(4096, R.lstate(r, c["channels"])["period"] >> 2))
        for row in judged:
            w, y = want[row][sel].astype(np.float64), got[row][idx[sel]].astype(np.float64)
            assert np.isfinite(y).all(), what + (row,)
            d_amp, d_ms = np.abs(y - w), np.abs(y * y - w * w) / (g * g)
            small = (w / g) ** 2 < 1e-3 * level * level
            allow_a = tol * level * abs(g)
            allow_b = np.where(small, max(MS_TOL, ms_floor), ms_floor) * level * level
            ratio = np.minimum(d_amp / max(allow_a, 1e-300), d_ms / np.maximum(allow_b, 1e-300))
            i = int(np.argmax(ratio))
            if ratio[i] > worst:
                worst = float(ratio[i])
                where = (row, "call at %d" % call["pos"], "sample %d" % int(idx[sel][i]), "got %.9g want %.9g" % (y[i], w[i]),
                         "|got - want| / level %.3g" % (d_amp[i] / max(level * abs(g), 1e-300)),
                         "|got^2 - want^2| / level^2 %.3g" % (d_ms[i] / max(level * level, 1e-300)))
    print("measured: %s: worst ratio to the bound %.3f %s" % (" ".join(what), worst, " ".join(str(v) for v in where) if worst > 1.0 else ""))
    assert worst <= 1.0 or not hold, what + where
    return worst


def _pending(gpu, bank, name):
    v = ctypes.c_int()
    gpu.check(getattr(gpu.lib, name)(bank.handle, ctypes.byref(v)))
    return v.value


def _run_loudness_bank(gpu, cases, exact):
    c0, M, K = cases[0], len(cases), cases[0]["channels"]
    xs = [R.rows(c) for c in cases]
    bank = gpu.LoudnessBank(M, K, float(c0["a"]))
    bank.set_exact(exact)
    bank.set_sample_rate(c0["sample_rate"])
    calls = {call["step"]: call for call in R.walk(c0)}
    got = [np.full((1 + K, c["n"]), R.SENTINEL, f32) for c in cases]
    level, k_call, worst_loud = [0.0] * M, 0, 0.0
    for si, (op, ch, a, length, flags) in enumerate(c0["steps"]):
        name = OPS[op]
        if name == "process":
            call = calls[si]
            for k in range(K):
                bank.set_bound(k, call["in_at"][k] is not None)
            x = np.concatenate([R.call_input(c, x_, call) for c, x_ in zip(cases, xs)])
            null, gain = bool(flags & R.PF_NULL), (float(a) if flags & R.PF_GAIN else None)
            if length:
                out = None if null else gpu.DeviceBuffer((M, length))
                chb = gpu.DeviceBuffer.from_host(np.full((M * K, length), R.SENTINEL, f32))
                bank.process(out, chb, gpu.DeviceBuffer.from_host(np.ascontiguousarray(x)), length, gain=gain)
                y, yc = (None if null else out.download()), chb.download()
            else:
                bank.process(None, None, gpu.DeviceBuffer((M * K, 1)), 0, gain=gain)
            for m in range(M):
                if length == 0:
                    continue
                lo = call["pos"]
                if not null:
                    got[m][0, lo:lo + length] = y[m]
                for k in range(K):
                    row = yc[m * K + k]
                    if call["active"][k] and call["in_at"][k] is not None:
                        assert not np.any(row == R.SENTINEL), (cases[m]["name"], si, k)
                        if call["have"][k]:
                            got[m][1 + k, lo:lo + length] = row
                    else:
                        assert np.all(row == R.SENTINEL), (cases[m]["name"], si, k, "a channel that is left out was written")
        elif name == "bind":
            pass
        elif name == "set_designation":
            bank.set_designation(ch, int(a))
        elif name == "set_link":
            bank.set_link(ch, float(a))
        elif name == "set_active":
            bank.set_active(ch, a != 0)
        elif name == "set_weighting":
            bank.set_weighting(int(a))
        elif name == "set_period":
            bank.set_period(float(a))
        elif name == "clear":
            bank.clear()
        elif name == "update_settings":
            gpu.check(gpu.lib.mi_loudness_bank_update_settings(bank.handle, None))
        elif name == "set_sample_rate":
            bank.set_sample_rate(length)
        loud = bank.loudness()
        for m, c in enumerate(cases):
            pend, latency, want = (int(v) for v in c["step_results"][si])
            what = (c["name"], "step %d" % si, name)
            assert bank.latency() == latency, what
            if not c.get("skip_pending"):
                assert _pending(gpu, bank, "mi_loudness_bank_needs_update") == pend, what
            want = float(R.from_bits(want))
            level[m] = max(level[m], want)
            tol = _tol(c["calls"][min(k_call, len(c["calls"]) - 1)]["weighting"])
            ratio = abs(float(loud[m]) - want) / (2.0 * tol * max(level[m], 1e-30))
            worst_loud = max(worst_loud, ratio)
            assert ratio <= 1.0 or not exact, what + (float(loud[m]), want)
        k_call += int(name == "process")
    bank.close()
    print("measured: %s bank %s: loudness() worst ratio to the bound %.3f" % (c0["name"], "exact" if exact else "default", worst_loud))
    return max([_judge_loudness(c, g, (c["name"], "bank", "exact" if exact else "default"), hold=exact) for c, g in zip(cases, got)])


LOUDNESS_GROUPS = _groups(_cases(R.LOUDNESS))
ILUFS_GROUPS = _groups(_cases(R.ILUFS))


def test_cases_that_share_a_configuration_share_a_bank():
    for groups, count in ((LOUDNESS_GROUPS, 13), (ILUFS_GROUPS, 9)):
        assert any(len(g) > 1 for g in groups) and sum(len(g) for g in groups) >= count


@pytest.mark.parametrize("group", LOUDNESS_GROUPS, ids=[g[0]["name"].replace(" ", "_") for g in LOUDNESS_GROUPS])
@pytest.mark.parametrize("exact", [True, False], ids=["exact", "default"])
def test_loudness_bank_gives_the_references_output_and_integers(gpu, group, exact):
    """exact: integers and floats held.  default: integers held, floats measured and printed (the module's docstring)."""
    t0 = time.perf_counter()
    _run_loudness_bank(gpu, group, exact)
    print("measured: %.2f s" % (time.perf_counter() - t0))


def _judge_ilufs(c, out, what, hold=True):
    """The whole output row against the recording.  The samples at which the output may step are integers of the recording: a call's
    first sample and the ends of the quarter blocks, counted back from the call's end by the recorded nBlockOffset and nBlockSize.
    Every step of the recording and every step of `out` is at one of them, and where one of the two rows steps the other does too
    unless its own values on either side are the same float: a gated mean that moves by less than an ulp in one arithmetic and by
    one ulp in the other is no step at another sample (the values themselves are held to tol x the case's peak below)."""
    want = c["out"]
    at_w, at_g = (set(int(v) for v in R.steps_of(row)[0]) for row in (want, out))
    allowed = set()
    for call, r in zip(R.walk(c), c["calls"]):
        st = R.istate(r, c["channels"])
        lo, p = call["pos"], call["pos"] + call["len"] - st["block_offset"]
        allowed.add(lo)
        while p > lo:
            allowed.add(p)
            p -= st["block_size"]
    assert at_w <= allowed and at_g <= allowed, what + ("the output steps elsewhere", sorted(at_g - allowed)[:8], sorted(at_w - allowed)[:8])
    one_sided = sorted(at_w ^ at_g)
    print("measured: %s: %d steps recorded, %d on one side only %s" % (" ".join(what), len(at_w), len(one_sided), one_sided[:8]))
    ulp = lambda v: float(np.spacing(np.abs(f32(v))))
    for p_ in one_sided if hold else ():
        assert abs(float(want[p_]) - float(want[p_ - 1])) <= ulp(want[p_]) and abs(float(out[p_]) - float(out[p_ - 1])) <= ulp(out[p_]), \
            what + ("a step on one side only", p_, float(want[p_ - 1]), float(want[p_]), float(out[p_ - 1]), float(out[p_]))
    keep = want != R.SENTINEL
    assert np.array_equal(keep, out != R.SENTINEL), what
    peak = float(np.abs(want[keep]).max())
    assert peak > 0
    worst, where = 0.0, ()
    for call, r in zip(R.walk(c), c["calls"]):
        lo, hi = call["pos"], call["pos"] + call["len"]
        if call["flags"] & R.PF_NULL or hi == lo:
            continue
        err = np.abs(out[lo:hi].astype(np.float64) - want[lo:hi])
        i = int(np.argmax(err))
        ratio = float(err[i]) / (_tol(r["weighting"]) * peak)
        if ratio > worst:
            worst, where = ratio, ("call at %d" % lo, "sample %d" % (lo + i), "got %.9g want %.9g" % (out[lo + i], want[lo + i]), "|got - want| / peak %.3g" % (err[i] / peak))
    print("measured: %s: worst ratio to the bound %.3f %s" % (" ".join(what), worst, " ".join(where) if worst > 1.0 else ""))
    assert worst <= 1.0 or not hold, what + where
    return worst


def _run_ilufs_bank(gpu, cases, exact):
    c0, M, K = cases[0], len(cases), cases[0]["channels"]
    xs = [R.rows(c) for c in cases]
    bank = gpu.ILUFSBank(M, K, float(c0["a"]), float(c0["b"]))
    bank.set_exact(exact)
    bank.set_sample_rate(c0["sample_rate"])
    calls = {call["step"]: call for call in R.walk(c0)}
    got = [np.full(c["n"], R.SENTINEL, f32) for c in cases]
    level = [0.0] * M
    k_call, worst_loud, worst_hist = 0, 0.0, 0.0
    on = [True] * K
    for si, (op, ch, a, length, flags) in enumerate(c0["steps"]):
        name = OPS[op]
        if name == "process":
            call = calls[si]
            for k in range(K):                              # a channel takes part when it is enabled AND has an input (ILUFSMeter.cpp:370)
                want_on = bool(call["active"][k] and call["in_at"][k] is not None)
                if want_on != on[k]:
                    bank.set_active(k, want_on)
                    on[k] = want_on
            x = np.concatenate([R.call_input(c, x_, call) for c, x_ in zip(cases, xs)])
            null = bool(flags & R.PF_NULL)
            out = None if null else gpu.DeviceBuffer((M, length))
            bank.process(out, gpu.DeviceBuffer.from_host(np.ascontiguousarray(x)), length, gain=float(a) if flags & R.PF_GAIN else float(R.DEFAULT_GAIN))
            if not null:
                y = out.download()
                for m in range(M):
                    got[m][call["pos"]:call["pos"] + length] = y[m]
        elif name in ("bind", "set_active"):
            pass                                            # walk() has both
        elif name == "set_designation":
            bank.set_designation(ch, int(a))
        elif name == "set_weighting":
            bank.set_weighting(int(a))
        elif name == "set_period":
            bank.set_integration_period(float(a))
        elif name == "clear":
            bank.clear()
        elif name == "update_settings":
            gpu.check(gpu.lib.mi_ilufs_bank_update_settings(bank.handle, None))
        elif name == "set_sample_rate":
            bank.set_sample_rate(length)
        loud = bank.loudness()
        hist, head, count = bank.history()
        for m, c in enumerate(cases):
            pend, _, want = (int(v) for v in c["step_results"][si])
            what = (c["name"], "step %d" % si, name)
            assert _pending(gpu, bank, "mi_ilufs_bank_needs_update") == pend, what
            want = float(R.from_bits(want))
            level[m] = max(level[m], want)
            tol = _tol(c["calls"][min(k_call, len(c["calls"]) - 1)]["weighting"])
            ratio = abs(float(loud[m]) - want) / (3 * tol * max(level[m], 1e-30))
            worst_loud = max(worst_loud, ratio)
            assert ratio <= 1.0 or not exact, what + (float(loud[m]), want)
            if name == "process":
                st = R.istate(c["calls"][k_call], K)
                assert (hist.shape[1], int(head[m]), int(count[m])) == (st["ms_size"], st["ms_head"], st["ms_count"]), what
                ratio = float(np.abs(hist[m].astype(np.float64) - st["hist"]).max()) / max(3 * tol * max(level[m] ** 2, float(st["hist"].max())), 1e-300)
                worst_hist = max(worst_hist, ratio)
                assert ratio <= 1.0 or not exact, what + ("history",)
        k_call += int(name == "process")
    bank.close()
    print("measured: %s bank %s: worst ratio to the bound %.3f (loudness()), %.3f (history)" % (c0["name"], "exact" if exact else "default", worst_loud, worst_hist))
    return max([_judge_ilufs(c, g, (c["name"], "bank", "exact" if exact else "default"), hold=exact) for c, g in zip(cases, got)])


@pytest.mark.parametrize("group", ILUFS_GROUPS, ids=[g[0]["name"].replace(" ", "_") for g in ILUFS_GROUPS])
@pytest.mark.parametrize("exact", [True, False], ids=["exact", "default"])
def test_ilufs_bank_gives_the_references_output_and_integers(gpu, group, exact):
    """exact: integers and floats held.  default: integers held, floats measured and printed (the module's docstring)."""
    t0 = time.perf_counter()
    _run_ilufs_bank(gpu, group, exact)
    print("measured: %.2f s" % (time.perf_counter() - t0))


# ---- the drop-in C++ classes ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def class_results(gpu, loudness, ilufs, tmp_path_factory):
    """oracle/loudness_driver.cpp compiled against the product's headers and library, run over every recorded case, in a process
    whose biquad banks start in the exact mode (MI_DSPU_EXACT_IIR=1, how a host chooses for the class layer) and in one with the
    default."""
    data = loudness + ilufs
    d = tmp_path_factory.mktemp("loudness_class")
    exe = str(d / "loudness_class")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-I" + os.path.join(PKG, "include"), "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "oracle", "loudness_driver.cpp"), "-o", exe, "-L" + PKG, "-lmi_dspu", "-Wl,-rpath," + PKG,
                           "-Wl,-rpath,/opt/rocm/lib"])
    (d / "cases.bin").write_bytes(R.case_bytes(data))
    results = {}
    for exact in (True, False):
        env = {k: v for k, v in os.environ.items() if k != "MI_DSPU_EXACT_IIR"}
        if exact:
            env["MI_DSPU_EXACT_IIR"] = "1"
        t0 = time.perf_counter()
        dst = str(d / ("results_%d.bin" % exact))
        out = subprocess.run([exe, str(d / "cases.bin"), dst], capture_output=True, text=True, timeout=120, env=env)
        assert out.returncode == 0, out
        print("measured: the classes over %d cases in %.2f s (%s)" % (len(data), time.perf_counter() - t0, "exact" if exact else "default"))
        with open(dst, "rb") as f:
            results[exact] = R.parse_results(f.read(), data, reference=False)
    return data, results


ALL_CASES = [c["name"] for g in LOUDNESS_GROUPS + ILUFS_GROUPS for c in g]


@pytest.mark.parametrize("name", ALL_CASES, ids=[n.replace(" ", "_").replace(",", "") for n in ALL_CASES])
@pytest.mark.parametrize("exact", [True, False], ids=["exact", "default"])
def test_cpp_classes_give_the_references_output_getters_and_integers(class_results, name, exact):
    """exact: integers, getters and floats held.  default: integers and getters held, floats measured and printed."""
    data, results = class_results
    results = results[exact]
    c, r = [(c, r) for c, r in zip(data, results) if c["name"] == name][0]
    K = c["channels"]
    assert len(r["calls"]) == len(c["calls"])
    level = 0.0
    k_call = 0
    for si, (s, got, want) in enumerate(zip(c["steps"], r["steps"], c["step_results"])):
        what = (c["name"], "step %d" % si, OPS[s[0]])
        if not c.get("skip_pending"):
            assert int(got[0]) == int(want[0]), what + ("needs_update",)
        assert int(got[1]) == int(want[1]), what + ("latency",)
        g, w = float(R.from_bits(got[2])), float(R.from_bits(want[2]))
        level = max(level, w)
        tol = _tol(c["calls"][min(k_call, len(c["calls"]) - 1)]["weighting"])
        assert abs(g - w) <= (2.0 if c["kind"] == R.LOUDNESS else 3.0) * tol * max(level, 1e-30) or not exact, what + ("loudness()", g, w)
        k_call += int(s[0] == OP["process"])
    for i, (got, want) in enumerate(zip(r["calls"], c["calls"])):
        for key in ("designation", "link", "active"):
            assert np.array_equal(got[key], want[key]), (c["name"], "call %d" % i, key)
        assert (got["weighting"], got["period"], got["sample_rate"]) == (want["weighting"], want["period"], want["sample_rate"]), (c["name"], i)
    out = np.concatenate([q["out"] for q in r["calls"]])
    if c["kind"] == R.ILUFS:
        _judge_ilufs(c, out, (c["name"], "class", "exact" if exact else "default"), hold=exact)
    else:
        rows_ = [out] + [np.concatenate([v if v is not None else np.full(len(q["out"]), R.SENTINEL, f32) for q in r["calls"] for v in [q["ch_out"][k]]])
                         for k in range(K)]
        _judge_loudness(c, np.stack(rows_), (c["name"], "class", "exact" if exact else "default"), hold=exact)
