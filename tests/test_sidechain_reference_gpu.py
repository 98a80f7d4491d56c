"""The Sidechain bank and the drop-in C++ class on the device against the REFERENCE'S OWN class: the results stored in
tests/golden/sidechain_ref_vectors.npz (tests/golden/make_sidechain_vectors.py; the host side is
tests/test_sidechain_reference_host.py).  Nothing here reads the reference tree or oracle/_ref/.

One channel per case, the shorter cases padded with zeros, the calls cut at the union of the cases' cuts, the setter events applied
per channel ahead of the call they were recorded ahead of.  A channel whose get_params() equals the recorded parameters in every bit
ahead of every one of its calls takes the DIRECT path: its output, fRmsValue, nRefresh and the ring position after every call are
the reference's bits.  A libm that rounds fTau differently would move an LPF channel to the FALLBACK: the restatement fed the
library's own parameters.  Each test fails unless three quarters of its cases are direct, and every case that is never in LPF mode
has to be.  process(out, NULL, n) holds for a whole bank, so a case with such a call has a bank of its own.  The ring's samples
cannot be read back from the bank: they are held through the outputs that depend on them."""
import os
import subprocess
import time

import numpy as np
import pytest

import sidechain_ref as ref
import sidechain_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "lsp-dsp-units_amd")
f32 = np.float32
bits = R.bits
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def data():
    """Every case but the single-sample one of 8300 samples, which is 8300 calls: the host test holds the restatement to it."""
    return [c for c in R.load() if not (c["single"] and c["n"] > R.WHOLE)]


def _report(what, cases, directs):
    n = int(np.count_nonzero(directs))
    print("%s: %d of %d cases on the direct path (parameters bit-identical to the reference's)" % (what, n, len(directs)))
    assert 4 * n >= 3 * len(directs), (what, n, len(directs))
    assert all(d for c, d in zip(cases, directs) if not c["lpf"]), [c["name"] for c, d in zip(cases, directs) if not (c["lpf"] or d)]


def _apply(bank, ch, setter, a):
    if setter == "clear":
        bank.clear(ch)
    elif setter in ("set_reactivity", "set_gain"):
        getattr(bank, setter)(ch, float(a))
    else:
        getattr(bank, setter)(ch, int(a))


def _recorded(c):
    """Per call the recorded (nReactivity, fTau, capacity, mid-side flag); a single-sample case keeps the last row only, and its
    windows come from the restatement's integer arithmetic (fTau: None where an event changes it; no such case is in LPF mode)."""
    if not c["single"]:
        return [(p["reactivity"], p["tau"], p["capacity"], int(f) & 1) for p, f in zip(R.recorded_params(c), R.column(c, "flags"))]
    st = R.Settings(c)
    assert not (c["events"] and c["lpf"])
    return [(p["reactivity"], None if c["events"] else p["tau"], p["capacity"], st.flags & 1) for p in R.single_params(c)]


def _run_bank(gpu, cases, premixed):
    """The cases as the channels of one bank -> direct per case."""
    inputs, C, N = cases[0]["inputs"], len(cases), max(c["n"] for c in cases)
    ends = [np.cumsum(c["calls"]) for c in cases]
    starts = [{int(e - m): k for k, (e, m) in enumerate(zip(en, c["calls"]))} for en, c in zip(ends, cases)]
    cuts = sorted({int(e) for en in ends for e in en})
    x0, x1 = np.zeros((C, N), f32), np.zeros((C, N), f32)
    bank = gpu.SidechainBank(C, inputs, float(cases[0]["max_reactivity"]))
    for ch, c in enumerate(cases):
        x0[ch, :c["n"]] = c["in0"]
        if inputs == 2:
            x1[ch, :c["n"]] = c["in1"]
        bank.configure(ch, c["sample_rate"], float(c["reactivity"]), c["mode"], c["source"], c["stereo"], float(c["gain"]))
    got = np.zeros((C, N), f32)
    params, states = [[] for _ in cases], [[] for _ in cases]
    pos = 0
    for cut in cuts:
        m, null = cut - pos, False
        for ch, c in enumerate(cases):
            k = starts[ch].get(pos)
            if k is not None:
                for setter, a in R.events_before(c, k):
                    _apply(bank, ch, setter, a)
                null = null or bool(c["null"][k])
        assert not null or C == 1
        bank.update_settings()
        for ch in range(C):
            if pos in starts[ch]:
                params[ch].append(bank.get_params(ch))
        d0 = gpu.DeviceBuffer.from_host(np.ascontiguousarray(x0[:, pos:cut]))
        d1 = gpu.DeviceBuffer.from_host(np.ascontiguousarray(x1[:, pos:cut])) if inputs == 2 else None
        dout = gpu.DeviceBuffer((C, m))
        if null:
            bank.process(dout, None, None, m)
        elif premixed:
            mix = gpu.DeviceBuffer((C, m))
            bank.premix(mix, d0, d1, m)
            bank.process_premixed(dout, mix, m)
        else:
            bank.process(dout, d0, d1, m)
        got[:, pos:cut] = dout.download()
        for ch in range(C):
            if cut in ends[ch]:
                states[ch].append(bank.get_state(ch))
        pos = cut
    bank.close()

    directs = []
    for ch, c in enumerate(cases):
        what = (c["name"], "premixed" if premixed else "process")
        p = params[ch]
        assert len(p) == len(c["calls"]) == len(states[ch])
        assert all(bits(q["interval"]) == bits(f32(1.0) / f32(q["reactivity"])) for q in p), what
        direct = all((q["reactivity"], q["capacity"], q["flags"] & 1) == (w[0], w[2], w[3]) and (w[1] is None or bits(q["tau"]) == bits(w[1]))
                     for q, w in zip(p, _recorded(c)))
        directs.append(direct)
        out = got[ch, :c["n"]]
        if direct:
            assert c["out"].mismatch(out) is None, what + (c["out"].mismatch(out),)
            rows = c["state"]
        else:
            want, rows, _, _ = R.replay(c, [dict(reactivity=q["reactivity"], tau=q["tau"], interval=q["interval"], capacity=q["capacity"]) for q in p])
            assert np.array_equal(bits(out), bits(want)), what + ("fallback", np.flatnonzero(bits(out) != bits(want))[:4])
        calls = [len(c["calls"]) - 1] if c["single"] and direct else range(len(c["calls"]))
        for k in calls:
            row = rows[0 if c["single"] and direct else k]
            rms, refresh, head = states[ch][k]
            assert (int(bits(rms)[0]), refresh, head) == (int(row[3]), int(row[2]), int(row[6])), what + (direct, "state after call %d" % k)
    return directs


def _groups(cases):
    """The cases that can share a bank: by number of inputs, a case with an in == NULL call alone, the single-sample cases (a call
    per sample) among themselves."""
    groups = {}
    for i, c in enumerate(cases):
        groups.setdefault((c["inputs"], bool(c["single"]), i if any(c["null"]) else -1), []).append(c)
    return list(groups.values())


@pytest.mark.parametrize("premixed", [False, True], ids=["process", "premix_process_premixed"])
def test_bank_gives_the_references_output_and_state(gpu, data, premixed):
    t0 = time.perf_counter()
    cases, directs = [], []
    for group in _groups(data):
        cases += group
        directs += _run_bank(gpu, group, premixed)
    _report("SidechainBank", cases, directs)
    assert len(cases) == len(data) >= 80
    print("measured: %.2f s" % (time.perf_counter() - t0))


def test_bank_set_sample_rate_takes_the_channel_back_to_stereo(gpu, data):
    """Sidechain.cpp:91 assigns nFlags, so the mid-side flag goes: the recording shows it, and the bank's flags follow."""
    c = [c for c in data if c["name"] == "sample rate midside"][0]
    assert list(R.column(c, "flags")) == [1, 1, 0, 0, 0]
    bank = gpu.SidechainBank(1, 2, float(c["max_reactivity"]))
    bank.configure(0, c["sample_rate"], float(c["reactivity"]), c["mode"], c["source"], c["stereo"], float(c["gain"]))
    bank.update_settings()
    assert bank.get_params(0)["flags"] == gpu.SidechainBank.SCF_MIDSIDE
    bank.set_sample_rate(0, 96000)
    assert bank.get_params(0)["flags"] == gpu.SidechainBank.SCF_UPDATE | gpu.SidechainBank.SCF_CLEAR
    bank.update_settings()
    assert bank.get_params(0)["flags"] == 0 and bank.get_state(0) == (0.0, 0, 0)
    bank.close()


# ---- the drop-in C++ class ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def class_results(gpu, tmp_path_factory):
    """oracle/sidechain_driver.cpp compiled against the product's headers and library, run over EVERY recorded case: the
    single-sample one of 8300 samples too, so process(const float *) crosses a counted refresh on the device."""
    data = R.load()
    d = tmp_path_factory.mktemp("sidechain_class")
    exe = str(d / "sidechain_class")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-I" + os.path.join(PKG, "include"), "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "oracle", "sidechain_driver.cpp"), "-o", exe, "-L" + PKG, "-lmi_dspu", "-Wl,-rpath," + PKG,
                           "-Wl,-rpath,/opt/rocm/lib"])
    (d / "cases.bin").write_bytes(R.case_bytes(data))
    t0 = time.perf_counter()
    out = subprocess.run([exe, str(d / "cases.bin"), str(d / "results.bin")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out
    print("measured: the class over %d cases in %.2f s" % (len(data), time.perf_counter() - t0))
    return data, R.parse_results((d / "results.bin").read_bytes(), data, reference=False)


def test_cpp_class_gives_the_references_output_and_state(class_results):
    data, class_results = class_results
    directs = []
    for c, r in zip(data, class_results):
        got = r["state"][-1:] if c["single"] else r["state"]
        want = c["state"]
        cols = [R.STATE.index(k) for k in ("reactivity", "tau", "capacity", "flags")]
        direct = np.array_equal(got[:, cols], want[:, cols])
        directs.append(direct)
        if direct:
            assert c["out"].mismatch(r["out"]) is None, (c["name"], c["out"].mismatch(r["out"]))
            rows = want
        else:
            assert c["lpf"] and not c["single"], c["name"]
            tau = r["state"][:, 1].copy().view(f32)
            params = [dict(p, tau=t) for p, t in zip(R.recorded_params(c), tau)]
            out, rows, _, _ = R.replay(c, params)
            assert np.array_equal(bits(out), bits(r["out"])), (c["name"], "fallback")
        for name in ("reactivity", "refresh", "rms", "flags", "capacity", "head"):
            k = R.STATE.index(name)
            assert np.array_equal(got[:, k], rows[:, k]), (c["name"], direct, name, got[:, k], rows[:, k])
    _report("Sidechain class", data, directs)


def test_cpp_class_single_sample_overload_is_the_block_path(class_results):
    """What Sidechain.h documents: process(const float *) is one sample through the block path.  It gives the recorded calls of
    length 1 bit for bit (and the recorded single-sample results where the reference's two overloads agree: PEAK and LPF); in RMS
    and UNIFORM it differs from the recorded single-sample results, by the division and the order of the sum that
    tests/test_sidechain_reference_host.py shows on the same recordings."""
    data, class_results = class_results
    seen = 0
    for c, r in zip(data, class_results):
        if not c["single"]:
            continue
        seen += 1
        assert np.array_equal(bits(r["single_out"]), bits(r["out"])), c["name"]
        tau_same = r["state"][-1, 1] == c["state"][-1, 1]
        if c["mode"] != ref.SCM_LPF or tau_same:
            assert c["out"].mismatch(r["single_out"]) is None, c["name"]
        if c["mode"] == ref.SCM_PEAK or (c["mode"] == ref.SCM_LPF and tau_same):
            assert c["single_out"].mismatch(r["single_out"]) is None, c["name"]
        elif c["mode"] != ref.SCM_LPF:
            assert c["single_out"].mismatch(r["single_out"]) is not None, c["name"]
    assert seen == 5 and any(c["single"] and c["n"] > ref.REFRESH_RATE for c in data)
