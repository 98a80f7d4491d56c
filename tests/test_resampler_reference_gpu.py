"""The TruePeak bank and the drop-in C++ class on the device against the REFERENCE'S OWN class: the results stored in
tests/golden/truepeak_ref_vectors.npz (tests/golden/make_resampler_vectors.py; the host side is
tests/test_resampler_reference_host.py).  Nothing here reads the reference tree or oracle/_ref/.  No libm is involved, so every case
is held to the reference's bits directly.  A bank has one sample rate, so the cases of one rate and the same events share a bank,
one channel each.  The second half holds the Oversampler bank and class to tests/golden/oversampler_ref_vectors.npz."""
import os
import subprocess
import time

import numpy as np
import pytest

import resampler_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "lsp-dsp-units_amd")
f32 = np.float32
bits = R.bits
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def data():
    return R.load()


def _groups(cases):
    groups = {}
    for c in cases:
        groups.setdefault((c["sample_rate"], tuple(c["calls"]), tuple(c["events"])), []).append(c)
    return list(groups.values())


def _run_bank(gpu, cases):
    """The cases as the channels of one bank: process() out of place and in place bit for bit, process_max() the recorded maximum
    of process(), latency() and oversampling() after every call."""
    c0, C = cases[0], len(cases)
    bank = gpu.TruePeakBank(C)
    bank.set_sample_rate(c0["sample_rate"])
    x = np.stack([c["x"] for c in cases])
    want = np.stack([c["out"] for c in cases])
    pos = 0
    for i, (n, kind) in enumerate(c0["calls"]):
        for before, setter, a in c0["events"]:
            if before == i:
                bank.set_sample_rate(a) if setter == "set_sample_rate" else bank.clear()
        what = (c0["name"], "call %d" % i, kind)
        din = gpu.DeviceBuffer.from_host(np.ascontiguousarray(x[:, pos:pos + n]))
        if kind == "process_max":
            peaks = gpu.DeviceBuffer((C,))
            bank.process_max(peaks, din, n)
            got = peaks.download().reshape(C)
            maxima = np.array([R.call_maxima(c)[i] for c in cases], f32)
            assert np.array_equal(bits(got), bits(maxima)), what + (got, maxima)
        else:
            dout = din if kind == "in_place" else gpu.DeviceBuffer((C, n))
            bank.process(dout, din, n)
            got = dout.download()
            bad = np.argwhere(bits(got) != bits(want[:, pos:pos + n]))
            assert len(bad) == 0, what + (bad[:4],)
        assert bank.latency() == R.column(c0, "latency")[i] and bank.oversampling() == R.column(c0, "times")[i], what
        pos += n
    bank.close()


def test_bank_gives_the_references_true_peaks(gpu, data):
    t0 = time.perf_counter()
    groups = _groups(data)
    assert sorted(len(g) for g in groups) == [1] * 5 + [4] * 6          # one bank per factor, four signals; the event cases alone
    for g in groups:
        _run_bank(gpu, g)
    print("measured: %.2f s" % (time.perf_counter() - t0))


def test_bank_process_max_deviates_from_the_references_return_value_as_documented(gpu, data):
    """The reference returns 0.0f from process_max() with oversampling on (TruePeakMeter.cpp:271; recorded).  The bank returns the
    largest value process() writes for the block (include/mi_dspu.h, TruePeakMeter.h): a deliberate, documented deviation."""
    c = [c for c in data if c["name"] == "4x noise"][0]
    i = [k for k, (n, kind) in enumerate(c["calls"]) if kind == "process_max"][0]
    assert bits(R.column(c, "returned")[i]) == 0 and R.call_maxima(c)[i] > 0.5
    bank = gpu.TruePeakBank(1)
    bank.set_sample_rate(c["sample_rate"])
    pos, peaks = 0, gpu.DeviceBuffer((1,))
    for k in range(i + 1):
        n = c["calls"][k][0]
        bank.process_max(peaks, gpu.DeviceBuffer.from_host(np.ascontiguousarray(c["x"][None, pos:pos + n])), n)
        pos += n
    got = peaks.download().reshape(1)[0]
    assert bits(got) == bits(R.call_maxima(c)[i]) and bits(got) != bits(R.column(c, "returned")[i])
    bank.close()


@pytest.fixture(scope="module")
def class_results(gpu, data, tmp_path_factory):
    """oracle/truepeak_driver.cpp compiled against the product's headers and library, run over the recorded cases."""
    d = tmp_path_factory.mktemp("truepeak_class")
    exe = str(d / "truepeak_class")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-I" + os.path.join(PKG, "include"), "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "oracle", "truepeak_driver.cpp"), "-o", exe, "-L" + PKG, "-lmi_dspu", "-Wl,-rpath," + PKG,
                           "-Wl,-rpath,/opt/rocm/lib"])
    (d / "cases.bin").write_bytes(R.case_bytes(data, {}))
    t0 = time.perf_counter()
    out = subprocess.run([exe, str(d / "cases.bin"), str(d / "results.bin")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out
    print("measured: the class over %d cases in %.2f s" % (len(data), time.perf_counter() - t0))
    return R.parse_results((d / "results.bin").read_bytes(), data)


def test_cpp_class_gives_the_references_true_peaks(data, class_results):
    for c, r in zip(data, class_results):
        assert np.array_equal(bits(r["out"]), bits(c["out"])), (c["name"], np.flatnonzero(bits(r["out"]) != bits(c["out"]))[:4])
        assert np.array_equal(r["state"][:, 0], R.column(c, "latency")), c["name"]
        pos = 0
        for i, (n, kind) in enumerate(c["calls"]):
            if kind == "process_max":           # the documented deviation: the block's maximum, where the reference returns 0.0f
                assert r["state"][i, 1] == bits(R.call_maxima(c)[i])[0], (c["name"], i)
            else:                               # out of place and in place
                assert np.array_equal(bits(r["own"][pos:pos + n]), bits(c["out"][pos:pos + n])), (c["name"], i, kind)
            pos += n


# ---- Oversampler ------------------------------------------------------------------------------------------------------------
# The recordings were made with a filter that copies: what the Oversampler ASKS of its filter is compared (get_filter() against the
# recorded update requests), and the samples are compared where the filter does not act.  A case that runs process() with filtering
# on (the recorded filter copies, so filtering equals the unfiltered path) runs here with filtering off; a downsample step with
# filtering on runs, for what it does to the state, and its samples are not compared: the real filter is held to the biquad oracle
# by tests/test_oversampler_gpu.py.
@pytest.fixture(scope="module")
def os_data():
    return R.os_load()


def _unfiltered(case):
    """The case's steps with process() cases switched to filtering off -> (steps, whether `modified` still is the recorded one)."""
    if not any(op == "process" for op, _ in case["steps"]):
        return case["steps"], True
    return [("set_filtering", 0) if op == "set_filtering" else (op, a) for op, a in case["steps"]], False


def _compare(stored, got, skip, what):
    if not skip.any():
        assert stored.mismatch(got) is None, what + (stored.mismatch(got),)
    else:
        assert stored.n <= 2000, what                   # stored whole
        bad = np.flatnonzero((bits(got) != bits(stored.whole)) & ~skip)
        assert len(bad) == 0 and (~skip).sum() >= stored.n // 4, what + (bad[:4],)


def _filter_bits(fp):
    return (fp["nType"], fp["nSlope"]) + tuple(int(bits(fp[k])[0]) for k in ("fFreq", "fFreq2", "fGain", "fQuality"))


def _scale_callback(gpu, channels, factor):
    """A device callback without another runtime: a one-section biquad bank y = factor * x + 0 in the exact mode, enqueued in place
    on the stream it is given (what the driver's callback computes on the host)."""
    scaler = gpu.BiquadBank(channels, 1)
    scaler.set_exact(True)
    scaler.set_all_chains(np.broadcast_to(np.array([factor, 0, 0, 0, 0], f32), (channels, 1, 5)))

    def cb(buf, samples, stride, ch, stream):
        scaler.process(buf, buf, samples, out_stride=stride, in_stride=stride, stream=stream or None)
    cb.bank = scaler
    return cb


def _run_oversampler_bank(gpu, case, C=2):
    steps, same_modified = _unfiltered(case)
    bank = gpu.OversamplerBank(C)
    cb = _scale_callback(gpu, C, -0.5)
    x = np.tile(case["x"], (C, 1))
    up, down, up_skip, down_skip = [], [], [], []
    pos, last, filt, request = 0, None, True, None
    for k, (op, a) in enumerate(steps):
        what = (case["name"], "step %d" % k, op, a)
        if op == "set_mode":
            bank.set_mode(a)
        elif op == "set_sample_rate":
            bank.set_sample_rate(a)
        elif op == "set_filtering":
            bank.set_filtering(bool(a))
            filt = bool(a)
        elif op == "update_settings":
            bank.update_settings()
        elif op == "upsample":
            last = gpu.DeviceBuffer((C, a * bank.oversampling()))
            bank.upsample(last, gpu.DeviceBuffer.from_host(np.ascontiguousarray(x[:, pos:pos + a])), a)
            up.append(last.download())
            pos += a
        elif op == "downsample":
            out = gpu.DeviceBuffer((C, a))
            bank.downsample(out, last, a)
            down.append(out.download())
            down_skip.append(np.full(a, filt))
        else:
            out = gpu.DeviceBuffer((C, a))
            bank.process(out, gpu.DeviceBuffer.from_host(np.ascontiguousarray(x[:, pos:pos + a])), a, callback=cb)
            down.append(out.download())
            down_skip.append(np.full(a, filt))
            pos += a
        assert (bank.oversampling(), bank.latency()) == tuple(int(v) for v in case["state"][k, :2]), what
        assert not same_modified or int(bank.modified()) == case["state"][k, 2], what
        # the design request: the last update() the reference's filter got
        for clear, rate, fp in R.os_calls(case, k):
            request = request if clear else (rate, fp)
        if op in ("set_sample_rate", "update_settings") and request is not None and request[1][0] != 0:
            got, rate = bank.get_filter()
            assert (rate, _filter_bits(got)) == request, what + (rate, got, request)
    bank.close()
    for ch in range(C):
        if up:
            _compare(case["up"], np.concatenate([u[ch] for u in up]), np.zeros(case["up"].n, bool), (case["name"], "up", ch))
        if down:
            _compare(case["down"], np.concatenate([d[ch] for d in down]), np.concatenate(down_skip), (case["name"], "down", ch))


def test_oversampler_bank_gives_the_references_samples_and_filter_requests(gpu, os_data):
    t0 = time.perf_counter()
    for c in os_data:
        _run_oversampler_bank(gpu, c)
    assert len(os_data) == 36
    print("measured: %.2f s" % (time.perf_counter() - t0))


@pytest.fixture(scope="module")
def os_class_results(gpu, os_data, tmp_path_factory):
    """oracle/oversampler_driver.cpp compiled against the product's headers and library, run over the recorded cases (process()
    cases with filtering off, see above)."""
    d = tmp_path_factory.mktemp("oversampler_class")
    exe = str(d / "oversampler_class")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-ffp-contract=off", "-I" + os.path.join(PKG, "include"), "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "oracle", "oversampler_driver.cpp"), "-o", exe, "-L" + PKG, "-lmi_dspu", "-Wl,-rpath," + PKG,
                           "-Wl,-rpath,/opt/rocm/lib"])
    cases = [dict(c, steps=_unfiltered(c)[0]) for c in os_data]
    (d / "cases.bin").write_bytes(R.os_case_bytes(cases, {}))
    t0 = time.perf_counter()
    out = subprocess.run([exe, str(d / "cases.bin"), str(d / "results.bin")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out
    print("measured: the class over %d cases in %.2f s" % (len(cases), time.perf_counter() - t0))
    return R.os_parse_results((d / "results.bin").read_bytes(), cases)


def test_oversampler_cpp_class_gives_the_references_samples(os_data, os_class_results):
    for c, r in zip(os_data, os_class_results):
        steps, same_modified = _unfiltered(c)
        assert np.array_equal(r["state"][:, :2], c["state"][:, :2]), c["name"]
        assert not same_modified or np.array_equal(r["state"][:, 2], c["state"][:, 2]), c["name"]
        filt, skip = True, []
        for op, a in steps:
            filt = bool(a) if op == "set_filtering" else filt
            if op in ("downsample", "process"):
                skip.append(np.full(a, filt))
        _compare(c["up"], r["up"], np.zeros(c["up"].n, bool), (c["name"], "up"))
        _compare(c["down"], r["down"], np.concatenate(skip) if skip else np.zeros(0, bool), (c["name"], "down"))
