"""The DynFilterBank and the drop-in DynamicFilters class on the device against the REFERENCE'S OWN DynamicFilters class: the results
stored in tests/golden/dynfilter_ref_streams.npz (tests/golden/make_dynfilter_vectors.py; the host side is
tests/test_dynfilter_reference_host.py).  Nothing here reads the reference tree or oracle/_ref/.

One bank of one channel per case, with the case's number of filters: the events (set_params with the same type, with a new type --
which clears the memory of ALL filters of the object --, with the two frequencies the wrong way round, set_filter_active) ahead of
the call they were recorded ahead of.  The rule is tests/test_dynfilter_gpu.py::check with the recorded output as the reference and
the restatement's float64 run as exact arithmetic; coef_tol 0 for bilinear and 1e-3 for matched-Z types, as there."""
import os
import subprocess
import time

import numpy as np
import pytest

import dynfilter_reference as R
from oracle import dynamic_filters as df

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "lsp-dsp-units_amd")
f32 = np.float32
pytestmark = pytest.mark.gpu


check, coef_tol = R.check, R.coef_tol


@pytest.fixture(scope="module")
def cases():
    """Every recorded stream and the six longer cases, each with the restatement's float64 run."""
    out = R.load("streams")
    for c in out:
        c["exact"] = R.replay(c, df, exact=True)[1]
    return out


def _run_bank(gpu, c):
    bank = gpu.DynFilterBank(1, c["filters"])
    bank.set_sample_rate(c["sample_rate"])
    out = []
    for i, (fid, offset, n) in enumerate(c["calls"]):
        for before, kind, efid, fp in c["events"]:
            if before == i:
                if kind == R.SET_PARAMS:
                    bank.set_params(efid, fp[0], fp[1], float(fp[2]), float(fp[3]), float(fp[4]), float(fp[5]))
                else:
                    bank.set_filter_active(efid, True)
        din = gpu.DeviceBuffer.from_host(np.ascontiguousarray(c["x"][None, offset:offset + n]))
        dg = gpu.DeviceBuffer.from_host(np.ascontiguousarray(c["gain"][None, offset:offset + n]))
        dout = gpu.DeviceBuffer((1, n))
        bank.process(fid, dout, din, dg, n)
        out.append(dout.download()[0])
    bank.close()
    return np.concatenate(out)


def test_bank_gives_the_recorded_streams(gpu, cases):
    """54 types x 600 samples in two calls with the memory carried."""
    streams = [c for c in cases if c["name"].startswith("stream")]
    assert len(streams) == 54
    for c in streams:
        check(_run_bank(gpu, c), c["out"], c["exact"], c["name"], coef_tol(c))


def test_bank_keeps_clears_swaps_and_copies_as_the_reference(gpu, cases):
    """The six longer cases: 1, 2, 4, 8, 12 and 15 cascades, calls of 1024, 2100 and 100 samples, and every event.  Each call is held
    on its own as well, so that the short calls after an event are not judged against the peak of the long ones."""
    long_ = [c for c in cases if c["name"].startswith("long")]
    assert len(long_) == 6
    for c in long_:
        y = _run_bank(gpu, c)
        check(y, c["out"], c["exact"], c["name"], coef_tol(c))
        at = 0
        for i, (fid, offset, n) in enumerate(c["calls"]):
            w = slice(at, at + n)
            check(y[w], c["out"][w], c["exact"][w], "%s, call %d" % (c["name"], i), coef_tol(c))
            at += n


@pytest.fixture(scope="module")
def class_results(gpu, cases, tmp_path_factory):
    """oracle/dynfilter_driver.cpp compiled against the product's headers and library, run on the device over the same cases."""
    d = tmp_path_factory.mktemp("dynfilter_class")
    exe = str(d / "dynfilter_class")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-I" + os.path.join(PKG, "include"), "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "oracle", "dynfilter_driver.cpp"), "-o", exe, "-L" + PKG, "-lmi_dspu", "-Wl,-rpath," + PKG,
                           "-Wl,-rpath,/opt/rocm/lib"])
    (d / "cases.bin").write_bytes(R.case_bytes(cases))
    t0 = time.perf_counter()
    out = subprocess.run([exe, str(d / "cases.bin"), str(d / "results.bin")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out
    print("measured: the class over %d cases in %.2f s" % (len(cases), time.perf_counter() - t0))
    return R.parse_results((d / "results.bin").read_bytes(), cases)


def test_cpp_class_gives_the_references_output_and_params(cases, class_results):
    """DynamicFilters::process through the class, and get_params(): type, slope, the swapped fFreq, gain and quality in every bit, the
    transformed fFreq2 within the distance the host test allows between two libms."""
    PARAM_ULP_SEEN, ulps = R.PARAM_ULP_SEEN, R.ulps
    direct = 0
    for c, r in zip(cases, class_results):
        check(r["out"], c["out"], c["exact"], "class, " + c["name"], coef_tol(c))
        got, want = r["params"], c["params"]
        assert np.array_equal(got[:, [0, 1, 2, 4, 5]], want[:, [0, 1, 2, 4, 5]]), c["name"]
        d = int(ulps(got[:, 3].copy().view(f32), want[:, 3].copy().view(f32)).max())
        assert d <= 2 * PARAM_ULP_SEEN, (c["name"], d)
        direct += int(d == 0)
    print("DynamicFilters class: %d of %d cases with get_params() bit-identical to the reference's" % (direct, len(cases)))
    assert 4 * direct >= 3 * len(cases)
