"""The BiquadBank, the EqualizerBank in IIR mode and the drop-in Filter / FilterBank classes on the device against the REFERENCE'S OWN
Filter and FilterBank classes: the results stored in tests/golden/filter_ref_designs.npz and filter_ref_streams.npz
(tests/golden/make_filter_vectors.py; the host side is tests/test_filter_reference_host.py).  Nothing here reads the reference tree or
oracle/_ref/.

One channel per stream case, the shorter cases padded with zeros, the calls cut at the union of the cases' cuts (and at cuts of our
own: splitting a call between two events changes nothing in the reference).  What is new for a channel is set ahead of the call it
was recorded ahead of.  A case whose sections the product's designer gives in every bit on this machine takes the DIRECT path: the
device's output is held to the recorded output.  A libm that rounds a tanf or expf differently moves a case to the FALLBACK: the
oracle's recurrence over the product's own sections with the recorded clear / keep decisions.  Each test fails unless three quarters
of its cases are direct."""
import os
import re
import subprocess
import time

import numpy as np
import pytest

import filter_reference as R
import oracle
from conftest import assert_iir_parity
from oracle import filter_design as fd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "lsp-dsp-units_amd")
f32 = np.float32
bits = R.bits
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def streams():
    return R.load_streams()


CHUNK = 16          # samples per chunk of the time-parallel kernels (csrc/biquad.hip: "chunks of 16" -- its streamable calls are whole chunks)


def _tiles():
    """The sub-block lengths of csrc/biquad.hip (`using small = geom<L>`, `using big = geom<L>`, BLOCK = 64 * 2 L) and its chunk."""
    with open(os.path.join(PKG, "csrc", "biquad.hip")) as f:
        src = f.read()
    big = int(re.search(r"using\s+big\s*=\s*geom<(\d+)>", src).group(1))
    small = int(re.search(r"using\s+small\s*=\s*geom<(\d+)>", src).group(1))
    assert re.search(r"BLOCK\s*=\s*64\s*\*\s*W", src) and re.search(r"W\s*=\s*2\s*\*\s*L", src)
    assert "(samples %% %d) != 0" % CHUNK in src, "the kernel's chunk is no longer %d samples" % CHUNK
    return 128 * small, 128 * big, CHUNK


def _report(what, directs):
    n = int(np.count_nonzero(directs))
    print("%s: %d of %d cases on the direct path (sections bit-identical to the reference's)" % (what, n, len(directs)))
    assert 4 * n >= 3 * len(directs), (what, n, len(directs))


def _params(c, call):
    """The parameters in force at a call."""
    cur = c["fp"]
    for e in c["events"]:
        if e[0] <= call and e[1] == R.UPDATE:
            cur = e[3]
    return cur


def _product_sections(mi, c):
    """Per call the sections of the product's host designer, both filters of a shared bank in the bank's order."""
    out = []
    design = lambda fp: mi.design_filter(fp[0], fp[1], float(fp[2]), float(fp[3]), float(fp[4]), float(fp[5]), sample_rate=c["sample_rate"])[2].reshape(-1, 5)
    for i in range(len(c["calls"])):
        mine, other = design(_params(c, i)), design(c["other"])
        out.append(np.concatenate({0: [mine], 3: [mine], 1: [other, mine], 2: [mine, other]}[c["shared"]]))
    return out


def _hold(mi, c, got, what, sections=None):
    """A channel's output against the case: direct against the recorded output, else against the oracle over the product's sections."""
    sections = _product_sections(mi, c) if sections is None else sections
    direct = all(a.shape == b.shape and np.array_equal(bits(a), bits(b)) for a, b in zip(sections, c["sections"]))
    if direct:
        ref32, case = c["out"], c
    else:
        case = dict(c, sections=sections)
        ref32 = R.replay(case, oracle, [b[1] for b in R.boundaries(c)])[0]
    assert_iir_parity(got, ref32, R.replay_f64(case, oracle, [b[1] for b in R.boundaries(c)]), "%s, %s (%s)" % (what, c["name"], "direct" if direct else "fallback"))
    return direct


def _cuts(cases, extra):
    ends = [np.cumsum(c["calls"]) for c in cases]
    N = max(int(e[-1]) for e in ends)
    cuts = sorted({int(e) for en in ends for e in en} | {int(e) for e in extra if 0 < e < N} | {N})
    starts = [{int(e - m): k for k, (e, m) in enumerate(zip(en, c["calls"]))} for en, c in zip(ends, cases)]
    return N, cuts, starts


# ---- BiquadBank fed the recorded sections -----------------------------------------------------------------------------------
def _run_biquad_bank(gpu, cases, extra, exact):
    N, cuts, starts = _cuts(cases, extra)
    C = len(cases)
    bounds = [R.boundaries(c) for c in cases]
    x = np.zeros((C, N), f32)
    for ch, c in enumerate(cases):
        x[ch, :len(c["x"])] = c["x"]
    bank = gpu.BiquadBank(C, max(len(s) for c in cases for s in c["sections"]))
    bank.set_exact(exact)
    got = np.zeros((C, N), f32)
    pos = 0
    for cut in cuts:
        m = cut - pos
        for ch, c in enumerate(cases):
            k = starts[ch].get(pos)
            if k is not None and (bounds[ch][k][0] or k == 0):
                bank.set_chains(ch, c["sections"][k], clear=bounds[ch][k][1])
        bank.commit()
        din, dout = gpu.DeviceBuffer.from_host(np.ascontiguousarray(x[:, pos:cut])), gpu.DeviceBuffer((C, m))
        bank.process(dout, din, m)
        got[:, pos:cut] = dout.download()
        pos = cut
    bank.close()
    return got, [cut - prev for prev, cut in zip([0] + cuts, cuts)]


def _groups(streams):
    """(what, cases, cuts of our own): every case in one bank, and each of the two long cases alone, so that calls of more than one
    sub-block occur; our own cuts stand one sample around the kernel's sub-block lengths and its chunk."""
    small, big, chunk = _tiles()
    long_ = [c for c in streams if len(c["x"]) > big]
    assert len(long_) == 2 and all(max(c["calls"]) > big for c in long_)
    out = [("every case", streams, []),
           ("every case, cuts around the chunk", streams, [chunk - 1, chunk + 1, 2 * chunk])]
    for c in long_:
        first = c["calls"][0]
        base = first if first < small + 2 else 0                    # the start of a recorded call of more than one sub-block
        out.append((c["name"], [c], []))
        out.append((c["name"] + ", cuts around the small sub-block", [c], [base + small - 1, base + small, base + small + 1]))
        out.append((c["name"] + ", cuts around the large sub-block", [c], [base + big - 1, base + big, base + big + 1]))
        out.append((c["name"] + ", one cut at the large sub-block", [c], [base + big]))
    return out


def test_biquad_bank_exact_mode_gives_the_recorded_bits(gpu, streams):
    lengths = set()
    for what, cases, extra in _groups(streams):
        got, lens = _run_biquad_bank(gpu, cases, extra, exact=True)
        lengths |= set(lens)
        for ch, c in enumerate(cases):
            n = len(c["x"])
            assert np.array_equal(bits(got[ch, :n]), bits(c["out"])), (what, c["name"], int(np.flatnonzero(bits(got[ch, :n]) != bits(c["out"]))[0]))
    small, big, chunk = _tiles()
    assert {1, chunk - 1, small - 1, small, big - 1, big, big + 1} <= lengths and max(lengths) >= big + small, sorted(lengths)


def test_biquad_bank_gives_the_recorded_output(gpu, streams):
    """The default, time-parallel kernels: conftest.assert_iir_parity against the recorded output and the float64 run of the recorded
    sections.  The sections are the recorded ones, so every case is direct."""
    for what, cases, extra in _groups(streams):
        got, _ = _run_biquad_bank(gpu, cases, extra, exact=False)
        for ch, c in enumerate(cases):
            assert _hold(gpu, c, got[ch, :len(c["x"])], "BiquadBank, " + what, sections=c["sections"])


# ---- EqualizerBank in IIR mode ----------------------------------------------------------------------------------------------
def test_equalizer_bank_designs_and_keeps_or_clears_as_the_reference(gpu, streams):
    """Every case on a shared bank (an Equalizer is a FilterBank shared by its filters: Equalizer.cpp:256-259) as one channel of an
    EqualizerBank of two filters, driven by the recorded PARAMETERS: the product's designer and its decision to keep or to clear the
    delays are on the path.  The generator made sure that the wrong decision moves the output by more than 100 x TOL."""
    cases = [c for c in streams if c["shared"] != 0]
    assert len(cases) >= 15 and all(c["sample_rate"] == 48000 for c in cases)
    N, cuts, starts = _cuts(cases, [])
    C = len(cases)
    x = np.zeros((C, N), f32)
    bank = gpu.EqualizerBank(C, 2, 8)
    bank.set_sample_rate(48000)
    bank.set_mode(gpu.EqualizerBank.IIR)
    slot = lambda c: 1 if c["shared"] == 1 else 0
    for ch, c in enumerate(cases):
        x[ch, :len(c["x"])] = c["x"]
        bank.set_params(slot(c), *[v if k < 2 else float(v) for k, v in enumerate(c["fp"])], channel=ch)
        other = c["other"] if c["shared"] in (1, 2) else (fd.FLT_NONE, 1, 1000.0, 1000.0, 1.0, 0.0)
        bank.set_params(1 - slot(c), *[v if k < 2 else float(v) for k, v in enumerate(other)], channel=ch)
    got = np.zeros((C, N), f32)
    pos = 0
    for cut in cuts:
        m = cut - pos
        for ch, c in enumerate(cases):
            k = starts[ch].get(pos)
            for e in c["events"]:
                if k is not None and e[0] == k:
                    assert e[1] == R.UPDATE and e[2] == 48000
                    bank.set_params(slot(c), *[v if j < 2 else float(v) for j, v in enumerate(e[3])], channel=ch)
        din, dout = gpu.DeviceBuffer.from_host(np.ascontiguousarray(x[:, pos:cut])), gpu.DeviceBuffer((C, m))
        bank.process(dout, din, m)
        got[:, pos:cut] = dout.download()
        pos = cut
    bank.close()
    _report("EqualizerBank", [_hold(gpu, c, got[ch, :len(c["x"])], "EqualizerBank") for ch, c in enumerate(cases)])


# ---- the drop-in C++ classes ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def class_results(gpu, tmp_path_factory):
    """oracle/filter_driver.cpp compiled against the product's headers and library, run on the device over every stream case and
    every recorded design, the APO designs with their freq_chart."""
    streams, designs = R.load_streams(), R.load_designs()
    cases = streams + [dict(R.design_case(d["sample_rate"], d["fp"], chart=d["chart"] is not None), sections=[d["sections"]], inactive=[d["inactive"]],
                            latency=[d["latency"]], limited=[d["limited"]], out=np.zeros(0, f32), irs=[], chart=d["chart"]) for d in designs]
    d = tmp_path_factory.mktemp("filter_class")
    exe = str(d / "filter_class")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-I" + os.path.join(PKG, "include"), "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "oracle", "filter_driver.cpp"), "-o", exe, "-L" + PKG, "-lmi_dspu", "-Wl,-rpath," + PKG,
                           "-Wl,-rpath,/opt/rocm/lib"])
    (d / "cases.bin").write_bytes(R.case_bytes(cases))
    t0 = time.perf_counter()
    out = subprocess.run([exe, str(d / "cases.bin"), str(d / "results.bin")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out
    print("measured: the classes over %d cases in %.2f s" % (len(cases), time.perf_counter() - t0))
    return cases, R.parse_results((d / "results.bin").read_bytes(), cases)


def test_cpp_classes_give_the_references_sections_and_reports(class_results):
    """chain(i), size(), inactive(), latency() and get_params() after the limit, for every call of every case."""
    cases, results = class_results
    directs, charts = [], []
    for c, r in zip(cases, results):
        assert r["inactive"] == c["inactive"] and r["latency"] == c["latency"], c["name"]
        assert all(np.array_equal(a, b) for a, b in zip(r["limited"], c["limited"])), (c["name"], c["fp"])
        assert [len(s) for s in r["sections"]] == [len(s) for s in c["sections"]], (c["name"], c["fp"])
        directs.append(all(np.array_equal(bits(a), bits(b)) for a, b in zip(r["sections"], c["sections"])))
        if c.get("chart") is not None:
            # both overloads of freq_chart: the recorded bits where the sections are, else one part in 1e6 of the largest magnitude
            for got in (r["charts"][0]["packed"], r["charts"][0]["split"]):
                same = np.array_equal(got.astype(np.complex64).view(f32).view(np.uint32), c["chart"].view(f32).view(np.uint32))
                assert same or float(np.abs(got - c["chart"]).max()) <= 1e-6 * float(np.abs(c["chart"]).max()), (c["fp"], got, c["chart"])
                charts.append(same)
    assert len(charts) == 2 * 183
    _report("Filter class, freq_chart of the APO designs", charts)
    _report("Filter / FilterBank classes, sections", directs)


def test_cpp_classes_give_the_references_output(gpu, class_results):
    """The stream cases through Filter::process on the device: own bank and shared bank, every keep and every clear, FLT_NONE, and
    impulse_response() between two calls without a trace in the stream."""
    cases, results = class_results
    directs = []
    irs = 0
    for c, r in zip(cases, results):
        if not len(c["x"]):
            continue
        directs.append(_hold(gpu, c, r["out"], "Filter class", sections=r["sections"]))
        for k, (got, want) in enumerate(zip(r["irs"], c["irs"])):
            call = [e[0] for e in c["events"] if e[1] == R.IMPULSE][k]
            sec = r["sections"][call]
            ref32 = oracle.biquad_impulse_response(len(got), sec, np.zeros((len(sec), 2), f32))
            if directs[-1]:
                assert np.array_equal(bits(ref32), bits(want)), c["name"]
            delta = np.zeros(len(got), f32)
            delta[0] = 1
            assert_iir_parity(got, ref32, oracle.biquad_cascade_f64(delta, sec), "impulse response %d, %s" % (k, c["name"]))
            irs += 1
    assert irs >= 3
    _report("Filter / FilterBank classes, output", directs)
