"""The Limiter, AutoGain and SimpleAutoGain banks and the drop-in C++ classes on the device against the REFERENCE'S OWN classes:
the results stored in tests/golden/limiter_ref_vectors.npz and autogain_ref_vectors.npz (tests/golden/make_gain_vectors.py; the
host side is tests/test_gain_reference_host.py).  Nothing here reads the reference tree or oracle/_ref/.

A channel whose get_params() equals the recorded parameters in every bit ahead of every call (for the Limiter also get_patch()
the table evaluated from the recorded coefficients) takes the DIRECT path: its gain and its state after every call are the
reference's bits, NaN at the same places.  A libm that rounds an expf differently would move a channel to the FALLBACK: the
restatement fed the library's own parameters, as the banks' own tests do.  Each test fails unless three quarters of its cases
are direct.  The reference does not count patches: the bank's count is held to the restatement's on either path.

A Limiter chunk is counted from a call's first sample, so a case holds for its own cuts only: cases share a bank where they
share the bank's maxima AND the call lengths.  AutoGain and SimpleAutoGain run as one bank each, cut at every case's call ends."""
import os
import subprocess

import numpy as np
import pytest

import gain_reference as R
from gain_reference import gv, lr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "lsp-dsp-units_amd")
f32 = np.float32


@pytest.fixture(scope="module")
def data():
    return R.load()


def _report(what, directs):
    n = int(np.count_nonzero(directs))
    print("%s: %d of %d cases on the direct path (parameters bit-identical to the reference's)" % (what, n, len(directs)))
    assert 4 * n >= 3 * len(directs), (what, n, len(directs))


def _first(a, b):
    return np.flatnonzero(R.bits(a) != R.bits(b))[:4]


def _audio(rows, n, seed=5):
    return (np.random.default_rng(seed).uniform(0.25, 1.0, (rows, n)) * np.where(np.arange(n) % 3 == 0, -1.0, 1.0)).astype(f32)


def _product(audio, gain):
    with np.errstate(all="ignore"):
        return (np.asarray(audio, f32) * np.asarray(gain, f32)).astype(f32)


# ---- Limiter ------------------------------------------------------------------------------------------------------------------
def _limiter_want(c, params, patches):
    """(direct, gain, nHead per call, envelope per call, (patches, chunks) per call) that a channel with these parameters and
    tables ahead of its calls owes."""
    direct = all(R.all_same(params[k], R.limiter_params(c, k)) and
                 np.array_equal(R.bits(patches[k]), R.bits(R.limiter_table(R.limiter_params(c, k)))) for k in range(len(c["calls"])))
    provider = R.recorded_limiter(c) if direct else (lambda k, s: (params[k], patches[k]))
    gain, heads, envs, counts, _ = R.run_limiter(c, provider)
    if direct:                                      # the reference's own results; the restatement only counts the patches
        gain = c["out"][0]
        heads = [R.row("limiter", c, k)["head"] for k in range(len(c["calls"]))]
        envs = [R.row("limiter", c, k)["envelope"] for k in range(len(c["calls"]))]
    return direct, gain, heads, envs, [(sum(p), len(p)) for p in counts]


def _limiter_banks(gpu, cases, apply=False):
    """Every group of cases that can share a bank through process() (or process_apply on an audio of its own), the setter
    events between the calls: -> [direct per case]."""
    groups = {}
    for c in cases:
        groups.setdefault(R.limiter_bank_key(c), []).append(c)
    directs = []
    for (max_sr, max_la, calls), cs in groups.items():
        C, n = len(cs), sum(calls)
        bank = gpu.LimiterBank(C, max_sr, max_la)
        for ch, c in enumerate(cs):
            R.limiter_bank_setup(bank, ch, c)
        x = np.stack([c["inputs"][0] for c in cs])
        audio = _audio(C, n, seed=7)
        got = np.zeros((C, n), f32)
        params, tables, lat, states = ([[] for _ in cs] for _ in range(4))
        pos = 0
        for k, m in enumerate(calls):
            for ch, c in enumerate(cs):
                for name, args in R.events_before(c, k):
                    getattr(bank, name)(ch, *args)
            bank.update_settings()
            for ch in range(C):
                params[ch].append(bank.get_params(ch))
                tables[ch].append(bank.get_patch(ch))
                lat[ch].append(bank.get_latency(ch))
            din, dout = gpu.DeviceBuffer.from_host(np.ascontiguousarray(x[:, pos:pos + m])), gpu.DeviceBuffer((C, m))
            if apply:
                bank.process_apply(dout, gpu.DeviceBuffer.from_host(np.ascontiguousarray(audio[:, pos:pos + m])), din, m)
            else:
                bank.process(dout, din, m)
            got[:, pos:pos + m] = dout.download()
            for ch in range(C):
                states[ch].append(bank.get_state(ch))
            pos += m
        bank.close()
        for ch, c in enumerate(cs):
            what = ("limiter", c["name"], "process_apply" if apply else "process")
            direct, gain, heads, envs, counts = _limiter_want(c, params[ch], tables[ch])
            directs.append(direct)
            want, pos = gain, 0
            if apply:                               # out = f32(audio[i - latency] x gain[i]), the latency the call's own
                want = np.zeros(n, f32)
                for k, m in enumerate(calls):
                    assert lat[ch][k] == params[ch][k]["lookahead"]
                    want[pos:pos + m] = _product(lr.delayed(audio[ch], pos, m, lat[ch][k]), gain[pos:pos + m])
                    pos += m
            assert R.same(got[ch], want), what + (direct, "first differences at", _first(got[ch], want))
            for k in range(len(calls)):
                head, env, patches, chunks, overrun = states[ch][k]
                assert head == heads[k], what + (direct, "nHead after call %d" % k, head, heads[k])
                assert R.same(env, envs[k]), what + (direct, "ALR envelope after call %d" % k, env, envs[k])
                assert (patches, chunks) == counts[k] and overrun == 0, what + ("patches and chunks of call %d" % k, patches, chunks, counts[k])
    return directs


@pytest.mark.gpu
def test_limiter_banks_give_the_references_gain_and_state(gpu, data):
    _report("limiter banks", _limiter_banks(gpu, data["limiter"][:gv.LIM_GENERAL]))


@pytest.mark.gpu
def test_limiter_process_apply_is_the_references_gain_on_the_delayed_audio(gpu, data):
    _report("limiter process_apply", _limiter_banks(gpu, data["limiter"][:gv.LIM_GENERAL], apply=True))


@pytest.mark.gpu
def test_long_limiter_cases_with_the_chunk_boundary_in_four_places(gpu, data):
    """8192 + 300 samples as one call and cut at 5000, 4096 and 8191, a bank each: every run against what the reference recorded
    for that very cut (the same input in another cut is another result: test_gain_reference_host.py prints how far apart)."""
    _report("long limiter cases", _limiter_banks(gpu, data["limiter"][gv.LIM_GENERAL:]))


# ---- AutoGain and SimpleAutoGain: one bank, cut at every case's call ends ---------------------------------------------------
def _cut_run(gpu, bank, cases, rows, launch, fill):
    """The recorded inputs through `bank`, cut at every case's call ends (a shorter case goes on with `fill`), the setter events
    of a case ahead of the call they belong to: the output [C, n], and per case the get_params() ahead of every call and the
    get_state() after it.  rows: how many input rows a case has; launch(bank, out, inputs, count)."""
    C, n = len(cases), max(len(c["inputs"][0]) for c in cases)
    x = [np.full((C, n), fill[r], f32) for r in range(rows)]
    for ch, c in enumerate(cases):
        for r in range(rows):
            x[r][ch, :len(c["inputs"][r])] = c["inputs"][r]
    starts = [np.concatenate([[0], np.cumsum(c["calls"])]) for c in cases]
    cuts = sorted({int(e) for s in starts for e in s[1:]} | {n})
    got = np.zeros((C, n), f32)
    params, states, a = [[] for _ in cases], [[] for _ in cases], 0
    for b in cuts:
        begins = [(ch, int(np.flatnonzero(starts[ch][:-1] == a)[0])) for ch in range(C) if a in starts[ch][:-1]]
        for ch, k in begins:
            for name, args in R.events_before(cases[ch], k):
                R.bank_event(bank, ch, name, args)
        bank.update_settings()
        for ch, k in begins:
            params[ch].append(bank.get_params(ch))
        dout = gpu.DeviceBuffer((C, b - a))
        launch(bank, dout, [gpu.DeviceBuffer.from_host(np.ascontiguousarray(v[:, a:b])) for v in x], b - a)
        got[:, a:b] = dout.download()
        for ch in range(C):
            if b in starts[ch][1:]:
                states[ch].append(bank.get_state(ch))
        a = b
    return got, params, states


def _autogain_bank(gpu, cases):
    bank = gpu.AutoGainBank(len(cases))
    for ch, c in enumerate(cases):
        R.autogain_bank_setup(bank, ch, c)
    return bank


def _autogain_want(c, params, scalar=False):
    direct = all(R.all_same(params[k], R.autogain_params(c, k)) for k in range(len(c["calls"])))
    if direct:
        states = [(R.row("autogain", c, k)["curr_gain"], R.row("autogain", c, k)["out_gain"], R.row("autogain", c, k)["flags"])
                  for k in range(len(c["calls"]))]
        return True, c["out"][1 if scalar else 0], states
    vca, states, _ = R.run_autogain(c, lambda k: params[k], scalar=scalar)
    return False, vca, states


def _check_autogain(cases, got, params, states, what, scalar=False, audio=None):
    directs = []
    for ch, c in enumerate(cases):
        direct, vca, want_states = _autogain_want(c, params[ch], scalar)
        directs.append(direct)
        n = len(c["inputs"][0])
        want = vca if audio is None else _product(audio[ch, :n], vca)
        assert R.same(got[ch, :n], want), ("autogain", c["name"], what, direct, "first differences at", _first(got[ch, :n], want))
        for k, (g, o, f) in enumerate(states[ch]):
            w = want_states[k]
            assert R.same(g, w[0]) and R.same(o, w[1]) and f == w[2], ("autogain", c["name"], what, direct, "state after call %d" % k, (g, o, f), w)
    return directs


@pytest.mark.gpu
def test_autogain_bank_gives_the_references_gain_and_state(gpu, data):
    cases = data["autogain"]
    bank = _autogain_bank(gpu, cases)
    got, params, states = _cut_run(gpu, bank, cases, 3, lambda b, out, d, m: b.process(out, d[0], d[1], d[2], m), (0.0, 0.0, 1.0))
    bank.close()
    _report("autogain bank", _check_autogain(cases, got, params, states, "process"))


@pytest.mark.gpu
def test_autogain_process_level_and_process_apply(gpu, data):
    cases = data["autogain"]
    C = len(cases)
    levels = gpu.DeviceBuffer.from_host(np.array([R.settings(c)["level"] for c in cases], f32))
    bank = _autogain_bank(gpu, cases)
    got, params, states = _cut_run(gpu, bank, cases, 3, lambda b, out, d, m: b.process_level(out, d[0], d[1], levels, m), (0.0, 0.0, 1.0))
    bank.close()
    _report("autogain process_level", _check_autogain(cases, got, params, states, "process_level", scalar=True))

    n = max(len(c["inputs"][0]) for c in cases)
    audio, at = _audio(C, n), [0]

    def launch(b, out, d, m):
        da = gpu.DeviceBuffer.from_host(np.ascontiguousarray(audio[:, at[0]:at[0] + m]))
        b.process_apply(out, da, d[0], d[1], d[2], m)
        at[0] += m
    bank = _autogain_bank(gpu, cases)
    got, params, states = _cut_run(gpu, bank, cases, 3, launch, (0.0, 0.0, 1.0))
    bank.close()
    _check_autogain(cases, got, params, states, "process_apply", audio=audio)


@pytest.mark.gpu
def test_simple_autogain_bank_gives_the_references_gain_and_state(gpu, data):
    cases = data["simple"]
    bank = gpu.SimpleAutoGainBank(len(cases))
    for ch, c in enumerate(cases):
        R.simple_bank_setup(bank, ch, c)
    got, params, states = _cut_run(gpu, bank, cases, 1, lambda b, out, d, m: b.process(out, d[0], m), (0.0,))
    bank.close()
    directs = []
    for ch, c in enumerate(cases):
        direct = all(R.all_same(params[ch][k], R.simple_params(c, k)) for k in range(len(c["calls"])))
        directs.append(direct)
        if direct:
            want, want_states = c["out"][0], [R.row("simple", c, k)["curr_gain"] for k in range(len(c["calls"]))]
        else:
            want, want_states, _ = R.run_simple(c, lambda k: params[ch][k])
        n = len(c["inputs"][0])
        assert R.same(got[ch, :n], want), ("simple", c["name"], direct, "first differences at", _first(got[ch, :n], want))
        for k, g in enumerate(states[ch]):
            assert R.same(g, want_states[k]), ("simple", c["name"], direct, "fCurrGain after call %d" % k, g, want_states[k])
    _report("simple autogain bank", directs)


# ---- the drop-in classes: one program, two libraries -------------------------------------------------------------------
@pytest.fixture(scope="module")
def class_results(gpu, data, tmp_path_factory):
    """oracle/gain_driver.cpp, the text that was compiled with the reference's classes to record the vectors, compiled against
    lsp-dsp-units_amd/include and libmi_dspu.so and run once on the same cases."""
    d = tmp_path_factory.mktemp("gain_driver")
    exe = str(d / "gain_ours")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-I" + os.path.join(PKG, "include"), "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "oracle", "gain_driver.cpp"), "-o", exe, "-L" + PKG, "-lmi_dspu", "-Wl,-rpath," + PKG,
                           "-Wl,-rpath,/opt/rocm/lib"])
    cases = [c for cls in R.CLASSES for c in data[cls]]
    (d / "cases.bin").write_bytes(gv.case_bytes([R.case_for_driver(c) for c in cases]))
    out = subprocess.run([exe, str(d / "cases.bin"), str(d / "results.bin")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out
    res = gv.parse_results((d / "results.bin").read_bytes(), cases)
    return {cls: [(c, r) for c, r in zip(cases, res) if c["cls"] == cls] for cls in R.CLASSES}


def _fields(cls, names):
    return [gv.CALLF[cls].index(n) for n in names]


@pytest.mark.gpu
def test_limiter_class_gives_what_the_references_class_gave(class_results):
    directs = []
    for c, r in class_results["limiter"]:
        what = ("limiter", c["name"], "class")
        ours = dict(c, calli=r["calli"], callf=r["callf"])
        calls = range(len(c["calls"]))
        for field in ("max_lookahead", "latency"):      # nMaxLookahead of init() and get_latency() ahead of every call
            j = gv.CALLI["limiter"].index(field)
            assert np.array_equal(r["calli"][:, j], c["calli"][:, j]), what + (field, r["calli"][:, j], c["calli"][:, j])
        params = [R.limiter_params(ours, k) for k in calls]
        direct = all(R.all_same(params[k], R.limiter_params(c, k)) for k in calls)
        directs.append(direct)
        if direct:
            gain, heads = c["out"][0], [R.row("limiter", c, k)["head"] for k in calls]
            envs = [R.row("limiter", c, k)["envelope"] for k in calls]
        else:                                       # the class shows no table: the host formula on its own coefficients
            gain, heads, envs, _, _ = R.run_limiter(c, R.recorded_limiter(ours))
        assert R.same(r["out"][0], gain), what + (direct, "first differences at", _first(r["out"][0], gain))
        for k in calls:
            mine = R.row("limiter", ours, k)
            assert mine["head"] == heads[k] and R.same(mine["envelope"], envs[k]), what + (direct, "state after call %d" % k, mine["head"], heads[k])
    _report("limiter class", directs)


@pytest.mark.gpu
def test_autogain_class_gives_what_the_references_class_gave(class_results):
    directs = []
    for c, r in class_results["autogain"]:
        what = ("autogain", c["name"], "class")
        ours = dict(c, calli=r["calli"], callf=r["callf"])
        calls = range(len(c["calls"]))
        params = [R.autogain_params(ours, k) for k in calls]
        assert np.array_equal(r["calli"][:, 0], c["calli"][:, 0]), what + ("nFlags ahead of the calls",)
        for scalar in (False, True):
            direct, vca, states = _autogain_want(c, params, scalar)
            got = r["out"][1 if scalar else 0]
            assert R.same(got, vca), what + (scalar, direct, "first differences at", _first(got, vca))
            if not scalar:
                directs.append(direct)
                for k in calls:
                    mine = R.row("autogain", ours, k)
                    assert R.same(mine["curr_gain"], states[k][0]) and R.same(mine["out_gain"], states[k][1]) and mine["flags"] == states[k][2], \
                        what + (direct, "state after call %d" % k, mine, states[k])
    _report("autogain class", directs)


@pytest.mark.gpu
def test_simple_autogain_class_gives_what_the_references_class_gave(class_results):
    directs = []
    for c, r in class_results["simple"]:
        what = ("simple", c["name"], "class")
        ours = dict(c, calli=r["calli"], callf=r["callf"])
        calls = range(len(c["calls"]))
        params = [R.simple_params(ours, k) for k in calls]
        direct = all(R.all_same(params[k], R.simple_params(c, k)) for k in calls)
        directs.append(direct)
        if direct:
            want, states, after = c["out"][0], [R.row("simple", c, k)["curr_gain"] for k in calls], c["after"]
        else:
            want, states, after = R.run_simple(c, lambda k: params[k])
        assert R.same(r["out"][0], want), what + (direct, "first differences at", _first(r["out"][0], want))
        for k in calls:
            assert R.same(R.row("simple", ours, k)["curr_gain"], states[k]), what + (direct, "fCurrGain after call %d" % k)
        assert R.same(r["after"], after), what + (direct, "fCurrGain after every setter event", r["after"], after)
    _report("simple autogain class", directs)
