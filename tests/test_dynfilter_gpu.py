"""GPU parity of mi_dynfilter_bank_* (lsp::dspu::DynamicFilters) against the CPU oracle, through the C-ABI."""
import os

import numpy as np
import pytest

import oracle
from oracle import dynamic_filters as df
from oracle import filter_design as fd
from conftest import IIR_EXACT_FACTOR, IIR_REF_FACTOR, NOISE_FLOOR, TOL, record_parity
from dynfilter_reference import check      # conftest.assert_iir_parity's rule with a coefficient allowance

pytestmark = pytest.mark.gpu
SR = 48000
TYPES = [t for t in range(1, len(fd.FILTER_TYPES)) if df.cascade_count(t, 1) > 0]


def gains(rng, C, n, kind):
    """Per-channel gain curves: what a dynamics processor feeds a dynamic equaliser."""
    t = np.arange(n) / float(SR)
    if kind == "constant":
        g = np.full((C, n), 1.8)
    elif kind == "sweep":                                    # slow envelope, 0.3 .. 3
        g = np.exp(np.log(3.0) * np.sin(2 * np.pi * (3.0 + rng.uniform(0, 4, (C, 1))) * t + rng.uniform(0, 6, (C, 1))))
    else:                                                    # sample-to-sample changes
        g = np.exp(rng.uniform(-1.0, 1.0, (C, n)))
    return g.astype(np.float32)


@pytest.mark.parametrize("t", TYPES)
def test_every_type_matches_the_oracle(gpu, t):
    """Three blocks with carried memory, a slowly moving gain per channel, 3 channels; bilinear and matched types."""
    rng = np.random.default_rng(100 + t)
    C, n, blocks = 3, 1500, 3
    slope = 2 if df.cascade_count(t, 2) <= 16 else 1
    bank = gpu.DynFilterBank(C, 2)
    bank.set_sample_rate(SR)
    bank.set_params(1, t, slope, 1200.0, 5000.0, 1.0, 0.6)
    bank.set_filter_active(1)
    refs = [df.DynamicFilters(2) for _ in range(C)]
    for r in refs:
        r.set_sample_rate(SR)
        r.set_params(1, t, slope, 1200.0, 5000.0, 1.0, 0.6)
        r.set_filter_active(1, True)
    x = (rng.standard_normal((C, n * blocks)) * 0.25).astype(np.float32)
    g = gains(rng, C, n * blocks, "sweep")
    y = np.empty_like(x)
    ref, exact = np.empty_like(x), np.empty(x.shape, np.float64)
    for b in range(blocks):
        seg = slice(b * n, (b + 1) * n)
        din, dg, dout = gpu.DeviceBuffer.from_host(x[:, seg]), gpu.DeviceBuffer.from_host(g[:, seg]), gpu.DeviceBuffer((C, n))
        bank.process(1, dout, din, dg, n)
        y[:, seg] = dout.download()
        for c in range(C):
            ref[c, seg], exact[c, seg] = refs[c].process(1, x[c, seg], g[c, seg], exact=True)
    for c in range(C):
        check(y[c], ref[c], exact[c], "%s ch %d" % (fd.FILTER_TYPES[t], c), coef_tol=0.0 if (t & 1) else 1e-3)
    bank.close()


@pytest.mark.parametrize("t", TYPES)
def test_every_type_on_whole_super_blocks(gpu, t):
    """A call of 4096 samples: two whole super-blocks of the kernel compiled for the type, the path without the
    per-sample guards (dynfilter.hip, run_sections<FULL>), followed by a ragged call of 2048 + 100 with carried memory.
    Bilinear types and their matched-Z twins (coefficient tolerance as in test_every_type_matches_the_oracle)."""
    rng = np.random.default_rng(4100 + t)
    C, calls = 2, (4096, 2148)
    n = sum(calls)
    slope = 2 if df.cascade_count(t, 2) <= 16 else 1
    bank = gpu.DynFilterBank(C, 1)
    bank.set_sample_rate(SR)
    bank.set_params(0, t, slope, 900.0, 4000.0, 1.0, 0.8)
    bank.set_filter_active(0)
    refs = [df.DynamicFilters(1) for _ in range(C)]
    for r in refs:
        r.set_sample_rate(SR)
        r.set_params(0, t, slope, 900.0, 4000.0, 1.0, 0.8)
        r.set_filter_active(0, True)
    x = (rng.standard_normal((C, n)) * 0.25).astype(np.float32)
    g = gains(rng, C, n, "jumpy" if t % 4 == 1 else "sweep")
    y = np.empty_like(x)
    ref, exact = np.empty_like(x), np.empty(x.shape, np.float64)
    pos = 0
    for m in calls:
        seg = slice(pos, pos + m)
        din, dg, dout = gpu.DeviceBuffer.from_host(x[:, seg]), gpu.DeviceBuffer.from_host(g[:, seg]), gpu.DeviceBuffer((C, m))
        bank.process(0, dout, din, dg, m)
        y[:, seg] = dout.download()
        for c in range(C):
            ref[c, seg], exact[c, seg] = refs[c].process(0, x[c, seg], g[c, seg], exact=True)
        pos += m
    for c in range(C):
        check(y[c], ref[c], exact[c], "%s ch %d, whole super-blocks" % (fd.FILTER_TYPES[t], c), coef_tol=0.0 if (t & 1) else 1e-3)
    bank.close()


@pytest.mark.parametrize("t", [fd.FLT_BT_RLC_RESONANCE, fd.FLT_MT_RLC_RESONANCE, fd.FLT_BT_RLC_BELL, fd.FLT_BT_RLC_LOSHELF,
                               fd.FLT_BT_RLC_HISHELF, fd.FLT_BT_BWC_BELL, fd.FLT_BT_LRX_LOSHELF, fd.FLT_BT_AMPLIFIER])
def test_gain_samples_of_zero(gpu, t):
    """Gain samples of exactly 0 (and next to the ends of the float range) among ordinary ones: logf(g) = -inf and 1 / g =
    inf reach the builders' divisions.  Where the reference's arithmetic stays finite (RLC_RESONANCE: t = {1, 0, 1},
    DynamicFilters.cpp:964-980) the device must follow it and the memory must stay usable for the block behind; where the
    reference itself leaves the finite numbers (a division by the gain) only the blocks before are compared."""
    rng = np.random.default_rng(700 + t)
    C, n = 2, 1024
    bank = gpu.DynFilterBank(C, 1)
    bank.set_sample_rate(SR)
    bank.set_params(0, t, 1, 1200.0, 5000.0, 1.0, 0.6)
    bank.set_filter_active(0)
    refs = [df.DynamicFilters(1) for _ in range(C)]
    for r in refs:
        r.set_sample_rate(SR)
        r.set_params(0, t, 1, 1200.0, 5000.0, 1.0, 0.6)
        r.set_filter_active(0, True)
    x = (rng.standard_normal((3, C, n)) * 0.25).astype(np.float32)
    g = gains(rng, C, 3 * n, "sweep").reshape(C, 3, n).transpose(1, 0, 2).copy()
    g[1, 0, 100:140] = 0.0                                    # a stretch of zeros, single zeros, tiny and large gains
    g[1, 0, 500] = 0.0
    g[1, 1, 300:310] = np.float32(1e-30)
    g[1, 1, 700:705] = np.float32(50.0)
    finite = True
    for b in range(3):
        din, dg, dout = gpu.DeviceBuffer.from_host(x[b]), gpu.DeviceBuffer.from_host(g[b]), gpu.DeviceBuffer((C, n))
        bank.process(0, dout, din, dg, n)
        y = dout.download()
        for c in range(C):
            with np.errstate(all="ignore"):
                ref, exact = refs[c].process(0, x[b, c], g[b, c], exact=True)
            if not (np.all(np.isfinite(ref)) and np.all(np.isfinite(exact))):
                finite = False                                # the reference left the finite numbers: nothing to hold on to
            if finite:
                check(y[c], ref, exact, "%s block %d ch %d" % (fd.FILTER_TYPES[t], b, c), coef_tol=0.0 if (t & 1) else 1e-3)
    if t in (fd.FLT_BT_RLC_RESONANCE, fd.FLT_BT_AMPLIFIER):
        assert finite, "the reference's arithmetic is finite at gain 0 for this type"
    bank.close()


@pytest.mark.parametrize("kind", ["constant", "sweep", "jumpy"])
def test_gain_shapes_sizes_and_in_place(gpu, kind):
    """Constant, slowly varying and sample-to-sample gains; ragged call sizes around the 1024-sample block and the
    16-sample chunk; in-place calls; padded rows."""
    rng = np.random.default_rng(7)
    C = 5
    t = fd.FLT_BT_LRX_BELL
    bank = gpu.DynFilterBank(C, 1)
    bank.set_sample_rate(SR)
    bank.set_params(0, t, 2, 900.0, 900.0, 1.0, 1.0)
    bank.set_filter_active(0)
    refs = [df.DynamicFilters(1) for _ in range(C)]
    for r in refs:
        r.set_sample_rate(SR); r.set_params(0, t, 2, 900.0, 900.0, 1.0, 1.0); r.set_filter_active(0, True)
    sizes = [1, 15, 16, 17, 1023, 1024, 1025, 2048, 3000, 4096, 77]
    total = sum(sizes)
    x = (rng.standard_normal((C, total)) * 0.25).astype(np.float32)
    g = gains(rng, C, total, kind)
    y = np.empty_like(x)
    pos = 0
    for i, n in enumerate(sizes):
        pad = 8 if (i & 1) else 0
        hx = np.zeros((C, n + pad), np.float32); hx[:, :n] = x[:, pos:pos + n]
        hg = np.ones((C, n + pad), np.float32); hg[:, :n] = g[:, pos:pos + n]
        din, dg = gpu.DeviceBuffer.from_host(hx), gpu.DeviceBuffer.from_host(hg)
        dout = din if (i % 3 == 0) else gpu.DeviceBuffer((C, n + pad))
        bank.process(0, dout, din, dg, n, n + pad, n + pad, n + pad)
        y[:, pos:pos + n] = dout.download()[:, :n]
        pos += n
    for c in range(C):
        ref, exact = refs[c].process(0, x[c], g[c], exact=True)
        check(y[c], ref, exact, "%s ch %d" % (kind, c))
    bank.close()


def test_constant_gain_equals_the_static_bank(gpu):
    """A constant gain vector filters every sample with the same sections: the dynamic bank then computes what the static
    biquad bank computes with those sections (both within round-off of the oracle; identical operation order per sample)."""
    rng = np.random.default_rng(9)
    C, n = 4, 4096
    t, slope = fd.FLT_BT_RLC_BELL, 3
    bank = gpu.DynFilterBank(C, 1)
    bank.set_sample_rate(SR); bank.set_params(0, t, slope, 2000.0, 2000.0, 1.0, 0.8); bank.set_filter_active(0)
    sec = gpu.dynfilter_sections(t, slope, 2000.0, 2000.0, 0.8, 2.2, SR)
    static = gpu.BiquadBank(C, len(sec))
    for c in range(C):
        static.set_chains(c, sec)
    x = (rng.standard_normal((C, n)) * 0.25).astype(np.float32)
    din, dg = gpu.DeviceBuffer.from_host(x), gpu.DeviceBuffer.from_host(np.full((C, n), 2.2, np.float32))
    d1, d2 = gpu.DeviceBuffer((C, n)), gpu.DeviceBuffer((C, n))
    bank.process(0, d1, din, dg, n)
    static.process(d2, din, n)
    y1, y2 = d1.download(), d2.download()
    for c in range(C):
        ref, _ = oracle.biquad_cascade(x[c], sec)
        exact = oracle.biquad_cascade_f64(x[c], sec)
        check(y1[c], ref, exact, "dynamic ch %d" % c)
        check(y2[c], ref, exact, "static ch %d" % c)
        assert np.abs(y1[c] - y2[c]).max() <= 2 * TOL * np.abs(exact).max()
    bank.close(); static.close()


def test_bypass_clear_and_bad_arguments(gpu):
    """inactive / FLT_NONE / slope 0: a copy (DynamicFilters.cpp:207-212); a change of type clears every filter's memory at
    the next process() (:132-133, 214-219); set_filter_active always activates (.h:147-153); refusals."""
    rng = np.random.default_rng(3)
    C, n = 2, 600
    x = (rng.standard_normal((C, n)) * 0.25).astype(np.float32)
    g = np.full((C, n), 2.0, np.float32)
    bank = gpu.DynFilterBank(C, 2)
    bank.set_sample_rate(SR)
    din, dg, dout = gpu.DeviceBuffer.from_host(x), gpu.DeviceBuffer.from_host(g), gpu.DeviceBuffer((C, n))
    bank.process(0, dout, din, dg, n)                        # FLT_NONE, inactive
    np.testing.assert_array_equal(dout.download(), x)
    bank.set_params(0, fd.FLT_BT_RLC_LOSHELF, 0, 500.0, 500.0, 1.0, 0.0); bank.set_filter_active(0, False)
    assert bank.get_params(0)[1] is True                     # "false" activates as well
    bank.process(0, dout, din, dg, n)                        # slope 0
    np.testing.assert_array_equal(dout.download(), x)
    # memory: two filters run, then filter 1 changes its type -> both memories are cleared at the next process()
    refs = [df.DynamicFilters(2) for _ in range(C)]
    def both(name, *a):
        getattr(bank, name)(*a)
        for r in refs:
            getattr(r, name)(*a)
    both("set_sample_rate", SR)
    both("set_params", 0, fd.FLT_BT_RLC_LOSHELF, 2, 500.0, 500.0, 1.0, 0.0); both("set_filter_active", 0, True)
    both("set_params", 1, fd.FLT_BT_BWC_HIPASS, 3, 300.0, 300.0, 1.0, 0.0); both("set_filter_active", 1, True)
    for step in range(3):
        if step == 2:
            both("set_params", 1, fd.FLT_MT_RLC_BELL, 2, 3000.0, 3000.0, 1.0, 0.5)
        for fid in (0, 1):
            bank.process(fid, dout, din, dg, n)
            y = dout.download()
            for c in range(C):
                ref, exact = refs[c].process(fid, x[c], g[c], exact=True)
                check(y[c], ref, exact, "step %d filter %d ch %d" % (step, fid, c), coef_tol=1e-3 if (step == 2 and fid == 1) else 0.0)
    with pytest.raises(gpu.MiError):
        bank.set_params(5, fd.FLT_BT_RLC_BELL, 1, 1000.0, 1000.0, 1.0, 0.0)
    with pytest.raises(gpu.MiError):
        bank.set_params(0, fd.FLT_BT_RLC_ENVELOPE, 1, 1000.0, 1000.0, 1.0, 0.0)
    with pytest.raises(gpu.MiError):
        bank.process(0, dout, din, None, n)                  # an active filter needs its gain rows
    bank.close()


def coefficient_sensitivity(r, fid, x, g, memory64, exact, rng):
    """How far the output moves when the per-sample design moves by what separates two libms (device / numpy: tanf, expf,
    logf, sqrtf inside the designer): the cut-off and the gain curve one float32 ulp up or down -- which the design's
    cancellations (a1 = 2 (B2 kf^2 - B0) / (...) next to z = 1, the matched transform's normalisation) turn into many ulps
    of a coefficient -- and every resulting coefficient two ulps on top.  float64 recursion from the same memory, so this is
    the sensitivity of the FILTER, not round-off of the recursion."""
    p = r.params[fid]
    f0 = p["fFreq"]
    worst = 0.0
    try:
        for k in range(3):
            p["fFreq"] = np.nextafter(np.float32(f0), np.float32(np.inf if (k & 1) else -np.inf)) if k < 2 else f0
            gg = np.nextafter(g, np.where(rng.integers(0, 2, g.shape) == 1, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32))
            coef = np.asarray(r.coefficients(fid, gg.astype(np.float32)), np.float32)
            nc = coef.shape[0]
            up = np.nextafter(np.nextafter(coef, np.float32(np.inf)), np.float32(np.inf))
            dn = np.nextafter(np.nextafter(coef, np.float32(-np.inf)), np.float32(-np.inf))
            pert = np.where(rng.integers(0, 2, coef.shape) == 1, up, dn).astype(np.float32)
            yp, _ = oracle.binding.dyn_biquad_cascade_f64(x, pert, memory64[:nc])
            worst = max(worst, float(np.abs(yp - exact).max()))
    finally:
        p["fFreq"] = f0
    return worst


@pytest.mark.parametrize("seed", range(8))
def test_random_operation_sequences(gpu, seed):
    """Differential stress: two filters per object re-parameterised at random (type changes clear every filter's memory at
    the next process(), anything else keeps it), sample-rate changes, every gain shape, ragged and in-place calls -- against
    one oracle object per channel run through the same script.  tests/experiments/stress_sweep.py runs it over any seeds.
    The yardsticks are read over the channel's last 1024 outputs (a call of a few samples has no peak or noise of its own):
    the float32 recursion's own noise (conftest's IIR rule) plus the filter's sensitivity to a one-ulp move of the design's
    inputs (coefficient_sensitivity), which is what separates the device's libm from numpy's inside the designer."""
    rng = np.random.default_rng(19000 + seed)
    C, NF = 3, 2
    bank = gpu.DynFilterBank(C, NF)
    refs = [df.DynamicFilters(NF) for _ in range(C)]

    def both(name, *a):
        getattr(bank, name)(*a)
        for r in refs:
            getattr(r, name)(*a)

    def retune(fid):
        t = int(rng.choice(TYPES))
        slope = int(rng.integers(1, 4))
        if df.cascade_count(t, slope) > 16:
            slope = 1
        f1, f2 = float(rng.uniform(700.0, 9000.0)), float(rng.uniform(700.0, 9000.0))
        both("set_params", fid, t, slope, f1, f2, 1.0, float(rng.uniform(0.0, 1.5)))
        return t
    both("set_sample_rate", SR)
    types = [retune(f) for f in range(NF)]
    matched_seen = [not (t & 1) for t in types]              # a matched-Z type since the memory was last cleared (see check())
    # per channel and filter, while the memory lives: the oracle's last 1024 outputs (float32, float64) and the largest
    # coefficient sensitivity seen
    recent = [[[np.zeros(0), np.zeros(0), 0.0] for _ in range(NF)] for _ in range(C)]
    for f in range(NF):
        both("set_filter_active", f, True)
    log = []
    for step in range(14):
        op = rng.choice(["process", "process", "process", "retune", "rate"])
        if op == "process":
            fid = int(rng.integers(0, NF))
            n = int(rng.choice([1, 15, 16, 17, 1000, 1024, 1025, 2500, int(rng.integers(1, 4000))]))
            kind = str(rng.choice(["constant", "sweep", "jumpy"]))
            x = (rng.standard_normal((C, n)) * 0.25).astype(np.float32)
            g = gains(rng, C, n, kind)
            din, dg = gpu.DeviceBuffer.from_host(x), gpu.DeviceBuffer.from_host(g)
            dout = din if rng.integers(0, 2) else gpu.DeviceBuffer((C, n))
            bank.process(fid, dout, din, dg, n)
            y = dout.download()
            for c in range(C):
                r = refs[c]
                if r.clear_mem:                              # a type change: every filter starts from silence at this call
                    for f in range(NF):
                        recent[c][f] = [np.zeros(0), np.zeros(0), 0.0]
                mem64 = np.zeros_like(r.memory64[fid]) if r.clear_mem else r.memory64[fid].copy()
                ref, exact = r.process(fid, x[c], g[c], exact=True)
                w = recent[c][fid]
                w[0] = np.concatenate([w[0], ref])[-max(n, 1024):]
                w[1] = np.concatenate([w[1], exact])[-max(n, 1024):]
                w[2] = max(w[2], coefficient_sensitivity(r, fid, x[c], g[c], mem64, exact, rng))
                peak = max(float(np.abs(w[1]).max()), 1e-30)
                noise = float(np.abs(w[0] - w[1]).max()) / peak
                sens = w[2] / peak
                e32 = float(np.abs(y[c] - ref).max()) / peak
                e64 = float(np.abs(y[c] - exact).max()) / peak
                msg = "seed %d step %d filter %d ch %d %s n %d %s: vs oracle %.2e, vs float64 %.2e, oracle's own noise %.2e, one-ulp design sensitivity %.2e" \
                      % (seed, step, fid, c, fd.FILTER_TYPES[types[fid]], n, log[-6:], e32, e64, noise, sens)
                assert np.all(np.isfinite(y[c])), msg
                # Measured over seeds 2000-2599 (15 000 checks, MI_TEST_TRACE): bilinear types -- 99.96 % inside the plain IIR
                # rule, the three others at <= 0.24 of 4 x sensitivity, worst error 4.2e-5; the sensitivity itself has a
                # long tail (1 % of the designs move by 1e-2 for one ulp of the cut-off), hence the cap.  Matched-Z types:
                # 12 % beyond the plain rule, worst 3.7e-4 -- the normalisation next to z = 1 (Filter.cpp:2369-2411) turns
                # the last bit of an expf into 1e-4 of a numerator, which a perturbation of the inputs does not reproduce.
                extra = min(4.0 * sens, 1e-4) + (1e-3 if matched_seen[fid] else 0.0)
                record_parity("dynamic filters script: |gpu - exact| <= max(1e-5, 4 noise) + min(4 x one-ulp design sensitivity, 1e-4) (+1e-3 matched-Z)",
                              e64, max(TOL, IIR_EXACT_FACTOR * noise) + extra, noise=noise, sensitivity=sens)
                if os.environ.get("MI_TEST_TRACE"):
                    with open(os.environ["MI_TEST_TRACE"], "a") as f:
                        f.write("%d %g %g %g %g %d\n" % (types[fid], e64, e32, noise, sens, int(matched_seen[fid])))
                assert e64 <= max(TOL, IIR_EXACT_FACTOR * noise) + extra and e32 <= max(TOL, IIR_REF_FACTOR * noise) + extra, msg
        elif op == "retune":
            fid = int(rng.integers(0, NF))
            old = types[fid]
            types[fid] = retune(fid)
            if types[fid] != old:                            # every filter's memory goes at the next process()
                matched_seen = [not (t & 1) for t in types]
            elif not (types[fid] & 1):
                matched_seen[fid] = True
        else:
            both("set_sample_rate", int(rng.choice([44100, 48000, 96000])))
        log.append(str(op))
    bank.close()
