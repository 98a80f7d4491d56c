"""Every bank on a caller's own non-blocking stream: same bits as on the default stream.  A non-blocking stream does not
wait for the null stream and is not waited for by it, so an internal launch or copy that went to the wrong stream races
with the rest of the call and shows up as a difference.  The eight newer banks are created, configured per channel and called at
once on the stream, with a setting changed between the first and the second call, while the null stream is kept busy."""
import ctypes

import numpy as np
import pytest

from oracle import filter_design as fd
import compressor_ref as cr
import dynproc_ref as dr
import expander_ref as er
import gate_ref as gr
import workloads as wl

pytestmark = pytest.mark.gpu
C, N, CALLS = 64, 4096, 3
# the envelope dynamics: bank class, per-channel settings, the setting changed on a few channels between the first and the second call
DYNAMICS = {
    "compressor": ("CompressorBank", cr.channel_settings, lambda b: (b.set_ratio(3, 2.5), b.set_timings(40, 0.7, 3.3))),
    "expander": ("ExpanderBank", er.channel_settings, lambda b: (b.set_ratio(3, 2.5), b.set_timings(40, 0.7, 3.3))),
    "gate": ("GateBank", gr.channel_settings, lambda b: (b.set_threshold(3, 0.2, 0.08), b.set_threshold(40, 0.12, 0.05))),
    "dynproc": ("DynamicProcessorBank", dr.channel_settings,
                lambda b: (b.set_attack_time(3, 0, 0.7),
                           b.set_dot(42, [i for i, d in enumerate(dr.channel_settings(42)["dots"]) if d is not None][0], None))),
}
NEWER = ("dynfilter", "truepeak", "oversampler", "sidechain") + tuple(DYNAMICS)


def _sidechain_settings(ch, shift=0):
    """Distinct, valid settings of a sidechain channel (max reactivity 10 ms): RMS and UNIFORM in turn, every source, both stereo
    modes, windows from 1 to 457 samples."""
    k = ch + shift
    return dict(sample_rate=48000, reactivity=0.02 + 0.15 * k, mode=(1, 3)[k % 2], source=k % 6, stereo_mode=(k // 6) % 2,
                gain=(1.0, 0.5, -1.5, 2.0)[k % 4])


@pytest.fixture(scope="module")
def side_stream(gpu):
    hip = ctypes.CDLL("libamdhip64.so")
    s = ctypes.c_void_p()
    assert hip.hipStreamCreateWithFlags(ctypes.byref(s), 1) == 0          # hipStreamNonBlocking
    yield s.value
    hip.hipStreamDestroy(s)


def _run(gpu, kind, st):
    rng = np.random.default_rng(33)
    calls = 6 if kind == "ilufs" else CALLS              # the integrated meter reads 0 until its first 400 ms block is full
    xs = [(rng.standard_normal((C, N)) * 0.25).astype(np.float32) for _ in range(calls)]
    outs = []
    buf = lambda shape=(C, N): gpu.DeviceBuffer(shape)                    # noqa: E731
    change = last = lambda: []                      # between the first and the second call; one further call after the last
    ds = load = None
    if kind in NEWER:
        if st is not None:
            # Memsets of 1 GiB keep the null stream busy for milliseconds while st runs on: whatever a bank sends to the null
            # stream without waiting for it -- at creation or with a changed setting -- then lands after the work on st that
            # needed it, and the bits differ.
            load = gpu.DeviceBuffer((1 << 28,))
            busy = lambda: [gpu.check(gpu.lib.mi_dspu_memset(ctypes.c_void_p(load.ptr), 0, load.size * 4, None)) for _ in range(16)]   # noqa: E731
        else:
            busy = lambda: None                                                              # noqa: E731
        # inputs and outputs are on the device before the bank exists: nothing of the test's own stands between the bank's
        # creation (which initialises device memory on the null stream), its configuration and its first process() on st
        if kind in DYNAMICS:
            xs = [np.abs(x) for x in xs]
        ds = [gpu.DeviceBuffer.from_host(x, stream=st) for x in xs]
        y, z = buf(), buf()
        busy()                                      # ... in front of the bank's creation
    if kind in DYNAMICS:
        cls, settings, alter = DYNAMICS[kind]
        b = getattr(gpu, cls)(C)
        for c in range(C):
            b.configure(c, **settings(c))
        step = lambda d: (b.process(y, z, d, N, stream=st), [y, z])[1]                       # noqa: E731  (gain, env)
        change = lambda: alter(b)                                                            # noqa: E731
        last = lambda: (b.process_apply(y, ds[0], ds[1], N, stream=st), [y])[1]              # noqa: E731
    elif kind == "sidechain":
        seconds = iter([gpu.DeviceBuffer.from_host((rng.standard_normal((C, N)) * 0.25).astype(np.float32), stream=st) for _ in xs])
        b = gpu.SidechainBank(C, 2, 10.0)
        for c in range(C):
            b.configure(c, **_sidechain_settings(c))
        step = lambda d: (b.process(y, d, next(seconds), N, stream=st), [y])[1]              # noqa: E731
        # a higher rate makes the channel's ring longer: all rings are re-made on st (the reactivity alone keeps the ring)
        change = lambda: (b.set_sample_rate(5, 96000), b.set_reactivity(5, 7.5), b.set_mode(9, b.SCM_LPF))   # noqa: E731
    elif kind == "truepeak":
        pk = buf((C,))
        b = gpu.TruePeakBank(C); b.set_sample_rate(48000)
        step = lambda d: (b.process(y, d, N, stream=st), b.process_max(pk, d, N, stream=st), [y, pk])[2]     # noqa: E731
        change = lambda: b.set_sample_rate(96000)                                            # noqa: E731  (four times -> twice)
    elif kind == "oversampler":
        b = gpu.OversamplerBank(C); b.set_sample_rate(48000); b.set_mode(b.MODES["4X16BIT"]); b.set_filtering(True)
        b.update_settings(stream=st)
        step = lambda d: (b.process(y, d, N, stream=st), [y])[1]                             # noqa: E731
        # eight times: the state is cleared, the filter designed anew and the scratch grows, all on st
        change = lambda: (b.set_mode(b.MODES["8X16BIT"]), b.update_settings(stream=st))      # noqa: E731
    elif kind == "dynfilter":
        gains = iter([gpu.DeviceBuffer.from_host(np.exp(rng.uniform(-1.0, 1.0, (C, N))).astype(np.float32), stream=st) for _ in xs])
        b = gpu.DynFilterBank(C, 2); b.set_sample_rate(48000)
        b.set_params(0, fd.FLT_BT_RLC_BELL, 2, 1200.0, 5000.0, 1.0, 0.6); b.set_filter_active(0)
        b.set_params(1, fd.FLT_BT_BWC_LOPASS, 2, 3000.0, 3000.0, 1.0, 0.6); b.set_filter_active(1)

        def step(d):
            g = next(gains)
            b.process(0, y, d, g, N, stream=st)
            b.process(1, z, y, g, N, stream=st)
            return [y, z]
        change = lambda: b.set_params(1, fd.FLT_BT_RLC_HISHELF, 1, 2500.0, 2500.0, 1.0, 0.6)   # noqa: E731  (a new type clears the memory)
    elif kind == "biquad":
        b = gpu.BiquadBank(C, 8)
        q = wl.design(fd.FLT_BT_LRX_LOPASS, 4, 3000.0, 0, 1.0, 0.75)
        for c in range(C):
            b.set_chains(c, q)
        step = lambda d: (lambda y: (b.process(y, d, N, stream=st), [y])[1])(buf())          # noqa: E731
    elif kind == "convolver":
        b = gpu.ConvolverBank(rng.standard_normal((C, 9000)).astype(np.float32), 11, stream=st)
        step = lambda d: (lambda y: (b.process(y, d, N, stream=st), [y])[1])(buf())          # noqa: E731
    elif kind == "equalizer":
        b = gpu.EqualizerBank(C, 4, 11); b.set_mode(2); b.set_sample_rate(48000)
        for c in range(C):
            b.set_params(0, fd.FLT_BT_RLC_BELL, 1, 500.0 + 100.0 * c, 1000.0, 2.0, 1.0, channel=c)
        step = lambda d: (lambda y: (b.process(y, d, N, stream=st), [y])[1])(buf())          # noqa: E731
    elif kind == "spectral":
        b = gpu.SpectralBank(C, 12); b.set_rank(11)
        b.bind_mask(np.linspace(0.0, 1.0, 2 << 11).astype(np.float32), stream=st)
        step = lambda d: (lambda y: (b.process(y, d, N, stream=st), [y])[1])(buf())          # noqa: E731
    elif kind == "analyzer":
        b = gpu.AnalyzerBank(C, 12, 48000, 1.0, 0)
        for what, v in ((b.SAMPLE_RATE, 48000), (b.RATE, 48000 / 2048.0), (b.RANK, 12), (b.WINDOW, 0), (b.REACTIVITY, 0.2), (b.SHIFT, 1.0)):
            b.configure(what, v)

        def step(d):
            b.process(d, N, stream=st)
            r = buf((2049,))
            b.reduce_bins(r, stream=st)
            return [r]
    elif kind == "delay":
        b = gpu.DelayBank(C, 6000)
        for c in range(C):
            b.set_delay(50 * c, channel=c)
        step = lambda d: (lambda y: (b.process(y, d, N, stream=st), [y])[1])(buf())          # noqa: E731
    elif kind == "loudness":
        b = gpu.LoudnessBank(C // 2, 2, 400.0); b.set_sample_rate(48000)
        step = lambda d: (lambda y, c: (b.process(y, c, d, N, stream=st), [y, c])[1])(buf((C // 2, N)), buf())   # noqa: E731
    elif kind == "ilufs":
        b = gpu.ILUFSBank(C // 2, 2, 10.0, 400.0); b.set_sample_rate(48000)
        step = lambda d: (lambda y: (b.process(y, d, N, stream=st), [y])[1])(buf((C // 2, N)))                    # noqa: E731
    elif kind == "splitter":
        b = gpu.SplitterBank(C, 12, 3); b.set_rank(11); b.set_chunk_rank(9)
        b.bind_copy(0, stream=st)
        b.bind_mask(1, np.linspace(1.0, 0.0, 1 << 11).astype(np.float32), stream=st)
        b.bind_mask(2, np.linspace(0.0, 1.0, 1 << 11).astype(np.float32), stream=st)
        step = lambda d: (lambda ys: (b.process(ys, d, N, stream=st), ys)[1])([buf(), buf(), buf()])             # noqa: E731
    else:
        b = gpu.CrossoverBank(C, 3); b.set_sample_rate(48000)
        for i, f in enumerate((500.0, 4000.0)):
            b.set_slope(i, 2); b.set_frequency(i, f)
        step = lambda d: (lambda ys: (b.process(ys, d, N, stream=st), ys)[1])([buf(), buf(), buf()])             # noqa: E731
    for k, x in enumerate(xs):
        if k == 1:
            if load is not None:
                busy()                              # ... and in front of the changed settings
            change()
        d = ds[k] if ds is not None else gpu.DeviceBuffer.from_host(x, stream=st)
        outs.extend(o.download(stream=st) for o in step(d))
    outs.extend(o.download(stream=st) for o in last())
    b.close()
    if load is not None:
        load.free()
    return outs


@pytest.mark.parametrize("kind", ["biquad", "convolver", "equalizer", "spectral", "analyzer", "delay", "loudness", "ilufs",
                                  "splitter", "crossover", "dynfilter", "truepeak", "oversampler", "compressor", "sidechain",
                                  "expander", "gate", "dynproc"])
def test_side_stream_gives_the_same_bits(gpu, side_stream, kind):
    ref = _run(gpu, kind, None)
    for _ in range(2):
        got = _run(gpu, kind, side_stream)
        assert len(got) == len(ref)
        assert max(float(np.abs(r).max()) for r in ref) > 0.0
        for a, r in zip(got, ref):
            assert np.isfinite(r).all()
            np.testing.assert_array_equal(a, r)


def test_two_banks_on_two_streams_do_not_disturb_each_other(gpu):
    """Two convolver banks and two spectral banks fed alternately on two non-blocking streams, nothing waited for until the
    end: each gives what it gives alone (the banks share only read-only tables)."""
    hip = ctypes.CDLL("libamdhip64.so")
    streams = []
    for _ in range(2):
        s = ctypes.c_void_p()
        assert hip.hipStreamCreateWithFlags(ctypes.byref(s), 1) == 0
        streams.append(s.value)
    rng = np.random.default_rng(44)
    irs = [rng.standard_normal((C, 20000)).astype(np.float32) for _ in range(2)]
    xs = [[(rng.standard_normal((C, N)) * 0.25).astype(np.float32) for _ in range(4)] for _ in range(2)]
    masks = [np.linspace(0.0, 1.0, 2 << 11).astype(np.float32), np.linspace(1.0, 0.0, 2 << 11).astype(np.float32)]

    def make(i, st):
        cv = gpu.ConvolverBank(irs[i], 11, stream=st)
        sp = gpu.SpectralBank(C, 12); sp.set_rank(11); sp.bind_mask(masks[i], stream=st)
        return cv, sp

    alone = []
    for i in range(2):
        cv, sp = make(i, None)
        res = []
        for x in xs[i]:
            d, y, z = gpu.DeviceBuffer.from_host(x), gpu.DeviceBuffer((C, N)), gpu.DeviceBuffer((C, N))
            cv.process(y, d, N); sp.process(z, y, N)
            res.append(z.download())
        alone.append(res)
        cv.close(); sp.close()

    banks = [make(i, streams[i]) for i in range(2)]
    ins = [[gpu.DeviceBuffer.from_host(x, stream=streams[i]) for x in xs[i]] for i in range(2)]
    mids = [[gpu.DeviceBuffer((C, N)) for _ in range(4)] for _ in range(2)]
    outs = [[gpu.DeviceBuffer((C, N)) for _ in range(4)] for _ in range(2)]
    for k in range(4):
        for i in range(2):
            banks[i][0].process(mids[i][k], ins[i][k], N, stream=streams[i])
            banks[i][1].process(outs[i][k], mids[i][k], N, stream=streams[i])
    for i in range(2):
        for k in range(4):
            np.testing.assert_array_equal(outs[i][k].download(stream=streams[i]), alone[i][k])
        banks[i][0].close(); banks[i][1].close()
    for s in streams:
        hip.hipStreamDestroy(ctypes.c_void_p(s))


def test_two_dynamics_chains_on_two_streams_do_not_disturb_each_other(gpu):
    """Two chains sidechain -> compressor process_apply -> true-peak process_max with different settings, fed alternately on
    two non-blocking streams for four calls, nothing waited for until the end: each gives the bits it gives alone on the
    default stream."""
    hip = ctypes.CDLL("libamdhip64.so")
    streams = []
    for _ in range(2):
        s = ctypes.c_void_p()
        assert hip.hipStreamCreateWithFlags(ctypes.byref(s), 1) == 0
        streams.append(s.value)
    rng = np.random.default_rng(45)
    xs = [[(rng.standard_normal((C, N)) * 0.25).astype(np.float32) for _ in range(4)] for _ in range(2)]

    def make(i):
        sc = gpu.SidechainBank(C, 1, 10.0)
        cp = gpu.CompressorBank(C)
        for c in range(C):
            sc.configure(c, **_sidechain_settings(c, shift=3 * i))
            cp.configure(c, **cr.channel_settings(c + 7 * i))
        tp = gpu.TruePeakBank(C); tp.set_sample_rate((48000, 96000)[i])
        return sc, cp, tp

    def feed(banks, x, mid, out, pk, st):
        sc, cp, tp = banks
        sc.process(mid, x, None, N, stream=st)
        cp.process_apply(out, x, mid, N, stream=st)
        tp.process_max(pk, out, N, stream=st)

    alone = []
    for i in range(2):
        banks = make(i)
        res = []
        for x in xs[i]:
            d, mid, out, pk = gpu.DeviceBuffer.from_host(x), gpu.DeviceBuffer((C, N)), gpu.DeviceBuffer((C, N)), gpu.DeviceBuffer((C,))
            feed(banks, d, mid, out, pk, None)
            res.append((out.download(), pk.download()))
        alone.append(res)
        for b in banks:
            b.close()
    assert all(np.isfinite(o).all() and np.abs(o).max() > 0.0 and p.min() > 0.0 for res in alone for o, p in res)

    ins = [[gpu.DeviceBuffer.from_host(x, stream=streams[i]) for x in xs[i]] for i in range(2)]
    mids, outs = ([[gpu.DeviceBuffer((C, N)) for _ in range(4)] for _ in range(2)] for _ in range(2))
    peaks = [[gpu.DeviceBuffer((C,)) for _ in range(4)] for _ in range(2)]
    chains = [make(i) for i in range(2)]
    for k in range(4):
        for i in range(2):
            feed(chains[i], ins[i][k], mids[i][k], outs[i][k], peaks[i][k], streams[i])
    for i in range(2):
        for k in range(4):
            np.testing.assert_array_equal(outs[i][k].download(stream=streams[i]), alone[i][k][0])
            np.testing.assert_array_equal(peaks[i][k].download(stream=streams[i]), alone[i][k][1])
        for b in chains[i]:
            b.close()
    for s in streams:
        hip.hipStreamDestroy(ctypes.c_void_p(s))


def test_biquad_bank_inside_a_hip_graph(gpu):
    """The biquad bank keeps everything that changes from call to call (filter memory) on the device and takes no host
    decision in a steady-state process(): a run of calls can be captured once into a hipGraph and replayed.  Three replays
    of a four-call graph equal twelve eager calls, bit for bit."""
    hip = ctypes.CDLL("libamdhip64.so")
    s = ctypes.c_void_p()
    assert hip.hipStreamCreateWithFlags(ctypes.byref(s), 1) == 0
    st = s.value
    rng = np.random.default_rng(55)
    q = wl.design(fd.FLT_BT_LRX_LOPASS, 4, 3000.0, 0, 1.0, 0.75)
    xs = [(rng.standard_normal((C, N)) * 0.25).astype(np.float32) for _ in range(4)]

    def bank():
        b = gpu.BiquadBank(C, 8)
        for c in range(C):
            b.set_chains(c, q)
        b.commit(st)
        return b

    eager = bank()
    ref = []
    for rep in range(3):
        for x in xs:
            d, y = gpu.DeviceBuffer.from_host(x, stream=st), gpu.DeviceBuffer((C, N))
            eager.process(y, d, N, stream=st)
            ref.append(y.download(stream=st))
    eager.close()

    b = bank()
    ins = [gpu.DeviceBuffer.from_host(x, stream=st) for x in xs]
    outs = [gpu.DeviceBuffer((C, N)) for _ in xs]
    graph, exe = ctypes.c_void_p(), ctypes.c_void_p()
    del d, y                                    # (a buffer released while the stream captures would end the capture)
    import gc
    gc.collect()
    assert hip.hipStreamBeginCapture(s, 0) == 0
    for k in range(4):
        b.process(outs[k], ins[k], N, stream=st)
    assert hip.hipStreamEndCapture(s, ctypes.byref(graph)) == 0
    assert hip.hipGraphInstantiate(ctypes.byref(exe), graph, None, None, ctypes.c_size_t(0)) == 0
    for rep in range(3):
        assert hip.hipGraphLaunch(exe, s) == 0
        for k, y in enumerate(outs):
            np.testing.assert_array_equal(y.download(stream=st), ref[rep * 4 + k])
    hip.hipGraphExecDestroy(exe); hip.hipGraphDestroy(graph)
    b.close()
    hip.hipStreamDestroy(s)
