"""mi_depopper_bank (lsp::dspu::Depopper) on the device against tests/depopper_ref.py fed the bank's own designed values and fade
tables through the getters: env, gain, every state word and the logical contents of both buffers bit for bit on every channel
(NaN at the same positions), after every call.  Across tiles, workgroups and both buffer wraps; every RMS length, fade length,
delay and mode on both sides of the tile and of the 32-sample refresh; events on tile and call edges, several in a tile, patches
over one another and into the previous call; thresholds met exactly, silences, subnormals, NaN and Inf; setters and init()
between calls; in place, strides, a NULL env, one call against split calls, the state's round trip; graph capture, two streams,
lifetime, bad arguments; the reference's recorded cases."""
import ctypes
import os
import sys

import numpy as np
import pytest

import depopper_ref as dr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_depopper_vectors as gen  # noqa: E402

T, G = 256, 4                           # tile_chain_device.h: samples of a tile, channels of a workgroup
f32 = np.float32
u32 = np.uint32
SR = 48000
CHANNELS = [1, G - 1, G, G + 1, 2 * G + 1]
COUNTS = [1, 31, 32, 33, T - 1, T, T + 1, 2 * T + 3]
UNEVEN = (113, 1, T, 31, 700, T + 1, 32, 33, T - 1, 2 * T + 3)
# (max_rms ms, nRmsLen, fade-out, fade-in, fade-in delay, fade-out delay, fade-in mode, fade-out mode), times in samples
GRID = [(1.0, 48, 480, 300, 0, 0, 0, 0), (2.0, 1, 0, 0, 0, 0, 1, 1), (2.0, 31, 1, 1, 1, 0, 2, 2), (2.0, 32, T - 1, 300, 0, 1, 3, 3),
        (2.0, 33, T + 1, 300, 40, 40, 4, 4), (1.0, 48, 480, 1, 1, 40, 0, 3), (2.0, 96, 480, 300, 0, 0, 2, 1), (2.0, 96, 0, 300, 40, 1, 4, 0),
        (1.0, 1, T + 1, 0, 0, 40, 1, 2), (1.0, 32, 1, 300, 1, 1, 3, 4), (2.0, 33, T - 1, 1, 40, 0, 0, 2), (1.0, 31, 480, 300, 0, 40, 2, 3)]


def _same(got, want):
    """bit for bit; NaN at the same positions whatever its payload"""
    got, want = np.ascontiguousarray(got, f32), np.ascontiguousarray(want, f32)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(u32)[~nan], want.view(u32)[~nan])


def _apply(bank, ref, ch, op):
    """One recorded operation (make_depopper_vectors) on channel ch of the bank and on its restatement; the setters' returns agree."""
    w, a = int(op[0]), op[1:]
    if w == gen.INIT:
        bank.init(ch, int(a[0]), a[1], a[2])
        ref.init(int(a[0]), a[1], a[2])
        return
    name = {gen.IN_MODE: "set_fade_in_mode", gen.OUT_MODE: "set_fade_out_mode", gen.IN_TIME: "set_fade_in_time", gen.OUT_TIME: "set_fade_out_time",
            gen.IN_THRESH: "set_fade_in_threshold", gen.OUT_THRESH: "set_fade_out_threshold", gen.IN_DELAY: "set_fade_in_delay",
            gen.OUT_DELAY: "set_fade_out_delay", gen.RMS_LENGTH: "set_rms_length"}[w]
    arg = int(a[0]) if w in (gen.IN_MODE, gen.OUT_MODE) else a[0]
    got, want = getattr(bank, name)(ch, arg), getattr(ref, name)(arg)
    assert got == want or (got != got and want != want), (name, got, want)


def _feed(bank, ch):
    return lambda: (bank.get_params(ch), bank.get_fade_table(ch, 0), bank.get_fade_table(ch, 1))


def _setup_ops(row, **more):
    max_rms, rms, fo, fi, di, do, mi_, mo = row
    return gen.setup(max_rms=max_rms, rms=rms, fade_out=fo, fade_in=fi, in_delay=di, out_delay=do, in_mode=mi_, out_mode=mo, **more)


def _make(gpu, rows, **more):
    """A bank with one GRID row per channel and the restatements, each fed its channel's getters."""
    bank = gpu.DepopperBank(len(rows))
    refs = []
    for ch, row in enumerate(rows):
        ref = dr.Depopper()
        ref.feed = _feed(bank, ch)
        for op in _setup_ops(row, **more):
            _apply(bank, ref, ch, op)
        refs.append(ref)
    bank.update_settings()
    for ch, row in enumerate(rows):
        p = bank.get_params(ch)
        assert (p["rms_len"], p["fade_out"]["samples"], p["fade_in"]["samples"], p["fade_in"]["delay_samples"], p["fade_out"]["delay_samples"]) == row[1:6]
        assert p["look_count"] == row[1] + row[2] and p["reconfigure"] == 0 and bank.latency(ch) == row[2]
    return bank, refs


def _rows(C, shift=0):
    return [GRID[(ch + shift) % len(GRID)] for ch in range(C)]


def _signal(seed, C, n):
    """Bursts of noise between stretches of exact silence or of a hiss, of lengths on both sides of the tile and of the fades, so
    that events fall on tile and call edges in one channel or another."""
    rng = np.random.default_rng(seed)
    x = np.zeros((C, n))
    for ch in range(C):
        at = int(rng.integers(0, 40))
        while at < n:
            burst = int(rng.choice([1, 3, 40, T - 2, T, T + 3, 500]))
            x[ch, at:at + burst] = 0.5 * rng.standard_normal(min(burst, n - at))
            at += burst
            gap = int(rng.choice([1, 3, 40, T - 2, T, T + 3, 800]))
            if rng.random() < 0.3:
                x[ch, at:at + gap] = 1e-3 * rng.standard_normal(min(gap, max(n - at, 0)))
            at += gap
    return x.astype(f32)


def _same_state(bank, refs, what=""):
    for ch, ref in enumerate(refs):
        s = bank.get_state(ch, buffers=True)
        w = ref.state_words()
        assert _same(s["rms"], f32(ref.fRms)), (what, ch, "fRms", s["rms"], ref.fRms)
        assert [s["state"], s["counter"], s["delay"], s["rms_off"], s["look_off"]] == [int(v) for v in w[1:]], (what, ch, s, w)
        rb, gb = ref.buffers()
        assert _same(s["rms_buf"], rb), (what, ch, "the squares")
        assert _same(s["gain_buf"], gb), (what, ch, "the gains")


def _call(gpu, bank, refs, x, what="", env=True, stream=None):
    """One process() of x [C, n] on the bank and on the restatements; env, gain and the state are compared."""
    C, n = x.shape
    bank.update_settings(stream=stream)                         # the getters that feed the restatements are current
    want = [ref.process(x[ch]) for ch, ref in enumerate(refs)]
    dx = gpu.DeviceBuffer.from_host(x)
    de, dg = gpu.DeviceBuffer.from_host(np.full((C, n), 7.0, f32)), gpu.DeviceBuffer.from_host(np.full((C, n), 7.0, f32))
    bank.process(de if env else None, dg, dx, n, stream=stream)
    e, g = de.download(stream), dg.download(stream)
    for ch in range(C):
        if env:
            bad = np.argwhere(e[ch].view(u32) != want[ch][0].view(u32))
            assert _same(e[ch], want[ch][0]), (what, "env", ch, n, bad[:4].ravel(), e[ch][bad[:4]].ravel(), want[ch][0][bad[:4]].ravel())
        else:
            assert np.all(e[ch] == 7.0), (what, "a NULL env was written")
        bad = np.argwhere(g[ch].view(u32) != want[ch][1].view(u32))
        assert _same(g[ch], want[ch][1]), (what, "gain", ch, n, bad[:4].ravel(), g[ch][bad[:4]].ravel(), want[ch][1][bad[:4]].ravel())
    _same_state(bank, refs, what)
    return e, g


def _stream_calls(gpu, bank, refs, x, calls, what=""):
    at, k = 0, 0
    while at < x.shape[1]:
        m = min(calls[k % len(calls)], x.shape[1] - at)
        _call(gpu, bank, refs, x[:, at:at + m], (what, at, m))
        at, k = at + m, k + 1


@pytest.mark.gpu
@pytest.mark.parametrize("C", CHANNELS)
def test_channels_and_counts(gpu, C):
    """Every count as a call of its own, one after the other on the same bank: the state carries over."""
    bank, refs = _make(gpu, _rows(C, C))
    x = _signal(10 + C, C, 2 * sum(COUNTS))
    _stream_calls(gpu, bank, refs, x, COUNTS + COUNTS[::-1])
    bank.close()


@pytest.mark.gpu
def test_every_setting_of_the_grid(gpu):
    bank, refs = _make(gpu, GRID)
    _stream_calls(gpu, bank, refs, _signal(20, len(GRID), 2600), UNEVEN)
    bank.close()


@pytest.mark.gpu
@pytest.mark.parametrize("shift", [0, 6])
def test_streams_past_both_buffer_wraps(gpu, shift):
    """nRmsMax - nRmsMin and nLookMax - nLookMin are 0x1000 here: 9000 samples wrap both twice, at offsets of their own."""
    C = G + 1
    bank, refs = _make(gpu, _rows(C, shift))
    for ch in range(C):
        p = bank.get_params(ch)
        assert p["rms_max_off"] - p["rms_min_off"] == 0x1000 and p["look_max_off"] - p["look_min_off"] == 0x1000
    _stream_calls(gpu, bank, refs, _signal(30 + shift, C, 9000), UNEVEN[::-1] if shift else UNEVEN)
    bank.close()


def _gate(n, bursts):
    x = np.zeros(n, f32)
    for lo, hi in bursts:
        x[lo:hi] = 1.0
    return x


@pytest.mark.gpu
def test_events_on_edges_and_several_in_a_tile(gpu):
    """With an RMS length of 1 the envelope is |x|: a burst [lo, hi) of ones opens at lo and has its event at hi.  Events at the
    first and the last sample of a tile and of a call; two and three in one tile (fade, wait, closed, fade) with patches over one
    another; a fade-out begun before the fade-in is over; a patch that reaches back into the previous call."""
    n = 4 * T
    rows = [(1.0, 1, 480, 300, 0, 0, 0, 0), (1.0, 1, T - 1, 300, 0, 0, 1, 4), (1.0, 1, 40, 10, 0, 1, 2, 2), (2.0, 1, T + 1, 0, 0, 0, 3, 3),
            (1.0, 1, 100, 300, 1, 0, 4, 1)]
    shapes = [[(10, T), (T + 40, 2 * T - 1), (2 * T + 1, 3 * T)],                              # events at 256, 511, 768: tile edges
              [(5, 8), (11, 14), (17, 60), (300, 303), (306, 309), (600, 700)],                # three in tile 0, two in tile 1
              [(0, 1), (3, 4), (6, 7), (9, 200), (T - 1, T), (2 * T, 2 * T + 1)],              # every third sample, and single ones on edges
              [(20, 120), (130, 140), (500, 700), (701, 702), (1000, 1023)],
              [(100, 101), (110, 400), (402, 420), (800, 1024)]]                               # still open at the end
    for calls in ((n,), (T, 1, T - 1, 44, 300), (11, 3, 3, 500)):
        bank, refs = _make(gpu, rows, in_thr=0.5, out_thr=0.5)
        x = np.stack([_gate(n, s) for s in shapes])
        _stream_calls(gpu, bank, refs, x, calls, calls)
        bank.close()


@pytest.mark.gpu
def test_thresholds_met_exactly_silences_subnormals_nan_and_inf(gpu):
    x = gen.signals()
    rows = [(1.0, 32, 100, 40, 0, 0, 0, 0), (2.0, 32, T + 1, 300, 1, 40, 2, 3), (1.0, 32, 0, 1, 0, 0, 1, 1)]
    bank, refs = _make(gpu, rows, in_thr=0.25, out_thr=0.125)
    sig = np.stack([x[gen.SIG_SPECIAL, :3400]] * 3)
    e, g = _call(gpu, bank, refs, sig[:, :1800], "special")
    assert np.isnan(e).any() and np.any(e == f32(0.25)) and np.any(e == f32(0.125)) and np.any((e > 0) & (e < f32(1e-19)))
    _stream_calls(gpu, bank, refs, sig[:, 1800:], UNEVEN, "special")
    bank.close()
    # the recorded row of silences, 1 to 60 samples between bursts of 70 (the gap of 60 ends at 6040), with gaps of 800, T and
    # 500 laid over it; every length up to 800 is in the test below
    bank, refs = _make(gpu, _rows(3, 4))
    sil = np.stack([x[gen.SIG_SILENCES, :6100]] * 3)
    sil[1, 200:200 + 800] = 0.0
    sil[2, 1000:1000 + T] = 0.0
    sil[2, 2000:2000 + 500] = 0.0
    _stream_calls(gpu, bank, refs, sil, (1300, T + 3, 700), "silences")
    bank.close()


# settings under which a silence ends in every part of the automaton: inside the RMS window (1, 31, 48 and 96 samples) plus the
# fade-out delay (0, 1 and 40), inside a WAIT, after it, with the fade-in (0, 1, 10 and 300) over or not
SILENCE_ROWS = [(1.0, 1, 480, 300, 0, 0, 0, 0), (2.0, 31, T - 1, 1, 0, 40, 2, 3), (2.0, 96, 100, 10, 1, 40, 1, 4), (1.0, 1, 40, 0, 0, 1, 3, 2),
                (2.0, 31, 480, 300, 40, 0, 4, 1), (1.0, 48, T + 1, 10, 0, 40, 0, 0), (2.0, 1, T + 1, 300, 1, 40, 2, 2), (2.0, 96, 480, 1, 0, 1, 3, 0)]


def _silences(C, seed):
    """Every silence length from 1 to 800 once, dealt to the C rows in a shuffled order, each after a burst of 1 to 130 samples
    (so a silence begins and ends on every phase of the tile and of the 32-sample refresh) -> x [C, n], the lengths it holds"""
    rng = np.random.default_rng(seed)
    deal = rng.permutation(np.arange(1, 801)).reshape(C, -1)
    rows = []
    for gaps in deal:
        parts = []
        for gap in gaps:
            burst = int(rng.choice([1, 2, 7, 33, 45, 70, 130]))
            parts += [rng.choice([-1.0, 1.0], burst) * rng.uniform(0.25, 0.75, burst), np.zeros(gap)]
        rows.append(np.concatenate(parts))
    n = max(r.size for r in rows) + 1
    x = np.stack([np.concatenate([r, rng.choice([-1.0, 1.0], n - r.size) * rng.uniform(0.25, 0.75, n - r.size)]) for r in rows]).astype(f32)
    found = set()
    for row in x:                                               # the lengths as the signal itself holds them
        edges = np.flatnonzero(np.diff(np.concatenate([[0], (row == 0).astype(np.int8), [0]])))
        found |= set((edges[1::2] - edges[::2]).tolist())
    return x, found


@pytest.mark.gpu
def test_silence_of_every_length_up_to_800(gpu):
    C = 2 * len(SILENCE_ROWS)
    x, found = _silences(C, 40)
    assert found == set(range(1, 801))
    bank, refs = _make(gpu, SILENCE_ROWS + SILENCE_ROWS)
    _stream_calls(gpu, bank, refs, x, (3001, T + 3, 1777, 2 * T), "every silence")
    bank.close()


@pytest.mark.gpu
def test_setters_and_init_between_calls(gpu):
    """The RMS length (fRms is re-summed over the new one), the fade-out time (nLookCount moves the emission), the modes, the
    thresholds and delays, and init() with new maxima (buffers and offsets start over, nCounter and nDelay stay)."""
    C = 3
    bank, refs = _make(gpu, [(2.0, 48, 480, 300, 0, 0, 0, 0)] * C)
    x = _signal(50, C, 3400)
    steps = [[(gen.RMS_LENGTH, gen.ms_for(10))], [(gen.OUT_TIME, gen.ms_for(100))], [(gen.OUT_MODE, 3), (gen.IN_MODE, 1)],
             [(gen.RMS_LENGTH, gen.ms_for(96, most=2.0)), (gen.OUT_TIME, gen.ms_for(480, most=10.0)), (gen.IN_DELAY, gen.ms_for(5))],
             [(gen.IN_THRESH, 0.3), (gen.OUT_THRESH, 0.2)],
             [(gen.INIT, SR, 5.0, 1.0), (gen.OUT_TIME, gen.ms_for(200)), (gen.RMS_LENGTH, gen.ms_for(40))],
             [(gen.INIT, 44100, 10.0, 2.0)], [(gen.RMS_LENGTH, gen.ms_for(33))]]
    at = 0
    for k, ops in enumerate([[]] + steps):
        for ch in range(C):
            for op in (ops if ch != 1 or k % 2 else []):            # channel 1 takes every other step only
                _apply(bank, refs[ch], ch, np.array(list(op) + [0, 0, 0], np.float64)[:4])
        if ops:
            assert bank.get_params(0)["reconfigure"] == 1
        m = (377, T, 400)[k % 3]
        _call(gpu, bank, refs, x[:, at:at + m], ("step", k))
        at += m
    bank.close()


@pytest.mark.gpu
def test_a_refused_update_touches_no_channel(gpu):
    """Channel 0 asks for a good design, channel 2 for one that is refused: the getters of both go on reporting what the device
    holds, and once channel 2 is mended both designs arrive."""
    C = 3
    bank, refs = _make(gpu, [(2.0, 48, 480, 300, 0, 0, 2, 3)] * C)
    x = _signal(55, C, 3 * 400)
    _call(gpu, bank, refs, x[:, :400], "before")

    def seen(ch):
        p = bank.get_params(ch)
        return ([p["rms_len"], p["look_count"], p["fade_out"]["samples"], p["fade_in"]["samples"], bank.latency(ch)] +
                [int(v) for v in f32(p["rms_norm"]).reshape(1).view(u32)] + [bytes(np.asarray(bank.get_fade_table(ch, k), f32)) for k in (0, 1)])

    def both(ch, what, value):
        _apply(bank, refs[ch], ch, np.array([what, value, 0, 0], np.float64))

    was = [seen(ch) for ch in range(C)]
    both(0, gen.RMS_LENGTH, gen.ms_for(10))
    both(0, gen.OUT_TIME, gen.ms_for(100))
    both(2, gen.OUT_TIME, 10.5)
    for call in (bank.update_settings, lambda: bank.get_state(0)):
        with pytest.raises(gpu.MiError) as err:
            call()
        assert err.value.code == -1 and "channel 2" in str(err.value)
    assert [seen(ch) for ch in range(C)] == was and [bank.get_params(ch)["reconfigure"] for ch in range(C)] == [1, 0, 1]
    # mended (not with the 10 ms it had: the setter compares with the old value clamped to max_fade, and would store nothing)
    both(2, gen.OUT_TIME, gen.ms_for(T - 1))
    _call(gpu, bank, refs, x[:, 400:800], "mended")
    assert seen(0)[:3] == [10, 110, 100] and seen(1) == was[1] and seen(2)[:3] == [48, 48 + T - 1, T - 1]
    _call(gpu, bank, refs, x[:, 800:], "after")
    bank.close()


@pytest.mark.gpu
def test_call_forms(gpu):
    """In place with env as src and with gain as src, rows with strides, a NULL env, and one call against split calls."""
    C, n, stride = G + 1, 2 * T + 77, 2 * T + 96
    x = _signal(60, C, 3 * n)
    whole, refs = _make(gpu, _rows(C, 2))
    want_e, want_g = _call(gpu, whole, refs, x, "one call")
    whole.close()
    bank, refs = _make(gpu, _rows(C, 2))
    # env in place, rows `stride` apart
    pad = np.full((C, stride), 7.0, f32)
    pad[:, :n] = x[:, :n]
    de, dg = gpu.DeviceBuffer.from_host(pad), gpu.DeviceBuffer.from_host(np.full((C, stride), 7.0, f32))
    bank.process(de, dg, de, n, env_stride=stride, gain_stride=stride, src_stride=stride)
    e, g = de.download(), dg.download()
    assert _same(e[:, :n], want_e[:, :n]) and _same(g[:, :n], want_g[:, :n]) and np.all(e[:, n:] == 7.0) and np.all(g[:, n:] == 7.0)
    # gain in place, env apart and unaligned rows (an odd stride)
    odd = np.full((C, n + 1), 7.0, f32)
    odd[:, :n] = x[:, n:2 * n]
    dg, de = gpu.DeviceBuffer.from_host(odd), gpu.DeviceBuffer((C, n))
    bank.process(de, dg, dg, n, gain_stride=n + 1, src_stride=n + 1)
    assert _same(de.download(), want_e[:, n:2 * n]) and _same(dg.download()[:, :n], want_g[:, n:2 * n])
    # no env
    dx, dg = gpu.DeviceBuffer.from_host(x[:, 2 * n:]), gpu.DeviceBuffer((C, n))
    bank.process(None, dg, dx, n)
    assert _same(dg.download(), want_g[:, 2 * n:])
    bank.close()


@pytest.mark.gpu
def test_state_round_trip(gpu):
    """get_state() of one bank, buffers included, set on a fresh twin: the twin goes on with the same bits."""
    C = 3
    bank, refs = _make(gpu, _rows(C, 3))
    x = _signal(70, C, 1500)
    _call(gpu, bank, refs, x[:, :700], "before")
    twin, _ = _make(gpu, _rows(C, 3))
    for ch in range(C):
        s = bank.get_state(ch, buffers=True)
        twin.set_state(ch, s["rms"], s["state"], s["counter"], s["delay"], s["rms_off"], s["look_off"], s["rms_buf"], s["gain_buf"])
    _same_state(twin, refs, "twin")
    _call(gpu, twin, refs, x[:, 700:], "after")
    with pytest.raises(gpu.MiError) as e:
        twin.set_state(0, 0.0, 4, 0, 0, s["rms_off"], s["look_off"])
    assert e.value.code == -1
    with pytest.raises(gpu.MiError) as e:
        twin.set_state(0, 0.0, 0, 0, 0, 0, s["look_off"])
    assert e.value.code == -1
    bank.close()
    twin.close()


@pytest.mark.gpu
def test_recorded_cases(gpu):
    """The reference's own outputs, state words and buffers (the fade tables are this host's, as the recordings' were the
    recording host's: the sine and Gaussian cases rest on the same libm)."""
    x, cases = gen.load()
    for c in cases:
        bank = gpu.DepopperBank(1)
        env, gain, at = [], [], 0
        for op in c["ops"]:
            w = int(op[0])
            if w == gen.PROCESS:
                m = int(op[1])
                dx, de, dg = gpu.DeviceBuffer.from_host(x[c["signal"], at:at + m]), gpu.DeviceBuffer((1, m)), gpu.DeviceBuffer((1, m))
                bank.process(de, dg, dx, m)
                env.append(de.download()[0])
                gain.append(dg.download()[0])
                at += m
            elif w == gen.RECONFIGURE:
                bank.update_settings()
            elif w == gen.INIT:
                bank.init(0, int(op[1]), op[2], op[3])
            else:
                getattr(bank, _SETTERS[w])(0, int(op[1]) if w in (gen.IN_MODE, gen.OUT_MODE) else op[1])
        assert _same(np.concatenate(env), c["env"]), c["name"]
        assert _same(np.concatenate(gain), c["gain"]), c["name"]
        s = bank.get_state(0, buffers=True)
        assert [int(f32(s["rms"]).view(u32)), s["state"], s["counter"], s["delay"], s["rms_off"], s["look_off"]] == [int(v) for v in c["state"]], c["name"]
        assert _same(s["rms_buf"], c["rms_buf"]) and _same(s["gain_buf"], c["gain_buf"]), c["name"]
        bank.close()


@pytest.mark.gpu
def test_cpp_class_on_the_recorded_cases(gpu, tmp_path):
    """lsp::dspu::Depopper of the library: the generator's own driver, compiled against the mirror header and the library instead
    of the reference's sources, on the recorded cases -- env, gain, every state word, the designed values and both host buffers."""
    import subprocess
    pkg = os.path.join(ROOT, "lsp-dsp-units_amd")
    src, exe = str(tmp_path / "driver.cpp"), str(tmp_path / "driver")
    with open(src, "w") as f:
        f.write(gen.DRIVER)
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-DDEPOPPER_NO_TABLES", "-I" + os.path.join(pkg, "include"), "-I" + os.path.join(ROOT, "include"),
                           src, "-o", exe, "-L" + pkg, "-lmi_dspu", "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib"])
    x, cases = gen.load()
    got = gen.run(exe, x, [(c["name"], c["signal"], c["n"], c["ops"]) for c in cases], str(tmp_path))
    for c, r in zip(cases, got):
        assert _same(r["env"], c["env"]) and _same(r["gain"], c["gain"]), c["name"]
        assert np.array_equal(r["state"], c["state"]) and np.array_equal(r["design"], c["design"]), (c["name"], r["state"], c["state"])
        assert _same(r["rms_buf"], c["rms_buf"]) and _same(r["gain_buf"], c["gain_buf"]), c["name"]


_SETTERS = {gen.IN_MODE: "set_fade_in_mode", gen.OUT_MODE: "set_fade_out_mode", gen.IN_TIME: "set_fade_in_time", gen.OUT_TIME: "set_fade_out_time",
            gen.IN_THRESH: "set_fade_in_threshold", gen.OUT_THRESH: "set_fade_out_threshold", gen.IN_DELAY: "set_fade_in_delay",
            gen.OUT_DELAY: "set_fade_out_delay", gen.RMS_LENGTH: "set_rms_length"}


def _stream(gpu):
    st = ctypes.c_void_p()
    gpu.check(gpu.lib.mi_dspu_stream_create(ctypes.byref(st)))
    return st


@pytest.mark.gpu
def test_graph_capture_replays_direct_calls(gpu):
    C, n = 2 * G + 1, T + 100
    st = _stream(gpu)
    (bank, refs), (twin, _) = _make(gpu, _rows(C, 1)), _make(gpu, _rows(C, 1))
    x = _signal(80, C, 9 * n)
    dx = [gpu.DeviceBuffer.from_host(x[:, i * n:(i + 1) * n]) for i in range(3)]
    e, g, te, tg = ([gpu.DeviceBuffer((C, n)) for _ in range(3)] for _ in range(4))
    gpu.check(gpu.lib.mi_dspu_graph_begin_capture(st))
    for i in range(3):
        bank.process(e[i], g[i], dx[i], n, stream=st.value)
    exe = ctypes.c_void_p()
    gpu.check(gpu.lib.mi_dspu_graph_end_capture(st, ctypes.byref(exe)))
    xr = np.concatenate([x[:, :3 * n]] * 3, axis=1)                 # every replay reads the same three blocks
    for rep in range(3):
        gpu.check(gpu.lib.mi_dspu_graph_launch(exe, st))
        for i in range(3):
            twin.process(te[i], tg[i], dx[i], n, stream=st.value)
        got = [np.concatenate([v.download(stream=st.value) for v in bufs], axis=1) for bufs in (e, g, te, tg)]
        want = [ref.process(xr[ch, rep * 3 * n:(rep + 1) * 3 * n]) for ch, ref in enumerate(refs)]
        assert _same(got[0], got[2]) and _same(got[1], got[3]), rep
        assert _same(got[0], np.stack([w[0] for w in want])) and _same(got[1], np.stack([w[1] for w in want])), rep
        _same_state(bank, refs, rep)                                # the state advances on every replay
    gpu.lib.mi_dspu_graph_destroy(exe)
    bank.close()
    twin.close()
    gpu.check(gpu.lib.mi_dspu_stream_destroy(st))


@pytest.mark.gpu
def test_setter_and_state_access_inside_a_capture_are_refused(gpu):
    C, n = 3, T + 100
    st = _stream(gpu)
    bank, refs = _make(gpu, _rows(C))
    x = _signal(90, C, 2 * n)
    d0, d1, de, dg = gpu.DeviceBuffer.from_host(x[:, :n]), gpu.DeviceBuffer.from_host(x[:, n:]), gpu.DeviceBuffer((C, n)), gpu.DeviceBuffer((C, n))
    bank.process(de, dg, d0, n, stream=st.value)
    for ch, ref in enumerate(refs):
        ref.process(x[ch, :n])
    gpu.check(gpu.lib.mi_dspu_graph_begin_capture(st))
    bank.set_rms_length(0, gen.ms_for(20))
    for call in (lambda: bank.process(de, dg, d1, n, stream=st.value), lambda: bank.update_settings(stream=st.value)):
        with pytest.raises(gpu.MiError) as err:
            call()
        assert err.value.code == -5 and "update_settings" in str(err.value)
    for call in (lambda: bank.get_state(1, stream=st.value), lambda: bank.set_state(1, 0.0, 0, 0, 0, 64, 576, stream=st.value)):
        with pytest.raises(gpu.MiError) as err:
            call()
        assert err.value.code == -5 and "captured" in str(err.value)
    gpu.check(gpu.lib.mi_dspu_memset(ctypes.c_void_p(de.ptr), 0, 16, st))              # (so that the capture is not empty)
    exe = ctypes.c_void_p()
    gpu.check(gpu.lib.mi_dspu_graph_end_capture(st, ctypes.byref(exe)))
    gpu.lib.mi_dspu_graph_destroy(exe)
    refs[0].set_rms_length(gen.ms_for(20))
    _call(gpu, bank, refs, x[:, n:], "after the capture", stream=st.value)  # nothing was lost, nothing happened twice
    bank.close()
    gpu.check(gpu.lib.mi_dspu_stream_destroy(st))


@pytest.mark.gpu
def test_two_banks_on_two_streams(gpu):
    C, n, calls = 6, T + 57, 4
    streams = [_stream(gpu) for _ in range(2)]
    made = [_make(gpu, _rows(C, 2)), _make(gpu, _rows(C, 7))]
    sig = [_signal(100 + i, C, calls * n) for i in range(2)]
    ins = [[gpu.DeviceBuffer.from_host(sig[i][:, k * n:(k + 1) * n]) for k in range(calls)] for i in range(2)]
    envs, gains = ([[gpu.DeviceBuffer((C, n)) for _ in range(calls)] for _ in range(2)] for _ in range(2))
    for k in range(calls):
        for i in range(2):
            made[i][0].process(envs[i][k], gains[i][k], ins[i][k], n, stream=streams[i].value)
    for i in range(2):
        e = np.concatenate([v.download(stream=streams[i].value) for v in envs[i]], axis=1)
        g = np.concatenate([v.download(stream=streams[i].value) for v in gains[i]], axis=1)
        want = [ref.process(sig[i][ch]) for ch, ref in enumerate(made[i][1])]
        assert _same(e, np.stack([w[0] for w in want])) and _same(g, np.stack([w[1] for w in want])), i
        made[i][0].close()
    for s in streams:
        gpu.check(gpu.lib.mi_dspu_stream_destroy(s))


def _free_bytes():
    hip = ctypes.CDLL("libamdhip64.so")             # the runtime the library itself runs on (already loaded)
    free, total = ctypes.c_size_t(), ctypes.c_size_t()
    assert hip.hipDeviceSynchronize() == 0
    assert hip.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) == 0
    return free.value


@pytest.mark.gpu
def test_create_use_destroy_returns_device_memory(gpu):
    x = _signal(1, 8, 1024)
    dx, de, dg = gpu.DeviceBuffer.from_host(x), gpu.DeviceBuffer((8, 1024)), gpu.DeviceBuffer((8, 1024))

    def cycle():
        bank = gpu.DepopperBank(8)
        for ch in range(8):
            bank.init(ch, SR, 10.0, 2.0)
            bank.set_rms_length(ch, 1.0)
            bank.set_fade_out_time(ch, 5.0)
        bank.process(de, dg, dx, 1024)
        bank.init(3, SR, 20.0, 4.0)                 # new buffers for one channel
        bank.set_fade_in_time(2, 100.0)             # a longer table
        bank.process(de, dg, dx, 1024)
        bank.close()

    for _ in range(3):
        cycle()
    before = _free_bytes()
    for _ in range(20):
        cycle()
    after = _free_bytes()
    assert before - after < 8 << 20, "%.1f MiB of device memory did not come back after 20 objects" % ((before - after) / 2 ** 20)


@pytest.mark.gpu
def test_bad_arguments_and_refusals_on_a_live_bank(gpu):
    """Every bad argument and every refused configuration comes back as an error code before any launch; nothing is written."""
    import importlib
    capi = importlib.import_module("lsp-dsp-units_amd.capi")
    lib, C, n = gpu.lib, 3, 64
    buf, other = gpu.DeviceBuffer.from_host(np.full((C, n), 7.0, f32)), gpu.DeviceBuffer.from_host(np.full((C, n), 7.0, f32))
    p, q = ctypes.c_void_p(buf.ptr), ctypes.c_void_p(other.ptr)
    bank = gpu.DepopperBank(C)
    h = bank.handle
    assert lib.mi_depopper_bank_process(h, None, q, p, n, n, n, n, None) == -1 and b"init" in lib.mi_dspu_last_error()     # never init()ed
    for ch in range(C):
        bank.init(ch, SR, 10.0, 1.0)
    assert lib.mi_depopper_bank_process(h, None, q, p, n, n, n, n, None) == -1 and b"nRmsLen == 0" in lib.mi_dspu_last_error()
    assert lib.mi_depopper_bank_update_settings(h, None) == -1 and lib.mi_depopper_bank_get_state(h, 0, ctypes.byref(capi.DepopperState()), None, None, None) == -1
    for ch in range(C):
        bank.set_rms_length(ch, 5.0)                                # clamped to max_rms, not refused
    bank.update_settings()
    assert bank.get_params(0)["rms_len"] == 48 and bank.get_params(0)["rms_length"] == f32(1.0)
    for bad, text in ((10.5, b"fade-out"), (-1.0, b"fade-out"), (float("nan"), b"not a number")):
        bank.set_fade_out_time(1, bad)
        assert lib.mi_depopper_bank_process(h, None, q, p, n, n, n, n, None) == -1 and text in lib.mi_dspu_last_error(), bad
        assert b"channel 1" in lib.mi_dspu_last_error()
    bank.set_fade_out_time(1, 10.0)
    bank.set_fade_in_time(2, 30000.0)                               # 1.44e6 samples of table
    assert lib.mi_depopper_bank_process(h, None, q, p, n, n, n, n, None) == -1 and b"2^20" in lib.mi_dspu_last_error()
    bank.set_fade_in_time(2, 1.0)
    assert lib.mi_depopper_bank_process(h, None, q, p, 0, 0, 0, 0, None) == 0                  # nothing to do, the settings are sent
    assert lib.mi_depopper_bank_process(h, None, q, None, n, n, n, n, None) == -1              # no input
    assert lib.mi_depopper_bank_process(h, None, None, p, n, n, n, n, None) == -1              # no gain
    assert lib.mi_depopper_bank_process(h, p, p, q, n, n, n, n, None) == -1                    # env and gain the same
    assert lib.mi_depopper_bank_process(h, None, q, p, n, n, n - 1, n, None) == -1             # a stride shorter than count
    assert lib.mi_depopper_bank_process(h, None, p, p, n, n, n + 4, n, None) == -1             # in place with different strides
    assert lib.mi_depopper_bank_process(h, None, q, p, 1 << 31, 1 << 31, 1 << 31, 1 << 31, None) == -1
    assert lib.mi_depopper_bank_init(h, C, SR, 10.0, 1.0) == -1 and lib.mi_depopper_bank_set_rms_length(h, C, 1.0, None) == -1
    assert lib.mi_depopper_bank_set_fade_in_mode(h, 0, 5, None) == -1 and lib.mi_depopper_bank_init(h, 0, SR, -1.0, 1.0) == -1
    assert lib.mi_depopper_bank_init(h, 0, SR, float("nan"), 1.0) == -1 and lib.mi_depopper_bank_init(h, 0, SR, 1e9, 1.0) == -1
    assert lib.mi_depopper_bank_get_params(h, C, None) == -1 and lib.mi_depopper_bank_latency(h, 0, None) == -1
    assert lib.mi_depopper_bank_get_fade_table(h, 0, 0, None, 0, None) == -1
    assert np.all(buf.download() == 7.0) and np.all(other.download() == 7.0)
    bank.close()
