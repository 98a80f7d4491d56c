"""The stream kernels' pipeline positions and sub-block counters (biquad_stream_kernel, biquad_stream_chain_kernel), bit for bit.

One mi_biquad_bank_process_blocks call walks the 2048-sample sub-blocks of all its blocks in one launch: wave w of a channel's
workgroup takes sub-blocks w, w + NW, ..., found through two counters (block, sub-block of the block) that go on by NW sub-blocks a
turn, and hands the filter state on through a cell per pipeline position.  Three ways to the same result are compared here on
the `uint32` views of every output and of the filter memory:

  * the process_blocks call (the stream kernel),
  * the same blocks as separate process() calls on a second bank with the same chains and start state,
  * the same process_blocks call under MI_DSPU_TEST_PATH=blocks_loop (the super-block loop of the one-block kernel).

The shapes are those where a wrong position or a wrong counter shows: 1, 8 and 9 channels; blocks of one full and one 16-sample
sub-block (2064), of two full ones (4096) and of three with the last partial (4112); 2 blocks (of 2064 samples: four sub-blocks, the
smallest launch with four waves, and a pipeline longer than the work), 3 and 5 (sub-block counts that are no multiple of four)
and 20 (the bench's); 1, 8, 12 (scan operands in LDS) and 13 (not in LDS) sections.  Every case makes a second call on the
same bank straight after the first: the state the last position's wave wrote is the state the next call starts from.
Input: seeded noise at 0.25, low-pass cut-offs from 200 Hz up.
"""
import numpy as np
import pytest

from oracle import filter_design as fd

import workloads as wl

pytestmark = pytest.mark.gpu

WAYS = ("blocks", "separate", "blocks_loop")


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def chain(c, sections):
    """`sections` low-pass sections for channel c: cut-offs 200 Hz (channel 0) and up."""
    parts, k = [], 0
    while sum(len(p) for p in parts) < sections:
        parts.append(wl.design(fd.FLT_BT_LRX_LOPASS, 4, 200.0 * (c + 1) + 310.0 * k, 0, 1.0, 0.75))
        k += 1
    return np.concatenate(parts)[:sections].astype(np.float32)


def run(gpu, monkeypatch, way, coef, max_sec, x, off=(), plan=None):
    """x: [calls][blocks][C][n].  plan(bufs of the call's inputs) -> (ins, outs, buffers to read back); default: an output
    buffer per block.  Returns the buffers read back after every call and the filter memory after every call."""
    calls, nb, C, n = x.shape
    if way == "blocks_loop":
        monkeypatch.setenv("MI_DSPU_TEST_PATH", "blocks_loop")
    else:
        monkeypatch.delenv("MI_DSPU_TEST_PATH", raising=False)
    bank = gpu.BiquadBank(C, max_sec)
    try:
        for c in range(C):
            bank.set_chains(c, coef[c], False)
        for c in off:
            bank.set_row_enabled(c, False)
        got, states = [], []
        for call in range(calls):
            bufs = [gpu.DeviceBuffer.from_host(x[call, b]) for b in range(nb)]
            if plan is None:
                ins, outs = bufs, [gpu.DeviceBuffer.from_host(np.full((C, n), 7.0, np.float32)) for _ in range(nb)]
                back = outs
            else:
                ins, outs, back = plan(bufs)
            if way == "separate":
                for o, i in zip(outs, ins):
                    bank.process(o, i, n)
            else:
                bank.process_blocks(outs, ins, n)
            got.append([b.download() for b in back])
            states.append(bank.get_state())
    finally:
        bank.close()
        monkeypatch.delenv("MI_DSPU_TEST_PATH", raising=False)
    return got, states


def compare(gpu, monkeypatch, coef, max_sec, x, what, off=(), plan=None):
    res = {way: run(gpu, monkeypatch, way, coef, max_sec, x, off, plan) for way in WAYS}
    ref_out, ref_state = res["separate"]
    assert any(np.abs(b).max() > 1e-3 for b in ref_out[-1]), what          # (the comparison is not one of silence)
    for way in ("blocks", "blocks_loop"):
        out, state = res[way]
        for call in range(len(ref_out)):
            for b, (u, v) in enumerate(zip(out[call], ref_out[call])):
                assert same_bits(u, v), "%s: %s against separate calls, call %d, buffer %d: %d samples differ" % (
                    what, way, call, b, int(np.count_nonzero(u.view(np.uint32) != v.view(np.uint32))))
            assert same_bits(state[call], ref_state[call]), "%s: %s against separate calls, filter memory after call %d" % (what, way, call)


def noise(seed, shape):
    return (np.random.default_rng(seed).standard_normal(shape) * 0.25).astype(np.float32)


@pytest.mark.parametrize("sections", [1, 8, 12, 13])
@pytest.mark.parametrize("nb", [2, 3, 5, 20])
@pytest.mark.parametrize("n", [2064, 4096, 4112])
@pytest.mark.parametrize("C", [1, 8, 9])
def test_blocks_call_separate_calls_and_block_loop_give_the_same_bits(gpu, monkeypatch, C, n, nb, sections):
    """Every combination of the shapes above, two calls each."""
    coef = [chain(c, sections) for c in range(C)]
    x = noise(1000 * C + n + 17 * nb + sections, (2, nb, C, n))
    compare(gpu, monkeypatch, coef, sections, x, "C %d, n %d, %d blocks, %d sections" % (C, n, nb, sections))


@pytest.mark.parametrize("n,nb", [(2064, 2), (4112, 3), (4096, 5)])
def test_section_counts_that_differ_and_a_row_switched_off(gpu, monkeypatch, n, nb):
    """Nine channels with 8, 7, ..., 1 and no sections, row 2 switched off (its output buffer keeps what it held)."""
    C = 9
    coef = [chain(c, 8 - c) if c < 8 else np.zeros((0, 5), np.float32) for c in range(C)]
    x = noise(31 + n + nb, (2, nb, C, n))
    compare(gpu, monkeypatch, coef, 8, x, "mixed bank, n %d, %d blocks" % (n, nb), off=(2,))


@pytest.mark.parametrize("C,n,nb", [(9, 4112, 5), (1, 2064, 2)])
def test_blocks_processed_in_place(gpu, monkeypatch, C, n, nb):
    coef = [chain(c, 8) for c in range(C)]
    x = noise(77 + C + n, (2, nb, C, n))
    compare(gpu, monkeypatch, coef, 8, x, "in place, C %d, n %d, %d blocks" % (C, n, nb), plan=lambda bufs: (bufs, bufs, bufs))


def test_an_output_buffer_that_comes_round_four_sub_blocks_later(gpu, monkeypatch):
    """A ring of two output buffers under blocks of two sub-blocks: block b and block b + 2 write the same rows, four sub-blocks
    apart -- through the same pipeline position, so through the same wave, in order.  What is read back is what the last two
    blocks left."""
    C, n, nb = 9, 4096, 5
    coef = [chain(c, 8) for c in range(C)]
    x = noise(4242, (2, nb, C, n))

    def plan(bufs):
        ring = [gpu.DeviceBuffer.from_host(np.full((C, n), 7.0, np.float32)) for _ in range(2)]
        return bufs, [ring[b % 2] for b in range(len(bufs))], ring
    compare(gpu, monkeypatch, coef, 8, x, "ring of two outputs", plan=plan)


def test_crossover_run_of_blocks_against_block_by_block(gpu):
    """biquad_stream_chain_kernel shares the loop: a Crossover of two split points (three bands), 8 channels, 5 blocks of 4096 as one
    call against the same blocks one call each on a twin bank, every band, and a further block through both (the memories)."""
    C, bands, n, K = 8, 3, 4096, 5
    x = noise(555, (K + 1, C, n))

    def make():
        bank = gpu.CrossoverBank(C, bands)
        bank.set_sample_rate(48000)
        for i, f in enumerate((200.0, 3000.0)):
            bank.set_slope(i, 2)
            bank.set_frequency(i, f)
        return bank
    a, b = make(), make()
    try:
        dins = [gpu.DeviceBuffer.from_host(x[k]) for k in range(K + 1)]
        mk = lambda: [gpu.DeviceBuffer.from_host(np.full((C, n), 7.0, np.float32)) for _ in range(bands)]
        oa, ob = [mk() for _ in range(K + 1)], [mk() for _ in range(K + 1)]
        a.process_blocks(oa[:K], dins[:K], n)
        a.process(oa[K], dins[K], n)
        for k in range(K + 1):
            b.process(ob[k], dins[k], n)
        for k in range(K + 1):
            for q in range(bands):
                ya, yb = oa[k][q].download(), ob[k][q].download()
                assert np.abs(yb).max() > 1e-3 and not np.any(yb == 7.0)
                assert same_bits(ya, yb), "block %d band %d" % (k, q)
    finally:
        a.close()
        b.close()
