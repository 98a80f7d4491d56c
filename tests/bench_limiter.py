"""Timing of mi_limiter_bank (not a test, not bench.py), after bench_gate.py: 1024 channels x 4096 samples, in one session
    no_patches        a signal that never exceeds the threshold: the floor.  MODEL: per channel 4 B read and 4 B written per sample
                      and the window's round trip, 2 x 4 ML x 4 B; the row reports bytes / kernel time and its fraction of
                      --hbm-gbs (the machine's streaming rate as measured elsewhere; 4000 GB/s unless given)
    sparse_bursts     about one patch per chunk
    dense             noise at four times the threshold: us per call and ns per patch -- the arg-max and the patch, the figure the
                      kernel is to be judged by
    alr               the same quiet signal with the ALR follower on: its serial chain on one lane per channel
    process_apply     bursts, with the delayed audio
    ml3840 / ml240    HERM_THIN, 48 kHz, 5 ms look-ahead (the reference test's configuration) at init(192000, 20) and init(48000, 5)
    and mi_compressor_bank's process in the same session: the yardstick.
Figures as tests/bench_expander.py takes them (kernel time from events, median of 20; us per call over a warmed-up window).
One JSON line.
Usage: python tests/bench_limiter.py [--channels C] [--samples S] [--calls K] [--warmup W] [--repeats R] [--hbm-gbs G]"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=1024)
    ap.add_argument("--samples", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--hbm-gbs", type=float, default=4000.0)
    a = ap.parse_args()
    mi = importlib.import_module("lsp-dsp-units_amd")
    if mi.device_count() <= 0:
        raise SystemExit("bench_limiter: no HIP device (there is no CPU fallback)")
    import compressor_ref as cr
    import limiter_ref as lr
    from bench_expander import measure
    C, n = a.channels, a.samples
    rng = np.random.default_rng(1)
    xq = (0.05 * rng.standard_normal((C, n))).astype(np.float32)
    xs = xq.copy()
    xs[:, n // 2] = 1.5
    xd = rng.standard_normal((C, n)).astype(np.float32)
    xb = lr.bursts(2, C, n, every=1500)
    dq, ds, dd, db = (mi.DeviceBuffer.from_host(x) for x in (xq, xs, xd, xb))
    daudio, dgain, denv = mi.DeviceBuffer.from_host(xb[::-1].copy()), mi.DeviceBuffer((C, n)), mi.DeviceBuffer((C, n))

    def bank(max_sr=48000, max_la=5.0, threshold=0.5, alr=False, same=False):
        b = mi.LimiterBank(C, max_sr, max_la)
        for ch in range(C):
            if same:
                b.configure(ch, 48000, 0, 0.5, 5.0, 1.5, 1.5, knee=1.0)
            else:
                b.configure(ch, 48000, ch % 12, threshold, 1.0 + 0.004 * (ch % 1000), 0.5 + 0.001 * (ch % 1000), 1.0 + 0.002 * (ch % 1000),
                            alr=alr, alr_attack=1.0, alr_release=20.0)
        b.update_settings()
        return b

    comp = mi.CompressorBank(C)
    for ch in range(C):
        comp.configure(ch, **cr.channel_settings(ch))
    comp.update_settings()
    plain, dense, alr, big, small = bank(), bank(threshold=0.25), bank(alr=True), bank(192000, 20.0, same=True), bank(same=True)
    cases = [("no_patches", lambda: plain.process(dgain, dq, n)),
             ("sparse_bursts", lambda: plain.process(dgain, ds, n)),
             ("dense", lambda: dense.process(dgain, dd, n)),
             ("alr", lambda: alr.process(dgain, dq, n)),
             ("process_apply", lambda: plain.process_apply(dgain, daudio, db, n)),
             ("ml3840_herm_thin_5ms", lambda: big.process(dgain, ds, n)),
             ("ml240_herm_thin_5ms", lambda: small.process(dgain, ds, n)),
             ("compressor_process_bursts", lambda: comp.process(dgain, denv, db, n))]
    rows = measure(mi, cases, n, a.calls, a.warmup, max(a.repeats, 5))
    banks = {"no_patches": plain, "sparse_bursts": plain, "dense": dense, "alr": alr, "process_apply": plain, "ml3840_herm_thin_5ms": big,
             "ml240_herm_thin_5ms": small}
    for row, (name, call) in zip(rows, cases):
        del row["cycles_per_sample_and_chain"]
        b = banks.get(name)
        if b is None:
            continue
        call()                                                      # the patches of one more call of this case
        st = [b.get_state(ch) for ch in range(C)]
        patches = np.array([s[2] for s in st])
        row["patches_per_channel_median_max"] = [int(np.median(patches)), int(patches.max())]
        row["overruns"] = int(sum(s[4] for s in st))
        if patches.max() > 0:
            # the workgroups of a launch run side by side: the time per patch of ONE channel's loop is the kernel time over the
            # waves of workgroups the device runs one after another, which this row cannot see; it reports time x CUs / patches
            row["ns_per_patch_and_cu"] = round(row["kernel_us"] * 1e3 * 256 / float(patches.sum()), 2)
        if name == "no_patches":
            ml = 240
            byts = C * (8.0 * n + 2 * 4 * ml * 4)
            row["model_bytes"] = int(byts)
            row["model_us_at_hbm_rate"] = round(byts / (a.hbm_gbs * 1e3), 3)
            row["fraction_of_model"] = round(byts / (a.hbm_gbs * 1e3) / row["kernel_us"], 3)
    print(json.dumps({"bench": "limiter", "channels": C, "samples": n, "calls": a.calls, "repeats": max(a.repeats, 5), "rows": rows}))


if __name__ == "__main__":
    main()
