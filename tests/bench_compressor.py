"""Timing of mi_compressor_bank (not a test, not bench.py): 1024 channels x 4096 samples, in one session
    process with and without env, process_apply, curve alone,
    process with a flat curve (every envelope below both knees: no logf / expf) -- the follower with its loads and stores,
    which says whether the gain pass hides under the follower,
    and the biquad bank's exact mode at one section (mi_biquad_bank_set_exact): the serial recurrence the project already has.
Device events around a warmed-up window of calls (us per call) and around single launches (the kernel's own time,
mi_dspu_profile_next_launch, median of 20); one JSON line.  The follower is a dependent chain per channel, so the figure
next to the times is cycles per sample and chain at 2.4 GHz; bytes against HBM at 8 TB/s are reported as the other bound.
Usage: python tests/bench_compressor.py [--channels C] [--samples S] [--calls K] [--warmup W]"""
import argparse
import ctypes
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM = 8.0e12
CLOCK = 2.4e9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=1024)
    ap.add_argument("--samples", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    mi = importlib.import_module("lsp-dsp-units_amd")
    if mi.device_count() <= 0:
        raise SystemExit("bench_compressor: no HIP device (there is no CPU fallback)")
    import compressor_ref as cr
    lib, C, n = mi.lib, a.channels, a.samples
    x = cr.sidechain(1, C, n)
    din, daudio = mi.DeviceBuffer.from_host(x), mi.DeviceBuffer.from_host(x[::-1].copy())
    dgain, denv = mi.DeviceBuffer((C, n)), mi.DeviceBuffer((C, n))
    ev0, ev1 = ctypes.c_void_p(), ctypes.c_void_p()
    mi.check(lib.mi_dspu_event_create(ctypes.byref(ev0)))
    mi.check(lib.mi_dspu_event_create(ctypes.byref(ev1)))

    def bank(flat=False):
        b = mi.CompressorBank(C)
        for ch in range(C):
            s = cr.channel_settings(ch)
            if flat:
                s.update(mode=cr.CM_DOWNWARD, attack_threshold=1e6, knee=1.0)
            b.configure(ch, **s)
        b.update_settings()
        return b

    biquad = mi.BiquadBank(C, 1)
    biquad.set_all_chains(np.tile(np.array([[[0.2, 0.3, 0.2, 0.5, -0.2]]], np.float32), (C, 1, 1)))
    biquad.set_exact(True)
    biquad.commit()
    full, flat = bank(), bank(True)
    cases = [("process", 12, lambda: full.process(dgain, denv, din, n)),
             ("process_no_env", 8, lambda: full.process(dgain, None, din, n)),
             ("process_apply", 12, lambda: full.process_apply(dgain, daudio, din, n)),
             ("curve", 8, lambda: full.curve(dgain, din, n)),
             ("process_no_env_flat_curve", 8, lambda: flat.process(dgain, None, din, n)),
             ("biquad_exact_1_section", 8, lambda: biquad.process(dgain, din, n))]
    rows = []
    ms = ctypes.c_float()
    for name, nbytes, call in cases:
        for _ in range(a.warmup):
            call()
        mi.check(lib.mi_dspu_stream_synchronize(None))
        mi.check(lib.mi_dspu_event_record(ev0, None))
        for _ in range(a.calls):
            call()
        mi.check(lib.mi_dspu_event_record(ev1, None))
        mi.check(lib.mi_dspu_event_synchronize(ev1))
        mi.check(lib.mi_dspu_event_elapsed_ms(ctypes.byref(ms), ev0, ev1))
        us = ms.value * 1e3 / a.calls
        kernel = []
        for _ in range(20):
            mi.check(lib.mi_dspu_profile_next_launch(ev0, ev1))
            call()
            mi.check(lib.mi_dspu_event_synchronize(ev1))
            mi.check(lib.mi_dspu_event_elapsed_ms(ctypes.byref(ms), ev0, ev1))
            kernel.append(ms.value * 1e3)
        kus = float(np.median(kernel))
        rows.append({"case": name, "us_per_call": round(us, 3), "kernel_us": round(kus, 3), "kernel": mi.last_launch(),
                     "msamples_per_s": round(C * n / us, 1), "hbm_bound_us": round(C * n * nbytes / HBM * 1e6, 3),
                     "cycles_per_sample_and_chain": round(kus * 1e-6 * CLOCK / n, 2)})
    print(json.dumps({"bench": "compressor", "channels": C, "samples": n, "calls": a.calls, "rows": rows}))


if __name__ == "__main__":
    main()
