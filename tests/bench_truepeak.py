"""Timing of mi_truepeak_bank (not a test, not bench.py): 1024 channels x 4096 samples, N = 2, 4, 8, process and process_max.
Device events around a warmed-up window of calls (us per call, Msamples/s) and around single launches (the kernel's own
time, mi_dspu_profile_next_launch); one JSON line with both against the two bounds:
    bytes  8 B per sample for process (read + write), 4 for process_max; HBM 8 TB/s
    ops    (N - 1) * 2a multiplies and as many adds, plus N max operations, per input sample; vector unit
           256 CUs x 4 SIMDs x 32 packed-f32 operations per clock (2.4 GHz)
Usage: python tests/bench_truepeak.py [--channels C] [--samples S] [--calls K] [--warmup W]"""
import argparse
import ctypes
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM = 8.0e12
VALU = 256 * 4 * 32 * 2.4e9
A = 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=1024)
    ap.add_argument("--samples", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    mi = importlib.import_module("lsp-dsp-units_amd")
    if mi.device_count() <= 0:
        raise SystemExit("bench_truepeak: no HIP device (there is no CPU fallback)")
    lib, C, n = mi.lib, a.channels, a.samples
    x = (np.random.default_rng(1).standard_normal((C, n)) * 0.5).astype(np.float32)
    din, dout, peaks = mi.DeviceBuffer.from_host(x), mi.DeviceBuffer((C, n)), mi.DeviceBuffer((C,))
    ev0, ev1 = ctypes.c_void_p(), ctypes.c_void_p()
    mi.check(lib.mi_dspu_event_create(ctypes.byref(ev0)))
    mi.check(lib.mi_dspu_event_create(ctypes.byref(ev1)))
    rows = []
    for times, sr in ((4, 48000), (2, 96000), (8, 22050)):
        for mode in ("process", "process_max"):
            bank = mi.TruePeakBank(C)
            bank.set_sample_rate(sr)
            call = (lambda: bank.process(dout, din, n)) if mode == "process" else (lambda: bank.process_max(peaks, din, n))
            for _ in range(a.warmup):
                call()
            mi.check(lib.mi_dspu_stream_synchronize(None))
            mi.check(lib.mi_dspu_event_record(ev0, None))
            for _ in range(a.calls):
                call()
            mi.check(lib.mi_dspu_event_record(ev1, None))
            mi.check(lib.mi_dspu_event_synchronize(ev1))
            ms = ctypes.c_float()
            mi.check(lib.mi_dspu_event_elapsed_ms(ctypes.byref(ms), ev0, ev1))
            us = ms.value * 1e3 / a.calls
            kernel = []                                         # the process kernel's own duration (events at its begin / end)
            for _ in range(20):
                mi.check(lib.mi_dspu_profile_next_launch(ev0, ev1))
                call()
                mi.check(lib.mi_dspu_event_synchronize(ev1))
                mi.check(lib.mi_dspu_event_elapsed_ms(ctypes.byref(ms), ev0, ev1))
                kernel.append(ms.value * 1e3)
            kus = float(np.median(kernel))
            samples = C * n
            nbytes = samples * (8 if mode == "process" else 4)
            ops = samples * ((times - 1) * 2 * A * 2 + times)
            hbm_us, valu_us = nbytes / HBM * 1e6, ops / VALU * 1e6
            rows.append({"times": times, "mode": mode, "us_per_call": round(us, 3), "msamples_per_s": round(samples / us, 1),
                         "kernel_us": round(kus, 3), "hbm_bound_us": round(hbm_us, 3), "valu_bound_us": round(valu_us, 3),
                         "bound": "vector" if valu_us >= hbm_us else "hbm", "of_bound": round(max(hbm_us, valu_us) / us, 3),
                         "kernel_of_bound": round(max(hbm_us, valu_us) / kus, 3)})
            bank.close()
    print(json.dumps({"bench": "truepeak", "channels": C, "samples": n, "calls": a.calls, "rows": rows}))


if __name__ == "__main__":
    main()
