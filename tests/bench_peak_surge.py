"""Timing of mi_peakmeter_bank and mi_surge_bank (not a test, not bench.py): 1024 channels x 4096 samples, in one session
    the peak meter with and without dst (hold 257 samples, release 5 ms) and its block-rate process_value,
    the surge protector's process, process without out and process_mul (transition 257, shutdown 300),
    and beside them the sidechain bank's PEAK row (one input) and the compressor's process without an envelope row: the cheapest
    and the dearest chain the tile walk already carries.
Device events around a warmed-up window of calls (us per call) and around single launches (the kernel's own time,
mi_dspu_profile_next_launch, median of 20); one JSON line.  Every row carries its bytes-per-sample model against HBM at 8 TB/s,
cycles per sample and chain at 2.4 GHz, and the ratios of the kernel time to the sidechain row's and to the compressor's.
Usage: python tests/bench_peak_surge.py [--channels C] [--samples S] [--calls K] [--warmup W]"""
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
        raise SystemExit("bench_peak_surge: no HIP device (there is no CPU fallback)")
    import compressor_ref as cr
    import sidechain_ref as sr
    lib, C, n = mi.lib, a.channels, a.samples
    rng = np.random.default_rng(1)
    # bursts every 600 samples or so over quiet noise: the meter holds, decays and is overtaken; the level comes and goes
    x = (rng.standard_normal((C, n)) * 0.05).astype(np.float32)
    x[rng.random((C, n)) < 1.0 / 600] = 0.9
    level = np.where((np.arange(n)[None, :] // 700 + np.arange(C)[:, None]) % 2 == 0, 0.9, 0.05).astype(np.float32)
    dx, dlevel, dout = mi.DeviceBuffer.from_host(x), mi.DeviceBuffer.from_host(level), mi.DeviceBuffer((C, n))
    dpeaks = mi.DeviceBuffer((C,))
    ev0, ev1 = ctypes.c_void_p(), ctypes.c_void_p()
    mi.check(lib.mi_dspu_event_create(ctypes.byref(ev0)))
    mi.check(lib.mi_dspu_event_create(ctypes.byref(ev1)))

    side = mi.SidechainBank(C, 1, 50.0)
    comp = mi.CompressorBank(C)
    peak = mi.PeakMeterBank(C)
    surge = mi.SurgeProtectorBank(C)
    for ch in range(C):
        side.configure(ch, 48000, 50.0, sr.SCM_PEAK, sr.SCS_MIDDLE)
        comp.configure(ch, **cr.channel_settings(ch))
        peak.configure(ch, 48000, 257.5 / 48.0, 5.0)
        surge.configure(ch, 257, 300, 0.5, 0.25)
    side.update_settings()
    comp.update_settings()
    peak.update_settings()
    surge.process(None, None, 0)
    cases = [("sidechain_peak_one_input", 8, lambda: side.process(dout, dx, None, n)),
             ("compressor_process_no_env", 8, lambda: comp.process(dout, None, dx, n)),
             ("peakmeter_process", 8, lambda: peak.process(dout, dx, n, peaks=dpeaks)),
             ("peakmeter_process_no_dst", 4, lambda: peak.process(None, dx, n, peaks=dpeaks)),
             ("peakmeter_process_value", 8.0 / n, lambda: peak.process_value(dpeaks, dx, 64)),
             ("surge_process", 8, lambda: surge.process(dout, dlevel, n)),
             ("surge_process_no_out", 4, lambda: surge.process(None, dlevel, n)),
             ("surge_process_mul", 12, lambda: surge.process_mul(dout, dlevel, n))]
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
                     "msamples_per_s": round(C * n / us, 1), "bytes_per_sample": round(nbytes, 4),
                     "hbm_bound_us": round(C * n * nbytes / HBM * 1e6, 3),
                     "cycles_per_sample_and_chain": round(kus * 1e-6 * CLOCK / n, 2),
                     "ratio_to_sidechain_peak": round(kus / rows[0]["kernel_us"], 3) if rows else 1.0,
                     "ratio_to_compressor": round(kus / rows[1]["kernel_us"], 3) if len(rows) > 1 else None})
    print(json.dumps({"bench": "peak_surge", "channels": C, "samples": n, "calls": a.calls, "rows": rows}))


if __name__ == "__main__":
    main()
