"""Timing of mi_correlometer_bank and mi_panometer_bank (not a test, not bench.py): 1024 channels x 4096 samples, in one session
    the correlometer at periods 40 and 2400 (max_period 2400),
    the panometer at periods 40 and 2400 under both laws,
    and beside them the sidechain bank's two-input RMS row at N = 2400: the window detector the project already has.
Device events around a warmed-up window of calls (us per call) and around single launches (the kernel's own time,
mi_dspu_profile_next_launch, median of 20); one JSON line.  Every row carries its bytes-per-sample model -- 8 in (two rows), 4 out,
8 into the two rings and, where the period reaches past the tile, 8 back out of them for the tail samples (at period 40 the
40 samples before each tile instead: 8 * 40 / 256) -- against HBM at 8 TB/s, cycles per sample and chain at 2.4 GHz, and the
ratio of the kernel time to the sidechain row's.
Usage: python tests/bench_stereo_meters.py [--channels C] [--samples S] [--calls K] [--warmup W]"""
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
MAX_PERIOD = 2400


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=1024)
    ap.add_argument("--samples", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    mi = importlib.import_module("lsp-dsp-units_amd")
    if mi.device_count() <= 0:
        raise SystemExit("bench_stereo_meters: no HIP device (there is no CPU fallback)")
    import sidechain_ref as sr
    lib, C, n = mi.lib, a.channels, a.samples
    rng = np.random.default_rng(1)
    x = (rng.standard_normal((C, n)) * 0.25).astype(np.float32)
    y = (0.6 * x + 0.8 * rng.standard_normal((C, n)) * 0.25).astype(np.float32)
    da, db, dout = mi.DeviceBuffer.from_host(x), mi.DeviceBuffer.from_host(y), mi.DeviceBuffer((C, n))
    ev0, ev1 = ctypes.c_void_p(), ctypes.c_void_p()
    mi.check(lib.mi_dspu_event_create(ctypes.byref(ev0)))
    mi.check(lib.mi_dspu_event_create(ctypes.byref(ev1)))

    def correlometer(period):
        b = mi.CorrelometerBank(C, MAX_PERIOD)
        for ch in range(C):
            b.configure(ch, period)
        b.update_settings()
        return b

    def panometer(period, law):
        b = mi.PanometerBank(C, MAX_PERIOD)
        for ch in range(C):
            b.configure(ch, period, law=law)
        b.update_settings()
        return b

    side = mi.SidechainBank(C, 2, 50.0)
    for ch in range(C):
        side.configure(ch, 48000, 50.0, sr.SCM_RMS, sr.SCS_MIDDLE)
    side.update_settings()
    banks = {"correlometer_n40": correlometer(40), "correlometer_n2400": correlometer(2400),
             "panometer_linear_n40": panometer(40, 0), "panometer_linear_n2400": panometer(2400, 0),
             "panometer_equal_power_n40": panometer(40, 1), "panometer_equal_power_n2400": panometer(2400, 1)}
    cases = [("sidechain_rms_n2400_two_inputs_middle", 20.0, lambda: side.process(dout, da, db, n))]
    cases += [(name, 28.0 if name.endswith("n2400") else 20.0 + 8.0 * 40 / 256, (lambda b=b: b.process(dout, da, db, n)))
              for name, b in banks.items()]
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
                     "msamples_per_s": round(C * n / us, 1), "bytes_per_sample": round(nbytes, 2),
                     "hbm_bound_us": round(C * n * nbytes / HBM * 1e6, 3),
                     "cycles_per_sample_and_chain": round(kus * 1e-6 * CLOCK / n, 2),
                     "ratio_to_sidechain": round(kus / rows[0]["kernel_us"], 3) if rows else 1.0})
    print(json.dumps({"bench": "stereo_meters", "channels": C, "samples": n, "calls": a.calls, "rows": rows}))


if __name__ == "__main__":
    main()
