"""Timing of mi_oversampler_bank (not a test, not bench.py): 1024 channels x 4096 samples; upsample, downsample and
process at 2X16BIT, 4X16BIT, 8X16BIT, 4X2 and 8X24BIT.  Device events around a warmed-up window of calls (us per call)
and, for upsample, around single launches of the upsample kernel (its own time, mi_dspu_profile_next_launch); one JSON
line with both against the models, per INPUT sample:
    upsample    bytes 4 + 4N (read the input, write N values); operations (N - 1) * 2a multiplies and as many adds
    downsample  bytes 12N + 4: the filter reads and writes N values, the decimation reads their lines and writes one value
    process     bytes 16N + 8: upsample, the filter in place, the decimation; the upsample's operations
    HBM 8 TB/s; vector unit 256 CUs x 4 SIMDs x 32 packed-f32 operations per clock (2.4 GHz).  The filter's own
    arithmetic is the biquad bank's (bench.py prices it) and is not modelled here.
Usage: python tests/bench_oversampler.py [--channels C] [--samples S] [--calls K] [--warmup W]"""
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
MODES = ("2X16BIT", "4X16BIT", "8X16BIT", "4X2", "8X24BIT")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=1024)
    ap.add_argument("--samples", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    mi = importlib.import_module("lsp-dsp-units_amd")
    if mi.device_count() <= 0:
        raise SystemExit("bench_oversampler: no HIP device (there is no CPU fallback)")
    lib, C, n = mi.lib, a.channels, a.samples
    x = (np.random.default_rng(1).standard_normal((C, n)) * 0.5).astype(np.float32)
    din, dout, dover = mi.DeviceBuffer.from_host(x), mi.DeviceBuffer((C, n)), mi.DeviceBuffer((C, 8 * n))
    dover.zero()
    ev0, ev1 = ctypes.c_void_p(), ctypes.c_void_p()
    mi.check(lib.mi_dspu_event_create(ctypes.byref(ev0)))
    mi.check(lib.mi_dspu_event_create(ctypes.byref(ev1)))
    ms = ctypes.c_float()
    rows = []
    for name in MODES:
        bank = mi.OversamplerBank(C)
        bank.set_mode(mi.OversamplerBank.MODES[name])
        bank.set_sample_rate(48000)
        bank.update_settings()
        bank.reserve(n)
        N, lat = bank.oversampling(), bank.latency()
        calls = {"upsample": lambda: bank.upsample(dover, din, n), "downsample": lambda: bank.downsample(dout, dover, n),
                 "process": lambda: bank.process(dout, din, n)}
        for what in ("upsample", "downsample", "process"):
            call = calls[what]
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
            samples = C * n
            nbytes = samples * {"upsample": 4 + 4 * N, "downsample": 12 * N + 4, "process": 16 * N + 8}[what]
            ops = 0 if what == "downsample" else samples * (N - 1) * 2 * lat * 2
            hbm_us, valu_us = nbytes / HBM * 1e6, ops / VALU * 1e6
            row = {"mode": name, "what": what, "us_per_call": round(us, 3), "hbm_model_us": round(hbm_us, 3),
                   "valu_model_us": round(valu_us, 3), "bound": "vector" if valu_us >= hbm_us else "hbm",
                   "of_bound": round(max(hbm_us, valu_us) / us, 3)}
            if what == "upsample":                              # the upsample kernel's own duration (events at its begin / end)
                kernel = []
                for _ in range(20):
                    mi.check(lib.mi_dspu_profile_next_launch(ev0, ev1))
                    call()
                    mi.check(lib.mi_dspu_event_synchronize(ev1))
                    mi.check(lib.mi_dspu_event_elapsed_ms(ctypes.byref(ms), ev0, ev1))
                    kernel.append(ms.value * 1e3)
                kus = float(np.median(kernel))
                row.update(kernel_us=round(kus, 3), kernel_of_bound=round(max(hbm_us, valu_us) / kus, 3))
            rows.append(row)
        bank.close()
    print(json.dumps({"bench": "oversampler", "channels": C, "samples": n, "calls": a.calls, "rows": rows}))


if __name__ == "__main__":
    main()
