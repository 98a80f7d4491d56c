"""Timing of mi_sidechain_bank (not a test, not bench.py): 1024 channels x 4096 samples, in one session
    one input in each of the four modes (the window modes at N = 2400), RMS at N = 40 (last out of the same tile),
    two inputs with the MIDDLE source,
    and beside them the compressor bank's flat-curve run (compressor_kernel with every envelope below both knees): the serial
    follower the project already has.
Device events around a warmed-up window of calls (us per call) and around single launches (the kernel's own time,
mi_dspu_profile_next_launch, median of 20); one JSON line.  Every row carries its bytes-per-sample model -- 4 per input row
read, 4 written, and for all modes 4 into the ring, for the window modes 4 back out of it (last, where N reaches past the
tile) -- against HBM at 8 TB/s, and cycles per sample and chain at 2.4 GHz.
Usage: python tests/bench_sidechain.py [--channels C] [--samples S] [--calls K] [--warmup W]"""
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
        raise SystemExit("bench_sidechain: no HIP device (there is no CPU fallback)")
    import compressor_ref as cr
    import sidechain_ref as sr
    lib, C, n = mi.lib, a.channels, a.samples
    x = cr.sidechain(1, C, n)
    din, din1, dout = mi.DeviceBuffer.from_host(x), mi.DeviceBuffer.from_host(x[::-1].copy()), mi.DeviceBuffer((C, n))
    ev0, ev1 = ctypes.c_void_p(), ctypes.c_void_p()
    mi.check(lib.mi_dspu_event_create(ctypes.byref(ev0)))
    mi.check(lib.mi_dspu_event_create(ctypes.byref(ev1)))

    def sidechain(mode, ms, inputs=1):
        b = mi.SidechainBank(C, inputs, 50.0)
        for ch in range(C):
            b.configure(ch, 48000, ms, mode, sr.SCS_MIDDLE)
        b.update_settings()
        return b

    flat = mi.CompressorBank(C)
    for ch in range(C):
        s = cr.channel_settings(ch)
        s.update(mode=cr.CM_DOWNWARD, attack_threshold=1e6, knee=1.0)
        flat.configure(ch, **s)
    flat.update_settings()
    banks = {"peak": sidechain(sr.SCM_PEAK, 50.0), "rms_n2400": sidechain(sr.SCM_RMS, 50.0), "lpf": sidechain(sr.SCM_LPF, 50.0),
             "uniform_n2400": sidechain(sr.SCM_UNIFORM, 50.0), "rms_n40": sidechain(sr.SCM_RMS, 40.5 / 48.0),
             "rms_n2400_two_inputs_middle": sidechain(sr.SCM_RMS, 50.0, 2)}
    # bytes per sample: input rows + output + ring write (+ ring read for `last` beyond the tile)
    model = {"peak": 12, "rms_n2400": 16, "lpf": 12, "uniform_n2400": 16, "rms_n40": 12, "rms_n2400_two_inputs_middle": 20}
    cases = [(name, model[name], (lambda b=b, two=name.endswith("middle"): b.process(dout, din, din1 if two else None, n)))
             for name, b in banks.items()]
    cases.append(("compressor_no_env_flat_curve", 8, lambda: flat.process(dout, None, din, n)))
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
                     "msamples_per_s": round(C * n / us, 1), "bytes_per_sample": nbytes,
                     "hbm_bound_us": round(C * n * nbytes / HBM * 1e6, 3),
                     "cycles_per_sample_and_chain": round(kus * 1e-6 * CLOCK / n, 2)})
    print(json.dumps({"bench": "sidechain", "channels": C, "samples": n, "calls": a.calls, "rows": rows}))


if __name__ == "__main__":
    main()
