"""Timing of mi_metergraph_bank (not a test, not bench.py): in one session, for 1024 channels x 4096 samples,
    process with MM_ABS_MAXIMUM at the periods 2400 (20 frames per second at 48 kHz), 64 and 1,
    process with each of the five methods at period 2400, and with gains at period 2400,
    read of 333 frames,
    a device-to-device hipMemcpyAsync of one [channels][samples] float array as the yardstick,
    and the PeakMeter bank's process without dst (the other read-only pass over such rows), timed the same way.
Per row: device events around a warmed-up window of back-to-back calls (us per call), around single calls (median of nine after a
warm-up), and the kernel's own time (mi_dspu_profile_next_launch).  The traffic model is 4 B per sample at 8 TB/s (the copy moves
8); read moves 4 B per frame.  One JSON line.
Usage: python tests/bench_metergraph.py [--calls K] [--warmup W]"""
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
f32 = np.float32
METHODS = ("abs_maximum", "abs_minimum", "sign_maximum", "sign_minimum", "peak")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    mi = importlib.import_module("lsp-dsp-units_amd")
    if mi.device_count() <= 0:
        raise SystemExit("bench_metergraph: no HIP device (there is no CPU fallback)")
    lib = mi.lib
    rng = np.random.default_rng(1)
    ev0, ev1 = ctypes.c_void_p(), ctypes.c_void_p()
    mi.check(lib.mi_dspu_event_create(ctypes.byref(ev0)))
    mi.check(lib.mi_dspu_event_create(ctypes.byref(ev1)))
    ms = ctypes.c_float()

    def events_around(call):
        mi.check(lib.mi_dspu_stream_synchronize(None))
        mi.check(lib.mi_dspu_event_record(ev0, None))
        call()
        mi.check(lib.mi_dspu_event_record(ev1, None))
        mi.check(lib.mi_dspu_event_synchronize(ev1))
        mi.check(lib.mi_dspu_event_elapsed_ms(ctypes.byref(ms), ev0, ev1))
        return ms.value * 1e3

    def measure(name, call, model_bytes, armed, copy):
        for _ in range(a.warmup):
            call()
        window = events_around(lambda: [call() for _ in range(a.calls)]) / a.calls
        single = [events_around(call) for _ in range(12)][3:]
        kernel = None
        if armed:
            kernel = []
            for i in range(12):
                mi.check(lib.mi_dspu_profile_next_launch(ev0, ev1))
                call()
                mi.check(lib.mi_dspu_event_synchronize(ev1))
                mi.check(lib.mi_dspu_event_elapsed_ms(ctypes.byref(ms), ev0, ev1))
                kernel.append(ms.value * 1e3)
            kernel = kernel[3:]
        best = float(np.median(kernel if kernel else single))
        model = model_bytes / HBM * 1e6
        row = {"case": name, "us_per_call": round(window, 3), "call_us": round(float(np.median(single)), 3),
               "kernel_us": None if kernel is None else round(float(np.median(kernel)), 3),
               "min_max_us": [round(min(kernel or single), 3), round(max(kernel or single), 3)],
               "model_us": round(model, 3), "multiple_of_model": round(best / model, 2), "TB_per_s": round(model_bytes / best * 1e-6, 3)}
        if copy is not None:
            row["kernel_over_copy_call"] = round(best / copy["call_us"], 3)
            row["window_over_copy_window"] = round(window / copy["us_per_call"], 3)
        return row

    C, n, frames = 1024, 4096, 333
    x = mi.DeviceBuffer.from_host((rng.standard_normal((C, n)) * 0.5).astype(f32))
    out = mi.DeviceBuffer((C, n))
    out.zero()
    gains = mi.DeviceBuffer.from_host(np.full(C, 0.5, f32))
    rows, keep = [], []
    copy = measure("copy_d2d", lambda: mi.check(lib.mi_dspu_copy_d2d(ctypes.c_void_p(out.ptr), ctypes.c_void_p(x.ptr), C * n * 4, None)),
                   C * n * 8, False, None)
    rows.append(copy)
    pm = mi.PeakMeterBank(C)
    for ch in range(C):
        pm.configure(ch, 48000, 5.0, 300.0)
    pm.update_settings()
    keep.append(pm)
    rows.append(measure("peakmeter_process_no_dst", lambda: pm.process(None, x, n), C * n * 4, True, copy))

    def bank_of(method, period):
        b = mi.MeterGraphBank(C, frames)
        for ch in range(C):
            b.init(ch, frames, period, 0.0)
            b.set_method(ch, method)
        b.update_settings()
        keep.append(b)
        return b

    for period in (2400, 64, 1):
        b = bank_of(0, period)
        rows.append(measure("process_abs_maximum_period_%d" % period, lambda b=b: b.process(x, n), C * n * 4, True, copy))
    for m, name in enumerate(METHODS[1:], 1):
        b = bank_of(m, 2400)
        rows.append(measure("process_%s_period_2400" % name, lambda b=b: b.process(x, n), C * n * 4, True, copy))
    b = bank_of(0, 2400)
    rows.append(measure("process_gains_abs_maximum_period_2400", lambda: b.process(x, n, gains=gains), C * n * 4, True, copy))
    rows.append(measure("read_333_frames", lambda: b.read(out, frames), C * frames * 8, True, None))
    for buf in (x, out, gains):
        buf.free()
    print(json.dumps({"bench": "metergraph", "channels": C, "samples": n, "calls": a.calls, "rows": rows}))


if __name__ == "__main__":
    main()
