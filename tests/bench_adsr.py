"""Timing of mi_adsr_bank (not a test, not bench.py): in one session, for 1024 channels x 4096 samples and for 4 channels x 1 Mi samples
    process, process_mul, generate, generate_mul in place and generate_mul with a source, each with NONE, CUBIC and EXP curves in
    all four segments (hold and break on),
    a device-to-device hipMemcpyAsync of one [channels][samples] float array as the yardstick,
    and the Oscillator bank's rectangular row (a generator with no arithmetic to speak of), timed the same way.
Per row: device events around a warmed-up window of back-to-back calls (us per call: for generate* that includes the small launches
that carry start and step), around single calls (median of nine after a warm-up), and the kernel's own time
(mi_dspu_profile_next_launch).  Models at 8 TB/s: process 8 B per sample, process_mul 12, generate 4, generate_mul 8 and 8.
One JSON line.
Usage: python tests/bench_adsr.py [--calls K] [--warmup W]"""
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
FN = {"none": 0, "cubic": 3, "exp": 5}
OPS = (("process", 8), ("process_mul", 12), ("generate", 4), ("generate_mul", 8), ("generate_mul_src", 8))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    mi = importlib.import_module("lsp-dsp-units_amd")
    if mi.device_count() <= 0:
        raise SystemExit("bench_adsr: no HIP device (there is no CPU fallback)")
    lib = mi.lib
    rng = np.random.default_rng(1)
    ev0, ev1 = ctypes.c_void_p(), ctypes.c_void_p()
    mi.check(lib.mi_dspu_event_create(ctypes.byref(ev0)))
    mi.check(lib.mi_dspu_event_create(ctypes.byref(ev1)))
    ms = ctypes.c_float()

    def bank_of(channels, fn):
        b = mi.ADSREnvelopeBank(channels)
        for ch in range(channels):
            j = 0.0001 * (ch % 100)
            b.set_attack(ch, 0.1 + j, 0.3, FN[fn])
            b.set_hold(ch, 0.2 + j, 1)
            b.set_decay(ch, 0.4 + j, 0.3, FN[fn])
            b.set_break(ch, 0.5, 1)
            b.set_slope(ch, 0.6 + j, 0.7, FN[fn])
            b.set_release(ch, 0.8 + j, 0.7, FN[fn])
            b.set_sustain_level(ch, 0.3)
        b.update_settings()
        return b

    def events_around(call):
        mi.check(lib.mi_dspu_stream_synchronize(None))
        mi.check(lib.mi_dspu_event_record(ev0, None))
        call()
        mi.check(lib.mi_dspu_event_record(ev1, None))
        mi.check(lib.mi_dspu_event_synchronize(ev1))
        mi.check(lib.mi_dspu_event_elapsed_ms(ctypes.byref(ms), ev0, ev1))
        return ms.value * 1e3

    def measure(name, call, samples, model_bytes, armed, copy):
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
        model = samples * model_bytes / HBM * 1e6
        row = {"case": name, "us_per_call": round(window, 3), "call_us": round(float(np.median(single)), 3),
               "kernel_us": None if kernel is None else round(float(np.median(kernel)), 3),
               "min_max_us": [round(min(kernel or single), 3), round(max(kernel or single), 3)],
               "model_us": round(model, 3), "multiple_of_model": round(best / model, 2),
               "TB_per_s": round(samples * model_bytes / best * 1e-6, 3)}
        if copy is not None:
            row["kernel_over_copy_call"] = round(best / copy["call_us"], 3)
            row["window_over_copy_window"] = round(window / copy["us_per_call"], 3)
        return row

    rows, keep = [], []
    for C, n, tag in ((1024, 4096, "1024x4096"), (4, 1 << 20, "4x1Mi")):
        t = mi.DeviceBuffer.from_host(rng.uniform(-0.05, 1.05, (C, n)).astype(f32))
        x = mi.DeviceBuffer.from_host((rng.standard_normal((C, n)) * 0.5).astype(f32))
        out = mi.DeviceBuffer((C, n))
        out.zero()
        start = np.full(C, -0.02, f32)
        step = np.full(C, 1.04 / n, f32)
        copy = measure("copy_d2d_" + tag, lambda: mi.check(lib.mi_dspu_copy_d2d(ctypes.c_void_p(out.ptr), ctypes.c_void_p(x.ptr), C * n * 4, None)),
                       C * n, 8, False, None)
        rows.append(copy)
        osc = mi.OscillatorBank(C)
        for ch in range(C):
            osc.set(ch, 2, 48000), osc.set(ch, 1, 100.0 + 0.37 * ch), osc.set(ch, 0, 4)       # sample rate, frequency, rectangular
        osc.update_settings()
        keep.append(osc)
        rows.append(measure("oscillator_rectangular_" + tag, lambda: osc.process(out, n), C * n, 4, True, copy))
        for fn in FN:
            b = bank_of(C, fn)
            keep.append(b)
            calls = {"process": lambda b=b: b.process(out, t, n), "process_mul": lambda b=b: b.process_mul(out, t, n),
                     "generate": lambda b=b: b.generate(out, start, step, n), "generate_mul": lambda b=b: b.generate_mul(out, start, step, n),
                     "generate_mul_src": lambda b=b: b.generate_mul(out, start, step, n, src=x)}
            for op, model_bytes in OPS:
                rows.append(measure("%s_%s_%s" % (op, fn, tag), calls[op], C * n, model_bytes, True, copy))
        for buf in (t, x, out):
            buf.free()
    print(json.dumps({"bench": "adsr", "calls": a.calls, "rows": rows}))


if __name__ == "__main__":
    main()
