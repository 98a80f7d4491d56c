"""Timing of mi_oscillator_bank (not a test, not bench.py): 1024 channels x 4096 samples in one session
    overwrite with a rectangular wave (no arithmetic to speak of), a sawtooth, a sine, a squared sine,
    add and mul of a sawtooth with a source,
    4 channels x 1 Mi samples of a sawtooth and of a sine (the case the split along time exists for),
    1024 x 65536 of a rectangular wave, a sawtooth and a sine beside a copy of that size,
    a band-limited sawtooth at 2x, 4x and 8x beside OversamplerBank.downsample alone on rows of the same size,
    and a device-to-device hipMemcpyAsync of one [channels][samples] float array as the yardstick.
Per row: device events around a warmed-up window of back-to-back calls (us per call), around single calls (median of nine after a
warm-up), and for the plain functions the synthesis kernel's own time (mi_dspu_profile_next_launch).  Models at 8 TB/s: overwrite
4 B per sample, add and mul 8 B, BL 4 N B for the synthesis plus the downsample's (4 N read, 4 N written and 4 N read by the
filter and the decimation, 4 written).  One JSON line.
Usage: python tests/bench_oscillator.py [--channels C] [--samples S] [--calls K] [--warmup W]"""
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
FN = {"sine": 0, "squared_sine": 2, "rectangular": 4, "sawtooth": 5, "bl_sawtooth": 10}
SET_FUNCTION, SET_FREQUENCY, SET_SAMPLE_RATE, SET_WIDTH, SET_OVER_MODE = 0, 1, 2, 9, 15
MODES = {2: 1, 4: 15, 8: 29}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=1024)
    ap.add_argument("--samples", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    mi = importlib.import_module("lsp-dsp-units_amd")
    if mi.device_count() <= 0:
        raise SystemExit("bench_oscillator: no HIP device (there is no CPU fallback)")
    lib, C, n = mi.lib, a.channels, a.samples
    rng = np.random.default_rng(1)
    ev0, ev1 = ctypes.c_void_p(), ctypes.c_void_p()
    mi.check(lib.mi_dspu_event_create(ctypes.byref(ev0)))
    mi.check(lib.mi_dspu_event_create(ctypes.byref(ev1)))
    ms = ctypes.c_float()

    def bank_of(channels, fn, mode=0):
        b = mi.OscillatorBank(channels)
        for ch in range(channels):
            b.set(ch, SET_SAMPLE_RATE, 48000)
            b.set(ch, SET_FREQUENCY, 100.0 + 0.37 * ch)
            b.set(ch, SET_WIDTH, 0.5)
            b.set(ch, SET_OVER_MODE, mode)
            b.set(ch, SET_FUNCTION, FN[fn])
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

    def measure(name, call, samples, model_bytes, armed, by):
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
        row = {"case": name, "us_per_call": round(window, 3), "call_us": round(float(np.median(single)), 3),
               "kernel_us": None if kernel is None else round(float(np.median(kernel)), 3),
               "min_max_us": [round(min(kernel or single), 3), round(max(kernel or single), 3)],
               "model_us": round(samples * model_bytes / HBM * 1e6, 3), "multiple_of_model": round(best / (samples * model_bytes / HBM * 1e6), 2)}
        if "copy_d2d" in by:
            row["multiple_of_copy"] = round(best / by["copy_d2d"]["call_us"] * (C * n) / samples, 3)    # per sample
        by[name] = row
        return row

    rows, by, keep = [], {}, []
    x = mi.DeviceBuffer.from_host((rng.standard_normal((C, n)) * 0.5).astype(f32))
    out = mi.DeviceBuffer((C, n))
    rows.append(measure("copy_d2d", lambda: mi.check(lib.mi_dspu_copy_d2d(ctypes.c_void_p(out.ptr), ctypes.c_void_p(x.ptr), C * n * 4, None)),
                        C * n, 8, False, by))
    for fn in ("rectangular", "sawtooth", "sine", "squared_sine"):
        b = bank_of(C, fn)
        keep.append(b)
        rows.append(measure("overwrite_" + fn, lambda b=b: b.process(out, n), C * n, 4, True, by))
    b = bank_of(C, "sawtooth")
    keep.append(b)
    rows.append(measure("add_sawtooth", lambda: b.process(out, n, src=x, op=1), C * n, 8, True, by))
    rows.append(measure("mul_sawtooth", lambda: b.process(out, n, src=x, op=2), C * n, 8, True, by))
    long_n = 1 << 20
    long_out = mi.DeviceBuffer((4, long_n))
    for fn in ("sawtooth", "sine"):
        b4 = bank_of(4, fn)
        keep.append(b4)
        rows.append(measure("overwrite_%s_4x1Mi" % fn, lambda b4=b4: b4.process(long_out, long_n), 4 * long_n, 4, True, by))
    # ... and rows sixteen times as long, where the launch's fill and drain no longer dominate
    big_n = 16 * n
    big_x, big_out = mi.DeviceBuffer((C, big_n)), mi.DeviceBuffer((C, big_n))
    big_x.zero()
    rows.append(measure("copy_d2d_x16", lambda: mi.check(lib.mi_dspu_copy_d2d(ctypes.c_void_p(big_out.ptr), ctypes.c_void_p(big_x.ptr), C * big_n * 4, None)),
                        C * big_n, 8, False, by))
    for fn in ("rectangular", "sawtooth", "sine"):
        b = bank_of(C, fn)
        keep.append(b)
        rows.append(measure("overwrite_%s_x16" % fn, lambda b=b: b.process(big_out, big_n), C * big_n, 4, True, by))
    big_x.free()
    big_out.free()
    for times, mode in sorted(MODES.items()):
        bl = bank_of(C, "bl_sawtooth", mode)
        bl.reserve(n)
        keep.append(bl)
        r = measure("bl_sawtooth_%dx" % times, lambda bl=bl: bl.process(out, n), C * n, 4 * times + 12 * times + 4, False, by)
        over = mi.OversamplerBank(C)
        over.set_sample_rate(48000)
        over.set_mode(mode)
        over.update_settings()
        keep.append(over)
        rows_ptr, stride = bl.synth_rows()
        d = measure("downsample_alone_%dx" % times, lambda over=over, rows_ptr=rows_ptr, stride=stride: over.downsample(out, rows_ptr, n, in_stride=stride),
                    C * n, 12 * times + 4, False, by)
        r["synth_share_of_call"] = round(1.0 - d["call_us"] / r["call_us"], 3)
        rows += [r, d]
    print(json.dumps({"bench": "oscillator", "channels": C, "samples": n, "calls": a.calls, "rows": rows}))


if __name__ == "__main__":
    main()
