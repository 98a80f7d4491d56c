"""Timing of mi_qcounter_bank (not a test, not bench.py): in one session, at 1024 channels x 4096 samples and at 4 channels x 1 Mi
samples, with a period of 48000 and 256 levels of [-1, 1) unless the row's name says otherwise,
    process of uniform random rows, of a sine, of a constant row (every lane of every wave in one bin) and of the constant row with
    the wave-level combining compiled out,
    process with 16, 4096 and 8191 levels (the last on the global-atomic path: 8193 words do not fit the LDS budget),
    process with a pending recount of the full window (a range change before every call),
    read of the 258 counters of every channel,
    a device-to-device hipMemcpyAsync of one [channels][samples] float array as the yardstick,
    and MeterGraphBank.process at period 2400 (a read-only pass over such rows), timed the same way.
Per row: device events around a warmed-up window of back-to-back calls (us per call), around single calls (median of nine after a
warm-up), and the kernel's own time (mi_dspu_profile_next_launch).  The traffic model is 12 B per sample while count <= nPeriod (the
row in, the ring out, the evicted samples back in) and 8 B per sample above nPeriod, at 8 TB/s; the copy moves 8.  One JSON line.
Usage: python tests/bench_quantized_counter.py [--calls K] [--warmup W]"""
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
PERIOD = 48000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    mi = importlib.import_module("lsp-dsp-units_amd")
    if mi.device_count() <= 0:
        raise SystemExit("bench_quantized_counter: no HIP device (there is no CPU fallback)")
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

    def measure(name, call, model_bytes, armed, copy, calls, prepare=None):
        """prepare: host work before every call that is not timed; such a row has the kernel's own time only"""
        if prepare is not None:
            return kernel_only(name, call, model_bytes, prepare)
        for _ in range(a.warmup):
            call()
        window = events_around(lambda: [call() for _ in range(calls)]) / calls
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

    def kernel_only(name, call, model_bytes, prepare):
        kernel = []
        for i in range(12):
            prepare()
            mi.check(lib.mi_dspu_stream_synchronize(None))
            mi.check(lib.mi_dspu_profile_next_launch(ev0, ev1))
            call()
            mi.check(lib.mi_dspu_event_synchronize(ev1))
            mi.check(lib.mi_dspu_event_elapsed_ms(ctypes.byref(ms), ev0, ev1))
            kernel.append(ms.value * 1e3)
        kernel = kernel[3:]
        best, model = float(np.median(kernel)), model_bytes / HBM * 1e6
        return {"case": name, "us_per_call": None, "call_us": None, "kernel_us": round(best, 3), "min_max_us": [round(min(kernel), 3), round(max(kernel), 3)],
                "model_us": round(model, 3), "multiple_of_model": round(best / model, 2), "TB_per_s": round(model_bytes / best * 1e-6, 3)}

    shapes = []
    for C, n in ((1024, 4096), (4, 1 << 20)):
        calls = a.calls if n <= 4096 else max(4, a.calls // 4)
        per_sample = 12 if n <= PERIOD else 8
        t = np.arange(n, dtype=np.float64)
        signals = {"uniform": rng.uniform(-1.1, 1.1, (C, n)).astype(f32),
                   "sine": np.broadcast_to((0.9 * np.sin(2 * np.pi * 441.0 / 48000.0 * t)).astype(f32), (C, n)),
                   "constant": np.full((C, n), 0.3, f32)}
        bufs = {k: mi.DeviceBuffer.from_host(v) for k, v in signals.items()}
        out = mi.DeviceBuffer((C, n))
        out.zero()
        rows, keep = [], []
        copy = measure("copy_d2d", lambda: mi.check(lib.mi_dspu_copy_d2d(ctypes.c_void_p(out.ptr), ctypes.c_void_p(bufs["uniform"].ptr), C * n * 4, None)),
                       C * n * 8, False, None, calls)
        rows.append(copy)
        mg = mi.MeterGraphBank(C, 333)
        for ch in range(C):
            mg.init(ch, 333, 2400, 0.0)
        mg.update_settings()
        keep.append(mg)
        rows.append(measure("metergraph_process_period_2400", lambda: mg.process(bufs["uniform"], n), C * n * 4, True, copy, calls))

        def bank_of(levels, signal):
            b = mi.QuantizedCounterBank(C, PERIOD, levels)
            for ch in range(C):
                b.set_range(ch, -1.0, 1.0, levels)
                b.set_period(ch, PERIOD)
            for _ in range((PERIOD + n - 1) // n + 1):                 # the window is full: every call evicts as much as it counts
                b.process(bufs[signal], n)
            keep.append(b)
            return b

        for signal in ("uniform", "sine", "constant"):
            b = bank_of(256, signal)
            rows.append(measure("process_%s" % signal, lambda b=b, s=signal: b.process(bufs[s], n), C * n * per_sample, True, copy, calls))
        b = bank_of(256, "constant")
        b.set_wave_combining(False)
        rows.append(measure("process_constant_no_wave_combining", lambda: b.process(bufs["constant"], n), C * n * per_sample, True, copy, calls))
        for levels in (16, 4096, 8191):
            b = bank_of(levels, "uniform")
            name = "process_uniform_levels_%d%s" % (levels, "_global_atomics" if levels + 2 > 8192 else "")
            rows.append(measure(name, lambda b=b: b.process(bufs["uniform"], n), C * n * per_sample, True, copy, calls))
        b = bank_of(256, "uniform")
        flip = [0]

        def change_range():
            flip[0] ^= 1
            for ch in range(C):
                b.set_value_range(ch, -1.0, 1.0 + 0.25 * flip[0])
            b.read(out, 258)                                            # sends the table; recounts nothing

        # the history that remains is read and counted anew, then the row in and the ring out
        rows.append(measure("process_uniform_pending_recount", lambda: b.process(bufs["uniform"], n), C * (max(PERIOD - n, 0) * 4 + n * 8), True, None,
                            calls, prepare=change_range))
        rows.append(measure("read_258_counters", lambda: b.read(out, 258), C * 258 * 8, True, None, calls))
        for buf in list(bufs.values()) + [out]:
            buf.free()
        shapes.append({"channels": C, "samples": n, "calls": calls, "rows": rows})
    print(json.dumps({"bench": "quantized_counter", "period": PERIOD, "levels": 256, "shapes": shapes}))


if __name__ == "__main__":
    main()
