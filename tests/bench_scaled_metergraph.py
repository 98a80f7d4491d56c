"""Timing of mi_scaled_metergraph_bank (not a test, not bench.py): in one session, for 1024 channels x 4096 samples, a subsampling of
32, 333 frames and a longest period of 2400,
    process with MM_ABS_MAXIMUM and no period change at the periods 2400 (20 frames per second at 48 kHz) and 64,
    process with a period change in every channel (2400 <-> 64 before every call: the call re-decimates and skips the frames sampler),
    process with gains at period 2400,
    read of 333 frames,
    a device-to-device hipMemcpyAsync of one [channels][samples] float array as the yardstick,
    and MeterGraphBank.process at the same periods, timed the same way.
Per row: device events around a warmed-up window of back-to-back calls (us per call; for the period-change row that includes the
1024 set_period() calls and the upload of the table, which is host work), around single calls (median of nine after a warm-up),
and the kernel's own time (mi_dspu_profile_next_launch).  The traffic model is 4 B per sample at 8 TB/s (the copy moves 8): the
row comes from HBM once, its second pass is served by the cache; read moves 4 B per frame.  One JSON line.
Usage: python tests/bench_scaled_metergraph.py [--calls K] [--warmup W]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    mi = importlib.import_module("lsp-dsp-units_amd")
    if mi.device_count() <= 0:
        raise SystemExit("bench_scaled_metergraph: no HIP device (there is no CPU fallback)")
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

    def measure(name, call, model_bytes, armed, copy, before=None):
        """`before`: host work ahead of every call (the setters); the armed launch is the first one behind it."""
        def whole():
            if before is not None:
                before()
            call()
        for _ in range(a.warmup):
            whole()
        window = events_around(lambda: [whole() for _ in range(a.calls)]) / a.calls
        single = [events_around(whole) for _ in range(12)][3:]
        kernel = None
        if armed:
            kernel = []
            for i in range(12):
                if before is not None:
                    before()
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

    C, n, frames, sub, longest = 1024, 4096, 333, 32, 2400
    subframes = (frames * longest + sub - 1) // sub
    x = mi.DeviceBuffer.from_host((rng.standard_normal((C, n)) * 0.5).astype(f32))
    out = mi.DeviceBuffer((C, n))
    out.zero()
    gains = mi.DeviceBuffer.from_host(np.full(C, 0.5, f32))
    rows, keep = [], []
    copy = measure("copy_d2d", lambda: mi.check(lib.mi_dspu_copy_d2d(ctypes.c_void_p(out.ptr), ctypes.c_void_p(x.ptr), C * n * 4, None)),
                   C * n * 8, False, None)
    rows.append(copy)

    def plain_bank(period):
        b = mi.MeterGraphBank(C, frames)
        for ch in range(C):
            b.init(ch, frames, period, 0.0)
        b.update_settings()
        keep.append(b)
        return b

    def scaled_bank(period):
        b = mi.ScaledMeterGraphBank(C, frames, subframes)
        for ch in range(C):
            b.init(ch, frames, sub, longest)
            b.set_period(ch, period)
        b.update_settings()
        b.process(x, n)                                             # the first call takes the period over
        keep.append(b)
        return b

    by = {}
    for period in (2400, 64):
        b = plain_bank(period)
        by["plain", period] = measure("metergraph_process_period_%d" % period, lambda b=b: b.process(x, n), C * n * 4, True, copy)
        rows.append(by["plain", period])
    for period in (2400, 64):
        b = scaled_bank(period)
        by["scaled", period] = measure("process_no_change_period_%d" % period, lambda b=b: b.process(x, n), C * n * 4, True, copy)
        by["scaled", period]["kernel_over_metergraph_kernel"] = round(by["scaled", period]["kernel_us"] / by["plain", period]["kernel_us"], 3)
        rows.append(by["scaled", period])
    b = scaled_bank(2400)
    turn = [0]

    def other_period():
        turn[0] ^= 1
        for ch in range(C):
            b.set_period(ch, 64 if turn[0] else 2400)
        b.update_settings()

    rows.append(measure("process_period_change_every_channel", lambda: b.process(x, n), C * n * 4, True, copy, before=other_period))
    b = scaled_bank(2400)
    rows.append(measure("process_gains_period_2400", lambda: b.process(x, n, gains=gains), C * n * 4, True, copy))
    rows.append(measure("read_333_frames", lambda: b.read(out, frames), C * frames * 8, True, None))
    for buf in (x, out, gains):
        buf.free()
    print(json.dumps({"bench": "scaled_metergraph", "channels": C, "samples": n, "subsampling": sub, "frames": frames, "calls": a.calls, "rows": rows}))


if __name__ == "__main__":
    main()
