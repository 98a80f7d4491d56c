"""Timing of mi_dyndelay_bank (not a test, not bench.py): 1024 channels x 4096 samples, lines for 1000 samples (staged in LDS) and for
48000 (worked on in global memory), in one session
    fdelay == delay (the plain echo), fdelay == 0, fdelay == 7 (every run is cut after 7 steps: lane 0 walks them all),
    a sine-modulated chorus, uniform random rows,
    the echo at a delay 64 above a multiple of 2048 (the tag arrays' size: tails and feeds share slots, runs are cut short),
    and beside them a device-to-device hipMemcpyAsync of one [channels][samples] float array and the delay bank's process.
Device events around a warmed-up window of calls (us per call) and around single launches (the kernel's own time,
mi_dspu_profile_next_launch, median after a warm-up; around the one call for the copy and the delay bank, which take no armed
events).  Every row carries the share of its steps that ran one per lane, from the kernel's debug counters in a call of its own
(the timed calls do not count), its multiple of the same-session copy and of the all-serial row of the same line.  One JSON line.
Usage: python tests/bench_dyndelay.py [--channels C] [--samples S] [--calls K] [--warmup W]"""
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


def rows_of(kind, max_size, C, n, rng):
    near = float(max_size - 100)
    t = np.arange(n)[None, :] + 37 * np.arange(C)[:, None]
    if kind == "echo":
        return np.full((C, n), near, f32), np.full((C, n), near, f32)
    if kind == "fdelay_0":
        return np.full((C, n), near, f32), np.zeros((C, n), f32)
    if kind == "fdelay_7":
        return np.full((C, n), near, f32), np.full((C, n), 7, f32)
    if kind == "chorus":
        return (near / 2 + near / 2.1 * np.sin(t / 83.0)).astype(f32), (near / 4 + near / 4.3 * np.sin(t / 47.0 + 1.0)).astype(f32)
    if kind == "random":
        return rng.uniform(0, max_size, (C, n)).astype(f32), rng.uniform(0, max_size, (C, n)).astype(f32)
    if kind == "echo_shared_slots":
        d = float((max_size // 2048) * 2048 + 64 - (2048 if (max_size // 2048) * 2048 + 64 > max_size else 0))     # 47168 of 48000
        return np.full((C, n), d, f32), np.full((C, n), d, f32)
    raise ValueError(kind)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=1024)
    ap.add_argument("--samples", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    mi = importlib.import_module("lsp-dsp-units_amd")
    if mi.device_count() <= 0:
        raise SystemExit("bench_dyndelay: no HIP device (there is no CPU fallback)")
    lib, C, n = mi.lib, a.channels, a.samples
    rng = np.random.default_rng(1)
    x = mi.DeviceBuffer.from_host((rng.standard_normal((C, n)) * 0.5).astype(f32))
    g = mi.DeviceBuffer.from_host(rng.uniform(-0.9, 0.9, (C, n)).astype(f32))
    out = mi.DeviceBuffer((C, n))
    ev0, ev1 = ctypes.c_void_p(), ctypes.c_void_p()
    mi.check(lib.mi_dspu_event_create(ctypes.byref(ev0)))
    mi.check(lib.mi_dspu_event_create(ctypes.byref(ev1)))
    delay = mi.DelayBank(C, 1024)
    delay.set_delay(257)

    copy = lambda: mi.check(lib.mi_dspu_copy_d2d(ctypes.c_void_p(out.ptr), ctypes.c_void_p(x.ptr), C * n * 4, None))  # noqa: E731
    cases = [("copy_d2d", None, None, copy), ("delay_process", None, None, lambda: delay.process(out, x, n))]
    keep = []
    for max_size in (1000, 48000):
        for kind in ("echo", "fdelay_0", "fdelay_7", "chorus", "random") + (("echo_shared_slots",) if max_size > 4096 else ()):
            bank = mi.DynamicDelayBank(C, max_size)
            d, fd = [mi.DeviceBuffer.from_host(r) for r in rows_of(kind, max_size, C, n, rng)]
            keep.append((bank, d, fd))
            cases.append(("%s_%d" % (kind, max_size), bank, max_size,
                          lambda bank=bank, d=d, fd=fd: bank.process(out, x, d, g, fd, n)))
    rows, by = [], {}
    ms = ctypes.c_float()
    for name, bank, max_size, call in cases:
        share = None
        if bank is not None:
            bank.count_steps(True)
            call()
            side, total = bank.steps()
            bank.count_steps(False)
            share = side / total
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
        for i in range(12):
            if bank is None:
                mi.check(lib.mi_dspu_stream_synchronize(None))
                mi.check(lib.mi_dspu_event_record(ev0, None))
                call()
                mi.check(lib.mi_dspu_event_record(ev1, None))
            else:
                mi.check(lib.mi_dspu_profile_next_launch(ev0, ev1))
                call()
            mi.check(lib.mi_dspu_event_synchronize(ev1))
            mi.check(lib.mi_dspu_event_elapsed_ms(ctypes.byref(ms), ev0, ev1))
            if i >= 3:
                kernel.append(ms.value * 1e3)
        kus = float(np.median(kernel))
        nbytes = 8 if bank is None else 20
        serial = by.get("fdelay_7_%s" % max_size)
        row = {"case": name, "us_per_call": round(us, 3), "kernel_us": round(kus, 3), "kernel_us_min_max": [round(min(kernel), 3), round(max(kernel), 3)],
               "kernel": {"copy_d2d": "hipMemcpyAsync", "delay_process": "mi_delay_bank_process"}.get(name) or mi.last_launch(),
               "parallel_share": None if share is None else round(share, 4), "bytes_per_sample": nbytes,
               "hbm_bound_us": round(C * n * nbytes / HBM * 1e6, 3),
               "multiple_of_copy": round(kus / by["copy_d2d"]["kernel_us"], 3) if by else 1.0,
               "ns_per_step_of_a_channel": None if bank is None else round(kus * 1e3 / n, 2),
               "multiple_of_all_serial": None if serial is None else round(kus / serial["kernel_us"], 4)}
        rows.append(row)
        by[name] = row
    for name in by:                                             # the rows in front of their line's all-serial row
        tail = name.rsplit("_", 1)[-1]
        if by[name]["multiple_of_all_serial"] is None and "fdelay_7_" + tail in by and name not in ("copy_d2d", "delay_process"):
            by[name]["multiple_of_all_serial"] = round(by[name]["kernel_us"] / by["fdelay_7_" + tail]["kernel_us"], 4)
    print(json.dumps({"bench": "dyndelay", "channels": C, "samples": n, "calls": a.calls, "rows": rows}))


if __name__ == "__main__":
    main()
