"""Timing of mi_velvet_bank (not a test, not bench.py): 1024 channels x 4096 samples per call, in one session
    OVN, OVNA and ARN at W = 10 with the LCG core and with the MLS core, TRN plain and crushed: overwrite, and add with a source,
    the LCG bank's uniform call (overwrite and add) on the same rows,
    and a device-to-device hipMemcpyAsync of one [channels][samples] float array as the yardstick.
Per row: device events around a warmed-up window of back-to-back calls (us per call; the window is stretched until it lasts
--window-ms) and around single calls (median of nine after a warm-up), both as multiples of the copy and of LCG uniform in the same
run.  The floor of a velvet call is the serial generator chain, as for LCG: `draws` is the number of draws a channel consumes per call
(counted by the numpy restatement for channel 0; it depends on the draws), and draws / 4 dependent steps of one generator bound it.
The measuring process is a child of this script and runs under a timeout; the parent never opens the device.  One JSON line.
Usage: python tests/bench_velvet.py [--channels C] [--samples S] [--warmup W] [--window-ms T] [--timeout SECONDS]"""
import argparse
import ctypes
import importlib
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CLOCK = 2.4e9
f32 = np.float32
OVERWRITE, ADD = 0, 1
CASES = (("ovn_lcg", 0, 1, False), ("ovn_mls", 0, 0, False), ("ovna_lcg", 1, 1, False), ("ovna_mls", 1, 0, False), ("arn_lcg", 2, 1, False),
         ("arn_mls", 2, 0, False), ("trn", 3, 1, False), ("trn_crushed", 3, 1, True))
SEED = 0x9E3779B9


def draws_of(type_, core, crush, n, segment):
    """Draws that channel 0 consumes in a call of n samples cut into segments of `segment`: the restatement counts them."""
    import velvet_ref as V
    u = V.Velvet()
    u.init(SEED, 23, 0x55)
    u.type, u.core, u.crush = type_, core, crush
    for at in range(0, n, segment):
        u.segment(min(segment, n - at))
    return len(u.drawn)


def measure_all(a):
    mi = importlib.import_module("lsp-dsp-units_amd")
    if mi.device_count() <= 0:
        raise SystemExit("bench_velvet: no HIP device (there is no CPU fallback)")
    lib, C, n = mi.lib, a.channels, a.samples
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

    def measure(name, call, by, draws=None):
        for _ in range(a.warmup):
            call()
        calls, window = 20, 0.0
        while True:                                             # a window that lasts: not the clock and the scheduler
            window = events_around(lambda: [call() for _ in range(calls)])
            if window >= a.window_ms * 1e3 or calls >= 20000:
                break
            calls *= 4
        single = [events_around(call) for _ in range(12)][3:]
        best = float(np.median(single))
        row = {"case": name, "calls": calls, "us_per_call": round(window / calls, 3), "call_us": round(best, 3),
               "min_max_us": [round(min(single), 3), round(max(single), 3)]}
        for ref in ("copy_d2d", "lcg_overwrite_uniform"):
            if ref in by:
                row["window_multiple_of_" + ref.split("_")[0]] = round(row["us_per_call"] / by[ref]["us_per_call"], 3)
        if draws:
            row["draws"] = draws
            row["window_cycles_per_chain_step"] = round(row["us_per_call"] * 1e-6 * CLOCK / (draws / 4), 2)
        by[name] = row
        return row

    rows, by, keep = [], {}, []
    x = mi.DeviceBuffer.from_host((rng.standard_normal((C, n)) * 0.5).astype(f32))
    out = mi.DeviceBuffer((C, n))
    rows.append(measure("copy_d2d", lambda: mi.check(lib.mi_dspu_copy_d2d(ctypes.c_void_p(out.ptr), ctypes.c_void_p(x.ptr), C * n * 4, None)), by))
    lcg = mi.LCGBank(C)
    for ch in range(C):
        lcg.init(ch, SEED * (ch + 1))
        lcg.set_amplitude(ch, 0.5)
    rows.append(measure("lcg_overwrite_uniform", lambda: lcg.process(out, n), by, draws=n))
    rows.append(measure("lcg_add_uniform", lambda: lcg.process(out, n, src=x, op=ADD), by, draws=n))
    for name, type_, core, crush in CASES:
        b = mi.VelvetBank(C)
        keep.append(b)
        for ch in range(C):
            b.init(ch, SEED * (ch + 1), 23, 0x55 + ch)
            b.set_velvet_type(ch, type_)
            b.set_core_type(ch, core)
            b.set_crush(ch, crush)
            b.set_velvet_window_width(ch, 10.0)
            b.set_amplitude(ch, 0.5)
        rows.append(measure("velvet_overwrite_" + name, lambda b=b: b.process(out, n), by, draws=draws_of(type_, core, crush, n, n)))
        rows.append(measure("velvet_add_" + name, lambda b=b: b.process(out, n, src=x, op=ADD), by, draws=draws_of(type_, core, crush, n, 256)))
    rows.append(measure("copy_d2d_again", lambda: mi.check(lib.mi_dspu_copy_d2d(ctypes.c_void_p(out.ptr), ctypes.c_void_p(x.ptr), C * n * 4, None)), by))
    rows.append(measure("lcg_overwrite_uniform_again", lambda: lcg.process(out, n), by, draws=n))
    sources = {f: mi.source_sha(f) for f in ("velvet.hip", "noise.hip", "randomizer_device.h", "mls_device.h")}    # what the loaded library was built from
    print(json.dumps({"bench": "velvet", "channels": C, "samples": n, "window_ms": a.window_ms, "clock_hz": CLOCK, "sources": sources, "rows": rows}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=1024)
    ap.add_argument("--samples", type=int, default=4096)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=200.0)
    ap.add_argument("--timeout", type=float, default=240.0)
    ap.add_argument("--measure", action="store_true", help="this process measures (the child)")
    a = ap.parse_args()
    if a.measure:
        return measure_all(a)
    child = [sys.executable, os.path.abspath(__file__), "--measure"] + [v for v in sys.argv[1:]]
    try:
        sys.exit(subprocess.run(child, timeout=a.timeout).returncode)
    except subprocess.TimeoutExpired:
        raise SystemExit("bench_velvet: the measuring process did not finish in %g s and was ended" % a.timeout)


if __name__ == "__main__":
    main()
