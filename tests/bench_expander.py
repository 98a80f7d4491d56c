"""Timing of mi_expander_bank (not a test, not bench.py), after bench_compressor.py: 1024 channels x 4096 samples, in one session
    process with and without env, process_apply, curve alone,
    process with a flat curve (downward, the threshold above every envelope's knee end: no logf / expf) -- the follower alone,
    and mi_compressor_bank's process in the same session: the yardstick (the same chain, one knee more).
Device events around single launches (the kernel's own time, median of 20) and around a warmed-up window of calls (us per
call); every figure is taken `--repeats` times and reported as median, smallest and largest, so that a difference can be held
against the spread.  One JSON line.
Usage: python tests/bench_expander.py [--channels C] [--samples S] [--calls K] [--warmup W] [--repeats R]"""
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

CLOCK = 2.4e9


def measure(mi, cases, n, calls, warmup, repeats):
    """cases: (name, call) -> rows of kernel time (median of 20 launches) and us per call, each `repeats` times."""
    lib = mi.lib
    ev0, ev1 = ctypes.c_void_p(), ctypes.c_void_p()
    mi.check(lib.mi_dspu_event_create(ctypes.byref(ev0)))
    mi.check(lib.mi_dspu_event_create(ctypes.byref(ev1)))
    ms = ctypes.c_float()
    rows = []
    for name, call in cases:
        for _ in range(warmup):
            call()
        per_call, kernel = [], []
        for _ in range(repeats):
            mi.check(lib.mi_dspu_stream_synchronize(None))
            mi.check(lib.mi_dspu_event_record(ev0, None))
            for _ in range(calls):
                call()
            mi.check(lib.mi_dspu_event_record(ev1, None))
            mi.check(lib.mi_dspu_event_synchronize(ev1))
            mi.check(lib.mi_dspu_event_elapsed_ms(ctypes.byref(ms), ev0, ev1))
            per_call.append(ms.value * 1e3 / calls)
            one = []
            for _ in range(20):
                mi.check(lib.mi_dspu_profile_next_launch(ev0, ev1))
                call()
                mi.check(lib.mi_dspu_event_synchronize(ev1))
                mi.check(lib.mi_dspu_event_elapsed_ms(ctypes.byref(ms), ev0, ev1))
                one.append(ms.value * 1e3)
            kernel.append(float(np.median(one)))
        kus = float(np.median(kernel))
        rows.append({"case": name, "kernel": mi.last_launch(), "kernel_us": round(kus, 3),
                     "kernel_us_min_max": [round(min(kernel), 3), round(max(kernel), 3)],
                     "us_per_call": round(float(np.median(per_call)), 3),
                     "us_per_call_min_max": [round(min(per_call), 3), round(max(per_call), 3)],
                     "cycles_per_sample_and_chain": round(kus * 1e-6 * CLOCK / n, 2)})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=1024)
    ap.add_argument("--samples", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    mi = importlib.import_module("lsp-dsp-units_amd")
    if mi.device_count() <= 0:
        raise SystemExit("bench_expander: no HIP device (there is no CPU fallback)")
    import compressor_ref as cr
    import expander_ref as er
    C, n = a.channels, a.samples
    x = er.sidechain(1, C, n)
    din, daudio = mi.DeviceBuffer.from_host(x), mi.DeviceBuffer.from_host(x[::-1].copy())
    dgain, denv = mi.DeviceBuffer((C, n)), mi.DeviceBuffer((C, n))

    def bank(flat=False):
        b = mi.ExpanderBank(C)
        for ch in range(C):
            s = er.channel_settings(ch)
            if flat:
                s.update(mode=er.EM_DOWNWARD, attack_threshold=1e-6, knee=1.0, ratio=1.0)
            b.configure(ch, **s)
        b.update_settings()
        return b

    comp = mi.CompressorBank(C)
    for ch in range(C):
        comp.configure(ch, **cr.channel_settings(ch))
    comp.update_settings()
    full, flat = bank(), bank(True)
    cases = [("process", lambda: full.process(dgain, denv, din, n)),
             ("process_no_env", lambda: full.process(dgain, None, din, n)),
             ("process_apply", lambda: full.process_apply(dgain, daudio, din, n)),
             ("curve", lambda: full.curve(dgain, din, n)),
             ("process_no_env_flat_curve", lambda: flat.process(dgain, None, din, n)),
             ("compressor_process", lambda: comp.process(dgain, denv, din, n)),
             ("compressor_process_no_env", lambda: comp.process(dgain, None, din, n))]
    rows = measure(mi, cases, n, a.calls, a.warmup, max(a.repeats, 5))
    print(json.dumps({"bench": "expander", "channels": C, "samples": n, "calls": a.calls, "repeats": max(a.repeats, 5), "rows": rows}))


if __name__ == "__main__":
    main()
