"""Timing of mi_lcg_bank and mi_mls_bank (not a test, not bench.py): 1024 channels x 4096 samples in one session
    overwrite for each LCG distribution, and for MLS at register widths 23 and 64,
    add with a source for LCG uniform and for MLS,
    4 channels x 1 Mi samples for both,
    and a device-to-device hipMemcpyAsync of one [channels][samples] float array as the yardstick.
Per row: device events around a warmed-up window of back-to-back calls (us per call) and around single calls (median of nine after a
warm-up).  MLS writes 4 B per sample from tables that stay in cache: its bound is the copy, and the row says how many copies it
takes per sample, a call against a call and the window against the window.  The floor of LCG is not memory but the serial chain: draws / 4 dependent steps of two 32-bit multiplies, a shift
and two adds per generator; the row says how many cycles (at 2.4 GHz) a call takes per step of one chain.  The 4 x 1 Mi row of LCG
is the latency of ONE chain from end to end: a Randomizer cannot be split along time.  One JSON line.
Usage: python tests/bench_noise.py [--channels C] [--samples S] [--calls K] [--warmup W]"""
import argparse
import ctypes
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CLOCK = 2.4e9
f32 = np.float32
DISTRIBUTIONS = ("uniform", "exponential", "triangular", "gaussian")
DRAWS = (1, 2, 1, 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=1024)
    ap.add_argument("--samples", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    mi = importlib.import_module("lsp-dsp-units_amd")
    if mi.device_count() <= 0:
        raise SystemExit("bench_noise: no HIP device (there is no CPU fallback)")
    lib, C, n = mi.lib, a.channels, a.samples
    rng = np.random.default_rng(1)
    ev0, ev1 = ctypes.c_void_p(), ctypes.c_void_p()
    mi.check(lib.mi_dspu_event_create(ctypes.byref(ev0)))
    mi.check(lib.mi_dspu_event_create(ctypes.byref(ev1)))
    ms = ctypes.c_float()

    def lcg_of(channels, dist):
        b = mi.LCGBank(channels)
        for ch in range(channels):
            b.init(ch, 0x9E3779B9 * (ch + 1))
            b.set_distribution(ch, dist)
            b.set_amplitude(ch, 0.5)
        return b

    def mls_of(channels, bits):
        b = mi.MLSBank(channels)
        for ch in range(channels):
            b.set_n_bits(ch, bits)
            b.set_state(ch, 0x9E3779B97F4A7C15 * (ch + 1))
            b.set_amplitude(ch, 0.5)
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

    def measure(name, call, samples, by, calls=a.calls, chain_steps=None):
        for _ in range(a.warmup):
            call()
        window = events_around(lambda: [call() for _ in range(calls)]) / calls
        single = [events_around(call) for _ in range(12)][3:]
        best = float(np.median(single))
        row = {"case": name, "us_per_call": round(window, 3), "call_us": round(best, 3), "min_max_us": [round(min(single), 3), round(max(single), 3)]}
        if "copy_d2d" in by:                                    # per sample; call against call, window against window
            row["call_multiple_of_copy"] = round(best / by["copy_d2d"]["call_us"] * (C * n) / samples, 3)
            row["window_multiple_of_copy"] = round(window / by["copy_d2d"]["us_per_call"] * (C * n) / samples, 3)
        if chain_steps:
            row["chain_steps"] = chain_steps
            row["call_cycles_per_chain_step"] = round(best * 1e-6 * CLOCK / chain_steps, 2)
            row["window_cycles_per_chain_step"] = round(window * 1e-6 * CLOCK / chain_steps, 2)
        by[name] = row
        return row

    rows, by, keep = [], {}, []
    x = mi.DeviceBuffer.from_host((rng.standard_normal((C, n)) * 0.5).astype(f32))
    out = mi.DeviceBuffer((C, n))
    rows.append(measure("copy_d2d", lambda: mi.check(lib.mi_dspu_copy_d2d(ctypes.c_void_p(out.ptr), ctypes.c_void_p(x.ptr), C * n * 4, None)), C * n, by))
    for dist, name in enumerate(DISTRIBUTIONS):
        b = lcg_of(C, dist)
        keep.append(b)
        rows.append(measure("lcg_overwrite_" + name, lambda b=b: b.process(out, n), C * n, by, chain_steps=DRAWS[dist] * n // 4))
    b = lcg_of(C, 0)
    keep.append(b)
    rows.append(measure("lcg_add_uniform", lambda: b.process(out, n, src=x, op=1), C * n, by, chain_steps=n // 4))
    for bits in (23, 64):
        m = mls_of(C, bits)
        keep.append(m)
        rows.append(measure("mls_overwrite_%d_bits" % bits, lambda m=m: m.process(out, n), C * n, by))
    m = mls_of(C, 23)
    keep.append(m)
    rows.append(measure("mls_add_23_bits", lambda: m.process(out, n, src=x, op=1), C * n, by))
    long_n = 1 << 20
    long_out = mi.DeviceBuffer((4, long_n))
    m4 = mls_of(4, 23)
    rows.append(measure("mls_overwrite_23_bits_4x1Mi", lambda: m4.process(long_out, long_n), 4 * long_n, by))
    for dist in (0, 3):
        b4 = lcg_of(4, dist)
        keep.append(b4)
        rows.append(measure("lcg_overwrite_%s_4x1Mi" % DISTRIBUTIONS[dist], lambda b4=b4: b4.process(long_out, long_n), 4 * long_n, by, calls=4,
                            chain_steps=DRAWS[dist] * long_n // 4))
    sources = {f: mi.source_sha(f) for f in ("noise.hip", "randomizer_device.h", "mls_device.h")}    # what the loaded library was built from
    print(json.dumps({"bench": "noise", "channels": C, "samples": n, "calls": a.calls, "clock_hz": CLOCK, "sources": sources, "rows": rows}))


if __name__ == "__main__":
    main()
