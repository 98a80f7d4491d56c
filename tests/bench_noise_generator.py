"""Timing of mi_noise_generator_bank (not a test, not bench.py): 1024 channels x 4096 samples per call, colour filter of order 50
(25 sections), in one session
    the LCG bank's own uniform overwrite, and mi_biquad_bank_process of 25 sections on the same shape (the parts a pink call is made of),
    the generator's white overwrite (must cost the LCG bank's call), pink overwrite (against the sum of the two parts) and pink add
    with a source (two more passes: the scratch rows and the combine launch), each with the colour filter in the fast and in the
    exact mode,
    and a device-to-device hipMemcpyAsync of one [channels][samples] float array as the yardstick.
Per row: device events around a warmed-up window of back-to-back calls (us per call; the window is stretched until it lasts
--window-ms) and around single calls (median of nine after a warm-up).  The measuring process is a child of this script and runs
under a timeout; the parent never opens the device.  One JSON line.
Usage: python tests/bench_noise_generator.py [--channels C] [--samples S] [--warmup W] [--window-ms T] [--timeout SECONDS]"""
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

f32 = np.float32
OVERWRITE, ADD = 0, 1
ORDER = 50
SEED = 0x9E3779B9


def measure_all(a):
    mi = importlib.import_module("lsp-dsp-units_amd")
    if mi.device_count() <= 0:
        raise SystemExit("bench_noise_generator: no HIP device (there is no CPU fallback)")
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

    def measure(name, call, by):
        for _ in range(a.warmup):
            call()
        calls, window = 20, 0.0
        while True:                                             # a window that lasts: not the clock and the scheduler
            window = events_around(lambda: [call() for _ in range(calls)])
            if window >= a.window_ms * 1e3 or calls >= 20000:
                break
            calls *= 4
        single = [events_around(call) for _ in range(12)][3:]
        row = {"case": name, "calls": calls, "us_per_call": round(window / calls, 3), "call_us": round(float(np.median(single)), 3),
               "min_max_us": [round(min(single), 3), round(max(single), 3)]}
        by[name] = row
        return row

    def generator(color, exact):
        b = mi.NoiseGeneratorBank(C)
        b.set_exact(exact)
        for ch in range(C):
            b.init(ch, 23, 0x55 + ch, SEED * (ch + 1), SEED * (ch + 3), 23, 0x77 + ch)
            b.set_sample_rate(ch, 48000)
            b.set_generator(ch, b.GEN_LCG)
            b.set_noise_color(ch, color)
            b.set_coloring_order(ch, ORDER)
            b.set_amplitude(ch, 0.5)
        b.reserve(n)
        b.update_settings()
        return b

    rows, by, keep = [], {}, []
    x = mi.DeviceBuffer.from_host((rng.standard_normal((C, n)) * 0.5).astype(f32))
    out = mi.DeviceBuffer((C, n))
    copy = lambda: mi.check(lib.mi_dspu_copy_d2d(ctypes.c_void_p(out.ptr), ctypes.c_void_p(x.ptr), C * n * 4, None))
    rows.append(measure("copy_d2d", copy, by))
    lcg = mi.LCGBank(C)
    for ch in range(C):
        lcg.init(ch, SEED * (ch + 1))
        lcg.set_amplitude(ch, 0.5)
    rows.append(measure("lcg_overwrite_uniform", lambda: lcg.process(out, n), by))
    # the sections of a pink tilt of this order, on a biquad bank of its own
    tilt = mi.SpectralTiltBank(1)
    tilt.set_sample_rate(0, 48000)
    tilt.set_order(0, ORDER)
    tilt.set_slope(0, -0.5, tilt.NEPER_PER_NEPER)
    tilt.set_lower_frequency(0, 10.0)
    tilt.set_upper_frequency(0, 0.9 * 0.5 * 48000)
    tilt.update_settings()
    coef = tilt.get_chains(0)
    tilt.close()
    for exact in (False, True):
        mode = "exact" if exact else "fast"
        bq = mi.BiquadBank(C, coef.shape[0])
        keep.append(bq)
        bq.set_exact(exact)
        bq.set_all_chains(np.broadcast_to(coef, (C,) + coef.shape).copy())
        rows.append(measure("biquad_%d_sections_%s" % (coef.shape[0], mode), lambda bq=bq: bq.process(out, x, n), by))
        white, pink = generator(0, exact), generator(1, exact)
        keep += [white, pink]
        rows.append(measure("generator_white_overwrite_" + mode, lambda b=white: b.process(out, n), by))
        rows.append(measure("generator_pink_overwrite_" + mode, lambda b=pink: b.process(out, n), by))
        rows.append(measure("generator_pink_add_" + mode, lambda b=pink: b.process(out, n, src=x, op=ADD), by))
        parts = by["lcg_overwrite_uniform"]["us_per_call"] + by["biquad_%d_sections_%s" % (coef.shape[0], mode)]["us_per_call"]
        by["generator_white_overwrite_" + mode]["window_multiple_of_lcg"] = round(by["generator_white_overwrite_" + mode]["us_per_call"] / by["lcg_overwrite_uniform"]["us_per_call"], 3)
        by["generator_pink_overwrite_" + mode]["window_multiple_of_parts"] = round(by["generator_pink_overwrite_" + mode]["us_per_call"] / parts, 3)
        by["generator_pink_add_" + mode]["window_multiple_of_parts"] = round(by["generator_pink_add_" + mode]["us_per_call"] / parts, 3)
    rows.append(measure("copy_d2d_again", copy, by))
    rows.append(measure("lcg_overwrite_uniform_again", lambda: lcg.process(out, n), by))
    sources = {f: mi.source_sha(f) for f in ("noise_generator.hip", "spectral_tilt.hip", "noise.hip", "velvet.hip", "biquad.hip")}
    print(json.dumps({"bench": "noise_generator", "channels": C, "samples": n, "order": ORDER, "window_ms": a.window_ms, "sources": sources, "rows": rows}))


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
        raise SystemExit("bench_noise_generator: the measuring process did not finish in %g s and was ended" % a.timeout)


if __name__ == "__main__":
    main()
