"""Timing of mi_bypass_bank and mi_crossfade_bank (not a test, not bench.py): 1024 channels x 4096 samples, in one session
    the bypass steady off (process, process_wet: the wet row copied or scaled) and steady on (the dry row copied),
    every channel ramping over 240 samples, and over the whole block (a ramp of 5000 samples),
    the crossfade steady and fading over 240 samples,
    and beside them a device-to-device hipMemcpyAsync of one [channels][samples] float array and the delay bank's process.
Device events around a warmed-up window of calls (us per call; steady rows only: a ramp has to be set up again before every
call) and around single launches (the kernel's own time, mi_dspu_profile_next_launch, median of 20 after a warm-up; around the one
call for the copy and the delay bank, which take no armed events: that figure holds the launch's overhead too); one JSON line.  The steady rows carry their multiple of the same-session copy (the model: 8 bytes per sample, as the copy), the ramp
rows their extra time over the steady row of the same entry.
Usage: python tests/bench_bypass_crossfade.py [--channels C] [--samples S] [--calls K] [--warmup W]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=1024)
    ap.add_argument("--samples", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    mi = importlib.import_module("lsp-dsp-units_amd")
    if mi.device_count() <= 0:
        raise SystemExit("bench_bypass_crossfade: no HIP device (there is no CPU fallback)")
    lib, C, n = mi.lib, a.channels, a.samples
    rng = np.random.default_rng(1)
    dry = mi.DeviceBuffer.from_host((rng.standard_normal((C, n)) * 0.5).astype(np.float32))
    wet = mi.DeviceBuffer.from_host((rng.standard_normal((C, n)) * 0.5).astype(np.float32))
    out = mi.DeviceBuffer((C, n))
    ev0, ev1 = ctypes.c_void_p(), ctypes.c_void_p()
    mi.check(lib.mi_dspu_event_create(ctypes.byref(ev0)))
    mi.check(lib.mi_dspu_event_create(ctypes.byref(ev1)))

    off, on, ramp, xf = mi.BypassBank(C), mi.BypassBank(C), mi.BypassBank(C), mi.CrossfadeBank(C)
    delay = mi.DelayBank(C, 1024)
    delay.set_delay(257)
    for bank in (off, on, ramp, xf):
        bank.init(bank.ALL, 48000, 0.005)
    on.set_bypass(on.ALL, True)
    on.process(out, dry, wet, n)                                # the ramp down runs out here: steady on from now
    direction = [False]

    def turn_round():                                           # every channel starts a ramp of 240 samples, down and up in turn
        direction[0] = not direction[0]
        ramp.set_bypass(ramp.ALL, direction[0])
        ramp.process(None, None, None, 0)                       # what was recorded goes out before the timed launch

    def whole_block():                                          # ... or one of 5000 samples, down from 1
        ramp.init(ramp.ALL, 5000, 1.0)
        ramp.set_bypass(ramp.ALL, True)
        ramp.process(None, None, None, 0)

    def fade():
        xf.toggle(xf.ALL)
        xf.process(None, None, None, 0)

    copy = lambda: mi.check(lib.mi_dspu_copy_d2d(ctypes.c_void_p(out.ptr), ctypes.c_void_p(wet.ptr), C * n * 4, None))  # noqa: E731
    # (name, bytes per sample, what sets a ramp up before a call, the call, the steady row a ramp row is held against)
    cases = [("copy_d2d", 8, None, copy, None),
             ("delay_process", 8, None, lambda: delay.process(out, wet, n), None),
             ("bypass_off_process", 8, None, lambda: off.process(out, dry, wet, n), None),
             ("bypass_off_process_wet", 8, None, lambda: off.process_wet(out, dry, wet, 0.75, n), None),
             ("bypass_on_process", 8, None, lambda: on.process(out, dry, wet, n), None),
             ("bypass_ramp_240", 8, turn_round, lambda: ramp.process(out, dry, wet, n), "bypass_off_process"),
             ("bypass_ramp_whole_block", 12, whole_block, lambda: ramp.process(out, dry, wet, n), "bypass_off_process"),
             ("crossfade_steady", 8, None, lambda: xf.process(out, dry, wet, n), None),
             ("crossfade_fade_240", 8, fade, lambda: xf.process(out, dry, wet, n), "crossfade_steady")]
    rows, by = [], {}
    ms = ctypes.c_float()
    for name, nbytes, arm, call, against in cases:
        us = None
        if arm is None:
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
        for i in range(25):
            if arm is not None:
                arm()
            if name in ("copy_d2d", "delay_process"):           # no launch that takes the armed events: events around the one call
                mi.check(lib.mi_dspu_stream_synchronize(None))
                mi.check(lib.mi_dspu_event_record(ev0, None))
                call()
                mi.check(lib.mi_dspu_event_record(ev1, None))
            else:
                mi.check(lib.mi_dspu_profile_next_launch(ev0, ev1))
                call()
            mi.check(lib.mi_dspu_event_synchronize(ev1))
            mi.check(lib.mi_dspu_event_elapsed_ms(ctypes.byref(ms), ev0, ev1))
            if i >= 5:                                          # the first five warm up
                kernel.append(ms.value * 1e3)
        kus = float(np.median(kernel))
        row = {"case": name, "us_per_call": None if us is None else round(us, 3), "kernel_us": round(kus, 3),
               "kernel_us_min_max": [round(min(kernel), 3), round(max(kernel), 3)],
               "kernel": {"copy_d2d": "hipMemcpyAsync", "delay_process": "mi_delay_bank_process"}.get(name) or mi.last_launch(), "bytes_per_sample": nbytes,
               "hbm_bound_us": round(C * n * nbytes / HBM * 1e6, 3),
               "multiple_of_copy": round(kus / by["copy_d2d"]["kernel_us"], 3) if by else 1.0,
               "window_multiple_of_copy": round(us / by["copy_d2d"]["us_per_call"], 3) if by and us is not None else (1.0 if not by else None),
               "extra_over_steady_us": round(kus - by[against]["kernel_us"], 3) if against else None}
        rows.append(row)
        by[name] = row
    print(json.dumps({"bench": "bypass_crossfade", "channels": C, "samples": n, "calls": a.calls, "rows": rows}))


if __name__ == "__main__":
    main()
