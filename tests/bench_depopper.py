"""Timing of mi_depopper_bank (not a test, not bench.py): 1024 channels x 4096 samples at 48 kHz, in one session
    a device-to-device copy of one plane, the panometer's period-40 row (the same shape of chain: two dependent roundings per
    sample and a refreshed sum) and the surge protector's process (the same kind of automaton),
    and the depopper with a fade-in and a fade-out of 5 ms: steady closed (silence), steady open (noise), bursts (the level comes
    and goes every 300 samples: one event per 600 samples and channel) at an RMS length of 1 ms, and open and bursts at 10 ms.
Device events around a warmed-up window of calls (us per call) and around single launches (the kernel's own time,
mi_dspu_profile_next_launch, median of 20); one JSON line.  Every depopper row carries its kernel time as a multiple of the
panometer row's and of the copy's window time, and cycles per sample and chain at 2.4 GHz.
Usage: python tests/bench_depopper.py [--channels C] [--samples S] [--calls K] [--warmup W]"""
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

HBM = 8.0e12
CLOCK = 2.4e9
SR = 48000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=1024)
    ap.add_argument("--samples", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    mi = importlib.import_module("lsp-dsp-units_amd")
    if mi.device_count() <= 0:
        raise SystemExit("bench_depopper: no HIP device (there is no CPU fallback)")
    lib, C, n = mi.lib, a.channels, a.samples
    rng = np.random.default_rng(1)
    noise = (rng.standard_normal((C, n)) * 0.25).astype(np.float32)
    other = (0.6 * noise + 0.8 * rng.standard_normal((C, n)) * 0.25).astype(np.float32)
    gate = ((np.arange(n)[None, :] // 300 + np.arange(C)[:, None]) % 2 == 0)
    silence, bursts = np.zeros((C, n), np.float32), np.where(gate, noise, 0.0).astype(np.float32)
    level = np.where(gate, 0.9, 0.05).astype(np.float32)
    dev = {k: mi.DeviceBuffer.from_host(v) for k, v in (("noise", noise), ("other", other), ("silence", silence), ("bursts", bursts), ("level", level))}
    denv, dgain = mi.DeviceBuffer((C, n)), mi.DeviceBuffer((C, n))
    ev0, ev1 = ctypes.c_void_p(), ctypes.c_void_p()
    mi.check(lib.mi_dspu_event_create(ctypes.byref(ev0)))
    mi.check(lib.mi_dspu_event_create(ctypes.byref(ev1)))

    pano = mi.PanometerBank(C, 2400)
    surge = mi.SurgeProtectorBank(C)
    for ch in range(C):
        pano.configure(ch, 40, law=0)
        surge.configure(ch, 257, 300, 0.5, 0.25)
    pano.update_settings()
    surge.process(None, None, 0)

    def depopper(rms_ms):
        b = mi.DepopperBank(C)
        for ch in range(C):
            b.init(ch, SR, 10.0, 10.0)
            b.set_fade_in_time(ch, 5.0)
            b.set_fade_out_time(ch, 5.0)
            b.set_fade_in_threshold(ch, 0.1)
            b.set_fade_out_threshold(ch, 0.05)
            b.set_rms_length(ch, rms_ms)
        b.update_settings()
        return b

    d1, d10 = depopper(1.0), depopper(10.0)
    copy = lambda: mi.check(lib.mi_dspu_copy_d2d(ctypes.c_void_p(dgain.ptr), ctypes.c_void_p(dev["noise"].ptr), C * n * 4, None))  # noqa: E731
    cases = [("copy_d2d", 8, False, copy),
             ("panometer_linear_n40", 20.0 + 8.0 * 40 / 256, True, lambda: pano.process(dgain, dev["noise"], dev["other"], n)),
             ("surge_process", 8, True, lambda: surge.process(dgain, dev["level"], n)),
             ("depopper_closed_rms_1ms", 12, True, lambda: d1.process(denv, dgain, dev["silence"], n)),
             ("depopper_open_rms_1ms", 12, True, lambda: d1.process(denv, dgain, dev["noise"], n)),
             ("depopper_bursts_rms_1ms", 12, True, lambda: d1.process(denv, dgain, dev["bursts"], n)),
             ("depopper_bursts_rms_1ms_no_env", 8, True, lambda: d1.process(None, dgain, dev["bursts"], n)),
             ("depopper_open_rms_10ms", 12, True, lambda: d10.process(denv, dgain, dev["noise"], n)),
             ("depopper_bursts_rms_10ms", 12, True, lambda: d10.process(denv, dgain, dev["bursts"], n))]
    rows = []
    ms = ctypes.c_float()
    for name, nbytes, is_kernel, call in cases:
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
        kus = us
        if is_kernel:
            kernel = []
            for _ in range(20):
                mi.check(lib.mi_dspu_profile_next_launch(ev0, ev1))
                call()
                mi.check(lib.mi_dspu_event_synchronize(ev1))
                mi.check(lib.mi_dspu_event_elapsed_ms(ctypes.byref(ms), ev0, ev1))
                kernel.append(ms.value * 1e3)
            kus = float(np.median(kernel))
        rows.append({"case": name, "us_per_call": round(us, 3), "kernel_us": round(kus, 3), "kernel": mi.last_launch() if is_kernel else "copy",
                     "msamples_per_s": round(C * n / us, 1), "bytes_per_sample": round(nbytes, 2),
                     "hbm_bound_us": round(C * n * nbytes / HBM * 1e6, 3),
                     "cycles_per_sample_and_chain": round(kus * 1e-6 * CLOCK / n, 2),
                     "ratio_to_copy": round(kus / rows[0]["us_per_call"], 3) if rows else 1.0,
                     "ratio_to_panometer": round(kus / rows[1]["kernel_us"], 3) if len(rows) > 1 else None})
    print(json.dumps({"bench": "depopper", "channels": C, "samples": n, "calls": a.calls, "rows": rows}))


if __name__ == "__main__":
    main()
