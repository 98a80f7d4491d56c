"""Timing of mi_dynproc_bank (not a test, not bench.py), after bench_expander.py: 1024 channels x 4096 samples, in one session
    process with and without env, process_apply, curve alone,
    process with no spline enabled (the gain is expf(0)) -- the follower with its loads and stores,
    process with one reaction range against five in both tables (no spline) -- the cost of the look-up as the tables fill
    (the kernel runs the same padded cascade either way: a difference would be data, not code),
    and mi_compressor_bank's process in the same session: the yardstick (the same chain without the look-up).
Figures as tests/bench_expander.py takes them (kernel time from events, median of 20; us per call over a warmed-up window;
every figure `--repeats` times, median, smallest and largest), with the ratio of every kernel time to the compressor's.  One
JSON line.
Usage: python tests/bench_dynproc.py [--channels C] [--samples S] [--calls K] [--warmup W] [--repeats R]"""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


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
        raise SystemExit("bench_dynproc: no HIP device (there is no CPU fallback)")
    import compressor_ref as cr
    import dynproc_ref as dr
    from bench_expander import measure
    C, n = a.channels, a.samples
    x = dr.sweep(1, C, n)
    din, daudio = mi.DeviceBuffer.from_host(x), mi.DeviceBuffer.from_host(x[::-1].copy())
    dgain, denv = mi.DeviceBuffer((C, n)), mi.DeviceBuffer((C, n))

    def bank(splines=True, ranges=None):
        b = mi.DynamicProcessorBank(C)
        for ch in range(C):
            s = dr.channel_settings(ch)
            if not splines:
                s.update(dots=[])
            if ranges is not None:
                lv = [0.01, 0.04, 0.16, 0.5][:ranges - 1]
                s.update(attack_levels=lv, release_levels=lv)
            b.configure(ch, **s)
        b.update_settings()
        return b

    comp = mi.CompressorBank(C)
    for ch in range(C):
        comp.configure(ch, **cr.channel_settings(ch))
    comp.update_settings()
    full, bare, one, five = bank(), bank(splines=False), bank(False, 1), bank(False, 5)
    cases = [("process", lambda: full.process(dgain, denv, din, n)),
             ("process_no_env", lambda: full.process(dgain, None, din, n)),
             ("process_apply", lambda: full.process_apply(dgain, daudio, din, n)),
             ("curve", lambda: full.curve(dgain, din, n)),
             ("process_no_env_no_spline", lambda: bare.process(dgain, None, din, n)),
             ("process_no_env_no_spline_1_range", lambda: one.process(dgain, None, din, n)),
             ("process_no_env_no_spline_5_ranges", lambda: five.process(dgain, None, din, n)),
             ("compressor_process", lambda: comp.process(dgain, denv, din, n)),
             ("compressor_process_no_env", lambda: comp.process(dgain, None, din, n))]
    rows = measure(mi, cases, n, a.calls, a.warmup, max(a.repeats, 5))
    yard = {r["case"]: r["kernel_us"] for r in rows}["compressor_process"]
    for r in rows:
        r["kernel_over_compressor_process"] = round(r["kernel_us"] / yard, 3)
    print(json.dumps({"bench": "dynproc", "channels": C, "samples": n, "calls": a.calls, "repeats": max(a.repeats, 5), "rows": rows}))


if __name__ == "__main__":
    main()
