"""Timing of mi_gate_bank (not a test, not bench.py), after bench_compressor.py: 1024 channels x 4096 samples, in one session
    process with and without env, process_apply and curve on the burst signal (every channel toggles dozens of times),
    process on a signal that never toggles -- the difference is what the second steps cost, and next to the compressor what
    the crossing test, the branch and the bit words cost,
    process with a flat curve (both zones at 1: no logf / expf) -- the follower alone,
    and mi_compressor_bank's process in the same session: the yardstick.
Figures as tests/bench_expander.py takes them (kernel time from events, median of 20; us per call over a warmed-up window;
each `--repeats` times with smallest and largest).  One JSON line.
Usage: python tests/bench_gate.py [--channels C] [--samples S] [--calls K] [--warmup W] [--repeats R]"""
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
        raise SystemExit("bench_gate: no HIP device (there is no CPU fallback)")
    import compressor_ref as cr
    import gate_ref as gr
    from bench_expander import measure
    C, n = a.channels, a.samples
    xb, xq = gr.bursts(1, C, n), gr.quiet(2, C, n)
    dburst, dquiet, daudio = mi.DeviceBuffer.from_host(xb), mi.DeviceBuffer.from_host(xq), mi.DeviceBuffer.from_host(xb[::-1].copy())
    dgain, denv = mi.DeviceBuffer((C, n)), mi.DeviceBuffer((C, n))

    def bank(flat=False):
        b = mi.GateBank(C)
        for ch in range(C):
            s = gr.channel_settings(ch)
            if flat:
                s.update(open_zone=1.0, close_zone=1.0)
            b.configure(ch, **s)
        b.update_settings()
        return b

    comp = mi.CompressorBank(C)
    for ch in range(C):
        comp.configure(ch, **cr.channel_settings(ch))
    comp.update_settings()
    full, flat = bank(), bank(True)
    cases = [("process_bursts", lambda: full.process(dgain, denv, dburst, n)),
             ("process_no_env_bursts", lambda: full.process(dgain, None, dburst, n)),
             ("process_never_toggles", lambda: full.process(dgain, denv, dquiet, n)),
             ("process_apply_bursts", lambda: full.process_apply(dgain, daudio, dburst, n)),
             ("curve", lambda: full.curve(dgain, dburst, n)),
             ("process_no_env_flat_curve_bursts", lambda: flat.process(dgain, None, dburst, n)),
             ("compressor_process_bursts", lambda: comp.process(dgain, denv, dburst, n))]
    rows = measure(mi, cases, n, a.calls, a.warmup, max(a.repeats, 5))
    print(json.dumps({"bench": "gate", "channels": C, "samples": n, "calls": a.calls, "repeats": max(a.repeats, 5), "rows": rows}))


if __name__ == "__main__":
    main()
