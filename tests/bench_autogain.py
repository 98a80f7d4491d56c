"""Timing of mi_autogain_bank and mi_simple_autogain_bank (not a test, not bench.py), after bench_limiter.py: 1024 channels x
4096 samples, in one session
    process           the signal of tests/autogain_ref.py (surges, a deep drop, silence, slow drifts), all four combinations of
                      quick amplifier x max-gain limiting across channels
    silence           lshort below the silence threshold everywhere: the chain's short way (apply_gain_limiting alone)
    process_level     the same signal with one expected level per channel from device memory (two rows in LDS instead of three)
    process_apply     ... with the multiply by the audio in the same launch
    simple_process    SimpleAutoGain on levels around its threshold
    and mi_compressor_bank's process in the same session: the yardstick.
Figures as tests/bench_expander.py takes them (kernel time from events, median of 20; us per call over a warmed-up window;
cycles per sample and chain = kernel time x clock / samples).  No pass / fail threshold.  One JSON line.
Usage: python tests/bench_autogain.py [--channels C] [--samples S] [--calls K] [--warmup W] [--repeats R]"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=1024)
    ap.add_argument("--samples", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    mi = importlib.import_module("lsp-dsp-units_amd")
    if mi.device_count() <= 0:
        raise SystemExit("bench_autogain: no HIP device (there is no CPU fallback)")
    import autogain_ref as ar
    import compressor_ref as cr
    import limiter_ref as lr
    from bench_expander import measure
    C, n = a.channels, a.samples
    lengths, left = [], n
    while left > 0:
        for k in ar.LENGTHS:
            lengths.append(min(k, left))
            left -= lengths[-1]
    ll, ls, le = ar.signal(1, C, lengths=tuple(k for k in lengths if k > 0))
    rng = np.random.default_rng(2)
    dl, ds, de = (mi.DeviceBuffer.from_host(x) for x in (ll, ls, le))
    dquiet = mi.DeviceBuffer.from_host(np.full((C, n), 1e-5, np.float32))
    dlevels = mi.DeviceBuffer.from_host(le[:, 0])
    daudio = mi.DeviceBuffer.from_host(rng.standard_normal((C, n)).astype(np.float32))
    dsimple = mi.DeviceBuffer.from_host(ar.simple_signal(3, C, n))
    dsc = mi.DeviceBuffer.from_host(lr.bursts(2, C, n, every=1500))
    dout, denv = mi.DeviceBuffer((C, n)), mi.DeviceBuffer((C, n))

    def bank():
        b = mi.AutoGainBank(C)
        for ch in range(C):
            quick, limit = ar.switches(ch)
            b.configure(ch, quick_amp=quick, limit=limit, **ar.settings_of(ch))
        b.update_settings()
        return b

    simple = mi.SimpleAutoGainBank(C)
    for ch in range(C):
        simple.set_sample_rate(ch, 1000)
        simple.set_speed(ch, 100.0 + ch % 5, 120.0 - ch % 7)
        simple.set_threshold(ch, 0.1)
        simple.set_gain(ch, 0.25, 4.0)
    simple.update_settings()
    comp = mi.CompressorBank(C)
    for ch in range(C):
        comp.configure(ch, **cr.channel_settings(ch))
    comp.update_settings()
    plain, quiet, level, apply_ = bank(), bank(), bank(), bank()
    cases = [("process", lambda: plain.process(dout, dl, ds, de, n)),
             ("silence", lambda: quiet.process(dout, dl, dquiet, de, n)),
             ("process_level", lambda: level.process_level(dout, dl, ds, dlevels, n)),
             ("process_apply", lambda: apply_.process_apply(dout, daudio, dl, ds, de, n)),
             ("simple_process", lambda: simple.process(dout, dsimple, n)),
             ("compressor_process_bursts", lambda: comp.process(dout, denv, dsc, n))]
    rows = measure(mi, cases, n, a.calls, a.warmup, max(a.repeats, 5))
    yard = rows[-1]["cycles_per_sample_and_chain"]
    for row in rows:
        row["against_compressor"] = round(row["cycles_per_sample_and_chain"] / yard, 2)
    states = [plain.get_state(ch) for ch in range(0, C, max(C // 16, 1))]
    print(json.dumps({"bench": "autogain", "channels": C, "samples": n, "calls": a.calls, "repeats": max(a.repeats, 5), "rows": rows,
                      "gains_finite_after": bool(np.all(np.isfinite([s[0] for s in states])))}))


if __name__ == "__main__":
    main()
