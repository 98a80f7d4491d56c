"""bench.py's launcher contract, checked without a GPU: `--gpus N` must be the number of ranks that run.

* WORLD_SIZE set by a launcher and different from --gpus: refuse, loudly, before anything else happens;
* WORLD_SIZE unset and --gpus N > 1: bench.py starts the N ranks itself through torch.distributed.run (here: on a box
  without a HIP device every rank ends with "needs a HIP device", which is the proof that N rank processes were started and
  that the parent, which must never touch the GPU before spawning, left with their status)."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _run(args, env_extra, timeout=300):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(env_extra)
    return subprocess.run([sys.executable, BENCH] + args, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout)


def test_gpus_must_match_world_size():
    r = _run(["--gpus", "2", "--steps", "1", "--warmup", "0"], {"WORLD_SIZE": "4", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode != 0
    assert b"--gpus 2" in r.stderr and b"WORLD_SIZE=4" in r.stderr, r.stderr[-400:]
    assert not r.stdout.strip()                             # no JSON line from a refused run


def test_effective_cores_respects_the_cgroup_quota():
    sys.path.insert(0, ROOT)
    import importlib
    bench = importlib.import_module("bench")
    n = bench._effective_cores()
    affinity = len(os.sched_getaffinity(0))
    assert 1 <= n <= affinity
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
    except OSError:
        return
    if q != "max":
        assert n <= -(-int(q) // int(per))


def test_gpus_n_spawns_n_ranks_without_a_launcher():
    import importlib
    mi = importlib.import_module("lsp-dsp-units_amd")
    if mi.device_count() > 0:
        import pytest
        pytest.skip("GPU box: the rehearsal of this path is a gpu test (tests/test_sharding_gloo.py covers the sharded arithmetic)")
    r = _run(["--gpus", "2", "--steps", "1", "--warmup", "0", "--workload", "biquad", "--no-cpu-baseline"], {})
    assert r.returncode != 0                                # the ranks' status, not the parent's own
    assert r.stderr.count(b"bench.py needs a HIP device") >= 2, r.stderr[-800:]


def _canned_full_result():
    """A full (detail) result as bench.py builds it: round 4's 20 KB line, committed under profiles/."""
    import json
    return json.load(open(os.path.join(ROOT, "profiles", "r04_driver_cmd_bench_line.json")))


def test_final_line_fits_the_drivers_tail(tmp_path, capsys, monkeypatch):
    """the driver keeps the last ~8 KB of stdout + stderr and parses the final line; round 4's line had grown to
    20 KB and BENCH_r04 was `parsed: null`.  The line must stay under 4 KB, parse from the last 4096 bytes of stdout, and carry
    the contract's keys with `roofline` and `cpu_baseline`."""
    import importlib
    import json
    sys.path.insert(0, ROOT)
    bench = importlib.import_module("bench")
    full = _canned_full_result()
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))       # (the detail file goes to <ROOT>/gpurun_out)
    print("x" * 20000)                                      # whatever was on stdout before the line
    bench.emit(full)
    out = capsys.readouterr()
    assert out.err == ""                                    # nothing on stderr: the driver's tail is one buffer for both
    tail = out.out.encode()[-4096:].decode()
    last = tail.rstrip("\n").split("\n")[-1]
    assert len(last) < 4096
    line = json.loads(last)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in line, k
    assert line["value"] == full["value"] and line["ms_per_step"] == full["ms_per_step"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic", "kernel"):
        assert k in line["roofline"], k
    assert line["roofline"]["frac"] == full["roofline"]["frac"]
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in line["cpu_baseline"], k
    assert "workload" in line["config"] and "model" not in line["config"]
    for sub in ("convolver", "equalizer", "spectral"):
        assert line[sub]["value"] == full[sub]["value"] and "frac" in line[sub]["roofline"]
    detail = json.load(open(os.path.join(str(tmp_path), line["detail"])))
    assert detail["timing"]["region_ms"]["in_order"] == full["timing"]["region_ms"]["in_order"]     # nothing is lost, only moved


def test_final_line_sheds_parts_rather_than_grow():
    import importlib
    import json
    sys.path.insert(0, ROOT)
    bench = importlib.import_module("bench")
    full = _canned_full_result()
    full["next_rows"] = {"row%d" % i: {"value": 1.0, "ms_per_step": 0.1, "whole_step": {"frac": 0.5}} for i in range(200)}
    full["config"]["workload"] = "w" * 5000
    line = bench.compact_line(full, "gpurun_out/bench_detail.json")
    text = json.dumps(line)
    assert len(text) <= bench.LINE_LIMIT
    assert "roofline" in line and "cpu_baseline" in line and "value" in line


def test_plain_run_refuses_what_only_the_full_run_does():
    """A run without --full measures the headline alone; asking it for a sub-workload or for repeated regions is refused
    before anything else happens (no JSON line, no device touched)."""
    for extra, word in ((["--workload", "convolver"], b"--full"), (["--regions", "5"], b"--full"),
                        (["--full", "--workload", "spectral", "--dump-outputs", "x"], b"--dump-outputs")):
        r = _run(["--gpus", "1", "--steps", "1", "--warmup", "0"] + extra, {})
        assert r.returncode != 0, extra
        assert word in r.stderr, (extra, r.stderr[-400:])
        assert not r.stdout.strip(), extra


def test_dump_outputs_writes_float32_within_the_limit(tmp_path, monkeypatch):
    import importlib
    import numpy as np
    sys.path.insert(0, ROOT)
    bench = importlib.import_module("bench")
    out = np.random.default_rng(1).standard_normal((64, 256)).astype(np.float32)
    bench._dump_outputs(str(tmp_path / "a"), "biquad_out", out)
    got = np.load(str(tmp_path / "a" / "biquad_out.npy"))
    assert got.dtype == np.float32 and np.array_equal(got, out)
    assert not (tmp_path / "a" / "biquad_out_channels.npy").exists()
    # over the limit: the rows of a fixed seeded sample of the channels, and which rows they are
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 16 * out[0].nbytes)
    for d in ("b", "c"):
        bench._dump_outputs(str(tmp_path / d), "biquad_out", out)
    files = [tmp_path / "b" / "biquad_out.npy", tmp_path / "b" / "biquad_out_channels.npy"]
    assert sum(os.path.getsize(str(f)) for f in files) <= bench.DUMP_LIMIT_BYTES
    rows = np.load(str(files[1]))
    assert rows.dtype == np.float64 and len(rows) > 0 and np.all(np.diff(rows) > 0)
    assert np.array_equal(np.load(str(files[0])), out[rows.astype(np.int64)])
    assert np.array_equal(rows, np.load(str(tmp_path / "c" / "biquad_out_channels.npy")))


@pytest.mark.gpu
def test_plain_run_is_lean_and_its_outputs_repeat(gpu, tmp_path):
    """Without --full: one timed region of exactly --steps steps, the contract's keys and nothing measured beside them.  The
    blocks --dump-outputs writes are those of step W + K - 1, recomputed here from the same seeded inputs by W + K process()
    calls of a fresh bank: a wrong ring slot, a block of the warm-up or of the scratch bank's settle phase, or a number of steps
    other than W + K would differ.  A second run and a --full run (whose timed regions repeat a clock-sized number of times)
    write the same bits."""
    import json
    import numpy as np
    sys.path.insert(0, ROOT)
    import importlib
    bench = importlib.import_module("bench")
    C, n, ring, W, K = 128, 4096, 4, 3, 7
    common = ["--gpus", "1", "--steps", str(K), "--warmup", str(W), "--channels", str(C), "--ring", str(ring)]
    lines, outs = {}, {}
    for d, extra in (("a", []), ("b", []), ("full", ["--full", "--workload", "biquad", "--no-cpu-baseline"])):
        r = _run(common + extra + ["--dump-outputs", str(tmp_path / d)], {"MI_BENCH_DETAIL": "bench_detail_test.json"}, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        lines[d] = json.loads(r.stdout.decode().strip().splitlines()[-1])
        outs[d] = np.load(str(tmp_path / d / "biquad_out.npy"))
    line = lines["a"]
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in line, k
    assert line["steps"] == K and line["warmup"] == W and line["timing"]["regions"] == 1
    assert line["ms_per_step"] > 0 and line["value"] > 0 and line["timing"]["settle_calls"] > 0
    for k in ("roofline", "cpu_baseline", "per_call", "exact_mode", "convolver", "next_rows"):
        assert k not in line, k
    assert "roofline" in lines["full"] and lines["full"]["timing"]["regions"] > 1

    # bench.py's inputs: C2 cutoffs from seed 3 designed by the product's designer, blocks from torch's CPU generator, seed 2 + rank
    fc = np.exp(np.random.default_rng(3).uniform(np.log(200.0), np.log(18000.0), size=C))
    coef = np.zeros((C, 8, 5), np.float32)
    for c in range(C):
        coef[c] = gpu.design_filter(bench.FLT_BT_LRX_LOPASS, 4, float(fc[c]), float(fc[c]), 1.0, 0.75, 48000)[2]
    # (torch in a child process of its own: a second HIP runtime in this one leaves the tests that call HIP directly without a device)
    xp = str(tmp_path / "x.npy")
    subprocess.check_call([sys.executable, "-c", "import sys, numpy, torch; g = torch.Generator(device='cpu'); g.manual_seed(2); "
                           "numpy.save(sys.argv[1], (torch.randn((%d, %d, %d), generator=g, dtype=torch.float32) * 0.25).numpy())"
                           % (ring, C, n), xp])
    x = np.load(xp)
    bank = gpu.BiquadBank(C, 8)
    bank.set_all_chains(coef)
    ins = [gpu.DeviceBuffer.from_host(np.ascontiguousarray(x[k])) for k in range(ring)]
    out = gpu.DeviceBuffer((C, n))
    for i in range(W + K):
        bank.process(out, ins[i % ring], n)
    want = out.download()
    bank.close()
    assert outs["a"].dtype == np.float32 and outs["a"].shape == (C, n) and np.abs(want).max() > 0
    assert np.array_equal(outs["a"], want), np.abs(outs["a"] - want).max()
    assert np.array_equal(outs["b"], want) and np.array_equal(outs["full"], want)
