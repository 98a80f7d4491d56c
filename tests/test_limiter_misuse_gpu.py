"""The limiter bank under what test_streams_gpu.py, test_lifecycle_gpu.py and test_abi_bad_args_gpu.py hold the other banks to:
a caller's own stream and two streams at once, create / use / destroy cycles and calls after close(), and every entry point
on a live bank with zeros and NULL for all other arguments.  Each in a child process with a time limit, so that a crash or a
hang is reported by name."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PRELUDE = r'''
import ctypes, importlib, os, sys
import numpy as np
sys.path.insert(0, %r)
sys.path.insert(0, os.path.join(%r, "tests"))
gpu = importlib.import_module("lsp-dsp-units_amd")
capi = importlib.import_module("lsp-dsp-units_amd.capi")
import limiter_ref as lr
f32 = np.float32
C, n = 6, 700

def make(seed=0):
    b = gpu.LimiterBank(C, 48000, 0.5)
    for ch in range(C):
        b.configure(ch, 48000, (ch + seed) %% 12, 0.3 + 0.02 * ch, 0.2 + 0.05 * ch, 0.2, 0.4, alr=(ch %% 2 == 0))
    return b

def same(a, b):
    return np.array_equal(np.ascontiguousarray(a, f32).view(np.uint32), np.ascontiguousarray(b, f32).view(np.uint32))

def stream():
    st = ctypes.c_void_p()
    gpu.check(gpu.lib.mi_dspu_stream_create(ctypes.byref(st)))
    return st
''' % (ROOT, ROOT)

STREAMS = PRELUDE + r'''
x = [lr.bursts(1, C, 2 * n), lr.bursts(2, C, 2 * n)]
def run(b, x, st):
    s = None if st is None else st.value
    out = []
    for k in range(2):
        d, g = gpu.DeviceBuffer.from_host(x[:, k * n:(k + 1) * n], stream=s), gpu.DeviceBuffer((C, n))
        if k == 1:
            b.set_threshold(1, 0.2, False)              # a pending setting: the upload and the window's scaling go on the stream
        b.process(g, d, n, stream=s)
        out.append(g.download(stream=s))
    return np.concatenate(out, axis=1), [b.get_state(ch, stream=s) for ch in range(C)]
# the default stream, a stream of the caller's own, and two banks on two streams taking turns
base = [run(make(i), x[i], None) for i in range(2)]
st = [stream(), stream()]
side = run(make(0), x[0], st[0])
assert same(side[0], base[0][0]) and side[1] == base[0][1], "a side stream gives other bits"
banks = [make(0), make(1)]
outs = [[], []]
for k in range(2):
    for i in range(2):
        s = st[i].value
        d, g = gpu.DeviceBuffer.from_host(x[i][:, k * n:(k + 1) * n], stream=s), gpu.DeviceBuffer((C, n))
        if k == 1:
            banks[i].set_threshold(1, 0.2, False)
        banks[i].process(g, d, n, stream=s)
        outs[i].append((g, d))
for i in range(2):
    got = np.concatenate([g.download(stream=st[i].value) for g, _ in outs[i]], axis=1)
    assert same(got, base[i][0]), "two streams disturb each other (bank %d)" % i
    assert [banks[i].get_state(ch, stream=st[i].value) for ch in range(C)] == base[i][1]
for s in st:
    gpu.check(gpu.lib.mi_dspu_stream_destroy(s))
print("DONE", flush=True)
'''

LIFETIMES = PRELUDE + r'''
hip = ctypes.CDLL("libamdhip64.so")
def free_bytes():
    free, total = ctypes.c_size_t(), ctypes.c_size_t()
    assert hip.hipDeviceSynchronize() == 0 and hip.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) == 0
    return free.value
x = lr.bursts(3, C, n)
def cycle():
    b = make()
    d, g = gpu.DeviceBuffer.from_host(x), gpu.DeviceBuffer((C, n))
    b.process(g, d, n)
    b.process_apply(g, d, d, n)
    out = g.download()
    b.close()
    return out, b
first, _ = cycle()
before = free_bytes()
for _ in range(20):
    out, b = cycle()
    assert same(out, first)
assert before - free_bytes() < (4 << 20), "device memory does not come back: %d bytes" % (before - free_bytes())
# after close(): every method answers with an error, none touches the freed bank; closing twice is allowed
b.close()
d = gpu.DeviceBuffer.from_host(x)
for call in (lambda: b.process(d, d, n), lambda: b.process_apply(d, d, d, n), lambda: b.update_settings(), lambda: b.clear(),
             lambda: b.set_mode(0, 1), lambda: b.get_state(0), lambda: b.get_patch(0), lambda: b.get_params(0), lambda: b.get_latency(0)):
    try:
        call()
    except gpu.MiError as e:
        assert e.code < 0
    else:
        raise AssertionError("a closed bank answered")
# a bank that is dropped without close() is destroyed with its last reference
b = make(); del b
print("DONE", flush=True)
'''

BAD_ARGS = PRELUDE + r'''
bad, calls = [], 0
for name, (res, args) in sorted(capi.PROTOTYPES.items()):
    if not name.startswith("mi_limiter_bank_") or name.endswith(("_create", "_destroy")) or res is not ctypes.c_int:
        continue
    b = make()                                       # a fresh bank for every call
    print("CALL", name, flush=True)
    zeros = [ctypes.c_void_p(b.handle.value)]
    for a in args[1:]:
        if a in (ctypes.c_float, ctypes.c_double):
            zeros.append(0.0)
        elif a in (ctypes.c_int, ctypes.c_uint32, ctypes.c_size_t, ctypes.c_uint64, ctypes.c_int64):
            zeros.append(0)
        else:
            zeros.append(None)
    code = getattr(capi.lib, name)(*zeros)
    calls += 1
    if code > 0:
        bad.append((name, code))
    # ... and with a count but NULL buffers
    if name.endswith(("_process", "_process_apply")):
        zeros[1 + [i for i, a in enumerate(args[1:]) if a is ctypes.c_size_t][0]] = 64
        code = getattr(capi.lib, name)(*zeros)
        if code >= 0:
            bad.append((name, "NULL buffers", code))
    d = gpu.DeviceBuffer.from_host(lr.bursts(4, C, n))
    b.process(d, d, n)                               # the bank still works
    b.close()
h = ctypes.c_void_p()
for channels, sr, ms in ((0, 48000, 1.0), (1 << 21, 48000, 1.0), (2, 48000, -1.0), (2, 192000, 25.0), (2, 48000, float("nan"))):
    code = capi.lib.mi_limiter_bank_create(ctypes.byref(h), channels, sr, ms)
    if code >= 0 or h.value:
        bad.append(("create", channels, sr, ms, code))
if capi.lib.mi_limiter_bank_create(None, 2, 48000, 1.0) >= 0:
    bad.append(("create", "NULL result"))
print("DONE", calls, bad, flush=True)
sys.exit(1 if bad or calls < 15 else 0)
'''


@pytest.mark.parametrize("child", ["STREAMS", "LIFETIMES", "BAD_ARGS"])
def test_in_a_child_process(gpu, child):
    r = subprocess.run([sys.executable, "-c", globals()[child]], capture_output=True, text=True, timeout=240)
    calls = [ln.split()[1] for ln in r.stdout.splitlines() if ln.startswith("CALL")]
    assert r.returncode == 0 and "DONE" in r.stdout, "last call: %s\n%s\n%s" % (calls[-1] if calls else None, r.stdout[-1500:], r.stderr[-2500:])
