"""The AutoGain and SimpleAutoGain banks under what test_streams_gpu.py, test_lifecycle_gpu.py and test_abi_bad_args_gpu.py hold
the other banks to: a caller's own stream and two streams at once, create / use / destroy cycles and calls after close(), and
every entry point on a live bank with zeros and NULL for all other arguments.  Each in a child process with a time limit, so
that a crash or a hang is reported by name."""
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
import autogain_ref as ar
f32 = np.float32
C, n = 6, 550

class Auto:
    """the two calls of a bank, so that both kinds go through the same cases"""
    prefix = "mi_autogain_bank_"
    def __init__(self, seed=0):
        self.b = gpu.AutoGainBank(C)
        for ch in range(C):
            quick, limit = ar.switches(ch + seed)
            self.b.configure(ch, quick_amp=quick, limit=limit, **ar.settings_of(ch + seed))
    def data(self, seed):
        return ar.signal(seed, C)
    def call(self, x, k, st=None):
        d = [gpu.DeviceBuffer.from_host(v[:, k * n:(k + 1) * n], stream=st) for v in x]
        out = gpu.DeviceBuffer((C, n))
        if k == 1:
            self.b.set_max_gain(1, 0.5, True)           # a pending upload: it goes on the stream
            self.b.set_deviation(2, 3.0)
        self.b.process(out, d[0], d[1], d[2], n, stream=st)
        return out, d
    def state(self, st=None):
        return [self.b.get_state(ch, stream=st) for ch in range(C)]
    def others(self, x):
        d = [gpu.DeviceBuffer.from_host(v[:, :n]) for v in x]
        lv = gpu.DeviceBuffer.from_host(x[2][:, 0])
        return [lambda: self.b.process_level(d[0], d[0], d[1], lv, n), lambda: self.b.process_apply(d[1], d[1], d[0], d[1], d[2], n)]
    def methods(self, d):
        b = self.b
        return [lambda: b.process(d, d, d, d, n), lambda: b.process_level(d, d, d, d, n), lambda: b.process_apply(d, d, d, d, d, n),
                lambda: b.update_settings(), lambda: b.set_deviation(0, 2.0), lambda: b.enable_quick_amplifier(0, True),
                lambda: b.get_state(0), lambda: b.get_params(0)]

class Simple(Auto):
    prefix = "mi_simple_autogain_bank_"
    def __init__(self, seed=0):
        self.b = gpu.SimpleAutoGainBank(C)
        for ch in range(C):
            self.b.set_sample_rate(ch, 1000)
            self.b.set_speed(ch, 100.0 + ch + seed, 120.0 - ch)
            self.b.set_threshold(ch, 0.1)
            self.b.set_gain(ch, 0.25, 4.0)
    def data(self, seed):
        return (ar.simple_signal(seed, C, 2 * n),)
    def call(self, x, k, st=None):
        d = gpu.DeviceBuffer.from_host(x[0][:, k * n:(k + 1) * n], stream=st)
        out = gpu.DeviceBuffer((C, n))
        if k == 1:
            self.b.set_max_gain(1, 0.5)                 # recorded: sent and applied on the stream
            self.b.set_max_gain(1, 2.0)
            self.b.set_fall(2, 60.0)
        self.b.process(out, d, n, stream=st)
        return out, d
    def others(self, x):
        return []
    def methods(self, d):
        b = self.b
        return [lambda: b.process(d, d, n), lambda: b.update_settings(), lambda: b.set_grow(0, 2.0), lambda: b.set_max_gain(0, 3.0),
                lambda: b.get_state(0), lambda: b.get_params(0)]

KINDS = (Auto, Simple)

def same(a, b):
    return np.array_equal(np.ascontiguousarray(a, f32).view(np.uint32), np.ascontiguousarray(b, f32).view(np.uint32))

def stream():
    st = ctypes.c_void_p()
    gpu.check(gpu.lib.mi_dspu_stream_create(ctypes.byref(st)))
    return st
''' % (ROOT, ROOT)

STREAMS = PRELUDE + r'''
def run(u, x, st):
    s = None if st is None else st.value
    out = [u.call(x, k, s)[0].download(stream=s) for k in range(2)]
    return np.concatenate(out, axis=1), u.state(s)
for kind in KINDS:
    x = [kind().data(1), kind().data(2)]
    # the default stream, a stream of the caller's own, and two banks on two streams taking turns
    base = [run(kind(i), x[i], None) for i in range(2)]
    st = [stream(), stream()]
    side = run(kind(0), x[0], st[0])
    assert same(side[0], base[0][0]) and side[1] == base[0][1], "a side stream gives other bits"
    units, outs = [kind(0), kind(1)], [[], []]
    for k in range(2):
        for i in range(2):
            outs[i].append(units[i].call(x[i], k, st[i].value))
    for i in range(2):
        got = np.concatenate([g.download(stream=st[i].value) for g, _ in outs[i]], axis=1)
        assert same(got, base[i][0]), "two streams disturb each other (%s %d)" % (kind.__name__, i)
        assert units[i].state(st[i].value) == base[i][1]
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
for kind in KINDS:
    x = kind().data(3)
    def cycle():
        u = kind()
        out = [u.call(x, k)[0].download() for k in range(2)]
        for f in u.others(x):
            f()
        u.b.close()
        return np.concatenate(out, axis=1), u
    first, _ = cycle()
    before = free_bytes()
    for _ in range(20):
        out, u = cycle()
        assert same(out, first)
    assert before - free_bytes() < (4 << 20), "device memory does not come back: %d bytes" % (before - free_bytes())
    # after close(): every method answers with an error, none touches the freed bank; closing twice is allowed
    u.b.close()
    d = gpu.DeviceBuffer.from_host(np.ones((C, n), f32))
    for call in u.methods(d):
        try:
            call()
        except gpu.MiError as e:
            assert e.code < 0
        else:
            raise AssertionError("a closed bank answered")
    # a bank that is dropped without close() is destroyed with its last reference
    u = kind(); del u
print("DONE", flush=True)
'''

BAD_ARGS = PRELUDE + r'''
bad, calls = [], 0
for kind in KINDS:
    for name, (res, args) in sorted(capi.PROTOTYPES.items()):
        if not name.startswith(kind.prefix) or name.endswith(("_create", "_destroy")) or res is not ctypes.c_int:
            continue
        u = kind()                                       # a fresh bank for every call
        print("CALL", name, flush=True)
        zeros = [ctypes.c_void_p(u.b.handle.value)]
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
        # ... with a NULL bank
        if getattr(capi.lib, name)(None, *zeros[1:]) >= 0:
            bad.append((name, "NULL bank"))
        # ... and with a count but NULL buffers
        if "_process" in name:
            zeros[1 + [i for i, a in enumerate(args[1:]) if a is ctypes.c_size_t][0]] = 64
            code = getattr(capi.lib, name)(*zeros)
            if code >= 0:
                bad.append((name, "NULL buffers", code))
        x = u.data(4)
        u.call(x, 0)[0].download()                       # the bank still works
        u.b.close()
    h = ctypes.c_void_p()
    create = getattr(capi.lib, kind.prefix + "create")
    for channels in (0, 1 << 21):
        code = create(ctypes.byref(h), channels)
        if code >= 0 or h.value:
            bad.append((kind.prefix, "create", channels, code))
    if create(None, 2) >= 0:
        bad.append((kind.prefix, "create", "NULL result"))
    if getattr(capi.lib, kind.prefix + "destroy")(None) != 0:
        bad.append((kind.prefix, "destroy", "NULL bank"))
print("DONE", calls, bad, flush=True)
sys.exit(1 if bad or calls < 19 + 12 else 0)
'''


@pytest.mark.parametrize("child", ["STREAMS", "LIFETIMES", "BAD_ARGS"])
def test_in_a_child_process(gpu, child):
    r = subprocess.run([sys.executable, "-c", globals()[child]], capture_output=True, text=True, timeout=240)
    calls = [ln.split()[1] for ln in r.stdout.splitlines() if ln.startswith("CALL")]
    assert r.returncode == 0 and "DONE" in r.stdout, "last call: %s\n%s\n%s" % (calls[-1] if calls else None, r.stdout[-1500:], r.stderr[-2500:])
