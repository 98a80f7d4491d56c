"""What the sample entries of the per-channel table banks refuse, and what they let through: NULL rows, a count at the entry's
limit, strides shorter than the rows, in place with different strides, and the two refusals that are a bank's own.  Raw
capi.lib calls (the Python wrappers default the strides), 2 channels x 8 samples in buffers of 2 x 24 floats with row stride
16, the stride cases again on a bank of one channel.  A refusal names its C entry, launches nothing and leaves every
channel's state as it was.  The expected codes are read from the entries' sources: MI_OK = 0, MI_EINVAL = -1.

Where an entry's own rules differ from the general ones, the table says so:
  - mi_truepeak_bank_process_max wants its `peaks` array even for count == 0 (it zeroes it);
  - the Oversampler's upsample() and downsample() refuse dst == src whatever the strides;
  - a Sidechain bank of two inputs refuses in0 without in1 ("without the second one"), and NULL in0 is silence;
  - downsample() with the anti-alias filter on hands src to the biquad bank, whose own stride check has no exemption for a
    bank of one channel;
  - the dynamics' get_state() takes each of its result pointers or NULL.
The curve entries word their count refusal "too many" or "too large".

The checks run in a child process with a time limit, so that a crash or a hang is reported by the entry's name."""
import ctypes
import importlib
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

MI_OK, MI_EINVAL = 0, -1
COUNT, STRIDE, WIDE, ROW = 8, 16, 24, 24            # samples; the valid row stride; another one; floats of a buffer's row
BANKS = ("compressor", "expander", "gate", "dynproc", "sidechain1", "sidechain2", "limiter", "autogain", "simple_autogain",
         "correlometer", "panometer", "truepeak", "oversampler")


class Row:
    """One pointer argument of a sample entry.  need: "req" (NULL is refused with NULL in the message), "opt" (NULL is allowed),
    "second" (the Sidechain's in1: refused when missing beside in0).  times: the row holds count x times samples.
    strided: False for the per-channel arrays (levels, peaks), which have no stride argument and are no sample rows.
    single: False where a bank of one channel refuses a short stride too."""

    def __init__(self, name, out=False, need="req", times=1, strided=True, single=True):
        self.name, self.out, self.need, self.times, self.strided, self.single = name, out, need, times, strided, single


class Entry:
    """A sample entry: its C name, the rows, the order of its arguments ("n": count, "st": stream, ("p", row), ("s", row),
    ("v", value)), its count limit, and what is its own: alias "never" (dst == src always refused), own = pairs of rows
    that must differ, zero_needs = rows wanted even for count == 0."""

    def __init__(self, name, rows, args, limit=1 << 31, alias="same stride", own=(), zero_needs=(), count_words=("too large",)):
        self.name, self.rows, self.args, self.limit, self.alias, self.own = name, rows, args, limit, alias, own
        self.zero_needs, self.count_words = zero_needs, count_words


def _args(*names, tail=()):
    """pointers, count, the strides of the strided ones, stream"""
    return [("p", n) for n in names] + ["n"] + [("s", n) for n in names] + list(tail) + ["st"]


def entries(kind, times=1):
    p = "mi_%s_bank_" % kind.rstrip("12")
    if kind in ("compressor", "expander", "gate", "dynproc"):
        out_in = [Row("out", out=True), Row("in")]
        curve_args = _args("out", "in")
        if kind == "gate":
            curve_args = [("p", "out"), ("p", "in"), "n", ("v", 0), ("s", "out"), ("s", "in"), "st"]
        es = [Entry(p + "process", [Row("gain", out=True), Row("env", out=True, need="opt"), Row("in")], _args("gain", "env", "in"),
                    own=[("gain", "env")]),
              Entry(p + "process_apply", [Row("dst", out=True), Row("audio"), Row("sc")], _args("dst", "audio", "sc")),
              Entry(p + "curve", out_in, curve_args, count_words=("too large", "too many"))]
        if kind == "dynproc":
            es.append(Entry(p + "model", out_in, _args("out", "in"), count_words=("too large", "too many")))
        return es
    if kind in ("sidechain1", "sidechain2"):
        two = kind == "sidechain2"
        rows = [Row("out", out=True), Row("in0", need="opt")] + ([Row("in1", need="second")] if two else [])
        args = [("p", "out"), ("p", "in0"), ("p", "in1") if two else ("v", None), "n", ("s", "out"), ("s", "in0"),
                ("s", "in1") if two else ("v", STRIDE), "st"]
        return [Entry(p + "process", rows, args), Entry(p + "premix", rows, args),
                Entry(p + "process_premixed", [Row("out", out=True), Row("in", need="opt")], _args("out", "in"))]
    if kind == "limiter":
        return [Entry(p + "process", [Row("gain", out=True), Row("sc")], _args("gain", "sc"), limit=1 << 30),
                Entry(p + "process_apply", [Row("dst", out=True), Row("audio"), Row("sc")], _args("dst", "audio", "sc"), limit=1 << 30)]
    if kind == "autogain":
        levels = [Row("vca", out=True), Row("long"), Row("short"), Row("levels", strided=False)]
        return [Entry(p + "process", [Row("vca", out=True), Row("long"), Row("short"), Row("exp")], _args("vca", "long", "short", "exp")),
                Entry(p + "process_level", levels, [("p", "vca"), ("p", "long"), ("p", "short"), ("p", "levels"), "n", ("s", "vca"),
                                                    ("s", "long"), ("s", "short"), "st"], own=[("vca", "levels")]),
                Entry(p + "process_apply", [Row("dst", out=True), Row("audio"), Row("long"), Row("short"), Row("exp")],
                      _args("dst", "audio", "long", "short", "exp"))]
    if kind == "simple_autogain":
        return [Entry(p + "process", [Row("dst", out=True), Row("src")], _args("dst", "src"))]
    if kind in ("correlometer", "panometer"):
        return [Entry(p + "process", [Row("out", out=True), Row("a"), Row("b")], _args("out", "a", "b"))]
    if kind == "truepeak":
        return [Entry(p + "process", [Row("dst", out=True), Row("src")], _args("dst", "src")),
                Entry(p + "process_max", [Row("peaks", strided=False), Row("src")], [("p", "peaks"), ("p", "src"), "n", ("s", "src"), "st"],
                      zero_needs=("peaks",))]
    assert kind == "oversampler"
    return [Entry(p + "upsample", [Row("dst", out=True, times=times), Row("src")], _args("dst", "src"), limit=1 << 27, alias="never"),
            Entry(p + "downsample", [Row("dst", out=True), Row("src", times=times, single=False)], _args("dst", "src"), limit=1 << 27,
                  alias="never"),
            Entry(p + "process", [Row("dst", out=True), Row("src")], _args("dst", "src", tail=[("v", None), ("v", None)]), limit=1 << 27)]


OVERSAMPLING = 2


def make_bank(gpu, kind, channels):
    """the bank configured as its own GPU test configures it, settings on the device"""
    if HERE not in sys.path:
        sys.path.insert(0, HERE)
    if kind in ("compressor", "expander", "gate", "dynproc"):
        ref = importlib.import_module({"compressor": "compressor_ref", "expander": "expander_ref", "gate": "gate_ref",
                                       "dynproc": "dynproc_ref"}[kind])
        b = {"compressor": gpu.CompressorBank, "expander": gpu.ExpanderBank, "gate": gpu.GateBank,
             "dynproc": gpu.DynamicProcessorBank}[kind](channels)
        for ch in range(channels):
            b.configure(ch, **ref.channel_settings(ch))
    elif kind in ("sidechain1", "sidechain2"):
        b = gpu.SidechainBank(channels, int(kind[-1]), 10.0)
        for ch in range(channels):
            b.configure(ch, sample_rate=48000, reactivity=1.0 + ch, mode=(b.SCM_RMS, b.SCM_LPF)[ch % 2], gain=(1.0, 0.5)[ch % 2])
    elif kind == "limiter":
        b = gpu.LimiterBank(channels, 48000, 0.5)
        for ch in range(channels):
            b.configure(ch, sample_rate=48000, mode=ch % 4, threshold=0.5, lookahead=0.3, attack=0.2, release=0.2)
    elif kind == "autogain":
        ar = importlib.import_module("autogain_ref")
        b = gpu.AutoGainBank(channels)
        for ch in range(channels):
            b.configure(ch, quick_amp=True, limit=ch % 2 == 0, **ar.settings_of(ch))
    elif kind == "simple_autogain":
        b = gpu.SimpleAutoGainBank(channels)
        for ch in range(channels):
            b.set_sample_rate(ch, 1000), b.set_speed(ch, 100.0, 120.0), b.set_threshold(ch, 0.1), b.set_gain(ch, 0.25, 4.0)
    elif kind in ("correlometer", "panometer"):
        b = (gpu.CorrelometerBank if kind == "correlometer" else gpu.PanometerBank)(channels, 64)
        for ch in range(channels):
            b.configure(ch, 5 + ch)
    elif kind == "truepeak":
        b = gpu.TruePeakBank(channels)
        b.set_sample_rate(48000)
    else:
        b = gpu.OversamplerBank(channels)
        b.set_sample_rate(48000), b.set_mode(b.MODES["%dX16BIT" % OVERSAMPLING]), b.set_filtering(True)
    b.update_settings()
    return b


class Checker:
    def __init__(self, gpu, capi):
        self.gpu, self.capi, self.lib, self.cases = gpu, capi, capi.lib, 0
        # one buffer per role a row can play, all of 2 x ROW floats holding 0.1 (AutoGain's levels have to be > 0)
        import numpy as np
        self.bufs = [gpu.DeviceBuffer.from_host(np.full((2, ROW), 0.1, np.float32)) for _ in range(6)]

    def handle(self, bank):
        return ctypes.c_void_p(bank.handle.value if hasattr(bank.handle, "value") else bank.handle)

    def state(self, bank):
        if not hasattr(bank, "get_state"):
            return None
        return [repr(bank.get_state(ch)) for ch in range(bank.channels)]

    def message(self):
        return (self.lib.mi_dspu_last_error() or b"").decode("utf-8", "replace")

    def call(self, bank, e, ptrs, strides, count=COUNT):
        argv = [self.handle(bank)]
        for a in e.args:
            if a == "n":
                argv.append(count)
            elif a == "st":
                argv.append(None)
            elif a[0] == "p":
                argv.append(ptrs[a[1]])
            elif a[0] == "s":
                argv.append(strides[a[1]])
            else:
                argv.append(a[1])
        print("CALL", e.name, ptrs, strides, count, flush=True)
        self.cases += 1
        return getattr(self.lib, e.name)(*argv)

    def valid(self, e):
        ptrs = {r.name: self.bufs[i].ptr for i, r in enumerate(e.rows)}
        return ptrs, {r.name: STRIDE for r in e.rows if r.strided}

    def accepted(self, bank, e, ptrs, strides, count=COUNT):
        code = self.call(bank, e, ptrs, strides, count)
        assert code == MI_OK, (e.name, code, self.message(), ptrs, strides, count)

    def refused(self, bank, e, ptrs, strides, count=COUNT, words=()):
        """MI_EINVAL with the entry's name (and one of `words`) in the message, no launch, the state untouched"""
        launch, state = self.lib.mi_dspu_last_launch(), self.state(bank)
        code = self.call(bank, e, ptrs, strides, count)
        msg = self.message()
        assert code == MI_EINVAL, (e.name, code, msg, ptrs, strides, count)
        assert e.name in msg and (not words or any(w in msg for w in words)), (e.name, msg, words)
        assert self.lib.mi_dspu_last_launch() == launch, (e.name, msg, launch, self.lib.mi_dspu_last_launch())
        assert self.state(bank) == state, (e.name, msg, state, self.state(bank))

    def sample_entries(self, kind, bank, single):
        for e in entries(kind, OVERSAMPLING):
            assert e.name in self.capi.PROTOTYPES, e.name
            ptrs, strides = self.valid(e)
            self.accepted(bank, e, ptrs, strides)                                                    # 1
            nothing = {r.name: None for r in e.rows}
            if e.zero_needs:                                                                         # 2
                self.refused(bank, e, nothing, strides, 0, words=("NULL",))
                self.accepted(bank, e, dict(nothing, **{n: ptrs[n] for n in e.zero_needs}), strides, 0)
            else:
                self.accepted(bank, e, nothing, strides, 0)
            for r in e.rows:                                                                         # 3
                without = dict(ptrs, **{r.name: None})
                if r.need == "req":
                    self.refused(bank, e, without, strides, words=("NULL",))
                elif r.need == "second":
                    self.refused(bank, e, without, strides)
                else:
                    self.accepted(bank, e, without, strides)
            self.refused(bank, e, ptrs, strides, e.limit, words=e.count_words)                       # 4
            for r in e.rows:                                                                         # 5
                for short in sorted({COUNT - 1, COUNT * r.times - 1}) if r.strided else ():
                    self.refused(bank, e, ptrs, dict(strides, **{r.name: short}), words=("shorter",))
                    if r.single:
                        self.accepted(single, e, ptrs, dict(strides, **{r.name: short}))
                    else:
                        assert self.call(single, e, ptrs, dict(strides, **{r.name: short})) == MI_EINVAL, (e.name, r.name, self.message())
            for o in (r for r in e.rows if r.out):                                                   # 6
                for i in (r for r in e.rows if not r.out and r.strided):
                    same = dict(ptrs, **{i.name: ptrs[o.name]})
                    if e.alias == "never":
                        self.refused(bank, e, same, dict(strides, **{o.name: STRIDE, i.name: WIDE}))
                        self.refused(bank, e, same, strides)
                    else:
                        self.refused(bank, e, same, dict(strides, **{o.name: STRIDE, i.name: WIDE}), words=("in place",))
                        self.refused(bank, e, same, dict(strides, **{o.name: WIDE, i.name: STRIDE}), words=("in place",))
                        self.accepted(bank, e, same, strides)
            for a, b in e.own:                                                                       # 7
                self.refused(bank, e, dict(ptrs, **{b: ptrs[a]}), strides)

    def channel_entries(self, kind, bank):
        """every per-channel getter and setter: channel == channels, and NULL for the parameters or the state"""
        if kind in ("truepeak", "oversampler"):
            return                                                  # no per-channel entries: their second argument is no channel
        p = "mi_%s_bank_" % kind.rstrip("12")
        c_u32 = ctypes.c_uint32
        for name, (res, args) in sorted(self.capi.PROTOTYPES.items()):
            what = name[len(p):]
            if not name.startswith(p) or len(args) < 2 or args[1] is not c_u32 or what == "create":
                continue
            assert what.startswith(("set_", "get_", "enable_")) or what == "clear", name
            zeros = [0.0 if a in (ctypes.c_float, ctypes.c_double) else 0 if a in (ctypes.c_int, c_u32, ctypes.c_size_t) else None
                     for a in args[2:]]
            for channel in (bank.channels, bank.channels + 7):
                print("CALL", name, channel, flush=True)
                self.cases += 1
                code = getattr(self.lib, name)(self.handle(bank), channel, *zeros)
                assert code == MI_EINVAL and name in self.message(), (name, channel, code, self.message())
            structs = [a for a in args[2:] if isinstance(getattr(a, "_type_", None), type) and issubclass(a._type_, ctypes.Structure)]
            if what in ("get_params", "get_latency", "get_patch") or (what in ("get_state", "set_state") and structs):
                print("CALL", name, "NULL", flush=True)
                self.cases += 1
                code = getattr(self.lib, name)(self.handle(bank), 0, *zeros)
                assert code == MI_EINVAL and name in self.message(), (name, code, self.message())
            elif what == "get_state":                               # every result pointer is optional
                print("CALL", name, "NULL", flush=True)
                self.cases += 1
                code = getattr(self.lib, name)(self.handle(bank), 0, *zeros)
                assert code == MI_OK, (name, code, self.message())


def child():
    sys.path.insert(0, ROOT)
    gpu = importlib.import_module("lsp-dsp-units_amd")
    capi = importlib.import_module("lsp-dsp-units_amd.capi")
    k = Checker(gpu, capi)
    for kind in BANKS:
        print("BANK", kind, flush=True)
        bank, single = make_bank(gpu, kind, 2), make_bank(gpu, kind, 1)
        k.sample_entries(kind, bank, single)
        k.channel_entries(kind, bank)
        bank.close(), single.close()
    print("CASES", k.cases, flush=True)


def test_sample_entries_and_channel_entries_refuse_what_their_sources_say(gpu):
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, timeout=300)
    lines = r.stdout.splitlines()
    last = [ln for ln in lines if ln.startswith("CALL")][-1:]
    assert r.returncode == 0, "last call: %s\n%s\n%s" % (last, r.stdout[-1500:], r.stderr[-3000:])
    assert [ln.split()[1] for ln in lines if ln.startswith("BANK")] == list(BANKS)
    cases = [int(ln.split()[1]) for ln in lines if ln.startswith("CASES")]
    print("cases:", cases)
    # 33 sample entries with at least 10 calls each, and the channel entries of eleven banks
    assert len(cases) == 1 and cases[0] >= 500, cases


if __name__ == "__main__":
    child()
