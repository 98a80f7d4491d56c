"""lsp::dspu::Bypass and lsp::dspu::Crossfade restated in numpy float32, from what the classes do: the gain runs as the serial
float32 sum g += delta, one step per sample (so the gains of a ramp are formed one by one); the mix under it and the tail after
it are element-wise and written as array expressions, every product and sum rounded on its own.

Both classes return (out, copied): copied marks the samples that are a plain copy of an input (or zeros), where even a NaN's
payload has to come through; everywhere else a NaN went through arithmetic and only its NaN-ness is the reference's.

replay() runs an operation list of tests/golden/bypass_crossfade_ref_vectors.npz on anything with these classes' methods."""
import numpy as np

f32 = np.float32
S_ON, S_ACTIVE, S_OFF = 0, 1, 2
PROCESS, PROCESS_WET, PROCESS_DRYWET = range(3)
BYPASS, CROSSFADE = range(2)
# the operations of a recorded case: (what, argument, flags, float bits, float bits)
B_INIT, B_SET_BYPASS, B_SET_FIELDS, B_PROCESS, B_PROCESS_WET, B_PROCESS_DRYWET = range(6)
X_INIT, X_TOGGLE, X_RESET, X_PROCESS = range(4)
HAS_A, HAS_B = 1, 2                 # flags of a process operation: dry | fade_out is there, wet | fade_in is there


def bits(v):
    return int(f32(v).view(np.uint32))


def flt(u):
    return np.uint32(u).view(f32)


def ramp_length(sample_rate, time):
    """float(sample_rate) * time in float32, anything below 1 taken up to 1; None where the banks refuse (NaN, 2^32 and more)."""
    with np.errstate(all="ignore"):
        length = f32(sample_rate) * f32(time)
    if np.isnan(length) or length >= f32(4294967296.0):
        return None
    return f32(1.0) if length < f32(1.0) else length


def _gains(gain, delta, limit, goes_on):
    """The gains before each step of a ramp of at most `limit` samples, and the gain after the last step taken."""
    g, out = f32(gain), []
    with np.errstate(all="ignore"):
        while len(out) < limit and goes_on(g, len(out)):
            out.append(g)
            g = f32(g + delta)
    return np.array(out, f32), g


class Bypass:
    def __init__(self):
        self.state, self.delta, self.gain = S_OFF, f32(0.0), f32(0.0)

    def init(self, sample_rate, time):
        length = ramp_length(sample_rate, time)
        assert length is not None
        self.state, self.delta, self.gain = S_OFF, f32(1.0) / length, f32(1.0)

    def bypassing(self):
        return self.state == S_ON or (self.state == S_ACTIVE and bool(self.delta < 0))

    def set_bypass(self, bypass):
        if self.state not in (S_ON, S_ACTIVE, S_OFF) or bool(bypass) == self.bypassing():
            return False
        self.state, self.delta = S_ACTIVE, f32(-self.delta)
        return True

    def set_fields(self, state, delta, gain):
        self.state, self.delta, self.gain = int(state), f32(delta), f32(gain)

    def fields(self):
        return self.state, bits(self.delta), bits(self.gain)

    def process(self, dry, wet, variant=PROCESS, wet_gain=1.0, dry_gain=1.0):
        wet = np.asarray(wet, f32)
        count = wet.size
        out, copied = np.zeros(count, f32), np.zeros(count, bool)
        if count == 0:
            return out, copied
        wg, dg = f32(wet_gain), f32(dry_gain)
        up = bool(self.delta > 0)                       # anything else goes down: 0, -0 and NaN too
        g, after = _gains(self.gain, self.delta, count, (lambda v, i: v < 1) if up else (lambda v, i: v > 0))
        n = g.size
        self.gain = after
        with np.errstate(all="ignore"):
            w = wet[:n]
            if dry is None:
                out[:n] = w * g if variant == PROCESS else (w * g) * wg
            else:
                d = np.asarray(dry, f32)[:n]
                if variant == PROCESS:
                    out[:n] = d + (w - d) * g
                elif variant == PROCESS_WET:
                    out[:n] = d + (w * wg - d) * g
                else:
                    out[:n] = d + (w * wg - d * dg) * g
            if n == count:
                return out, copied                      # the ramp used up the block: no clamp before the next call
            if up:
                self.gain, self.state = f32(1.0), S_OFF
                if variant == PROCESS:
                    out[n:], copied[n:] = wet[n:], True
                else:
                    out[n:] = wet[n:] * wg
            else:
                self.gain, self.state = f32(0.0), S_ON
                if dry is None:
                    copied[n:] = True                   # zeros
                elif variant == PROCESS_DRYWET:
                    out[n:] = np.asarray(dry, f32)[n:] * dg
                else:
                    out[n:], copied[n:] = np.asarray(dry, f32)[n:], True
        return out, copied


class Crossfade:
    def __init__(self):
        self.samples, self.counter, self.delta, self.gain = 0, 0, f32(0.0), f32(1.0)

    def init(self, sample_rate, time):
        length = ramp_length(sample_rate, time)
        assert length is not None
        self.samples = int(length)

    def toggle(self):
        if self.counter > 0:
            return False
        with np.errstate(all="ignore"):
            self.delta = f32(1.0) / f32(self.samples)
        self.gain, self.counter = f32(0.0), self.samples
        return True

    def reset(self):
        self.counter, self.delta, self.gain = 0, f32(0.0), f32(0.0)

    def set_fields(self, counter, delta, gain):
        self.counter, self.delta, self.gain = int(counter), f32(delta), f32(gain)

    def fields(self):
        return self.counter, bits(self.delta), bits(self.gain)

    def process(self, fade_out, fade_in, count):
        out, copied = np.zeros(count, f32), np.zeros(count, bool)
        if count == 0:
            return out, copied
        if fade_out is None and fade_in is None:
            n = min(self.counter, count)
            self.counter -= n
            with np.errstate(all="ignore"):
                self.gain = f32(self.gain + f32(self.delta * f32(n)))
            copied[:] = True
            return out, copied
        g, after = _gains(self.gain, self.delta, count, lambda v, i: i < self.counter)
        n = g.size
        self.gain, self.counter = after, self.counter - n
        fo = None if fade_out is None else np.asarray(fade_out, f32)
        fi = None if fade_in is None else np.asarray(fade_in, f32)
        with np.errstate(all="ignore"):
            if fo is None:
                out[:n] = fi[:n] * g
            elif fi is None:
                out[:n] = fo[:n] * (f32(1.0) - g)
            else:
                out[:n] = fo[:n] + (fi[:n] - fo[:n]) * g
        src = fi if bool(self.gain > 0) else fo
        if src is not None:
            out[n:] = src[n:]
        copied[n:] = True
        return out, copied


def same(got, want, copied):
    """Bit for bit; where arithmetic made a NaN, a NaN."""
    got, want = np.asarray(got, f32), np.asarray(want, f32)
    equal = got.view(np.uint32) == want.view(np.uint32)
    return bool(np.all(equal | (~np.asarray(copied, bool) & np.isnan(got) & np.isnan(want))))


def replay(case, x, unit):
    """The operations of a recorded case on `unit` (a Bypass or a Crossfade of this module, or anything with their methods, whose
    process returns the samples, or the samples and `copied`): (out, copied, answers)."""
    n = x.shape[1]
    a, b = x[case["signal"][0]], x[case["signal"][1]]
    out, copied, answers, at = np.zeros(n, f32), np.zeros(n, bool), [], 0
    for what, arg, flags, u, v in case["ops"]:
        what, arg, answer = int(what), int(arg), 0
        ra = a[at:at + arg] if flags & HAS_A else None
        rb = b[at:at + arg] if flags & HAS_B else None
        r = None
        if case["kind"] == BYPASS:
            if what == B_INIT:
                unit.init(arg, flt(u))
            elif what == B_SET_BYPASS:
                answer = int(unit.set_bypass(bool(arg)))
            elif what == B_SET_FIELDS:
                unit.set_fields(flags, flt(u), flt(v))
            elif what == B_PROCESS:
                r = unit.process(ra, rb)
            elif what == B_PROCESS_WET:
                r = unit.process(ra, rb, PROCESS_WET, flt(u))
            else:
                assert what == B_PROCESS_DRYWET
                r = unit.process(ra, rb, PROCESS_DRYWET, flt(u), flt(v))
        else:
            if what == X_INIT:
                unit.init(arg, flt(u))
            elif what == X_TOGGLE:
                answer = int(unit.toggle())
            elif what == X_RESET:
                unit.reset()
            else:
                assert what == X_PROCESS
                r = unit.process(ra, rb, arg)
        if r is not None:
            o, c = r if isinstance(r, tuple) else (r, np.zeros(arg, bool))
            out[at:at + arg], copied[at:at + arg] = o, c
            at += arg
        answers.append(answer)
    assert at == n, (case["name"], at)
    return out, copied, np.array(answers, np.uint32)
