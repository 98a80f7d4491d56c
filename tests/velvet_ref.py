"""lsp::dspu::Velvet restated in numpy (reference: src/main/noise/Velvet.cpp) on noise_ref.py's Randomizer (its LCG class) and MLS,
for the recorded cases of tests/golden/velvet_ref_vectors.npz and for the device tests.  No GPU.

Every float expression keeps the reference's types and order and rounds once per operation (the reference is recorded with
-ffp-contract=off): the window index is size_t(float(scan) * W + rv * k) in float32, ARN's position is a serial float32 sum that is
truncated at every step, amplitude and offset are mul_k2 and add_k2 (two roundings).  A call with a source is cut into segments of
BUF_LIM_SIZE = 256, each of which restarts scan and idx; a later write to a sample replaces an earlier one.  Nothing transcendental
is involved: every sample and every state word is bit for bit.  A float-to-index conversion that is out of range (undefined in the
reference) saturates and ends the segment, as the device bank defines it."""
import numpy as np

import noise_ref as R

f32, f64, u32, u64 = np.float32, np.float64, np.uint32, np.uint64

# ---- operations of a recorded case: (what, a, b, c); 0 .. 4, SET_AMPLITUDE, SET_OFFSET and POKE_LAST are noise_ref's --------------
INIT = R.INIT                                               # a: randseed, b: mlsnbits, c: mlsseed (below 2^53)
SET_CORE, SET_TYPE, SET_WIDTH, SET_DELTA, SET_CRUSH, SET_CRUSH_PROB = 13, 14, 15, 16, 17, 18
INIT_SAME = 19                                              # a: randseed, b: mlsnbits; mlsseed is the current nState
P_ADD_NULL, P_MUL_NULL = 20, 21                             # a: samples; process_add / process_mul with src == NULL
PROCESS_OPS = R.PROCESS_OPS + (P_ADD_NULL, P_MUL_NULL)
CORE_MLS, CORE_LCG = 0, 1                                   # vn_core_t
OVN, OVNA, ARN, TRN = range(4)                              # vn_velvet_type_t
TYPES = ("OVN", "OVNA", "ARN", "TRN")
BUF_LIM_SIZE = 256
MAX_COUNT = 1 << 24
WORDS = 25                                                  # Randomizer: 17 (noise_ref.LCG.words); MLS: nBits .. nState, bSync


def roundf(x):
    """C's roundf: halves away from zero; the sign of a zero result is x's."""
    x = np.asarray(x, f32)
    return np.copysign(np.floor(np.abs(x.astype(f64)) + 0.5), x).astype(f32)


def to_index(x):
    """size_t(x) where it is defined; out of range and NaN: None (the segment ends)."""
    x = float(x)
    return int(x) if 0.0 <= x < 4294967296.0 else None


class Velvet:
    """One lsp::dspu::Velvet."""

    def __init__(self):
        self.rand, self.mls = R.LCG(), R.MLS()
        self.core, self.type, self.crush, self.prob = CORE_MLS, OVN, False, f32(0.5)
        self.width, self.delta, self.amplitude, self.offset = f32(10), f32(0.5), f32(1), f32(0)
        self.drawn = []                                     # (role, raw draw) of everything drawn, for tests: 'p'osition, 's'pike, 'c'rush, 't'rn

    # ---- setters, Velvet.cpp:71-130
    def init(self, randseed, n_bits, mls_seed):
        self.rand.init(randseed)
        self.mls.amplitude, self.mls.offset = f32(1), f32(0)
        self.mls.set_n_bits(int(n_bits) & 0xFF)
        self.mls.set_state(int(mls_seed))

    def set_width(self, w):
        w = f32(w)
        self.width = w if w > f32(2) else f32(2)            # lsp_max(width, MIN_WINDOW_WIDTH)

    @staticmethod
    def limit01(v):
        v = f32(v)
        return f32(0) if v < 0 else f32(1) if v > 1 else v

    def set_delta(self, d): self.delta = self.limit01(d)
    def set_crush_prob(self, p): self.prob = self.limit01(p)

    # ---- draws
    def rv(self, role):
        r = self.rand
        assert r.buf_id != R.UNSET
        b = r.buf_id
        r.last[b] = R.step(r.last[b], r.mul1[b], r.mul2[b], r.add[b])
        r.buf_id = (b + 1) & 3
        self.drawn.append((role, r.last[b]))
        return R.linear([r.last[b]])[0]

    def spike(self):
        if self.crush:                                      # get_crushed_spike(), :150-153
            return f32(1) if self.rv("c") > self.prob else f32(-1)
        if self.core == CORE_MLS:                           # get_spike(), :137-148: process_single() at amplitude 1 and offset 0
            hi, lo = self.mls.levels()
            return hi if self.mls.progress() else lo
        return f32(f32(2) * roundf(self.rv("s")) - f32(1))

    def segment(self, n):
        """do_process(dst, n), :155-258."""
        W, one = self.width, f32(1)
        dst = np.zeros(n, f32)
        with np.errstate(all="ignore"):
            if self.type in (OVN, OVNA):
                k = f32(W - one) if self.type == OVN else W
                scan = 0
                while True:
                    idx = to_index(f32(f32(scan) * W) + f32(self.rv("p") * k))
                    if idx is None or idx >= n:
                        break
                    dst[idx] = self.spike()
                    scan += 1
            elif self.type == ARN:
                k = f32(f32(f32(2) * self.delta) * f32(W - one))
                b = f32(f32(one - self.delta) * f32(W - one))
                idx = 0
                while True:
                    idx = to_index(f32(f32(idx) + f32(f32(one + b) + f32(k * self.rv("p")))))
                    if idx is None or idx >= n:
                        break
                    dst[idx] = self.spike()
            elif self.type == TRN:
                k = f32(W / f32(W - one))
                rv = np.array([self.rv("t") for _ in range(n)], f32)
                dst = roundf(k * (rv - f32(0.5)))
                if self.crush:
                    rv = np.array([self.rv("c") for _ in range(n)], f32)
                    dst = (np.where(rv > self.prob, f32(-1), f32(1)).astype(f32) * np.abs(dst)).astype(f32)
        return dst

    def scaled(self, n):
        with np.errstate(all="ignore"):
            return ((self.segment(n) * self.amplitude).astype(f32) + self.offset).astype(f32)

    def process(self, what, src, n):
        """process_overwrite / process_add / process_mul, :260-319: what is one of PROCESS_OPS, src the n source samples (or None)."""
        if what == R.P_OVERWRITE or what == P_ADD_NULL:
            return self.scaled(n)
        if what == P_MUL_NULL:
            return np.zeros(n, f32)
        out = np.empty(n, f32)
        for at in range(0, n, BUF_LIM_SIZE):
            k = min(BUF_LIM_SIZE, n - at)
            out[at:at + k] = R.combine(what, src[at:at + k], self.scaled(k))
        return out

    def words(self):
        """The Randomizer's 17 words, then nBits, nFeedbackBit, nFeedbackMask, nActiveMask, nTapsMask, nOutputMask, nState, bSync."""
        return np.concatenate([self.rand.words(), self.mls.words()[:8]])


def apply(unit, op):
    what, a, b, c = int(op[0]), op[1], op[2], op[3]
    if what == INIT: unit.init(int(a), int(b), int(c))
    elif what == INIT_SAME: unit.init(int(a), int(b), unit.mls.state)
    elif what == R.SET_AMPLITUDE: unit.amplitude = f32(a)
    elif what == R.SET_OFFSET: unit.offset = f32(a)
    elif what == R.POKE_LAST: unit.rand.last[int(a)] = int(b)
    elif what == SET_CORE: unit.core = int(a)
    elif what == SET_TYPE: unit.type = int(a)
    elif what == SET_WIDTH: unit.set_width(a)
    elif what == SET_DELTA: unit.set_delta(a)
    elif what == SET_CRUSH: unit.crush = bool(a)
    elif what == SET_CRUSH_PROB: unit.set_crush_prob(a)
    else: raise ValueError(what)


def run_case(case, unit=None):
    """(out, the unit at the end) of a case dict with ops [k, 4] and src [N]; samples that no operation fills stay 0."""
    unit = unit or Velvet()
    src = np.asarray(case["src"], f32)
    out, at = np.zeros(src.size, f32), 0
    for op in case["ops"]:
        if int(op[0]) in PROCESS_OPS:
            n = int(op[1])
            out[at:at + n] = unit.process(int(op[0]), src[at:at + n], n)
            at += n
        else:
            apply(unit, op)
    assert at <= src.size, (at, src.size)
    return out, unit
