"""lsp::dspu::Randomizer, LCG and MLS restated in numpy (reference: src/main/util/Randomizer.cpp, src/main/noise/LCG.cpp, MLS.cpp), for
the recorded cases of tests/golden/noise_ref_vectors.npz and for the device tests.  No GPU.

Every float expression keeps the reference's types and order and rounds once per operation (the reference is recorded with
-ffp-contract=off).  The three transcendentals (expf, logf, cosf) are parameters: STAR is the float64 function of the float32
argument rounded once to float32 (S*), BELOW and ABOVE its float32 neighbours; a sample that one of them made obeys the interval
rule (inside()), every other sample and every state word is bit for bit.

The MLS register is also given in closed form over GF(2), as the device evaluates it: the update is s' = M s, sample i of a call is
the parity of rows[i] & s0 with rows[i] = row 0 of M^i, and the state after n samples is M^n s0, a product of the powers M^(2^p)."""
import numpy as np

f32, f64, u32, u64 = np.float32, np.float64, np.uint32, np.uint64

# ---- operations of a recorded case: (what, a, b, c) ------------------------------------------------------------------------
P_OVERWRITE, P_ADD, P_ADD_INPLACE, P_MUL, P_MUL_INPLACE = range(5)      # a: samples
INIT, SET_DISTRIBUTION, SET_AMPLITUDE, SET_OFFSET, POKE_LAST = 5, 6, 7, 8, 9    # INIT a: seed; POKE_LAST a: generator, b: vLast
SET_N_BITS, SET_STATE, SET_STATE_CURRENT = 10, 11, 12                   # SET_STATE a: low word, b: high word
PROCESS_OPS = (P_OVERWRITE, P_ADD, P_ADD_INPLACE, P_MUL, P_MUL_INPLACE)
KIND_LCG, KIND_MLS = 0, 1

LCG_UNIFORM, LCG_EXPONENTIAL, LCG_TRIANGULAR, LCG_GAUSSIAN = range(4)   # lcg_dist_t, LCG.h
DISTRIBUTIONS = ("uniform", "exponential", "triangular", "gaussian")
DRAWS = {LCG_UNIFORM: 1, LCG_EXPONENTIAL: 2, LCG_TRIANGULAR: 1, LCG_GAUSSIAN: 2}

# ---- Randomizer ---------------------------------------------------------------------------------------------------------------
MUL1 = (0x43ca16c1, 0x451222f3, 0x465e0183, 0x47f27263, 0x4212ffe9, 0x4433f6ad, 0x40f31425, 0x412318bb,
        0x48f39cbf, 0x49b18a45, 0x4d341bbf, 0x4e93a169, 0x4bacd5e5, 0x4c55e139, 0x4f11db4d, 0x4a901f8b)
MUL2 = (0x4c37c68f, 0x4d59b853, 0x4ef1d1e9, 0x4fe16c01, 0x40fc2271, 0x44e335c1, 0x450fc1bb, 0x48cc3d07,
        0x493737a9, 0x4182e63f, 0x42198197, 0x43fc5611, 0x4ac116eb, 0x4b0faf0d, 0x46777db9, 0x4730a64d)
ADDERS = (0x000551ff, 0x000633f5, 0x00011fcf, 0x00021b81, 0x00075af1, 0x00080be5, 0x000330a7, 0x00040d0b,
          0x000c2521, 0x000dd113, 0x0009eea5, 0x000ae007, 0x00092df5, 0x000b42bd, 0x000e1b15, 0x000f054d)
RAND_RANGE = 2.32830643654e-10                  # the literal of Randomizer.cpp:26, not 2^-32
RAND_LAMBDA = 2.718281828459045 * 1.4142135623730951        # M_E * M_SQRT2, a double product
EXP_LAMBDA = f32(46.722748)                     # expf(float(RAND_LAMBDA)), bits 0x423AE418
TWO_PI = 2.0 * 3.141592653589793                # 2.0f * M_PI, a double
HALF_SQRT2 = 1.4142135623730951 * 0.5           # M_SQRT2 * RAND_T, a double
M32 = 0xFFFFFFFF
UNSET = (1 << 64) - 1                           # nBufID of a Randomizer that was never init()ed: size_t(-1)


def step(last, mul1, mul2, add):
    """One generator, Randomizer.cpp:113, in uint32_t."""
    return (mul1 * last + (((mul2 * last) & M32) >> 16) + add) & M32


def seed_words(seed):
    """init(seed), :86-99: (vLast, vMul1, vMul2, vAdd) of the four generators."""
    seed &= M32
    out = []
    for i in range(4):
        reseed = ((seed << (i * 8)) | (seed >> ((4 - i) * 8))) & M32 if i else seed
        out.append((reseed ^ (seed >> 4), MUL1[(reseed >> 4) & 15], MUL2[(reseed >> 8) & 15], ADDERS[reseed & 15]))
    return out


def linear(raw):
    """generate_linear's return, :114: one float64 product rounded once to float32."""
    return (np.asarray(raw, u32).astype(f64) * f64(RAND_RANGE)).astype(f32)


class Transcendentals:
    """expf, logf and cosf of float32 arrays: S* moved by `exp`, `log`, `cos` float32 steps (-1, 0, 1)."""

    def __init__(self, exp=0, log=0, cos=0):
        self.moves = dict(exp=exp, log=log, cos=cos)

    def _of(self, name, fn, x):
        with np.errstate(all="ignore"):
            s = fn(np.asarray(x, f32).astype(f64)).astype(f32)
            m = self.moves[name]
            return s if m == 0 else np.nextafter(s, f32(np.inf if m > 0 else -np.inf))

    def exp(self, x): return self._of("exp", np.exp, x)
    def log(self, x): return self._of("log", np.log, x)
    def cos(self, x): return self._of("cos", np.cos, x)


STAR = Transcendentals()
EXP_NEIGHBOURS = (Transcendentals(exp=-1), Transcendentals(exp=1))
GAUSS_NEIGHBOURS = tuple(Transcendentals(log=a, cos=b) for a in (-1, 0, 1) for b in (-1, 0, 1) if (a, b) != (0, 0))


RND_LINEAR, RND_EXP, RND_TRIANGLE, RND_GAUSSIAN = range(4)     # random_function_t, Randomizer.h


def shaped(func, rv, rv2=None, fn=STAR):
    """Randomizer::random(func) from its draws as floats, :117-143 (rv2: the second draw of RND_GAUSSIAN)."""
    with np.errstate(all="ignore"):
        if func == RND_EXP:
            x = (f64(RAND_LAMBDA) * rv.astype(f64)).astype(f32)
            return ((fn.exp(x) - f32(1)) / (EXP_LAMBDA - f32(1))).astype(f32)
        if func == RND_TRIANGLE:
            low = (f64(HALF_SQRT2) * np.sqrt(rv).astype(f64)).astype(f32)
            high = f32(1) - np.sqrt(f32(4) - f32(2) * (f32(1) + rv)) * f32(0.5)
            return np.where(rv <= f32(0.5), low, high).astype(f32)
        if func == RND_GAUSSIAN:
            arg = (f64(TWO_PI) * rv2.astype(f64)).astype(f32)
            return (np.sqrt(f32(-2) * fn.log(rv)) * fn.cos(arg)).astype(f32)
        return rv


def samples(raw, dist, amplitude, offset, fn=STAR):
    """LCG::process_single over the draws `raw` (one per sample, or two for exponential and Gaussian), LCG.cpp:60-85."""
    A, off = f32(amplitude), f32(offset)
    raw = np.asarray(raw, u32)
    with np.errstate(all="ignore"):
        if dist == LCG_EXPONENTIAL:
            sign = np.where(linear(raw[0::2]) >= f32(0.5), f32(1), f32(-1)).astype(f32)
            return ((sign * A) * shaped(RND_EXP, linear(raw[1::2]), fn=fn) + off).astype(f32)
        if dist == LCG_TRIANGULAR:
            return (((f32(2) * A) * shaped(RND_TRIANGLE, linear(raw)) - f32(0.5)) + off).astype(f32)
        if dist == LCG_GAUSSIAN:
            return (A * shaped(RND_GAUSSIAN, linear(raw[0::2]), linear(raw[1::2]), fn) + off).astype(f32)
        return ((f32(2) * A) * (linear(raw) - f32(0.5)) + off).astype(f32)     # LCG_UNIFORM and the default: branch


class LCG:
    """One lsp::dspu::LCG: a Randomizer, a distribution, amplitude and offset."""

    def __init__(self):
        self.last, self.mul1, self.mul2, self.add = [0] * 4, [0] * 4, [0] * 4, [0] * 4
        self.buf_id = UNSET
        self.dist, self.amplitude, self.offset = LCG_UNIFORM, f32(1), f32(0)

    def init(self, seed):
        w = seed_words(int(seed))
        self.last, self.mul1, self.mul2, self.add = ([g[k] for g in w] for k in range(4))
        self.buf_id = 0

    def draws(self, n):
        assert self.buf_id != UNSET
        out = np.empty(n, u32)
        b = self.buf_id
        for i in range(n):
            self.last[b] = step(self.last[b], self.mul1[b], self.mul2[b], self.add[b])
            out[i] = self.last[b]
            b = (b + 1) & 3
        self.buf_id = b
        return out

    def process(self, n, fn=STAR):
        return samples(self.draws(DRAWS.get(self.dist, 1) * n), self.dist, self.amplitude, self.offset, fn)

    def transcendental(self):
        return self.dist in (LCG_EXPONENTIAL, LCG_GAUSSIAN)

    def words(self):
        """vLast[4], vMul1[4], vMul2[4], vAdd[4], nBufID."""
        return np.array(self.last + self.mul1 + self.mul2 + self.add + [self.buf_id], u64)


# ---- MLS ----------------------------------------------------------------------------------------------------------------------
MAX_BITS = 64
M64 = (1 << 64) - 1
# taps of a primitive polynomial per register width 1 .. 64 (Stahnke, Primitive Binary Polynomials, Math. Comp. 27 (1973))
TAPS = (1, 3, 3, 3, 5, 3, 3, 99, 17, 9, 5, 153, 27, 6147, 3, 45, 9, 129, 99, 9, 5, 3, 33, 27, 9, 387, 387, 9, 5, 98307, 9, 402653187,
        8193, 49155, 5, 2049, 5125, 99, 17, 2621445, 9, 12582915, 99, 201326595, 27, 3145731, 33, 402653187, 513, 201326595, 98307, 9,
        98307, 206158430211, 16777217, 6291459, 129, 524289, 6291459, 3, 98307, 216172782113783811, 3, 27)


def parity(v):
    return bin(v).count("1") & 1


class MLS:
    """One lsp::dspu::MLS with mls_t = uint64_t: the serial register."""

    def __init__(self):
        self.n_bits, self.feedback_bit, self.feedback_mask, self.active_mask, self.taps_mask = MAX_BITS, 0, 0, 0, 0
        self.output_mask, self.state, self.amplitude, self.offset, self.sync = 1, 0, f32(1), f32(0), True

    def set_n_bits(self, n):
        if n != self.n_bits:
            self.n_bits, self.sync = int(n), True

    def set_state(self, s):
        if s != self.state:
            self.state, self.sync = int(s) & M64, True

    def update_settings(self):
        if not self.sync:
            return
        self.n_bits = min(max(self.n_bits, 1), MAX_BITS)
        self.feedback_bit = self.n_bits - 1
        self.feedback_mask = 1 << self.feedback_bit
        self.active_mask = M64 if self.n_bits == MAX_BITS else ~(M64 << self.n_bits) & M64
        self.taps_mask = TAPS[self.n_bits - 1]
        self.state &= self.active_mask
        if self.state == 0:
            self.state |= self.active_mask
        self.sync = False

    def get_period(self):
        return M64 if self.n_bits == MAX_BITS else ((1 << self.n_bits) - 1) & M64

    def progress(self):
        self.update_settings()
        out = self.state & self.output_mask
        fb = parity(self.state & self.taps_mask)
        self.state >>= 1
        self.state = (self.state & ~self.feedback_mask) | (fb << self.feedback_bit)
        return out

    def levels(self):
        with np.errstate(all="ignore"):
            return f32(self.amplitude) + f32(self.offset), -f32(self.amplitude) + f32(self.offset)

    def process(self, n, fn=None):
        bits = np.array([self.progress() for _ in range(n)], bool)
        hi, lo = self.levels()
        return np.where(bits, hi, lo).astype(f32)

    def transcendental(self):
        return False

    def words(self):
        """nBits, nFeedbackBit, nFeedbackMask, nActiveMask, nTapsMask, nOutputMask, nState, bSync, get_period()."""
        return np.array([self.n_bits, self.feedback_bit, self.feedback_mask, self.active_mask, self.taps_mask, self.output_mask,
                         self.state, int(self.sync), self.get_period()], u64)


# the closed form: 64 x 64 matrices over GF(2) as 64 row words; (A v) bit k = parity(A[k] & v)
def transition(n_bits):
    """M of a register of n_bits: bit k of the next state is bit k + 1 of this one, the top bit is the parity of the taps."""
    return [1 << (k + 1) if k < n_bits - 1 else TAPS[n_bits - 1] if k == n_bits - 1 else 0 for k in range(64)]


def vecmat(v, B):
    """The row vector v times B: the xor of the rows of B that v selects."""
    out, k = 0, 0
    while v:
        if v & 1:
            out ^= B[k]
        v >>= 1
        k += 1
    return out


def matmul(A, B):
    return [vecmat(a, B) for a in A]


def matvec(A, v):
    return sum(parity(A[k] & v) << k for k in range(64))


def rows(n_bits, n):
    """rows[i] = row 0 of M^i, i < n: sample i of a call is parity(rows[i] & state0)."""
    M, out, r = transition(n_bits), [], 1
    for _ in range(n):
        out.append(r)
        r = vecmat(r, M)
    return out


def powers(n_bits, n):
    """M^(2^p), p < n."""
    out, P = [], transition(n_bits)
    for _ in range(n):
        out.append(P)
        P = matmul(P, P)
    return out


def advance(pw, state, count):
    """M^count state, from the powers of M."""
    p = 0
    while count:
        if count & 1:
            state = matvec(pw[p], state)
        count >>= 1
        p += 1
    return state


# ---- cases --------------------------------------------------------------------------------------------------------------------
def apply(unit, op):
    what, a, b = int(op[0]), op[1], op[2]
    if what == INIT: unit.init(int(a))
    elif what == SET_DISTRIBUTION: unit.dist = int(a)
    elif what == SET_AMPLITUDE: unit.amplitude = f32(a)
    elif what == SET_OFFSET: unit.offset = f32(a)
    elif what == POKE_LAST: unit.last[int(a)] = int(b)
    elif what == SET_N_BITS: unit.set_n_bits(int(a))
    elif what == SET_STATE: unit.set_state(int(a) | (int(b) << 32))
    elif what == SET_STATE_CURRENT: unit.set_state(unit.state)
    else: raise ValueError(what)


def combine(what, src, v):
    with np.errstate(all="ignore"):
        if what in (P_ADD, P_ADD_INPLACE):
            return (src + v).astype(f32)
        if what in (P_MUL, P_MUL_INPLACE):
            return (src * v).astype(f32)
        return v


def run_case(case, fn=STAR):
    """(out, which samples a transcendental made, the unit at the end) of a case dict with kind, ops [k, 4] and src [N]."""
    unit = LCG() if case["kind"] == KIND_LCG else MLS()
    src = np.asarray(case["src"], f32)
    out, trans, at = np.zeros(src.size, f32), np.zeros(src.size, bool), 0
    for op in case["ops"]:
        if int(op[0]) in PROCESS_OPS:
            n = int(op[1])
            trans[at:at + n] = unit.transcendental()
            out[at:at + n] = combine(int(op[0]), src[at:at + n], unit.process(n, fn))
            at += n
        else:
            apply(unit, op)
    assert at == src.size, (at, src.size)
    return out, trans, unit


def neighbours(case, trans):
    """The case's outputs with every neighbouring transcendental that the interval rule admits (none without such samples)."""
    if not trans.any():
        return []
    kinds = {int(op[1]) for op in case["ops"] if int(op[0]) == SET_DISTRIBUTION}
    fns = (EXP_NEIGHBOURS if LCG_EXPONENTIAL in kinds else ()) + (GAUSS_NEIGHBOURS if LCG_GAUSSIAN in kinds else ())
    return [run_case(case, fn)[0] for fn in fns]


def bits(a):
    return np.ascontiguousarray(a, f32).view(u32)


def same(got, want):
    """Bit for bit; where arithmetic made a NaN, a NaN."""
    got, want = np.asarray(got, f32), np.asarray(want, f32)
    return (bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))


def inside(got, star, others):
    """The interval rule: got lies in the closed interval that the restatement's outputs with S* and with the neighbouring
    transcendentals span.  NaN where any of them is NaN."""
    got = np.asarray(got, f32).astype(f64)
    all_ = np.stack([np.asarray(v, f32).astype(f64) for v in [star] + list(others)])
    nan = np.isnan(all_).any(axis=0)
    with np.errstate(invalid="ignore"):
        ok = (got >= np.where(nan, 0, all_).min(axis=0)) & (got <= np.where(nan, 0, all_).max(axis=0))
    return np.where(nan, np.isnan(got), ok)


def agree(got, want_bits, star, others, trans):
    """The comparison rule of a whole row: the indices that break it.  want_bits: what non-transcendental samples must equal."""
    bad = ~same(got, want_bits) & ~trans
    if trans.any():
        bad |= ~inside(got, star, others) & trans
    return np.nonzero(bad)[0]
