"""lsp::dspu::Oscillator (src/main/util/Oscillator.cpp, include/.../util/Oscillator.h) restated in numpy float32: every product
and every sum is rounded on its own, the settings words keep the reference's mix of double and float.  The phase accumulator is
advanced serially, one step per sample, as the reference's loops do; the value of a sample depends on its phase alone.
tests/test_oscillator_host.py pins this to the recorded reference cases; the GPU tests hold the bank to it.

The sine is a parameter: sine(x, cosine) takes the float32 arguments and returns float32 values.  The default is S*, the float64
sine of the float32 argument rounded once; the reference's own bits are its C library's sinf, within one ulp of S*.  inside()
is the interval rule that goes with it.

Where the reference has no defined behaviour this restatement has the bank's:
  * a double or float that does not fit a uint32_t converts through int64_t, the low 32 bits kept, NaN and what does not fit
    int64_t as 0 (the reference's x86-64 build does that);
  * a trapezoid sample takes the first branch, in source order, that holds (:430-443 can write twice);
  * get_periods (:635-689) as the C++ class defines it: a read position outside the buffer reads 0.0f (the reference's goes
    negative at the first refill and reads in front of its buffer), and a period that is not positive and finite writes nothing."""
import math

import numpy as np

f32, f64, u32 = np.float32, np.float64, np.uint32

(FG_SINE, FG_COSINE, FG_SQUARED_SINE, FG_SQUARED_COSINE, FG_RECTANGULAR, FG_SAWTOOTH, FG_TRAPEZOID, FG_PULSETRAIN, FG_PARABOLIC,
 FG_BL_RECTANGULAR, FG_BL_SAWTOOTH, FG_BL_TRAPEZOID, FG_BL_PULSETRAIN, FG_BL_PARABOLIC) = range(14)
FUNCTIONS = ("sine", "cosine", "squared sine", "squared cosine", "rectangular", "sawtooth", "trapezoid", "pulsetrain", "parabolic",
             "BL rectangular", "BL sawtooth", "BL trapezoid", "BL pulsetrain", "BL parabolic")
SINUSOIDS = (FG_SINE, FG_COSINE, FG_SQUARED_SINE, FG_SQUARED_COSINE)
DC_WAVEDC, DC_ZERO = 0, 1
OP_OVERWRITE, OP_ADD, OP_MUL = 0, 1, 2
PROCESS_BUF_LIMIT_SIZE = 12 * 1024                          # :26
M_1_PI = 0.31830988618379067154
M_SQRT1_2 = 0.70710678118654752440
UNSET_RATE = (1 << 64) - 1                                  # size_t(-1), :52

# the operations of a recorded case: rows of (what, a, b, c)
(P_OVERWRITE, P_ADD, P_ADD_NULL, P_ADD_INPLACE, P_MUL, P_MUL_NULL, P_MUL_INPLACE, SET_FUNCTION, SET_FREQUENCY, SET_SAMPLE_RATE,
 SET_PHASE, SET_BITS, SET_DC_OFFSET, SET_DC_REFERENCE, SET_AMPLITUDE, SET_DUTY, SET_WIDTH, SET_TRAPEZOID, SET_PULSETRAIN,
 SET_PARABOLIC_WIDTH, SET_SQUARED_INVERSION, SET_PARABOLIC_INVERSION, SET_OVER_MODE, RESET_PHASE, UPDATE, GET_PERIODS) = range(26)
PROCESS_OPS = (P_OVERWRITE, P_ADD, P_ADD_NULL, P_ADD_INPLACE, P_MUL, P_MUL_NULL, P_MUL_INPLACE)
# the words a recorded case ends with, in this order (floats as their bits)
WORDS = ("nPhaseAcc", "nPhaseAccMask", "fAcc2Phase", "nFreqCtrlWord", "nInitPhaseWord", "fReferencedDC", "sq.fAmplitude", "sq.fWaveDC",
         "rect.nDutyWord", "rect.fWaveDC", "rect.fBLPeakAtten", "saw.nWidthWord", "saw.fCoeffs0", "saw.fCoeffs1", "saw.fCoeffs2",
         "saw.fCoeffs3", "saw.fBLPeakAtten", "trap.nPoints0", "trap.nPoints1", "trap.nPoints2", "trap.nPoints3", "trap.fCoeffs0",
         "trap.fCoeffs1", "trap.fCoeffs2", "trap.fCoeffs3", "trap.fBLPeakAtten", "pulse.nTrainPoints0", "pulse.nTrainPoints1",
         "pulse.nTrainPoints2", "pulse.fWaveDC", "pulse.fBLPeakAtten", "par.fAmplitude", "par.nWidthWord", "par.fWaveDC",
         "par.fBLPeakAtten", "nOversampling", "nFreqCtrlWord_Over")


def to_u32(x):
    """double or float -> uint32_t as the bank defines it: through int64_t, the low 32 bits; NaN and beyond int64_t: 0."""
    x = float(x)
    if math.isnan(x) or abs(x) >= 9223372036854775808.0:
        return 0
    return int(x) & 0xFFFFFFFF


def sine_star(x, cosine):
    """S*: the float64 sine or cosine of the float32 argument, rounded once."""
    x = np.asarray(x, f32).astype(f64)
    return (np.cos(x) if cosine else np.sin(x)).astype(f32)


def sine_next(x, cosine):
    return np.nextafter(sine_star(x, cosine), f32(np.inf))


def sine_prev(x, cosine):
    return np.nextafter(sine_star(x, cosine), f32(-np.inf))


def serial_phases(p0, w, mask, n):
    """nPhaseAcc = (nPhaseAcc + w) & mask, n times: the phases of the n samples and the phase after them."""
    out, p = np.empty(n, u32), int(p0)
    for i in range(n):
        out[i] = p
        p = (p + w) & mask
    return out, p


def closed_phases(p0, w, mask, n):
    """(p0 + i w) & mask in uint32_t arithmetic."""
    with np.errstate(over="ignore"):
        return (u32(p0) + np.arange(n, dtype=u32) * u32(w)) & u32(mask)


class Oscillator:
    def __init__(self, sine=sine_star, oversampler=None):
        """oversampler(): a fresh tests/oversampler_ref.OversamplerRef of one channel (the BL functions need two)."""
        self.sine = sine
        self.function, self.amplitude, self.frequency, self.dc_offset = FG_SINE, f32(1), f32(0), f32(0)     # :44-50
        self.dc_reference, self.referenced_dc, self.init_phase = DC_WAVEDC, f32(0), f32(0)
        self.sample_rate, self.acc, self.bits, self.max_bits, self.mask, self.acc2phase = UNSET_RATE, 0, 32, 32, 0, f32(0)
        self.freq_word, self.init_word = 0, 0
        self.sq_invert, self.sq_amplitude, self.sq_wave_dc = False, f32(0), f32(0)
        self.duty, self.duty_word, self.rect_wave_dc, self.rect_atten = f32(0.5), 0, f32(0), f32(0)
        self.width, self.width_word, self.saw_coeffs, self.saw_atten = f32(1), 0, [f32(0)] * 4, f32(0)
        self.raise_ratio, self.fall_ratio, self.points, self.trap_coeffs, self.trap_atten = f32(0.25), f32(0.25), [0] * 4, [f32(0)] * 4, f32(0)
        self.pos_ratio, self.neg_ratio, self.train, self.pulse_wave_dc, self.pulse_atten = f32(0), f32(0), [0] * 3, f32(0), f32(0)
        self.par_invert, self.par_amplitude, self.par_width, self.par_word, self.par_wave_dc, self.par_atten = False, f32(1), f32(0), 0, f32(0), f32(0)
        self.oversampling, self.over_mode, self.freq_word_over, self.sync = 0, 0, 0, True
        self.over = oversampler() if oversampler else None
        self.over_periods = oversampler() if oversampler else None
        self.double_writes = 0
        self.synth = np.zeros(PROCESS_BUF_LIMIT_SIZE, f32)              # vSynthBuffer: get_periods reads what is left in it

    # -- setters, Oscillator.h:207-257 and Oscillator.cpp:749-890 ------------------------------------------------------------
    def set_phase_accumulator_bits(self, bits):             # .h:207-215
        if self.bits == bits or bits > self.max_bits:
            return
        self.bits, self.acc, self.sync = bits, 0, True

    def set_sample_rate(self, sr):                          # .h:221-229
        if self.sample_rate == sr:
            return
        self.sample_rate, self.acc, self.sync = sr, 0, True

    def reset_phase_accumulator(self):                      # .h:234
        self.acc = 0

    def set_function(self, function):                       # .h:240-244
        self.function, self.sync = function, True

    def set_frequency(self, frequency):                     # .h:250-257
        if self.frequency == f32(frequency):
            return
        self.frequency, self.sync = f32(frequency), True

    def set_phase(self, phase):                             # :749-757
        if self.init_phase == f32(phase):
            return
        self.init_phase, self.sync = f32(phase), True

    def set_dc_offset(self, dc):                            # :765-771: no bSync
        if self.dc_offset != f32(dc):                       # -0.0f == 0.0f: not stored
            self.dc_offset = f32(dc)

    def set_dc_reference(self, ref):                        # :773-777
        self.dc_reference, self.sync = ref, True

    def set_squared_sinusoid_inversion(self, invert):       # :779-786
        if self.sq_invert != bool(invert):
            self.sq_invert, self.sync = bool(invert), True

    def set_parabolic_inversion(self, invert):              # :788-795
        if self.par_invert != bool(invert):
            self.par_invert, self.sync = bool(invert), True

    def set_duty_ratio(self, duty):                         # :797-804
        duty = f32(duty)
        if self.duty == duty or duty < 0 or duty > 1 or np.isnan(duty):
            return                                          # NaN: both comparisons of :799 are false and it is stored
        self.duty, self.sync = duty, True

    def set_width(self, width):                             # :806-817
        width = f32(0) if f32(width) < 0 else f32(1) if f32(width) > 1 else f32(width)
        if self.width != width:
            self.width, self.sync = width, True

    def set_trapezoid_ratios(self, rise, fall):             # :819-838
        rise = f32(0) if f32(rise) < 0 else f32(1) if f32(rise) > 1 else f32(rise)
        fall = f32(fall)
        if fall < 0:
            fall = f32(0)
        elif fall > f32(1) - rise:
            fall = f32(1) - rise
        if rise == self.raise_ratio and fall == self.fall_ratio:
            return
        self.raise_ratio, self.fall_ratio, self.sync = rise, fall, True

    def set_pulsetrain_ratios(self, pos, neg):              # :840-858
        pos = f32(0) if f32(pos) < 0 else f32(1) if f32(pos) > 1 else f32(pos)
        neg = f32(0) if f32(neg) < 0 else f32(1) if f32(neg) > 1 else f32(neg)
        if pos == self.pos_ratio and neg == self.neg_ratio:
            return
        self.pos_ratio, self.neg_ratio, self.sync = pos, neg, True

    def set_parabolic_width(self, width):                   # :860-872
        width = f32(0) if f32(width) < 0 else f32(1) if f32(width) > 1 else f32(width)
        if self.par_width != width:
            self.par_width, self.sync = width, True

    def set_oversampler_mode(self, mode):                   # :874-881
        if mode != self.over_mode:
            self.over_mode, self.sync = mode, True

    def set_amplitude(self, amplitude):                     # :883-890
        if self.amplitude != f32(amplitude):
            self.amplitude, self.sync = f32(amplitude), True

    def get_exact_frequency(self):                          # .h:262-265: float(size_t product) * (1.0f / (float(mask) + 1.0f))
        with np.errstate(all="ignore"):
            return f32(f32((self.sample_rate * self.freq_word) & ((1 << 64) - 1)) * f32(f32(1) / f32(f32(u32(self.mask)) + f32(1))))

    def get_exact_phase(self):                              # :759-763, in double; round() is half away from zero
        x = self.mask + 1.0
        v = x * float(self.init_phase) * float(f32(0.5)) * M_1_PI
        r = math.floor(abs(v) + 0.5) * (1 if v >= 0 else -1) if math.isfinite(v) else v
        return f32(r * (2.0 * math.pi / x))

    # -- update_settings, :151-357 ---------------------------------------------------------------------------------------------
    def update_settings(self):
        if not self.sync:                                                               # :153
            return
        self.mask = 0xFFFFFFFF if self.bits == self.max_bits else (1 << self.bits) - 1  # :156-159
        m1 = self.mask + 1.0                                                            # double
        self.acc2phase = f32(2.0 * math.pi * (1.0 / m1))                                # :161
        with np.errstate(all="ignore"):
            self.freq_word = to_u32(f64(m1 * float(self.frequency)) / f64(float(self.sample_rate)))    # :162
        self.acc = (self.acc - self.init_word) & self.mask                              # :164
        ph = float(self.init_phase)
        t = ph * 0.5 * M_1_PI
        fl = math.floor(t) if math.isfinite(t) else t
        self.init_word = to_u32(m1 * 0.5 * M_1_PI * (ph - 2.0 * math.pi * fl))          # :165
        self.acc = (self.acc + self.init_word) & self.mask                              # :166

        fm1 = f32(f32(u32(self.mask)) + f32(1))                                         # nPhaseAccMask + 1.0f: float 2^32 for 32 bits
        A, fn = self.amplitude, self.function
        with np.errstate(all="ignore"):
            if fn in (FG_SINE, FG_COSINE):                                              # :170-173
                self.referenced_dc = self.dc_offset
            elif fn in (FG_SQUARED_SINE, FG_SQUARED_COSINE):                            # :174-195
                self.sq_amplitude = f32(-A) if self.sq_invert else A
                self.sq_wave_dc = f32(f32(0.5) * self.sq_amplitude)
                self.referenced_dc = f32(self.dc_offset - self.sq_wave_dc) if self.dc_reference == DC_ZERO else self.dc_offset
            elif fn in (FG_RECTANGULAR, FG_BL_RECTANGULAR):                             # :197-220
                self.duty_word = self.mask if self.duty == 1 else to_u32(f32(self.duty * fm1))
                self.rect_wave_dc = f32(A * f32(f32(f32(2) * self.duty) - f32(1)))
                self.referenced_dc = f32(self.dc_offset - self.rect_wave_dc) if self.dc_reference == DC_ZERO else self.dc_offset
                self.rect_atten = f32(0.6)
            elif fn in (FG_SAWTOOTH, FG_BL_SAWTOOTH):                                   # :222-247
                self.width_word = self.mask if self.width == 1 else to_u32(f32(self.width * fm1))
                ww = f32(u32(self.width_word))
                c = self.saw_coeffs
                c[0] = f32(f32(f32(2) * A) / ww)
                c[1] = f32(-A)
                c[2] = f32(f32(f32(-2) * A) / f32(fm1 - ww))
                c[3] = f32(f32(A * f32(fm1 + ww)) / f32(fm1 - ww))
                self.referenced_dc = self.dc_offset
                if self.width > f32(0.60):
                    self.saw_atten = f32(f32(f32(0.64) / f32(0.4)) - self.width)
                elif self.width < f32(0.40):
                    self.saw_atten = f32(self.width + f32(0.6))
                else:
                    self.saw_atten = f32(1)
            elif fn in (FG_TRAPEZOID, FG_BL_TRAPEZOID):                                 # :249-279
                p, r, fa = self.points, self.raise_ratio, self.fall_ratio
                p[0] = to_u32(f32(f32(r * f32(0.5)) * fm1))
                p[1] = to_u32(f32(f32(f32(f32(1) - fa) * f32(0.5)) * fm1))
                p[2] = to_u32(f32(f32(f32(f32(1) + fa) * f32(0.5)) * fm1)) if fa < 1 else self.mask
                p[3] = to_u32(f32(f32(f32(f32(2) - r) * f32(0.5)) * fm1)) if r > 0 else self.mask
                c = self.trap_coeffs
                c[0] = f32(A / f32(u32(p[0])))
                c[1] = f32(f32(f32(-2) * A) / f32(u32((p[2] - p[1]) & 0xFFFFFFFF)))
                c[2] = f32(A / fa)
                c[3] = f32(f32(f32(-2) * A) / r)
                self.referenced_dc = self.dc_offset
                low = r if r < fa else fa
                self.trap_atten = f32(low + f32(0.6)) if low < f32(0.4) else f32(1)
            elif fn in (FG_PULSETRAIN, FG_BL_PULSETRAIN):                               # :281-308
                t = self.train
                t[0] = to_u32(f32(f32(self.pos_ratio * f32(0.5)) * fm1))
                t[1] = to_u32(f32(f32(0.5) * fm1))
                t[2] = self.mask if self.neg_ratio == 1 else to_u32(f32(f32(f32(f32(1) + self.neg_ratio) * f32(0.5)) * fm1))
                self.pulse_wave_dc = f32(f32(f32(0.5) * A) * f32(self.pos_ratio - self.neg_ratio))
                self.referenced_dc = f32(self.dc_offset - self.pulse_wave_dc) if self.dc_reference == DC_ZERO else self.dc_offset
                high = self.neg_ratio if self.neg_ratio > self.pos_ratio else self.pos_ratio
                self.pulse_atten = f32(0.6) if high > f32(0.5) else f32(M_SQRT1_2)      # a double stored to a float
            elif fn in (FG_PARABOLIC, FG_BL_PARABOLIC):                                 # :310-338
                self.par_amplitude = f32(-A) if self.par_invert else A
                self.par_word = self.mask if self.par_width == 1 else to_u32(f32(self.par_width * fm1))
                self.par_wave_dc = f32(f32(f32(f32(2) * self.par_amplitude) * self.par_width) / f32(3))
                self.referenced_dc = f32(self.dc_offset - self.par_wave_dc) if self.dc_reference == DC_ZERO else self.dc_offset
                self.par_atten = f32(1)
        for o in (self.over, self.over_periods):                                        # :343-351
            if o is not None:
                o.set_sample_rate(self.sample_rate)
                o.set_mode(self.over_mode)
                if o.modified():
                    o.update_settings()
        self.oversampling = times_of(self.over_mode)                                    # :353
        self.freq_word_over = self.freq_word // self.oversampling                       # :354
        self.sync = False

    # -- do_process, :359-633 --------------------------------------------------------------------------------------------------
    def wave(self, ph, sine=None):
        """The value of the function at each phase of ph (uint32): one branch of do_process without its accumulator.  The BL
        branches give the oversampled row that goes to the downsampler."""
        sine = sine or self.sine
        ph = np.asarray(ph, u32)
        pf = ph.astype(f32)                                 # round to nearest even
        A, dc, fn = self.amplitude, self.referenced_dc, self.function
        with np.errstate(all="ignore"):
            if fn in (FG_SINE, FG_COSINE):                  # :372, :380
                return A * sine(self.acc2phase * pf, fn == FG_COSINE) + dc
            if fn in (FG_SQUARED_SINE, FG_SQUARED_COSINE):  # :390-391, :401-402
                x = sine(f32(f32(0.5) * self.acc2phase) * pf, fn == FG_SQUARED_COSINE)
                return self.sq_amplitude * x * x + dc
            if fn in (FG_RECTANGULAR, FG_BL_RECTANGULAR):   # :410, :490
                v = np.where(ph < self.duty_word, A, f32(-A)).astype(f32) + dc
                return self.rect_atten * v if fn == FG_BL_RECTANGULAR else v
            if fn in (FG_SAWTOOTH, FG_BL_SAWTOOTH):         # :418-421, :514-517
                c = self.saw_coeffs
                v = np.where(ph < self.width_word, c[0] * pf + c[1] + dc, c[2] * pf + c[3] + dc).astype(f32)
                return self.saw_atten * v if fn == FG_BL_SAWTOOTH else v
            if fn in (FG_TRAPEZOID, FG_BL_TRAPEZOID):       # :430-443, :542-555: the first branch that holds
                p, c = self.points, self.trap_coeffs
                conds = self.trapezoid_branches(ph)
                self.double_writes += int(np.count_nonzero(np.sum(conds, axis=0) != 1))     # what the reference leaves undefined
                vals = [c[0] * pf + dc, np.full(ph.shape, A + dc, f32), c[1] * pf + c[2] + dc, np.full(ph.shape, dc - A, f32),
                        c[0] * pf + c[3] + dc]
                v = np.select(conds, vals, f32(0)).astype(f32)
                return self.trap_atten * v if fn == FG_BL_TRAPEZOID else v
            if fn in (FG_PULSETRAIN, FG_BL_PULSETRAIN):     # :453-458, :580-585: the else branch is not scaled
                t, k = self.train, (self.pulse_atten if fn == FG_BL_PULSETRAIN else None)
                up, down, rest = A + dc, dc - A, f32(0) + dc
                if k is not None:
                    up, down = k * up, k * down
                return np.where(ph <= t[0], up, np.where((ph >= t[1]) & (ph <= t[2]), down, rest)).astype(f32)
            if fn in (FG_PARABOLIC, FG_BL_PARABOLIC):       # :467-473, :610-616: the else branch is not scaled
                x = f32(f32(2) / f32(u32(self.par_word))) * pf - f32(1)
                v = self.par_amplitude * (f32(1) - x * x) + dc
                if fn == FG_BL_PARABOLIC:
                    v = self.par_atten * v
                return np.where(ph < self.par_word, v, f32(0) + dc).astype(f32)
        raise ValueError(fn)

    def trapezoid_branches(self, ph):
        p = self.points
        return [ph < p[0], (ph >= p[0]) & (ph <= p[1]), (ph > p[1]) & (ph < p[2]), (ph >= p[2]) & (ph <= p[3]), ph > p[3]]

    def do_process(self, over, count, sine=None):
        if self.function < FG_BL_RECTANGULAR:
            ph, self.acc = serial_phases(self.acc, self.freq_word, self.mask, count)
            return np.asarray(self.wave(ph, sine), f32)
        # :481-498 and its four siblings: chunks of PROCESS_BUF_LIMIT_SIZE / N; the filter's state runs on from chunk to chunk, so
        # one downsample over the whole row gives the same values
        ph, self.acc = serial_phases(self.acc, self.freq_word_over, self.mask, self.oversampling * count)
        row = np.asarray(self.wave(ph), f32)
        self.last_synth = row
        return over.downsample(row[None, :])[0]

    # -- process_*, :691-747 ---------------------------------------------------------------------------------------------------
    def process(self, count, op=OP_OVERWRITE, src=None, sine=None):
        self.update_settings()
        s = self.do_process(self.over, count, sine)
        for lo in range(0, count, PROCESS_BUF_LIMIT_SIZE):  # every chunk lands at the start of vSynthBuffer
            chunk = s[lo:lo + PROCESS_BUF_LIMIT_SIZE]
            self.synth[:chunk.size] = chunk
        if op == OP_OVERWRITE:                              # :733-747
            return s
        base = np.zeros(count, f32) if src is None else np.asarray(src, f32)       # fill_zero / copy, :695-698
        with np.errstate(all="ignore"):
            return (base + s if op == OP_ADD else base * s).astype(f32)            # add2 / mul2

    def get_periods(self, periods, skip, samples):          # :635-689
        backup, self.acc = self.acc, self.init_word
        out = np.empty(samples, f32)
        with np.errstate(all="ignore"):
            duration = f32(f32(self.sample_rate) / self.frequency)
            if not duration > 0 or np.isinf(duration):      # the reference's loops do not end for these: nothing is written
                self.acc = backup
                return None
            out_samples, skip_samples = f32(duration * f32(periods)), f32(duration * f32(skip))
            step = f32(out_samples / f32(samples))
        buf_size = 0
        while skip_samples > 0:
            to_do = limited(f32(f32(out_samples + skip_samples) + step))
            self.synth[:to_do] = self.do_process(self.over_periods, to_do)
            buf_size = to_do
            skip_samples = f32(skip_samples - f32(to_do))
        t, at = f32(f32(buf_size) + skip_samples), 0
        while at < samples:
            if t < buf_size:
                out[at] = self.synth[int(t)] if 0 <= t < PROCESS_BUF_LIMIT_SIZE else f32(0)     # in front of the buffer: 0.0f, the class's rule
                t = f32(t + step)
                at += 1
            else:
                to_do = limited(f32(out_samples + step))
                self.synth[:to_do] = self.do_process(self.over_periods, to_do)
                out_samples = f32(out_samples - f32(to_do))
                buf_size = PROCESS_BUF_LIMIT_SIZE
                t = f32(t - f32(buf_size))
        self.acc = backup
        return out

    def words(self):
        """The settings words and coefficients in the order of WORDS, as uint32 (floats by their bits)."""
        c, t = self.saw_coeffs, self.trap_coeffs
        vals = [self.acc, self.mask, self.acc2phase, self.freq_word, self.init_word, self.referenced_dc, self.sq_amplitude, self.sq_wave_dc,
                self.duty_word, self.rect_wave_dc, self.rect_atten, self.width_word, c[0], c[1], c[2], c[3], self.saw_atten,
                self.points[0], self.points[1], self.points[2], self.points[3], t[0], t[1], t[2], t[3], self.trap_atten,
                self.train[0], self.train[1], self.train[2], self.pulse_wave_dc, self.pulse_atten, self.par_amplitude, self.par_word,
                self.par_wave_dc, self.par_atten, self.oversampling, self.freq_word_over]
        return np.array([int(np.asarray(v, f32).view(u32)) if isinstance(v, np.floating) else int(v) for v in vals], u32)


def limited(want):
    """:652-654, :675-677: a float count of samples, rounded up, at most one buffer and none for a negative one."""
    want = math.ceil(float(want))
    return PROCESS_BUF_LIMIT_SIZE if want >= PROCESS_BUF_LIMIT_SIZE else max(int(want), 0)


def times_of(mode):
    """Oversampler::get_oversampling, Oversampler.cpp:146-195."""
    return (2, 3, 4, 6, 8)[(mode - 1) // 6] if 1 <= mode <= 30 else 1


def apply(osc, op, rows=None, at=0, sine=None):
    """One operation of a recorded case on osc; a process operation returns its output."""
    what, a, b, c = int(op[0]), op[1], op[2], op[3]
    if what in PROCESS_OPS:
        n = int(a)
        src = None if what in (P_OVERWRITE, P_ADD_NULL, P_MUL_NULL) else rows[at:at + n]
        kind = OP_OVERWRITE if what == P_OVERWRITE else OP_ADD if what in (P_ADD, P_ADD_NULL, P_ADD_INPLACE) else OP_MUL
        return osc.process(n, kind, src, sine)
    if what == GET_PERIODS:
        return osc.get_periods(int(a), int(b), int(c))
    {SET_FUNCTION: lambda: osc.set_function(int(a)), SET_FREQUENCY: lambda: osc.set_frequency(f32(a)),
     SET_SAMPLE_RATE: lambda: osc.set_sample_rate(int(a)), SET_PHASE: lambda: osc.set_phase(f32(a)),
     SET_BITS: lambda: osc.set_phase_accumulator_bits(int(a)), SET_DC_OFFSET: lambda: osc.set_dc_offset(f32(a)),
     SET_DC_REFERENCE: lambda: osc.set_dc_reference(int(a)), SET_AMPLITUDE: lambda: osc.set_amplitude(f32(a)),
     SET_DUTY: lambda: osc.set_duty_ratio(f32(a)), SET_WIDTH: lambda: osc.set_width(f32(a)),
     SET_TRAPEZOID: lambda: osc.set_trapezoid_ratios(f32(a), f32(b)), SET_PULSETRAIN: lambda: osc.set_pulsetrain_ratios(f32(a), f32(b)),
     SET_PARABOLIC_WIDTH: lambda: osc.set_parabolic_width(f32(a)),
     SET_SQUARED_INVERSION: lambda: osc.set_squared_sinusoid_inversion(bool(a)),
     SET_PARABOLIC_INVERSION: lambda: osc.set_parabolic_inversion(bool(a)), SET_OVER_MODE: lambda: osc.set_oversampler_mode(int(a)),
     RESET_PHASE: osc.reset_phase_accumulator, UPDATE: osc.update_settings}[what]()
    return None


def run_case(case, sine=None, oversampler=None):
    """A recorded case (ops [k, 4], src [N]) -> out [N], the periods that its GET_PERIODS operations returned (concatenated), the
    oscillator, and which samples a sinusoid made."""
    osc = Oscillator(oversampler=oversampler)
    src, at = case["src"], 0
    out, periods, sinus = np.zeros(src.size, f32), [], np.zeros(src.size, bool)
    for op in case["ops"]:
        r = apply(osc, op, src, at, sine)
        if int(op[0]) in PROCESS_OPS:
            out[at:at + r.size] = r
            sinus[at:at + r.size] = osc.function in SINUSOIDS
            at += r.size
        elif int(op[0]) == GET_PERIODS:
            periods.append(r)
    assert at == src.size, (at, src.size)
    return out, (np.concatenate(periods) if periods else np.zeros(0, f32)), osc, sinus


def bits(a):
    return np.ascontiguousarray(a, f32).view(u32)


def same(got, want, made=True):
    """The rule of tests/dyndelay_ref.py::same: bit for bit; where arithmetic made a NaN, a NaN."""
    got, want = np.asarray(got, f32), np.asarray(want, f32)
    return bool(got.shape == want.shape and np.all((bits(got) == bits(want)) | (np.asarray(made, bool) & np.isnan(got) & np.isnan(want))))


def inside(got, star, below, above):
    """The interval rule for sinusoid samples: got lies in the closed interval that the restatement's outputs with S*, its float32
    predecessor and its successor span.  NaN only where all three are NaN."""
    got = np.asarray(got, f32).astype(f64)
    three = np.stack([np.asarray(v, f32).astype(f64) for v in (star, below, above)])
    nan = np.isnan(three).any(axis=0)
    with np.errstate(invalid="ignore"):
        ok = (got >= np.nanmin(np.where(nan, 0, three), axis=0)) & (got <= np.nanmax(np.where(nan, 0, three), axis=0))
    return np.where(nan, np.isnan(got) & np.isnan(three).all(axis=0), ok)
