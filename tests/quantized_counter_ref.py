"""lsp::dspu::QuantizedCounter (src/main/stat/QuantizedCounter.cpp) restated in numpy, word for word: the history ring, the
nMaxLevels + 2 counters, nHead, nCount and the settings.  What the bank, the class and this file share:

  * the bin of a sample is trunc((v - fMinValue) * fRStep) with both roundings in float32.  Where C++ leaves the conversion to
    int32_t undefined it is DEFINED as the reference's compiled class has it on x86-64: a NaN, a product >= 2^31 or <= -1 counts
    as below, one in [nLevels, 2^31) as above (bin_words());
  * process() leaves the window of the last min(nPeriod, samples seen) samples for ANY count: the reference's own loop, fed in
    pieces of at most nCapacity - nPeriod, where it is exact.  QuantizedCounter(defect=True) runs the reference's loop on the
    whole call instead: with nCount + count > nCapacity the copy overwrites samples that are not evicted yet and the wrong ones
    are taken out.  That is the reference's defect; nothing else here reproduces it.

`mutation` names one deliberate error (MUTATIONS) for the tests that show that the recorded cases catch it."""
import numpy as np

f32, u32 = np.float32, np.uint32
BUFFER_GAP = 0x400
SET_PERIOD, SET_LEVELS, SET_MIN, SET_MAX, SET_VALUE_RANGE, SET_RANGE, UPDATE, CLEAR, PROCESS, PROCESS_WHOLE = range(10)
OP_NAMES = ("set_period", "set_levels", "set_min_value", "set_max_value", "set_value_range", "set_range", "update_settings", "clear",
            "process", "process in one call of the reference")
MUTATIONS = ("round", "nan_bin0", "inf_above", "evict_first", "recount_window")


def capacity_of(max_period):
    """nCapacity, :74, :85"""
    return (((max_period + BUFFER_GAP) * 4 + 63) & ~63) // 4


def rstep_of(levels, min_value, max_value):
    """fRStep, :169: one float32 division"""
    with np.errstate(all="ignore"):
        return f32(f32(levels) / f32(f32(max_value) - f32(min_value)))


def bin_words(v, min_value, rstep, levels, max_levels, mutation=None):
    """The word of vCounters that each sample counts in."""
    with np.errstate(all="ignore"):
        v = np.asarray(v, f32)
        s = ((v - f32(min_value)).astype(f32) * f32(rstep)).astype(f32)
        below = ~(s > f32(-1.0)) | (s >= f32(2147483648.0))
        above = s >= f32(levels)
        if mutation == "nan_bin0":
            below &= ~np.isnan(s)
        if mutation == "inf_above":
            above |= s >= f32(2147483648.0)
            below &= ~above
        t = np.where(below | above | np.isnan(s), f32(0.0), s)
        if mutation == "round":
            idx = np.rint(t).astype(np.int64)
            above |= ~below & (idx >= levels)
            below |= idx < 0
        else:
            idx = np.trunc(t).astype(np.int64)
    return np.where(below, max_levels, np.where(above, max_levels + 1, idx)).astype(np.int64)


def make_plan(head, count, period, capacity, n):
    """The closed form of one call, as mi_qcounter::make_plan has it."""
    c0 = min(count, period)
    late = min(c0, max(0, c0 + n - period))
    evict = (count - c0) + late
    store_from = max(0, n - capacity)
    return dict(tail=(head + capacity - count) % capacity, evict=evict, remain=count - evict, keep_from=max(0, n - period),
                store_from=store_from, store_pos=(head + store_from) % capacity, head_after=(head + n) % capacity,
                count_after=min(c0 + n, period))


class QuantizedCounter:
    def __init__(self, max_period, max_levels, defect=False, mutation=None):
        assert mutation is None or mutation in MUTATIONS
        self.max_period, self.max_levels = int(max_period), int(max_levels)
        self.capacity = capacity_of(self.max_period)
        self.period = self.levels = self.head = self.count = 0
        self.min_value = self.max_value = self.rstep = f32(0.0)
        self.update = True
        self.history = np.zeros(self.capacity, f32)
        self.counters = np.zeros(self.max_levels + 2, u32)
        self.defect, self.mutation = defect, mutation

    # ---- setters, :100-160
    def set_period(self, period):
        self.period = min(max(int(period), 1), self.max_period)

    def set_levels(self, levels):
        levels = min(max(int(levels), 1), self.max_levels)
        if levels != self.levels:
            self.levels, self.update = levels, True

    def set_min_value(self, v):
        if not (self.min_value == f32(v)):
            self.min_value, self.update = f32(v), True

    def set_max_value(self, v):
        if not (self.max_value == f32(v)):
            self.max_value, self.update = f32(v), True

    def set_value_range(self, lo, hi):
        if self.min_value == f32(lo) and self.max_value == f32(hi):
            return
        self.min_value, self.max_value, self.update = f32(lo), f32(hi), True

    def set_range(self, lo, hi, levels):
        levels = min(max(int(levels), 1), self.max_levels)
        if self.levels == levels and self.min_value == f32(lo) and self.max_value == f32(hi):
            return
        self.levels, self.min_value, self.max_value, self.update = levels, f32(lo), f32(hi), True

    # ---- the counters
    def _add(self, values, sign):
        words = bin_words(values, self.min_value, self.rstep, self.levels, self.max_levels, self.mutation)
        delta = np.bincount(words, minlength=self.max_levels + 2).astype(np.int64)
        self.counters = ((self.counters.astype(np.int64) + sign * delta) & 0xFFFFFFFF).astype(u32)

    def _span(self, tail, n):
        """n ring words from position tail on"""
        return self.history[(tail + np.arange(n)) % self.capacity]

    def update_settings(self):                                  # :162-187
        if not self.update:
            return
        if self.mutation == "evict_first":                      # invisible behind process(), visible behind an explicit call
            self._evict()
        self.update = False
        self.rstep = rstep_of(self.levels, self.min_value, self.max_value)
        self.counters[:] = 0
        n = min(self.count, self.period) if self.mutation == "recount_window" else self.count
        if n > 0:
            self._add(self._span((self.head + self.capacity - n) % self.capacity, n), 1)

    def clear(self):                                            # :189-196
        self.head = self.count = 0
        self.counters[:] = 0

    def _evict(self):                                           # :228-240
        if self.count > self.period:
            n = self.count - self.period
            self._add(self._span((self.head + self.capacity - self.count) % self.capacity, n), -1)
            self.count -= n

    def _process_reference(self, data):                         # :242-266
        self.update_settings()
        self._evict()
        offset = 0
        while offset < len(data):
            to_do = min(len(data) - offset, self.capacity - self.head)
            self.history[self.head:self.head + to_do] = data[offset:offset + to_do]
            self._add(data[offset:offset + to_do], 1)
            self.count += to_do
            self.head = (self.head + to_do) % self.capacity
            self._evict()
            offset += to_do

    def process(self, data):
        data = np.asarray(data, f32)
        if self.defect or len(data) == 0:
            return self._process_reference(data)
        offset = 0
        while offset < len(data):                               # nPeriod does not change inside a call
            piece = self.capacity - self.period
            self._process_reference(data[offset:offset + piece])
            offset += piece

    def process_closed_form(self, data):
        """The same call as the kernel forms it: one plan, the final window counted directly."""
        data = np.asarray(data, f32)
        n = len(data)
        pl = make_plan(self.head, self.count, self.period, self.capacity, n)
        if self.update:
            self.update = False
            self.rstep = rstep_of(self.levels, self.min_value, self.max_value)
            self.counters[:] = 0
            self._add(self._span((pl["tail"] + pl["evict"]) % self.capacity, pl["remain"]), 1)
        else:
            self._add(self._span(pl["tail"], pl["evict"]), -1)
        self._add(data[pl["keep_from"]:], 1)
        stored = data[pl["store_from"]:]
        self.history[(pl["store_pos"] + np.arange(len(stored))) % self.capacity] = stored
        self.head, self.count = pl["head_after"], pl["count_after"]

    # ---- what a test compares
    def below(self):
        return int(self.counters[self.max_levels])

    def above(self):
        return int(self.counters[self.max_levels + 1])

    def settings_words(self):
        """counters, then nHead, nCount, nPeriod, nLevels, fMinValue, fMaxValue, fRStep (bits), bUpdate"""
        tail = np.array([self.head, self.count, self.period, self.levels, 0, 0, 0, int(self.update)], u32)
        tail[4:7] = np.array([self.min_value, self.max_value, self.rstep], f32).view(u32)
        return np.concatenate([self.counters, tail])

    def state_words(self):
        """Every word of the object: the ring in storage order, then settings_words()."""
        return np.concatenate([self.history.view(u32), self.settings_words()])


def apply(q, op, x, closed_form=False):
    """One row of a case's operation list: code, row of x, offset, n or the integer argument, two float arguments."""
    code, n = int(op[0]), int(op[3])
    if code == SET_PERIOD:
        q.set_period(n)
    elif code == SET_LEVELS:
        q.set_levels(n)
    elif code == SET_MIN:
        q.set_min_value(f32(op[4]))
    elif code == SET_MAX:
        q.set_max_value(f32(op[4]))
    elif code == SET_VALUE_RANGE:
        q.set_value_range(f32(op[4]), f32(op[5]))
    elif code == SET_RANGE:
        q.set_range(f32(op[4]), f32(op[5]), n)
    elif code == UPDATE:
        q.update_settings()
    elif code == CLEAR:
        q.clear()
    elif code in (PROCESS, PROCESS_WHOLE):
        row = x[int(op[1]), int(op[2]):int(op[2]) + n]
        if code == PROCESS_WHOLE:
            was, q.defect = q.defect, True
            q.process(row)
            q.defect = was
        elif closed_form:
            q.process_closed_form(row)
        else:
            q.process(row)
    else:
        raise ValueError(code)
