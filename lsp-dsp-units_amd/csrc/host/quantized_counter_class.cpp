// lsp::dspu::QuantizedCounter (src/main/stat/QuantizedCounter.cpp) on a mi_qcounter_bank of one channel kept beside the object
// (beside.h).  The object's fields are what counts: the setters are the reference's host work on them.  process() and an
// update_settings() over a window that holds samples hand the settings to the bank, run its kernel on the staged row and read
// nHead, nCount, the ring and the counters back into vHistory and vCounters, the host's copies, so the inline getters are the
// reference's.  The bin rule and the window of a call of any length are the bank's (quantized_counter_bank.h).
#include <lsp-plug.in/dsp-units/stat/QuantizedCounter.h>

#include <cstddef>
#include <cstdlib>
#include <cstring>

#include "beside.h"
#include "../quantized_counter_bank.h"

namespace lsp
{
namespace dspu
{
namespace
{
    // the sizes that the bank of one channel was made for
    struct counter_held { uint32_t max_period = 0, max_levels = 0; };

    typedef mi_host::registry<mi_host::beside<mi_qcounter_bank_t, counter_held, mi_qcounter_bank_destroy> > qcounters;

    static_assert(sizeof(QuantizedCounter) == 72, "sizeof(QuantizedCounter)");

    uint32_t limited(size_t v, uint32_t most)      { return (v < 1) ? 1u : (v > most) ? most : uint32_t(v); }
}

QuantizedCounter::QuantizedCounter()    { construct(); }
QuantizedCounter::~QuantizedCounter()   { destroy(); }

void QuantizedCounter::construct()                              // :42-62
{
    qcounters::drop(this);                                      // whatever lived at this address before
    nPeriod = 0;
    nLevels = 0;
    nHead = 0;
    nCapacity = 0;
    nCount = 0;
    nMaxPeriod = 0;
    nMaxLevels = 0;
    fMinValue = 0.0f;
    fMaxValue = 0.0f;
    fRStep = 0.0f;
    bUpdate = true;
    vHistory = NULL;
    vCounters = NULL;
    pData = NULL;
}

void QuantizedCounter::destroy()                                // :64-70
{
    qcounters::drop(this);
    free(pData);
    pData = NULL;
    vHistory = NULL;
    vCounters = NULL;
}

status_t QuantizedCounter::init(size_t max_period, size_t max_levels)      // :72-98; the settings stay as they are
{
    if (max_period < 1 || max_levels < 1 || max_levels > (size_t(1) << 24) || max_period > size_t(UINT32_MAX) - 2 * mi_qcounter::BUFFER_GAP)
        return STATUS_INVALID_VALUE;
    const size_t capacity = mi_qcounter::capacity_of(max_period);
    const size_t szof_history = capacity * sizeof(float);
    const size_t szof_levels = ((max_levels + 2) * sizeof(uint32_t) + 63) & ~size_t(63);
    uint8_t *data = static_cast<uint8_t *>(calloc(szof_history + szof_levels + 64, 1));     // zeroed: the ring and the counters
    if (data == NULL)
        return STATUS_NO_MEM;
    qcounters::drop(this);                                      // a bank of other sizes
    free(pData);
    pData = data;
    uint8_t *ptr = data + ((64 - (reinterpret_cast<uintptr_t>(data) & 63)) & 63);
    vHistory = reinterpret_cast<float *>(ptr);
    vCounters = reinterpret_cast<uint32_t *>(ptr + szof_history);
    nHead = 0;
    nCapacity = uint32_t(capacity);
    nCount = 0;
    nMaxPeriod = uint32_t(max_period);
    nMaxLevels = uint32_t(max_levels);
    return STATUS_OK;
}

void QuantizedCounter::set_period(size_t period)                // :100-107
{
    nPeriod = limited(period, nMaxPeriod);
}

void QuantizedCounter::set_levels(size_t levels)                // :109-117
{
    const uint32_t v = limited(levels, nMaxLevels);
    if (v == nLevels)
        return;
    nLevels = v;
    bUpdate = true;
}

void QuantizedCounter::set_min_value(float min)                 // :119-126
{
    if (fMinValue == min)
        return;
    fMinValue = min;
    bUpdate = true;
}

void QuantizedCounter::set_max_value(float max)                 // :128-135
{
    if (fMaxValue == max)
        return;
    fMaxValue = max;
    bUpdate = true;
}

void QuantizedCounter::set_value_range(float min, float max)    // :137-146
{
    if ((fMinValue == min) && (fMaxValue == max))
        return;
    fMinValue = min;
    fMaxValue = max;
    bUpdate = true;
}

void QuantizedCounter::set_range(float min, float max, size_t levels)      // :148-160
{
    const uint32_t v = limited(levels, nMaxLevels);
    if ((nLevels == v) && (fMinValue == min) && (fMaxValue == max))
        return;
    nLevels = v;
    fMinValue = min;
    fMaxValue = max;
    bUpdate = true;
}

namespace
{
    // The bank of `self` for these sizes, with the object's window (a fresh bank gets the host's copies) and its settings.  Where
    // the object's bUpdate is set the bank's is too, whatever values the bank held before: a value that was changed and changed
    // back recounts in the reference as well.
    qcounters::entry *ready(const void *self, uint32_t max_period, uint32_t max_levels, uint32_t head, uint32_t count, const float *history,
                            const uint32_t *counters, uint32_t period, uint32_t levels, float min_value, float max_value, bool update)
    {
        qcounters::entry *p = qcounters::of(self, [=](qcounters::entry &e) { return mi_qcounter_bank_create(&e.bank, 1, max_period, max_levels); });
        if (p == nullptr)
            return nullptr;
        counter_held &h = p->held;
        if (h.max_period != max_period || h.max_levels != max_levels)      // the entry is new: init() drops the old one
        {
            const mi_qcounter_state_t s = { head, count, 0 };
            if (mi_qcounter_bank_set_state(p->bank, 0, &s, history, counters, nullptr) != MI_OK)
                return nullptr;
            h.max_period = max_period, h.max_levels = max_levels;
        }
        if ((period != 0 && mi_qcounter_bank_set_period(p->bank, 0, period) != MI_OK) ||
            mi_qcounter_bank_set_range(p->bank, 0, min_value, max_value, levels) != MI_OK)
            return nullptr;
        int pending = 0;
        if (mi_qcounter_bank_needs_update(p->bank, 0, &pending) != MI_OK)
            return nullptr;
        if (update && !pending)
        {
            const float other = (min_value == 0.0f) ? 1.0f : 0.0f;
            if (mi_qcounter_bank_set_min_value(p->bank, 0, other) != MI_OK || mi_qcounter_bank_set_min_value(p->bank, 0, min_value) != MI_OK)
                return nullptr;
        }
        return p;
    }
}

void QuantizedCounter::update_settings()                        // :162-187
{
    if (!bUpdate)
        return;
    if (nCount > 0)                                             // the samples held are counted anew on the device
    {
        qcounters::entry *p = ready(this, nMaxPeriod, nMaxLevels, nHead, nCount, vHistory, vCounters, nPeriod, nLevels, fMinValue, fMaxValue, true);
        mi_qcounter_state_t st;
        if (p == nullptr || mi_qcounter_bank_update_settings(p->bank, nullptr) != MI_OK ||
            mi_qcounter_bank_get_state(p->bank, 0, &st, nullptr, vCounters, nullptr) != MI_OK)
            return;
    }
    else
        for (size_t i = 0; vCounters != NULL && i < size_t(nMaxLevels) + 2; ++i)
            vCounters[i] = 0;
    bUpdate = false;
    fRStep = mi_qcounter::rstep_of(nLevels, fMinValue, fMaxValue);
}

void QuantizedCounter::clear()                                  // :189-196
{
    nHead = 0;
    nCount = 0;
    for (size_t i = 0; vCounters != NULL && i < size_t(nMaxLevels) + 2; ++i)
        vCounters[i] = 0;
    qcounters::entry *p = qcounters::find(this);
    if (p != nullptr)
        mi_qcounter_bank_clear(p->bank, 0);
}

void QuantizedCounter::process(const float *data, size_t count) // :242-266
{
    // Without a ring, a period or levels the reference's state is meaningless (a step of 0 / 0, a window of nothing); and the
    // kernel counts in 32 bits.  Nothing is done then.
    if (vHistory == NULL || nPeriod == 0 || nLevels == 0 || count >= (size_t(1) << 31))
        return;
    qcounters::entry *p = ready(this, nMaxPeriod, nMaxLevels, nHead, nCount, vHistory, vCounters, nPeriod, nLevels, fMinValue, fMaxValue, bUpdate);
    if (p == nullptr || !p->buf.reserve((count > 0) ? count : 1))
        return;
    mi_qcounter_state_t st;
    if ((count > 0 && !p->buf.up(0, data, count)) ||
        mi_qcounter_bank_process(p->bank, p->buf.row(0), count, count, nullptr) != MI_OK ||
        mi_qcounter_bank_get_state(p->bank, 0, &st, vHistory, vCounters, nullptr) != MI_OK)
        return;
    nHead = st.head;
    nCount = st.count;
    if (bUpdate)
    {
        bUpdate = false;
        fRStep = mi_qcounter::rstep_of(nLevels, fMinValue, fMaxValue);
    }
}

void QuantizedCounter::dump(IStateDumper *v) const              // :268-287
{
    v->write("nPeriod", nPeriod);
    v->write("nLevels", nLevels);
    v->write("nHead", nHead);
    v->write("nCapacity", nCapacity);
    v->write("nCount", nCount);
    v->write("nMaxPeriod", nMaxPeriod);
    v->write("nMaxLevels", nMaxLevels);

    v->write("fMinValue", fMinValue);
    v->write("fMaxValue", fMaxValue);
    v->write("fRStep", fRStep);
    v->write("bUpdate", bUpdate);

    v->write("vHistory", vHistory);
    v->write("vCounters", vCounters);

    v->write("pData", pData);
}

} // namespace dspu
} // namespace lsp
