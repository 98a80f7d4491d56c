// lsp::dspu::Panometer (src/main/meters/Panometer.cpp) on a mi_panometer_bank of one channel kept beside the object (beside.h).
// The object's fields are what counts: before every device call the bank is handed nPeriod, enPanLaw and fDefault and -- where
// they are not what process() read back after the previous call -- fValueA, fValueB, nHead and nWindow; afterwards they are read
// back.  clear() zeroes the device's rings at once.  The rings live on the device only: vInA, vInB and pData stay NULL.
#include <lsp-plug.in/dsp-units/meters/Panometer.h>

#include <cstddef>

#include "beside.h"

namespace lsp
{
namespace dspu
{
namespace
{
    constexpr size_t BUFFER_SIZE = 0x400, DEFAULT_ALIGN = 0x40;         // Panometer.cpp:30; lsp-common-lib's alignment

    struct pan_held { float va = 0.0f, vb = 0.0f; uint32_t head = 0, window = 0, known = 0; };

    typedef mi_host::registry<mi_host::beside<mi_panometer_bank_t, pan_held, mi_panometer_bank_destroy> > panometers;

    // the entry of `self`, its bank made for the object's nMaxPeriod at the first call
    panometers::entry *of(const void *self, uint32_t max_period)
    {
        return panometers::of(self, [max_period](panometers::entry &e) { return mi_panometer_bank_create(&e.bank, 1, max_period); });
    }

    int send_state(mi_panometer_bank_t *bank, const pan_held &now)
    {
        const mi_panometer_state_t s = { now.va, now.vb, now.head, now.window };
        return mi_panometer_bank_set_state(bank, 0, &s, 0, nullptr);
    }

    static_assert(sizeof(void *) != 8 || sizeof(Panometer) == 64, "sizeof(Panometer)");
}

Panometer::Panometer()  { construct(); }
Panometer::~Panometer() { destroy(); }

void Panometer::construct()                                     // :42-58
{
    panometers::drop(this);                                     // whatever lived at this address before
    vInA = vInB = NULL;
    enPanLaw = PAN_LAW_EQUAL_POWER;
    fValueA = fValueB = fNorm = 0.0f;
    fDefault = 0.5f;
    nCapacity = nHead = nMaxPeriod = nPeriod = nWindow = 0;
    pData = NULL;
}

void Panometer::destroy()                                       // :60-69
{
    panometers::drop(this);
    vInA = vInB = NULL;
    pData = NULL;
}

status_t Panometer::init(size_t max_period)                     // :71-100
{
    destroy();
    if (max_period >= (size_t(1) << 28))
        return STATUS_NO_MEM;
    nCapacity = uint32_t((max_period + BUFFER_SIZE + DEFAULT_ALIGN - 1) / DEFAULT_ALIGN * DEFAULT_ALIGN);
    nHead = 0;
    nMaxPeriod = uint32_t(max_period);
    nPeriod = 0;
    return STATUS_OK;
}

void Panometer::set_pan_law(pan_law_t law)                      // :102-105
{
    enPanLaw = law;
}

void Panometer::set_default_pan(float dfl)                      // :107-110
{
    fDefault = dfl;
}

void Panometer::set_period(size_t period)                       // :112-123
{
    period = (period < nMaxPeriod) ? period : nMaxPeriod;
    if (period == nPeriod)
        return;
    nPeriod = uint32_t(period);
    nWindow = uint32_t(period);
    fValueA = fValueB = 0.0f;
    fNorm = (period > 0) ? 1.0f / float(period) : 1.0f;
}

void Panometer::clear()                                         // :125-131
{
    nHead = nPeriod;
    if (nMaxPeriod == 0)
        return;
    panometers::entry *p = of(this, nMaxPeriod);
    if (p == nullptr)
        return;
    const mi_panometer_state_t s = { fValueA, fValueB, nHead, 0 };
    (void)mi_panometer_bank_set_state(p->bank, 0, &s, 1, nullptr);     // the rings; process() sends the state as it is then
    p->held.known = 0;
}

void Panometer::process(float *dst, const float *a, const float *b, size_t count)          // :133-216
{
    if (count == 0 || nPeriod == 0 || nCapacity == 0)
        return;                                                 // a period of 0: the reference never returns
    panometers::entry *p = of(this, nMaxPeriod);
    if (p == nullptr || !p->buf.reserve(count, 3))
        return;
    mi_panometer_params_t q;
    if (mi_panometer_bank_get_params(p->bank, 0, &q) != MI_OK)
        return;
    if (q.period != nPeriod)
    {
        if (mi_panometer_bank_set_period(p->bank, 0, nPeriod) != MI_OK)
            return;
        p->held.known = 0;                                      // the bank's own zeroed sums give way to the object's
    }
    if (mi_panometer_bank_set_pan_law(p->bank, 0, (enPanLaw == PAN_LAW_LINEAR) ? MI_PAN_LAW_LINEAR : MI_PAN_LAW_EQUAL_POWER) != MI_OK ||
        mi_panometer_bank_set_default_pan(p->bank, 0, fDefault) != MI_OK)
        return;
    if (!p->hand_over_state({ fValueA, fValueB, nHead % nCapacity, (nWindow < nPeriod) ? nWindow : nPeriod, 1 }, send_state))
        return;
    p->held.known = 0;
    float *d_a = p->buf.row(0), *d_b = p->buf.row(1), *d_out = p->buf.row(2);
    mi_panometer_state_t s;
    if (!p->buf.up(0, a, count) || !p->buf.up(1, b, count) ||
        mi_panometer_bank_process(p->bank, d_out, d_a, d_b, count, count, count, count, nullptr) != MI_OK ||
        !p->buf.down(dst, 2, count) ||
        mi_panometer_bank_get_state(p->bank, 0, &s, nullptr) != MI_OK)
        return;
    p->held = pan_held{ s.value_a, s.value_b, s.head, s.window, 1 };
    fValueA = s.value_a, fValueB = s.value_b;
    nHead = s.head;
    nWindow = s.window;
}

void Panometer::dump(IStateDumper *v) const                     // :218-234
{
    v->write("vInA", vInA);
    v->write("vInB", vInB);
    v->write("enPanLaw", int(enPanLaw));
    v->write("fValueA", fValueA);
    v->write("fValueB", fValueB);
    v->write("fNorm", fNorm);
    v->write("fDefault", fDefault);
    v->write("nCapacity", nCapacity);
    v->write("nHead", nHead);
    v->write("nMaxPeriod", nMaxPeriod);
    v->write("nPeriod", nPeriod);
    v->write("nWindow", nWindow);
    v->write("pData", pData);
}

} // namespace dspu
} // namespace lsp
