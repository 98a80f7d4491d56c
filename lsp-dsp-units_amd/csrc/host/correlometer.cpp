// lsp::dspu::Correlometer (src/main/meters/Correlometer.cpp) on a mi_correlometer_bank of one channel kept beside the object
// (beside.h).  The object's fields are what counts: before every device call the bank is handed nPeriod and -- where they are
// not what process() read back after the previous call -- sCorr, nHead and nWindow; afterwards they are read back.  clear()
// zeroes the device's rings at once.  The rings live on the device only: vInA, vInB and pData stay NULL.
#include <lsp-plug.in/dsp-units/meters/Correlometer.h>

#include <cstddef>

#include "beside.h"

namespace lsp
{
namespace dspu
{
namespace
{
    constexpr size_t BUFFER_SIZE = 0x400, DEFAULT_ALIGN = 0x40;         // Correlometer.cpp:29; lsp-common-lib's alignment

    struct corr_held { float v = 0.0f, a = 0.0f, b = 0.0f; uint32_t head = 0, window = 0, known = 0; };

    typedef mi_host::registry<mi_host::beside<mi_correlometer_bank_t, corr_held, mi_correlometer_bank_destroy> > correlometers;

    // the entry of `self`, its bank made for the object's nMaxPeriod at the first call
    correlometers::entry *of(const void *self, uint32_t max_period)
    {
        return correlometers::of(self, [max_period](correlometers::entry &e) { return mi_correlometer_bank_create(&e.bank, 1, max_period); });
    }

    int send_state(mi_correlometer_bank_t *bank, const corr_held &now)
    {
        const mi_correlometer_state_t s = { now.v, now.a, now.b, now.head, now.window };
        return mi_correlometer_bank_set_state(bank, 0, &s, 0, nullptr);
    }

    static_assert(sizeof(void *) != 8 || sizeof(Correlometer) == 64, "sizeof(Correlometer)");
}

Correlometer::Correlometer()  { construct(); }
Correlometer::~Correlometer() { destroy(); }

void Correlometer::construct()                                  // :41-57
{
    correlometers::drop(this);                                  // whatever lived at this address before
    sCorr.v = sCorr.a = sCorr.b = 0.0f;
    vInA = vInB = NULL;
    nCapacity = nHead = nMaxPeriod = nPeriod = nWindow = 0;
    nFlags = CF_UPDATE;
    pData = NULL;
}

void Correlometer::destroy()                                    // :59-66
{
    correlometers::drop(this);
    vInA = vInB = NULL;
    pData = NULL;
}

status_t Correlometer::init(size_t max_period)                  // :68-101
{
    destroy();
    if (max_period >= (size_t(1) << 28))
        return STATUS_NO_MEM;
    sCorr.v = sCorr.a = sCorr.b = 0.0f;
    nCapacity = uint32_t((max_period + BUFFER_SIZE + DEFAULT_ALIGN - 1) / DEFAULT_ALIGN * DEFAULT_ALIGN);
    nHead = 0;
    nMaxPeriod = uint32_t(max_period);
    nPeriod = 0;
    nFlags = 0;
    return STATUS_OK;
}

void Correlometer::set_period(size_t period)                    // :103-111
{
    period = (period < nMaxPeriod) ? period : nMaxPeriod;
    if (period == nPeriod)
        return;
    nPeriod = uint32_t(period);
    nFlags |= CF_UPDATE;
}

void Correlometer::update_settings()                            // :113-120
{
    if (nFlags == 0)
        return;
    nWindow = nPeriod;
    nFlags = 0;
}

void Correlometer::clear()                                      // :122-132
{
    sCorr.v = sCorr.a = sCorr.b = 0.0f;
    nHead = nPeriod;
    if (nMaxPeriod == 0)
        return;
    correlometers::entry *p = of(this, nMaxPeriod);
    if (p == nullptr)
        return;
    const mi_correlometer_state_t s = { 0.0f, 0.0f, 0.0f, nHead, 0 };
    (void)mi_correlometer_bank_set_state(p->bank, 0, &s, 1, nullptr);  // the rings; process() sends the state as it is then
    p->held.known = 0;
}

void Correlometer::process(float *dst, const float *a, const float *b, size_t count)       // :134-184
{
    update_settings();
    if (count == 0 || nPeriod == 0 || nCapacity == 0)
        return;                                                 // a period of 0: the reference never returns
    correlometers::entry *p = of(this, nMaxPeriod);
    if (p == nullptr || !p->buf.reserve(count, 3))
        return;
    mi_correlometer_params_t q;
    if (mi_correlometer_bank_get_params(p->bank, 0, &q) != MI_OK)
        return;
    if (q.period != nPeriod)
    {
        if (mi_correlometer_bank_set_period(p->bank, 0, nPeriod) != MI_OK)
            return;
        p->held.known = 0;                                      // the bank's own nWindow = nPeriod gives way to the object's
    }
    if (!p->hand_over_state({ sCorr.v, sCorr.a, sCorr.b, nHead % nCapacity, (nWindow < nPeriod) ? nWindow : nPeriod, 1 }, send_state))
        return;
    p->held.known = 0;
    float *d_a = p->buf.row(0), *d_b = p->buf.row(1), *d_out = p->buf.row(2);
    mi_correlometer_state_t s;
    if (!p->buf.up(0, a, count) || !p->buf.up(1, b, count) ||
        mi_correlometer_bank_process(p->bank, d_out, d_a, d_b, count, count, count, count, nullptr) != MI_OK ||
        !p->buf.down(dst, 2, count) ||
        mi_correlometer_bank_get_state(p->bank, 0, &s, nullptr) != MI_OK)
        return;
    p->held = corr_held{ s.v, s.a, s.b, s.head, s.window, 1 };
    sCorr.v = s.v, sCorr.a = s.a, sCorr.b = s.b;
    nHead = s.head;
    nWindow = s.window;
}

void Correlometer::dump(IStateDumper *v) const                  // :186-206
{
    v->begin_object("sCorr", &sCorr, sizeof(dsp::correlation_t));
    {
        v->write("v", sCorr.v);
        v->write("a", sCorr.a);
        v->write("b", sCorr.b);
    }
    v->end_object();
    v->write("vInA", vInA);
    v->write("vInB", vInB);
    v->write("nCapacity", nCapacity);
    v->write("nHead", nHead);
    v->write("nMaxPeriod", nMaxPeriod);
    v->write("nPeriod", nPeriod);
    v->write("nWindow", nWindow);
    v->write("nFlags", nFlags);
    v->write("pData", pData);
}

} // namespace dspu
} // namespace lsp
