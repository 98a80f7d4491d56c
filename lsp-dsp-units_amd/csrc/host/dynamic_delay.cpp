// lsp::dspu::DynamicDelay (src/main/util/DynamicDelay.cpp) on a mi_dyndelay_bank of one channel.  pData is the handle: a record
// of the bank, a staging buffer for process()'s five rows and the head as the device holds it.  nHead moves on the host by
// the call's samples, as on the device; where the member is not what the device holds it is sent in front of the call.
#include <lsp-plug.in/dsp-units/util/DynamicDelay.h>
#include <lsp-plug.in/dsp-units/units.h>

#include <cstddef>
#include <new>

#include "beside.h"

namespace lsp
{
namespace dspu
{
namespace
{
    struct handle
    {
        mi_dyndelay_bank_t *bank = nullptr;
        mi_host::rows       buf;                    // [5][cap]: out, in, delay, fgain, fdelay
        uint32_t            head = 0;               // nHead on the device

        ~handle() { mi_dyndelay_bank_destroy(bank); }
    };

    handle *of(uint8_t *p) { return reinterpret_cast<handle *>(p); }

    // the member's head to the device where the two differ
    bool hand_over_head(handle *h, uint32_t head)
    {
        if (h->head == head)
            return true;
        const mi_dyndelay_state_t s = { head };
        if (mi_dyndelay_bank_set_state(h->bank, 0, &s, nullptr) != MI_OK)
            return false;
        h->head = head;
        return true;
    }

    static_assert(sizeof(DynamicDelay) == 32, "sizeof(DynamicDelay)");
}

bool dynamic_delay_read_line(const DynamicDelay *d, float *dst, size_t offset, size_t count)
{
    const handle *h = (d != NULL) ? of(d->pData) : nullptr;
    return h != nullptr && mi_dyndelay_bank_read_line(h->bank, 0, dst, offset, count, nullptr) == MI_OK;
}

DynamicDelay::DynamicDelay()    { construct(); }
DynamicDelay::~DynamicDelay()   { destroy(); }

void DynamicDelay::construct()                                  // :42-49
{
    vDelay = NULL;
    nHead = 0;
    nCapacity = 0;
    nMaxDelay = 0;
    pData = NULL;
}

void DynamicDelay::destroy()                                    // :51-63
{
    if (pData == NULL)
        return;
    delete of(pData);
    vDelay = NULL;
    nHead = 0;
    nCapacity = 0;
    nMaxDelay = 0;
    pData = NULL;
}

status_t DynamicDelay::init(size_t max_size)                    // :65-89
{
    handle *h = new (std::nothrow) handle();
    if (h == nullptr)
        return STATUS_NO_MEM;
    uint32_t max_delay = 0, capacity = 0;
    if (mi_dyndelay_bank_create(&h->bank, 1, max_size) != MI_OK || mi_dyndelay_bank_get(h->bank, 0, &max_delay, &capacity, nullptr) != MI_OK)
    {
        delete h;
        return STATUS_NO_MEM;
    }
    if (pData != NULL)
        delete of(pData);
    nHead = 0;
    nCapacity = capacity;
    nMaxDelay = int32_t(max_delay);
    pData = reinterpret_cast<uint8_t *>(h);
    return STATUS_OK;
}

void DynamicDelay::clear()                                      // :91-95
{
    handle *h = of(pData);
    if (h == nullptr || mi_dyndelay_bank_clear(h->bank, nullptr) != MI_OK)
        return;
    nHead = 0, h->head = 0;
}

void DynamicDelay::process(float *out, const float *in, const float *delay, const float *fgain, const float *fdelay, size_t samples)   // :97-118
{
    handle *h = of(pData);
    if (h == nullptr || samples == 0 || !hand_over_head(h, nHead) || !h->buf.reserve(samples, 5))
        return;
    const mi_host::rows &b = h->buf;
    const float *staged[4] = { in, delay, fgain, fdelay };
    for (size_t k = 0; k < 4; ++k)
        if (!b.up(k + 1, staged[k], samples))
            return;
    const size_t cap = b.capacity();
    if (mi_dyndelay_bank_process(h->bank, b.row(0), b.row(1), b.row(2), b.row(3), b.row(4), samples, cap, cap, cap, cap, cap, nullptr) != MI_OK)
        return;
    nHead = uint32_t((size_t(nHead) + samples) % nCapacity);     // what the kernel leaves in the device's head
    h->head = nHead;
    b.down(out, 0, samples);
}

void DynamicDelay::copy(DynamicDelay *s)                        // :124-148
{
    handle *h = of(pData), *hs = (s != NULL) ? of(s->pData) : nullptr;
    if (h == nullptr || hs == nullptr || h == hs || !hand_over_head(hs, s->nHead))
        return;
    if (mi_dyndelay_bank_copy(h->bank, 0, hs->bank, 0, nullptr) != MI_OK)
        return;
    nHead = 0, h->head = 0;
}

void DynamicDelay::swap(DynamicDelay *d)                        // :150-157
{
    float *line = vDelay;           vDelay = d->vDelay;         d->vDelay = line;
    uint32_t head = nHead;          nHead = d->nHead;           d->nHead = head;
    uint32_t capacity = nCapacity;  nCapacity = d->nCapacity;   d->nCapacity = capacity;
    int32_t max_delay = nMaxDelay;  nMaxDelay = d->nMaxDelay;   d->nMaxDelay = max_delay;
    uint8_t *data = pData;          pData = d->pData;           d->pData = data;
}

void DynamicDelay::dump(IStateDumper *v) const                  // :159-166
{
    v->write("vDelay", vDelay);
    v->write("nHead", nHead);
    v->write("nCapacity", nCapacity);
    v->write("nMaxDelay", nMaxDelay);
    v->write("pData", pData);
}

} // namespace dspu
} // namespace lsp
