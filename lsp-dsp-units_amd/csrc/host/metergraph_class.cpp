// lsp::dspu::MeterGraph (src/main/util/MeterGraph.cpp) on a mi_metergraph_bank of one channel kept beside the object (beside.h).
// The object's fields are what counts.  process(float) is the reference's host work on them.  The array forms hand nPeriod,
// enMethod, fCurrent and nCount to the bank where they differ from what it holds, run the kernel on the staged row, read fCurrent
// and nCount back and append the frames that the call produced -- their number is a closed form of nCount, nPeriod and n
// (metergraph_bank.h) -- to sBuffer one by one, as the reference does.  The bank's own ring only carries those frames over.
#include <lsp-plug.in/dsp-units/util/MeterGraph.h>

#include <cmath>
#include <cstddef>
#include <vector>

#include "beside.h"
#include "../metergraph_bank.h"

namespace lsp
{
namespace dspu
{
namespace
{
    // what the bank of one channel holds: its ring's size, the settings, and the state that the last call read back
    struct graph_held { uint32_t frames = 0, period = 0, method = 0, count = 0, head = 0; float current = 0.0f; };

    typedef mi_host::registry<mi_host::beside<mi_metergraph_bank_t, graph_held, mi_metergraph_bank_destroy> > graphs;

    static_assert(sizeof(MeterGraph) == 40, "sizeof(MeterGraph)");

    // the bank of `self` with a ring of `frames` words and the object's settings and state on the device
    graphs::entry *ready(const void *self, uint32_t frames, uint32_t period, uint32_t method, float current, uint32_t count)
    {
        // a ring of 1 until the first call tells the size: held.frames is 0 then, and the bank is made anew just below
        graphs::entry *p = graphs::of(self, [](graphs::entry &e) { return mi_metergraph_bank_create(&e.bank, 1, 1); });
        if (p == nullptr)
            return nullptr;
        graph_held &h = p->held;
        if (h.frames != frames)
        {
            mi_metergraph_bank_destroy(p->bank);
            p->bank = nullptr;
            h = graph_held();
            if (mi_metergraph_bank_create(&p->bank, 1, frames) != MI_OK || mi_metergraph_bank_init(p->bank, 0, frames, period, 0.0f) != MI_OK)
                return nullptr;
            h.frames = frames, h.period = period;
        }
        if (h.period != period)
        {
            if (mi_metergraph_bank_set_period(p->bank, 0, period) != MI_OK)
                return nullptr;
            h.period = period;
        }
        if (h.method != method)
        {
            if (mi_metergraph_bank_set_method(p->bank, 0, method) != MI_OK)
                return nullptr;
            h.method = method;
        }
        if (memcmp(&h.current, &current, sizeof(float)) != 0 || h.count != count)
        {
            const mi_metergraph_state_t s = { current, count, h.head };
            if (mi_metergraph_bank_set_state(p->bank, 0, &s, nullptr, nullptr) != MI_OK)
                return nullptr;
            h.current = current, h.count = count;
        }
        return p;
    }
}

MeterGraph::MeterGraph()    { construct(); }
MeterGraph::~MeterGraph()   { destroy(); }

void MeterGraph::construct()                                    // :40-48 (fDefault is left as it is there too; 0 here)
{
    graphs::drop(this);                                         // whatever lived at this address before
    sBuffer.construct();
    fCurrent = 0.0f;
    fDefault = 0.0f;
    nCount = 0;
    nPeriod = 1;
    enMethod = MM_ABS_MAXIMUM;
}

void MeterGraph::destroy()                                      // :50-53
{
    graphs::drop(this);
    sBuffer.destroy();
}

bool MeterGraph::init(size_t frames, size_t period, float default_value)      // :55-68
{
    if (period <= 0)
        return false;
    if (!sBuffer.init(frames, default_value))
        return false;
    fCurrent = 0.0f;
    fDefault = default_value;
    nCount = 0;
    nPeriod = uint32_t(period);
    return true;
}

void MeterGraph::process(float sample)                          // :70-111
{
    fCurrent = (nCount == 0) ? mi_metergraph::first_single(uint32_t(enMethod), sample) :
                               mi_metergraph::fold_single(uint32_t(enMethod), fCurrent, sample);
    if ((++nCount) >= nPeriod)                                  // :105
    {
        sBuffer.append(fCurrent);
        nCount = 0;
    }
}

namespace
{
    // The array forms, :113-244.  A period of 0 makes the reference loop for ever (:118): nothing is done.  Neither without a
    // ring (the reference's append would divide by a capacity of 0) nor beyond what the kernel counts in 32 bits.
    struct outcome { bool ok; float current; uint32_t count; std::vector<float> frames; uint32_t appended; };

    outcome run(const void *self, const float *s, const float *gain, size_t n, uint32_t frames, uint32_t period, uint32_t method,
                float current, uint32_t count)
    {
        outcome o = { false, current, count, {}, 0 };
        graphs::entry *p = ready(self, frames, period, method, current, count);
        const size_t cap = (n > size_t(frames) + 1) ? n : size_t(frames) + 1;
        if (p == nullptr || !p->buf.reserve(cap, 2))
            return o;
        float *d_src = p->buf.row(0), *d_out = p->buf.row(1);
        const mi_metergraph::plan pl = mi_metergraph::make_plan(count, period, uint32_t(n));
        const uint32_t kept = (pl.frames < frames) ? pl.frames : frames;
        mi_metergraph_state_t st;
        o.frames.resize(kept);
        if (!p->buf.up(0, s, n) ||
            (gain != nullptr && mi_dspu_copy_h2d(d_out + frames, gain, sizeof(float), nullptr) != MI_OK) ||  // behind the frames; cap > frames
            mi_metergraph_bank_process(p->bank, d_src, (gain != nullptr) ? d_out + frames : nullptr, n, n, nullptr) != MI_OK ||
            (kept != 0 && mi_metergraph_bank_read(p->bank, d_out, kept, kept, nullptr) != MI_OK) ||
            (kept != 0 && !p->buf.down(o.frames.data(), 1, kept)) ||
            mi_metergraph_bank_get_state(p->bank, 0, &st, nullptr, nullptr) != MI_OK)
            return o;
        p->held.current = st.current, p->held.count = st.count, p->held.head = st.head;
        o.ok = true, o.current = st.current, o.count = st.count, o.appended = pl.frames;
        return o;
    }
}

namespace
{
    // frame j of the call lands in slot (nHead + j) % capacity: of more frames than the ring holds only the last `capacity` stay,
    // behind as many steps of the head as the others took
    void append_frames(RingBuffer &ring, const outcome &o, float filler)
    {
        const size_t kept = o.frames.size(), frames = ring.size();
        if (o.appended > kept)
            for (size_t i = 0, skipped = (o.appended - kept) % frames; i < skipped; ++i)
                ring.append(filler);
        for (size_t i = 0; i < kept; ++i)
            ring.append(o.frames[i]);
    }

    bool runs(size_t n, uint32_t period, size_t frames)    { return n != 0 && period != 0 && frames != 0 && n < (size_t(1) << 31); }
}

void MeterGraph::process(const float *s, size_t n)              // :113-178
{
    if (!runs(n, nPeriod, sBuffer.size()))
        return;
    const outcome o = run(this, s, nullptr, n, uint32_t(sBuffer.size()), nPeriod, uint32_t(enMethod), fCurrent, nCount);
    if (!o.ok)
        return;
    fCurrent = o.current;
    nCount = o.count;
    append_frames(sBuffer, o, fDefault);
}

void MeterGraph::process(const float *s, float gain, size_t n)  // :180-244
{
    if (!runs(n, nPeriod, sBuffer.size()))
        return;
    const outcome o = run(this, s, &gain, n, uint32_t(sBuffer.size()), nPeriod, uint32_t(enMethod), fCurrent, nCount);
    if (!o.ok)
        return;
    fCurrent = o.current;
    nCount = o.count;
    append_frames(sBuffer, o, fDefault);
}

void MeterGraph::read(float *dst, size_t count) const           // :246-258
{
    const ssize_t capacity = sBuffer.size();
    const ssize_t delta = ssize_t(count) - capacity;
    if (delta > 0)
    {
        for (ssize_t i = 0; i < delta; ++i)
            dst[i] = fDefault;
        dst += delta;
        count = capacity;
    }
    sBuffer.get(dst, count - 1, count);
}

void MeterGraph::dump(IStateDumper *v) const                    // :260-268
{
    v->write_object("sBuffer", &sBuffer);
    v->write("fCurrent", fCurrent);
    v->write("fDefault", fDefault);
    v->write("nCount", nCount);
    v->write("nPeriod", nPeriod);
    v->write("enMethod", enMethod);
}

} // namespace dspu
} // namespace lsp
