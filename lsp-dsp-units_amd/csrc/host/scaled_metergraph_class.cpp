// lsp::dspu::ScaledMeterGraph (src/main/util/ScaledMeterGraph.cpp) on a mi_scaled_metergraph_bank of one channel kept beside the
// object (beside.h).  The object's fields and its two host rings are what counts.  process(float), update_period() and the
// setters are the reference's host work on them (the folds are scaled_metergraph_bank.h's, the ones the kernels run).  The array
// forms hand the settings, the state words and both rings to the bank where they differ from what it holds, run the kernel on the
// staged row, and bring every state word and both rings back, so the object is left as the reference leaves it.
#include <lsp-plug.in/dsp-units/util/ScaledMeterGraph.h>

#include <cmath>
#include <cstddef>

#include "beside.h"
#include "../scaled_metergraph_bank.h"

namespace lsp
{
namespace dspu
{
namespace
{
    namespace sm = mi_scaled_metergraph;

    // what the bank of one channel holds: its geometry, the settings, the state as the last call read it back, and whether its
    // rings are the object's (fill() changes words without moving a head or a count)
    struct graph_held
    {
        uint32_t frames = 0, subsampling = 0, max_period = 0, period = 0, method = 0, rings_differ = 1;
        mi_scaled_metergraph_state_t state = { 0.0f, 0, 0, 0.0f, 0, 0, 0 };
    };

    typedef mi_host::registry<mi_host::beside<mi_scaled_metergraph_bank_t, graph_held, mi_scaled_metergraph_bank_destroy> > graphs;

    static_assert(sizeof(ScaledMeterGraph) == 96, "sizeof(ScaledMeterGraph)");

    void rings_changed(const void *self)
    {
        graphs::entry *p = graphs::find(self);
        if (p != nullptr)
            p->held.rings_differ = 1;
    }

    // the head of a ring as the reference counts it: this library's RawRingBuffer may stand AT its capacity (RawRingBuffer.h)
    uint32_t head_of(const RawRingBuffer &r)    { return uint32_t(r.position() % r.size()); }

    void take_ring(RawRingBuffer &r, uint32_t head)
    {
        r.reset();
        r.advance(head);
    }

    // init()'s limits: where the reference is undefined, and what the bank counts in 32 bits
    bool defined(size_t frames, size_t subsampling, size_t max_period)
    {
        const size_t limit = size_t(1) << 31;
        return frames >= 1 && subsampling >= 1 && max_period >= subsampling && max_period < limit && frames < limit && frames * max_period < limit;
    }
}

ScaledMeterGraph::ScaledMeterGraph()    { construct(); }
ScaledMeterGraph::~ScaledMeterGraph()   { destroy(); }

void ScaledMeterGraph::construct()                              // :42-59
{
    graphs::drop(this);                                         // whatever lived at this address before
    sHistory.sBuffer.construct();
    sHistory.fCurrent = 0.0f;
    sHistory.nCount = 0;
    sHistory.nPeriod = 0;
    sHistory.nFrames = 0;
    sFrames.sBuffer.construct();
    sFrames.fCurrent = 0.0f;
    sFrames.nCount = 0;
    sFrames.nPeriod = 0;
    sFrames.nFrames = 0;
    nPeriod = 0;
    nMaxPeriod = 0;
    enMethod = MM_ABS_MAXIMUM;
}

void ScaledMeterGraph::destroy()                                // :61-65
{
    graphs::drop(this);
    sHistory.sBuffer.destroy();
    sFrames.sBuffer.destroy();
}

bool ScaledMeterGraph::init(size_t frames, size_t subsampling, size_t max_period)      // :67-91
{
    if (!defined(frames, subsampling, max_period))              // refused before anything is touched
        return false;
    const size_t subframes = (frames * max_period + subsampling - 1) / subsampling;
    if (!sHistory.sBuffer.init(subframes + sm::FRAMES_GAP))
        return false;
    if (!sFrames.sBuffer.init(frames + sm::FRAMES_GAP))
        return false;
    sHistory.nFrames = uint32_t(subframes);
    sHistory.nPeriod = uint32_t(subsampling);
    sHistory.fCurrent = 0.0f;
    sHistory.nCount = 0;
    sFrames.nFrames = uint32_t(frames);
    sFrames.nPeriod = 0;
    sFrames.fCurrent = 0.0f;
    sFrames.nCount = 0;
    nPeriod = 0;
    nMaxPeriod = uint32_t(max_period);
    rings_changed(this);
    return true;
}

void ScaledMeterGraph::set_period(size_t period)                // :93-96
{
    nPeriod = sm::limit_period(period, sHistory.nPeriod, nMaxPeriod);
}

void ScaledMeterGraph::set_method(meter_method_t m)             // :98-101
{
    enMethod = m;
}

void ScaledMeterGraph::process_sampler(sampler_t *sampler, float sample)       // :103-145
{
    float pushed;
    sampler->fCurrent = sm::fold_single(uint32_t(enMethod), sampler->fCurrent, sampler->nCount, sample, &pushed);
    if ((++sampler->nCount) >= sampler->nPeriod)                // :140
    {
        sampler->sBuffer.push(pushed);                          // :142: the sample, not fCurrent
        sampler->nCount = 0;
    }
}

bool ScaledMeterGraph::update_period()                          // :269-342
{
    if (nPeriod == sFrames.nPeriod)
        return false;
    if (sHistory.nCount > 0)
    {
        sHistory.sBuffer.push(sHistory.fCurrent);
        sHistory.nCount = 0;
    }
    else if (sFrames.nCount > 0)
        sHistory.sBuffer.push(sFrames.fCurrent);
    sFrames.nCount = 0;
    sFrames.nPeriod = nPeriod;
    sFrames.fCurrent = -1.0f;
    const size_t subsamples = sm::subsamples(sFrames.nPeriod, sFrames.nFrames, sHistory.nPeriod);
    sFrames.sBuffer.reset();
    for (size_t i = 0; i < subsamples; ++i)
    {
        sFrames.fCurrent = sm::fold_sub(uint32_t(enMethod), sFrames.fCurrent, sHistory.sBuffer.read(subsamples - i));
        sFrames.nCount += sHistory.nPeriod;
        if (sFrames.nCount >= sFrames.nPeriod)                  // :333
        {
            sFrames.sBuffer.push(sFrames.fCurrent);
            sFrames.nCount -= sFrames.nPeriod;
            sFrames.fCurrent = -1.0f;
        }
    }
    return true;
}

void ScaledMeterGraph::process(float sample)                    // :344-349
{
    if (sFrames.nFrames == 0)                                   // no rings: the reference's push divides by a capacity of 0
        return;
    process_sampler(&sHistory, sample);
    if (!update_period())
        process_sampler(&sFrames, sample);
}

namespace
{
    struct graph_fields
    {
        RawRingBuffer *history, *ring;
        uint32_t frames, subframes, subsampling, max_period, period, method;
        mi_scaled_metergraph_state_t state;
    };

    // The array forms, :351-363, through the bank: false where nothing could be done (the object is left as it was).
    bool run(const void *self, graph_fields &g, const float *s, const float *gain, size_t n)
    {
        graphs::entry *p = graphs::of(self, [&g](graphs::entry &e) { return mi_scaled_metergraph_bank_create(&e.bank, 1, g.frames, g.subframes); });
        if (p == nullptr)
            return false;
        graph_held &h = p->held;
        if (h.frames != g.frames || h.subsampling != g.subsampling || h.max_period != g.max_period)
        {
            if (h.frames != 0)                                  // a bank of another geometry: made anew
            {
                mi_scaled_metergraph_bank_destroy(p->bank);
                p->bank = nullptr;
                h = graph_held();
                if (mi_scaled_metergraph_bank_create(&p->bank, 1, g.frames, g.subframes) != MI_OK)
                    return false;
            }
            if (mi_scaled_metergraph_bank_init(p->bank, 0, g.frames, g.subsampling, g.max_period) != MI_OK)
                return false;
            h.frames = g.frames, h.subsampling = g.subsampling, h.max_period = g.max_period;
        }
        if (h.period != g.period)
        {
            if (mi_scaled_metergraph_bank_set_period(p->bank, 0, g.period) != MI_OK)
                return false;
            h.period = g.period;
        }
        if (h.method != g.method)
        {
            if (mi_scaled_metergraph_bank_set_method(p->bank, 0, g.method) != MI_OK)
                return false;
            h.method = g.method;
        }
        if (h.rings_differ || memcmp(&h.state, &g.state, sizeof(g.state)) != 0)
        {
            if (mi_scaled_metergraph_bank_set_state(p->bank, 0, &g.state, g.history->begin(), g.ring->begin(), nullptr) != MI_OK)
                return false;
            h.state = g.state, h.rings_differ = 0;
        }
        if (!p->buf.reserve(n, 2))
            return false;
        mi_scaled_metergraph_state_t after;
        h.rings_differ = 1;                                     // until everything is back
        if (!p->buf.up(0, s, n) ||
            (gain != nullptr && !p->buf.up(1, gain, 1)) ||
            mi_scaled_metergraph_bank_process(p->bank, p->buf.row(0), (gain != nullptr) ? p->buf.row(1) : nullptr, n, n, nullptr) != MI_OK ||
            mi_scaled_metergraph_bank_get_state(p->bank, 0, &after, g.history->begin(), g.ring->begin(), nullptr) != MI_OK)
            return false;
        h.state = g.state = after, h.rings_differ = 0;
        return true;
    }
}

void ScaledMeterGraph::process(const float *s, size_t count)    // :351-356
{
    process_block(s, nullptr, count);
}

void ScaledMeterGraph::process(const float *s, float gain, size_t count)       // :358-363
{
    process_block(s, &gain, count);
}

void ScaledMeterGraph::process_block(const float *s, const float *gain, size_t count)
{
    // Nothing is done without rings, beyond what the kernel counts in 32 bits, or before any set_period(): with
    // sFrames.nPeriod == 0 the reference's loop never ends (:152).  Without samples only update_period() is left of the call.
    if (sFrames.nFrames == 0 || nPeriod == 0 || count >= (size_t(1) << 31))
        return;
    if (count == 0)
    {
        if (update_period())
            rings_changed(this);
        return;
    }
    graph_fields g = { &sHistory.sBuffer, &sFrames.sBuffer, sFrames.nFrames, sHistory.nFrames, sHistory.nPeriod, nMaxPeriod, nPeriod, uint32_t(enMethod),
                       { sHistory.fCurrent, sHistory.nCount, head_of(sHistory.sBuffer), sFrames.fCurrent, sFrames.nCount, head_of(sFrames.sBuffer),
                         sFrames.nPeriod } };
    if (!run(this, g, s, gain, count))
        return;
    sHistory.fCurrent = g.state.history_current, sHistory.nCount = g.state.history_count;
    sFrames.fCurrent = g.state.frames_current, sFrames.nCount = g.state.frames_count, sFrames.nPeriod = g.state.frames_period;
    take_ring(sHistory.sBuffer, g.state.history_head);
    take_ring(sFrames.sBuffer, g.state.frames_head);
}

void ScaledMeterGraph::read(float *dst, size_t count)           // :365-369
{
    count = (count < sFrames.nFrames) ? count : sFrames.nFrames;
    sFrames.sBuffer.read(dst, count, count);
}

float ScaledMeterGraph::level() const                           // :371-374
{
    return (sFrames.sBuffer.size() != 0) ? sFrames.sBuffer.read(1) : 0.0f;
}

void ScaledMeterGraph::fill(float level)                        // :376-383
{
    sFrames.sBuffer.fill(level);
    sFrames.nCount = 0;
    sHistory.sBuffer.fill(level);
    sHistory.nCount = 0;
    rings_changed(this);
}

void ScaledMeterGraph::dump(IStateDumper *v) const              // :385-406
{
    const sampler_t *both[2] = { &sHistory, &sFrames };
    const char *names[2] = { "sHistory", "sFrames" };
    for (int i = 0; i < 2; ++i)
    {
        v->begin_object(names[i], both[i], sizeof(sampler_t));
        v->write_object("sBuffer", &both[i]->sBuffer);
        v->write("fCurrent", both[i]->fCurrent);
        v->write("nCount", both[i]->nCount);
        v->write("nPeriod", both[i]->nPeriod);
        v->write("nFrames", both[i]->nFrames);
        v->end_object();
    }
    v->write("nPeriod", nPeriod);
    v->write("nMaxPeriod", nMaxPeriod);
    v->write("enMethod", enMethod);
}

} // namespace dspu
} // namespace lsp
