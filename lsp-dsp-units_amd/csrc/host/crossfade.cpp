// lsp::dspu::Crossfade (src/main/ctl/Crossfade.cpp) on a mi_crossfade_bank of one channel kept beside the object (beside.h).
// The object's fields are what counts: init(), toggle() and reset() are host code on them as in the reference; before a device
// call the bank is handed nCounter, fDelta and fGain where they are not what the previous call read back, and afterwards the
// three are read back.
#include <lsp-plug.in/dsp-units/ctl/Crossfade.h>
#include <lsp-plug.in/dsp-units/units.h>

#include <cstddef>

#include "beside.h"

#pragma clang fp contract(off)

namespace lsp
{
namespace dspu
{
namespace
{
    // a fresh bank's state is construct()'s
    struct fade_held { uint32_t counter = 0; float delta = 0.0f, gain = 1.0f; };
    typedef mi_host::registry<mi_host::beside<mi_crossfade_bank_t, fade_held, mi_crossfade_bank_destroy> > crossfades;

    int send_state(mi_crossfade_bank_t *bank, const fade_held &now)
    {
        const mi_crossfade_state_t s = { now.counter, now.delta, now.gain };
        return mi_crossfade_bank_set_state(bank, 0, &s, nullptr);
    }

    static_assert(sizeof(Crossfade) == 24, "sizeof(Crossfade)");
}

Crossfade::Crossfade()  { construct(); }
Crossfade::~Crossfade() { destroy(); }

void Crossfade::construct()                                     // :39-45
{
    crossfades::drop(this);                                     // whatever lived at this address before
    nSamples = 0;
    nCounter = 0;
    fDelta = 0.0f;
    fGain = 1.0f;
}

void Crossfade::destroy()                                       // :47-49
{
    crossfades::drop(this);
}

void Crossfade::init(int sample_rate, float time)               // :51-55
{
    // ssize_t(float) is undefined for NaN and from 2^63 on, and the bank counts in 32 bits: clamped here into [1, 2^32 - 1],
    // NaN to 1, as PeakMeter::update_settings clamps its hold time
    const float samples = float(sample_rate) * time;
    nSamples = !(samples >= 1.0f) ? 1u : (samples >= 4294967296.0f) ? size_t(UINT32_MAX) : size_t(samples);
}

bool Crossfade::toggle()                                        // :57-67
{
    if (active())
        return false;
    nCounter = nSamples;
    fDelta = 1.0f / float(nSamples);
    fGain = 0.0f;
    return true;
}

void Crossfade::reset()                                         // :69-74
{
    nCounter = 0;
    fDelta = 0.0f;
    fGain = 0.0f;
}

void Crossfade::process(float *dst, const float *fade_out, const float *fade_in, size_t count)     // :76-156
{
    if (count == 0)
        return;
    crossfades::entry *p = crossfades::of_one(this, mi_crossfade_bank_create);
    // a counter set beyond 32 bits through a derived class is beyond every block as well
    const fade_held now = { (nCounter < size_t(UINT32_MAX)) ? uint32_t(nCounter) : UINT32_MAX, fDelta, fGain };
    if (p == nullptr || !p->hand_over_state(now, send_state) || !p->buf.reserve(count, 3))
        return;
    float *d_dst = p->buf.row(0), *d_out = (fade_out != NULL) ? p->buf.row(1) : NULL, *d_in = (fade_in != NULL) ? p->buf.row(2) : NULL;
    mi_crossfade_state_t s;
    if ((fade_out != NULL && !p->buf.up(1, fade_out, count)) ||
        (fade_in != NULL && !p->buf.up(2, fade_in, count)) ||
        mi_crossfade_bank_process(p->bank, d_dst, d_out, d_in, count, count, count, count, nullptr) != MI_OK ||
        !p->buf.down(dst, 0, count) ||
        mi_crossfade_bank_get_state(p->bank, 0, &s, nullptr) != MI_OK)
        return;
    p->held = fade_held{ s.counter, s.delta, s.gain };
    nCounter = s.counter;
    fDelta = s.delta;
    fGain = s.gain;
}

void Crossfade::dump(IStateDumper *v) const                     // :158-164
{
    v->write("nSamples", nSamples);
    v->write("nCounter", nCounter);
    v->write("fDelta", fDelta);
    v->write("fGain", fGain);
}

} // namespace dspu
} // namespace lsp
