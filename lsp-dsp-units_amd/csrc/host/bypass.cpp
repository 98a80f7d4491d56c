// lsp::dspu::Bypass (src/main/ctl/Bypass.cpp) on a mi_bypass_bank of one channel kept beside the object (beside.h).  The
// object's fields are what counts: init(), set_bypass() and bypassing() are host code on them as in the reference; before a
// device call the bank is handed nState, fDelta and fGain where they are not what the previous call read back, and afterwards
// the three are read back.
#include <lsp-plug.in/dsp-units/ctl/Bypass.h>
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
    struct bypass_held { uint32_t state = MI_BYPASS_OFF; float delta = 0.0f, gain = 0.0f; };
    typedef mi_host::registry<mi_host::beside<mi_bypass_bank_t, bypass_held, mi_bypass_bank_destroy> > bypasses;

    int send_state(mi_bypass_bank_t *bank, const bypass_held &now)
    {
        const mi_bypass_state_t s = { now.state, now.delta, now.gain };
        return mi_bypass_bank_set_state(bank, 0, &s, nullptr);
    }

    enum { PROCESS, PROCESS_WET, PROCESS_DRYWET };

    // one of the three process calls on host rows; *held: the object's three fields, in and out
    void run(const void *self, int variant, float *dst, const float *dry, const float *wet, float dry_gain, float wet_gain, size_t count,
             bypass_held *fields)
    {
        bypasses::entry *p = bypasses::of_one(self, mi_bypass_bank_create);
        if (p == nullptr || !p->hand_over_state(*fields, send_state) || !p->buf.reserve(count, 3))
            return;
        float *d_dst = p->buf.row(0), *d_wet = p->buf.row(1), *d_dry = (dry != NULL) ? p->buf.row(2) : NULL;
        if (!p->buf.up(1, wet, count) || (dry != NULL && !p->buf.up(2, dry, count)))
            return;
        const int r = (variant == PROCESS) ? mi_bypass_bank_process(p->bank, d_dst, d_dry, d_wet, count, count, count, count, nullptr) :
                      (variant == PROCESS_WET) ? mi_bypass_bank_process_wet(p->bank, d_dst, d_dry, d_wet, wet_gain, count, count, count, count, nullptr) :
                      mi_bypass_bank_process_drywet(p->bank, d_dst, d_dry, d_wet, dry_gain, wet_gain, count, count, count, count, nullptr);
        mi_bypass_state_t s;
        if (r != MI_OK || !p->buf.down(dst, 0, count) ||
            mi_bypass_bank_get_state(p->bank, 0, &s, nullptr) != MI_OK)
            return;
        p->held = bypass_held{ s.state, s.delta, s.gain };
        *fields = p->held;
    }

    static_assert(sizeof(Bypass) == 12, "sizeof(Bypass)");
}

Bypass::Bypass()    { construct(); }
Bypass::~Bypass()   { destroy(); }

void Bypass::construct()                                        // :39-44
{
    bypasses::drop(this);                                       // whatever lived at this address before
    nState = S_OFF;
    fDelta = 0.0f;
    fGain = 0.0f;
}

void Bypass::destroy()                                          // :46-51
{
    bypasses::drop(this);
    nState = S_OFF;
    fDelta = 0.0f;
    fGain = 0.0f;
}

bool Bypass::bypassing() const                                  // :84-93
{
    return nState == S_ON || (nState == S_ACTIVE && fDelta < 0.0f);
}

bool Bypass::set_bypass(bool bypass)                            // :53-82
{
    // a final state turns active, an active one only turns round; either way the step changes its sign
    const bool valid = nState == S_ON || nState == S_ACTIVE || nState == S_OFF;
    if (!valid || bypass == bypassing())
        return false;
    nState = S_ACTIVE;
    fDelta = -fDelta;
    return true;
}

void Bypass::init(int sample_rate, float time)                  // :95-104
{
    // all float32, and defined for every input: a NaN length stays NaN (NaN < 1 is false), as in the reference
    const float samples = float(sample_rate) * time;
    nState = S_OFF;
    fDelta = 1.0f / ((samples < 1.0f) ? 1.0f : samples);
    fGain = 1.0f;
}

void Bypass::process(float *dst, const float *dry, const float *wet, size_t count)                              // :106-206
{
    if (count == 0)
        return;
    bypass_held f = { uint32_t(nState), fDelta, fGain };
    run(this, PROCESS, dst, dry, wet, 1.0f, 1.0f, count, &f);
    nState = state_t(f.state), fDelta = f.delta, fGain = f.gain;
}

void Bypass::process_wet(float *dst, const float *dry, const float *wet, float wet_gain, size_t count)          // :208-308
{
    if (count == 0)
        return;
    bypass_held f = { uint32_t(nState), fDelta, fGain };
    run(this, PROCESS_WET, dst, dry, wet, 1.0f, wet_gain, count, &f);
    nState = state_t(f.state), fDelta = f.delta, fGain = f.gain;
}

void Bypass::process_drywet(float *dst, const float *dry, const float *wet, float dry_gain, float wet_gain, size_t count)    // :310-410
{
    if (count == 0)
        return;
    bypass_held f = { uint32_t(nState), fDelta, fGain };
    run(this, PROCESS_DRYWET, dst, dry, wet, dry_gain, wet_gain, count, &f);
    nState = state_t(f.state), fDelta = f.delta, fGain = f.gain;
}

void Bypass::dump(IStateDumper *v) const                        // :412-417
{
    v->write("nState", nState);
    v->write("fDelta", fDelta);
    v->write("fGain", fGain);
}

} // namespace dspu
} // namespace lsp
