// lsp::dspu::SurgeProtector (src/main/dynamics/SurgeProtector.cpp) on a mi_surge_bank of one channel kept beside the object
// (beside.h).  The object's fields are what counts: the setters and reset() act on them at once, as in the reference; before
// every device call the bank is handed the two maxima and the two thresholds where they differ from its own, and fGain, the two
// counters and bOn where they are not what the previous call read back; afterwards the four are read back.
#include <lsp-plug.in/dsp-units/dynamics/SurgeProtector.h>

#include <cstddef>

#include "beside.h"

namespace lsp
{
namespace dspu
{
namespace
{
    struct surge_held { float gain = 0.0f; uint32_t transition = 0, shutdown = 0, on = 0; };
    typedef mi_host::registry<mi_host::beside<mi_surge_bank_t, surge_held, mi_surge_bank_destroy> > protectors;

    int send_state(mi_surge_bank_t *bank, const surge_held &now)
    {
        const mi_surge_state_t s = { now.gain, now.transition, now.shutdown, now.on };
        return mi_surge_bank_set_state(bank, 0, &s, nullptr);
    }

    // the device counts in 32 bits
    uint32_t narrow(size_t v)   { return (v < size_t(UINT32_MAX)) ? uint32_t(v) : UINT32_MAX; }

    static_assert(sizeof(void *) != 8 || sizeof(SurgeProtector) == 56, "sizeof(SurgeProtector)");
}

SurgeProtector::SurgeProtector()    { construct(); }
SurgeProtector::~SurgeProtector()   { destroy(); }

void SurgeProtector::construct()                                // :41-51
{
    protectors::drop(this);                                     // whatever lived at this address before
    fGain = 0.0f;
    nTransitionTime = nTransitionMax = 0;
    nShutdownTime = nShutdownMax = 0;
    fOnThreshold = fOffThreshold = 0.0f;
    bOn = false;
}

void SurgeProtector::destroy()                                  // :53-63
{
    protectors::drop(this);
    fGain = 0.0f;
    nTransitionTime = nTransitionMax = 0;
    nShutdownTime = nShutdownMax = 0;
    fOnThreshold = fOffThreshold = 0.0f;
    bOn = false;
}

void SurgeProtector::reset()                                    // :65-69
{
    bOn = false;
    nTransitionTime = 0;
}

void SurgeProtector::set_transition_time(size_t time)           // :71-75
{
    nTransitionMax = time;
    nTransitionTime = (nTransitionTime < time) ? nTransitionTime : time;
}

void SurgeProtector::set_shutdown_time(size_t time)             // :77-81
{
    nShutdownMax = time;
    nShutdownTime = (nShutdownTime < time) ? nShutdownTime : time;
}

void SurgeProtector::set_on_threshold(float threshold)      { fOnThreshold = threshold; }
void SurgeProtector::set_off_threshold(float threshold)     { fOffThreshold = threshold; }

void SurgeProtector::set_threshold(float on, float off)         // :93-97
{
    fOnThreshold = on;
    fOffThreshold = off;
}

namespace
{
    // the bank of `self` with the object's settings and state on the device
    protectors::entry *ready(const void *self, const mi_surge_params_t &want, const surge_held &now)
    {
        protectors::entry *p = protectors::of_one(self, mi_surge_bank_create);
        if (p == nullptr)
            return nullptr;
        mi_surge_params_t q;
        if (mi_surge_bank_get_params(p->bank, 0, &q) != MI_OK)
            return nullptr;
        if (q.transition_max != want.transition_max && mi_surge_bank_set_transition_time(p->bank, 0, want.transition_max) != MI_OK)
            return nullptr;
        if (q.shutdown_max != want.shutdown_max && mi_surge_bank_set_shutdown_time(p->bank, 0, want.shutdown_max) != MI_OK)
            return nullptr;
        if ((memcmp(&q.on_threshold, &want.on_threshold, sizeof(float)) != 0 || memcmp(&q.off_threshold, &want.off_threshold, sizeof(float)) != 0) &&
            mi_surge_bank_set_threshold(p->bank, 0, want.on_threshold, want.off_threshold) != MI_OK)
            return nullptr;
        if (q.transition_max != want.transition_max || q.shutdown_max != want.shutdown_max)
        {
            // the bank's setters have clamped ITS counters; what the device holds then is read, so that the object's state is
            // sent only where it differs
            mi_surge_state_t s;
            if (mi_surge_bank_get_state(p->bank, 0, &s, nullptr) != MI_OK)
                return nullptr;
            p->held = surge_held{ s.gain, s.transition_time, s.shutdown_time, s.on };
        }
        return p->hand_over_state(now, send_state) ? p : nullptr;
    }
}

float SurgeProtector::process(float in)                         // :99-149
{
    process(NULL, &in, 1);
    return fGain;
}

void SurgeProtector::process(const float *in, size_t samples)   // :151-155
{
    process(NULL, in, samples);
}

void SurgeProtector::process(float *out, const float *in, size_t samples)      // :157-167
{
    if (samples == 0)
        return;
    const mi_surge_params_t want = { narrow(nTransitionMax), narrow(nShutdownMax), fOnThreshold, fOffThreshold };
    protectors::entry *p = ready(this, want, surge_held{ fGain, narrow(nTransitionTime), narrow(nShutdownTime), bOn ? 1u : 0u });
    if (p == nullptr || !p->buf.reserve(samples, 2))
        return;
    float *d_in = p->buf.row(0), *d_out = p->buf.row(1);
    mi_surge_state_t s;
    if (!p->buf.up(0, in, samples) ||
        mi_surge_bank_process(p->bank, (out != NULL) ? d_out : NULL, d_in, samples, samples, samples, nullptr) != MI_OK ||
        (out != NULL && !p->buf.down(out, 1, samples)) ||
        mi_surge_bank_get_state(p->bank, 0, &s, nullptr) != MI_OK)
        return;
    p->held = surge_held{ s.gain, s.transition_time, s.shutdown_time, s.on };
    fGain = s.gain;
    nTransitionTime = s.transition_time;
    nShutdownTime = s.shutdown_time;
    bOn = s.on != 0;
}

void SurgeProtector::process_mul(float *out, const float *in, size_t samples)  // :169-179
{
    if (out == NULL)
    {
        process(in, samples);
        return;
    }
    if (samples == 0)
        return;
    const mi_surge_params_t want = { narrow(nTransitionMax), narrow(nShutdownMax), fOnThreshold, fOffThreshold };
    protectors::entry *p = ready(this, want, surge_held{ fGain, narrow(nTransitionTime), narrow(nShutdownTime), bOn ? 1u : 0u });
    if (p == nullptr || !p->buf.reserve(samples, 2))
        return;
    float *d_in = p->buf.row(0), *d_out = p->buf.row(1);
    mi_surge_state_t s;
    if (!p->buf.up(0, in, samples) || !p->buf.up(1, out, samples) ||
        mi_surge_bank_process_mul(p->bank, d_out, d_in, samples, samples, samples, nullptr) != MI_OK ||
        !p->buf.down(out, 1, samples) ||
        mi_surge_bank_get_state(p->bank, 0, &s, nullptr) != MI_OK)
        return;
    p->held = surge_held{ s.gain, s.transition_time, s.shutdown_time, s.on };
    fGain = s.gain;
    nTransitionTime = s.transition_time;
    nShutdownTime = s.shutdown_time;
    bOn = s.on != 0;
}

void SurgeProtector::dump(IStateDumper *v) const                // :181-191
{
    v->write("fGain", fGain);
    v->write("nTransitionTime", nTransitionTime);
    v->write("nTransitionMax", nTransitionMax);
    v->write("nShutdownTime", nShutdownTime);
    v->write("nShutdownMax", nShutdownMax);
    v->write("fOnThreshold", fOnThreshold);
    v->write("fOffThreshold", fOffThreshold);
    v->write("bOn", bOn);
}

} // namespace dspu
} // namespace lsp
