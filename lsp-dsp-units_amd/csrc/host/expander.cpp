// lsp::dspu::Expander (src/main/dynamics/Expander.cpp) on a mi_expander_bank of one channel.  The class has no
// member to hang the bank on (its 92 bytes are the reference's), so the bank and its staging buffers live beside the object
// (beside.h).  Before every device call the bank is handed the object's own fTau*, fReleaseThresh, nHold, sExp and bUpward;
// process() also sends fEnvelope, fPeak and nHoldCounter when they are not what it read back after the previous call, and
// reads them back afterwards.
#include <lsp-plug.in/dsp-units/dynamics/Expander.h>

#include <cmath>
#include <cstring>

#include "beside.h"
#include "expander_bank.h"

namespace lsp
{
namespace dspu
{
namespace
{
    typedef mi_host::registry<mi_host::beside<mi_expander_bank_t, mi_host::follow_held, mi_expander_bank_destroy> > besides;

    // the object's computed fields as the bank's channel 0
    bool hand_over(besides::entry *p, float ta, float tr, float rt, uint32_t hold, const dsp::expander_knee_t &k, bool upward)
    {
        mi_expander_params_t q;
        q.tau_attack = ta;
        q.tau_release = tr;
        q.release_threshold = rt;
        q.hold = hold;
        static_assert(sizeof(k) == sizeof(q.k), "knee layouts");
        memcpy(&q.k, &k, sizeof(q.k));
        q.upward = upward ? 1 : 0;
        return mi::expander_bank_set_params(p->bank, 0, &q) == MI_OK;
    }

    int send_state(mi_expander_bank_t *bank, const mi_host::follow_held &s)
    {
        return mi::expander_bank_set_state(bank, 0, s.e, s.peak, s.hold, nullptr);
    }
}

Expander::Expander()  { construct(); }
Expander::~Expander() { destroy(); }

void Expander::construct()                                      // Expander.cpp:70-101
{
    besides::drop(this);                                        // whatever lived at this address before
    fAttackThresh = 0.0f;
    fReleaseThresh = 0.0f;
    fAttack = 0.0f;
    fRelease = 0.0f;
    fKnee = 0.0f;
    fRatio = 1.0f;
    fEnvelope = 0.0f;
    fHold = 0.0f;
    fPeak = 0.0f;
    fTauAttack = 0.0f;
    fTauRelease = 0.0f;
    sExp.start = 0.0f;
    sExp.end = 0.0f;
    sExp.threshold = 0.0f;
    sExp.herm[0] = sExp.herm[1] = sExp.herm[2] = 0.0f;
    sExp.tilt[0] = sExp.tilt[1] = 0.0f;
    nHold = 0;
    nHoldCounter = 0;
    nSampleRate = 0;
    bUpdate = true;
    bUpward = true;
}

void Expander::destroy()                                        // :103-105
{
    besides::drop(this);
}

void Expander::update_settings()                                // :200-245
{
    if (!bUpdate)
        return;
    mi_expander_settings_t s;
    s.sample_rate = nSampleRate;
    s.mode = bUpward ? MI_EM_UPWARD : MI_EM_DOWNWARD;
    s.attack_threshold = fAttackThresh;
    s.release_threshold = fReleaseThresh;
    s.attack = fAttack;
    s.release = fRelease;
    s.hold = fHold;
    s.knee = fKnee;
    s.ratio = fRatio;
    mi_expander_params_t p;
    mi_expander_compute_params(&s, &p);
    fTauAttack = p.tau_attack;
    fTauRelease = p.tau_release;
    nHold = p.hold;
    static_assert(sizeof(sExp) == sizeof(p.k), "knee layouts");
    memcpy(&sExp, &p.k, sizeof(sExp));
    bUpdate = false;
}

void Expander::process(float *out, float *env, const float *in, size_t samples)        // :247-292
{
    update_settings();
    besides::entry *p = besides::of_one(this, mi_expander_bank_create);
    if (p == nullptr || samples == 0 || !p->buf.reserve(samples, 2) ||
        !hand_over(p, fTauAttack, fTauRelease, fReleaseThresh, nHold, sExp, bUpward) ||
        !p->hand_over_state({ fEnvelope, fPeak, uint32_t(nHoldCounter) }, send_state))
        return;
    float *d_in = p->buf.row(0), *d_env = p->buf.row(1);
    if (!p->buf.up(0, in, samples) ||
        mi_expander_bank_process(p->bank, d_in, (env != nullptr) ? d_env : nullptr, d_in, samples, samples, samples, samples, nullptr) != MI_OK ||
        !p->buf.down(out, 0, samples))
        return;
    if (env != nullptr && !p->buf.down(env, 1, samples))
        return;
    if (mi_expander_bank_get_state(p->bank, 0, &p->held.e, &p->held.peak, &p->held.hold, nullptr) != MI_OK)
        return;
    fEnvelope = p->held.e, fPeak = p->held.peak, nHoldCounter = p->held.hold;
}

float Expander::process(float *env, float s)                    // :294-323: one sample on the device
{
    float out = 0.0f, e = 0.0f;
    process(&out, &e, &s, 1);
    if (env != NULL)
        *env = e;
    return out;
}

void Expander::curve(float *out, const float *in, size_t dots)                          // :325-331
{
    besides::entry *p = besides::of_one(this, mi_expander_bank_create);
    if (p == nullptr || dots == 0 || !p->buf.reserve(dots, 2) ||
        !hand_over(p, fTauAttack, fTauRelease, fReleaseThresh, nHold, sExp, bUpward))
        return;
    if (p->buf.up(0, in, dots) &&
        mi_expander_bank_curve(p->bank, p->buf.row(0), p->buf.row(0), dots, dots, dots, nullptr) == MI_OK &&
        p->buf.down(out, 0, dots))
        mi_dspu_stream_synchronize(nullptr);
}

float Expander::curve(float in)                                 // :333-365
{
    float x = fabsf(in);
    if (bUpward)
    {
        if (x > sExp.threshold)
            x = sExp.threshold;
        if (x > sExp.start)
        {
            const float lx = logf(x);
            return (x >= sExp.end) ? x * expf(sExp.tilt[0] * lx + sExp.tilt[1]) :
                   x * expf((sExp.herm[0] * lx + sExp.herm[1]) * lx + sExp.herm[2]);
        }
    }
    else
    {
        if (x < sExp.threshold)
            return 0.0f;
        if (x < sExp.end)
        {
            const float lx = logf(x);
            return (x <= sExp.start) ? x * expf(sExp.tilt[0] * lx + sExp.tilt[1]) :
                   x * expf((sExp.herm[0] * lx + sExp.herm[1]) * lx + sExp.herm[2]);
        }
    }
    return x;
}

void Expander::amplification(float *out, const float *in, size_t dots)                  // :367-373: the scalar form, dot by dot
{
    for (size_t i = 0; i < dots; ++i)
        out[i] = amplification(in[i]);
}

float Expander::amplification(float in)                         // :375-407
{
    float x = fabsf(in);
    if (bUpward)
    {
        if (x > sExp.threshold)
            x = sExp.threshold;
        if (x > sExp.start)
        {
            const float lx = logf(x);
            return (x >= sExp.end) ? expf(sExp.tilt[0] * lx + sExp.tilt[1]) :
                   expf((sExp.herm[0] * lx + sExp.herm[1]) * lx + sExp.herm[2]);
        }
    }
    else
    {
        if (x < sExp.threshold)
            return 0.0f;
        if (x < sExp.end)
        {
            const float lx = logf(x);
            return (x <= sExp.start) ? expf(sExp.tilt[0] * lx + sExp.tilt[1]) :
                   expf((sExp.herm[0] * lx + sExp.herm[1]) * lx + sExp.herm[2]);
        }
    }
    return 1.0f;
}

void Expander::set_attack_threshold(float threshold)            // :107-113
{
    if (fAttackThresh == threshold)
        return;
    fAttackThresh = threshold;
    bUpdate = true;
}

void Expander::set_release_threshold(float threshold)           // :115-121
{
    if (fReleaseThresh == threshold)
        return;
    fReleaseThresh = threshold;
    bUpdate = true;
}

void Expander::set_threshold(float attack, float release)       // :123-130
{
    if ((fAttackThresh == attack) && (fReleaseThresh == release))
        return;
    fAttackThresh = attack;
    fReleaseThresh = release;
    bUpdate = true;
}

void Expander::set_timings(float attack, float release)         // :132-139
{
    if ((fAttack == attack) && (fRelease == release))
        return;
    fAttack = attack;
    fRelease = release;
    bUpdate = true;
}

void Expander::set_attack(float attack)                         // :141-147
{
    if (fAttack == attack)
        return;
    fAttack = attack;
    bUpdate = true;
}

void Expander::set_release(float release)                       // :149-155
{
    if (fRelease == release)
        return;
    fRelease = release;
    bUpdate = true;
}

void Expander::set_sample_rate(size_t sr)                       // :157-163
{
    if (sr == nSampleRate)
        return;
    nSampleRate = uint32_t(sr);
    bUpdate = true;
}

void Expander::set_knee(float knee)                             // :165-171: no limits
{
    if (knee == fKnee)
        return;
    fKnee = knee;
    bUpdate = true;
}

void Expander::set_ratio(float ratio)                           // :173-179
{
    if (ratio == fRatio)
        return;
    bUpdate = true;
    fRatio = ratio;
}

void Expander::set_mode(size_t mode)                            // :181-189
{
    const bool upward = (mode == EM_UPWARD);
    if (upward == bUpward)
        return;
    bUpward = upward;
    bUpdate = true;
}

void Expander::set_hold(float hold)                             // :191-198
{
    hold = (hold > 0.0f) ? hold : 0.0f;
    if (hold == fHold)
        return;
    fHold = hold;
    bUpdate = true;
}

void Expander::dump(IStateDumper *v) const                      // :409-438
{
    v->write("fAttackThresh", fAttackThresh);
    v->write("fReleaseThresh", fReleaseThresh);
    v->write("fAttack", fAttack);
    v->write("fRelease", fRelease);
    v->write("fKnee", fKnee);
    v->write("fRatio", fRatio);
    v->write("fEnvelope", fEnvelope);
    v->write("fHold", fHold);
    v->write("fPeak", fPeak);
    v->write("fTauAttack", fTauAttack);
    v->write("fTauRelease", fTauRelease);
    v->begin_object("sExp", &sExp, sizeof(dsp::expander_knee_t));
    {
        v->write("start", sExp.start);
        v->write("end", sExp.end);
        v->write("thresh", sExp.threshold);
        v->writev("herm", sExp.herm, 3);
        v->writev("tilt", sExp.tilt, 2);
    }
    v->end_object();
    v->write("nHold", nHold);
    v->write("nHoldCounter", nHoldCounter);
    v->write("nSampleRate", nSampleRate);
    v->write("bUpdate", bUpdate);
    v->write("bUpward", bUpward);
}

} // namespace dspu
} // namespace lsp
