// lsp::dspu::Expander (src/main/dynamics/Expander.cpp) on a mi_expander_bank of one channel, in the manner of
// host/compressor.cpp: the class has no member to hang the bank on (its 92 bytes are the reference's), so the bank and its
// staging buffers live in a table keyed by the object's address: made at the first call that needs the device, dropped in
// destroy() and in construct().  Before every device call the bank is handed the object's own fTau*, fReleaseThresh, nHold,
// sExp and bUpward; process() also sends fEnvelope, fPeak and nHoldCounter when they are not what it read back after the
// previous call, and reads them back afterwards.
#include <lsp-plug.in/dsp-units/dynamics/Expander.h>

#include <cmath>
#include <cstring>
#include <mutex>
#include <new>
#include <unordered_map>

#include "expander_bank.h"

namespace lsp
{
namespace dspu
{
namespace
{
    struct expander_impl
    {
        mi_expander_bank_t *bank = nullptr;
        float  *d_buf = nullptr;            // [2][cap]: the staged input (gain in place on it), the envelope
        size_t  cap = 0;
        float   e = 0.0f, peak = 0.0f;      // the follower's state as the device holds it
        uint32_t hold = 0;

        bool reserve(size_t n)
        {
            if (n <= cap)
                return true;
            mi_dspu_free(d_buf);
            d_buf = nullptr;
            cap = 0;
            if (mi_dspu_malloc(reinterpret_cast<void **>(&d_buf), 2 * n * sizeof(float)) != MI_OK)
                return false;
            cap = n;
            return true;
        }
    };

    std::mutex g_lock;
    std::unordered_map<const void *, expander_impl *> &table()
    {
        static std::unordered_map<const void *, expander_impl *> t;
        return t;
    }

    expander_impl *impl_of(const void *self, bool make)
    {
        std::lock_guard<std::mutex> guard(g_lock);
        auto it = table().find(self);
        if (it != table().end())
            return it->second;
        if (!make)
            return nullptr;
        expander_impl *p = new (std::nothrow) expander_impl();
        if (p == nullptr)
            return nullptr;
        if (mi_expander_bank_create(&p->bank, 1) != MI_OK)
        {
            delete p;
            return nullptr;
        }
        table()[self] = p;
        return p;
    }

    void drop(const void *self)
    {
        expander_impl *p = nullptr;
        {
            std::lock_guard<std::mutex> guard(g_lock);
            auto it = table().find(self);
            if (it == table().end())
                return;
            p = it->second;
            table().erase(it);
        }
        mi_expander_bank_destroy(p->bank);
        mi_dspu_free(p->d_buf);
        delete p;
    }

    // the object's computed fields as the bank's channel 0
    bool hand_over(expander_impl *p, float ta, float tr, float rt, uint32_t hold, const dsp::expander_knee_t &k, bool upward)
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

    // the object's follower state as the bank's, where the fields are not what the device holds
    bool hand_over_state(expander_impl *p, float e, float peak, uint32_t hold)
    {
        if (memcmp(&e, &p->e, sizeof(e)) == 0 && memcmp(&peak, &p->peak, sizeof(peak)) == 0 && hold == p->hold)
            return true;
        if (mi::expander_bank_set_state(p->bank, 0, e, peak, hold, nullptr) != MI_OK)
            return false;
        p->e = e, p->peak = peak, p->hold = hold;
        return true;
    }
}

Expander::Expander()  { construct(); }
Expander::~Expander() { destroy(); }

void Expander::construct()                                      // Expander.cpp:70-101
{
    drop(this);                                                 // whatever lived at this address before
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
    drop(this);
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
    expander_impl *p = impl_of(this, true);
    if (p == nullptr || samples == 0 || !p->reserve(samples) ||
        !hand_over(p, fTauAttack, fTauRelease, fReleaseThresh, nHold, sExp, bUpward) ||
        !hand_over_state(p, fEnvelope, fPeak, uint32_t(nHoldCounter)))
        return;
    float *d_in = p->d_buf, *d_env = p->d_buf + p->cap;
    if (mi_dspu_copy_h2d(d_in, in, samples * sizeof(float), nullptr) != MI_OK ||
        mi_expander_bank_process(p->bank, d_in, (env != nullptr) ? d_env : nullptr, d_in, samples, samples, samples, samples, nullptr) != MI_OK ||
        mi_dspu_copy_d2h(out, d_in, samples * sizeof(float), nullptr) != MI_OK)
        return;
    if (env != nullptr && mi_dspu_copy_d2h(env, d_env, samples * sizeof(float), nullptr) != MI_OK)
        return;
    if (mi_expander_bank_get_state(p->bank, 0, &p->e, &p->peak, &p->hold, nullptr) != MI_OK)
        return;
    fEnvelope = p->e, fPeak = p->peak, nHoldCounter = p->hold;
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
    expander_impl *p = impl_of(this, true);
    if (p == nullptr || dots == 0 || !p->reserve(dots) ||
        !hand_over(p, fTauAttack, fTauRelease, fReleaseThresh, nHold, sExp, bUpward))
        return;
    if (mi_dspu_copy_h2d(p->d_buf, in, dots * sizeof(float), nullptr) == MI_OK &&
        mi_expander_bank_curve(p->bank, p->d_buf, p->d_buf, dots, dots, dots, nullptr) == MI_OK &&
        mi_dspu_copy_d2h(out, p->d_buf, dots * sizeof(float), nullptr) == MI_OK)
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
