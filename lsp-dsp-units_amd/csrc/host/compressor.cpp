// lsp::dspu::Compressor (src/main/dynamics/Compressor.cpp) on a mi_compressor_bank of one channel.  The class has no member
// to hang the bank on (its 132 bytes are the reference's), so the bank and its staging buffers live beside the object
// (beside.h).  Before every device call the bank is handed the object's own fTau*, fReleaseThresh, nHold and sComp;
// process() also sends fEnvelope, fPeak and nHoldCounter when they are not what it read back after the previous call (a
// subclass may write the protected fields), and reads them back afterwards.
#include <lsp-plug.in/dsp-units/dynamics/Compressor.h>

#include <cmath>
#include <cstring>

#include "beside.h"
#include "compressor_bank.h"

namespace lsp
{
namespace dspu
{
namespace
{
    typedef mi_host::registry<mi_host::beside<mi_compressor_bank_t, mi_host::follow_held, mi_compressor_bank_destroy> > besides;

    inline float knee_gain(float x, float lx, const dsp::compressor_knee_t &k)     // Compressor.cpp:302-307
    {
        return (x <= k.start) ? k.gain :
               (x >= k.end) ? expf(lx * k.tilt[0] + k.tilt[1]) :
               expf((k.herm[0] * lx + k.herm[1]) * lx + k.herm[2]);
    }

    inline float x2_gain(float x, const dsp::compressor_x2_t &c)                    // :297-309, x = |input|
    {
        if ((x <= c.k[0].start) && (x <= c.k[1].start))
            return c.k[0].gain * c.k[1].gain;
        const float lx = logf(x);
        return knee_gain(x, lx, c.k[0]) * knee_gain(x, lx, c.k[1]);
    }
}

Compressor::Compressor()  { construct(); }
Compressor::~Compressor() { destroy(); }

void Compressor::construct()                                    // Compressor.cpp:46-83
{
    besides::drop(this);                                        // whatever lived at this address before
    fAttackThresh = 0.0f;
    fReleaseThresh = 0.0f;
    fBoostThresh = float(2.5119e-4);                            // GAIN_AMP_M_72_DB
    fAttack = 0.0f;
    fRelease = 0.0f;
    fKnee = 0.0f;
    fRatio = 1.0f;
    fHold = 0.0f;
    fEnvelope = 0.0f;
    fPeak = 0.0f;
    fTauAttack = 0.0f;
    fTauRelease = 0.0f;
    for (size_t i = 0; i < 2; ++i)
    {
        dsp::compressor_knee_t *k = &sComp.k[i];
        k->start = 0.0f;
        k->end = 0.0f;
        k->gain = 1.0f;
        k->herm[0] = k->herm[1] = k->herm[2] = 0.0f;
        k->tilt[0] = k->tilt[1] = 0.0f;
    }
    nHold = 0;
    nHoldCounter = 0;
    nSampleRate = 0;
    nMode = CM_DOWNWARD;
    bUpdate = true;
}

void Compressor::destroy()                                      // :85-87
{
    besides::drop(this);
}

void Compressor::update_settings()                              // :89-220
{
    if (!bUpdate)
        return;
    mi_compressor_settings_t s;
    s.sample_rate = nSampleRate;
    s.mode = nMode;
    s.attack_threshold = fAttackThresh;
    s.release_threshold = fReleaseThresh;
    s.boost_threshold = fBoostThresh;
    s.attack = fAttack;
    s.release = fRelease;
    s.hold = fHold;
    s.knee = fKnee;
    s.ratio = fRatio;
    mi_compressor_params_t p;
    mi_compressor_compute_params(&s, &p);
    fTauAttack = p.tau_attack;
    fTauRelease = p.tau_release;
    nHold = p.hold;
    static_assert(sizeof(sComp) == sizeof(p.k), "knee layouts");
    memcpy(&sComp, p.k, sizeof(sComp));
    bUpdate = false;
}

namespace
{
    // the object's computed fields as the bank's channel 0
    bool hand_over(besides::entry *p, float ta, float tr, float rt, uint32_t hold, const dsp::compressor_x2_t &c)
    {
        mi_compressor_params_t q;
        q.tau_attack = ta;
        q.tau_release = tr;
        q.release_threshold = rt;
        q.hold = hold;
        memcpy(q.k, &c, sizeof(q.k));
        return mi::compressor_bank_set_params(p->bank, 0, &q) == MI_OK;
    }

    int send_state(mi_compressor_bank_t *bank, const mi_host::follow_held &s)
    {
        return mi::compressor_bank_set_state(bank, 0, s.e, s.peak, s.hold, nullptr);
    }
}

void Compressor::process(float *out, float *env, const float *in, size_t samples)      // :222-267
{
    update_settings();
    besides::entry *p = besides::of_one(this, mi_compressor_bank_create);
    if (p == nullptr || samples == 0 || !p->buf.reserve(samples, 2) ||
        !hand_over(p, fTauAttack, fTauRelease, fReleaseThresh, nHold, sComp) ||
        !p->hand_over_state({ fEnvelope, fPeak, uint32_t(nHoldCounter) }, send_state))
        return;
    float *d_in = p->buf.row(0), *d_env = p->buf.row(1);
    if (!p->buf.up(0, in, samples) ||
        mi_compressor_bank_process(p->bank, d_in, (env != nullptr) ? d_env : nullptr, d_in, samples, samples, samples, samples, nullptr) != MI_OK ||
        !p->buf.down(out, 0, samples))
        return;
    if (env != nullptr && !p->buf.down(env, 1, samples))
        return;
    if (mi_compressor_bank_get_state(p->bank, 0, &p->held.e, &p->held.peak, &p->held.hold, nullptr) != MI_OK)
        return;
    fEnvelope = p->held.e, fPeak = p->held.peak, nHoldCounter = p->held.hold;
}

float Compressor::process(float *env, float in)                 // :269-311: one sample on the device
{
    float out = 0.0f, e = 0.0f;
    process(&out, &e, &in, 1);
    if (env != NULL)
        *env = e;
    return out;
}

void Compressor::curve(float *out, const float *in, size_t dots)                        // :313-316
{
    besides::entry *p = besides::of_one(this, mi_compressor_bank_create);
    if (p == nullptr || dots == 0 || !p->buf.reserve(dots, 2) ||
        !hand_over(p, fTauAttack, fTauRelease, fReleaseThresh, nHold, sComp))
        return;
    if (p->buf.up(0, in, dots) &&
        mi_compressor_bank_curve(p->bank, p->buf.row(0), p->buf.row(0), dots, dots, dots, nullptr) == MI_OK &&
        p->buf.down(out, 0, dots))
        mi_dspu_stream_synchronize(nullptr);
}

float Compressor::curve(float in)                               // :318-334
{
    const float x = fabsf(in);
    return x2_gain(x, sComp) * x;
}

void Compressor::reduction(float *out, const float *in, size_t dots)                    // :336-340: the curve, as the reference
{
    update_settings();
    curve(out, in, dots);
}

float Compressor::reduction(float in)                           // :342-360
{
    update_settings();
    return x2_gain(fabsf(in), sComp);
}

void Compressor::set_attack_threshold(float threshold)          // :362-368
{
    if (fAttackThresh == threshold)
        return;
    fAttackThresh = threshold;
    bUpdate = true;
}

void Compressor::set_release_threshold(float threshold)         // :370-376
{
    if (fReleaseThresh == threshold)
        return;
    fReleaseThresh = threshold;
    bUpdate = true;
}

void Compressor::set_threshold(float attack, float release)     // :378-385
{
    if ((fAttackThresh == attack) && (fReleaseThresh == release))
        return;
    fAttackThresh = attack;
    fReleaseThresh = release;
    bUpdate = true;
}

void Compressor::set_boost_threshold(float boost)               // :387-393
{
    if (fBoostThresh == boost)
        return;
    fBoostThresh = boost;
    bUpdate = true;
}

void Compressor::set_timings(float attack, float release)       // :395-402
{
    if ((fAttack == attack) && (fRelease == release))
        return;
    fAttack = attack;
    fRelease = release;
    bUpdate = true;
}

void Compressor::set_attack(float attack)                       // :404-410
{
    if (fAttack == attack)
        return;
    fAttack = attack;
    bUpdate = true;
}

void Compressor::set_release(float release)                     // :412-418
{
    if (fRelease == release)
        return;
    fRelease = release;
    bUpdate = true;
}

void Compressor::set_sample_rate(size_t sr)                     // :420-426
{
    if (sr == nSampleRate)
        return;
    nSampleRate = uint32_t(sr);
    bUpdate = true;
}

void Compressor::set_knee(float knee)                           // :428-435
{
    knee = (knee < 0.0f) ? 0.0f : (knee > 1.0f) ? 1.0f : knee;
    if (knee == fKnee)
        return;
    fKnee = knee;
    bUpdate = true;
}

void Compressor::set_ratio(float ratio)                         // :437-443
{
    if (ratio == fRatio)
        return;
    bUpdate = true;
    fRatio = ratio;
}

void Compressor::set_mode(size_t mode)                          // :445-452
{
    if (nMode == mode)
        return;
    nMode = uint32_t(mode);
    bUpdate = true;
}

void Compressor::set_hold(float hold)                           // :454-461
{
    hold = (hold > 0.0f) ? hold : 0.0f;
    if (hold == fHold)
        return;
    fHold = hold;
    bUpdate = true;
}

void Compressor::dump(IStateDumper *v) const                    // :463-501
{
    v->write("fAttackThresh", fAttackThresh);
    v->write("fReleaseThresh", fReleaseThresh);
    v->write("fBoostThresh", fBoostThresh);
    v->write("fAttack", fAttack);
    v->write("fRelease", fRelease);
    v->write("fKnee", fKnee);
    v->write("fRatio", fRatio);
    v->write("fHold", fHold);
    v->write("fEnvelope", fEnvelope);
    v->write("fPeak", fPeak);
    v->write("fTauAttack", fTauAttack);
    v->write("fTauRelease", fTauRelease);
    v->begin_object("sComp", &sComp, sizeof(sComp));
    {
        v->begin_array("k", sComp.k, 2);
        for (size_t i = 0; i < 2; ++i)
        {
            const dsp::compressor_knee_t *k = &sComp.k[i];
            v->begin_object(k, sizeof(dsp::compressor_knee_t));
            v->write("start", k->start);
            v->write("end", k->end);
            v->write("gain", k->gain);
            v->writev("herm", k->herm, 3);
            v->writev("tilt", k->tilt, 2);
            v->end_object();
        }
        v->end_array();
    }
    v->end_array();                                             // the reference closes the sComp object as an array
    v->write("nSampleRate", nSampleRate);
    v->write("nMode", nMode);
    v->write("bUpdate", bUpdate);
}

} // namespace dspu
} // namespace lsp
