// lsp::dspu::Gate (src/main/dynamics/Gate.cpp) on a mi_gate_bank of one channel.  The class has no member to hang the
// bank on (its 128 bytes are the reference's), so the bank and its staging buffers live beside the object (beside.h).  Before
// every device call the bank is handed the object's own fTau*, nHold and the two sKnee; process() also sends fEnvelope, fPeak,
// nHoldCounter and nCurve when they are not what it read back after the previous call (the scalar process() and a subclass
// write them), and reads them back afterwards.
#include <lsp-plug.in/dsp-units/dynamics/Gate.h>

#include <cmath>
#include <cstring>

#include "beside.h"
#include "gate_bank.h"

namespace lsp
{
namespace dspu
{
namespace
{
    struct gate_held { float e = 0.0f, peak = 0.0f; uint32_t hold = 0, curve = 0; };    // the state as the device holds it
    typedef mi_host::registry<mi_host::beside<mi_gate_bank_t, gate_held, mi_gate_bank_destroy> > besides;

    // the object's computed fields as the bank's channel 0
    bool hand_over(besides::entry *p, float ta, float tr, uint32_t hold, const dsp::gate_knee_t &k0, const dsp::gate_knee_t &k1)
    {
        mi_gate_params_t q;
        q.tau_attack = ta;
        q.tau_release = tr;
        q.hold = hold;
        q.reserved = 0;
        static_assert(sizeof(k0) == sizeof(q.k[0]), "knee layouts");
        memcpy(&q.k[0], &k0, sizeof(q.k[0]));
        memcpy(&q.k[1], &k1, sizeof(q.k[1]));
        return mi::gate_bank_set_params(p->bank, 0, &q) == MI_OK;
    }

    int send_state(mi_gate_bank_t *bank, const gate_held &s)
    {
        return mi::gate_bank_set_state(bank, 0, s.e, s.peak, s.hold, s.curve, nullptr);
    }

    inline float knee_gain(float x, const dsp::gate_knee_t *c)  // Gate.cpp:236-247, x = |input|
    {
        if (x <= c->start)
            return c->gain_start;
        if (x >= c->end)
            return c->gain_end;
        const float lx = logf(x);
        return expf(((c->herm[0] * lx + c->herm[1]) * lx + c->herm[2]) * lx + c->herm[3]);
    }
}

Gate::Gate()  { construct(); }
Gate::~Gate() { destroy(); }

void Gate::construct()                                          // Gate.cpp:41-74
{
    besides::drop(this);                                        // whatever lived at this address before
    for (size_t i = 0; i < 2; ++i)
    {
        curve_t *c = &sCurves[i];
        c->fThreshold = 0.0f;
        c->fZone = 1.0f;
        c->sKnee.start = 0.0f;
        c->sKnee.end = 0.0f;
        c->sKnee.gain_start = 0.0f;
        c->sKnee.gain_end = 0.0f;
        c->sKnee.herm[0] = c->sKnee.herm[1] = c->sKnee.herm[2] = c->sKnee.herm[3] = 0.0f;
    }
    fAttack = 0.0f;
    fRelease = 0.0f;
    fTauAttack = 0.0f;
    fTauRelease = 0.0f;
    fReduction = 0.0f;
    fEnvelope = 0.0f;
    fHold = 0.0f;
    fPeak = 0.0f;
    nHold = 0;
    nHoldCounter = 0;
    nSampleRate = 0;
    nCurve = 0;
    bUpdate = true;
}

void Gate::destroy()                                            // :76-78
{
    besides::drop(this);
}

void Gate::update_settings()                                    // :180-205: computes whether or not bUpdate is set
{
    mi_gate_settings_t s;
    s.sample_rate = nSampleRate;
    for (size_t i = 0; i < 2; ++i)
        s.threshold[i] = sCurves[i].fThreshold, s.zone[i] = sCurves[i].fZone;
    s.reduction = fReduction;
    s.attack = fAttack;
    s.release = fRelease;
    s.hold = fHold;
    mi_gate_params_t p;
    mi_gate_compute_params(&s, &p);
    fTauAttack = p.tau_attack;
    fTauRelease = p.tau_release;
    nHold = p.hold;
    for (size_t i = 0; i < 2; ++i)
    {
        static_assert(sizeof(sCurves[i].sKnee) == sizeof(p.k[i]), "knee layouts");
        memcpy(&sCurves[i].sKnee, &p.k[i], sizeof(p.k[i]));
    }
    bUpdate = false;
}

void Gate::process(float *out, float *env, const float *in, size_t samples)            // :267-367: no update_settings()
{
    besides::entry *p = besides::of_one(this, mi_gate_bank_create);
    if (p == nullptr || samples == 0 || !p->buf.reserve(samples, 2) ||
        !hand_over(p, fTauAttack, fTauRelease, nHold, sCurves[0].sKnee, sCurves[1].sKnee) ||
        !p->hand_over_state({ fEnvelope, fPeak, uint32_t(nHoldCounter), (nCurve != 0) ? 1u : 0u }, send_state))
        return;
    float *d_in = p->buf.row(0), *d_env = p->buf.row(1);
    if (!p->buf.up(0, in, samples) ||
        mi_gate_bank_process(p->bank, d_in, (env != nullptr) ? d_env : nullptr, d_in, samples, samples, samples, samples, nullptr) != MI_OK ||
        !p->buf.down(out, 0, samples))
        return;
    if (env != nullptr && !p->buf.down(env, 1, samples))
        return;
    if (mi_gate_bank_get_state(p->bank, 0, &p->held.e, &p->held.peak, &p->held.hold, &p->held.curve, nullptr) != MI_OK)
        return;
    fEnvelope = p->held.e, fPeak = p->held.peak, nHoldCounter = p->held.hold, nCurve = uint8_t(p->held.curve);
}

float Gate::process(float *env, float s)                        // :369-407: one step, the curve chosen by the old curve's knee
{
    const curve_t *c = &sCurves[nCurve];
    const float d = s - fEnvelope;
    if (d < 0.0f)
    {
        if (nHoldCounter > 0)
            --nHoldCounter;
        else
        {
            const float step = fTauRelease * d;
            fEnvelope = fEnvelope + step;
            fPeak = fEnvelope;
        }
    }
    else
    {
        const float step = fTauAttack * d;
        fEnvelope = fEnvelope + step;
        if (fEnvelope >= fPeak)
        {
            fPeak = fEnvelope;
            nHoldCounter = nHold;
        }
    }
    if (fEnvelope < c->sKnee.start)
        nCurve = 0;
    else if (fEnvelope > c->sKnee.end)
        nCurve = 1;
    if (env != NULL)
        *env = fEnvelope;
    return amplification(fEnvelope);
}

void Gate::curve(float *out, const float *in, size_t dots, bool hyst) const            // :207-210
{
    besides::entry *p = besides::of_one(this, mi_gate_bank_create);
    if (p == nullptr || dots == 0 || !p->buf.reserve(dots, 2) ||
        !hand_over(p, fTauAttack, fTauRelease, nHold, sCurves[0].sKnee, sCurves[1].sKnee))
        return;
    if (p->buf.up(0, in, dots) &&
        mi_gate_bank_curve(p->bank, p->buf.row(0), p->buf.row(0), dots, hyst ? 1 : 0, dots, dots, nullptr) == MI_OK &&
        p->buf.down(out, 0, dots))
        mi_dspu_stream_synchronize(nullptr);
}

float Gate::curve(float in, bool hyst) const                    // :212-226
{
    const float x = fabsf(in);
    return x * knee_gain(x, &sCurves[(hyst) ? 1 : 0].sKnee);
}

void Gate::amplification(float *out, const float *in, size_t dots, bool hyst) const    // :228-231: the scalar form, dot by dot
{
    for (size_t i = 0; i < dots; ++i)
        out[i] = amplification(in[i], hyst);
}

float Gate::amplification(float in, bool hyst) const            // :233-248
{
    return knee_gain(fabsf(in), &sCurves[(hyst) ? 1 : 0].sKnee);
}

float Gate::amplification(float in) const                       // :250-265
{
    return knee_gain(fabsf(in), &sCurves[nCurve].sKnee);
}

void Gate::set_threshold(float topen, float tclose)             // :80-87
{
    if ((topen == sCurves[0].fThreshold) && (tclose == sCurves[1].fThreshold))
        return;
    sCurves[0].fThreshold = topen;
    sCurves[1].fThreshold = tclose;
    bUpdate = true;
}

void Gate::set_open_threshold(float threshold)                  // :89-95
{
    if (threshold == sCurves[0].fThreshold)
        return;
    sCurves[0].fThreshold = threshold;
    bUpdate = true;
}

void Gate::set_close_threshold(float threshold)                 // :97-103
{
    if (threshold == sCurves[1].fThreshold)
        return;
    sCurves[1].fThreshold = threshold;
    bUpdate = true;
}

void Gate::set_reduction(float reduction)                       // :105-111
{
    if (reduction == fReduction)
        return;
    fReduction = reduction;
    bUpdate = true;
}

void Gate::set_timings(float attack, float release)             // :113-120
{
    if ((fAttack == attack) && (fRelease == release))
        return;
    fAttack = attack;
    fRelease = release;
    bUpdate = true;
}

void Gate::set_attack(float attack)                             // :122-128
{
    if (fAttack == attack)
        return;
    fAttack = attack;
    bUpdate = true;
}

void Gate::set_release(float release)                           // :130-136
{
    if (fRelease == release)
        return;
    fRelease = release;
    bUpdate = true;
}

void Gate::set_sample_rate(size_t sr)                           // :138-144
{
    if (sr == nSampleRate)
        return;
    nSampleRate = uint32_t(sr);
    bUpdate = true;
}

void Gate::set_zone(float open, float close)                    // :146-153
{
    if ((open == sCurves[0].fZone) && (close == sCurves[1].fZone))
        return;
    sCurves[0].fZone = open;
    sCurves[1].fZone = close;
    bUpdate = true;
}

void Gate::set_open_zone(float zone)                            // :155-161
{
    if (zone == sCurves[0].fZone)
        return;
    sCurves[0].fZone = zone;
    bUpdate = true;
}

void Gate::set_close_zone(float zone)                           // :163-169
{
    if (zone == sCurves[1].fZone)
        return;
    sCurves[1].fZone = zone;
    bUpdate = true;
}

void Gate::set_hold(float hold)                                 // :171-178
{
    hold = (hold > 0.0f) ? hold : 0.0f;
    if (hold == fHold)
        return;
    fHold = hold;
    bUpdate = true;
}

void Gate::dump(IStateDumper *v) const                          // :409-449
{
    v->begin_array("sCurves", sCurves, 2);
    for (size_t i = 0; i < 2; ++i)
    {
        const curve_t *c = &sCurves[i];
        v->begin_object(c, sizeof(curve_t));
        {
            v->write("fThreshold", c->fThreshold);
            v->write("fZone", c->fZone);
            const dsp::gate_knee_t *k = &c->sKnee;
            v->begin_object("sKnee", k, sizeof(dsp::gate_knee_t));
            {
                v->write("start", k->start);
                v->write("end", k->end);
                v->write("gain_start", k->gain_start);
                v->write("gain_end", k->gain_end);
                v->writev("herm", k->herm, 4);
            }
            v->end_object();
        }
        v->end_object();
    }
    v->end_array();
    v->write("fAttack", fAttack);
    v->write("fRelease", fRelease);
    v->write("fTauAttack", fTauAttack);
    v->write("fTauRelease", fTauRelease);
    v->write("fReduction", fReduction);
    v->write("fEnvelope", fEnvelope);
    v->write("fHold", fHold);
    v->write("fPeak", fPeak);
    v->write("nHold", nHold);
    v->write("nHoldCounter", nHoldCounter);
    v->write("nSampleRate", nSampleRate);
    v->write("nCurve", nCurve);
    v->write("bUpdate", bUpdate);
}

} // namespace dspu
} // namespace lsp
