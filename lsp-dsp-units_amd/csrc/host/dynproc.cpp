// lsp::dspu::DynamicProcessor (src/main/dynamics/DynamicProcessor.cpp): update_settings() in host float32
// (mi_dynproc_compute_params, what mi_dynproc_bank runs for its dirty channels), and the class on a mi_dynproc_bank of one
// channel.  The class has no member to hang the bank on (its 400 bytes are the reference's), so the bank and its staging
// buffers live beside the object (beside.h).  Before every device call the bank is handed the object's own fCount, nHold,
// vAttack, vRelease and vSplines; process() also sends fEnvelope, fPeak and nHoldCounter when they are not what it read back
// after the previous call (the scalar process() steps them on the host), and reads them back afterwards.
#include <lsp-plug.in/dsp-units/dynamics/DynamicProcessor.h>
#include <lsp-plug.in/dsp-units/units.h>

#include <cmath>
#include <cstring>

#include "beside.h"
#include "dynproc_bank.h"

#pragma clang fp contract(off)      // every product and every sum below rounds on its own, as the reference's build has it

namespace
{
    using lsp::dspu::millis_to_samples;

    constexpr float GAIN_AMP_MIN = 1e-6f, FLOAT_SAT_P_INF = 1e+10f, FLOAT_SAT_M_INF = 1e-10f;

    // interpolation::hermite_quadratic, src/main/misc/interpolation.cpp:103-109
    void hermite_quadratic(float *p, float x0, float y0, float k0, float x1, float k1)
    {
        p[0] = (k0 - k1) * 0.5f / (x0 - x1);
        p[1] = k0 - 2.0f * p[0] * x0;
        p[2] = y0 - (p[0] * x0 + p[1]) * x0;
    }

    // sort_reactions, :204-227: an exchange sort on the level that carries the time, then the time becomes tau
    void sort_reactions(mi_dynproc_reaction_t *s, size_t count, float sr)
    {
        for (size_t i = 0; i + 1 < count; ++i)
            for (size_t j = i + 1; j < count; ++j)
                if (s[j].level < s[i].level)
                {
                    const mi_dynproc_reaction_t tmp = s[i];
                    s[i] = s[j];
                    s[j] = tmp;
                }
        const float k707 = logf(float(1.0 - M_SQRT1_2));
        for (size_t i = 0; i < count; ++i)
            s[i].tau = 1.0f - expf(k707 / millis_to_samples(sr, s[i].tau));
    }

    // sort_splines, :229-285.  On entry thresh, makeup and knee_start hold a dot's input, output and knee; the sort swaps
    // these three only.
    void sort_splines(mi_dynproc_spline_t *s, size_t count, float in_ratio, float out_ratio)
    {
        if (count == 0)
            return;
        for (size_t i = 0; i + 1 < count; ++i)
            for (size_t j = i + 1; j < count; ++j)
                if (s[j].thresh < s[i].thresh)
                {
                    float tmp = s[i].thresh;
                    s[i].thresh = s[j].thresh;
                    s[j].thresh = tmp;
                    tmp = s[i].makeup;
                    s[i].makeup = s[j].makeup;
                    s[j].makeup = tmp;
                    tmp = s[i].knee_start;
                    s[i].knee_start = s[j].knee_start;
                    s[j].knee_start = tmp;
                }

        float sub = 0.0f;
        for (size_t i = 0; i < count; ++i)
        {
            s[i].pre_ratio = (i == 0) ? in_ratio - 1.0f : 0.0f;
            if (i + 1 < count)
            {
                const float dx = logf(s[i + 1].thresh / s[i].thresh);
                const float dy = logf(s[i + 1].makeup / s[i].makeup);
                s[i].post_ratio = dy / dx - 1.0f;
            }
            else
                s[i].post_ratio = (1.0f / out_ratio) - 1.0f;
            s[i].post_ratio -= sub;
            sub += s[i].post_ratio;

            const float thresh = logf(s[i].thresh);
            const float knee = logf(s[i].knee_start);
            s[i].thresh = thresh;
            s[i].knee_stop = thresh - knee;
            s[i].knee_start = thresh + knee;
            s[i].makeup = (i == 0) ? logf(s[i].makeup) - thresh : 0.0f;

            const float log_y1 = s[i].makeup + s[i].pre_ratio * knee;
            hermite_quadratic(s[i].herm, s[i].knee_start, log_y1, s[i].pre_ratio, s[i].knee_stop, s[i].post_ratio);
        }
    }

    // DynamicProcessor::update_settings, :339-395
    void compute_params(const mi_dynproc_settings_t &c, mi_dynproc_params_t &p)
    {
        p = mi_dynproc_params_t();
        p.attacks = 1;
        p.releases = 1;
        p.attack[0].level = 0.0f;
        p.attack[0].tau = c.attack_time[0];
        p.release[0].level = 0.0f;
        p.release[0].tau = c.release_time[0];
        for (size_t i = 0; i < MI_DYNPROC_DOTS; ++i)
        {
            if (c.attack_level[i] >= 0.0f)
            {
                const size_t idx = p.attacks++;
                p.attack[idx].level = c.attack_level[i];
                p.attack[idx].tau = c.attack_time[i + 1];
            }
            if (c.release_level[i] >= 0.0f)
            {
                const size_t idx = p.releases++;
                p.release[idx].level = c.release_level[i];
                p.release[idx].tau = c.release_time[i + 1];
            }
        }
        const float sr = float(c.sample_rate);
        p.hold = uint32_t(millis_to_samples(sr, c.hold));
        for (size_t i = 0; i < MI_DYNPROC_DOTS; ++i)
        {
            const mi_dynproc_dot_t &d = c.dot[i];
            if (d.input < 0 || d.output < 0 || d.knee < 0)
                continue;
            mi_dynproc_spline_t &s = p.spline[p.splines++];
            s.thresh = d.input;
            s.makeup = d.output;
            s.knee_start = d.knee;
        }
        sort_reactions(p.attack, p.attacks, sr);
        sort_reactions(p.release, p.releases, sr);
        sort_splines(p.spline, p.splines, c.in_ratio, c.out_ratio);
    }
} // namespace

extern "C" int mi_dynproc_compute_params(const mi_dynproc_settings_t *settings, mi_dynproc_params_t *params)
{
    MI_REQUIRE(settings != nullptr && params != nullptr, MI_EINVAL, "mi_dynproc_compute_params: NULL argument");
    compute_params(*settings, *params);
    return MI_OK;
}

namespace lsp
{
namespace dspu
{
namespace
{
    typedef mi_host::registry<mi_host::beside<mi_dynproc_bank_t, mi_host::follow_held, mi_dynproc_bank_destroy> > besides;

    // the object's computed fields as the bank's channel 0 (the three tables have the C-ABI's layouts)
    bool hand_over(besides::entry *p, uint32_t splines, uint32_t attacks, uint32_t releases, uint32_t hold, const void *attack,
                   const void *release, const void *spline)
    {
        mi_dynproc_params_t q = mi_dynproc_params_t();
        q.splines = splines, q.attacks = attacks, q.releases = releases, q.hold = hold;
        memcpy(q.attack, attack, sizeof(q.attack));
        memcpy(q.release, release, sizeof(q.release));
        memcpy(q.spline, spline, sizeof(q.spline));
        return mi::dynproc_bank_set_params(p->bank, 0, &q) == MI_OK;
    }

    int send_state(mi_dynproc_bank_t *bank, const mi_host::follow_held &s)
    {
        return mi::dynproc_bank_set_state(bank, 0, s.e, s.peak, s.hold, nullptr);
    }

    inline float limited(float x, float lo)
    {
        if (x < 0.0f)
            x = -x;
        if (x < lo)
            x = lo;
        else if (x > FLOAT_SAT_P_INF)
            x = FLOAT_SAT_P_INF;
        return x;
    }
}

static_assert(sizeof(mi_dynproc_spline_t) == 40 && sizeof(mi_dynproc_reaction_t) == 8 && sizeof(mi_dynproc_dot_t) == sizeof(dyndot_t),
              "the C-ABI's tables have the class's layouts");

DynamicProcessor::DynamicProcessor()  { construct(); }
DynamicProcessor::~DynamicProcessor() { destroy(); }

void DynamicProcessor::construct()                              // DynamicProcessor.cpp:43-74
{
    besides::drop(this);                                        // whatever lived at this address before
    fInRatio = 1.0f;
    fOutRatio = 1.0f;
    fEnvelope = 0.0f;
    fHold = 0.0f;
    fPeak = 0.0f;
    nHold = 0;
    nHoldCounter = 0;
    nSampleRate = 0;
    bUpdate = true;
    for (size_t i = 0; i < DYNAMIC_PROCESSOR_DOTS; ++i)
    {
        vDots[i].fInput = 0.0f;
        vDots[i].fOutput = 0.0f;
        vDots[i].fKnee = 0.0f;
        vAttackLvl[i] = 0.0f;
        vReleaseLvl[i] = 0.0f;
    }
    for (size_t i = 0; i < DYNAMIC_PROCESSOR_RANGES; ++i)
    {
        vAttackTime[i] = 0.0f;
        vReleaseTime[i] = 0.0f;
    }
    for (size_t i = 0; i < CT_TOTAL; ++i)
        fCount[i] = 0;
    // the reference leaves the computed tables as they were; raw memory becomes zeros here so that dump() reads no garbage
    memset(vSplines, 0, sizeof(vSplines));
    memset(vAttack, 0, sizeof(vAttack));
    memset(vRelease, 0, sizeof(vRelease));
}

void DynamicProcessor::destroy()                                // :76-78
{
    besides::drop(this);
}

// update_settings(), :339-395: computes whenever it is called, the caller asks modified() first.  ONE DIFFERENCE: the
// reference never clears bUpdate, so its modified() stays true for ever; here it is cleared, as every other unit does.
void DynamicProcessor::update_settings()
{
    mi_dynproc_settings_t s;
    s.sample_rate = nSampleRate;
    s.hold = fHold;
    s.in_ratio = fInRatio;
    s.out_ratio = fOutRatio;
    memcpy(s.dot, vDots, sizeof(s.dot));
    memcpy(s.attack_level, vAttackLvl, sizeof(s.attack_level));
    memcpy(s.release_level, vReleaseLvl, sizeof(s.release_level));
    memcpy(s.attack_time, vAttackTime, sizeof(s.attack_time));
    memcpy(s.release_time, vReleaseTime, sizeof(s.release_time));
    mi_dynproc_params_t p;
    compute_params(s, p);
    fCount[CT_SPLINES] = uint8_t(p.splines);
    fCount[CT_ATTACK] = uint8_t(p.attacks);
    fCount[CT_RELEASE] = uint8_t(p.releases);
    nHold = p.hold;
    memcpy(vAttack, p.attack, sizeof(vAttack));
    memcpy(vRelease, p.release, sizeof(vRelease));
    memcpy(vSplines, p.spline, sizeof(vSplines));
    bUpdate = false;
}

float DynamicProcessor::spline_amp(const spline_t *s, float lx)                         // :173-183
{
    if (lx <= s->fKneeStart)
        return s->fMakeup + s->fPreRatio * (lx - s->fThresh);
    if (lx >= s->fKneeStop)
        return s->fMakeup + s->fPostRatio * (lx - s->fThresh);
    return (s->vHermite[0] * lx + s->vHermite[1]) * lx + s->vHermite[2];
}

float DynamicProcessor::spline_model(const spline_t *s, float lx)                       // :185-193
{
    if (lx <= s->fThresh)
        return s->fMakeup + s->fPreRatio * (lx - s->fThresh);
    return s->fMakeup + s->fPostRatio * (lx - s->fThresh);
}

float DynamicProcessor::solve_reaction(const reaction_t *s, float x, size_t count)      // :195-202
{
    float r = s[0].fTau;
    for (size_t i = 1; i < count; ++i)
        if (x >= s[i].fLevel)
            r = s[i].fTau;
    return r;
}

void DynamicProcessor::process(float *out, float *env, const float *in, size_t samples)         // :397-442
{
    besides::entry *p = besides::of_one(this, mi_dynproc_bank_create);
    if (p == nullptr || samples == 0 || !p->buf.reserve(samples, 2) ||
        !hand_over(p, fCount[CT_SPLINES], fCount[CT_ATTACK], fCount[CT_RELEASE], nHold, vAttack, vRelease, vSplines) ||
        !p->hand_over_state({ fEnvelope, fPeak, nHoldCounter }, send_state))
        return;
    float *d_in = p->buf.row(0), *d_env = p->buf.row(1);
    if (!p->buf.up(0, in, samples) ||
        mi_dynproc_bank_process(p->bank, d_in, (env != nullptr) ? d_env : nullptr, d_in, samples, samples, samples, samples, nullptr) != MI_OK ||
        !p->buf.down(out, 0, samples))
        return;
    if (env != nullptr && !p->buf.down(env, 1, samples))
        return;
    if (mi_dynproc_bank_get_state(p->bank, 0, &p->held.e, &p->held.peak, &p->held.hold, nullptr) != MI_OK)
        return;
    fEnvelope = p->held.e, fPeak = p->held.peak, nHoldCounter = p->held.hold;
}

float DynamicProcessor::process(float *env, float s)            // :444-472: on the host; the gain has the scalar limit
{
    const float d = s - fEnvelope;
    if (d < 0.0f)
    {
        if (nHoldCounter > 0)
            --nHoldCounter;
        else
        {
            fEnvelope += d * solve_reaction(vRelease, fEnvelope, fCount[CT_RELEASE]);
            fPeak = fEnvelope;
        }
    }
    else
    {
        fEnvelope += d * solve_reaction(vAttack, fEnvelope, fCount[CT_ATTACK]);
        if (fEnvelope >= fPeak)
        {
            fPeak = fEnvelope;
            nHoldCounter = nHold;
        }
    }
    if (env != NULL)
        *env = fEnvelope;
    return reduction(fEnvelope);
}

void DynamicProcessor::curve(float *out, const float *in, size_t dots)                  // :474-496
{
    besides::entry *p = besides::of_one(this, mi_dynproc_bank_create);
    if (p == nullptr || dots == 0 || !p->buf.reserve(dots, 2) ||
        !hand_over(p, fCount[CT_SPLINES], fCount[CT_ATTACK], fCount[CT_RELEASE], nHold, vAttack, vRelease, vSplines))
        return;
    if (p->buf.up(0, in, dots) &&
        mi_dynproc_bank_curve(p->bank, p->buf.row(0), p->buf.row(0), dots, dots, dots, nullptr) == MI_OK &&
        p->buf.down(out, 0, dots))
        mi_dspu_stream_synchronize(nullptr);
}

float DynamicProcessor::curve(float in)                         // :498-516
{
    in = limited(in, FLOAT_SAT_M_INF);
    const float lx = logf(in);
    float gain = 0.0f;
    for (size_t j = 0; j < fCount[CT_SPLINES]; ++j)
        gain += spline_amp(&vSplines[j], lx);
    return expf(gain) * in;
}

void DynamicProcessor::model(float *out, const float *in, size_t dots)                  // :518-540
{
    besides::entry *p = besides::of_one(this, mi_dynproc_bank_create);
    if (p == nullptr || dots == 0 || !p->buf.reserve(dots, 2) ||
        !hand_over(p, fCount[CT_SPLINES], fCount[CT_ATTACK], fCount[CT_RELEASE], nHold, vAttack, vRelease, vSplines))
        return;
    if (p->buf.up(0, in, dots) &&
        mi_dynproc_bank_model(p->bank, p->buf.row(0), p->buf.row(0), dots, dots, dots, nullptr) == MI_OK &&
        p->buf.down(out, 0, dots))
        mi_dspu_stream_synchronize(nullptr);
}

float DynamicProcessor::model(float in)                         // :542-560
{
    in = limited(in, FLOAT_SAT_M_INF);
    const float lx = logf(in);
    float gain = 0.0f;
    for (size_t j = 0; j < fCount[CT_SPLINES]; ++j)
        gain += spline_model(&vSplines[j], lx);
    return expf(gain) * in;
}

void DynamicProcessor::reduction(float *out, const float *in, size_t dots)              // :562-584: the limit is GAIN_AMP_MIN
{
    for (size_t i = 0; i < dots; ++i)
    {
        const float lx = logf(limited(in[i], GAIN_AMP_MIN));
        float gain = 0.0f;
        for (size_t j = 0; j < fCount[CT_SPLINES]; ++j)
            gain += spline_amp(&vSplines[j], lx);
        out[i] = expf(gain);
    }
}

float DynamicProcessor::reduction(float in)                     // :586-604: the limit is FLOAT_SAT_M_INF
{
    const float lx = logf(limited(in, FLOAT_SAT_M_INF));
    float gain = 0.0f;
    for (size_t j = 0; j < fCount[CT_SPLINES]; ++j)
        gain += spline_amp(&vSplines[j], lx);
    return expf(gain);
}

void DynamicProcessor::set_sample_rate(size_t sr)               // :80-86
{
    if (sr == nSampleRate)
        return;
    nSampleRate = uint32_t(sr);
    bUpdate = true;
}

void DynamicProcessor::set_in_ratio(float ratio)                // :88-94
{
    if (fInRatio == ratio)
        return;
    fInRatio = ratio;
    bUpdate = true;
}

void DynamicProcessor::set_out_ratio(float ratio)               // :96-102
{
    if (fOutRatio == ratio)
        return;
    fOutRatio = ratio;
    bUpdate = true;
}

bool DynamicProcessor::get_dot(size_t id, dyndot_t *dst) const  // :104-110
{
    if ((id >= DYNAMIC_PROCESSOR_DOTS) || (dst == NULL))
        return false;
    *dst = vDots[id];
    return true;
}

float DynamicProcessor::attack_level(size_t id) const           // :112-115
{
    return (id >= DYNAMIC_PROCESSOR_DOTS) ? -1.0f : vAttackLvl[id];
}

void DynamicProcessor::set_attack_level(size_t id, float value) // :117-123
{
    if ((id >= DYNAMIC_PROCESSOR_DOTS) || (vAttackLvl[id] == value))
        return;
    vAttackLvl[id] = value;
    bUpdate = true;
}

float DynamicProcessor::release_level(size_t id) const          // :125-128
{
    return (id >= DYNAMIC_PROCESSOR_DOTS) ? -1.0f : vReleaseLvl[id];
}

void DynamicProcessor::set_release_level(size_t id, float value)    // :130-136
{
    if ((id >= DYNAMIC_PROCESSOR_DOTS) || (vReleaseLvl[id] == value))
        return;
    vReleaseLvl[id] = value;
    bUpdate = true;
}

float DynamicProcessor::attack_time(size_t id) const            // :138-141
{
    return (id >= DYNAMIC_PROCESSOR_RANGES) ? -1.0f : vAttackTime[id];
}

void DynamicProcessor::set_attack_time(size_t id, float value)  // :143-149
{
    if ((id >= DYNAMIC_PROCESSOR_RANGES) || (vAttackTime[id] == value))
        return;
    vAttackTime[id] = value;
    bUpdate = true;
}

float DynamicProcessor::release_time(size_t id) const           // :151-154
{
    return (id >= DYNAMIC_PROCESSOR_RANGES) ? -1.0f : vReleaseTime[id];
}

void DynamicProcessor::set_release_time(size_t id, float value) // :156-162
{
    if ((id >= DYNAMIC_PROCESSOR_RANGES) || (vReleaseTime[id] == value))
        return;
    vReleaseTime[id] = value;
    bUpdate = true;
}

void DynamicProcessor::set_hold(float hold)                     // :164-171
{
    hold = (hold > 0.0f) ? hold : 0.0f;
    if (hold == fHold)
        return;
    fHold = hold;
    bUpdate = true;
}

bool DynamicProcessor::set_dot(size_t id, const dyndot_t *src)  // :287-318
{
    if (id >= DYNAMIC_PROCESSOR_DOTS)
        return false;
    dyndot_t *dst = &vDots[id];
    if (src == NULL)
    {
        bUpdate = bUpdate || (dst->fInput >= 0.0f) || (dst->fOutput >= 0.0f) || (dst->fKnee >= 0.0f);
        dst->fInput = -1.0f;
        dst->fOutput = -1.0f;
        dst->fKnee = -1.0f;
    }
    else
    {
        bUpdate = bUpdate || (dst->fInput != src->fInput) || (dst->fOutput != src->fOutput) || (dst->fKnee != src->fKnee);
        dst->fInput = src->fInput;
        dst->fOutput = src->fOutput;
        dst->fKnee = src->fKnee;
    }
    return true;
}

bool DynamicProcessor::set_dot(size_t id, float in, float out, float knee)      // :320-337
{
    if (id >= DYNAMIC_PROCESSOR_DOTS)
        return false;
    dyndot_t *dst = &vDots[id];
    bUpdate = bUpdate || (dst->fInput != in) || (dst->fOutput != out) || (dst->fKnee != knee);
    dst->fInput = in;
    dst->fOutput = out;
    dst->fKnee = knee;
    return true;
}

void DynamicProcessor::dump(IStateDumper *v) const              // :606-682
{
    v->begin_array("vDots", vDots, DYNAMIC_PROCESSOR_DOTS);
    for (size_t i = 0; i < DYNAMIC_PROCESSOR_DOTS; ++i)
    {
        const dyndot_t *dot = &vDots[i];
        v->begin_object(dot, sizeof(dyndot_t));
        {
            v->write("fInput", dot->fInput);
            v->write("fOutput", dot->fOutput);
            v->write("fKnee", dot->fKnee);
        }
        v->end_object();
    }
    v->end_array();

    v->writev("vAttackLvl", vAttackLvl, DYNAMIC_PROCESSOR_DOTS);
    v->writev("vReleaseLvl", vReleaseLvl, DYNAMIC_PROCESSOR_DOTS);
    v->writev("vAttackTime", vAttackTime, DYNAMIC_PROCESSOR_RANGES);
    v->writev("vReleaseTime", vReleaseTime, DYNAMIC_PROCESSOR_RANGES);

    v->write("fInRatio", fInRatio);
    v->write("fOutRatio", fOutRatio);

    v->begin_array("vSplines", vSplines, DYNAMIC_PROCESSOR_DOTS);
    for (size_t i = 0; i < DYNAMIC_PROCESSOR_DOTS; ++i)
    {
        const spline_t *s = &vSplines[i];
        v->begin_object(s, sizeof(spline_t));
        {
            v->write("fPreRatio", s->fPreRatio);
            v->write("fPostRatio", s->fPostRatio);
            v->write("fKneeStart", s->fKneeStart);
            v->write("fKneeStop", s->fKneeStop);
            v->write("fThresh", s->fThresh);
            v->write("fMakeup", s->fMakeup);
            v->writev("vHermite", s->vHermite, 4);
        }
        v->end_object();
    }
    v->end_array();

    v->begin_array("vAttack", vAttack, DYNAMIC_PROCESSOR_RANGES);
    for (size_t i = 0; i < DYNAMIC_PROCESSOR_RANGES; ++i)
    {
        const reaction_t *r = &vAttack[i];
        v->begin_object(r, sizeof(reaction_t));
        {
            v->write("fLevel", r->fLevel);
            v->write("fTau", r->fTau);
        }
        v->end_object();
    }
    v->end_array();

    v->begin_array("vRelease", vRelease, DYNAMIC_PROCESSOR_RANGES);
    for (size_t i = 0; i < DYNAMIC_PROCESSOR_RANGES; ++i)
    {
        const reaction_t *r = &vRelease[i];
        v->begin_object(r, sizeof(reaction_t));
        {
            v->write("fLevel", r->fLevel);
            v->write("fTau", r->fTau);
        }
        v->end_object();
    }
    v->end_array();

    v->write("fEnvelope", fEnvelope);
    v->write("fHold", fHold);
    v->write("fPeak", fPeak);

    v->write("nHold", nHold);
    v->write("nHoldCounter", nHoldCounter);
    v->write("nSampleRate", nSampleRate);
    v->write("bUpdate", bUpdate);
}

} // namespace dspu
} // namespace lsp
