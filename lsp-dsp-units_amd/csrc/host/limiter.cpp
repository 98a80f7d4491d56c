// lsp::dspu::Limiter's update_settings() (src/main/dynamics/Limiter.cpp:396-548) with init_sat / init_exp / init_line
// (:278-394) on the host in float32, and the patch of apply_sat_patch / apply_exp_patch / apply_line_patch (:609-673) as a
// TABLE shape[t], t in [0, nRelease): the device multiplies gains by 1 - k shape[t] and never evaluates a polynomial or an
// exponent of its own, so one kernel serves the twelve modes and expf is this file's for every one of them (a device expf that
// differs in the last bit would move a peak decision, and everything after it).
//
// Below them lsp::dspu::Limiter on a mi_limiter_bank of one channel: the class has no member to hang the bank on (its 216
// bytes are the reference's), so the bank and its staging buffer live beside the object in host/beside.h's registry, keyed by
// the object's address: made in init(), dropped in destroy() and in construct().  Every setter goes to the bank as well, so the
// bank's own update_settings() sees what the object's sees; nHead and sALR.fEnvelope are read back after every process().
#include "limiter_bank.h"

#include <lsp-plug.in/dsp-units/dynamics/Limiter.h>
#include <lsp-plug.in/dsp-units/units.h>

#include <cmath>
#include <cstring>

#include "beside.h"

#pragma clang fp contract(off)      // every product and every sum below rounds on its own

namespace
{
    using lsp::dspu::millis_to_samples;

    // GAIN_AMP_M_9_DB of const.h:65, a double there
    constexpr double AMP_M_9_DB = 0.354813;

    // interpolation::hermite_cubic, src/main/misc/interpolation.cpp:112-131: the differences and products of float
    // arguments are float32, what is assigned to a double or meets one is double
    void hermite_cubic(float *p, float x0, float y0, float k0, float x1, float y1, float k1)
    {
        const double dx = x1 - x0;
        const double dy = y1 - y0;
        const double kx = dy / dx;
        const double xx1 = x1 * x1;
        const double xx2 = x0 + x1;
        const double a = ((k0 + k1) * dx - 2.0f * dy) / (dx * dx * dx);
        const double b = ((kx - k0) + a * ((2.0f * x0 - x1) * x0 - xx1)) / dx;
        const double c = kx - a * (xx1 + xx2 * x0) - b * xx2;
        const double d = y0 - x0 * (c + x0 * (b + x0 * a));
        p[0] = float(a), p[1] = float(b), p[2] = float(c), p[3] = float(d);
    }

    // interpolation::exponent, :224-230: k (x0 - x1) and k x0 are float32, exp and the quotients double, p[0] is read back
    // as the float it was stored as
    void exponent(float *p, float x0, float y0, float x1, float y1, float k)
    {
        const double e = exp(k * (x0 - x1));
        p[0] = float((y0 - e * y1) / (1.0 - e));
        p[1] = float((y0 - p[0]) / exp(k * x0));
        p[2] = k;
    }

    // interpolation::linear, :233-237
    void linear(float *p, float x0, float y0, float x1, float y1)
    {
        p[0] = (y1 - y0) / (x1 - x0);
        p[1] = y0 - p[0] * x0;
    }

    // interpolation::hermite_quadratic, :103-109
    void hermite_quadratic(float *p, float x0, float y0, float k0, float x1, float k1)
    {
        p[0] = (k0 - k1) * 0.5f / (x0 - x1);
        p[1] = k0 - 2.0f * p[0] * x0;
        p[2] = y0 - (p[0] * x0 + p[1]) * x0;
    }

    // the widths of one family: THIN, WIDE, TAIL, DUCK (:286-308, :327-349, :368-390)
    void widths(mi_limiter_params_t &p, uint32_t width, int64_t attack, int64_t release)
    {
        switch (width)
        {
            case 0:  p.attack = int32_t(attack);     p.plane = int32_t(attack); break;
            case 2:  p.attack = int32_t(attack / 2); p.plane = int32_t(attack); break;
            case 3:  p.attack = int32_t(attack);     p.plane = int32_t(attack + (release / 2)); break;
            default: p.attack = int32_t(attack / 2); p.plane = int32_t(attack + (release / 2)); break;
        }
        p.release = int32_t(attack + release + 1);
        p.middle = int32_t(attack);
    }
}

namespace mi
{
    void limiter_compute_params(const mi_limiter_settings_t &s, mi_limiter_params_t &p)
    {
        p = mi_limiter_params_t{};
        const float sr = float(s.sample_rate);
        p.lookahead = uint32_t(millis_to_samples(sr, s.lookahead));                                    // :406
        p.mode = s.mode;
        p.threshold = s.threshold;                                                                      // :418

        // :459-469
        const float thresh = float(s.threshold * s.knee * AMP_M_9_DB);
        p.ks = thresh * s.alr_knee;
        p.ke = 2.0f * thresh - p.ks;
        p.gain = thresh;
        hermite_quadratic(p.hermite, p.ks, p.ks, 1.0f, p.ke, 0.0f);
        const float att = millis_to_samples(sr, s.alr_attack), rel = millis_to_samples(sr, s.alr_release);
        const float k707 = logf(float(1.0 - M_SQRT1_2));
        p.tau_attack = (att < 1.0f) ? 1.0f : 1.0f - expf(k707 / att);
        p.tau_release = (rel < 1.0f) ? 1.0f : 1.0f - expf(k707 / rel);

        int64_t attack = int64_t(millis_to_samples(sr, s.attack)), release = int64_t(millis_to_samples(sr, s.release));
        const int64_t la = int64_t(p.lookahead);
        if (s.mode < 4)                                                                                 // init_sat, :278-312
        {
            attack = (attack < 8) ? 8 : (attack > la) ? la : attack;                                    // lsp_limit: below 8 it is 8, else above la it is la
            release = (attack < 8) ? 8 : (attack > la * 2) ? la * 2 : attack;                           // :284: FROM ATTACK
            widths(p, s.mode, attack, release);
            hermite_cubic(p.v_attack, -1.0f, 0.0f, 0.0f, float(p.attack), 1.0f, 0.0f);
            hermite_cubic(p.v_release, float(p.plane), 1.0f, 0.0f, float(p.release), 0.0f, 0.0f);
            return;
        }
        // init_exp, :314-353, and init_line, :355-394: here the upper limit wins
        if (attack > la)
            attack = la;
        else if (attack < 8)
            attack = 8;
        if (release > la * 2)
            release = la * 2;
        else if (release < 8)
            release = 8;
        if (s.mode < 8)
        {
            widths(p, 1, attack, release);              // :327-346 compare nMode with LM_HERM_*: never true in an LM_EXP_ mode
            exponent(p.v_attack, -1.0f, 0.0f, float(p.attack), 1.0f, 2.0f / float(attack));
            exponent(p.v_release, float(p.plane), 1.0f, float(p.release), 0.0f, 2.0f / float(release));
        }
        else
        {
            widths(p, s.mode - 8, attack, release);
            linear(p.v_attack, -1.0f, 0.0f, float(p.attack), 1.0f);
            linear(p.v_release, float(p.plane), 1.0f, float(p.release), 0.0f);
        }
    }

    // apply_sat_patch (:609-633), apply_exp_patch (:635-653), apply_line_patch (:655-673) without amp and the gain
    void limiter_compute_patch(const mi_limiter_params_t &p, float *shape)
    {
        for (int32_t t = 0; t < p.release; ++t)
        {
            const float x = float(t);
            const float *v = (t < p.attack) ? p.v_attack : p.v_release;
            if (t >= p.attack && t < p.plane)
                shape[t] = 1.0f;
            else if (p.mode < 4)
                shape[t] = ((v[0] * x + v[1]) * x + v[2]) * x + v[3];
            else if (p.mode < 8)
                shape[t] = v[0] + v[1] * expf(v[2] * x);
            else
                shape[t] = v[0] * x + v[1];
        }
    }
}

extern "C" {

int mi_limiter_compute_params(const mi_limiter_settings_t *settings, mi_limiter_params_t *params)
{
    MI_REQUIRE(settings != nullptr && params != nullptr, MI_EINVAL, "mi_limiter_compute_params: NULL argument");
    MI_REQUIRE(settings->mode < MI_LIMITER_MODES, MI_EINVAL, "mi_limiter_compute_params: mode %u out of range", settings->mode);
    mi::limiter_compute_params(*settings, *params);
    return MI_OK;
}

int mi_limiter_compute_patch(const mi_limiter_params_t *params, float *shape, size_t capacity)
{
    MI_REQUIRE(params != nullptr && (shape != nullptr || params->release <= 0), MI_EINVAL, "mi_limiter_compute_patch: NULL argument");
    MI_REQUIRE(params->mode < MI_LIMITER_MODES, MI_EINVAL, "mi_limiter_compute_patch: mode %u out of range", params->mode);
    MI_REQUIRE(params->release <= 0 || size_t(params->release) <= capacity, MI_EINVAL,
               "mi_limiter_compute_patch: %d entries do not fit into %zu", params->release, capacity);
    MI_REQUIRE(params->attack >= 0 && params->plane >= 0, MI_EINVAL, "mi_limiter_compute_patch: negative widths");
    mi::limiter_compute_patch(*params, shape);
    return MI_OK;
}

} // extern "C"

namespace lsp
{
namespace dspu
{
namespace
{
    struct limiter_impl
    {
        mi_limiter_bank_t *bank = nullptr;
        mi_host::rows buf;                  // [1][cap]: the staged sidechain, the gain in place on it

        ~limiter_impl() { if (bank != nullptr) mi_limiter_bank_destroy(bank); }
    };
    typedef mi_host::registry<limiter_impl> limiters;

    limiter_impl *impl_of(const void *self) { return limiters::find(self); }
}

Limiter::Limiter()  { construct(); }
Limiter::~Limiter() { destroy(); }

void Limiter::construct()                                       // Limiter.cpp:47-73
{
    limiters::drop(this);                                       // whatever lived at this address before
    fThreshold = 1.0f;
    fReqThreshold = 1.0f;
    fLookahead = 0.0f;
    fMaxLookahead = 0.0f;
    fAttack = 0.0f;
    fRelease = 0.0f;
    fKnee = float(0.50118);                                     // GAIN_AMP_M_6_DB
    nMaxLookahead = 0;
    nLookahead = 0;
    nHead = 0;
    nMaxSampleRate = 0;
    nSampleRate = 0;
    nUpdate = UP_ALL;
    nMode = LM_HERM_THIN;
    sALR.fAttack = 10.0f;
    sALR.fRelease = 50.0f;
    sALR.fEnvelope = 0.0f;
    sALR.fKnee = float(0.56234);                                // GAIN_AMP_M_5_DB
    sALR.bEnable = false;
    vGainBuf = NULL;
    vTmpBuf = NULL;
    vData = NULL;
}

void Limiter::destroy()                                         // :75-85
{
    limiters::drop(this);
    vGainBuf = NULL;
    vTmpBuf = NULL;
    vData = NULL;
}

bool Limiter::init(size_t max_sr, float max_lookahead)          // :87-109
{
    limiters::drop(this);
    limiter_impl *p = limiters::of(this, [max_sr, max_lookahead](limiter_impl &e)
    {
        return mi_limiter_bank_create(&e.bank, 1, uint32_t(max_sr), max_lookahead);
    });
    if (p == nullptr)
        return false;
    nMaxLookahead = size_t(millis_to_samples(float(max_sr), max_lookahead));
    nHead = 0;
    nMaxSampleRate = max_sr;
    fMaxLookahead = max_lookahead;
    // what the setters were given before init()
    mi_limiter_bank_set_sample_rate(p->bank, 0, uint32_t(nSampleRate));
    mi_limiter_bank_set_mode(p->bank, 0, uint32_t(nMode));
    mi_limiter_bank_set_threshold(p->bank, 0, fThreshold, 1);
    mi_limiter_bank_set_threshold(p->bank, 0, fReqThreshold, 0);
    mi_limiter_bank_set_attack(p->bank, 0, fAttack);
    mi_limiter_bank_set_release(p->bank, 0, fRelease);
    mi_limiter_bank_set_lookahead(p->bank, 0, fLookahead);
    mi_limiter_bank_set_knee(p->bank, 0, fKnee);
    mi_limiter_bank_set_alr_attack(p->bank, 0, sALR.fAttack);
    mi_limiter_bank_set_alr_release(p->bank, 0, sALR.fRelease);
    mi_limiter_bank_set_alr_knee(p->bank, 0, sALR.fKnee);
    mi_limiter_bank_set_alr(p->bank, 0, sALR.bEnable ? 1 : 0);
    return true;
}

float Limiter::set_attack(float attack)                         // :111-120
{
    const float old = fAttack;
    if (attack == old)
        return old;
    fAttack = attack;
    nUpdate |= UP_OTHER;
    if (limiter_impl *p = impl_of(this))
        mi_limiter_bank_set_attack(p->bank, 0, attack);
    return old;
}

float Limiter::set_release(float release)                       // :122-131
{
    const float old = fRelease;
    if (release == old)
        return old;
    fRelease = release;
    nUpdate |= UP_OTHER;
    if (limiter_impl *p = impl_of(this))
        mi_limiter_bank_set_release(p->bank, 0, release);
    return old;
}

float Limiter::set_threshold(float thresh, bool immediate)      // :133-144
{
    const float old = fReqThreshold;
    if (old == thresh)
        return old;
    fReqThreshold = thresh;
    if (immediate)
        fThreshold = thresh;
    nUpdate |= UP_THRESH | UP_ALR;
    if (limiter_impl *p = impl_of(this))
        mi_limiter_bank_set_threshold(p->bank, 0, thresh, immediate ? 1 : 0);
    return old;
}

void Limiter::set_mode(limiter_mode_t mode)                     // :146-152
{
    if (size_t(mode) == nMode || size_t(mode) >= MI_LIMITER_MODES)
        return;
    nMode = mode;
    nUpdate |= UP_MODE;
    if (limiter_impl *p = impl_of(this))
        mi_limiter_bank_set_mode(p->bank, 0, uint32_t(mode));
}

void Limiter::set_sample_rate(size_t sr)                        // :154-162
{
    if (sr == nSampleRate)
        return;
    limiter_impl *p = impl_of(this);
    if (p != nullptr && mi_limiter_bank_set_sample_rate(p->bank, 0, uint32_t(sr)) != MI_OK)
        return;                                                 // above init()'s maximum: refused
    nSampleRate = sr;
    nLookahead = size_t(millis_to_samples(float(nSampleRate), fLookahead));
    nUpdate |= UP_SR | UP_ALR | UP_MODE;
}

float Limiter::set_lookahead(float lk_ahead)                    // :164-176
{
    const float old = fLookahead;
    lk_ahead = (lk_ahead < fMaxLookahead) ? lk_ahead : fMaxLookahead;
    if (old == lk_ahead)
        return old;
    fLookahead = lk_ahead;
    nUpdate |= UP_LK;
    nLookahead = size_t(millis_to_samples(float(nSampleRate), fLookahead));
    if (limiter_impl *p = impl_of(this))
        mi_limiter_bank_set_lookahead(p->bank, 0, lk_ahead);
    return old;
}

float Limiter::set_knee(float knee)                             // :178-187
{
    const float old = fKnee;
    if (old == knee)
        return old;
    fKnee = knee;
    nUpdate |= UP_ALR;
    if (limiter_impl *p = impl_of(this))
        mi_limiter_bank_set_knee(p->bank, 0, knee);
    return old;
}

float Limiter::set_alr_attack(float attack)                     // :189-198
{
    const float old = sALR.fAttack;
    if (attack == old)
        return old;
    sALR.fAttack = attack;
    nUpdate |= UP_ALR;
    if (limiter_impl *p = impl_of(this))
        mi_limiter_bank_set_alr_attack(p->bank, 0, attack);
    return old;
}

float Limiter::set_alr_release(float release)                   // :200-209
{
    const float old = sALR.fRelease;
    if (release == old)
        return old;
    sALR.fRelease = release;
    nUpdate |= UP_ALR;
    if (limiter_impl *p = impl_of(this))
        mi_limiter_bank_set_alr_release(p->bank, 0, release);
    return old;
}

bool Limiter::set_alr(bool enable)                              // :211-218
{
    const bool old = sALR.bEnable;
    sALR.bEnable = enable;
    if (!enable)
        sALR.fEnvelope = 0.0f;
    if (limiter_impl *p = impl_of(this))
        mi_limiter_bank_set_alr(p->bank, 0, enable ? 1 : 0);
    return old;
}

float Limiter::set_alr_knee(float knee)                         // :220-229
{
    const float old = sALR.fKnee;
    if (knee == old)
        return old;
    sALR.fKnee = (knee > 1.0f) ? 1.0f / knee : knee;
    nUpdate |= UP_ALR;
    if (limiter_impl *p = impl_of(this))
        mi_limiter_bank_set_alr_knee(p->bank, 0, knee);
    return old;
}

void Limiter::update_settings()                                 // :396-548
{
    if (nUpdate == 0)
        return;
    nLookahead = size_t(millis_to_samples(float(nSampleRate), fLookahead));
    if (nUpdate & UP_THRESH)
        fThreshold = fReqThreshold;                             // (the gains that a lowered threshold scales are the bank's)
    mi_limiter_settings_t s;
    s.sample_rate = uint32_t(nSampleRate);
    s.mode = uint32_t(nMode);
    s.threshold = fThreshold;
    s.lookahead = fLookahead;
    s.attack = fAttack;
    s.release = fRelease;
    s.knee = fKnee;
    s.alr_attack = sALR.fAttack;
    s.alr_release = sALR.fRelease;
    s.alr_knee = sALR.fKnee;
    mi_limiter_params_t p;
    mi::limiter_compute_params(s, p);
    if (nUpdate & UP_ALR)
    {
        sALR.fKS = p.ks, sALR.fKE = p.ke, sALR.fGain = p.gain;
        sALR.fTauAttack = p.tau_attack, sALR.fTauRelease = p.tau_release;
        memcpy(sALR.vHermite, p.hermite, sizeof(sALR.vHermite));
    }
    memset(&sSat, 0, sizeof(sSat));                             // reset_sat / reset_exp / reset_line, then init_*
    sSat.nAttack = p.attack, sSat.nPlane = p.plane, sSat.nRelease = p.release, sSat.nMiddle = p.middle;
    if (nMode >= LM_LINE_THIN)
    {
        memcpy(sLine.vAttack, p.v_attack, sizeof(sLine.vAttack));
        memcpy(sLine.vRelease, p.v_release, sizeof(sLine.vRelease));
    }
    else
    {
        memcpy(sSat.vAttack, p.v_attack, sizeof(sSat.vAttack));
        memcpy(sSat.vRelease, p.v_release, sizeof(sSat.vRelease));
    }
    nUpdate = 0;
    if (limiter_impl *q = impl_of(this))
        mi_limiter_bank_update_settings(q->bank, nullptr);
}

void Limiter::process(float *gain, const float *sc, size_t samples)                    // :695-784
{
    update_settings();
    limiter_impl *p = impl_of(this);
    if (p == nullptr || samples == 0 || !p->buf.reserve(samples))
        return;
    if (!p->buf.up(0, sc, samples) ||
        mi_limiter_bank_process(p->bank, p->buf.row(0), p->buf.row(0), samples, samples, samples, nullptr) != MI_OK ||
        !p->buf.down(gain, 0, samples))
        return;
    uint32_t head = 0;
    float env = 0.0f;
    if (mi_limiter_bank_get_state(p->bank, 0, &head, &env, nullptr, nullptr, nullptr, nullptr) != MI_OK)
        return;
    nHead = head;
    sALR.fEnvelope = env;
}

void Limiter::dump(IStateDumper *v) const                       // :786-892
{
    v->write("fThreshold", fThreshold);
    v->write("fReqThreshold", fReqThreshold);
    v->write("fLookahead", fLookahead);
    v->write("fMaxLookahead", fMaxLookahead);
    v->write("fAttack", fAttack);
    v->write("fRelease", fRelease);
    v->write("fKnee", fKnee);
    v->write("nMaxLookahead", nMaxLookahead);
    v->write("nLookahead", nLookahead);
    v->write("nHead", nHead);
    v->write("nMaxSampleRate", nMaxSampleRate);
    v->write("nSampleRate", nSampleRate);
    v->write("nUpdate", nUpdate);
    v->write("nMode", nMode);
    v->begin_object("sALR", &sALR, sizeof(alr_t));
    {
        v->write("fKS", sALR.fKS);
        v->write("fKE", sALR.fKE);
        v->write("fGain", sALR.fGain);
        v->write("fTauAttack", sALR.fTauAttack);
        v->write("fTauRelease", sALR.fTauRelease);
        v->writev("vHermite", sALR.vHermite, 3);
        v->write("fAttack", sALR.fAttack);
        v->write("fRelease", sALR.fRelease);
        v->write("fEnvelope", sALR.fEnvelope);
        v->write("fKnee", sALR.fKnee);
        v->write("bEnable", sALR.bEnable);
    }
    v->end_object();
    v->write("vGainBuf", vGainBuf);
    v->write("vTmpBuf", vTmpBuf);
    v->write("vData", vData);
    const bool line = nMode >= LM_LINE_THIN, expo = !line && nMode >= LM_EXP_THIN;
    if (nMode > LM_LINE_DUCK)
        return;
    v->begin_object(line ? "sLine" : expo ? "sExp" : "sSat", &sSat, line ? sizeof(line_t) : sizeof(sat_t));
    {
        v->write("nAttack", sSat.nAttack);
        v->write("nPlane", sSat.nPlane);
        v->write("nRelease", sSat.nRelease);
        v->write("nMiddle", sSat.nMiddle);
        if (line)
        {
            v->writev("vAttack", sLine.vAttack, 2);
            v->writev("vRelease", sLine.vRelease, 2);
        }
        else
        {
            v->writev("vAttack", sSat.vAttack, 4);
            v->writev("vRelease", sSat.vRelease, 4);
        }
    }
    v->end_object();
}

} // namespace dspu
} // namespace lsp
