// lsp::dspu::AutoGain and SimpleAutoGain (src/main/dynamics/AutoGain.cpp, SimpleAutoGain.cpp) on banks of one channel
// (autogain.hip).  The classes have no member to hang a bank on (their 128 and 40 bytes are the reference's), so the bank and
// its staging buffer live in a table keyed by the object's address, as for Compressor: made at the first process() call,
// dropped in destroy() and in construct().  Before every device call the bank is handed the object's own computed fields, and
// the state where it is not what was read back after the previous call (the setters of SimpleAutoGain write fCurrGain; a
// subclass may write any of them).  update() is the banks' own (mi_autogain_compute_params, mi_simple_autogain_compute_params).
#include <lsp-plug.in/dsp-units/dynamics/AutoGain.h>
#include <lsp-plug.in/dsp-units/dynamics/SimpleAutoGain.h>

#include <cstring>

#include "autogain_bank.h"
#include "beside.h"

namespace lsp
{
namespace dspu
{
namespace
{
    // the state as the device holds it, beside the object (beside.h)
    struct autogain_held { float gain = 1.0f, out = 1.0f; uint32_t surge = 0; };
    struct simple_held { float gain = 1.0f; };
    typedef mi_host::registry<mi_host::beside<mi_autogain_bank_t, autogain_held, mi_autogain_bank_destroy> > autogains;
    typedef mi_host::registry<mi_host::beside<mi_simple_autogain_bank_t, simple_held, mi_simple_autogain_bank_destroy> > simples;

    int send_autogain_state(mi_autogain_bank_t *bank, const autogain_held &s)
    {
        return mi::autogain_bank_set_state(bank, 0, s.gain, s.out, s.surge, nullptr);
    }
    int send_simple_state(mi_simple_autogain_bank_t *bank, const simple_held &s)
    {
        return mi::simple_autogain_bank_set_state(bank, 0, s.gain, nullptr);
    }
}

AutoGain::AutoGain()  { construct(); }
AutoGain::~AutoGain() { destroy(); }

void AutoGain::construct()                                      // AutoGain.cpp:43-66
{
    autogains::drop(this);                                      // whatever lived at this address before
    nSampleRate = 0;
    sShort.fGrow = sShort.fFall = sShort.fKGrow = sShort.fKFall = 0.0f;
    sLong.fGrow = sLong.fFall = sLong.fKGrow = sLong.fKFall = 0.0f;
    init_compressor(sShortComp);
    init_compressor(sOutComp);
    fSilence = float(2.5119e-4);                                // GAIN_AMP_M_72_DB
    fDeviation = float(1.99526);                                // GAIN_AMP_P_6_DB
    fCurrGain = 1.0f;
    fMaxGain = float(3.98107);                                  // GAIN_AMP_P_12_DB
    fOutGain = 1.0f;
    nFlags = F_UPDATE;
}

void AutoGain::destroy()                                        // :68-70
{
    autogains::drop(this);
}

void AutoGain::init_compressor(compressor_t &c)                 // :72-81
{
    c.x1 = 1.0f;
    c.x2 = 1.0f;
    c.t = 1.0f;
    c.a = c.b = c.c = c.d = 0.0f;
}

status_t AutoGain::init()                                       // :83-88
{
    destroy();
    return STATUS_OK;
}

void AutoGain::set_timing(float *ptr, float value)              // :90-98
{
    value = (value > 0.0f) ? value : 0.0f;
    if (*ptr == value)
        return;
    *ptr = value;
    nFlags |= F_UPDATE;
}

status_t AutoGain::set_sample_rate(size_t sample_rate)          // :100-109
{
    if (nSampleRate == sample_rate)
        return STATUS_OK;
    nSampleRate = sample_rate;
    nFlags |= F_UPDATE;
    return STATUS_OK;
}

void AutoGain::set_silence_threshold(float threshold)           // :111-115
{
    fSilence = (0.0f > threshold) ? 0.0f : threshold;
}

void AutoGain::set_deviation(float deviation)                   // :117-125
{
    deviation = (1.0f > deviation) ? 1.0f : deviation;
    if (deviation == fDeviation)
        return;
    fDeviation = deviation;
    nFlags |= F_UPDATE;
}

void AutoGain::set_short_speed(float grow, float fall)          // :127-131
{
    set_timing(&sShort.fGrow, grow);
    set_timing(&sShort.fFall, fall);
}

void AutoGain::set_long_speed(float grow, float fall)           // :133-137
{
    set_timing(&sLong.fGrow, grow);
    set_timing(&sLong.fFall, fall);
}

void AutoGain::set_max_gain(float value, bool enable)           // :139-143
{
    fMaxGain = (0.0f > value) ? 0.0f : value;
    nFlags = enable ? (nFlags | F_MAX_GAIN) : (nFlags & ~size_t(F_MAX_GAIN));
}

void AutoGain::set_max_gain(float value)                        // :145-148
{
    fMaxGain = (0.0f > value) ? 0.0f : value;
}

void AutoGain::enable_max_gain(bool enable)                     // :150-153
{
    nFlags = enable ? (nFlags | F_MAX_GAIN) : (nFlags & ~size_t(F_MAX_GAIN));
}

void AutoGain::enable_quick_amplifier(bool enable)              // :175-178
{
    nFlags = enable ? (nFlags | F_QUICK_AMP) : (nFlags & ~size_t(F_QUICK_AMP));
}

void AutoGain::update()                                         // :155-173
{
    if (!(nFlags & F_UPDATE))
        return;
    mi_autogain_settings_t s = {};
    s.sample_rate = uint32_t(nSampleRate);
    s.short_grow = sShort.fGrow, s.short_fall = sShort.fFall, s.long_grow = sLong.fGrow, s.long_fall = sLong.fFall;
    s.silence = fSilence, s.deviation = fDeviation, s.max_gain = fMaxGain;
    mi_autogain_params_t p;
    mi_autogain_compute_params(&s, &p);
    sShort.fKGrow = p.short_kgrow, sShort.fKFall = p.short_kfall;
    sLong.fKGrow = p.long_kgrow, sLong.fKFall = p.long_kfall;
    static_assert(sizeof(sShortComp) == sizeof(p.short_comp), "curve layouts");
    memcpy(&sShortComp, &p.short_comp, sizeof(sShortComp));
    memcpy(&sOutComp, &p.out_comp, sizeof(sOutComp));
    nFlags &= ~size_t(F_UPDATE);
}

// both process() overloads: the rows go to the device side by side, the gain comes back from the first of them
void AutoGain::run(float *vca, const float *llong, const float *lshort, const float *lexp, float level, size_t count)
{
    update();
    autogains::entry *p = autogains::of_one(this, mi_autogain_bank_create);
    if (p == nullptr || count == 0 || !p->buf.reserve(count, 3))
        return;
    mi_autogain_params_t q;
    q.short_kgrow = sShort.fKGrow, q.short_kfall = sShort.fKFall, q.long_kgrow = sLong.fKGrow, q.long_kfall = sLong.fKFall;
    memcpy(&q.short_comp, &sShortComp, sizeof(q.short_comp));
    memcpy(&q.out_comp, &sOutComp, sizeof(q.out_comp));
    q.silence = fSilence, q.deviation = fDeviation, q.max_gain = fMaxGain;
    q.flags = uint32_t(nFlags) & (MI_AG_QUICK_AMP | MI_AG_MAX_GAIN);
    if (mi::autogain_bank_set_params(p->bank, 0, &q) != MI_OK)
        return;
    const uint32_t surge = uint32_t(nFlags) & (MI_AG_SURGE_UP | MI_AG_SURGE_DOWN);
    if (!p->hand_over_state({ fCurrGain, fOutGain, surge }, send_autogain_state))
        return;
    float *d_long = p->buf.row(0), *d_short = p->buf.row(1), *d_exp = p->buf.row(2);
    if (!p->buf.up(0, llong, count) || !p->buf.up(1, lshort, count))
        return;
    if (lexp != nullptr)
    {
        if (!p->buf.up(2, lexp, count) ||
            mi_autogain_bank_process(p->bank, d_long, d_long, d_short, d_exp, count, count, count, count, count, nullptr) != MI_OK)
            return;
    }
    else if (!p->buf.up(2, &level, 1) ||
             mi_autogain_bank_process_level(p->bank, d_long, d_long, d_short, d_exp, count, count, count, count, nullptr) != MI_OK)
        return;
    if (!p->buf.down(vca, 0, count))
        return;
    uint32_t flags = 0;
    if (mi_autogain_bank_get_state(p->bank, 0, &p->held.gain, &p->held.out, &flags, nullptr) != MI_OK)
        return;
    p->held.surge = flags & (MI_AG_SURGE_UP | MI_AG_SURGE_DOWN);
    fCurrGain = p->held.gain, fOutGain = p->held.out;
    nFlags = (nFlags & ~size_t(F_SURGE_UP | F_SURGE_DOWN)) | p->held.surge;
}

void AutoGain::process(float *vca, const float *llong, const float *lshort, const float *lexp, size_t count)   // :278-286
{
    run(vca, llong, lshort, lexp, 0.0f, count);
}

void AutoGain::process(float *vca, const float *llong, const float *lshort, float lexp, size_t count)          // :288-296
{
    run(vca, llong, lshort, nullptr, lexp, count);
}

void AutoGain::dump(const char *id, const timing_t *t, IStateDumper *v)         // :298-308
{
    v->begin_object(id, t, sizeof(timing_t));
    v->write("fGrow", t->fGrow);
    v->write("fFall", t->fFall);
    v->write("fKGrow", t->fKGrow);
    v->write("fKFall", t->fKFall);
    v->end_object();
}

void AutoGain::dump(const char *id, const compressor_t *c, IStateDumper *v)     // :310-323
{
    v->begin_object(id, c, sizeof(compressor_t));
    v->write("x1", c->x1);
    v->write("x2", c->x2);
    v->write("t", c->t);
    v->write("a", c->a);
    v->write("b", c->b);
    v->write("c", c->c);
    v->write("d", c->d);
    v->end_object();
}

void AutoGain::dump(IStateDumper *v) const                      // :325-339 (fMaxGain is not written there either)
{
    v->write("nSampleRate", nSampleRate);
    v->write("nFlags", nFlags);
    dump("sShort", &sShort, v);
    dump("sLong", &sLong, v);
    dump("sShortComp", &sShortComp, v);
    dump("sOutComp", &sOutComp, v);
    v->write("fSilence", fSilence);
    v->write("fDeviation", fDeviation);
    v->write("fCurrGain", fCurrGain);
    v->write("fOutGain", fOutGain);
}

SimpleAutoGain::SimpleAutoGain()  { construct(); }
SimpleAutoGain::~SimpleAutoGain() { destroy(); }

void SimpleAutoGain::construct()                                // SimpleAutoGain.cpp:43-56
{
    simples::drop(this);
    nSampleRate = 0;
    nFlags = F_UPDATE;
    fKGrow = 0.0f;
    fKFall = 0.0f;
    fGrow = 0.0f;
    fFall = 0.0f;
    fThreshold = 0.0f;
    fCurrGain = 1.0f;
    fMinGain = 0.000001f;
    fMaxGain = 1.0f;
}

void SimpleAutoGain::destroy()                                  // :58-60
{
    simples::drop(this);
}

status_t SimpleAutoGain::init()                                 // :62-66
{
    destroy();
    return STATUS_OK;
}

status_t SimpleAutoGain::set_sample_rate(size_t sample_rate)    // :68-77
{
    if (nSampleRate == sample_rate)
        return STATUS_OK;
    nSampleRate = uint32_t(sample_rate);
    nFlags |= F_UPDATE;
    return STATUS_OK;
}

void SimpleAutoGain::set_grow(float value)                      // :79-86
{
    if (fGrow == value)
        return;
    fGrow = value;
    nFlags |= F_UPDATE;
}

void SimpleAutoGain::set_fall(float value)                      // :88-95
{
    if (fFall == value)
        return;
    fFall = value;
    nFlags |= F_UPDATE;
}

void SimpleAutoGain::set_speed(float grow, float fall)          // :97-106
{
    if ((fGrow == grow) && (fFall == fall))
        return;
    fGrow = grow;
    fFall = fall;
    nFlags |= F_UPDATE;
}

void SimpleAutoGain::set_max_gain(float value)                  // :108-115
{
    if (fMaxGain == value)
        return;
    fMaxGain = value;
    fCurrGain = (fCurrGain < fMaxGain) ? fCurrGain : fMaxGain;           // lsp_min
}

void SimpleAutoGain::set_min_gain(float value)                  // :117-124
{
    if (fMinGain == value)
        return;
    fMinGain = value;
    fCurrGain = (fCurrGain > fMinGain) ? fCurrGain : fMinGain;           // lsp_max
}

void SimpleAutoGain::set_gain(float min, float max)             // :126-135
{
    if ((fMinGain == min) && (fMaxGain == max))
        return;
    fMinGain = min;
    fMaxGain = max;
    fCurrGain = gain();                                         // lsp_limit
}

void SimpleAutoGain::set_threshold(float threshold)             // :137-140
{
    fThreshold = threshold;
}

void SimpleAutoGain::update()                                   // :142-153
{
    if (!(nFlags & F_UPDATE))
        return;
    mi_simple_autogain_settings_t s = { nSampleRate, fGrow, fFall, fThreshold, fMinGain, fMaxGain };
    mi_simple_autogain_params_t p;
    mi_simple_autogain_compute_params(&s, &p);
    fKGrow = p.kgrow;
    fKFall = p.kfall;
    nFlags &= ~uint32_t(F_UPDATE);
}

void SimpleAutoGain::process(float *dst, const float *src, size_t count)        // :155-175
{
    update();
    simples::entry *p = simples::of_one(this, mi_simple_autogain_bank_create);
    if (p == nullptr || count == 0 || !p->buf.reserve(count, 1))
        return;
    const mi_simple_autogain_params_t q = { fKGrow, fKFall, fThreshold, fMinGain, fMaxGain };
    if (mi::simple_autogain_bank_set_params(p->bank, 0, &q) != MI_OK)
        return;
    if (!p->hand_over_state({ fCurrGain }, send_simple_state))
        return;
    if (!p->buf.up(0, src, count) ||
        mi_simple_autogain_bank_process(p->bank, p->buf.row(0), p->buf.row(0), count, count, count, nullptr) != MI_OK ||
        !p->buf.down(dst, 0, count) ||
        mi_simple_autogain_bank_get_state(p->bank, 0, &p->held.gain, nullptr) != MI_OK)
        return;
    fCurrGain = p->held.gain;
}

float SimpleAutoGain::process(float src)                        // :177-194: one sample on the device
{
    float out = 0.0f;
    process(&out, &src, 1);
    return out;
}

void SimpleAutoGain::dump(IStateDumper *v) const                // :196-209
{
    v->write("nSampleRate", nSampleRate);
    v->write("nFlags", nFlags);
    v->write("fKGrow", fKGrow);
    v->write("fKFall", fKFall);
    v->write("fGrow", fGrow);
    v->write("fFall", fFall);
    v->write("fThreshold", fThreshold);
    v->write("fCurrGain", fCurrGain);
    v->write("fMinGain", fMinGain);
    v->write("fMaxGain", fMaxGain);
}

} // namespace dspu
} // namespace lsp
