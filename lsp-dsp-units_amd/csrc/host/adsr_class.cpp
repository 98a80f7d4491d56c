// lsp::dspu::ADSREnvelope (src/main/util/ADSREnvelope.cpp) on a mi_adsr_bank of one channel kept beside the object (beside.h), and
// lsp::dspu::interpolation's two Hermite designs.  The object's fields are what counts: the setters are the reference's line for
// line (a NaN is refused), update_settings() takes the clamped times and the designed curves from mi_adsr_settings_update (the
// bank's own designer, no device) and names each curve's generator.  The scalar process(float) evaluates on the host
// (mi_adsr_settings_process: the device's arithmetic, its rule for expf included).  The array methods hand the fields to the bank,
// stage the caller's rows on the device and run the bank's kernel; the unit has no state to read back.
#include <lsp-plug.in/dsp-units/util/ADSREnvelope.h>
#include <lsp-plug.in/dsp-units/misc/interpolation.h>

#include <cmath>
#include <cstddef>

#include "adsr_bank.h"
#include "beside.h"

#pragma clang fp contract(off)

namespace lsp
{
namespace dspu
{
namespace interpolation
{
    void hermite_cubic(float *p, float x0, float y0, float k0, float x1, float y1, float k1)
    {
        mi_interpolation_hermite_cubic(p, x0, y0, k0, x1, y1, k1);
    }

    void hermite_quadro(float *p, float x0, float y0, float k0, float x1, float y1, float k1, float x2, float y2)
    {
        mi_interpolation_hermite_quadro(p, x0, y0, k0, x1, y1, k1, x2, y2);
    }
}

namespace
{
    struct adsr_held { uint32_t unused = 0; };                  // the unit has no state on the device
    typedef mi_host::registry<mi_host::beside<mi_adsr_bank_t, adsr_held, mi_adsr_bank_destroy> > envelopes;

    static_assert(sizeof(void *) != 8 || sizeof(ADSREnvelope) == 208, "sizeof(ADSREnvelope)");

    inline float lsp_limit(float x, float lo, float hi)     { return (x < lo) ? lo : ((x > hi) ? hi : x); }

    enum { OP_PROCESS, OP_PROCESS_MUL, OP_GENERATE, OP_GENERATE_MUL, OP_GENERATE_MUL_SRC };
}

ADSREnvelope::ADSREnvelope()    { construct(); }
ADSREnvelope::~ADSREnvelope()   { destroy(); }

void ADSREnvelope::construct()                                  // :40-58
{
    envelopes::drop(this);                                      // whatever lived at this address before
    for (size_t i = 0; i < P_TOTAL; ++i)
    {
        curve_t *cv         = &vCurve[i];
        cv->fTime           = 0.0f;
        cv->fCurve          = 0.5f;
        cv->enFunction      = ADSR_NONE;
        cv->pGenerator      = none_generator;
        memset(&cv->sParams, 0, sizeof(cv->sParams));           // (the reference leaves all but sNone.fK and fB unset)
    }
    fHoldTime       = 0.0f;
    fBreakLevel     = 0.0f;
    fSustainLevel   = 0.0f;
    nFlags          = F_RECONFIGURE;
}

void ADSREnvelope::destroy()
{
    envelopes::drop(this);
}

void ADSREnvelope::set_param(float &param, float value)        // :65-73
{
    if (std::isnan(value))
        return;                                                 // lsp_limit lets it through and nothing after that is defined
    const float normalized = lsp_limit(value, 0.0f, 1.0f);
    if (param == normalized)
        return;
    param           = normalized;
    nFlags         |= F_RECONFIGURE;
}

void ADSREnvelope::set_function(function_t &func, function_t value)    // :75-82
{
    if (func == value)
        return;
    func            = value;
    nFlags         |= F_RECONFIGURE;
}

void ADSREnvelope::set_flag(uint32_t flag, bool set)            // :84-89
{
    const bool on   = nFlags & flag;
    if (set != on)
        nFlags          = (set ? (nFlags | flag) : (nFlags & ~flag)) | F_RECONFIGURE;
}

void ADSREnvelope::set_curve(part_t part, float time, float curve, function_t func)    // :91-105
{
    if (std::isnan(time) || std::isnan(curve))
        return;
    curve_t *cv     = &vCurve[part];
    time            = lsp_limit(time, 0.0f, 1.0f);
    curve           = lsp_limit(curve, 0.0f, 1.0f);
    if ((cv->fTime == time) && (cv->fCurve == curve) && (cv->enFunction == func))
        return;
    cv->fTime       = time;
    cv->fCurve      = curve;
    cv->enFunction  = func;
    nFlags         |= F_RECONFIGURE;
}

void ADSREnvelope::set_hold(float time, bool enabled)           // :107-111
{
    set_param(fHoldTime, time);
    set_flag(F_USE_HOLD, enabled);
}

void ADSREnvelope::set_break(float level, bool enabled)         // :113-117
{
    set_param(fBreakLevel, level);
    set_flag(F_USE_BREAK, enabled);
}

namespace
{
    // the object's fields as the designer's settings, and back
    template <class Curve> void to_settings(mi_adsr_settings_t &s, const Curve *vCurve, float hold, float brk, float sustain, uint32_t flags)
    {
        for (int i = 0; i < MI_ADSR_PARTS; ++i)
        {
            s.curve[i].time = vCurve[i].fTime, s.curve[i].curve = vCurve[i].fCurve, s.curve[i].function = uint32_t(vCurve[i].enFunction);
            memcpy(s.curve[i].params, &vCurve[i].sParams, sizeof(s.curve[i].params));
        }
        s.hold_time = hold, s.break_level = brk, s.sustain_level = sustain, s.flags = flags;
    }
}

void ADSREnvelope::update_settings()                            // :238-293
{
    if (!(nFlags & F_RECONFIGURE))
        return;
    static_assert(sizeof(gen_params_t) == sizeof(float) * 6, "gen_params_t is the designer's six floats");
    mi_adsr_settings_t s;
    to_settings(s, vCurve, fHoldTime, fBreakLevel, fSustainLevel, nFlags);
    if (mi_adsr_settings_update(&s) != MI_OK)
        return;
    for (size_t i = 0; i < P_TOTAL; ++i)
    {
        curve_t *cv         = &vCurve[i];
        cv->fTime           = s.curve[i].time;
        memcpy(&cv->sParams, s.curve[i].params, sizeof(cv->sParams));
        switch (cv->enFunction)                                 // configure_curve's generators, :124-236
        {
            case ADSR_LINE: case ADSR_LINE2:    cv->pGenerator = line_generator; break;
            case ADSR_CUBIC:                    cv->pGenerator = cubic_generator; break;
            case ADSR_QUADRO:                   cv->pGenerator = quadro_generator; break;
            case ADSR_EXP:                      cv->pGenerator = exp_generator; break;
            default:                            cv->pGenerator = none_generator; break;
        }
    }
    fHoldTime       = s.hold_time;
    nFlags          = s.flags;
}

// the generators, :350-383: adsr_bank.h's, on a record that holds the parameters as curve 0
namespace
{
    template <class Params> float generate_with(uint32_t fn, const Params *params, float t)
    {
        mi_adsr::record r = {};
        r.fn[0] = fn;
        memcpy(r.p[0], params, sizeof(r.p[0]));
        return mi_adsr::curve<0>(r, t);
    }
}
float ADSREnvelope::none_generator(float t, const gen_params_t *params)    { return generate_with(MI_ADSR_NONE, params, t); }
float ADSREnvelope::line_generator(float t, const gen_params_t *params)    { return generate_with(MI_ADSR_LINE, params, t); }
float ADSREnvelope::cubic_generator(float t, const gen_params_t *params)   { return generate_with(MI_ADSR_CUBIC, params, t); }
float ADSREnvelope::quadro_generator(float t, const gen_params_t *params)  { return generate_with(MI_ADSR_QUADRO, params, t); }
float ADSREnvelope::exp_generator(float t, const gen_params_t *params)     { return generate_with(MI_ADSR_EXP, params, t); }

float ADSREnvelope::do_process(float t)                         // :295-326
{
    mi_adsr_settings_t s;
    to_settings(s, vCurve, fHoldTime, fBreakLevel, fSustainLevel, nFlags);
    float v = 0.0f;
    mi_adsr_settings_process(&s, t, &v);
    return v;
}

float ADSREnvelope::process(float value)                        // :328-332
{
    update_settings();
    return do_process(value);
}

namespace
{
    // one array operation of one object through its bank: the fields go over, the rows are staged, the result comes back
    bool run(const void *self, const mi_adsr_settings_t &s, int op, float *dst, const float *src, float start, float step, size_t count)
    {
        if (count == 0 || dst == NULL)
            return true;
        envelopes::entry *p = envelopes::of_one(self, mi_adsr_bank_create);
        if (p == NULL || !p->buf.reserve(count, 2))
            return false;
        if (mi_adsr_bank_set_settings(p->bank, 0, &s) != MI_OK)
            return false;
        float *d_dst = p->buf.row(0), *d_src = p->buf.row(1);
        const bool reads_dst = op == OP_PROCESS_MUL || op == OP_GENERATE_MUL, reads_src = op != OP_GENERATE && op != OP_GENERATE_MUL;
        if (reads_src && src == NULL)
            return false;
        if (reads_dst && !p->buf.up(0, dst, count))
            return false;
        if (reads_src && !p->buf.up(1, src, count))
            return false;
        int r;
        switch (op)
        {
            case OP_PROCESS:        r = mi_adsr_bank_process(p->bank, d_dst, d_src, count, count, count, NULL); break;
            case OP_PROCESS_MUL:    r = mi_adsr_bank_process_mul(p->bank, d_dst, d_src, count, count, count, NULL); break;
            case OP_GENERATE:       r = mi_adsr_bank_generate(p->bank, d_dst, &start, &step, count, count, NULL); break;
            case OP_GENERATE_MUL:   r = mi_adsr_bank_generate_mul(p->bank, d_dst, NULL, &start, &step, count, count, count, NULL); break;
            default:                r = mi_adsr_bank_generate_mul(p->bank, d_dst, d_src, &start, &step, count, count, count, NULL); break;
        }
        return r == MI_OK && p->buf.down(dst, 0, count) && mi_dspu_stream_synchronize(NULL) == MI_OK;
    }
}

#define ADSR_RUN(op, dst, src, start, step, count) \
    do { \
        update_settings(); \
        mi_adsr_settings_t s; \
        to_settings(s, vCurve, fHoldTime, fBreakLevel, fSustainLevel, nFlags); \
        run(this, s, op, dst, src, start, step, count); \
    } while (0)

void ADSREnvelope::process(float *dst, const float *src, size_t count)                  { ADSR_RUN(OP_PROCESS, dst, src, 0.0f, 0.0f, count); }
void ADSREnvelope::process_mul(float *dst, const float *src, size_t count)              { ADSR_RUN(OP_PROCESS_MUL, dst, src, 0.0f, 0.0f, count); }
void ADSREnvelope::generate(float *dst, float start, float step, size_t count)          { ADSR_RUN(OP_GENERATE, dst, NULL, start, step, count); }
void ADSREnvelope::generate_mul(float *dst, float start, float step, size_t count)      { ADSR_RUN(OP_GENERATE_MUL, dst, NULL, start, step, count); }
void ADSREnvelope::generate_mul(float *dst, const float *src, float start, float step, size_t count)
{
    ADSR_RUN(OP_GENERATE_MUL_SRC, dst, src, start, step, count);
}
#undef ADSR_RUN

void ADSREnvelope::dump(IStateDumper *v) const                  // :535-622, the reference's calls in the reference's order
{
    v->begin_array("vCurve", vCurve, P_TOTAL);
    {
        for (size_t i = 0; i < P_TOTAL; ++i)
        {
            const curve_t *c = &vCurve[i];
            v->begin_object(c, sizeof(curve_t));
            v->write("fTime", c->fTime);
            v->write("fCurve", c->fCurve);
            v->write("enFunction", int(c->enFunction));
            v->write("pGenerator", reinterpret_cast<const void *>(c->pGenerator));
            v->begin_object("sParams", &c->sParams, sizeof(gen_params_t));
            {
                switch (c->enFunction)
                {
                    case ADSR_LINE:
                    case ADSR_LINE2:
                    {
                        const gen_line_t *g = &c->sParams.sLine;
                        v->begin_object("sLine", g, sizeof(gen_line_t));
                        v->write("fT2", g->fT2);
                        v->write("fK1", g->fK1);
                        v->write("fB1", g->fB1);
                        v->write("fK2", g->fK2);
                        v->write("fB2", g->fB2);
                        v->end_object();
                        break;
                    }
                    case ADSR_CUBIC:
                    case ADSR_QUADRO:
                    {
                        const gen_hermite_t *g = &c->sParams.sHermite;
                        v->begin_object("sHermite", g, sizeof(gen_hermite_t));
                        v->write("fT0", g->fT0);
                        v->writev("fK", g->fK, (c->enFunction == ADSR_CUBIC) ? 4 : 5);
                        v->end_object();
                        break;
                    }
                    case ADSR_EXP:
                    {
                        const gen_exp_t *g = &c->sParams.sExp;
                        v->begin_object("sExp", g, sizeof(gen_exp_t));
                        v->write("fT0", g->fT0);
                        v->write("fKT", g->fKT);
                        v->writev("fA", g->fA, 2);
                        v->writev("fB", g->fB, 2);
                        v->end_object();
                        break;
                    }
                    default:
                    {
                        const gen_none_t *g = &c->sParams.sNone;
                        v->begin_object("sNone", g, sizeof(gen_none_t));
                        v->write("fT", g->fT);
                        v->write("fK", g->fK);
                        v->write("fB", g->fB);
                        v->end_object();
                        break;
                    }
                }
            }
            v->end_object();                                    // (the curve's own object stays open in the reference too)
        }
    }
    v->end_array();

    v->write("fHoldTime", fHoldTime);
    v->write("fBreakLevel", fBreakLevel);
    v->write("fSustainLevel", fSustainLevel);
    v->write("nFlags", nFlags);
}

} // namespace dspu
} // namespace lsp
