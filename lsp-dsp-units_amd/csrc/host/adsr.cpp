// The settings arithmetic of lsp::dspu::ADSREnvelope (src/main/util/ADSREnvelope.cpp:40-293): construct(), the setters and
// update_settings() on a mi_adsr_settings_t, shared by the bank (csrc/adsr.hip) and by whoever wants the designed curves without a
// device, and the two Hermite designs of src/main/misc/interpolation.cpp that it calls.  Host float32 in the reference's order;
// where the reference assigns to a double or meets one, so does this.  expf(-fKT) is the host libm's, as in the reference.
#include "adsr_bank.h"
#include "mi_common.h"

#include <cmath>
#include <cstdint>

#pragma clang fp contract(off)

namespace
{
    static_assert(sizeof(mi_adsr_curve_t) == 36 && sizeof(mi_adsr_settings_t) == 160, "mi_adsr_settings_t: the Python binding mirrors this layout");

    inline float limit01(float x) { return (x < 0.0f) ? 0.0f : ((x > 1.0f) ? 1.0f : x); }      // lsp_limit(x, 0.0f, 1.0f)
    inline float limit_range(float t, float prev) { return limit01((t > prev) ? t : prev); }  // :119-122

    // set_param, :65-73
    inline void set_param(mi_adsr_settings_t *s, float &param, float value)
    {
        const float normalized = limit01(value);
        if (param == normalized)
            return;
        param = normalized;
        s->flags |= MI_ADSR_RECONFIGURE;
    }
    // set_function, :75-82
    inline void set_function(mi_adsr_settings_t *s, uint32_t &func, uint32_t value)
    {
        if (func == value)
            return;
        func = value;
        s->flags |= MI_ADSR_RECONFIGURE;
    }
    // set_flag, :84-89
    inline void set_flag(mi_adsr_settings_t *s, uint32_t flag, bool set)
    {
        const bool on = s->flags & flag;
        if (set != on)
            s->flags = (set ? (s->flags | flag) : (s->flags & ~flag)) | MI_ADSR_RECONFIGURE;
    }
    // set_curve, :91-105
    inline void set_curve(mi_adsr_settings_t *s, int part, float time, float curve, uint32_t func)
    {
        mi_adsr_curve_t *cv = &s->curve[part];
        time = limit01(time);
        curve = limit01(curve);
        if ((cv->time == time) && (cv->curve == curve) && (cv->function == func))
            return;
        cv->time = time, cv->curve = curve, cv->function = func;
        s->flags |= MI_ADSR_RECONFIGURE;
    }

    // interpolation.cpp:33-98
    void swap_rows(double *a, double *b, size_t count)
    {
        for (size_t i = 0; i < count; ++i)
        {
            const double tmp = a[i];
            a[i] = b[i];
            b[i] = tmp;
        }
    }
    void sub_row(double *a, const double *b, size_t count)
    {
        const double k = a[0] / b[0];
        a[0] = 0.0f;
        for (size_t i = 1; i < count; ++i)
            a[i] -= k * b[i];
    }
    double solve_row(const double *row, const double *c, size_t count)
    {
        double sum = row[count];
        for (size_t i = 1; i < count; ++i)
            sum += row[i] * c[i];
        return -sum / row[0];
    }
    void solve_matrix(double *c, double *m, size_t vars)
    {
        const size_t cols = vars + 1;
        for (size_t i = 0; i < vars; ++i)
        {
            double *srow = &m[i * cols + i];
            if (fabs(srow[0]) < 1e-20f)
            {
                for (size_t j = i; j < vars; ++j)
                {
                    double *drow = &m[j * cols + i];
                    if (fabs(drow[0]) >= 1e-20f)
                    {
                        swap_rows(srow, drow, cols - i);
                        break;
                    }
                }
            }
            for (size_t j = i + 1; j < vars; ++j)
            {
                double *drow = &m[j * cols + i];
                if (fabs(drow[0]) < 1e-20f)
                    continue;
                sub_row(drow, srow, cols - i);
            }
        }
        for (size_t i = vars; i-- > 0; )
            c[i] = solve_row(&m[i * cols + i], &c[i], vars - i);
    }

    // interpolation::hermite_cubic, :112-131: the differences and products of float arguments are float32, what is assigned to a
    // double or meets one is double
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

    // interpolation::hermite_quadro, :134-177
    void hermite_quadro(float *p, float x0, float y0, float k0, float x1, float y1, float k1, float x2, float y2)
    {
        double m[5 * 6];
        const double X[3] = { x0, x1, x2 };
        const double Y[3] = { y0, y1, y2 };
        const double K[2] = { k0, k1 };
        for (size_t i = 0; i < 3; ++i)
        {
            const double x = X[i];
            double *r0 = &m[i * 6];
            r0[5] = -Y[i];
            r0[4] = 1.0;
            r0[3] = x;
            r0[2] = x * x;
            r0[1] = x * r0[2];
            r0[0] = r0[2] * r0[2];
            if (i < 2)
            {
                double *r1 = &m[(i + 3) * 6];
                r1[5] = -K[i];
                r1[4] = 0.0;
                r1[3] = 1.0;
                r1[2] = 2.0 * x;
                r1[1] = 3.0 * r0[2];
                r1[0] = 4.0 * r0[1];
            }
        }
        double c[5];
        solve_matrix(c, m, 5);
        for (size_t i = 0; i < 5; ++i)
            p[i] = float(c[i]);
    }

    // configure_curve, :124-236
    void configure_curve(mi_adsr_curve_t *curve, float x0, float x1, float y0, float y1)
    {
        float *g = curve->params;
        switch (curve->function)
        {
            case MI_ADSR_LINE:
            case MI_ADSR_LINE2:
            {
                // { fT2, fK1, fB1, fK2, fB2 }
                g[0] = (curve->function == MI_ADSR_LINE) ? 0.5f * (x0 + x1) : x1 + (x0 - x1) * curve->curve;
                const float cy = y0 + (y1 - y0) * curve->curve;
                g[1] = (cy - y0) / (g[0] - x0);
                g[2] = y0 - g[1] * x0;
                g[3] = (y1 - cy) / (x1 - g[0]);
                g[4] = cy - g[3] * g[0];
                break;
            }
            case MI_ADSR_CUBIC:
            {
                const float cx = 0.5f * (x0 + x1);
                const float cy = y0 + (y1 - y0) * curve->curve;
                const float k0 = (cy - y0) / (cx - x0);
                const float k1 = (y1 - cy) / (x1 - cx);
                g[0] = x0;
                hermite_cubic(&g[1], 0.0f, y0, k0, x1 - x0, y1, k1);
                break;
            }
            case MI_ADSR_QUADRO:
            {
                const float cx = 0.5f * (x0 + x1);
                const float cy = y0 + (y1 - y0) * (0.3f + curve->curve * 0.4f);
                g[0] = x0;
                hermite_quadro(&g[1], 0.0f, y0, 0.0f, x1 - x0, y1, 0.0f, cx - x0, cy);
                break;
            }
            case MI_ADSR_EXP:
            {
                // { fT0, fKT, fA[2], fB[2] }
                const float kt = 0.5f - curve->curve;
                const float ndx = 1.0f / (x1 - x0);
                g[0] = x0;
                g[1] = fabsf(kt) * 40.0f;
                const float ny = expf(-g[1]);
                if (kt >= 0.0f)
                    g[2] = y0, g[3] = (y1 - y0) * ny, g[4] = ndx, g[5] = 0.0f;
                else
                    g[2] = y1, g[3] = (y0 - y1) * ny, g[4] = -ndx, g[5] = 1.0f;
                break;
            }
            case MI_ADSR_NONE:
            default:
                // { fT, fK, fB }
                g[0] = x0;
                g[1] = (y1 - y0) / (x1 - x0);
                g[2] = y0;
                break;
        }
    }

    inline bool as_function(double v, uint32_t *f)
    {
        if (!(v >= 0.0 && v <= 4294967295.0) || v != std::floor(v))
            return false;
        *f = uint32_t(v);
        return true;
    }
} // namespace

extern "C" {

int mi_adsr_settings_init(mi_adsr_settings_t *s)                                        // construct(), :40-58
{
    MI_REQUIRE(s != nullptr, MI_EINVAL, "mi_adsr_settings_init: NULL settings");
    *s = mi_adsr_settings_t();
    for (int i = 0; i < MI_ADSR_PARTS; ++i)
    {
        s->curve[i].time = 0.0f;
        s->curve[i].curve = 0.5f;
        s->curve[i].function = MI_ADSR_NONE;
    }
    s->flags = MI_ADSR_RECONFIGURE;
    return MI_OK;
}

int mi_adsr_settings_set(mi_adsr_settings_t *s, uint32_t setter, double a, double b, double c)
{
    MI_REQUIRE(s != nullptr, MI_EINVAL, "mi_adsr_settings_set: NULL settings");
    MI_REQUIRE(setter <= MI_ADSR_SET_RELEASE, MI_EINVAL, "mi_adsr_settings_set: no setter %u", setter);
    // a NaN passes lsp_limit and what update_settings makes of it is not defined: refused, and nothing changes
    const bool three = setter == MI_ADSR_SET_ATTACK || setter == MI_ADSR_SET_DECAY || setter == MI_ADSR_SET_SLOPE || setter == MI_ADSR_SET_RELEASE;
    const bool two = setter == MI_ADSR_SET_HOLD || setter == MI_ADSR_SET_BREAK;
    MI_REQUIRE(!std::isnan(a) && !((three || two) && std::isnan(b)) && !(three && std::isnan(c)), MI_EINVAL,
               "mi_adsr_settings_set: setter %u was given a NaN", setter);
    const float fa = float(a), fb = float(b);
    uint32_t fn = 0;
    static const int PART_OF[4] = { MI_ADSR_ATTACK, MI_ADSR_DECAY, MI_ADSR_SLOPE, MI_ADSR_RELEASE };
    switch (setter)
    {
        case MI_ADSR_SET_ATTACK_TIME:   set_param(s, s->curve[MI_ADSR_ATTACK].time, fa); break;        // .h:161-165
        case MI_ADSR_SET_HOLD_TIME:     set_param(s, s->hold_time, fa); break;
        case MI_ADSR_SET_DECAY_TIME:    set_param(s, s->curve[MI_ADSR_DECAY].time, fa); break;
        case MI_ADSR_SET_SLOPE_TIME:    set_param(s, s->curve[MI_ADSR_SLOPE].time, fa); break;
        case MI_ADSR_SET_RELEASE_TIME:  set_param(s, s->curve[MI_ADSR_RELEASE].time, fa); break;
        case MI_ADSR_SET_ATTACK_CURVE: case MI_ADSR_SET_DECAY_CURVE: case MI_ADSR_SET_SLOPE_CURVE: case MI_ADSR_SET_RELEASE_CURVE:    // .h:167-170
            set_param(s, s->curve[PART_OF[setter - MI_ADSR_SET_ATTACK_CURVE]].curve, fa);
            break;
        case MI_ADSR_SET_ATTACK_FUNCTION: case MI_ADSR_SET_DECAY_FUNCTION: case MI_ADSR_SET_SLOPE_FUNCTION: case MI_ADSR_SET_RELEASE_FUNCTION:    // .h:172-175
            MI_REQUIRE(as_function(a, &fn), MI_EINVAL, "mi_adsr_settings_set: %g is no function", a);
            set_function(s, s->curve[PART_OF[setter - MI_ADSR_SET_ATTACK_FUNCTION]].function, fn);
            break;
        case MI_ADSR_SET_BREAK_LEVEL:   set_param(s, s->break_level, fa); break;                      // .h:177-178
        case MI_ADSR_SET_SUSTAIN_LEVEL: set_param(s, s->sustain_level, fa); break;
        case MI_ADSR_SET_HOLD_ENABLED:  set_flag(s, MI_ADSR_USE_HOLD, a != 0.0); break;               // .h:180-181
        case MI_ADSR_SET_BREAK_ENABLED: set_flag(s, MI_ADSR_USE_BREAK, a != 0.0); break;
        case MI_ADSR_SET_HOLD:                                                                      // :107-111
            set_param(s, s->hold_time, fa);
            set_flag(s, MI_ADSR_USE_HOLD, b != 0.0);
            break;
        case MI_ADSR_SET_BREAK:                                                                     // :113-117
            set_param(s, s->break_level, fa);
            set_flag(s, MI_ADSR_USE_BREAK, b != 0.0);
            break;
        default:                                                                                    // .h:183-188
            MI_REQUIRE(as_function(c, &fn), MI_EINVAL, "mi_adsr_settings_set: %g is no function", c);
            set_curve(s, (setter == MI_ADSR_SET_ATTACK) ? MI_ADSR_ATTACK : (setter == MI_ADSR_SET_DECAY) ? MI_ADSR_DECAY :
                         (setter == MI_ADSR_SET_SLOPE) ? MI_ADSR_SLOPE : MI_ADSR_RELEASE, fa, fb, fn);
            break;
    }
    return MI_OK;
}

int mi_adsr_settings_update(mi_adsr_settings_t *s)                                      // update_settings(), :238-293
{
    MI_REQUIRE(s != nullptr, MI_EINVAL, "mi_adsr_settings_update: NULL settings");
    if (!(s->flags & MI_ADSR_RECONFIGURE))
        return MI_OK;
    mi_adsr_curve_t *cv = s->curve;

    cv[MI_ADSR_ATTACK].time = limit_range(cv[MI_ADSR_ATTACK].time, 0.0f);
    if (s->flags & MI_ADSR_USE_HOLD)
    {
        s->hold_time = limit_range(s->hold_time, cv[MI_ADSR_ATTACK].time);
        cv[MI_ADSR_DECAY].time = limit_range(cv[MI_ADSR_DECAY].time, s->hold_time);
    }
    else
        cv[MI_ADSR_DECAY].time = limit_range(cv[MI_ADSR_DECAY].time, cv[MI_ADSR_ATTACK].time);
    if (s->flags & MI_ADSR_USE_BREAK)
    {
        cv[MI_ADSR_SLOPE].time = limit_range(cv[MI_ADSR_SLOPE].time, cv[MI_ADSR_DECAY].time);
        cv[MI_ADSR_RELEASE].time = limit_range(cv[MI_ADSR_RELEASE].time, cv[MI_ADSR_SLOPE].time);
    }
    else
        cv[MI_ADSR_RELEASE].time = limit_range(cv[MI_ADSR_RELEASE].time, cv[MI_ADSR_DECAY].time);

    configure_curve(&cv[MI_ADSR_ATTACK], 0.0f, cv[MI_ADSR_ATTACK].time, 0.0f, 1.0f);
    const float hold = (s->flags & MI_ADSR_USE_HOLD) ? s->hold_time : cv[MI_ADSR_ATTACK].time;
    const float decay = cv[MI_ADSR_DECAY].time;
    if (s->flags & MI_ADSR_USE_BREAK)
    {
        configure_curve(&cv[MI_ADSR_DECAY], hold, decay, 1.0f, s->break_level);
        configure_curve(&cv[MI_ADSR_SLOPE], decay, cv[MI_ADSR_SLOPE].time, s->break_level, s->sustain_level);
    }
    else
        configure_curve(&cv[MI_ADSR_DECAY], hold, decay, 1.0f, s->sustain_level);
    configure_curve(&cv[MI_ADSR_RELEASE], cv[MI_ADSR_RELEASE].time, 1.0f, s->sustain_level, 0.0f);

    s->flags &= ~uint32_t(MI_ADSR_RECONFIGURE);
    return MI_OK;
}

int mi_adsr_settings_process(const mi_adsr_settings_t *s, float t, float *value)       // do_process(), :295-326
{
    MI_REQUIRE(s != nullptr && value != nullptr, MI_EINVAL, "mi_adsr_settings_process: NULL argument");
    MI_REQUIRE(!(s->flags & MI_ADSR_RECONFIGURE), MI_ESTATE, "mi_adsr_settings_process: the settings need mi_adsr_settings_update() first");
    *value = mi_adsr::do_process(mi_adsr::record_of(*s, 1), t);
    return MI_OK;
}

int mi_interpolation_hermite_cubic(float *p, float x0, float y0, float k0, float x1, float y1, float k1)
{
    MI_REQUIRE(p != nullptr, MI_EINVAL, "mi_interpolation_hermite_cubic: NULL result");
    hermite_cubic(p, x0, y0, k0, x1, y1, k1);
    return MI_OK;
}

int mi_interpolation_hermite_quadro(float *p, float x0, float y0, float k0, float x1, float y1, float k1, float x2, float y2)
{
    MI_REQUIRE(p != nullptr, MI_EINVAL, "mi_interpolation_hermite_quadro: NULL result");
    hermite_quadro(p, x0, y0, k0, x1, y1, k1, x2, y2);
    return MI_OK;
}

} // extern "C"
