// sizeof and offsetof of lsp::dspu::ADSREnvelope, and what the host side of the class does with no device: compiled against this
// library's headers (and, where the reference tree exists, against the reference's: the same lines come out).
//   adsr_layout            sizeof of the class, of curve_t and of gen_params_t, then the offsets of nine members
//   adsr_layout behaviour  a fresh object, the setters' flags, update_settings()'s clamped times and designed curves, the
//                          generator that every function gets, the scalar process(float) on a grid, dump keys by function
//   adsr_layout device     the five array methods of six objects (needs a device)
#define private public
#define protected public
#include <lsp-plug.in/dsp-units/util/ADSREnvelope.h>
#include <lsp-plug.in/dsp-units/misc/interpolation.h>
#undef private
#undef protected
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <string>

using namespace lsp;
using namespace lsp::dspu;
typedef ADSREnvelope E;

struct keys: public IStateDumper
{
    std::string seen;
    int depth = 0;
    void note(const char *n) { seen += " "; seen += std::to_string(depth); seen += ":"; seen += n; }
    void begin_object(const char *n, const void *, size_t) override { note(n); ++depth; }
    void begin_object(const void *, size_t) override    { note("{}"); ++depth; }
    void end_object() override                          { --depth; }
    void begin_array(const char *n, const void *, size_t) override { note(n); ++depth; }
    void begin_array(const void *, size_t) override     { ++depth; }
    void end_array() override                           { --depth; }
    void write(const char *n, const void *) override    { note(n); }
    void write(const char *n, bool) override            { note(n); }
    void write(const char *n, signed int) override      { note(n); }
    void write(const char *n, unsigned int) override    { note(n); }
    void write(const char *n, signed long) override     { note(n); }
    void write(const char *n, unsigned long) override   { note(n); }
    void write(const char *n, signed long long) override { note(n); }
    void write(const char *n, unsigned long long) override { note(n); }
    void write(const char *n, float) override           { note(n); }
    void writev(const char *n, const float *, size_t) override { note(n); }
};

static unsigned fb(float f) { unsigned u; memcpy(&u, &f, 4); return u; }

static void configure(E &e, int fn)
{
    e.set_attack(0.1f, 0.25f, E::function_t(fn));
    e.set_hold(0.2f, true);
    e.set_decay(0.4f, 0.25f, E::function_t(fn));
    e.set_break(0.5f, true);
    e.set_slope(0.6f, 0.25f, E::function_t(fn));
    e.set_release(0.8f, 0.25f, E::function_t(fn));
    e.set_sustain_level(0.3f);
    e.update_settings();
}

static int generator_of(const E::curve_t &c)
{
    return (c.pGenerator == E::none_generator) ? 0 : (c.pGenerator == E::line_generator) ? 1 : (c.pGenerator == E::cubic_generator) ? 3 :
           (c.pGenerator == E::quadro_generator) ? 4 : (c.pGenerator == E::exp_generator) ? 5 : -1;
}

static void fields(const char *name, const E &e, int used)
{
    printf("%s", name);
    for (int p = 0; p < 4; ++p)
    {
        const E::curve_t &c = e.vCurve[p];
        float six[6];
        memcpy(six, &c.sParams, sizeof(six));
        printf(" %u %u %d %d", fb(c.fTime), fb(c.fCurve), int(c.enFunction), generator_of(c));
        for (int q = 0; q < used; ++q)
            printf(" %u", fb(six[q]));
    }
    printf(" %u %u %u %u\n", fb(e.fHoldTime), fb(e.fBreakLevel), fb(e.fSustainLevel), unsigned(e.nFlags));
}

int main(int argc, char **argv)
{
    if (argc == 1)
    {
        printf("sizeof %zu %zu %zu\n", sizeof(E), sizeof(E::curve_t), sizeof(E::gen_params_t));
        printf("offsetof %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", offsetof(E, vCurve), offsetof(E, fHoldTime), offsetof(E, fBreakLevel),
               offsetof(E, fSustainLevel), offsetof(E, nFlags), offsetof(E::curve_t, fCurve), offsetof(E::curve_t, enFunction),
               offsetof(E::curve_t, pGenerator), offsetof(E::curve_t, sParams));
        return 0;
    }
    if (strcmp(argv[1], "device") == 0)
    {
        // ---- the five array methods, which run on the device: 1027 samples per function, inputs that the test forms again
        enum { N = 1027 };
        static float t[N], data[N], out[N];
        for (int i = 0; i < N; ++i)
            t[i] = -0.05f + float(i) * (1.1f / N), data[i] = float(i % 17 - 8) * 0.25f;
        for (int fn = 0; fn < 6; ++fn)
        {
            E e;
            configure(e, fn);
            for (int op = 0; op < 5; ++op)
            {
                for (int i = 0; i < N; ++i)
                    out[i] = (op == 1 || op == 3) ? data[i] : -77.0f;
                switch (op)
                {
                    case 0: e.process(out, t, N); break;
                    case 1: e.process_mul(out, t, N); break;
                    case 2: e.generate(out, -0.05f, 1.1f / N, N); break;
                    case 3: e.generate_mul(out, -0.05f, 1.1f / N, N); break;
                    default: e.generate_mul(out, data, -0.05f, 1.1f / N, N); break;
                }
                printf("rows%d_%d", fn, op);
                for (int i = 0; i < N; ++i)
                    printf(" %u", fb(out[i]));
                printf("\n");
            }
            e.set_sustain_level(0.9f);                      // a change reaches the device with the next call
            e.generate(out, 0.7f, 0.0f, 5);
            printf("changed%d %u %u\n", fn, fb(out[0]), fb(out[4]));
        }
        return 0;
    }
    // ---- behaviour with no device
    {
        E e;
        fields("fresh", e, 0);
        printf("fresh_getters %u %u %u %u %u %d %u %u\n", fb(e.attack_time()), fb(e.hold_time()), fb(e.release_time()), fb(e.attack_curve()),
               fb(e.sustain_level()), int(e.attack_function()), fb(e.hold_enabled()), fb(e.break_enabled()));
        e.update_settings();
        unsigned flags[8];
        flags[0] = e.nFlags;
        e.set_attack_time(0.0f);            // the same value: nothing is asked for
        e.set_attack_curve(0.5f);
        e.set_attack_function(E::ADSR_NONE);
        e.set_hold_enabled(false);
        e.set_hold(0.0f, false);
        e.set_release(0.0f, 0.5f, E::ADSR_NONE);
        flags[1] = e.nFlags;
        e.set_sustain_level(7.0f);          // clamped
        flags[2] = e.nFlags;
        e.update_settings();
        e.set_sustain_level(1.0f);
        flags[3] = e.nFlags;
        e.set_break_enabled(true);
        flags[4] = e.nFlags;
        e.update_settings();
        e.set_relese_time(-3.0f);
        flags[5] = e.nFlags;
        e.set_decay_function(E::ADSR_EXP);
        flags[6] = e.nFlags;
        printf("flags %u %u %u %u %u %u %u %u\n", flags[0], flags[1], flags[2], flags[3], flags[4], flags[5], flags[6], fb(e.sustain_level()));
    }
    {
        E e;                                // times out of order are pushed up
        e.set_attack_time(0.5f), e.set_hold(0.3f, true), e.set_decay_time(0.2f), e.set_break(0.5f, true), e.set_slope_time(0.7f), e.set_relese_time(0.6f);
        e.update_settings();
        printf("pushed %u %u %u %u %u\n", fb(e.attack_time()), fb(e.hold_time()), fb(e.decay_time()), fb(e.slope_time()), fb(e.release_time()));
    }
    static const int USED[6] = { 3, 5, 5, 5, 6, 6 };
    for (int fn = 0; fn < 6; ++fn)
    {
        E e;
        configure(e, fn);
        char name[24];
        snprintf(name, sizeof(name), "designed%d", fn);
        fields(name, e, USED[fn]);
        printf("process%d", fn);
        for (int i = -2; i <= 66; ++i)
            printf(" %u", fb(e.process(float(i) / 64.0f)));
        printf("\n");
        keys k;
        e.dump(&k);
        printf("dump%d%s\n", fn, k.seen.c_str());
    }
    float p[5];
    interpolation::hermite_cubic(p, 0.0f, 1.0f, -2.5f, 0.2f, 0.5f, -1.0f);
    printf("cubic %u %u %u %u\n", fb(p[0]), fb(p[1]), fb(p[2]), fb(p[3]));
    interpolation::hermite_quadro(p, 0.0f, 1.0f, 0.0f, 0.2f, 0.5f, 0.0f, 0.1f, 0.8f);
    printf("quadro %u %u %u %u %u\n", fb(p[0]), fb(p[1]), fb(p[2]), fb(p[3]), fb(p[4]));
    return 0;
}
