// sizeof and offsetof of lsp::dspu::QuantizedCounter, and what the host side of the class does with no device: compiled against
// this library's headers (and, where the reference tree exists, against the reference's: the same lines come out).
//   quantized_counter_layout              sizeof of the class, then the offsets of the fourteen members
//   quantized_counter_layout behaviour    a fresh object, the setters' limits and their bUpdate rule, the inline members,
//                                         update_settings() and clear() on an empty window, dump keys
//   quantized_counter_layout IN OUT       the recorded cases on the device: the protocol of
//                                         tests/golden/make_quantized_counter_vectors.py's driver, each process() as ONE call
#define private public
#define protected public
#include <lsp-plug.in/dsp-units/stat/QuantizedCounter.h>
#undef private
#undef protected
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

using namespace lsp;
using namespace lsp::dspu;
typedef QuantizedCounter C;

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

static int run_cases(const char *in, const char *out)
{
    FILE *f = fopen(in, "rb"), *o = fopen(out, "wb");
    if (!f || !o) return 2;
    uint32_t h[3];                              // rows, row length, cases
    if (fread(h, 4, 3, f) != 3) return 3;
    const size_t len = h[1];
    std::vector<float> x(size_t(h[0]) * len);
    if (fread(x.data(), 4, x.size(), f) != x.size()) return 3;
    for (uint32_t c = 0; c < h[2]; ++c)
    {
        uint32_t q[3];                          // max_period, max_levels, ops
        if (fread(q, 4, 3, f) != 3) return 3;
        std::vector<double> ops(6 * size_t(q[2]));
        if (fread(ops.data(), 8, ops.size(), f) != ops.size()) return 3;
        C g;
        if (g.init(q[0], q[1]) != STATUS_OK) return 4;
        for (size_t j = 0; j < q[2]; ++j)
        {
            const double *p = &ops[6 * j];
            const size_t n = size_t(p[3]);
            const float *s = &x[size_t(p[1]) * len + size_t(p[2])];
            const float a = float(p[4]), b = float(p[5]);
            switch (int(p[0]))
            {
                case 0: g.set_period(n); break;
                case 1: g.set_levels(n); break;
                case 2: g.set_min_value(a); break;
                case 3: g.set_max_value(a); break;
                case 4: g.set_value_range(a, b); break;
                case 5: g.set_range(a, b, n); break;
                case 6: g.update_settings(); break;
                case 7: g.clear(); break;
                case 8: g.process(s, n); break;
                default: return 6;
            }
            std::vector<uint32_t> w(q[1] + 10);
            memcpy(w.data(), g.counters(), 4 * size_t(q[1] + 2));
            uint32_t *t = &w[q[1] + 2];
            t[0] = g.nHead, t[1] = uint32_t(g.count()), t[2] = uint32_t(g.period()), t[3] = uint32_t(g.levels()), t[4] = fb(g.fMinValue);
            t[5] = fb(g.fMaxValue), t[6] = fb(g.fRStep), t[7] = g.needs_update() ? 1 : 0;
            if (w[q[1]] != g.below() || w[q[1] + 1] != g.above()) return 7;
            fwrite(w.data(), 4, w.size(), o);
        }
        fwrite(g.vHistory, 4, g.nCapacity, o);
    }
    fclose(f);
    return fclose(o) == 0 ? 0 : 8;
}

static void line(const char *name, const C &c)
{
    printf("%s %u %u %u %u %u %u %u %u %u %u %d", name, c.nPeriod, c.nLevels, c.nHead, c.nCapacity, c.nCount, c.nMaxPeriod, c.nMaxLevels,
           fb(c.fMinValue), fb(c.fMaxValue), fb(c.fRStep), int(c.bUpdate));
    printf(" %zu %zu %zu %zu %d\n", c.period(), c.max_period(), c.levels(), c.count(), int(c.needs_update()));
}

int main(int argc, char **argv)
{
    if (argc == 1)
    {
        printf("sizeof %zu\n", sizeof(C));
        printf("offsetof %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", offsetof(C, nPeriod), offsetof(C, nLevels), offsetof(C, nHead),
               offsetof(C, nCapacity), offsetof(C, nCount), offsetof(C, nMaxPeriod), offsetof(C, nMaxLevels), offsetof(C, fMinValue),
               offsetof(C, fMaxValue), offsetof(C, fRStep), offsetof(C, bUpdate), offsetof(C, vHistory), offsetof(C, vCounters), offsetof(C, pData));
        return 0;
    }
    if (argc == 3)
        return run_cases(argv[1], argv[2]);
    // ---- behaviour with no device
    C c;
    line("fresh", c);
    const int res = int(c.init(40, 16));
    printf("init %d %d %d\n", res, int(c.vHistory != NULL && c.vCounters != NULL && c.pData != NULL),
           int((reinterpret_cast<uintptr_t>(c.vHistory) & 63) == 0 && reinterpret_cast<uint8_t *>(c.vCounters) == reinterpret_cast<uint8_t *>(c.vHistory) + 4 * 1072));
    line("inited", c);
    c.set_period(1000);                         // limited to max_period
    c.set_levels(100);                          // ... to max_levels
    line("limited_high", c);
    c.set_period(0);
    c.set_levels(0);
    line("limited_low", c);
    c.update_settings();                        // nothing held: host work.  min == max: the step is Inf
    line("updated", c);
    printf("counters %u %u %u %u\n", c.counters()[0], c.counters()[15], c.below(), c.above());
    c.set_levels(1);                            // unchanged values: no bUpdate
    c.set_min_value(0.0f);
    c.set_max_value(0.0f);
    c.set_value_range(0.0f, 0.0f);
    c.set_range(0.0f, 0.0f, 1);
    line("unchanged", c);
    c.set_range(-1.0f, 1.0f, 8);
    line("set_range", c);
    c.update_settings();
    line("updated_range", c);
    c.set_min_value(-2.0f);
    line("set_min", c);
    c.update_settings();
    c.set_max_value(2.0f);
    line("set_max", c);
    c.update_settings();
    c.set_value_range(-2.0f, 2.0f);
    line("same_value_range", c);
    c.set_value_range(1.0f, -1.0f);             // reversed: a negative step
    c.update_settings();
    line("reversed", c);
    c.set_period(7);
    c.clear();                                  // bUpdate and the settings stay
    line("cleared", c);
    keys k;
    c.dump(&k);
    printf("dump%s\n", k.seen.c_str());
    c.destroy();
    printf("destroyed %d\n", int(c.vHistory == NULL && c.vCounters == NULL));
    return 0;
}
