// sizeof and offsetof of lsp::dspu::MeterGraph, and what the host side of the class does with no device: compiled against this
// library's headers (and, where the reference tree exists, against the reference's: the same lines come out).
//   metergraph_layout              sizeof of the class and of RingBuffer, then the offsets of the six members
//   metergraph_layout behaviour    a fresh object, the inline members, the single-sample process(float) of every method inside one
//                                  long frame (no ring is needed before a frame closes), init() with a period of 0, dump keys
//   metergraph_layout IN OUT       the recorded cases on the device: the protocol of tests/golden/make_metergraph_vectors.py's driver
#define private public
#define protected public
#include <lsp-plug.in/dsp-units/util/MeterGraph.h>
#undef private
#undef protected
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

using namespace lsp;
using namespace lsp::dspu;
typedef MeterGraph G;

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

// the samples of the behaviour run: both signs, ties, zeros of both signs, a subnormal
static const float SAMPLES[20] = { 0.5f, -0.5f, 0.25f, -2.0f, 2.0f, 0.0f, -0.0f, 1e-40f, -3.0f, 3.0f,
                                   0.125f, -0.125f, 7.0f, -7.0f, 0.0625f, 1.0f, -1.0f, 9.0f, -0.03125f, 0.03125f };

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
        uint32_t q[3];                          // frames, period, ops
        float def;
        if (fread(q, 4, 3, f) != 3 || fread(&def, 4, 1, f) != 1) return 3;
        std::vector<double> ops(5 * size_t(q[2]));
        if (fread(ops.data(), 8, ops.size(), f) != ops.size()) return 3;
        G g;
        if (!g.init(q[0], q[1], def)) return 4;
        for (size_t j = 0; j < q[2]; ++j)
        {
            const double *p = &ops[5 * j];
            const size_t n = size_t(p[3]);
            const float *s = &x[size_t(p[1]) * len + size_t(p[2])];
            const float v = float(p[4]);
            std::vector<float> answer;
            switch (int(p[0]))
            {
                case 0: g.set_method(meter_method_t(int(p[3]))); break;
                case 1: g.set_period(n); break;
                case 2: g.set_default_value(v); break;
                case 3: g.fill(v); break;
                case 4: g.clear(); break;
                case 5: g.process(s, n); break;
                case 6: g.process(s, v, n); break;
                case 7: for (size_t i = 0; i < n; ++i) g.process(s[i]); break;
                case 8: answer.assign(n, -77.0f); g.read(answer.data(), n); break;
                case 9: answer.assign(1, g.level()); break;
                default: return 6;
            }
            std::vector<uint32_t> w(q[0] + 3);
            memcpy(w.data(), g.sBuffer.data(), 4 * size_t(q[0]));
            w[q[0]] = uint32_t(g.sBuffer.head_position()), w[q[0] + 1] = fb(g.fCurrent), w[q[0] + 2] = g.nCount;
            fwrite(w.data(), 4, w.size(), o);
            if (!answer.empty())
                fwrite(answer.data(), 4, answer.size(), o);
        }
    }
    fclose(f);
    return fclose(o) == 0 ? 0 : 8;
}

int main(int argc, char **argv)
{
    if (argc == 1)
    {
        printf("sizeof %zu %zu\n", sizeof(G), sizeof(RingBuffer));
        printf("offsetof %zu %zu %zu %zu %zu %zu\n", offsetof(G, sBuffer), offsetof(G, fCurrent), offsetof(G, fDefault), offsetof(G, nCount),
               offsetof(G, nPeriod), offsetof(G, enMethod));
        return 0;
    }
    if (argc == 3)
        return run_cases(argv[1], argv[2]);
    // ---- behaviour with no device
    {
        G g;                                    // construct() leaves fDefault as it finds it: not printed before it is set
        printf("fresh %u %u %u %d %zu %u %u\n", fb(g.fCurrent), g.nCount, g.nPeriod, int(g.enMethod), g.get_frames(), fb(g.period()), fb(g.level()));
        g.set_default_value(2.5f);
        g.set_period(77);
        g.set_method(MM_SIGN_MINIMUM);
        g.fill(1.0f);                           // no ring yet: nothing to fill
        g.clear();
        printf("inline %u %u %u %d %zu\n", fb(g.default_value()), fb(g.period()), g.nPeriod, int(g.enMethod), g.get_frames());
        g.set_period((size_t(1) << 32) + 5);    // uint32_t(period)
        printf("period_wraps %u %u\n", g.nPeriod, fb(g.period()));
        printf("init_period_0 %d %u\n", int(g.init(16, 0, 1.0f)), g.nPeriod);
        keys k;
        g.dump(&k);
        printf("dump%s\n", k.seen.c_str());
    }
    for (int m = 0; m < 6; ++m)                 // 5: no such method, runs as MM_ABS_MAXIMUM
    {
        G g;
        g.set_period(1000);
        g.set_method(meter_method_t(m));
        printf("single%d", m);
        for (int i = 0; i < 20; ++i)
        {
            g.process(SAMPLES[i]);
            printf(" %u %u", fb(g.fCurrent), g.nCount);
        }
        printf("\n");
    }
    return 0;
}
