// sizeof and offsetof of lsp::dspu::ScaledMeterGraph, and what the host side of the class does with no device: compiled against
// this library's headers.
//   scaled_metergraph_layout              sizeof of the class, of RawRingBuffer and of sampler_t, then the members' offsets
//   scaled_metergraph_layout behaviour    a fresh object, the inline members, the refused init() arguments, the single-sample
//                                         process(float) of every method with two period changes, dump keys
//   scaled_metergraph_layout IN OUT       the recorded cases on the device: the protocol of
//                                         tests/golden/make_scaled_metergraph_vectors.py's driver
#define private public
#define protected public
#include <lsp-plug.in/dsp-units/util/ScaledMeterGraph.h>
#undef private
#undef protected
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

using namespace lsp;
using namespace lsp::dspu;
typedef ScaledMeterGraph G;
typedef G::sampler_t S;

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

// the samples of the behaviour run: both signs, ties, zeros of both signs, a subnormal, -1.0f
static const float SAMPLES[24] = { 0.5f, -0.5f, 0.25f, -2.0f, 2.0f, 0.0f, -0.0f, 1e-40f, -3.0f, 3.0f, 0.125f, -0.125f,
                                   7.0f, -7.0f, 0.0625f, 1.0f, -1.0f, 9.0f, -0.03125f, 0.03125f, -1.0f, -0.0f, 4.0f, -4.0f };

// both rings in storage order, then both heads, sHistory's fCurrent, nCount, nPeriod, sFrames' three and the target nPeriod
static std::vector<uint32_t> words(const G &g)
{
    const size_t ch = g.sHistory.sBuffer.size(), cf = g.sFrames.sBuffer.size();
    std::vector<uint32_t> w(ch + cf + 9);
    memcpy(w.data(), g.sHistory.sBuffer.begin(), 4 * ch);
    memcpy(w.data() + ch, g.sFrames.sBuffer.begin(), 4 * cf);
    uint32_t *t = w.data() + ch + cf;
    t[0] = uint32_t(g.sHistory.sBuffer.position() % ch), t[1] = uint32_t(g.sFrames.sBuffer.position() % cf);
    t[2] = fb(g.sHistory.fCurrent), t[3] = g.sHistory.nCount, t[4] = g.sHistory.nPeriod;
    t[5] = fb(g.sFrames.fCurrent), t[6] = g.sFrames.nCount, t[7] = g.sFrames.nPeriod, t[8] = g.nPeriod;
    return w;
}

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
        uint32_t q[4];                          // frames, subsampling, max_period, ops
        if (fread(q, 4, 4, f) != 4) return 3;
        std::vector<double> ops(5 * size_t(q[3]));
        if (fread(ops.data(), 8, ops.size(), f) != ops.size()) return 3;
        G g;
        if (!g.init(q[0], q[1], q[2])) return 4;
        for (size_t j = 0; j < q[3]; ++j)
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
                case 2: g.fill(v); break;
                case 3: g.process(s, n); break;
                case 4: g.process(s, v, n); break;
                case 5: for (size_t i = 0; i < n; ++i) g.process(s[i]); break;
                case 6: answer.assign(n + 1, -77.0f); g.read(answer.data(), n); answer.resize(n); break;
                case 7: answer.assign(1, g.level()); break;
                default: return 6;
            }
            const std::vector<uint32_t> w = words(g);
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
        printf("sizeof %zu %zu %zu\n", sizeof(G), sizeof(RawRingBuffer), sizeof(S));
        printf("offsetof %zu %zu %zu %zu %zu\n", offsetof(G, sHistory), offsetof(G, sFrames), offsetof(G, nPeriod), offsetof(G, nMaxPeriod),
               offsetof(G, enMethod));
        printf("sampler %zu %zu %zu %zu %zu\n", offsetof(S, sBuffer), offsetof(S, fCurrent), offsetof(S, nCount), offsetof(S, nPeriod),
               offsetof(S, nFrames));
        return 0;
    }
    if (argc == 3)
        return run_cases(argv[1], argv[2]);
    // ---- behaviour with no device
    {
        G g;
        printf("fresh %u %u %u %u %u %u %u %u %u %u %d %zu %zu %zu %zu %u %u\n", fb(g.sHistory.fCurrent), g.sHistory.nCount, g.sHistory.nPeriod,
               g.sHistory.nFrames, fb(g.sFrames.fCurrent), g.sFrames.nCount, g.sFrames.nPeriod, g.sFrames.nFrames, g.nPeriod, g.nMaxPeriod,
               int(g.enMethod), g.sHistory.sBuffer.size(), g.sFrames.sBuffer.size(), g.subsampling(), g.frames(), fb(g.period()), fb(g.level()));
        // where the reference is undefined: refused, and nothing is touched
        const bool r0 = g.init(16, 0, 64), r1 = g.init(0, 4, 64), r2 = g.init(16, 8, 7), r3 = g.init(size_t(1) << 16, 4, size_t(1) << 15);
        printf("refused %d %d %d %d %zu %u\n", int(r0), int(r1), int(r2), int(r3), g.sHistory.sBuffer.size(), g.nMaxPeriod);
        g.process(SAMPLES, 8);                  // no rings, no period: nothing is done
        g.process(SAMPLES, 2.0f, 8);
        g.process(1.0f);
        printf("idle %u %u %u\n", fb(g.sHistory.fCurrent), g.sHistory.nCount, g.sFrames.nCount);
        const bool made = g.init(16, 4, 64);
        printf("init %d %zu %zu %u %u %u %u %u\n", int(made), g.sHistory.sBuffer.size(), g.sFrames.sBuffer.size(), g.sHistory.nFrames,
               g.sHistory.nPeriod, g.sFrames.nFrames, g.nMaxPeriod, g.nPeriod);
        g.process(SAMPLES, 8);                  // before any set_period(): the reference would not return; nothing is done
        printf("no_period %u %zu\n", g.sHistory.nCount, g.sHistory.sBuffer.position());
        g.set_method(MM_SIGN_MINIMUM);
        g.set_period(2);                        // limited to subsampling .. max_period
        printf("inline %zu %zu %d %u", g.subsampling(), g.frames(), int(g.method()), fb(g.period()));
        g.set_period(1000);
        printf(" %u", fb(g.period()));
        g.set_period((size_t(1) << 32) + 9);    // uint32_t(period)
        printf(" %u\n", fb(g.period()));
        keys k;
        g.dump(&k);
        printf("dump%s\n", k.seen.c_str());
    }
    for (int m = 0; m < 6; ++m)                 // 5: no such method, runs as MM_ABS_MAXIMUM
    {
        G g;
        g.init(3, 2, 8);
        g.set_method(meter_method_t(m));
        g.set_period(4);
        printf("single%d", m);
        for (int i = 0; i < 24; ++i)
        {
            if (i == 9) g.set_period(3);
            if (i == 17) g.set_period(8);
            if (i == 20) g.fill(-0.5f);
            g.process(SAMPLES[i]);
            const std::vector<uint32_t> w = words(g);
            for (size_t j = 0; j < w.size(); ++j)
                printf(" %u", w[j]);
        }
        printf("\n");
    }
    return 0;
}
