// sizeof and offsetof of lsp::dspu::Randomizer, LCG and MLS, and what the host side of the three classes computes with no device:
// compiled against this library's headers (and, where the reference tree exists, against the reference's: the same lines come out).
//   noise_layout            one line per class: its size and the offsets of its members in declaration order
//   noise_layout behaviour  fresh objects, the setters and update_settings(), dump keys, and streams of process_single() / random()
//                           as float bits (needs the library, not a device)
#define private public
#define protected public
#include <lsp-plug.in/dsp-units/noise/LCG.h>
#include <lsp-plug.in/dsp-units/noise/MLS.h>
#undef private
#undef protected
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <string>

using namespace lsp;
using namespace lsp::dspu;

struct keys: public IStateDumper
{
    std::string seen;
    int depth = 0;
    void note(const char *n) { seen += " "; seen += std::to_string(depth); seen += ":"; seen += n; }
    void begin_object(const char *n, const void *, size_t) override { note(n); ++depth; }
    void begin_object(const void *, size_t) override    { ++depth; }
    void end_object() override                          { --depth; }
    void begin_array(const char *n, const void *, size_t) override { note(n); ++depth; }
    void begin_array(const void *, size_t) override     { ++depth; }
    void end_array() override                           { --depth; }
    void write(const char *n, const void *) override    { note(n); }
    void write(const char *n, bool) override            { note(n); }
    void write(const char *n, signed int) override      { note(n); }
    void write(const char *n, unsigned int) override    { note(n); }
    void write(const char *n, unsigned long) override   { note(n); }
    void write(const char *n, unsigned long long) override { note(n); }
    void write(const char *n, float) override           { note(n); }
};

static unsigned fb(float f) { unsigned u; memcpy(&u, &f, 4); return u; }

int main(int argc, char **argv)
{
    if (argc == 1)
    {
        printf("Randomizer %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(Randomizer), offsetof(Randomizer, vRandom), offsetof(Randomizer, nBufID),
               sizeof(Randomizer::randgen_t), offsetof(Randomizer::randgen_t, vLast), offsetof(Randomizer::randgen_t, vMul1),
               offsetof(Randomizer::randgen_t, vMul2), offsetof(Randomizer::randgen_t, vAdd));
        printf("LCG %zu %zu %zu %zu %zu\n", sizeof(LCG), offsetof(LCG, enDistribution), offsetof(LCG, fAmplitude), offsetof(LCG, fOffset), offsetof(LCG, sRand));
        printf("MLS %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(MLS), sizeof(MLS::mls_t), offsetof(MLS, nBits), offsetof(MLS, nFeedbackBit),
               offsetof(MLS, nFeedbackMask), offsetof(MLS, nActiveMask), offsetof(MLS, nTapsMask), offsetof(MLS, nOutputMask), offsetof(MLS, nState),
               offsetof(MLS, fAmplitude), offsetof(MLS, fOffset), offsetof(MLS, bSync));
        return 0;
    }
    // ---- behaviour with no device
    Randomizer r; LCG l; MLS m;
    printf("fresh %d %d %g %g %d %zu %llu %llu %g %g %d %d\n", int(r.nBufID == size_t(-1)), int(l.enDistribution), l.fAmplitude, l.fOffset,
           int(l.sRand.nBufID == size_t(-1)), m.nBits, (unsigned long long)m.nState, (unsigned long long)m.nOutputMask, m.fAmplitude, m.fOffset,
           int(m.needs_update()), int(m.maximum_number_of_bits()));
    printf("uninit %g %d\n", r.random(RND_GAUSSIAN), int(r.nBufID == size_t(-1)));
    r.init(0x12345678);
    printf("init");
    for (int i = 0; i < 4; ++i)
        printf(" %u %u %u %u", r.vRandom[i].vLast, r.vRandom[i].vMul1, r.vRandom[i].vMul2, r.vRandom[i].vAdd);
    printf(" %zu\n", r.nBufID);
    for (int f = 0; f < 4; ++f)                                 // RND_LINEAR, RND_EXP, RND_TRIANGLE, RND_GAUSSIAN: 64 values each, one stream
    {
        printf("random%d", f);
        for (int i = 0; i < 64; ++i)
            printf(" %u", fb(r.random(random_function_t(f))));
        printf("\n");
    }
    for (int d = 0; d < 4; ++d)                                 // LCG::process_single, 64 samples per distribution
    {
        LCG g;
        g.init(77 + d);
        g.set_distribution(lcg_dist_t(d));
        g.set_amplitude(0.75f);
        g.set_offset(0.125f);
        printf("single%d", d);
        for (int i = 0; i < 64; ++i)
            printf(" %u", fb(g.process_single()));
        printf("\n");
    }
    m.set_n_bits(200);
    m.set_state(0xDEADBEEFCAFEF00DULL);
    printf("period %llu %d\n", (unsigned long long)m.get_period(), int(m.needs_update()));
    m.set_n_bits(23);
    m.set_amplitude(0.5f);
    m.set_offset(0.25f);
    printf("mls");
    for (int i = 0; i < 100; ++i)
        printf(" %u", fb(m.process_single()));
    printf("\n");
    printf("words %zu %zu %llu %llu %llu %llu %llu %d %llu\n", m.nBits, m.nFeedbackBit, (unsigned long long)m.nFeedbackMask, (unsigned long long)m.nActiveMask,
           (unsigned long long)m.nTapsMask, (unsigned long long)m.nOutputMask, (unsigned long long)m.nState, int(m.bSync), (unsigned long long)m.get_period());
    m.set_state(m.nState);                                      // the current state: nothing happens
    printf("same %d\n", int(m.needs_update()));
    keys kr, kl, km;
    r.dump(&kr); l.dump(&kl); m.dump(&km);
    printf("Randomizer%s\nLCG%s\nMLS%s\n", kr.seen.c_str(), kl.seen.c_str(), km.seen.c_str());
    return 0;
}
