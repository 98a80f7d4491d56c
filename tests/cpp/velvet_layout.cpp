// sizeof and offsetof of lsp::dspu::Velvet, and what the host side of the class does with no device: compiled against this library's
// headers (and, where the reference tree exists, against the reference's: the same lines come out).
//   velvet_layout            sizeof, then the offsets of the members in declaration order, then crush_t's size and offsets
//   velvet_layout behaviour  a fresh object, the setters' clamps, init(), dump keys (needs the library, not a device)
#define private public
#define protected public
#include <lsp-plug.in/dsp-units/noise/Velvet.h>
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

static void settings(const char *name, const Velvet &v)
{
    printf("%s %d %d %d %u %u %u %u %u\n", name, int(v.enCore), int(v.enVelvetType), int(v.sCrushParams.bCrush), fb(v.sCrushParams.fCrushProb),
           fb(v.fWindowWidth), fb(v.fARNdelta), fb(v.fAmplitude), fb(v.fOffset));
}

int main(int argc, char **argv)
{
    if (argc == 1)
    {
        printf("sizeof %zu\n", sizeof(Velvet));
        printf("offsetof %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", offsetof(Velvet, sRandomizer), offsetof(Velvet, sMLS), offsetof(Velvet, enCore),
               offsetof(Velvet, enVelvetType), offsetof(Velvet, sCrushParams), offsetof(Velvet, fWindowWidth), offsetof(Velvet, fARNdelta),
               offsetof(Velvet, fAmplitude), offsetof(Velvet, fOffset), sizeof(Velvet::crush_t), offsetof(Velvet::crush_t, bCrush),
               offsetof(Velvet::crush_t, fCrushProb));
        return 0;
    }
    // ---- behaviour with no device
    Velvet v;
    settings("fresh", v);
    printf("freshstate %d %zu %llu %d\n", int(v.sRandomizer.nBufID == size_t(-1)), v.sMLS.nBits, (unsigned long long)v.sMLS.nState, int(v.sMLS.bSync));
    v.set_core_type(VN_CORE_LCG);
    v.set_velvet_type(VN_VELVET_ARN);
    v.set_crush(true);
    v.set_crush_probability(1.5f);
    v.set_velvet_window_width(1.0f);
    v.set_delta_value(-0.25f);
    v.set_amplitude(-2.0f);
    v.set_offset(-0.0f);
    settings("clamped", v);
    v.set_crush_probability(-3.0f);
    v.set_velvet_window_width(10.7f);
    v.set_delta_value(7.0f);
    settings("clamped2", v);
    v.set_crush_probability(0.25f);
    v.set_velvet_window_width(2.0f);
    v.set_delta_value(0.75f);
    settings("kept", v);
    // init(seed, bits, state): the Randomizer's words, the MLS told and not yet updated; the same state again: nothing happens
    v.init(0x12345678, 23, 0x55);
    printf("init");
    for (int i = 0; i < 4; ++i)
        printf(" %u %u %u %u", v.sRandomizer.vRandom[i].vLast, v.sRandomizer.vRandom[i].vMul1, v.sRandomizer.vRandom[i].vMul2, v.sRandomizer.vRandom[i].vAdd);
    printf(" %zu\n", v.sRandomizer.nBufID);
    printf("mls %zu %llu %d %u %u\n", v.sMLS.nBits, (unsigned long long)v.sMLS.nState, int(v.sMLS.bSync), fb(v.sMLS.fAmplitude), fb(v.sMLS.fOffset));
    v.sMLS.bSync = false;
    v.init(0x12345678, 23, 0x55);
    printf("same %d\n", int(v.sMLS.bSync));
    v.init(1, 24, 0x55);
    printf("other %d %zu\n", int(v.sMLS.bSync), v.sMLS.nBits);
    keys k;
    v.dump(&k);
    printf("Velvet%s\n", k.seen.c_str());
    return 0;
}
