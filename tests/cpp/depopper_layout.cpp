// sizeof and offsetof of lsp::dspu::Depopper, and what the host side of the class does with no device: compiled against this
// library's headers (and, where the reference tree exists, against the reference's: the same lines come out).
//   depopper_layout            sizeof of the class and of fade_t, then the offsets of ten members
//   depopper_layout behaviour  a fresh object, the setters' returns and quirks, init()'s extents, reconfigure()'s designed values in
//                              every mode, dump keys (needs the library, not a device)
#define private public
#define protected public
#include <lsp-plug.in/dsp-units/util/Depopper.h>
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
    void write(const char *n, signed long) override     { note(n); }
    void write(const char *n, unsigned long) override   { note(n); }
    void write(const char *n, signed long long) override { note(n); }
    void write(const char *n, unsigned long long) override { note(n); }
    void write(const char *n, float) override           { note(n); }
    void writev(const char *n, const float *, size_t) override { note(n); }
};

static unsigned fb(float f) { unsigned u; memcpy(&u, &f, 4); return u; }

static void fade(const char *name, const Depopper::fade_t &f)
{
    printf("%s %d %u %u %u %ld %ld %u %u %u %u\n", name, int(f.enMode), fb(f.fThresh), fb(f.fTime), fb(f.fDelay), long(f.nSamples), long(f.nDelay),
           fb(f.fPoly[0]), fb(f.fPoly[1]), fb(f.fPoly[2]), fb(f.fPoly[3]));
}

static void extents(const char *name, const Depopper &d)
{
    printf("%s %ld %d %u %ld %ld %ld %ld %u %u %ld %ld %ld %ld %u %ld %ld %u %d %d\n", name, long(d.nSampleRate), int(d.nState), fb(d.fLookMax),
           long(d.nLookMin), long(d.nLookMax), long(d.nLookOff), long(d.nLookCount), fb(d.fRmsMax), fb(d.fRmsLength), long(d.nRmsMin), long(d.nRmsMax),
           long(d.nRmsOff), long(d.nRmsLen), fb(d.fRmsNorm), long(d.nCounter), long(d.nDelay), fb(d.fRms), int(d.pData != NULL), int(d.bReconfigure));
}

int main(int argc, char **argv)
{
    if (argc == 1)
    {
        printf("sizeof %zu %zu\n", sizeof(Depopper), sizeof(Depopper::fade_t));
        printf("offsetof %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", offsetof(Depopper, nSampleRate), offsetof(Depopper, nState),
               offsetof(Depopper, fLookMax), offsetof(Depopper, fRmsMax), offsetof(Depopper, nCounter), offsetof(Depopper, fRms),
               offsetof(Depopper, sFadeIn), offsetof(Depopper, sFadeOut), offsetof(Depopper, pGainBuf), offsetof(Depopper, bReconfigure));
        return 0;
    }
    // ---- behaviour with no device
    Depopper d;
    extents("fresh", d);
    fade("fresh_in", d.sFadeIn);
    fade("fresh_out", d.sFadeOut);
    printf("init %d\n", int(d.init(48000, 10.0f, 2.0f)));
    extents("inited", d);
    printf("buffers %d %d\n", int(d.pGainBuf == reinterpret_cast<float *>(d.pData)), int(d.pRmsBuf == d.pGainBuf + d.nLookMax));
    // the setters: the old value comes back clamped, the new one is stored as given; an "unchanged" value asks for nothing
    d.bReconfigure = false;
    unsigned olds[7];
    olds[0] = fb(d.set_fade_in_time(-3.0f));
    olds[1] = fb(d.set_fade_in_time(0.0f));             // the old value, clamped, is 0: nothing is stored, -3 stays
    olds[2] = fb(d.set_fade_out_time(25.0f));
    olds[3] = fb(d.set_fade_out_time(10.0f));           // 25 clamped to max_fade is 10: 25 stays
    olds[4] = fb(d.set_fade_in_threshold(-1.0f));
    olds[5] = fb(d.set_fade_in_threshold(0.0f));
    olds[6] = fb(d.set_rms_length(7.0f));               // clamped to max_rms
    printf("olds %u %u %u %u %u %u %u\n", olds[0], olds[1], olds[2], olds[3], olds[4], olds[5], olds[6]);
    printf("kept %u %u %u %u %d\n", fb(d.get_fade_in_time()), fb(d.get_fade_out_time()), fb(d.get_fade_in_threshold()), fb(d.rms_length()),
           int(d.needs_reconfiguration()));
    d.set_fade_out_threshold(0.25f);
    d.bReconfigure = false;
    olds[0] = fb(d.set_fade_out_delay(0.25f));          // compared with fThresh: "unchanged"
    olds[1] = unsigned(d.bReconfigure);
    olds[2] = fb(d.set_fade_out_delay(1.0f));
    olds[3] = unsigned(d.bReconfigure);
    printf("delay %u %u %u %u %u\n", olds[0], olds[1], olds[2], olds[3], fb(d.get_fade_out_delay()));
    olds[0] = unsigned(d.set_fade_in_mode(DPM_SINE));
    olds[1] = unsigned(d.set_fade_in_mode(DPM_GAUSSIAN));
    olds[2] = unsigned(d.set_fade_out_mode(DPM_PARABOLIC));
    printf("modes %u %u %u\n", olds[0], olds[1], olds[2]);
    printf("same %d\n", int(d.init(48000, 10.0f, 2.0f)));
    // reconfigure() in every mode on both sides
    d.set_fade_in_time(6.25f);
    d.set_fade_out_time(5.0f);
    d.set_fade_in_delay(0.5f);
    d.set_fade_in_threshold(0.1f);
    d.set_rms_length(1.0f);
    for (int m = DPM_LINEAR; m <= DPM_PARABOLIC; ++m)
    {
        d.set_fade_in_mode(depopper_mode_t(m));
        d.set_fade_out_mode(depopper_mode_t(m));
        d.reconfigure();
        char name[16];
        snprintf(name, sizeof(name), "in%d", m);
        fade(name, d.sFadeIn);
        snprintf(name, sizeof(name), "out%d", m);
        fade(name, d.sFadeOut);
    }
    extents("designed", d);
    printf("latency %zu\n", d.latency());
    printf("again %d\n", int(d.init(44100, 5.0f, 1.0f)));
    extents("inited2", d);
    keys k;
    d.dump(&k);
    printf("Depopper%s\n", k.seen.c_str());
    d.destroy();
    extents("destroyed", d);
    return 0;
}
