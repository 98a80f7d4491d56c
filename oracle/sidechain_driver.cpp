// One program, two libraries: runs lsp::dspu::Sidechain over a file of cases through the public class API (plus a subclass that
// reads the protected fields) and writes what the class computed and the state it was left in after every call.  oracle/Makefile
// compiles it with the reference's own Sidechain.cpp and RawRingBuffer.cpp into oracle/_ref/sidechain_ref (and, with a sanitizer,
// sidechain_ref_san); the GPU tests compile the same text against lsp-dsp-units_amd/include and libmi_dspu.so, without
// -DSIDECHAIN_DRIVER_REFERENCE.  The two result files are compared.
//
//   sidechain_driver <cases> <results>
//
// cases (native-endian 32-bit words, floats as their bits):
//   u32 magic 0x53434844, u32 count, then per case
//   u32 inputs (1 | 2), f32 max_reactivity, u32 sample_rate, f32 reactivity, u32 mode, u32 source, u32 stereo_mode, f32 gain,
//   u32 single                    1: a second object takes every sample through process(const float *) as well
//   u32 ncalls, per call u32 len, u32 null (1: process(out, NULL, len))
//   u32 nev, per event u32 before, u32 kind, f32 a         applied in file order ahead of call number `before`
//                                 0 set_reactivity(a)  1 set_mode(a)  2 set_source(a)  3 set_gain(a)  4 set_stereo_mode(a)  5 clear()
//                                 6 set_sample_rate(a)
//   u32 n, f32 in0[n], and with two inputs f32 in1[n]
// results, per case:
//   u32 ncalls, per call 9 words  nReactivity, fTau, nRefresh, fRmsValue, nFlags, the ring's capacity, its head, CRC-32 of the
//                                 bits of the last nReactivity ring values (oldest first), and the places this call went through:
//                                 1 refresh of RMS, window in one piece   2 ... wrapped   4 refresh of UNIFORM, one piece
//                                 8 ... wrapped   16 a window split at the ring's end inside one block (split < to_do)
//                                 32 refresh of PEAK or LPF   64 a refresh that the counter reached (not at the call's start)
//                                 128 a refresh at the call's start   256 the head left at the capacity
//                                 (with the product's class the ring lives on the device: CRC and places are written as 0)
//   u32 n, f32 out[n]
//   u32 n or 0, f32 pre_array[n], pre_scalar[n]       reference only: both preprocess() overloads on every sample
//   u32 n or 0, f32 single[n]                         cases with `single`
//   u32 nReactivity, f32 ring[nReactivity]            reference only (else 0): the last ring values after the last call
#include <lsp-plug.in/dsp-units/util/Sidechain.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace lsp;

typedef std::vector<float> fvec;
typedef std::vector<uint32_t> uvec;

struct event_t { uint32_t before, kind; float a; };

struct case_t
{
    uint32_t                inputs, sample_rate, mode, source, stereo, single;
    float                   max_reactivity, reactivity, gain;
    uvec                    len, null;
    std::vector<event_t>    events;
    fvec                    in[2];
};

static FILE *fin, *fout;

static void rd(void *p, size_t bytes)       { if (bytes && fread(p, 1, bytes, fin) != bytes) { fprintf(stderr, "short case file\n"); exit(2); } }
static uint32_t rd32()                      { uint32_t v; rd(&v, 4); return v; }
static float rdf()                          { float v; rd(&v, 4); return v; }
static void wr(const void *p, size_t bytes) { if (bytes && fwrite(p, 1, bytes, fout) != bytes) { fprintf(stderr, "write failed\n"); exit(3); } }
static void wr32(uint32_t v)                { wr(&v, 4); }
static void wrf(float v)                    { wr(&v, 4); }
static void wrv(const fvec &v)              { wr(v.data(), 4 * v.size()); }

// CRC-32 as zlib computes it, over the bytes of the floats
static uint32_t crc32(const fvec &v)
{
    const unsigned char *p = reinterpret_cast<const unsigned char *>(v.data());
    uint32_t c = 0xffffffffu;
    for (size_t i = 0; i < 4 * v.size(); ++i)
    {
        c ^= p[i];
        for (int k = 0; k < 8; ++k)
            c = (c >> 1) ^ (0xedb88320u & (0u - (c & 1u)));
    }
    return ~c;
}

enum
{
    P_RMS_WHOLE = 1, P_RMS_WRAPPED = 2, P_UNI_WHOLE = 4, P_UNI_WRAPPED = 8, P_SPLIT = 16, P_OTHER_REFRESH = 32, P_COUNTED = 64,
    P_AT_START = 128, P_HEAD_AT_END = 256
};

struct XSidechain: public dspu::Sidechain
{
    void state(uint32_t places)
    {
        wr32(uint32_t(nReactivity)); wrf(fTau); wr32(nRefresh); wrf(fRmsValue); wr32(nFlags);
        wr32(uint32_t(sBuffer.size())); wr32(uint32_t(sBuffer.position()));
#ifdef SIDECHAIN_DRIVER_REFERENCE
        wr32(crc32(ring()));
#else
        wr32(0);
#endif
        wr32(places);
    }

#ifdef SIDECHAIN_DRIVER_REFERENCE
    fvec ring() const
    {
        fvec v(nReactivity);
        const size_t cap = sBuffer.size(), head = sBuffer.position();
        for (size_t i = 0; i < v.size(); ++i)
            v[i] = sBuffer.begin()[(head + 2 * cap - v.size() + i) % cap];
        return v;
    }

    // the places process(out, in, samples) is about to go through: its own loop (Sidechain.cpp:452-553) on copies of the counters
    uint32_t walk(size_t samples)
    {
        update_settings();
        uint32_t places = 0;
        const size_t cap = sBuffer.size(), n = nReactivity;
        size_t head = sBuffer.position(), refresh = nRefresh;
        for (size_t offset = 0; offset < samples; )
        {
            if (refresh >= 0x2000)
            {
                const size_t tail = (head + cap - n) % cap;
                const bool whole = tail < head;
                places |= (nMode == dspu::SCM_RMS) ? (whole ? P_RMS_WHOLE : P_RMS_WRAPPED) :
                          (nMode == dspu::SCM_UNIFORM) ? (whole ? P_UNI_WHOLE : P_UNI_WRAPPED) : P_OTHER_REFRESH;
                places |= (offset > 0) ? P_COUNTED : P_AT_START;
                refresh %= 0x2000;
            }
            size_t to_do = samples - offset;
            if (to_do > 0x2000 - refresh)
                to_do = 0x2000 - refresh;
            if (to_do > 0x200)
                to_do = 0x200;
            head = (head + to_do > cap) ? head + to_do - cap : head + to_do;       // RawRingBuffer::push
            if ((nMode == dspu::SCM_RMS) || (nMode == dspu::SCM_UNIFORM))
            {
                const size_t tail = (head + cap - (n + to_do)) % cap;
                if (cap - tail < to_do)
                    places |= P_SPLIT;
            }
            offset += to_do;
            refresh += to_do;
        }
        if (head == cap)
            places |= P_HEAD_AT_END;
        return places;
    }

    void pre(float *array, float *scalar, const float *a, const float *b, size_t count)
    {
        const float *in[2] = { a, b };
        preprocess(array, in, count);
        for (size_t i = 0; i < count; ++i)
        {
            const float v[2] = { a[i], (b != NULL) ? b[i] : 0.0f };
            preprocess(&scalar[i], v);
        }
    }
#endif
};

static void apply(XSidechain &c, const event_t &e)
{
    switch (e.kind)
    {
        case 0:  c.set_reactivity(e.a); break;
        case 1:  c.set_mode(size_t(e.a)); break;
        case 2:  c.set_source(size_t(e.a)); break;
        case 3:  c.set_gain(e.a); break;
        case 4:  c.set_stereo_mode(dspu::sidechain_stereo_mode_t(int(e.a))); break;
        case 5:  c.clear(); break;
        case 6:  c.set_sample_rate(size_t(e.a)); break;
        default: fprintf(stderr, "no event of kind %u\n", e.kind); exit(2);
    }
}

static void configure(XSidechain &c, const case_t &k)
{
    if (!c.init(k.inputs, k.max_reactivity))
    {
        fprintf(stderr, "Sidechain::init(%u, %g) failed\n", k.inputs, k.max_reactivity);
        exit(4);
    }
    c.set_sample_rate(k.sample_rate);
    c.set_reactivity(k.reactivity);
    c.set_mode(k.mode);
    c.set_source(k.source);
    c.set_stereo_mode(dspu::sidechain_stereo_mode_t(k.stereo));
    c.set_gain(k.gain);
}

static void run(const case_t &k)
{
    XSidechain c, c2;
    configure(c, k);
    if (k.single)
        configure(c2, k);

    const size_t n = k.in[0].size();
    const bool two = k.inputs == 2;
    fvec out(n, 0.0f), single(n, 0.0f);
#ifdef SIDECHAIN_DRIVER_REFERENCE
    fvec pre_array(n, 0.0f), pre_scalar(n, 0.0f);
#endif
    size_t pos = 0;
    wr32(uint32_t(k.len.size()));
    for (size_t i = 0; i < k.len.size(); ++i)
    {
        const size_t len = k.len[i];
        for (size_t j = 0; j < k.events.size(); ++j)
            if (k.events[j].before == i)
            {
                apply(c, k.events[j]);
                if (k.single)
                    apply(c2, k.events[j]);
            }
        const float *in[2] = { k.in[0].data() + pos, two ? k.in[1].data() + pos : NULL };
        uint32_t places = 0;
#ifdef SIDECHAIN_DRIVER_REFERENCE
        places = c.walk(len);
        if (!k.null[i])
            c.pre(&pre_array[pos], &pre_scalar[pos], in[0], in[1], len);
#endif
        c.process(&out[pos], k.null[i] ? NULL : in, len);
        if (k.single)
            for (size_t t = 0; t < len; ++t)
            {
                const float v[2] = { in[0][t], two ? in[1][t] : 0.0f };
                single[pos + t] = c2.process(v);
            }
        pos += len;
        c.state(places);
    }
    wr32(uint32_t(n)); wrv(out);
#ifdef SIDECHAIN_DRIVER_REFERENCE
    wr32(uint32_t(n)); wrv(pre_array); wrv(pre_scalar);
#else
    wr32(0);
#endif
    if (k.single)
    {
        wr32(uint32_t(n)); wrv(single);
    }
    else
        wr32(0);
#ifdef SIDECHAIN_DRIVER_REFERENCE
    fvec ring = c.ring();
    wr32(uint32_t(ring.size())); wrv(ring);
#else
    wr32(0);
#endif
    c.destroy();
    c2.destroy();
}

int main(int argc, char **argv)
{
    if (argc != 3)
    {
        fprintf(stderr, "usage: %s <cases> <results>\n", argv[0]);
        return 1;
    }
    fin = fopen(argv[1], "rb");
    fout = fopen(argv[2], "wb");
    if ((fin == NULL) || (fout == NULL))
    {
        fprintf(stderr, "cannot open %s or %s\n", argv[1], argv[2]);
        return 1;
    }
    if (rd32() != 0x53434844u)
    {
        fprintf(stderr, "%s is not a case file\n", argv[1]);
        return 2;
    }
    uint32_t count = rd32();
    for (uint32_t ci = 0; ci < count; ++ci)
    {
        case_t k;
        k.inputs = rd32(); k.max_reactivity = rdf(); k.sample_rate = rd32(); k.reactivity = rdf();
        k.mode = rd32(); k.source = rd32(); k.stereo = rd32(); k.gain = rdf(); k.single = rd32();
        if ((k.inputs != 1) && (k.inputs != 2))
        {
            fprintf(stderr, "case %u: %u inputs\n", ci, k.inputs);
            return 2;
        }
        size_t ncalls = rd32(), total = 0;
        for (size_t i = 0; i < ncalls; ++i)
        {
            k.len.push_back(rd32());
            k.null.push_back(rd32());
            total += k.len.back();
            if (k.single && ((k.len.back() != 1) || k.null.back()))
            {
                fprintf(stderr, "case %u: a single-sample case has calls of one sample with an input\n", ci);
                return 2;
            }
        }
        k.events.resize(rd32());
        for (size_t i = 0; i < k.events.size(); ++i)
        {
            k.events[i].before = rd32(); k.events[i].kind = rd32(); k.events[i].a = rdf();
            if (k.events[i].before >= ncalls)
            {
                fprintf(stderr, "case %u: an event ahead of call %u of %u\n", ci, k.events[i].before, unsigned(ncalls));
                return 2;
            }
        }
        size_t n = rd32();
        if (total != n)
        {
            fprintf(stderr, "case %u: calls of %u samples for an input of %u\n", ci, unsigned(total), unsigned(n));
            return 2;
        }
        for (size_t j = 0; j < k.inputs; ++j)
        {
            k.in[j].resize(n);
            rd(k.in[j].data(), 4 * n);
        }
        run(k);
    }
    fclose(fin);
    if (fclose(fout) != 0)
        return 3;
    return 0;
}
