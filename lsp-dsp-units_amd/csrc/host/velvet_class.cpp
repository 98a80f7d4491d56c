// lsp::dspu::Velvet (src/main/noise/Velvet.cpp).  The class keeps its state in its own members -- the reference's object has no
// room for a handle -- and runs rows on a bank of one channel that the calling thread's objects share: sRandomizer, sMLS and the
// settings go in (set_state and the setters), the rows are staged, the kernel runs, both states come back (get_state).
#include <lsp-plug.in/dsp-units/noise/Velvet.h>

#include <cmath>
#include <cstring>

#include "beside.h"

#pragma clang fp contract(off)

namespace lsp
{
namespace dspu
{
namespace
{
    constexpr size_t PIECE = size_t(1) << 22;                   // samples per launch with a source: a multiple of BUF_LIM_SIZE

    // what the rows of the calling thread's objects run on: made at the first call, kept for the life of the thread
    struct bench
    {
        mi_velvet_bank_t   *bank = nullptr;
        mi_host::rows       buf;                                // [2][cap]: dst, src

        ~bench() { mi_velvet_bank_destroy(bank); }
    };
    thread_local bench tl_bench;

    static_assert(sizeof(Velvet) == 176, "the reference's size on LP64");
}

Velvet::Velvet()    { construct(); }
Velvet::~Velvet()   { destroy(); }

void Velvet::construct()                                        // :48-63
{
    enCore = VN_CORE_MLS;
    enVelvetType = VN_VELVET_OVN;
    sCrushParams.bCrush = false;
    sCrushParams.fCrushProb = 0.5f;
    fWindowWidth = 10.0f;
    fARNdelta = 0.5f;
    fAmplitude = 1.0f;
    fOffset = 0.0f;
    sRandomizer.construct();
    sMLS.construct();
}

void Velvet::destroy()
{
    sRandomizer.destroy();
    sMLS.destroy();
}

void Velvet::set_core_type(vn_core_t core)              { enCore = core; }
void Velvet::set_velvet_type(vn_velvet_type_t type)     { enVelvetType = type; }
void Velvet::set_amplitude(float amplitude)             { fAmplitude = amplitude; }
void Velvet::set_offset(float offset)                   { fOffset = offset; }
void Velvet::set_crush(bool crush)                      { sCrushParams.bCrush = crush; }

void Velvet::set_velvet_window_width(float width)               // :81-84
{
    if (std::isfinite(width))
        fWindowWidth = (width > 2.0f) ? width : 2.0f;
}

void Velvet::set_delta_value(float delta)               { fARNdelta = (delta < 0.0f) ? 0.0f : (delta > 1.0f) ? 1.0f : delta; }
void Velvet::set_crush_probability(float prob)          { sCrushParams.fCrushProb = (prob < 0.0f) ? 0.0f : (prob > 1.0f) ? 1.0f : prob; }

void Velvet::init(uint32_t randseed, uint8_t mlsnbits, MLS::mls_t mlsseed)      // :111-121
{
    sRandomizer.init(randseed);
    sMLS.set_amplitude(1.0f);
    sMLS.set_offset(0.0f);
    sMLS.set_n_bits(mlsnbits);
    sMLS.set_state(mlsseed);
}

void Velvet::init()                                             // :123-130
{
    sRandomizer.init();
    sMLS.set_amplitude(1.0f);
    sMLS.set_offset(0.0f);
}

float Velvet::get_random_value()    { return sRandomizer.random(RND_LINEAR); }

float Velvet::get_spike()                                       // :137-148
{
    if (enCore == VN_CORE_MLS)
        return sMLS.process_single();
    return 2.0f * roundf(get_random_value()) - 1.0f;
}

float Velvet::get_crushed_spike()   { return (get_random_value() > sCrushParams.fCrushProb) ? 1.0f : -1.0f; }

void Velvet::run(float *dst, const float *src, size_t count, unsigned op)
{
    bench &b = tl_bench;
    if (count == 0 || sRandomizer.nBufID > 3 || (src == nullptr && count > MI_VN_MAX_COUNT))
        return;
    if (b.bank == nullptr && mi_velvet_bank_create(&b.bank, 1) != MI_OK)
        return;
    mi_velvet_state_t s = mi_velvet_state_t();
    for (size_t i = 0; i < 4; ++i)
    {
        const Randomizer::randgen_t &g = sRandomizer.vRandom[i];
        s.rand.last[i] = g.vLast, s.rand.mul1[i] = g.vMul1, s.rand.mul2[i] = g.vMul2, s.rand.add[i] = g.vAdd;
    }
    s.rand.buf_id = uint32_t(sRandomizer.nBufID);
    mi_mls_settings_t &m = s.mls;
    m.n_bits = sMLS.nBits, m.feedback_bit = sMLS.nFeedbackBit, m.feedback_mask = sMLS.nFeedbackMask, m.active_mask = sMLS.nActiveMask;
    m.taps_mask = sMLS.nTapsMask, m.output_mask = sMLS.nOutputMask, m.state = sMLS.nState, m.sync = sMLS.bSync;
    m.amplitude = 1.0f, m.offset = 0.0f;
    if (mi_velvet_bank_set_state(b.bank, 0, &s, nullptr) != MI_OK)
        return;
    mi_velvet_bank_set_core_type(b.bank, 0, uint32_t(enCore));
    mi_velvet_bank_set_velvet_type(b.bank, 0, uint32_t(enVelvetType));
    mi_velvet_bank_set_velvet_window_width(b.bank, 0, fWindowWidth);
    mi_velvet_bank_set_delta_value(b.bank, 0, fARNdelta);
    mi_velvet_bank_set_crush(b.bank, 0, sCrushParams.bCrush);
    mi_velvet_bank_set_crush_probability(b.bank, 0, sCrushParams.fCrushProb);
    mi_velvet_bank_set_amplitude(b.bank, 0, fAmplitude);
    mi_velvet_bank_set_offset(b.bank, 0, fOffset);
    // without a source the call is one segment and one launch; with one it is cut where the segments are cut anyway
    const size_t piece = (src == nullptr) ? count : PIECE;
    for (size_t at = 0; at < count; at += piece)
    {
        const size_t n = (count - at < piece) ? count - at : piece;
        if (!b.buf.reserve(n, 2))
            break;
        float *d_dst = b.buf.row(0), *d_src = (src != nullptr) ? b.buf.row(1) : nullptr;
        if (src != nullptr && !b.buf.up(1, src + at, n))
            break;
        if (mi_velvet_bank_process(b.bank, d_dst, d_src, n, n, n, op, nullptr) != MI_OK)
            break;
        if (!b.buf.down(dst + at, 0, n) || mi_dspu_stream_synchronize(nullptr) != MI_OK)
            break;
    }
    if (mi_velvet_bank_get_state(b.bank, 0, &s, nullptr) != MI_OK)     // where the device got to, also behind a piece that failed
        return;
    for (size_t i = 0; i < 4; ++i)
        sRandomizer.vRandom[i].vLast = s.rand.last[i];
    sRandomizer.nBufID = s.rand.buf_id;
    sMLS.nBits = m.n_bits, sMLS.nFeedbackBit = m.feedback_bit, sMLS.nFeedbackMask = m.feedback_mask, sMLS.nActiveMask = m.active_mask;
    sMLS.nTapsMask = m.taps_mask, sMLS.nState = m.state, sMLS.bSync = m.sync != 0;
}

void Velvet::process_add(float *dst, const float *src, size_t count)    { run(dst, src, count, MI_OSC_ADD); }
void Velvet::process_mul(float *dst, const float *src, size_t count)    { run(dst, src, count, MI_OSC_MUL); }
void Velvet::process_overwrite(float *dst, size_t count)                { run(dst, nullptr, count, MI_OSC_OVERWRITE); }

void Velvet::dump(IStateDumper *v) const                        // :321-340
{
    v->write_object("sRandomizer", &sRandomizer);
    v->write_object("sMLS", &sMLS);
    v->write("enCore", enCore);
    v->write("enVelvetType", enVelvetType);
    v->begin_object("sCrushParams", &sCrushParams, sizeof(sCrushParams));
    {
        v->write("bCrush", sCrushParams.bCrush);
        v->write("fCrushProb", sCrushParams.fCrushProb);
    }
    v->end_object();
    v->write("fWindowWidth", fWindowWidth);
    v->write("fARNdelta", fARNdelta);
    v->write("fAmplitude", fAmplitude);
    v->write("fOffset", fOffset);
}

} // namespace dspu
} // namespace lsp
