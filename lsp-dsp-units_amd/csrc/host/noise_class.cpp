// lsp::dspu::Randomizer, LCG and MLS (src/main/util/Randomizer.cpp, src/main/noise/LCG.cpp, MLS.cpp).  Randomizer is plain host
// C++.  LCG and MLS keep their state in their own members -- the reference's objects have no room for a handle --, run
// process_single() on the host, and run rows on a bank of one channel that the calling thread's objects share: the members go
// in (set_state and the setters), the rows are staged, the kernel runs, the state comes back (get_state).
#include <lsp-plug.in/dsp-units/noise/LCG.h>
#include <lsp-plug.in/dsp-units/noise/MLS.h>

#include <chrono>
#include <cmath>
#include <cstring>

#include "beside.h"
#include "mls_device.h"

#pragma clang fp contract(off)

#define RAND_RANGE          2.32830643654e-10                   // Randomizer.cpp:26, the literal
#define RAND_LAMBDA         M_E * M_SQRT2
#define RAND_T              0.5f

namespace lsp
{
namespace dspu
{
namespace
{
    constexpr size_t PIECE = size_t(1) << 22;                   // samples per launch: below the banks' limit

    // what the rows of the calling thread's objects run on: made at the first call, kept for the life of the thread
    struct bench
    {
        mi_lcg_bank_t  *lcg = nullptr;
        mi_mls_bank_t  *mls = nullptr;
        mi_host::rows   buf;                                    // [2][cap]: dst, src

        ~bench()
        {
            mi_lcg_bank_destroy(lcg);
            mi_mls_bank_destroy(mls);
        }

        // one piece: src up, launch() between, dst down
        template <class Launch> bool piece(float *dst, const float *src, size_t n, Launch launch)
        {
            if (!buf.reserve(n, 2))
                return false;
            float *d_dst = buf.row(0), *d_src = (src != nullptr) ? buf.row(1) : nullptr;
            if (src != nullptr && !buf.up(1, src, n))
                return false;
            if (launch(d_dst, d_src) != MI_OK)
                return false;
            return buf.down(dst, 0, n) && mi_dspu_stream_synchronize(nullptr) == MI_OK;
        }
    };
    thread_local bench tl_bench;

    static_assert(sizeof(Randomizer) == 72 && sizeof(LCG) == 88 && sizeof(MLS) == 72, "the reference's sizes on LP64");
}

// ---- Randomizer -------------------------------------------------------------------------------------------------------------------
// (vMul1, vMul2 and vAdders are declared as in the reference and not defined: the tables live with mi_lcg_seed_words)
Randomizer::Randomizer()    { construct(); }
Randomizer::~Randomizer()   { destroy(); }

void Randomizer::construct()                                    // :69-80
{
    for (size_t i = 0; i < 4; ++i)
        vRandom[i].vAdd = 0, vRandom[i].vMul1 = 0, vRandom[i].vMul2 = 0, vRandom[i].vLast = 0;
    nBufID = -1;
}

void Randomizer::destroy()  {}

void Randomizer::init(uint32_t seed)                            // :86-99
{
    mi_lcg_state_t s;
    mi_lcg_seed_words(seed, &s);
    for (size_t i = 0; i < 4; ++i)
        vRandom[i].vAdd = s.add[i], vRandom[i].vMul1 = s.mul1[i], vRandom[i].vMul2 = s.mul2[i], vRandom[i].vLast = s.last[i];
    nBufID = 0;
}

void Randomizer::init()                                         // :101-106
{
    const auto now = std::chrono::system_clock::now().time_since_epoch();
    const uint64_t ns = uint64_t(std::chrono::duration_cast<std::chrono::nanoseconds>(now).count());
    init(uint32_t((ns / 1000000000ull) ^ (ns % 1000000000ull)));
}

float Randomizer::generate_linear()                             // :108-115
{
    if (nBufID > 3)                                             // never init()ed
        return 0.0f;
    randgen_t *rg   = &vRandom[nBufID];
    nBufID          = (nBufID + 1) & 0x03;
    rg->vLast       = (rg->vMul1 * rg->vLast) + ((rg->vMul2 * rg->vLast) >> 16) + rg->vAdd;
    return rg->vLast * RAND_RANGE;
}

float Randomizer::random(random_function_t func)                // :117-143
{
    float rv = generate_linear();
    switch (func)
    {
        case RND_EXP:
            return (expf(RAND_LAMBDA * rv) - 1.0f) / (expf(RAND_LAMBDA) - 1.0f);
        case RND_TRIANGLE:
            return (rv <= 0.5f) ?
                M_SQRT2 * RAND_T * sqrtf(rv) :
                2.0f*RAND_T - sqrtf(4.0f - 2.0f*(1.0f + rv)) * RAND_T;
        case RND_GAUSSIAN:
        {
            float rv2 = generate_linear();
            return sqrtf(-2.0f * logf(rv)) * cosf(2.0f * M_PI * rv2);
        }
        default:
            return rv;
    }
}

void Randomizer::dump(IStateDumper *v) const                    // :145-163
{
    v->begin_array("vRandom", vRandom, 4);
    for (size_t i = 0; i < 4; ++i)
    {
        const randgen_t *r = &vRandom[i];
        v->begin_object(r, sizeof(randgen_t));
        {
            v->write("vLast", r->vLast);
            v->write("vMul1", r->vMul1);
            v->write("vMul2", r->vMul2);
            v->write("vAdd", r->vAdd);
        }
        v->end_object();
    }
    v->end_array();
    v->write("nBufID", nBufID);
}

// ---- LCG --------------------------------------------------------------------------------------------------------------------------
LCG::LCG()      { construct(); }
LCG::~LCG()     { destroy(); }

void LCG::construct()                                           // :38-43
{
    enDistribution  = LCG_UNIFORM;
    fAmplitude      = 1.0f;
    fOffset         = 0.0f;
}

void LCG::destroy()             {}
void LCG::init(uint32_t seed)   { sRand.init(seed); }
void LCG::init()                { sRand.init(); }

float LCG::process_single()                                     // :60-85
{
    switch (enDistribution)
    {
        case LCG_EXPONENTIAL:
        {
            float sign;
            if (sRand.random(RND_LINEAR) >= 0.5f)
                sign = 1.0f;
            else
                sign = -1.0f;
            return sign * fAmplitude * sRand.random(RND_EXP) + fOffset;
        }
        case LCG_TRIANGULAR:
            return 2.0f * fAmplitude * sRand.random(RND_TRIANGLE) - 0.5f + fOffset;
        case LCG_GAUSSIAN:
            return fAmplitude * sRand.random(RND_GAUSSIAN) + fOffset;
        default:
        case LCG_UNIFORM:
            return 2.0f * fAmplitude * (sRand.random(RND_LINEAR) - 0.5f) + fOffset;
    }
}

void LCG::run(float *dst, const float *src, size_t count, unsigned op)
{
    bench &b = tl_bench;
    if (count == 0 || sRand.nBufID > 3)
        return;
    if (b.lcg == nullptr && mi_lcg_bank_create(&b.lcg, 1) != MI_OK)
        return;
    mi_lcg_state_t s;
    for (size_t i = 0; i < 4; ++i)
        s.last[i] = sRand.vRandom[i].vLast, s.mul1[i] = sRand.vRandom[i].vMul1, s.mul2[i] = sRand.vRandom[i].vMul2, s.add[i] = sRand.vRandom[i].vAdd;
    s.buf_id = uint32_t(sRand.nBufID);
    if (mi_lcg_bank_set_state(b.lcg, 0, &s, nullptr) != MI_OK)
        return;
    mi_lcg_bank_set_distribution(b.lcg, 0, uint32_t(enDistribution));
    mi_lcg_bank_set_amplitude(b.lcg, 0, fAmplitude);
    mi_lcg_bank_set_offset(b.lcg, 0, fOffset);
    for (size_t at = 0; at < count; at += PIECE)
    {
        const size_t n = (count - at < PIECE) ? count - at : PIECE;
        if (!b.piece(dst + at, (src != nullptr) ? src + at : nullptr, n, [&](float *d, const float *x)
                     { return mi_lcg_bank_process(b.lcg, d, x, n, n, n, op, nullptr); }))
            break;
    }
    if (mi_lcg_bank_get_state(b.lcg, 0, &s, nullptr) != MI_OK)  // where the device got to, also behind a piece that failed
        return;
    for (size_t i = 0; i < 4; ++i)
        sRand.vRandom[i].vLast = s.last[i];
    sRand.nBufID = s.buf_id;
}

void LCG::process_add(float *dst, const float *src, size_t count)   { run(dst, src, count, MI_OSC_ADD); }
void LCG::process_mul(float *dst, const float *src, size_t count)   { run(dst, src, count, MI_OSC_MUL); }
void LCG::process_overwrite(float *dst, size_t count)               { run(dst, nullptr, count, MI_OSC_OVERWRITE); }

void LCG::dump(IStateDumper *v) const                           // :105-113
{
    v->write_object("sRand", &sRand);
    v->write("enDistribution", enDistribution);
    v->write("fAmplitude", fAmplitude);
    v->write("fOffset", fOffset);
}

// ---- MLS --------------------------------------------------------------------------------------------------------------------------
MLS::MLS()      { construct(); }
MLS::~MLS()     { destroy(); }

void MLS::construct()                                           // :89-103
{
    nBits = sizeof(mls_t) * 8;
    nFeedbackBit = 0, nFeedbackMask = 0, nActiveMask = 0, nTapsMask = 0;
    nOutputMask = 1;
    nState = 0;
    fAmplitude = 1.0f, fOffset = 0.0f;
    bSync = true;
}

void MLS::destroy()                         {}
bool MLS::needs_update() const              { return bSync; }
size_t MLS::maximum_number_of_bits() const  { return sizeof(mls_t) * 8; }

void MLS::set_n_bits(size_t nbits)                              // :114-121
{
    if (nbits == nBits)
        return;
    nBits = nbits;
    bSync = true;
}

void MLS::set_state(mls_t targetstate)                          // :123-130
{
    if (targetstate == nState)
        return;
    nState = targetstate;
    bSync = true;
}

void MLS::set_amplitude(float amplitude)    { fAmplitude = amplitude; }
void MLS::set_offset(float offset)          { fOffset = offset; }

void MLS::update_settings()                                     // :153-179, the arithmetic the bank uses
{
    if (!bSync)
        return;
    mi_mls_settings_t s;
    mi_mls_settings_init(&s);
    s.n_bits = nBits, s.state = nState;
    mi_mls_settings_update(&s);
    nBits = s.n_bits, nFeedbackBit = s.feedback_bit, nFeedbackMask = s.feedback_mask, nActiveMask = s.active_mask;
    nTapsMask = s.taps_mask, nState = s.state;
    bSync = false;
}

MLS::mls_t MLS::xor_gate(mls_t value)       { return mls_t(__builtin_parityll(value)); }        // :182-197

MLS::mls_t MLS::get_period() const                              // :199-206
{
    return (nBits >= sizeof(mls_t) * 8) ? ~mls_t(0) : (mls_t(1) << nBits) - 1;
}

MLS::mls_t MLS::progress()                                      // :208-221
{
    update_settings();
    mls_t nOutput = nState & nOutputMask;
    mls_t nFeedbackValue = xor_gate(nState & nTapsMask);
    nState = nState >> 1;
    nState = (nState & ~nFeedbackMask) | (nFeedbackValue << nFeedbackBit);
    return nOutput;
}

float MLS::process_single()                                     // :223-227
{
    return progress() ? fAmplitude + fOffset : -fAmplitude + fOffset;
}

void MLS::run(float *dst, const float *src, size_t count, unsigned op)
{
    bench &b = tl_bench;
    if (count == 0)
        return;
    update_settings();                                          // progress() opens with it
    if (b.mls == nullptr && mi_mls_bank_create(&b.mls, 1) != MI_OK)
        return;
    mi_mls_bank_set_n_bits(b.mls, 0, nBits);
    mi_mls_bank_set_state(b.mls, 0, nState);
    mi_mls_bank_set_amplitude(b.mls, 0, fAmplitude);
    mi_mls_bank_set_offset(b.mls, 0, fOffset);
    for (size_t at = 0; at < count; at += PIECE)
    {
        const size_t n = (count - at < PIECE) ? count - at : PIECE;
        if (!b.piece(dst + at, (src != nullptr) ? src + at : nullptr, n, [&](float *d, const float *x)
                     { return mi_mls_bank_process(b.mls, d, x, n, n, n, op, nullptr); }))
            break;
    }
    uint64_t s = nState;
    if (mi_mls_bank_get_state(b.mls, 0, &s, nullptr) == MI_OK)  // where the device got to, also behind a piece that failed
        nState = s;
}

void MLS::process_add(float *dst, const float *src, size_t count)   { run(dst, src, count, MI_OSC_ADD); }
void MLS::process_mul(float *dst, const float *src, size_t count)   { run(dst, src, count, MI_OSC_MUL); }
void MLS::process_overwrite(float *dst, size_t count)               { run(dst, nullptr, count, MI_OSC_OVERWRITE); }

void MLS::dump(IStateDumper *v) const                           // :247-264
{
    v->write("vTapsMaskTable", static_cast<const void *>(mi_mls::taps()));
    v->write("nMaxBits", sizeof(mls_t) * 8);
    v->write("nBits", nBits);
    v->write("nFeedbackBit", nFeedbackBit);
    v->write("nFeedbackMask", nFeedbackMask);
    v->write("nActiveMask", nActiveMask);
    v->write("nTapsMask", nTapsMask);
    v->write("nOutputMask", nOutputMask);
    v->write("nState", nState);
    v->write("fAmplitude", fAmplitude);
    v->write("fOffset", fOffset);
    v->write("bSync", bSync);
}

} // namespace dspu
} // namespace lsp
