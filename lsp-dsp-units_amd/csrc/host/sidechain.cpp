// lsp::dspu::Sidechain (src/main/util/Sidechain.cpp) on a mi_sidechain_bank of one channel.  The class has no member to hang
// the bank on (its 80 bytes are the reference's), so the bank and its staging buffers live beside the object (beside.h's
// registry): made at the first call that needs the device, dropped in destroy() and in construct().  Before every device call
// the bank is handed the object's own nReactivity, fTau, nMode, nSource, fGain, the mid-side flag and the ring's capacity;
// process() also sends fRmsValue, nRefresh and the ring position when they are not what it read back after the previous
// call (set_mode() zeroes fRmsValue, update_settings() writes nRefresh, a subclass may write the protected fields), and
// reads them back afterwards.  An object whose storage is released without destroy() or its destructor leaves its entry
// behind until a Sidechain is constructed at that address again.
#include <lsp-plug.in/dsp-units/util/Sidechain.h>
#include <lsp-plug.in/dsp-units/units.h>

#include <cmath>
#include <cstddef>
#include <cstring>

#include "beside.h"
#include "sidechain_bank.h"

namespace lsp
{
namespace dspu
{
namespace
{
    constexpr uint32_t REFRESH_RATE = 0x2000;                   // Sidechain.cpp:31
    constexpr size_t   RING_EXTRA   = 0x200;                    // BLOCK_SIZE, :30

    struct sidechain_impl
    {
        mi_sidechain_bank_t *bank = nullptr;
        uint32_t inputs = 0;
        mi_host::rows buf;                  // [3][cap]: the staged inputs, the output
        float   rms = 0.0f;                 // the state as the device holds it: a fresh bank's, then what process() read back
        uint32_t refresh = 0, head = 0;
        bool    known = false;              // ... which it does only after the first hand-over

        ~sidechain_impl() { if (bank != nullptr) mi_sidechain_bank_destroy(bank); }
    };
    typedef mi_host::registry<sidechain_impl> sidechains;

    // the object's bank of `inputs` inputs
    sidechain_impl *impl_of(const void *self, uint32_t inputs)
    {
        sidechain_impl *p = sidechains::find(self);
        if (p != nullptr && p->inputs == inputs)
            return p;
        sidechains::drop(self);                                 // init() changed the number of inputs
        return sidechains::of(self, [inputs](sidechain_impl &e)
        {
            e.inputs = inputs;
            return mi_sidechain_bank_create(&e.bank, 1, inputs, 0.0f);
        });
    }

    // the layout of the reference class, LP64
    struct layout: public Sidechain
    {
        static void check()
        {
            constexpr bool lp64 = sizeof(void *) == 8 && sizeof(size_t) == 8;
            static_assert(!lp64 || sizeof(Sidechain) == 80, "sizeof(Sidechain)");
            static_assert(!lp64 || sizeof(RawRingBuffer) == 24, "sizeof(RawRingBuffer)");
            #pragma GCC diagnostic push
            #pragma GCC diagnostic ignored "-Winvalid-offsetof"
            static_assert(!lp64 || (offsetof(layout, sBuffer) == 0 && offsetof(layout, nReactivity) == 24 &&
                                    offsetof(layout, nSampleRate) == 32 && offsetof(layout, pPreEq) == 40 &&
                                    offsetof(layout, fReactivity) == 48 && offsetof(layout, fTau) == 52 &&
                                    offsetof(layout, fRmsValue) == 56 && offsetof(layout, fMaxReactivity) == 60 &&
                                    offsetof(layout, fGain) == 64 && offsetof(layout, nRefresh) == 68 &&
                                    offsetof(layout, nSource) == 72 && offsetof(layout, nMode) == 73 &&
                                    offsetof(layout, nChannels) == 74 && offsetof(layout, nFlags) == 75), "member offsets");
            #pragma GCC diagnostic pop
        }
    };
}

Sidechain::Sidechain()  { construct(); }
Sidechain::~Sidechain() { destroy(); }

void Sidechain::construct()                                     // Sidechain.cpp:43-60
{
    sidechains::drop(this);                                     // whatever lived at this address before
    sBuffer.construct();
    nReactivity = 0;
    fReactivity = 0.0f;
    fTau = 0.0f;
    fRmsValue = 0.0f;
    nSource = SCS_MIDDLE;
    nMode = SCM_RMS;
    nSampleRate = 0;
    nRefresh = 0;
    nChannels = 0;
    fMaxReactivity = 0.0f;
    fGain = 1.0f;
    nFlags = SCF_UPDATE | SCF_CLEAR;
    pPreEq = NULL;
}

void Sidechain::destroy()                                       // :62-65
{
    sidechains::drop(this);
    sBuffer.destroy();
}

bool Sidechain::init(size_t channels, float max_reactivity)     // :67-86
{
    if ((channels != 1) && (channels != 2))
        return false;
    nReactivity = 0;
    fReactivity = 0.0f;
    fTau = 0.0f;
    fRmsValue = 0.0f;
    nSource = SCS_MIDDLE;
    nMode = SCM_RMS;
    nSampleRate = 0;
    nRefresh = 0;
    nChannels = uint8_t(channels);
    fMaxReactivity = max_reactivity;
    fGain = 1.0f;
    nFlags = SCF_UPDATE | SCF_CLEAR;
    return true;
}

void Sidechain::set_sample_rate(size_t sr)                      // :88-93
{
    nSampleRate = sr;
    nFlags = SCF_UPDATE | SCF_CLEAR;
    const float m = millis_to_samples(float(sr), fMaxReactivity);
    const float c = ((m > 1.0f) ? m : 1.0f) + float(RING_EXTRA);
    sBuffer.init((c < 1073741824.0f) ? size_t(c) : 0);
}

void Sidechain::set_reactivity(float reactivity)                // :95-103
{
    if ((fReactivity == reactivity) || (reactivity < 0.0f) || (reactivity > fMaxReactivity))
        return;
    fReactivity = reactivity;
    nFlags |= SCF_UPDATE;
}

void Sidechain::set_stereo_mode(sidechain_stereo_mode_t mode)   // :105-112
{
    const sidechain_stereo_mode_t old = (nFlags & SCF_MIDSIDE) ? SCSM_MIDSIDE : SCSM_STEREO;
    if (old == mode)
        return;
    nFlags = uint8_t((mode == SCSM_MIDSIDE) ? (nFlags | SCF_MIDSIDE) : (nFlags & ~SCF_MIDSIDE));
    nFlags |= SCF_CLEAR;
}

void Sidechain::clear()                                         // :114-117
{
    nFlags |= SCF_CLEAR;
}

void Sidechain::update_settings()                               // :119-142
{
    if (!(nFlags & (SCF_UPDATE | SCF_CLEAR)))
        return;
    if (nFlags & SCF_UPDATE)
    {
        mi_sidechain_params_t p;
        const float react = (fReactivity >= 0.0f) ? fReactivity : 0.0f;
        if (mi_sidechain_compute_params(uint32_t(nSampleRate), (react > fMaxReactivity) ? react : fMaxReactivity, react, &p) == MI_OK)
        {
            nReactivity = p.reactivity;
            fTau = p.tau;
        }
        nRefresh = REFRESH_RATE;                                // force the function to be refreshed
    }
    if (nFlags & SCF_CLEAR)
    {
        fRmsValue = 0.0f;
        nRefresh = 0;
        sBuffer.fill(0.0f);
        if (pPreEq != NULL)
            pPreEq->reset();
    }
    nFlags &= ~(SCF_UPDATE | SCF_CLEAR);
}

void Sidechain::process(float *out, const float **in, size_t samples)      // :439-554
{
    const bool cleared = (nFlags & SCF_CLEAR) != 0;
    update_settings();
    if (samples == 0)
        return;
    if ((nChannels != 1) && (nChannels != 2))                   // :321-330: no source, no detector
    {
        if (in == NULL)
            return;
        memset(out, 0, samples * sizeof(float));
        if (pPreEq != NULL)
        {
            pPreEq->process(out, out, samples);
            for (size_t i = 0; i < samples; ++i)
                out[i] = fabsf(out[i]);
        }
        return;
    }
    const size_t capacity = sBuffer.size();
    if (capacity < nReactivity + RING_EXTRA || nReactivity < 1)
        return;                                                 // no sample rate was set: the reference has no ring either
    sidechain_impl *p = impl_of(this, nChannels);
    if (p == nullptr || !p->buf.reserve(samples, 3))
        return;

    // the object's fields as the bank's channel 0
    mi_sidechain_params_t q;
    q.reactivity = uint32_t(nReactivity);
    q.tau = fTau;
    q.interval = 1.0f / float(nReactivity);
    q.capacity = uint32_t(capacity);
    q.mode = nMode;
    q.source = nSource;
    q.flags = (nFlags & SCF_MIDSIDE) ? MI_SCF_MIDSIDE : 0;
    q.gain = fGain;
    if (mi::sidechain_bank_set_params(p->bank, 0, &q) != MI_OK)
        return;
    const uint32_t head = uint32_t(sBuffer.position());
    if (cleared || !p->known || memcmp(&fRmsValue, &p->rms, sizeof(float)) != 0 || nRefresh != p->refresh || head != p->head)
    {
        if (mi::sidechain_bank_set_state(p->bank, 0, fRmsValue, nRefresh, head, cleared, nullptr) != MI_OK)
            return;
    }
    p->known = false;

    float *d_in0 = p->buf.row(0), *d_in1 = p->buf.row(1), *d_out = p->buf.row(2);
    const bool two = nChannels == 2;
    if (in != NULL)
    {
        if (!p->buf.up(0, in[0], samples) || (two && !p->buf.up(1, in[1], samples)))
            return;
    }
    const float *a = (in != NULL) ? d_in0 : nullptr, *b = (in != NULL && two) ? d_in1 : nullptr;
    if (pPreEq != NULL && in != NULL)
    {
        // the signed source, the equalizer on it, then magnitude, gain, ring and detector
        if (mi_sidechain_bank_premix(p->bank, d_out, a, b, samples, samples, samples, samples, nullptr) != MI_OK ||
            !p->buf.down(out, 2, samples))
            return;
        pPreEq->process(out, out, samples);
        if (!p->buf.up(2, out, samples) ||
            mi_sidechain_bank_process_premixed(p->bank, d_out, d_out, samples, samples, samples, nullptr) != MI_OK)
            return;
    }
    else if (mi_sidechain_bank_process(p->bank, d_out, a, b, samples, samples, samples, samples, nullptr) != MI_OK)
        return;
    if (!p->buf.down(out, 2, samples) ||
        mi_sidechain_bank_get_state(p->bank, 0, &p->rms, &p->refresh, &p->head, nullptr) != MI_OK)
        return;
    p->known = true;
    fRmsValue = p->rms;
    nRefresh = p->refresh;
    sBuffer.reset();                                            // position() = p->head, which is the capacity after a block that
    if (p->head > 0)                                            // ended at the ring's end (RawRingBuffer.cpp:118-122): advance()
    {                                                           // alone would take it to 0.  The sample that this push
        const float nothing = 0.0f;                             // writes means nothing: the ring's samples live on the device
        sBuffer.advance(p->head - 1);
        sBuffer.push(&nothing, 1);
    }
}

float Sidechain::process(const float *in)                       // one sample through the block path (see the header)
{
    float out = 0.0f;
    const float *v[2] = { in, (nChannels == 2) ? in + 1 : in };
    process(&out, v, 1);
    return out;
}

void Sidechain::dump(IStateDumper *v) const                     // :626-642
{
    v->write_object("sBuffer", &sBuffer);
    v->write("nReactivity", nReactivity);
    v->write("nSampleRate", nSampleRate);
    v->write("pPreEq", pPreEq);
    v->write("fReactivity", fReactivity);
    v->write("fTau", fTau);
    v->write("fRmsValue", fRmsValue);
    v->write("fMaxReactivity", fMaxReactivity);
    v->write("fGain", fGain);
    v->write("nRefresh", nRefresh);
    v->write("nSource", nSource);
    v->write("nMode", nMode);
    v->write("nChannels", nChannels);
    v->write("nFlags", nFlags);
}

} // namespace dspu
} // namespace lsp
