// lsp::dspu::Depopper (src/main/util/Depopper.cpp) on a mi_depopper_bank of one channel kept beside the object (beside.h).  The
// object's fields and its two host buffers are what counts: init() makes and zeroes the buffers, the setters are the reference's
// line for line, reconfigure() takes the designed values from mi_depopper_compute_params (the bank's own designer, no device) and
// sums fRms over the object's buffer.  process() hands the fields to the bank (set_settings), the state words and the buffers'
// last nRmsMin / nLookMin entries where they are not what the previous call read back (set_state), runs the bank, and reads
// the state and both buffers' logical contents back to where the reference's shifted buffers would hold them.
#include <lsp-plug.in/dsp-units/util/Depopper.h>

#include <cstddef>
#include <cstdlib>
#include <vector>

#include "beside.h"

namespace lsp
{
namespace dspu
{
namespace
{
    // the state words as the device holds them, in 32-bit fields (the offsets stay below 2^31, the counters below 2^30)
    struct depopper_held { float rms = 0.0f; uint32_t state = 0; int32_t counter = 0, delay = 0; uint32_t rms_off = 0, look_off = 0, buffers = 0; };
    typedef mi_host::registry<mi_host::beside<mi_depopper_bank_t, depopper_held, mi_depopper_bank_destroy> > depoppers;

    static_assert(sizeof(void *) != 8 || sizeof(Depopper) == 248, "sizeof(Depopper)");

    inline float lsp_max(float a, float b)                  { return (a > b) ? a : b; }
    inline float lsp_limit(float x, float lo, float hi)     { return (x < lo) ? lo : ((x > hi) ? hi : x); }

    template <class Fade> void fade_settings(mi_depopper_fade_t &d, const Fade &f)
    {
        d.mode = uint32_t(f.enMode), d.threshold = f.fThresh, d.time = f.fTime, d.delay = f.fDelay;
    }
    template <class Fade> void fade_designed(Fade &f, const mi_depopper_fade_t &d)
    {
        f.nSamples = ssize_t(d.samples), f.nDelay = ssize_t(d.delay_samples);
        memcpy(f.fPoly, d.poly, sizeof(f.fPoly));
    }
}

Depopper::Depopper()    { construct(); }
Depopper::~Depopper()   { destroy(); }

void Depopper::construct()                                      // :44-94
{
    depoppers::drop(this);                                      // whatever lived at this address before
    nSampleRate         = -1;
    nState              = ST_CLOSED;
    fLookMax            = 0.0f;
    nLookMin = nLookMax = nLookOff = nLookCount = 0;
    fRmsMax             = 0.0f;
    fRmsLength          = 0.0f;
    nRmsMin = nRmsMax = nRmsOff = nRmsLen = 0;
    fRmsNorm            = 0.0f;
    nCounter = nDelay   = 0;
    fRms                = 0.0f;
    fade_t *fades[2]    = { &sFadeIn, &sFadeOut };
    for (fade_t *f : fades)
    {
        f->enMode       = DPM_LINEAR;
        f->fThresh      = 0.0001f;                              // GAIN_AMP_M_80_DB
        f->fTime        = 0.0f;
        f->fDelay       = 0.0f;
        f->nSamples     = 0;
        f->nDelay       = 0;
        f->fPoly[0] = f->fPoly[1] = f->fPoly[2] = f->fPoly[3] = 0.0f;
    }
    sFadeIn.fTime       = 50.0f;
    pGainBuf = pRmsBuf  = NULL;
    pData               = NULL;
    bReconfigure        = true;
}

void Depopper::destroy()                                        // :96-106
{
    depoppers::drop(this);
    free(pData);
    pData               = NULL;
    pGainBuf = pRmsBuf  = NULL;
}

bool Depopper::init(size_t srate, float max_fade, float max_rms)        // :108-151
{
    if ((nSampleRate == srate) && (fLookMax == max_fade) && (fRmsMax == max_rms))
        return true;

    // the extents are the designer's (init() of host/depopper.cpp); it refuses maxima whose conversion is undefined
    mi_depopper_params_t d = {};
    if (mi_depopper_compute_extents(srate, max_fade, max_rms, &d) != MI_OK)
        return false;

    free(pData);
    pData = NULL, pGainBuf = pRmsBuf = NULL;
    nSampleRate         = srate;
    fLookMax            = max_fade;
    fRmsMax             = max_rms;
    nLookMin            = ssize_t(d.look_min_off);
    nLookMax            = ssize_t(d.look_max_off);
    nLookOff            = nLookMin;
    nRmsMin             = ssize_t(d.rms_min_off);
    nRmsMax             = ssize_t(d.rms_max_off);
    nRmsOff             = nRmsMin;

    void *data          = NULL;
    if (posix_memalign(&data, 0x40, size_t(nRmsMax + nLookMax) * sizeof(float)) != 0)
        return false;
    memset(data, 0, size_t(nRmsMax + nLookMax) * sizeof(float));
    pData               = static_cast<uint8_t *>(data);
    pGainBuf            = static_cast<float *>(data);
    pRmsBuf             = &pGainBuf[nLookMax];
    nState              = ST_CLOSED;
    bReconfigure        = true;
    return true;
}

void Depopper::reconfigure()                                    // :254-270
{
    if (!bReconfigure)
        return;
    if (pData == NULL)
        return;                                                 // the reference reads a NULL buffer here
    mi_depopper_params_t s = {}, d = {};
    s.sample_rate = nSampleRate, s.look_max = fLookMax, s.rms_max = fRmsMax, s.rms_length = fRmsLength;
    fade_settings(s.fade_in, sFadeIn);
    fade_settings(s.fade_out, sFadeOut);
    if (mi_depopper_compute_params(&s, &d, NULL, 0, NULL, 0) != MI_OK && d.reconfigure != 0)
        return;                                                 // times that are no numbers: nothing is defined, nothing is written
    fade_designed(sFadeIn, d.fade_in);
    fade_designed(sFadeOut, d.fade_out);
    nRmsLen             = ssize_t(d.rms_len);
    nLookCount          = ssize_t(d.look_count);
    fRmsNorm            = d.rms_norm;

    float sum           = 0.0f;                                 // dsp::h_sum(&pRmsBuf[nRmsOff - nRmsLen], nRmsLen)
    if (nRmsLen >= 0 && nRmsLen <= nRmsOff)
        for (ssize_t i = nRmsOff - nRmsLen; i < nRmsOff; ++i)
            sum         = sum + pRmsBuf[i];
    fRms                = sum;
    bReconfigure        = false;
}

depopper_mode_t Depopper::set_fade_in_mode(depopper_mode_t mode)        // :272-282
{
    depopper_mode_t old = sFadeIn.enMode;
    if (mode == old)
        return old;
    sFadeIn.enMode      = mode;
    bReconfigure        = true;
    return old;
}

depopper_mode_t Depopper::set_fade_out_mode(depopper_mode_t mode)       // :284-294
{
    depopper_mode_t old = sFadeOut.enMode;
    if (mode == old)
        return old;
    sFadeOut.enMode     = mode;
    bReconfigure        = true;
    return old;
}

float Depopper::set_fade_in_time(float time)                    // :296-306
{
    float old           = lsp_max(0.0f, sFadeIn.fTime);
    if (old == time)
        return old;
    sFadeIn.fTime       = time;
    bReconfigure        = true;
    return old;
}

float Depopper::set_fade_out_time(float time)                   // :308-318
{
    float old           = lsp_limit(sFadeOut.fTime, 0.0f, fLookMax);
    if (old == time)
        return old;
    sFadeOut.fTime      = time;
    bReconfigure        = true;
    return old;
}

float Depopper::set_fade_in_threshold(float thresh)             // :320-330
{
    float old           = lsp_max(0.0f, sFadeIn.fThresh);
    if (old == thresh)
        return old;
    sFadeIn.fThresh     = thresh;
    bReconfigure        = true;
    return old;
}

float Depopper::set_fade_out_threshold(float thresh)            // :332-342
{
    float old           = lsp_max(0.0f, sFadeOut.fThresh);
    if (old == thresh)
        return old;
    sFadeOut.fThresh    = thresh;
    bReconfigure        = true;
    return old;
}

float Depopper::set_fade_in_delay(float delay)                  // :344-354
{
    float old           = lsp_max(0.0f, sFadeIn.fDelay);
    if (old == delay)
        return old;
    sFadeIn.fDelay      = delay;
    bReconfigure        = true;
    return old;
}

float Depopper::set_fade_out_delay(float delay)                 // :356-366
{
    float old           = lsp_max(0.0f, sFadeOut.fThresh);      // fThresh, as in the reference
    if (old == delay)
        return old;
    sFadeOut.fDelay     = delay;
    bReconfigure        = true;
    return old;
}

float Depopper::set_rms_length(float length)                    // :368-379
{
    length              = lsp_limit(length, 0.0f, fRmsMax);
    float old           = fRmsLength;
    if (old == length)
        return old;
    fRmsLength          = length;
    bReconfigure        = true;
    return old;
}

void Depopper::process(float *env, float *gain, const float *src, size_t count)        // :464-562
{
    const bool designed = bReconfigure;
    reconfigure();
    if (count == 0 || pData == NULL || bReconfigure)
        return;
    depoppers::entry *p = depoppers::of_one(this, mi_depopper_bank_create);
    if (p == NULL || !p->buf.reserve(count, 3))
        return;

    mi_depopper_params_t s = {};
    s.sample_rate = nSampleRate, s.look_max = fLookMax, s.rms_max = fRmsMax, s.rms_length = fRmsLength;
    fade_settings(s.fade_in, sFadeIn);
    fade_settings(s.fade_out, sFadeOut);
    s.reconfigure = designed ? 1u : 0u;
    if (mi_depopper_bank_set_settings(p->bank, 0, &s) != MI_OK || mi_depopper_bank_update_settings(p->bank, NULL) != MI_OK)
        return;                                                 // refused: env and gain stay as they are

    // the object's state where it is not what the device holds (the first call, init(), or fields written from outside)
    const depopper_held now = { fRms, uint32_t(nState), int32_t(nCounter), int32_t(nDelay), uint32_t(nRmsOff), uint32_t(nLookOff), 1 };
    if (memcmp(&now, &p->held, sizeof(now)) != 0)
    {
        const mi_depopper_state_t st = { fRms, uint32_t(nState), nCounter, nDelay, nRmsOff, nLookOff };
        if (mi_depopper_bank_set_state(p->bank, 0, &st, &pRmsBuf[nRmsOff - nRmsMin], &pGainBuf[nLookOff - nLookMin], NULL) != MI_OK)
            return;
        p->held = now;
    }

    float *d_src = p->buf.row(0), *d_env = p->buf.row(1), *d_gain = p->buf.row(2);
    mi_depopper_state_t st;
    const size_t kept_squares = nRmsMin, kept_gains = nLookMin;
    std::vector<float> squares(kept_squares), gains(kept_gains);
    if (!p->buf.up(0, src, count) ||
        mi_depopper_bank_process(p->bank, (env != NULL) ? d_env : NULL, d_gain, d_src, count, count, count, count, NULL) != MI_OK ||
        mi_depopper_bank_get_state(p->bank, 0, &st, squares.data(), gains.data(), NULL) != MI_OK)
    {
        p->held = depopper_held();
        return;
    }
    if ((env != NULL && !p->buf.down(env, 1, count)) ||
        !p->buf.down(gain, 2, count) || mi_dspu_stream_synchronize(NULL) != MI_OK)
    {
        p->held = depopper_held();
        return;
    }
    fRms = st.rms, nState = state_t(st.state), nCounter = ssize_t(st.counter), nDelay = ssize_t(st.delay);
    nRmsOff = ssize_t(st.rms_off), nLookOff = ssize_t(st.look_off);
    memcpy(&pRmsBuf[nRmsOff - nRmsMin], squares.data(), squares.size() * sizeof(float));
    memcpy(&pGainBuf[nLookOff - nLookMin], gains.data(), gains.size() * sizeof(float));
    p->held = depopper_held{ fRms, uint32_t(nState), int32_t(nCounter), int32_t(nDelay), uint32_t(nRmsOff), uint32_t(nLookOff), 1 };
}

namespace
{
    template <class Fade> void dump_fade(IStateDumper *v, const char *name, const Fade *fade)       // :564-577
    {
        v->begin_object(name, fade, sizeof(Fade));
        {
            v->write("enMode", fade->enMode);
            v->write("fThresh", fade->fThresh);
            v->write("fTime", fade->fTime);
            v->write("fDelay", fade->fDelay);
            v->write("nSamples", fade->nSamples);
            v->write("nDelay", fade->nDelay);
            v->writev("fPoly", fade->fPoly, 4);
        }
        v->end_object();
    }
}

void Depopper::dump(IStateDumper *v) const                      // :579-610
{
    v->write("nSampleRate", nSampleRate);
    v->write("nState", nState);

    v->write("fLookMax", fLookMax);
    v->write("nLookMin", nLookMin);
    v->write("nLookMax", nLookMax);
    v->write("nLookOff", nLookOff);
    v->write("nLookCount", nLookCount);

    v->write("fRmsMax", fRmsMax);
    v->write("fRmsLength", fRmsLength);
    v->write("nRmsMin", nRmsMin);
    v->write("nRmsMax", nRmsMax);
    v->write("nRmsOff", nRmsOff);
    v->write("nRmsLen", nRmsLen);
    v->write("fRmsNorm", fRmsNorm);

    v->write("nCounter", nCounter);
    v->write("nDelay", nDelay);
    v->write("fRms", fRms);

    dump_fade(v, "sFadeIn", &sFadeIn);
    dump_fade(v, "sFadeOut", &sFadeOut);

    v->write("pGainBuf", pGainBuf);
    v->write("pRmsBuf", pRmsBuf);
    v->write("pData", pData);

    v->write("bReconfigure", bReconfigure);
}

} // namespace dspu
} // namespace lsp
