// lsp::dspu::Depopper's designer on the host (src/main/util/Depopper.cpp): init(), the setters, calc_fade() and reconfigure() line
// for line, quirks included -- the setters compare the new value with a clamped old one and store it unclamped,
// set_fade_out_delay reads fThresh for its old value, M_PI * 0.5f * k is a double narrowed to float, k = 1.0f / time is infinite
// at a fade time of 0.  crossfade() is the reference's expression with this host's sinf and expf; the bank tabulates it for
// x = 0 .. nSamples - 1, so that the device never evaluates a transcendental.
#include "depopper_bank.h"

#include <cmath>
#include <cstring>

#pragma clang fp contract(off)

namespace mi_depopper
{
namespace
{
    constexpr float GAIN_AMP_M_80_DB = 0.0001f;             // const.h

    inline float millis_to_samples(float sr, float time)    { return (time * 0.001f) * sr; }      // units.h
    inline int64_t align_size(int64_t v, int64_t align)     { const int64_t off = v % align; return (off == 0) ? v : v + align - off; }
    inline float lsp_max(float a, float b)                  { return (a > b) ? a : b; }
    inline float lsp_limit(float x, float lo, float hi)     { return (x < lo) ? lo : ((x > hi) ? hi : x); }
    // a float that the reference turns into size_t / ssize_t: defined, and within what the bank counts
    inline bool countable(float v)                          { return v > -MAX_SAMPLES_FLOAT && v < MAX_SAMPLES_FLOAT; }

    void calc_fade(const unit &u, fade_t *fade, bool in)    // :153-252, after the two conversions
    {
        float time          = millis_to_samples(float(u.nSampleRate), fade->fTime);
        fade->nDelay        = int64_t(millis_to_samples(float(u.nSampleRate), fade->fDelay));
        fade->nSamples      = int64_t(time);
        float k             = 1.0f / time;

        switch (fade->enMode)
        {
            case MI_DEPOPPER_LINEAR:
                if (in)
                {
                    fade->fPoly[0]  = 0.0f;
                    fade->fPoly[1]  = k;
                }
                else
                {
                    fade->fPoly[0]  = 1.0f;
                    fade->fPoly[1]  = -k;
                }
                fade->fPoly[2]  = 0.0f;
                fade->fPoly[3]  = 0.0f;
                break;

            case MI_DEPOPPER_CUBIC:
                if (in)
                {
                    fade->fPoly[0]  =  0.0f;
                    fade->fPoly[1]  =  0.0f;
                    fade->fPoly[2]  = +3.0f * k*k;
                    fade->fPoly[3]  = -2.0f * k*k*k;
                }
                else
                {
                    fade->fPoly[0]  = +1.0f;
                    fade->fPoly[1]  =  0.0f;
                    fade->fPoly[2]  = -3.0f * k*k;
                    fade->fPoly[3]  = +2.0f * k*k*k;
                }
                break;

            case MI_DEPOPPER_SINE:
                fade->fPoly[0]  = float(M_PI * 0.5f * k);               // double * float * float, narrowed
                if (in)
                    fade->fPoly[1]  = 0.0f;
                else
                    fade->fPoly[1]  = float(M_PI_2);
                fade->fPoly[2]  = 0.0f;
                fade->fPoly[3]  = 0.0f;
                break;

            case MI_DEPOPPER_PARABOLIC:
                if (in)
                {
                    fade->fPoly[0]  = 0.0f;
                    fade->fPoly[1]  = 0.0f;
                    fade->fPoly[2]  = k*k;
                }
                else
                {
                    fade->fPoly[0]  = +1.0f;
                    fade->fPoly[1]  = -2.0f * k;
                    fade->fPoly[2]  = k*k;
                }
                fade->fPoly[3]  = 0.0f;
                break;

            case MI_DEPOPPER_GAUSSIAN:
            {
                float f0        = expf(-16.0f);
                float f4        = 1.0f;
                fade->fPoly[0]  = 4.0f * k;
                fade->fPoly[1]  = (in) ? -4.0f : 0.0f;
                fade->fPoly[2]  = 1.0f / (f4 - f0);
                fade->fPoly[3]  = -f0;
                break;
            }

            default:
                fade->fPoly[0]  = 0.0f;
                fade->fPoly[1]  = 0.0f;
                fade->fPoly[2]  = 0.0f;
                fade->fPoly[3]  = 0.0f;
                break;
        }
    }
} // namespace

void construct(unit &u)
{
    u.nSampleRate       = uint64_t(-1);
    u.fLookMax          = 0.0f;
    u.nLookMin = u.nLookMax = u.nLookCount = 0;
    u.fRmsMax           = 0.0f;
    u.fRmsLength        = 0.0f;
    u.nRmsMin = u.nRmsMax = u.nRmsLen = 0;
    u.fRmsNorm          = 0.0f;
    u.sFadeIn           = fade_t();
    u.sFadeIn.fThresh   = GAIN_AMP_M_80_DB;
    u.sFadeIn.fTime     = 50.0f;
    u.sFadeOut          = fade_t();
    u.sFadeOut.fThresh  = GAIN_AMP_M_80_DB;
    u.bReconfigure      = true;
    u.inited            = false;
}

int init(unit &u, uint64_t srate, float max_fade, float max_rms, const char **why)
{
    if ((u.nSampleRate == srate) && (u.fLookMax == max_fade) && (u.fRmsMax == max_rms))
        return 0;                                           // true without a buffer, too, as in the reference

    const float lk = millis_to_samples(float(srate), max_fade), rms = millis_to_samples(float(srate), max_rms);
    if (!(lk >= 0.0f && rms >= 0.0f && lk < MAX_BUFFER_FLOAT && rms < MAX_BUFFER_FLOAT))
    {
        *why = "the maximum fade or RMS time is negative, not a number (a size_t in the reference) or 2^24 samples and more";
        return -1;
    }

    u.nSampleRate       = srate;
    u.fLookMax          = max_fade;
    u.fRmsMax           = max_rms;

    int64_t lk_samp     = int64_t(lk);
    int64_t rms_samp    = int64_t(rms);
    int64_t lk_buf      = align_size(lk_samp, DEFAULT_ALIGN);
    int64_t rms_buf     = align_size(rms_samp, DEFAULT_ALIGN);

    u.nLookMin          = lk_buf + rms_buf;
    u.nLookMax          = u.nLookMin + ((lk_buf * 4 > BUF_SIZE) ? lk_buf * 4 : BUF_SIZE);
    u.nRmsMin           = rms_buf;
    u.nRmsMax           = u.nRmsMin + ((rms_buf * 4 > BUF_SIZE) ? rms_buf * 4 : BUF_SIZE);
    u.bReconfigure      = true;
    u.inited            = true;
    return 1;
}

uint32_t set_fade_mode(unit &u, bool in, uint32_t mode)
{
    fade_t &f = in ? u.sFadeIn : u.sFadeOut;
    uint32_t old = f.enMode;
    if (mode == old)
        return old;
    f.enMode        = mode;
    u.bReconfigure  = true;
    return old;
}

float set_fade_in_time(unit &u, float time)
{
    float old = lsp_max(0.0f, u.sFadeIn.fTime);
    if (old == time)
        return old;
    u.sFadeIn.fTime = time;
    u.bReconfigure  = true;
    return old;
}

float set_fade_out_time(unit &u, float time)
{
    float old = lsp_limit(u.sFadeOut.fTime, 0.0f, u.fLookMax);
    if (old == time)
        return old;
    u.sFadeOut.fTime = time;
    u.bReconfigure  = true;
    return old;
}

float set_fade_threshold(unit &u, bool in, float thresh)
{
    fade_t &f = in ? u.sFadeIn : u.sFadeOut;
    float old = lsp_max(0.0f, f.fThresh);
    if (old == thresh)
        return old;
    f.fThresh       = thresh;
    u.bReconfigure  = true;
    return old;
}

float set_fade_in_delay(unit &u, float delay)
{
    float old = lsp_max(0.0f, u.sFadeIn.fDelay);
    if (old == delay)
        return old;
    u.sFadeIn.fDelay = delay;
    u.bReconfigure  = true;
    return old;
}

float set_fade_out_delay(unit &u, float delay)
{
    float old = lsp_max(0.0f, u.sFadeOut.fThresh);          // fThresh, as in the reference (:358)
    if (old == delay)
        return old;
    u.sFadeOut.fDelay = delay;
    u.bReconfigure  = true;
    return old;
}

float set_rms_length(unit &u, float length)
{
    length = lsp_limit(length, 0.0f, u.fRmsMax);
    float old = u.fRmsLength;
    if (old == length)
        return old;
    u.fRmsLength    = length;
    u.bReconfigure  = true;
    return old;
}

const char *reconfigure(unit &u, bool *designed)
{
    if (designed != nullptr)
        *designed = false;
    if (!u.inited)
        return "a channel without init(): the reference has no buffers";
    const float sr = float(u.nSampleRate);
    const float conv[5] = { millis_to_samples(sr, u.sFadeIn.fTime), millis_to_samples(sr, u.sFadeIn.fDelay),
                            millis_to_samples(sr, u.sFadeOut.fTime), millis_to_samples(sr, u.sFadeOut.fDelay),
                            millis_to_samples(sr, u.fRmsLength) };
    for (float v : conv)
        if (!countable(v))
            return "a time that is not a number or too long (its conversion to ssize_t is undefined in the reference)";
    if (u.sFadeIn.enMode > MI_DEPOPPER_PARABOLIC || u.sFadeOut.enMode > MI_DEPOPPER_PARABOLIC)
        return "a fade mode that is none of depopper_mode_t";

    if (designed != nullptr)
        *designed = true;
    calc_fade(u, &u.sFadeIn, true);
    calc_fade(u, &u.sFadeOut, false);
    u.nRmsLen           = int64_t(conv[4]);
    u.nLookCount        = u.sFadeOut.nSamples + u.nRmsLen;
    u.fRmsNorm          = 1.0f / float(u.nRmsLen);

    if (u.nRmsLen == 0)
        return "nRmsLen == 0: fRmsNorm is 1 / 0 in the reference (set an RMS length of at least one sample)";
    if (!(u.sFadeOut.fTime >= 0.0f && u.sFadeOut.fTime <= u.fLookMax))
        return "a fade-out time below 0 or above max_fade: the reference patches and reads outside its gain buffer";
    if (u.sFadeIn.nSamples > MAX_FADE_IN_SAMPLES)
        return "a fade-in of more than 2^20 samples: the bank keeps one table entry per sample";
    return nullptr;
}

float crossfade(const fade_t &f, float x)
{
    if (x < 0.0f)
        return 0.0f;
    else if (x >= f.nSamples)
        return 1.0f;

    float gain;
    switch (f.enMode)
    {
        case MI_DEPOPPER_LINEAR:
        case MI_DEPOPPER_CUBIC:
        case MI_DEPOPPER_PARABOLIC:
            gain        = f.fPoly[0] + x*(f.fPoly[1] + x*(f.fPoly[2] + x*f.fPoly[3]));
            break;
        case MI_DEPOPPER_SINE:
            x           = sinf(f.fPoly[0] * x + f.fPoly[1]);
            gain        = x*x;
            break;
        case MI_DEPOPPER_GAUSSIAN:
            x           = (f.fPoly[0] * x + f.fPoly[1]);
            gain        = f.fPoly[2] * expf(-x*x) + f.fPoly[3];
            break;
        default:
            gain        = 0.0f;
            break;
    }
    return gain;
}

void tabulate(const fade_t &f, std::vector<float> &table)
{
    table.resize((f.nSamples > 0) ? size_t(f.nSamples) : 0);
    for (size_t x = 0; x < table.size(); ++x)
        table[x] = crossfade(f, float(int64_t(x)));
}

float square_threshold(float thresh)
{
    if (thresh != thresh)
        return thresh;                                      // s < NaN never holds, q < NaN neither
    if (!(thresh > 0.0f))
        return -INFINITY;                                   // s >= 0 is never below it
    // the bit patterns of the floats 0 .. +Inf are ordered as the floats are, and sqrtf is monotone
    uint32_t lo = 0, hi = 0x7f800000u;                      // sqrtf(+Inf) >= thresh always
    while (lo < hi)
    {
        const uint32_t mid = lo + (hi - lo) / 2;
        float q;
        memcpy(&q, &mid, sizeof(q));
        if (sqrtf(q) >= thresh)
            hi = mid;
        else
            lo = mid + 1;
    }
    float q;
    memcpy(&q, &lo, sizeof(q));
    return q;
}

} // namespace mi_depopper
