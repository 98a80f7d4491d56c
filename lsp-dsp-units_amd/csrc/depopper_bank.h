// lsp::dspu::Depopper's host side, shared by the bank (depopper.hip) and the designer (host/depopper.cpp): one unit's settings as
// the reference's fields, init(), the setters, calc_fade() and reconfigure() restated line for line (util/Depopper.h,
// src/main/util/Depopper.cpp), the two fade tables, and the two thresholds taken from the envelope to its square.
#pragma once
#include "mi_dspu.h"

#include <cstdint>
#include <vector>

namespace mi_depopper
{
    // lsp-common-lib's DEFAULT_ALIGN is not pinned by anything in the reference tree; 0x40 is a stand-in.  Nothing
    // on the device assumes that it is a multiple of 32.
    constexpr int64_t DEFAULT_ALIGN = 0x40;
    constexpr int64_t BUF_SIZE      = 0x1000;               // Depopper.cpp:28

    // What the bank can hold.  A fade-in table is one float per sample; counters and delays are 32 bits wide on the device.
    constexpr int64_t MAX_FADE_IN_SAMPLES = int64_t(1) << 20;
    constexpr float   MAX_SAMPLES_FLOAT   = 1073741824.0f;  // 2^30: what float -> integer conversions are asked to stay below
    constexpr float   MAX_BUFFER_FLOAT    = 16777216.0f;    // 2^24: ... and the two maxima of init(), which size the rings

    struct fade_t                                           // Depopper::fade_t
    {
        uint32_t    enMode = MI_DEPOPPER_LINEAR;
        float       fThresh = 0.0f, fTime = 0.0f, fDelay = 0.0f;
        int64_t     nSamples = 0, nDelay = 0;
        float       fPoly[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
    };

    struct unit                                             // the reference's fields, without the state words and the buffers
    {
        uint64_t    nSampleRate;
        float       fLookMax;
        int64_t     nLookMin, nLookMax, nLookCount;
        float       fRmsMax, fRmsLength;
        int64_t     nRmsMin, nRmsMax, nRmsLen;
        float       fRmsNorm;
        fade_t      sFadeIn, sFadeOut;
        bool        bReconfigure;
        bool        inited;                                 // pData != NULL
    };

    void        construct(unit &u);                                                     // :44-94
    // :108-151.  0: nothing changed; 1: new extents, the buffers and the state start over; < 0: the sizes are undefined in the
    // reference (why: the message)
    int         init(unit &u, uint64_t srate, float max_fade, float max_rms, const char **why);
    uint32_t    set_fade_mode(unit &u, bool in, uint32_t mode);                         // :272-294
    float       set_fade_in_time(unit &u, float time);                                  // :296-306
    float       set_fade_out_time(unit &u, float time);                                 // :308-318
    float       set_fade_threshold(unit &u, bool in, float thresh);                     // :320-342
    float       set_fade_in_delay(unit &u, float delay);                                // :344-354
    float       set_fade_out_delay(unit &u, float delay);                               // :356-366
    float       set_rms_length(unit &u, float length);                                  // :368-379
    // :153-252 and :254-270 without the sum: NULL, or why the reference's process() would leave its defined behaviour with
    // these settings (the bank refuses them).  *designed (may be NULL): whether the designed fields were written -- they are, as
    // the reference writes them, wherever its conversions are defined, also for settings that are then refused.
    const char *reconfigure(unit &u, bool *designed = nullptr);
    float       crossfade(const fade_t &f, float x);                                    // :381-420
    void        tabulate(const fade_t &f, std::vector<float> &table);                   // crossfade(f, x), x = 0 .. nSamples - 1
    // the smallest q >= 0 with sqrtf(q) >= thresh, so that  sqrtf(q) < thresh  is  q < square_threshold(thresh)  for every
    // q >= 0 and for NaN
    float       square_threshold(float thresh);
} // namespace mi_depopper
