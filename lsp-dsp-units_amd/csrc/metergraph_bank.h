// lsp::dspu::MeterGraph's bookkeeping, shared by the bank (metergraph.hip) and the class (host/metergraph_class.cpp): how one
// process(s, n) call is cut into chunks (src/main/util/MeterGraph.cpp:113-178), as a closed form of nCount, nPeriod and n, and
// the folds of one chunk's value into fCurrent, written once for the host and the device.
#pragma once
#include "mi_dspu.h"

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MI_MG_HD __host__ __device__ __forceinline__
#else
#define MI_MG_HD inline
#endif

namespace mi_metergraph
{
    // One call of n samples (n < 2^31) on a sampler with `count` samples in its open frame:
    //   pre           1: nCount == nPeriod on entry, so can_do is 0 and a frame is appended before any sample is read (:118, :171)
    //   first_len     the first chunk, lsp_min(n, nPeriod - nCount) in uint32_t arithmetic (:118): with nCount > nPeriod the
    //                 difference wraps and the whole call is this one chunk; it folds into fCurrent where the frame is open
    //   first_frame   1: the first chunk closes its frame
    //   full, tail    what follows from nCount == 0: `full` whole periods, then `tail` samples that open a frame
    //   frames        appended in all;  count_after: nCount when the call returns
    struct plan { uint32_t pre, first_len, first_frame, full, tail, frames, count_after; };

    MI_MG_HD plan make_plan(uint32_t count, uint32_t period, uint32_t n)
    {
        plan p = { 0, 0, 0, 0, 0, 0, count };
        if (n == 0 || period == 0)                              // while (n > 0), :115; a period of 0 never gets here
            return p;
        if (count == period)
            p.pre = 1, count = 0;
        const uint32_t room = period - count;                   // uint32_t, :118
        p.first_len = (n < room) ? n : room;
        count += p.first_len;                                   // :165
        if (count >= period)                                    // :171
            p.first_frame = 1, count = 0;
        const uint32_t rest = n - p.first_len;                  // != 0 only behind a closed frame
        p.full = rest / period, p.tail = rest % period;
        p.frames = p.pre + p.first_frame + p.full;
        p.count_after = (rest != 0) ? p.tail : count;
        return p;
    }

    MI_MG_HD bool is_abs(uint32_t method)   { return method != MI_MM_SIGN_MAXIMUM && method != MI_MM_SIGN_MINIMUM && method != MI_MM_PEAK; }
    MI_MG_HD bool is_max(uint32_t method)   { return method != MI_MM_ABS_MINIMUM && method != MI_MM_SIGN_MINIMUM; }

    // A chunk's value into a frame that is open (nCount != 0), block forms :126-161 and :193-227.  MM_ABS_MAXIMUM folds with
    // fCurrent > sample (:158, :224) where the single-sample form has < (:99): a frame that starts in one call and ends in
    // another holds the SMALLER of the two partial maxima.  Kept.
    MI_MG_HD float fold_block(uint32_t method, float current, float sample)
    {
        switch (method)
        {
            case MI_MM_SIGN_MINIMUM:    return (fabsf(current) > fabsf(sample)) ? sample : current;     // :129, :196
            case MI_MM_SIGN_MAXIMUM:    return (fabsf(current) < fabsf(sample)) ? sample : current;     // :136, :203
            case MI_MM_ABS_MINIMUM:     return (current > sample) ? sample : current;                   // :143, :210
            case MI_MM_PEAK:            return current;                                                 // :149, :216
            default:                    return (current > sample) ? sample : current;                   // :158, :224
        }
    }

    // process(float sample), :70-102, on an open frame (nCount != 0)
    MI_MG_HD float fold_single(uint32_t method, float current, float sample)
    {
        switch (method)
        {
            case MI_MM_SIGN_MINIMUM:    return (fabsf(current) > fabsf(sample)) ? sample : current;     // :76
            case MI_MM_SIGN_MAXIMUM:    return (fabsf(current) < fabsf(sample)) ? sample : current;     // :81
            case MI_MM_ABS_MINIMUM:     return (current > fabsf(sample)) ? fabsf(sample) : current;     // :86-88
            case MI_MM_PEAK:            return current;                                                 // :92
            default:                    return (current < fabsf(sample)) ? fabsf(sample) : current;     // :98-100
        }
    }
    // ... and what a sample is where it opens the frame (nCount == 0)
    MI_MG_HD float first_single(uint32_t method, float sample)
    {
        return is_abs(method) ? fabsf(sample) : sample;
    }
} // namespace mi_metergraph
