// lsp::dspu::ScaledMeterGraph's bookkeeping, shared by the bank (scaled_metergraph.hip) and the class
// (host/scaled_metergraph_class.cpp): the folds of its two samplers as src/main/util/ScaledMeterGraph.cpp writes them, and
// update_period() (:269-342) as a closed form.
//
// How one process(s, n) call of a sampler is cut into chunks (:147-206) is MeterGraph's cut: mi_metergraph::make_plan serves both
// samplers as it is.  Its `pre` is never set here: a sampler leaves nCount >= nPeriod nowhere (:140-144, :200-204 zero it, the
// re-decimation leaves less than the history's period, which is no more than any frame period, :95), so nCount < nPeriod holds
// at every entry and nCount == nPeriod does not occur.
#pragma once
#include "metergraph_bank.h"

namespace mi_scaled_metergraph
{
    using mi_metergraph::is_abs;
    using mi_metergraph::is_max;

    constexpr uint32_t FRAMES_GAP = 0x10;                       // :30: both rings are this much longer than what is read of them

    // A chunk's value into a frame that is open (nCount != 0), block forms :156-193 and :217-254.  MM_ABS_MAXIMUM folds with
    // fCurrent < sample (:189, :250): the natural sense, where MeterGraph's block forms have >.
    MI_MG_HD float fold_block(uint32_t method, float current, float sample)
    {
        switch (method)
        {
            case MI_MM_SIGN_MINIMUM:    return (fabsf(current) > fabsf(sample)) ? sample : current;     // :161, :222
            case MI_MM_SIGN_MAXIMUM:    return (fabsf(current) < fabsf(sample)) ? sample : current;     // :168, :229
            case MI_MM_ABS_MINIMUM:     return (current > sample) ? sample : current;                   // :175, :236
            case MI_MM_PEAK:            return current;                                                 // :181, :242
            default:                    return (current < sample) ? sample : current;                   // :189, :250
        }
    }

    // process_sampler(sampler, sample), :103-145: fCurrent after the sample; *pushed is what goes to the ring where the frame
    // closes: the SAMPLE (:142), after fabsf for the two ABS methods (:119, :131), not fCurrent.  Kept.
    MI_MG_HD float fold_single(uint32_t method, float current, uint32_t count, float sample, float *pushed)
    {
        *pushed = is_abs(method) ? fabsf(sample) : sample;
        return (count == 0) ? mi_metergraph::first_single(method, sample) : mi_metergraph::fold_single(method, current, sample);
    }

    // One sub-sample into the frame that update_period() is folding, :298-328.  "Unset" is fCurrent < 0.0f: a negative winner of
    // a SIGN method counts as unset and the next sub-sample replaces it; a NaN never compares and stays.  MM_PEAK has no case of
    // its own and runs as MM_ABS_MAXIMUM (:320).
    //     SIGN_MINIMUM  (fCurrent < 0 || fabsf(fCurrent) > fabsf(sub)) ? sub : fCurrent                :302
    //     SIGN_MAXIMUM  (fCurrent < 0 || fabsf(fCurrent) < fabsf(sub)) ? sub : fCurrent                :308
    //     ABS_MINIMUM   (fCurrent < 0 || fCurrent > fabsf(sub)) ? fabsf(sub) : fCurrent                :314-316
    //     otherwise     (fCurrent < 0 || fCurrent < fabsf(sub)) ? fabsf(sub) : fCurrent                :323-325
    // Written with selects, not as a switch over the four lines: inside redecimated()'s loop the gfx950 code that ROCm 7.2 made
    // of the switch took the SIGNED sub-sample as the default case's candidate for methods above 3 (MM_PEAK), which
    // tests/test_scaled_metergraph_gpu.py's recorded MM_PEAK cases show.
    MI_MG_HD float fold_sub(uint32_t method, float current, float sub)
    {
        const bool sign = method == MI_MM_SIGN_MAXIMUM || method == MI_MM_SIGN_MINIMUM;
        const float mag = fabsf(sub);
        const float held = sign ? fabsf(current) : current;
        const bool wins = is_max(method) ? (held < mag) : (held > mag);
        return (current < 0.0f || wins) ? (sign ? sub : mag) : current;
    }

    // The re-decimation of :287-339 for a frame period P, `frames` frames and a history period hp, 1 <= hp <= P and
    // frames * P < 2^32.  Sub-sample i (1-based, oldest first) is sHistory.sBuffer.read(subsamples - i + 1); after it nCount has
    // grown by hp, and a frame is pushed where floor(i * hp / P) grows.  With hp <= P it grows by one at most: frame k (0-based)
    // closes behind sub-sample ceil((k + 1) * P / hp), the last one behind sub-sample `subsamples`, so exactly `frames` frames
    // are pushed, fCurrent is -1.0f again behind the last, and nCount is what is left over, below hp.
    MI_MG_HD uint32_t subsamples(uint32_t P, uint32_t frames, uint32_t hp)
    {
        return uint32_t((uint64_t(P) * frames + hp - 1) / hp);                                          // :288-289
    }
    // the sub-samples of frame k: first .. last, 1-based and inclusive
    MI_MG_HD uint32_t group_last(uint32_t k, uint32_t P, uint32_t hp)
    {
        return uint32_t((uint64_t(k + 1) * P + hp - 1) / hp);
    }
    MI_MG_HD uint32_t group_first(uint32_t k, uint32_t P, uint32_t hp)
    {
        return (k == 0) ? 1u : group_last(k - 1, P, hp) + 1u;
    }
    MI_MG_HD uint32_t leftover(uint32_t P, uint32_t frames, uint32_t hp)
    {
        return uint32_t(uint64_t(subsamples(P, frames, hp)) * hp - uint64_t(P) * frames);
    }

    // set_period(), :95: lsp_limit(uint32_t(period), sHistory.nPeriod, nMaxPeriod)
    MI_MG_HD uint32_t limit_period(size_t period, uint32_t hp, uint32_t max_period)
    {
        const uint32_t p = uint32_t(period);
        return (p < hp) ? hp : (p > max_period) ? max_period : p;
    }
} // namespace mi_scaled_metergraph
