// lsp::dspu::QuantizedCounter's bookkeeping, shared by the bank (quantized_counter.hip) and the class
// (host/quantized_counter_class.cpp): the bin of one sample (src/main/stat/QuantizedCounter.cpp:203, :218) and the closed form of
// one process(data, count) call (:242-266) -- what leaves the window, what of the new row stays in it and where the ring is
// written -- from nHead, nCount, nPeriod, nCapacity and count, written once for the host and the device.
#pragma once
#include "mi_dspu.h"

#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MI_QC_HD __host__ __device__ __forceinline__
#else
#define MI_QC_HD inline
#endif

namespace mi_qcounter
{
    constexpr size_t BUFFER_GAP = 0x400;                        // :30

    // nCapacity of init(max_period, max_levels), :74, :85: the ring in floats, its bytes rounded up to 64
    inline size_t capacity_of(size_t max_period)               { return (((max_period + BUFFER_GAP) * sizeof(float) + 63) & ~size_t(63)) / sizeof(float); }

    // fRStep, :169: one float32 division.  An empty range gives +-Inf (or NaN with nLevels == 0), a reversed one a negative step.
    inline float rstep_of(uint32_t levels, float min_value, float max_value)
    {
        volatile float range = max_value - min_value;           // rounded to float32 before the division, whatever the host's flags
        return float(levels) / range;
    }

    // (v - fMinValue) * fRStep with both roundings to float32 and nothing contracted
    MI_QC_HD float scaled(float v, float min_value, float rstep)
    {
#if defined(__HIP_DEVICE_COMPILE__)
        return __fmul_rn(__fsub_rn(v, min_value), rstep);
#else
        volatile float d = v - min_value;
        volatile float s = d * rstep;
        return s;
#endif
    }

    // The word of vCounters that a sample counts in: a bin below nLevels, nMaxLevels (below) or nMaxLevels + 1 (above).
    // `int32_t index = s` (:203) is undefined in C++ where s is a NaN or outside int32_t.  This is a DEFINITION, the one that the
    // reference's compiled class shows on x86-64 (cvttss2si answers INT_MIN there, which is < 0):
    //     NaN, s >= 2^31, s <= -1      below
    //     nLevels <= s < 2^31          above
    //     otherwise                    bin trunc(s): -1 < s < 0 truncates to bin 0, as the reference has it
    // Compares and selects only; levels <= 2^24, so float(levels) is exact.
    MI_QC_HD uint32_t bin_of(float s, uint32_t levels, uint32_t max_levels)
    {
        const bool below = !(s > -1.0f) || (s >= 2147483648.0f);
        const bool above = s >= float(levels);
        const float t = (below || above) ? 0.0f : s;            // what is converted lies in (-1, 2^24]
        const uint32_t bin = uint32_t(int32_t(t));
        return below ? max_levels : above ? max_levels + 1 : bin;
    }

    // One call of n samples (n < 2^31) on a ring of `capacity` words with its head at `head` and `count` samples behind it
    // (count <= capacity, period < capacity).  The window after the call is the last min(period, samples seen) samples, whatever n:
    //   tail          the ring position of the oldest sample held, (nHead + nCapacity - nCount) % nCapacity (:230)
    //   evict         how many of the oldest leave: those beyond the period before the call (nCount - C0, C0 = min(nCount, nPeriod):
    //                 a period that was reduced, :248) and max(0, C0 + n - nPeriod) capped at C0 (:261)
    //   remain        count - evict: the history samples that stay, from (tail + evict) % capacity on
    //   keep_from     the suffix [keep_from, n) of the row stays in the window: the last min(n, nPeriod); what comes before it
    //                 enters and leaves within the call and is never counted
    //   store_from    the row's samples [store_from, n) are written to the ring, sample i to (head + i) % capacity: of more than
    //                 `capacity` samples only the last `capacity` (the last stores win); store_pos is where sample store_from goes
    //   head_after, count_after
    struct plan { uint32_t tail, evict, remain, keep_from, store_from, store_pos, head_after, count_after; };

    MI_QC_HD plan make_plan(uint32_t head, uint32_t count, uint32_t period, uint32_t capacity, uint32_t n)
    {
        plan p;
        const uint32_t c0 = (count < period) ? count : period;
        const uint64_t over = uint64_t(c0) + n;                 // C0 + n
        const uint32_t late = (over > period) ? ((over - period < c0) ? uint32_t(over - period) : c0) : 0;
        p.tail = uint32_t((uint64_t(head) + capacity - count) % capacity);
        p.evict = (count - c0) + late;
        p.remain = count - p.evict;
        p.keep_from = (n > period) ? n - period : 0;
        p.store_from = (n > capacity) ? n - capacity : 0;
        p.store_pos = uint32_t((uint64_t(head) + p.store_from) % capacity);
        p.head_after = uint32_t((uint64_t(head) + n) % capacity);
        p.count_after = (over < period) ? uint32_t(over) : period;
        return p;
    }
} // namespace mi_qcounter
