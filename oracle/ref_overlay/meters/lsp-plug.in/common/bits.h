// Ahead of oracle/ref_shim's <lsp-plug.in/common/bits.h> for oracle/_ref/loudness_ref only.  OURS, from the call site.
//   LoudnessMeter.cpp:297            round_pow2(n): the ring's length, used as a mask + 1 (:386, :414) -- the smallest power of two
//                                    that is not below n
#ifndef ORACLE_REF_OVERLAY_METERS_BITS_H_
#define ORACLE_REF_OVERLAY_METERS_BITS_H_

#include_next <lsp-plug.in/common/bits.h>

namespace lsp
{
    inline uint64_t round_pow2(uint64_t v)
    {
        uint64_t p = 1;
        while (p < v)
            p <<= 1;
        return p;
    }
}

#endif
