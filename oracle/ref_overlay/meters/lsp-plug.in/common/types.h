// Ahead of oracle/ref_overlay/filters' and oracle/ref_shim's <lsp-plug.in/common/types.h> for oracle/_ref/loudness_ref only: what
// LoudnessMeter.cpp and ILUFSMeter.cpp take from lsp-common-lib beside those.  All of it is OURS, written from the call sites;
// what is a choice of this stand-in says UNPINNED.
//   LoudnessMeter.cpp:472, :525      lsp_min(size_t, size_t, size_t)
//   ILUFSMeter.cpp:363               lsp_min(size_t, uint32_t, size_t): UNPINNED, the result has the type of the first argument
//                                    (every value there is below 2^32, so no candidate type changes the result)
//   LoudnessMeter.cpp:297            fixed_int(size_t): the value in a fixed-width integer type, for round_pow2()'s overloads
#ifndef ORACLE_REF_OVERLAY_METERS_TYPES_H_
#define ORACLE_REF_OVERLAY_METERS_TYPES_H_

#include_next <lsp-plug.in/common/types.h>

namespace lsp
{
    template <class A, class B, class C> inline A lsp_min(A a, B b, C c)
    {
        A r = (a < A(b)) ? a : A(b);
        return (r < A(c)) ? r : A(c);
    }

    inline uint64_t fixed_int(size_t v)     { return uint64_t(v); }
}

#endif
