// Ahead of oracle/ref_shim's <lsp-plug.in/common/types.h> for oracle/_ref/sidechain_ref only: the forms of lsp_max / lsp_min
// that Sidechain.cpp takes beside those.  :92 lsp_max(float, int), :127 lsp_max(ssize_t, int) and :462 lsp_min of three: the
// result has the type of the first argument.  That choice is this stand-in's (UNPINNED): at :92 it makes the ring's capacity
// size_t(max(samples, 1.0f) + 512.0f).
#ifndef ORACLE_REF_OVERLAY_SIDECHAIN_TYPES_H_
#define ORACLE_REF_OVERLAY_SIDECHAIN_TYPES_H_

#include_next <lsp-plug.in/common/types.h>

namespace lsp
{
    template <class A, class B> inline A lsp_max(A a, B b)                  { return (a > A(b)) ? a : A(b); }
    template <class A, class B> inline A lsp_min(A a, B b)                  { return (a < A(b)) ? a : A(b); }
    template <class A, class B, class C> inline A lsp_min(A a, B b, C c)    { return lsp_min(lsp_min(a, A(b)), A(c)); }
}

#endif
