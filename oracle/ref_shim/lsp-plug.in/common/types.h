// STAND-IN for lsp-common-lib's <lsp-plug.in/common/types.h>, which the reference tree does not carry.  Only what the seven
// dynamics classes and their headers take from it: the fixed-width types, the export markers, lsp_max / lsp_min /
// lsp_limit and lsp_setflag.  Used by oracle/Makefile to compile the reference's own class sources into oracle/_ref/; never
// by the product.
#ifndef ORACLE_REF_SHIM_COMMON_TYPES_H_
#define ORACLE_REF_SHIM_COMMON_TYPES_H_

#include <cstddef>
#include <cstdint>
#include <sys/types.h>

#define LSP_EXPORT_MODIFIER
#define LSP_IMPORT_MODIFIER

namespace lsp
{
    typedef uint32_t lsp_wchar_t;

    template <class T> inline T lsp_max(T a, T b)           { return (a > b) ? a : b; }
    template <class T> inline T lsp_min(T a, T b)           { return (a < b) ? a : b; }
    template <class T> inline T lsp_limit(T x, T lo, T hi)  { return (x < lo) ? lo : ((x > hi) ? hi : x); }

    // Limiter.cpp:283-284, lsp_limit(ssize_t, int, ssize_t): the limits taken to the type of the value.  Which limit wins
    // where hi < lo is this stand-in's choice (lo first, as above); no recorded case has a look-ahead under 8 samples.
    template <class T, class L, class H> inline T lsp_limit(T x, L lo, H hi)   { return lsp_limit<T>(x, T(lo), T(hi)); }

    // AutoGain.cpp:142, :152, :177: lsp_setflag(nFlags, F_..., enable) -> the new nFlags
    template <class T, class F> inline T lsp_setflag(T flags, F flag, bool set)    { return (set) ? T(flags | T(flag)) : T(flags & ~T(flag)); }
}

#endif
