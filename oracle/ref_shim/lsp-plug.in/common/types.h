// STAND-IN for lsp-common-lib's <lsp-plug.in/common/types.h>, which the reference tree does not carry.  Only what the four
// dynamics classes and their headers take from it: the fixed-width types, the export markers, and lsp_max / lsp_min /
// lsp_limit.  Used by oracle/Makefile to compile the reference's own class sources into oracle/_ref/; never by the product.
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
}

#endif
