// Ahead of oracle/ref_shim's <lsp-plug.in/common/types.h> for oracle/_ref/filter_ref and dynfilter_ref only: what Filter.cpp,
// FilterBank.cpp and DynamicFilters.cpp take from lsp-common-lib beside that.  All of it is OURS, written from the call sites;
// what is a choice of this stand-in says UNPINNED.
//   FilterBank.cpp:68, Filter.cpp:99     align_size(size, align): the size rounded up to a multiple of the alignment
//   Filter.cpp:106                       align_ptr(ptr, align): the pointer rounded up likewise
//   Filter.cpp:503, :603                 __lsp_aligned32 on a stack buffer
//   Filter.cpp:517.. lsp_min(size_t, unsigned): UNPINNED, the result has the type of the first argument
//   DynamicFilters.cpp                   STATUS_NO_MEM (only compared symbolically)
#ifndef ORACLE_REF_OVERLAY_FILTERS_TYPES_H_
#define ORACLE_REF_OVERLAY_FILTERS_TYPES_H_

#include_next <lsp-plug.in/common/types.h>

#define __lsp_aligned32         __attribute__((aligned(32)))

namespace lsp
{
    enum { STATUS_NO_MEM = 5 };

    template <class A, class B> inline A lsp_max(A a, B b)      { return (a > A(b)) ? a : A(b); }
    template <class A, class B> inline A lsp_min(A a, B b)      { return (a < A(b)) ? a : A(b); }

    inline size_t align_size(size_t size, size_t align)
    {
        size_t off = size % align;
        return (off == 0) ? size : size + align - off;
    }

    template <class T> inline T *align_ptr(T *ptr, size_t align)
    {
        uintptr_t p = uintptr_t(ptr), off = p % align;
        return reinterpret_cast<T *>((off == 0) ? p : p + align - off);
    }
}

#endif
