// STAND-IN for lsp-common-lib's <lsp-plug.in/common/alloc.h>, written from Limiter.cpp's two call sites (:79, :94): one block
// for the whole object, the aligned pointer returned typed and the block's own address kept in `ptr` for free_aligned().
#ifndef ORACLE_REF_SHIM_COMMON_ALLOC_H_
#define ORACLE_REF_SHIM_COMMON_ALLOC_H_

#include <cstdlib>
#include <lsp-plug.in/common/types.h>

namespace lsp
{
    static const size_t DEFAULT_ALIGN = 0x40;

    template <class T, class P> inline T *alloc_aligned(P * &ptr, size_t count, size_t align = DEFAULT_ALIGN)
    {
        // exactly count items past the aligned address: a sanitizer sees the first float outside what the caller asked for
        void *p = NULL;
        if (posix_memalign(&p, align, count * sizeof(T)) != 0)
            return NULL;
        ptr = static_cast<P *>(p);
        return static_cast<T *>(p);
    }

    template <class P> inline void free_aligned(P * &ptr)
    {
        free(ptr);
        ptr = NULL;
    }
}

#endif
