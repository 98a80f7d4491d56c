// Ahead of oracle/ref_shim's <lsp-plug.in/common/alloc.h> for oracle/_ref/loudness_ref only.  OURS, from the call sites.
//   LoudnessMeter.cpp:108-127, ILUFSMeter.cpp:137-138    advance_ptr_bytes<T>(ptr, bytes): the pointer as T *, then moved on
//   LoudnessMeter.cpp:303, ILUFSMeter.cpp:303            realloc_aligned<T>(ptr, count, align): a new aligned block (the callers
//                                                        clear it: nothing of the old one is kept), the old one freed
// UNPINNED: DEFAULT_ALIGN itself (oracle/ref_shim: 0x40).  ILUFSMeter.cpp:299 rounds the gating-block history to it, so it decides
// nMSSize; it belongs to lsp-common-lib, which the reference tree does not carry.
#ifndef ORACLE_REF_OVERLAY_METERS_ALLOC_H_
#define ORACLE_REF_OVERLAY_METERS_ALLOC_H_

#include_next <lsp-plug.in/common/alloc.h>

namespace lsp
{
    template <class T, class P> inline T *advance_ptr_bytes(P * &ptr, size_t bytes)
    {
        T *res = reinterpret_cast<T *>(ptr);
        ptr = reinterpret_cast<P *>(reinterpret_cast<uint8_t *>(ptr) + bytes);
        return res;
    }

    template <class T, class P> inline T *realloc_aligned(P * &ptr, size_t count, size_t align = DEFAULT_ALIGN)
    {
        P *old = ptr;
        T *res = alloc_aligned<T>(ptr, count, align);
        if (res == NULL)
        {
            ptr = old;
            return NULL;
        }
        free(old);
        return res;
    }
}

#endif
