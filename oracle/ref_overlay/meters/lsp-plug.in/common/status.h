// Ahead of oracle/ref_shim's <lsp-plug.in/common/status.h> for oracle/_ref/loudness_ref only: the code both meters return for a
// channel index out of range (LoudnessMeter.cpp:187, ILUFSMeter.cpp:218).  Only compared symbolically; the number is OURS.
#ifndef ORACLE_REF_OVERLAY_METERS_STATUS_H_
#define ORACLE_REF_OVERLAY_METERS_STATUS_H_

#include_next <lsp-plug.in/common/status.h>

namespace lsp
{
    enum { STATUS_OVERFLOW = 18 };
}

#endif
