// Ahead of oracle/ref_shim's <lsp-plug.in/common/types.h> for oracle/_ref/truepeak_ref only: lsp_max of three and four values
// (TruePeakMeter.cpp:124-146), nested from the left.  The values there are magnitudes, so the nesting changes no bit.
#ifndef ORACLE_REF_OVERLAY_RESAMPLER_TYPES_H_
#define ORACLE_REF_OVERLAY_RESAMPLER_TYPES_H_

#include_next <lsp-plug.in/common/types.h>

namespace lsp
{
    template <class T> inline T lsp_max(T a, T b, T c)          { return lsp_max(lsp_max(a, b), c); }
    template <class T> inline T lsp_max(T a, T b, T c, T d)     { return lsp_max(lsp_max(lsp_max(a, b), c), d); }
}

#endif
