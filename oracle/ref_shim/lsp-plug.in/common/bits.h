// STAND-IN for lsp-common-lib's <lsp-plug.in/common/bits.h>: AutoGain.cpp and SimpleAutoGain.cpp include it and use nothing
// of it.
#ifndef ORACLE_REF_SHIM_COMMON_BITS_H_
#define ORACLE_REF_SHIM_COMMON_BITS_H_

#include <lsp-plug.in/common/types.h>

#endif
