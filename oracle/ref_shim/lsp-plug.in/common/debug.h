// STAND-IN for lsp-common-lib's <lsp-plug.in/common/debug.h>: the log macros, empty.
#ifndef ORACLE_REF_SHIM_COMMON_DEBUG_H_
#define ORACLE_REF_SHIM_COMMON_DEBUG_H_

#define lsp_trace(...)  do {} while (0)
#define lsp_warn(...)   do {} while (0)
#define lsp_error(...)  do {} while (0)

#endif
