// STAND-IN for lsp-common-lib's <lsp-plug.in/common/status.h>: the status type alone.
#ifndef ORACLE_REF_SHIM_COMMON_STATUS_H_
#define ORACLE_REF_SHIM_COMMON_STATUS_H_

namespace lsp
{
    typedef int status_t;
    enum { STATUS_OK = 0 };
}

#endif
