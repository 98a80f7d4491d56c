// STAND-IN for lsp-common-lib's <lsp-plug.in/stdlib/stdio.h>: the C library's <cstdio>; Limiter.cpp uses it in comments only.
#ifndef ORACLE_REF_SHIM_STDLIB_STDIO_H_
#define ORACLE_REF_SHIM_STDLIB_STDIO_H_

#include <cstdio>

#endif
