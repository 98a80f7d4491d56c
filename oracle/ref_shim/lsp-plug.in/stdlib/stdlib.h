// STAND-IN for lsp-common-lib's <lsp-plug.in/stdlib/stdlib.h>: the C library's own (RawRingBuffer.cpp takes realloc and free).
#ifndef ORACLE_REF_SHIM_STDLIB_STDLIB_H_
#define ORACLE_REF_SHIM_STDLIB_STDLIB_H_

#include <cstdlib>
#include <stdlib.h>

#endif
