// STAND-IN for lsp-common-lib's <lsp-plug.in/stdlib/math.h>: the C library's <cmath> and the constants it may leave out.
#ifndef ORACLE_REF_SHIM_STDLIB_MATH_H_
#define ORACLE_REF_SHIM_STDLIB_MATH_H_

#include <cmath>
#include <math.h>
#include <lsp-plug.in/common/types.h>

#ifndef M_SQRT1_2
    #define M_SQRT1_2   0.70710678118654752440
#endif
#ifndef M_PI
    #define M_PI        3.14159265358979323846
#endif

#endif
