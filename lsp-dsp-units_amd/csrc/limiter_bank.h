// What limiter.hip (the bank) and host/limiter.cpp (parameters, the patch table, the Limiter class) need of each other
// beyond the C-ABI.
#pragma once
#include "mi_common.h"

namespace mi
{
    // Limiter::update_settings with init_sat / init_exp / init_line, and the patch as a table of p.release entries
    void        limiter_compute_params(const mi_limiter_settings_t &s, mi_limiter_params_t &p);
    void        limiter_compute_patch(const mi_limiter_params_t &p, float *shape);

    // entries a channel's table may take: attack <= max(8, ML), release <= max(8, 2 ML), one more
    inline uint32_t limiter_patch_capacity(uint32_t max_lookahead) { return 3u * max_lookahead + 17u; }
}
