// What the Expander class (host/expander.cpp) needs of its bank (expander.hip) beyond the C-ABI.
#pragma once
#include "mi_common.h"

namespace mi
{
    // The computed parameters of one channel of an expander bank, set as they stand: the Expander class hands over its own
    // fTau*, fReleaseThresh, nHold, sExp and bUpward, so that the device runs exactly what its fields say.
    int         expander_bank_set_params(mi_expander_bank_t *bank, uint32_t channel, const mi_expander_params_t *params);
    // ... and the follower's state of one channel (fEnvelope, fPeak, nHoldCounter), for an object whose fields were written.
    int         expander_bank_set_state(mi_expander_bank_t *bank, uint32_t channel, float envelope, float peak, uint32_t hold,
                                        hipStream_t st);
}
