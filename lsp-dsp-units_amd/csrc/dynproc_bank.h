// What the DynamicProcessor class (host/dynproc.cpp) needs of its bank (dynproc.hip) beyond the C-ABI.
#pragma once
#include "mi_common.h"

namespace mi
{
    // The computed parameters of one channel of a dynamic processor bank, set as they stand: the DynamicProcessor class hands
    // over its own fCount, nHold, vAttack, vRelease and vSplines, so that the device runs exactly what its fields say.
    int         dynproc_bank_set_params(mi_dynproc_bank_t *bank, uint32_t channel, const mi_dynproc_params_t *params);
    // ... and the follower's state of one channel (fEnvelope, fPeak, nHoldCounter), for an object whose fields were written.
    int         dynproc_bank_set_state(mi_dynproc_bank_t *bank, uint32_t channel, float envelope, float peak, uint32_t hold,
                                       hipStream_t st);
}
