// What the Compressor class (host/compressor.cpp) needs of its bank (compressor.hip) beyond the C-ABI.
#pragma once
#include "mi_common.h"

namespace mi
{
    // The computed parameters of one channel of a compressor bank, set as they stand: the Compressor class hands over its
    // own fTau*, fReleaseThresh, nHold and sComp, so that the device runs exactly what its fields say.
    int         compressor_bank_set_params(mi_compressor_bank_t *bank, uint32_t channel, const mi_compressor_params_t *params);
    // ... and the follower's state of one channel (fEnvelope, fPeak, nHoldCounter), for an object whose fields were written.
    int         compressor_bank_set_state(mi_compressor_bank_t *bank, uint32_t channel, float envelope, float peak, uint32_t hold,
                                          hipStream_t st);
}
