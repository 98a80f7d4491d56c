// What the Gate class (host/gate.cpp) needs of its bank (gate.hip) beyond the C-ABI.
#pragma once
#include "mi_common.h"

namespace mi
{
    // The computed parameters of one channel of a gate bank, set as they stand: the Gate class hands over its own fTau*,
    // nHold and the two sKnee, so that the device runs exactly what its fields say.
    int         gate_bank_set_params(mi_gate_bank_t *bank, uint32_t channel, const mi_gate_params_t *params);
    // ... and the state of one channel (fEnvelope, fPeak, nHoldCounter, nCurve), for an object whose fields were written.
    int         gate_bank_set_state(mi_gate_bank_t *bank, uint32_t channel, float envelope, float peak, uint32_t hold,
                                    uint32_t curve, hipStream_t st);
}
