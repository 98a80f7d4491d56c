// What the classes AutoGain and SimpleAutoGain (host/autogain.cpp) need of their banks (autogain.hip) beyond the C-ABI.
#pragma once
#include "mi_common.h"

namespace mi
{
    // The parameters and the state of one channel set as they stand: the classes hand over their own fields, so that the
    // device runs exactly what they say.
    int         autogain_bank_set_params(mi_autogain_bank_t *bank, uint32_t channel, const mi_autogain_params_t *params);
    int         autogain_bank_set_state(mi_autogain_bank_t *bank, uint32_t channel, float curr_gain, float out_gain, uint32_t surge,
                                        hipStream_t st);
    int         simple_autogain_bank_set_params(mi_simple_autogain_bank_t *bank, uint32_t channel,
                                                const mi_simple_autogain_params_t *params);
    // ... the gain as it stands: changes of the limits recorded for the channel before are dropped
    int         simple_autogain_bank_set_state(mi_simple_autogain_bank_t *bank, uint32_t channel, float curr_gain, hipStream_t st);
}
