// What the Sidechain class (host/sidechain.cpp) needs of its bank (sidechain.hip) beyond the C-ABI.
#pragma once
#include "mi_common.h"

namespace mi
{
    // The parameters of one channel, set as they stand: the Sidechain class hands over its own nReactivity, fTau, nMode, nSource,
    // nFlags & SCF_MIDSIDE, fGain and its ring's capacity, so that the device runs exactly what its fields say.  Nothing stays
    // pending for the channel.  A capacity other than the channel's re-makes its ring (zeroed, position 0).
    int         sidechain_bank_set_params(mi_sidechain_bank_t *bank, uint32_t channel, const mi_sidechain_params_t *params);
    // ... fRmsValue, nRefresh and the ring position of one channel, for an object whose fields were written; zero_ring: the
    // ring's samples as well (update_settings() with SCF_CLEAR).  Runs the bank's pending work first.
    int         sidechain_bank_set_state(mi_sidechain_bank_t *bank, uint32_t channel, float rms_value, uint32_t refresh, uint32_t position,
                                         bool zero_ring, hipStream_t st);
}
