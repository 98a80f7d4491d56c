// Between autogain.hip (the kernels and their launches) and host/autogain.cpp (the two banks' host side and the classes
// AutoGain and SimpleAutoGain): what lives in device memory, the launches, and what the classes need beyond the C-ABI.
#pragma once
#include "mi_common.h"

namespace mi
{
    // AutoGain: fCurrGain, fOutGain and the surge flags (MI_AG_SURGE_UP | MI_AG_SURGE_DOWN) of one channel between calls
    struct autogain_state { float gain, out; uint32_t surge, pad; };

    // SimpleAutoGain: a recorded change of the gain limits, to be applied to fCurrGain ...
    enum { SAG_MIN = 1, SAG_MAX = 2, SAG_LIMIT = 3 };          // lsp_min(g, hi), lsp_max(g, lo), lsp_limit(g, lo, hi)
    struct simple_autogain_op { uint32_t kind; float lo, hi; uint32_t pad; };
    // ... and where a channel's changes are in the table of them: ops[first .. first + count).  The launch that applies
    // them zeroes count.
    struct simple_autogain_pending { uint32_t first, count; };
    __host__ __device__ inline float simple_autogain_apply(float g, const simple_autogain_op &op)
    {
        switch (op.kind)
        {
            case SAG_MIN:   return (g < op.hi) ? g : op.hi;
            case SAG_MAX:   return (g > op.lo) ? g : op.lo;
            case SAG_LIMIT: return (g < op.lo) ? op.lo : (g > op.hi) ? op.hi : g;
            default:        return g;
        }
    }

    // vca (audio == NULL) or audio * vca.  lexp: rows, or with `level` one float per channel.  count > 0.
    int         autogain_launch(float *vca, const float *llong, const float *lshort, const float *lexp, bool level, const float *audio,
                                size_t vca_stride, size_t long_stride, size_t short_stride, size_t exp_stride, size_t audio_stride,
                                uint32_t count, uint32_t channels, const mi_autogain_params_t *params, autogain_state *state,
                                hipStream_t st);
    int         simple_autogain_launch(float *dst, const float *src, size_t dst_stride, size_t src_stride, uint32_t count,
                                       uint32_t channels, const mi_simple_autogain_params_t *params, float *gain,
                                       simple_autogain_pending *pending, const simple_autogain_op *ops, hipStream_t st);

    // The parameters and the state of one channel set as they stand: the classes hand over their own fields, so that the
    // device runs exactly what they say.
    int         autogain_bank_set_params(mi_autogain_bank_t *bank, uint32_t channel, const mi_autogain_params_t *params);
    int         autogain_bank_set_state(mi_autogain_bank_t *bank, uint32_t channel, float curr_gain, float out_gain, uint32_t surge,
                                        hipStream_t st);
    int         simple_autogain_bank_set_params(mi_simple_autogain_bank_t *bank, uint32_t channel,
                                                const mi_simple_autogain_params_t *params);
    int         simple_autogain_bank_set_state(mi_simple_autogain_bank_t *bank, uint32_t channel, float curr_gain, hipStream_t st);
}
