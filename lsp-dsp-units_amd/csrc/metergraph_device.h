// The sampler of the meter graphs on the device: one chunk of a row reduced by dsp::abs_max, abs_min, sign_max or sign_min.
//
// Our definition of the four (lsp-dsp-lib's generic ones): the result starts as the first element (its fabsf for
// the abs_* pair), every later element replaces it only where its magnitude is STRICTLY larger (smaller), the sign_* pair returns
// the signed element.  So the first of equal magnitudes wins, a NaN in first place is the result (no compare with it holds), and
// a NaN anywhere else is ignored.
//
// That is a reduction over (magnitude, index): associative, so lanes, waves and workgroups can share a chunk.  An element becomes
// a 64-bit key whose maximum is the winner:
//     high word   the magnitude's bits (monotonic for what is not a NaN; +0 == -0), inverted for the min pair;
//                 a NaN in first place gets the word that beats every other, a NaN elsewhere the one that loses to every other
//                 (it can tie with a first element only, which wins by its index)
//     low word    the index in the chunk, inverted: of equal magnitudes the earlier one wins
// The winner's index comes back and the value is read again from the row.  No key is 0 (an index is below 2^31).
#pragma once
#include "metergraph_bank.h"

namespace mi_metergraph
{
    typedef unsigned long long mkey;

    template <bool MAX> __device__ __forceinline__ mkey element_key(float x, uint32_t rel)
    {
        uint32_t mag = __float_as_uint(x) & 0x7fffffffu;
        if (mag > 0x7f800000u)                                  // NaN
            mag = ((rel == 0) == MAX) ? 0xffffffffu : 0u;
        const uint32_t high = MAX ? mag : ~mag;
        return (mkey(high) << 32) | mkey(~rel);
    }

    __device__ __forceinline__ mkey better(mkey a, mkey b)   { return (a > b) ? a : b; }

    // The keys of xs[0 .. len) that lane l of nl takes: single words up to the 16-byte grid, then 16 bytes at a time, then the rest.
    template <bool MAX> __device__ __forceinline__ mkey span_key(const float *xs, uint32_t len, uint32_t l, uint32_t nl)
    {
        mkey best = 0;
        uint32_t head = (4u - (uint32_t(reinterpret_cast<uintptr_t>(xs) >> 2) & 3u)) & 3u;
        head = (head < len) ? head : len;
        for (uint32_t i = l; i < head; i += nl)
            best = better(best, element_key<MAX>(xs[i], i));
        const uint32_t quads = (len - head) >> 2;
        const float4 *q = reinterpret_cast<const float4 *>(xs + head);
        for (uint32_t j = l; j < quads; j += nl)
        {
            const float4 v = q[j];
            const uint32_t i = head + 4u * j;
            best = better(best, element_key<MAX>(v.x, i));
            best = better(best, element_key<MAX>(v.y, i + 1));
            best = better(best, element_key<MAX>(v.z, i + 2));
            best = better(best, element_key<MAX>(v.w, i + 3));
        }
        for (uint32_t i = head + 4u * quads + l; i < len; i += nl)
            best = better(best, element_key<MAX>(xs[i], i));
        return best;
    }

    // the best key of a wave in every lane
    __device__ __forceinline__ mkey wave_best(mkey k)
    {
        #pragma unroll
        for (int d = 32; d >= 1; d >>= 1)
        {
            const uint32_t lo = __shfl_xor(uint32_t(k), d, 64), hi = __shfl_xor(uint32_t(k >> 32), d, 64);
            k = better(k, (mkey(hi) << 32) | lo);
        }
        return k;
    }

    // the best key of an aligned group of `group` lanes (a power of two up to 64) in each of them
    __device__ __forceinline__ mkey group_best(mkey k, uint32_t group)
    {
        for (uint32_t d = group >> 1; d >= 1; d >>= 1)
        {
            const uint32_t lo = __shfl_xor(uint32_t(k), int(d), 64), hi = __shfl_xor(uint32_t(k >> 32), int(d), 64);
            k = better(k, (mkey(hi) << 32) | lo);
        }
        return k;
    }

    // the chunk's value from the winner's index: fabsf for the abs_* pair, then the gain where the call has one (:195-223)
    __device__ __forceinline__ float chunk_value(const float *xs, uint32_t rel, uint32_t method, bool has_gain, float gain)
    {
        const float x = xs[rel];
        const float v = is_abs(method) ? fabsf(x) : x;
        return has_gain ? v * gain : v;
    }

    // one chunk by the lanes l of nl that share it (MM_PEAK takes s[0]: no reduction)
    __device__ __forceinline__ mkey chunk_key(const float *xs, uint32_t len, uint32_t method, uint32_t l, uint32_t nl)
    {
        if (method == MI_MM_PEAK)
            return element_key<true>(0.0f, 0);
        return is_max(method) ? span_key<true>(xs, len, l, nl) : span_key<false>(xs, len, l, nl);
    }

    __device__ __forceinline__ uint32_t key_index(mkey k)      { return ~uint32_t(k); }
} // namespace mi_metergraph
