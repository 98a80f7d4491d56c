// What compressor.hip, expander.hip, gate.hip and dynproc.hip share on the device, beside the tile walk of
// tile_chain_device.h: the follower's state, the end of its step, and the step and the kernel of the banks whose walk is the
// plain one.
//
// All four kernels have the same shape: wave 0 follows the envelope in place in LDS, lane c on row c; the helper wave of a
// row turns its envelope into the gain, multiplies the audio in if there is any and stores.  follow_kernel is that shape
// written once, over a small description of the bank (the Compressor's and the Expander's, in their files).  The Gate (curve bits
// beside the tile) and the DynamicProcessor (the row's table through a wave-uniform pointer, read anew for every tile) need
// something in the walk that only they use, so they keep kernels of their own and share the small pieces: shared code does
// not ask which bank it serves.
#pragma once
#include "tile_chain_device.h"

#pragma clang fp contract(off)      // the follower's product and sum round on their own

// The end of one sample of the follower (Compressor.cpp:231-256, Expander.cpp:258-278, Gate.cpp:284-306,
// DynamicProcessor.cpp:406-427), the same in all four: the input fell (neg) or rose, and en is e + tau * (s - e) with the bank's
// choice of tau.  A MACRO, as the walk is: as a function of its own, simplified before it meets the bank's choice of tau, it
// gave compressor_follow_tile other instructions (244 -> 263 lines, or 254 with the compare inside); the same tokens in place
// give the same chain.
#define MI_FOLLOW_SETTLE(e, peak, hold, neg, en, nhold) \
    do { \
        const bool held_ = (neg) && (hold) > 0; \
        const bool rearm_ = !(neg) && (en) >= (peak); \
        (e) = held_ ? (e) : (en); \
        (peak) = (((neg) && !held_) || rearm_) ? (en) : (peak); \
        (hold) = held_ ? (hold) - 1 : rearm_ ? (nhold) : (hold); \
    } while (0)

namespace mi_dynamics
{
    using namespace mi_tile_chain;

    constexpr int CURVE_BLOCK = 256;

    enum { VEC_IN = 1, VEC_GAIN = 2, VEC_ENV = 4, VEC_AUDIO = 8 };      // which buffers have 16-byte aligned rows

    struct follow_state { float e, peak; uint32_t hold; };
    struct device_state { float e, peak; uint32_t hold, pad; };     // [channels] between calls

    // One sample of the Compressor's follower (Compressor.cpp:231-256), which the Expander's is statement for statement
    // (Expander.cpp:258-278): release takes tau release only above the release threshold
    __device__ __forceinline__ void follow_step(float s, float &e, float &peak, uint32_t &hold, float ta, float tr, float rt,
                                                uint32_t nhold)
    {
        const float d = s - e;
        const bool neg = d < 0.0f;
        const float tau = (neg && e > rt) ? tr : ta;
        const float en = e + tau * d;
        MI_FOLLOW_SETTLE(e, peak, hold, neg, en, nhold);
    }

    // Bank describes a bank with the Compressor's follower:
    //     params_t                         a channel's parameters: tau_attack, tau_release, release_threshold, hold, and the curve
    //     row, load(params_t)              what a helper holds of its row's curve
    //     gain(e, row)                     the gain for the envelope e
    //     follow(lds row, n, state, ta, tr, rt, nhold)     the bank's own __noinline__ follower over a tile
    // gain (audio == NULL) or dst = audio * gain into `gain`, the envelope into `env` unless NULL.  vec: VEC_*.
    template <class Bank>
    __global__ __launch_bounds__(BLOCK) void follow_kernel(float *gain, float *env, const float *in, const float *audio,
                                                           size_t gain_stride, size_t env_stride, size_t in_stride,
                                                           size_t audio_stride, uint32_t count, uint32_t channels,
                                                           const typename Bank::params_t *params, device_state *state,
                                                           uint32_t vec)
    {
        __shared__ __attribute__((aligned(16))) float tile[2][GROUP][ROW];
        const role me = my_role(channels);
        const uint32_t r = me.r, ch = me.ch, c = me.c;

        // the follower's lane: its channel's state and taus; a helper: its row's curve
        follow_state fs = { 0.0f, 0.0f, 0 };
        float ta = 0.0f, tr = 0.0f, rt = 0.0f;
        uint32_t nhold = 0;
        typename Bank::row curve = {};
        if (me.valid && me.chain)
        {
            const device_state s = state[ch];
            fs = follow_state{ s.e, s.peak, s.hold };
            ta = params[ch].tau_attack, tr = params[ch].tau_release, rt = params[ch].release_threshold, nhold = params[ch].hold;
        }
        else if (me.valid)
            curve = Bank::load(params[ch]);
        const float *xs = in + size_t(ch) * in_stride;
        const float *as = (audio != nullptr) ? audio + size_t(ch) * audio_stride : nullptr;
        float *gs = gain + size_t(ch) * gain_stride;
        float *es = (env != nullptr) ? env + size_t(ch) * env_stride : nullptr;

        auto load_tile = [&](uint32_t k)
        {
            const extent t = tile_extent(count, k);
            float *l = &tile[k & 1][r][c];
            if ((vec & VEC_IN) && c + 4 <= t.n)
                *reinterpret_cast<float4 *>(l) = *reinterpret_cast<const float4 *>(xs + t.t0 + c);
            else
            {
                #pragma unroll
                for (uint32_t j = 0; j < 4; ++j)
                    if (c + j < t.n)
                        l[j] = xs[t.t0 + c + j];
            }
        };
        auto emit_tile = [&](uint32_t k)
        {
            const extent t = tile_extent(count, k);
            if (c >= t.n)
                return;
            const float4 e4 = *reinterpret_cast<const float4 *>(&tile[k & 1][r][c]);
            const float e[4] = { e4.x, e4.y, e4.z, e4.w };
            float g[4];
            #pragma unroll
            for (uint32_t j = 0; j < 4; ++j)
                g[j] = (c + j < t.n) ? Bank::gain(e[j], curve) : 0.0f;
            if (as != nullptr)
            {
                float a[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
                if ((vec & VEC_AUDIO) && c + 4 <= t.n)
                {
                    const float4 a4 = *reinterpret_cast<const float4 *>(as + t.t0 + c);
                    a[0] = a4.x, a[1] = a4.y, a[2] = a4.z, a[3] = a4.w;
                }
                else
                {
                    #pragma unroll
                    for (uint32_t j = 0; j < 4; ++j)
                        if (c + j < t.n)
                            a[j] = as[t.t0 + c + j];
                }
                #pragma unroll
                for (uint32_t j = 0; j < 4; ++j)
                    g[j] = a[j] * g[j];
            }
            store_quad(gs + t.t0 + c, g, vec & VEC_GAIN, c, t.n);
            if (es != nullptr)
                store_quad(es + t.t0 + c, e, vec & VEC_ENV, c, t.n);
        };

        MI_TILE_CHAIN_WALK(me, count, k, load_tile(k),
                           fs = Bank::follow((lds_float *)&tile[k & 1][r][0], tile_extent(count, k).n, fs, ta, tr, rt, nhold),
                           emit_tile(k));
        if (me.valid && me.chain)
            state[ch] = device_state{ fs.e, fs.peak, fs.hold, 0 };
    }
} // namespace mi_dynamics
