// lsp::dspu::SurgeProtector as a bank of `channels` protectors (src/main/dynamics/SurgeProtector.cpp): the output fades in when a
// signal appears and out when it stops.  Per sample (:99-149) the on/off decision comes first -- while on, a level at or above
// fOffThreshold zeroes nShutdownTime, anything else (NaN too) counts it up, and at nShutdownMax the protector goes off; while
// off, a level at or above fOnThreshold turns it on -- then the gain, from nTransitionTime BEFORE it moves towards
// nTransitionMax (on) or 0 (off).
//
// While nTransitionTime <= nTransitionMax (the setters' clamp and set_state's check keep it so) the gain is a function of that
// counter and the flag alone:  sqrtf(float(t) / float(nTransitionMax)) where nTransitionMax != 0 (1 at t == max, 0 at t == 0, as
// the reference's two constants), on ? 1 : 0 where it is 0.  So the serial part is integer-only.  surge_kernel runs on the tile
// walk of tile_chain_device.h:
//     prepare          the level tile into LDS
//     chain            two compares, two counters, one flag; row[i] becomes the BITS of the counter before the step (of the flag
//                      where nTransitionMax is 0)
//     emit             the correctly rounded quotient and root per sample (__fdiv_rn, sqrt_rn) into `out`, or (MUL) out *= gain,
//                      `out` read and written by the same lane
// By the walk's invariant `out` may be the level row.  fGain, both counters and the flag go back to the state array at the end.
// out and the state match tests/peak_surge_ref.py bit for bit.
//
// The setters of the reference act on the live counters AT ONCE (set_transition_time(5), then (100): the counter is at most 5),
// and so does reset().  The bank records them in call order and applies them to the device state before the next launch or
// state access (update_settings), as simple_autogain's recorded operations are.
#include "bank_core.h"
#include "tile_chain_device.h"

#include <vector>

#pragma clang fp contract(off)

namespace
{
    using namespace mi_tile_chain;

    enum { VEC_OUT = 1, VEC_IN = 2 };
    enum : uint32_t { OP_TRANSITION_MAX, OP_SHUTDOWN_MAX, OP_RESET };
    constexpr size_t COUNT_LIMIT = size_t(1) << 31;     // the kernel counts samples in 32 bits

    struct device_state { float gain; uint32_t transition, shutdown, on; };     // fGain, nTransitionTime, nShutdownTime, bOn
    struct recorded_op { uint32_t channel, kind, value; };

    // as sidechain.hip's: the correctly rounded float32 root through float64
    __device__ __forceinline__ float sqrt_rn(float q)
    {
        return float(__builtin_sqrt(double(q)));
    }

    // what the chain left for sample i -> fGain after it (SurgeProtector.cpp:126-145)
    __device__ __forceinline__ float gain_of(uint32_t bits, uint32_t tmax, float ftmax)
    {
        if (tmax == 0)
            return (bits != 0) ? 1.0f : 0.0f;
        return sqrt_rn(__fdiv_rn(float(bits), ftmax));
    }

    // One tile of one channel, SurgeProtector.cpp:101-145 without the gain.  A function of its own so that its instructions can
    // be looked at.
    __device__ __noinline__ device_state surge_chain_tile(lds_float *row, uint32_t n, device_state s, const mi_surge_params_t p)
    {
        uint32_t t = s.transition, sd = s.shutdown;
        bool on = s.on != 0;
        const uint32_t tmax = p.transition_max, sdmax = p.shutdown_max;
        const float on_thr = p.on_threshold, off_thr = p.off_threshold;
        // the branches of :101-145 as selects: a branch per sample costs the lane more than the few integer operations it skips
        chain_batches(row, 0, n, [&](float v)
        {
            const bool there = v >= off_thr, appears = v >= on_thr;
            const uint32_t counted = there ? 0u : sd + 1u;              // nShutdownTime while on
            sd = on ? counted : (appears ? 0u : sd);
            on = on ? (counted < sdmax) : appears;
            const uint32_t before = t;
            t = on ? t + ((t < tmax) ? 1u : 0u) : t - ((t > 0) ? 1u : 0u);
            return __uint_as_float((tmax != 0) ? before : uint32_t(on));
        });
        return device_state{ s.gain, t, sd, uint32_t(on) };
    }

    template <bool MUL>
    __global__ __launch_bounds__(BLOCK) void surge_kernel(float *out, const float *in, size_t out_stride, size_t in_stride,
                                                          uint32_t count, uint32_t channels, const mi_surge_params_t *params,
                                                          device_state *state, uint32_t vec)
    {
        __shared__ __attribute__((aligned(16))) float tile[2][GROUP][ROW];      // the level, then the counter's (flag's) bits
        const role me = my_role(channels);
        const uint32_t r = me.r, ch = me.ch, c = me.c;
        mi_surge_params_t p = {};
        device_state s = {};
        if (me.valid)
            p = params[ch];
        if (me.valid && me.chain)
            s = state[ch];
        const uint32_t tmax = p.transition_max;
        const float ftmax = float(tmax);
        const float *xs = in + size_t(ch) * in_stride;
        float *os = (out != nullptr) ? out + size_t(ch) * out_stride : nullptr;

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
            if (os == nullptr || c >= t.n)
                return;
            const float4 v4 = *reinterpret_cast<const float4 *>(&tile[k & 1][r][c]);
            const float b[4] = { v4.x, v4.y, v4.z, v4.w };
            float g[4];
            #pragma unroll
            for (uint32_t j = 0; j < 4; ++j)
                g[j] = gain_of(__float_as_uint(b[j]), tmax, ftmax);
            if (MUL)
            {
                float a[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
                if ((vec & VEC_OUT) && c + 4 <= t.n)
                {
                    const float4 a4 = *reinterpret_cast<const float4 *>(os + t.t0 + c);
                    a[0] = a4.x, a[1] = a4.y, a[2] = a4.z, a[3] = a4.w;
                }
                else
                {
                    #pragma unroll
                    for (uint32_t j = 0; j < 4; ++j)
                        if (c + j < t.n)
                            a[j] = os[t.t0 + c + j];
                }
                #pragma unroll
                for (uint32_t j = 0; j < 4; ++j)
                    g[j] = a[j] * g[j];                                         // out[i] *= gain, :178
            }
            store_quad(os + t.t0 + c, g, vec & VEC_OUT, c, t.n);
        };

        MI_TILE_CHAIN_WALK(me, count, k, load_tile(k),
                           s = surge_chain_tile((lds_float *)&tile[k & 1][r][0], tile_extent(count, k).n, s, p),
                           emit_tile(k));
        if (me.valid && me.chain)
        {
            // fGain: the last sample's, out of the last tile (which nobody writes after the walk's last barrier)
            const uint32_t last = count - 1;
            s.gain = gain_of(__float_as_uint(tile[(last / TILE) & 1][r][last % TILE]), tmax, ftmax);
            state[ch] = s;
        }
    }
} // namespace

struct mi_surge_bank : mi_bank::settings_bank<mi_surge_params_t, mi_surge_params_t, device_state>
{
    static constexpr const char *NAME = "mi_surge_bank";

    std::vector<recorded_op>    ops;                // what the setters and reset() do to the state, in call order

    static mi_surge_params_t fresh_settings() { return mi_surge_params_t{}; }          // construct(), :41-51
    static mi_surge_params_t fresh_params() { return mi_surge_params_t{}; }
    static device_state fresh_state() { return device_state{}; }
    static void compute(const mi_surge_params_t &s, mi_surge_params_t &p) { p = s; }
};

namespace
{
    // the recorded operations onto the device state, then the changed settings onto the device table
    int surge_update(mi_surge_bank *b, hipStream_t st)
    {
        if (!b->ops.empty())
        {
            const int r = mi::refuse_capture(mi_surge_bank::NAME, st);
            if (r != MI_OK)
                return r;
            std::vector<device_state> hs(b->channels);
            MI_HIP_CHECK(hipMemcpyAsync(hs.data(), b->d_state, hs.size() * sizeof(device_state), hipMemcpyDeviceToHost, st));
            MI_HIP_CHECK(hipStreamSynchronize(st));
            for (const recorded_op &op : b->ops)
            {
                device_state &s = hs[op.channel];
                if (op.kind == OP_TRANSITION_MAX)
                    s.transition = (s.transition < op.value) ? s.transition : op.value;    // lsp_limit(.., 0, time), :74
                else if (op.kind == OP_SHUTDOWN_MAX)
                    s.shutdown = (s.shutdown < op.value) ? s.shutdown : op.value;           // :80
                else
                    s.on = 0, s.transition = 0;                                             // reset(), :65-69
            }
            MI_HIP_CHECK(hipMemcpyAsync(b->d_state, hs.data(), hs.size() * sizeof(device_state), hipMemcpyHostToDevice, st));
            MI_HIP_CHECK(hipStreamSynchronize(st));                     // `hs` is gone after this returns
            b->ops.clear();
        }
        return mi_bank::update(b, st);
    }

    template <bool MUL>
    int surge_process(mi_surge_bank *b, const char *entry, float *out, const float *in, size_t count, size_t out_stride, size_t in_stride,
                      void *stream)
    {
        MI_REQUIRE(b != nullptr, MI_ESTATE, "%s: NULL bank", entry);
        hipStream_t st = mi::as_stream(stream);
        const int r = surge_update(b, st);
        if (r != MI_OK || count == 0)
            return r;
        const int k = mi_bank::check_rows(entry, b->channels, count, COUNT_LIMIT,
                                          { { out, out_stride, count, mi_bank::OUTPUT }, { in, in_stride, count, mi_bank::REQUIRED } });
        if (k != MI_OK)
            return k;
        const uint32_t vec = (mi::aligned16(out, out_stride, b->channels) ? VEC_OUT : 0) | (mi::aligned16(in, in_stride, b->channels) ? VEC_IN : 0);
        hipEvent_t ev0 = nullptr, ev1 = nullptr;
        mi::take_profile_events(&ev0, &ev1);
        MI_LAUNCH(surge_kernel<MUL>, dim3((b->channels + GROUP - 1) / GROUP), dim3(BLOCK), 0, st, ev0, ev1, out, in, out_stride,
                  in_stride, uint32_t(count), b->channels, b->d_params, b->d_state, vec);
        MI_HIP_CHECK(hipGetLastError());
        return MI_OK;
    }
} // namespace

extern "C" {

int mi_surge_bank_create(mi_surge_bank_t **bank, uint32_t channels)                                          // :41-51
{
    return mi_bank::create(bank, "mi_surge_bank_create", channels);
}

int mi_surge_bank_destroy(mi_surge_bank_t *b)
{
    return mi_bank::destroy(b);
}

int mi_surge_bank_set_transition_time(mi_surge_bank_t *b, uint32_t channel, uint32_t samples)                // :71-75
{
    MI_BANK_SETTER("surge", "set_transition_time");
    c.transition_max = samples;
    b->update[channel] = 1;
    b->ops.push_back(recorded_op{ channel, OP_TRANSITION_MAX, samples });
    return MI_OK;
}

int mi_surge_bank_set_shutdown_time(mi_surge_bank_t *b, uint32_t channel, uint32_t samples)                  // :77-81
{
    MI_BANK_SETTER("surge", "set_shutdown_time");
    c.shutdown_max = samples;
    b->update[channel] = 1;
    b->ops.push_back(recorded_op{ channel, OP_SHUTDOWN_MAX, samples });
    return MI_OK;
}

int mi_surge_bank_set_on_threshold(mi_surge_bank_t *b, uint32_t channel, float threshold)                    // :83-86
{
    MI_BANK_SETTER("surge", "set_on_threshold");
    c.on_threshold = threshold;
    b->update[channel] = 1;
    return MI_OK;
}

int mi_surge_bank_set_off_threshold(mi_surge_bank_t *b, uint32_t channel, float threshold)                   // :88-91
{
    MI_BANK_SETTER("surge", "set_off_threshold");
    c.off_threshold = threshold;
    b->update[channel] = 1;
    return MI_OK;
}

int mi_surge_bank_set_threshold(mi_surge_bank_t *b, uint32_t channel, float on, float off)                   // :93-97
{
    MI_BANK_SETTER("surge", "set_threshold");
    c.on_threshold = on, c.off_threshold = off;
    b->update[channel] = 1;
    return MI_OK;
}

int mi_surge_bank_reset(mi_surge_bank_t *b, uint32_t channel)                                                // :65-69
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_surge_bank_reset: NULL bank");
    MI_REQUIRE(channel < b->channels || channel == UINT32_MAX, MI_EINVAL, "mi_surge_bank_reset: channel %u out of range", channel);
    for (uint32_t ch = 0; ch < b->channels; ++ch)
        if (channel == UINT32_MAX || ch == channel)
            b->ops.push_back(recorded_op{ ch, OP_RESET, 0 });
    return MI_OK;
}

int mi_surge_bank_get_params(const mi_surge_bank_t *b, uint32_t channel, mi_surge_params_t *params)
{
    const int r = mi_bank::get_checks(b, "mi_surge_bank_get_params", channel, params);
    if (r == MI_OK)
        *params = b->cfg[channel];
    return r;
}

int mi_surge_bank_get_state(mi_surge_bank_t *b, uint32_t channel, mi_surge_state_t *state, void *stream)
{
    device_state s;
    int r = mi_bank::get_checks(b, "mi_surge_bank_get_state", channel, state);
    if (r == MI_OK)
        r = mi::refuse_state_access(mi::as_stream(stream));
    if (r == MI_OK)
        r = surge_update(b, mi::as_stream(stream));             // the setters have acted by now
    if (r == MI_OK)
        r = mi_bank::get_state(b, "mi_surge_bank_get_state", channel, &s, stream);
    if (r != MI_OK)
        return r;
    state->gain = s.gain, state->transition_time = s.transition, state->shutdown_time = s.shutdown, state->on = s.on;
    return MI_OK;
}

int mi_surge_bank_set_state(mi_surge_bank_t *b, uint32_t channel, const mi_surge_state_t *state, void *stream)
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_surge_bank_set_state: NULL bank");
    MI_REQUIRE(state != nullptr, MI_EINVAL, "mi_surge_bank_set_state: NULL state");
    MI_REQUIRE(channel < b->channels, MI_EINVAL, "mi_surge_bank_set_state: channel %u out of range", channel);
    const mi_surge_params_t &c = b->cfg[channel];
    MI_REQUIRE(state->transition_time <= c.transition_max && state->shutdown_time <= c.shutdown_max && state->on <= 1, MI_EINVAL,
               "mi_surge_bank_set_state: counters %u, %u above their maxima %u, %u, or a flag of %u", state->transition_time,
               state->shutdown_time, c.transition_max, c.shutdown_max, state->on);
    hipStream_t st = mi::as_stream(stream);
    int r = mi::refuse_state_access(st);
    if (r == MI_OK)
        r = surge_update(b, st);                                // what was recorded before this call does not undo it
    if (r != MI_OK)
        return r;
    const device_state s = { state->gain, state->transition_time, state->shutdown_time, state->on };
    return mi_bank::set_state(b, "mi_surge_bank_set_state", channel, s, true, st);
}

int mi_surge_bank_process(mi_surge_bank_t *b, float *out, const float *in, size_t count, size_t out_stride, size_t in_stride,
                          void *stream)                                                                      // :151-167
{
    return surge_process<false>(b, "mi_surge_bank_process", out, in, count, out_stride, in_stride, stream);
}

int mi_surge_bank_process_mul(mi_surge_bank_t *b, float *out, const float *in, size_t count, size_t out_stride, size_t in_stride,
                              void *stream)                                                                  // :169-179
{
    return surge_process<true>(b, "mi_surge_bank_process_mul", out, in, count, out_stride, in_stride, stream);
}

} // extern "C"
