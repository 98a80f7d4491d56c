// lsp::dspu::Panometer as a bank of `channels` panometers (src/main/meters/Panometer.cpp): process() (:133-216) -- the SQUARES of
// the samples into the two rings (dsp::sqr2), the refresh of fValueA and fValueB every nPeriod samples (dsp::h_sum over the
// window, sum(tail part) + sum(head part) where it wraps, :140-158), per sample v = (v + head) - tail for both, and the pan law
// on top: sl = sqrt(|va| * norm), sr = sqrt(|vb| * norm), out = sr / (sl + sr) where sl + sr > 1e-18 and fDefault otherwise
// (linear), the same without the roots and with 1e-36 (equal power).
//
// The step is TWO dependent roundings, (v + head) - tail, and cannot be folded into one increment.  panometer_kernel runs it
// in one launch on the walk of stereo_meter_device.h:
//     chain            wave 0, lanes 4 r + q: sum q of row r over two rows (the squared head samples, overwritten by the running
//                      sum, and the tail samples); both sums of a channel run side by side
//     emit             a tile out of LDS through |.| * norm, the roots of the linear law, the quotient or the default into `out`
//     prepare          loads of a and b (16 bytes where the rows allow), their squares into both rings, the tail samples (out
//                      of the same tile where i >= period, out of the ring otherwise), head and tail per sample into LDS, and
//                      the tile's refreshes, formed beside the chain and folded through the step of the sample they precede
// LDS, declared below: tile[2][4][4][260] floats (33280 B: buffers, channels, head and tail of two sums), hist[4][2][512] floats
// (16384 B), first[2][4] (32 B).
// out, fValueA, fValueB, nHead and nWindow match tests/stereo_meters_ref.py bit for bit: every product and every sum rounds
// once, the roots and the quotient are correctly rounded.  Inputs are finite; subnormals are kept.
#include "stereo_meter_bank_core.h"

#pragma clang fp contract(off)      // every product and every sum below rounds on its own

namespace
{
    using namespace mi_stereo_meter;

    constexpr float LINEAR_THRESHOLD = 1e-18f, POWER_THRESHOLD = 1e-36f;       // Panometer.cpp:190, :204

    // One tile of one sum of one channel: v = (v + head[i]) - tail[i], head[] in place; at first, first + period, ... head[]
    // holds the refreshed sum after that sample.  A function of its own so that its instructions can be looked at
    // (tests/test_stereo_meters_host.py).
    __device__ __noinline__ float panometer_chain_tile(lds_float *head, const lds_float *tail, uint32_t n, float sum, uint32_t first,
                                                       uint32_t period)
    {
        return chain_segments(head, n, sum, first, period, [&](uint32_t i, uint32_t to, float s)
        {
            chain_batches2(head, tail, i, to, [&](float h, float t) { return s = (s + h) - t; });
            return s;
        });
    }

    struct panometer
    {
        static constexpr int NS = 2, ROWS = 4;                      // va, vb: a row of heads and a row of tails each
        static __device__ __forceinline__ float ring_value(float x) { return x * x; }
        // dsp::h_sum's terms: the rings' values as they are
        static __device__ __forceinline__ float term(uint32_t q, float x, float y) { return (q & 1u) ? y : x; }
        static __device__ __forceinline__ void steps(lds_float *rows, uint32_t i, float ah, float bh, float at, float bt)
        {
            rows[i] = ah;
            rows[ROW + i] = at;
            rows[2 * ROW + i] = bh;
            rows[3 * ROW + i] = bt;
        }
        static __device__ __forceinline__ float fold(uint32_t q, const lds_float *rows, uint32_t i, float s)
        {
            return (s + rows[2 * q * ROW + i]) - rows[(2 * q + 1) * ROW + i];
        }
        static __device__ __forceinline__ float chain(lds_float *rows, uint32_t q, uint32_t n, float sum, uint32_t first, uint32_t period)
        {
            return panometer_chain_tile(rows + 2 * q * ROW, rows + (2 * q + 1) * ROW, n, sum, first, period);
        }
        static __device__ __forceinline__ void emit(const meter_params &p, const lds_float *rows, uint32_t c, float (&y)[4])
        {
            const f32x4 va = *reinterpret_cast<const lds_f32x4 *>(rows + c), vb = *reinterpret_cast<const lds_f32x4 *>(rows + 2 * ROW + c);
            const bool linear = p.law == MI_PAN_LAW_LINEAR;
            #pragma unroll
            for (int j = 0; j < 4; ++j)
            {
                float sl = fabsf(va[j]) * p.norm, sr = fabsf(vb[j]) * p.norm;
                if (linear)
                    sl = sqrt_rn(sl), sr = sqrt_rn(sr);
                const float den = sl + sr;
                y[j] = (den > (linear ? LINEAR_THRESHOLD : POWER_THRESHOLD)) ? __fdiv_rn(sr, den) : p.dflt;
            }
        }
    };

    __global__ __launch_bounds__(BLOCK) void panometer_kernel(float *out, const float *a, const float *b, size_t out_stride,
                                                              size_t a_stride, size_t b_stride, uint32_t count, uint32_t channels,
                                                              const meter_params *params, meter_state *state, float *rings,
                                                              size_t ring_stride, uint32_t vec)
    {
        __shared__ meter_lds<panometer> lds;
        meter_process<panometer>(lds, out, a, b, out_stride, a_stride, b_stride, count, channels, params, state, rings, ring_stride, vec);
    }
} // namespace

struct mi_panometer_bank : bank_core
{
};

extern "C" {

int mi_panometer_bank_create(mi_panometer_bank_t **bank, uint32_t channels, uint32_t max_period)             // :71-100
{
    return core_create(bank, "mi_panometer_bank_create", "mi_panometer_bank", channels, max_period);
}

int mi_panometer_bank_destroy(mi_panometer_bank_t *b)
{
    return core_destroy(b);
}

int mi_panometer_bank_set_period(mi_panometer_bank_t *b, uint32_t channel, uint32_t period)                  // :112-123
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_panometer_bank_set_period: NULL bank");
    return core_set_period(*b, channel, period, P_WINDOW | P_ZERO_SUMS);      // at once: nWindow = nPeriod, both sums 0
}

int mi_panometer_bank_set_pan_law(mi_panometer_bank_t *b, uint32_t channel, uint32_t law)                    // :102-105
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_panometer_bank_set_pan_law: NULL bank");
    MI_REQUIRE(channel < b->channels, MI_EINVAL, "mi_panometer_bank_set_pan_law: channel %u out of range", channel);
    MI_REQUIRE(law <= MI_PAN_LAW_EQUAL_POWER, MI_EINVAL, "mi_panometer_bank_set_pan_law: law %u", law);
    if (b->cfg[channel].law != law)
    {
        b->cfg[channel].law = law;
        b->up.touch(channel);
    }
    return MI_OK;
}

int mi_panometer_bank_set_default_pan(mi_panometer_bank_t *b, uint32_t channel, float default_pan)           // :107-110
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_panometer_bank_set_default_pan: NULL bank");
    MI_REQUIRE(channel < b->channels, MI_EINVAL, "mi_panometer_bank_set_default_pan: channel %u out of range", channel);
    if (memcmp(&b->cfg[channel].dflt, &default_pan, sizeof(float)) != 0)
    {
        b->cfg[channel].dflt = default_pan;
        b->up.touch(channel);
    }
    return MI_OK;
}

int mi_panometer_bank_clear(mi_panometer_bank_t *b, uint32_t channel)                                        // :125-131
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_panometer_bank_clear: NULL bank");
    return core_clear(*b, channel, false);
}

int mi_panometer_bank_update_settings(mi_panometer_bank_t *b, void *stream)
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_panometer_bank_update_settings: NULL bank");
    return core_update(*b, mi::as_stream(stream));
}

int mi_panometer_bank_get_params(const mi_panometer_bank_t *b, uint32_t channel, mi_panometer_params_t *params)
{
    const int r = mi_bank::get_checks(b, "mi_panometer_bank_get_params", channel, params);
    if (r != MI_OK)
        return r;
    const channel_cfg &c = b->cfg[channel];
    params->period = c.period, params->capacity = b->capacity, params->max_period = b->max_period, params->law = c.law;
    params->norm = c.norm, params->default_pan = c.dflt;
    return MI_OK;
}

int mi_panometer_bank_get_state(mi_panometer_bank_t *b, uint32_t channel, mi_panometer_state_t *state, void *stream)
{
    meter_state s;
    int r = mi_bank::get_checks(b, "mi_panometer_bank_get_state", channel, state);
    if (r == MI_OK)
        r = mi_bank::get_state(b, "mi_panometer_bank_get_state", channel, &s, stream);
    if (r != MI_OK)
        return r;
    state->value_a = s.sum[0], state->value_b = s.sum[1], state->head = s.head, state->window = s.window;
    return MI_OK;
}

int mi_panometer_bank_set_state(mi_panometer_bank_t *b, uint32_t channel, const mi_panometer_state_t *state, uint32_t zero_rings,
                                void *stream)
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_panometer_bank_set_state: NULL bank");
    MI_REQUIRE(state != nullptr, MI_EINVAL, "mi_panometer_bank_set_state: NULL state");
    const meter_state s = { { state->value_a, state->value_b, 0.0f }, state->head, state->window };
    return core_set_state(*b, channel, s, zero_rings != 0, mi::as_stream(stream));
}

int mi_panometer_bank_process(mi_panometer_bank_t *b, float *out, const float *a, const float *in_b, size_t count,
                              size_t out_stride, size_t a_stride, size_t b_stride, void *stream)              // :133-216
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_panometer_bank_process: NULL bank");
    bank_core &k = *b;
    hipStream_t st = mi::as_stream(stream);
    const int r = core_update(k, st);
    if (r != MI_OK || count == 0)
        return r;
    uint32_t vec = 0;
    const int c = core_check(k, "mi_panometer_bank_process", out, a, in_b, count, out_stride, a_stride, b_stride, &vec);
    if (c != MI_OK)
        return c;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    mi::take_profile_events(&ev0, &ev1);
    MI_LAUNCH(panometer_kernel, dim3((k.channels + GROUP - 1) / GROUP), dim3(BLOCK), 0, st, ev0, ev1, out, a, in_b, out_stride,
              a_stride, b_stride, uint32_t(count), k.channels, k.d_params, k.d_state, k.d_rings, k.ring_stride, vec);
    MI_HIP_CHECK(hipGetLastError());
    return MI_OK;
}

} // extern "C"
