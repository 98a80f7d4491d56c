// lsp::dspu::Correlometer as a bank of `channels` correlometers (src/main/meters/Correlometer.cpp): process() (:134-184) -- the
// samples into the two rings, the refresh of sCorr every nPeriod samples (dsp::corr_init over the window, in two pieces where it
// wraps, :143-157) and dsp::corr_incr: v += ah*bh - at*bt, a += ah*ah - at*at, b += bh*bh - bt*bt, out = v / sqrt(a * b) where
// a * b >= CORR_THRESHOLD, otherwise 0.
//
// The three increments of a sample do not depend on the sums, so every lane can form them, and what is left of the recurrence
// is ONE dependent add per sample and sum.  correlometer_kernel runs it in one launch on the walk of stereo_meter_device.h:
//     chain            wave 0, lanes 4 r + q: sum q of row r, its increments overwritten by the running sum in LDS; the three
//                      sums of a channel run side by side
//     emit             a tile out of LDS through a * b, the root and the quotient into `out`
//     prepare          loads of a and b (16 bytes where the rows allow), the samples into both rings, the tail samples (out of
//                      the same tile where i >= period, out of the ring otherwise), three increments per sample into LDS, and
//                      the tile's refreshes, formed beside the chain and folded through the step of the sample they precede
// LDS, declared below: tile[2][4][3][260] floats (24960 B: buffers, channels, sums), hist[4][2][512] floats (16384 B: the rings'
// last `period` samples and the tile's, what `last` and the refreshes read), first[2][4] (32 B).
// out, sCorr, nHead and nWindow match tests/stereo_meters_ref.py bit for bit: every product and every sum rounds once, the
// root and the quotient are correctly rounded.  Inputs are finite; subnormals are kept (the float32 denormal mode is on).
#include "stereo_meter_bank_core.h"

#pragma clang fp contract(off)      // every product and every sum below rounds on its own

namespace
{
    using namespace mi_stereo_meter;

    // dsp::corr_incr's threshold under which the correlation is 0: upstream lsp-dsp-lib's generic implementation; the reference
    // tree does not carry it
    constexpr float CORR_THRESHOLD = 1e-10f;

    // One tile of one sum of one channel: sum += d[i], the row in place; at first, first + period, ... the row holds the
    // refreshed sum after that sample.  A function of its own so that its instructions can be looked at
    // (tests/test_stereo_meters_host.py).
    __device__ __noinline__ float correlometer_chain_tile(lds_float *row, uint32_t n, float sum, uint32_t first, uint32_t period)
    {
        return chain_segments(row, n, sum, first, period, [&](uint32_t i, uint32_t to, float s)
        {
            chain_batches(row, i, to, [&](float d) { return s = s + d; });
            return s;
        });
    }

    struct correlometer
    {
        static constexpr int NS = 3, ROWS = 3;                      // v, a, b: one row each
        static __device__ __forceinline__ float ring_value(float x) { return x; }
        // dsp::corr_init's terms: x*y, x*x, y*y
        static __device__ __forceinline__ float term(uint32_t q, float x, float y)
        {
            const float l = (q == 2) ? y : x, r = (q == 1) ? x : y;
            return l * r;
        }
        static __device__ __forceinline__ void steps(lds_float *rows, uint32_t i, float ah, float bh, float at, float bt)
        {
            rows[i] = ah * bh - at * bt;
            rows[ROW + i] = ah * ah - at * at;
            rows[2 * ROW + i] = bh * bh - bt * bt;
        }
        static __device__ __forceinline__ float fold(uint32_t q, const lds_float *rows, uint32_t i, float s)
        {
            return s + rows[q * ROW + i];
        }
        static __device__ __forceinline__ float chain(lds_float *rows, uint32_t q, uint32_t n, float sum, uint32_t first, uint32_t period)
        {
            return correlometer_chain_tile(rows + q * ROW, n, sum, first, period);
        }
        static __device__ __forceinline__ void emit(const meter_params &, const lds_float *rows, uint32_t c, float (&y)[4])
        {
            const f32x4 v = *reinterpret_cast<const lds_f32x4 *>(rows + c), a = *reinterpret_cast<const lds_f32x4 *>(rows + ROW + c),
                        b = *reinterpret_cast<const lds_f32x4 *>(rows + 2 * ROW + c);
            #pragma unroll
            for (int j = 0; j < 4; ++j)
            {
                const float d = a[j] * b[j];
                y[j] = (d >= CORR_THRESHOLD) ? __fdiv_rn(v[j], sqrt_rn(d)) : 0.0f;
            }
        }
    };

    __global__ __launch_bounds__(BLOCK) void correlometer_kernel(float *out, const float *a, const float *b, size_t out_stride,
                                                                 size_t a_stride, size_t b_stride, uint32_t count, uint32_t channels,
                                                                 const meter_params *params, meter_state *state, float *rings,
                                                                 size_t ring_stride, uint32_t vec)
    {
        __shared__ meter_lds<correlometer> lds;
        meter_process<correlometer>(lds, out, a, b, out_stride, a_stride, b_stride, count, channels, params, state, rings, ring_stride, vec);
    }
} // namespace

struct mi_correlometer_bank : bank_core
{
};

extern "C" {

int mi_correlometer_bank_create(mi_correlometer_bank_t **bank, uint32_t channels, uint32_t max_period)       // :68-101
{
    return core_create(bank, "mi_correlometer_bank_create", "mi_correlometer_bank", channels, max_period);
}

int mi_correlometer_bank_destroy(mi_correlometer_bank_t *b)
{
    return core_destroy(b);
}

int mi_correlometer_bank_set_period(mi_correlometer_bank_t *b, uint32_t channel, uint32_t period)            // :103-111
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_correlometer_bank_set_period: NULL bank");
    return core_set_period(*b, channel, period, P_WINDOW);            // CF_UPDATE: nWindow = nPeriod at the next process()
}

int mi_correlometer_bank_clear(mi_correlometer_bank_t *b, uint32_t channel)                                  // :122-132
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_correlometer_bank_clear: NULL bank");
    return core_clear(*b, channel, true);
}

int mi_correlometer_bank_update_settings(mi_correlometer_bank_t *b, void *stream)
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_correlometer_bank_update_settings: NULL bank");
    return core_update(*b, mi::as_stream(stream));
}

int mi_correlometer_bank_get_params(const mi_correlometer_bank_t *b, uint32_t channel, mi_correlometer_params_t *params)
{
    const int r = mi_bank::get_checks(b, "mi_correlometer_bank_get_params", channel, params);
    if (r != MI_OK)
        return r;
    params->period = b->cfg[channel].period, params->capacity = b->capacity, params->max_period = b->max_period;
    return MI_OK;
}

int mi_correlometer_bank_get_state(mi_correlometer_bank_t *b, uint32_t channel, mi_correlometer_state_t *state, void *stream)
{
    meter_state s;
    int r = mi_bank::get_checks(b, "mi_correlometer_bank_get_state", channel, state);
    if (r == MI_OK)
        r = mi_bank::get_state(b, "mi_correlometer_bank_get_state", channel, &s, stream);
    if (r != MI_OK)
        return r;
    state->v = s.sum[0], state->a = s.sum[1], state->b = s.sum[2], state->head = s.head, state->window = s.window;
    return MI_OK;
}

int mi_correlometer_bank_set_state(mi_correlometer_bank_t *b, uint32_t channel, const mi_correlometer_state_t *state,
                                   uint32_t zero_rings, void *stream)
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_correlometer_bank_set_state: NULL bank");
    MI_REQUIRE(state != nullptr, MI_EINVAL, "mi_correlometer_bank_set_state: NULL state");
    const meter_state s = { { state->v, state->a, state->b }, state->head, state->window };
    return core_set_state(*b, channel, s, zero_rings != 0, mi::as_stream(stream));
}

int mi_correlometer_bank_process(mi_correlometer_bank_t *b, float *out, const float *a, const float *in_b, size_t count,
                                 size_t out_stride, size_t a_stride, size_t b_stride, void *stream)           // :134-184
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_correlometer_bank_process: NULL bank");
    bank_core &k = *b;
    hipStream_t st = mi::as_stream(stream);
    const int r = core_update(k, st);
    if (r != MI_OK || count == 0)
        return r;
    uint32_t vec = 0;
    const int c = core_check(k, "mi_correlometer_bank_process", out, a, in_b, count, out_stride, a_stride, b_stride, &vec);
    if (c != MI_OK)
        return c;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    mi::take_profile_events(&ev0, &ev1);
    MI_LAUNCH(correlometer_kernel, dim3((k.channels + GROUP - 1) / GROUP), dim3(BLOCK), 0, st, ev0, ev1, out, a, in_b, out_stride,
              a_stride, b_stride, uint32_t(count), k.channels, k.d_params, k.d_state, k.d_rings, k.ring_stride, vec);
    MI_HIP_CHECK(hipGetLastError());
    return MI_OK;
}

} // extern "C"
