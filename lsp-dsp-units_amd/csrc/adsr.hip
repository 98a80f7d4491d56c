// mi_adsr_bank -- `channels` x lsp::dspu::ADSREnvelope (reference: src/main/util/ADSREnvelope.cpp:295-533).  The unit keeps no
// stream state: a sample of any of the five array entry points is a function of one time value and the channel's designed record,
// so every sample of every channel is independent and the roof is memory traffic.
//
//   adsr_kernel<OP, VEC>     grid (tiles of TILE samples, channels): few channels x very long rows fill the device as well as many
//       short ones.  A lane owns 4 consecutive samples and, where the rows allow it (VEC), moves them as 16 bytes; rows whose base
//       or stride breaks that alignment take the same arithmetic sample by sample.  The channel's record (adsr_bank.h) is read
//       through a pointer that depends on blockIdx alone: uniform, so it sits in SGPRs, and the switch on a segment's function is
//       a scalar branch.  The stage of a sample comes from compares; lanes of a wave then differ only where the wave straddles a
//       segment boundary.  All inputs of a lane are read before anything is stored, so dst may be src.  Nothing but dst is written.
//   adsr_gen_kernel          start and step of generate*: up to PAIRS channels' values travel as the ARGUMENTS of a small launch in
//       front of the tiles and are written to the bank's table there.  Arguments are copied when a launch is issued or captured: no
//       host buffer has to outlive the call, nothing synchronises, and a captured call replays the values of capture time.
//
// generate*'s loops (:385-533) only move forward through the stages; in closed form sample i is at stage
// max(floor, stage_of(t_i)), floor = stage_of(start) for a negative step and 0 otherwise, a NaN t at "after".  t_0 is start itself
// (0 * step would make a NaN of an infinite step), t_i = start + float(i) * step in two roundings.
#include "adsr_bank.h"
#include "bank_core.h"

#include <vector>

#pragma clang fp contract(off)

namespace
{
    using mi_adsr::record;

    constexpr int      BLOCK = 256;
    constexpr uint32_t PER = 4, TILE = BLOCK * PER;
    constexpr size_t   COUNT_LIMIT = size_t(1) << 31;           // sample indices are 32-bit
    constexpr uint32_t PAIRS = 448;                             // 3584 bytes of arguments, below the 4 KiB a launch may carry

    enum { OP_PROCESS, OP_PROCESS_MUL, OP_GENERATE, OP_GENERATE_MUL, OP_GENERATE_MUL_SRC };

    struct gen_pairs { float2 v[PAIRS]; };                      // { start, step }
    struct no_state { uint32_t unused; };                       // the bank core keeps a state array; this unit has none

    template <bool VEC> __device__ __forceinline__ void load4(float (&v)[PER], const float *p, bool whole, uint32_t left)
    {
        if (VEC && whole)
        {
            const float4 q = *reinterpret_cast<const float4 *>(p);
            v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
        }
        else
        {
            #pragma unroll
            for (uint32_t k = 0; k < PER; ++k)
                v[k] = (k < left) ? p[k] : 0.0f;
        }
    }

    template <int OP, bool VEC>
    __global__ __launch_bounds__(BLOCK) void adsr_kernel(float *dst, const float *src, size_t dst_stride, size_t src_stride, uint32_t count,
                                                         const record *__restrict__ params, const float2 *__restrict__ gen)
    {
        constexpr bool GEN = OP >= OP_GENERATE;
        constexpr bool READS_SRC = OP == OP_PROCESS || OP == OP_PROCESS_MUL || OP == OP_GENERATE_MUL_SRC;
        constexpr bool READS_DST = OP == OP_PROCESS_MUL || OP == OP_GENERATE_MUL;
        const uint32_t ch = blockIdx.y;
        const record R = params[ch];
        if (!R.enabled)
            return;
        const uint32_t i0 = (blockIdx.x * BLOCK + threadIdx.x) * PER;
        if (i0 >= count)
            return;
        const uint32_t left = count - i0;
        const bool whole = left >= PER;
        float *out = dst + size_t(ch) * dst_stride + i0;
        float s[PER] = { 0.0f, 0.0f, 0.0f, 0.0f }, d[PER] = { 0.0f, 0.0f, 0.0f, 0.0f };
        if (READS_SRC)
            load4<VEC>(s, src + size_t(ch) * src_stride + i0, whole, left);
        if (READS_DST)
            load4<VEC>(d, out, whole, left);

        float start = 0.0f, step = 0.0f;
        int low = mi_adsr::BEFORE;                            // the stage that a negative step cannot go back below
        if (GEN)
        {
            const float2 g = gen[ch];
            start = g.x, step = g.y;
            low = (step < 0.0f) ? mi_adsr::stage_of(R, start, mi_adsr::AFTER) : mi_adsr::BEFORE;
        }
        float v[PER];
        #pragma unroll
        for (uint32_t k = 0; k < PER; ++k)
        {
            const uint32_t i = i0 + k;
            float t;
            int stage;
            if (GEN)
            {
                t = (i == 0) ? start : start + __uint2float_rn(i) * step;
                stage = mi_adsr::stage_of(R, t, mi_adsr::AFTER);
                stage = (stage > low) ? stage : low;
            }
            else
            {
                t = s[k];
                stage = mi_adsr::stage_of(R, t, mi_adsr::RELEASE);
            }
            const float g = mi_adsr::value_at(R, stage, t);
            [[maybe_unused]] const bool outside = stage == mi_adsr::BEFORE || stage == mi_adsr::AFTER, hold = stage == mi_adsr::HOLD;
            if (OP == OP_PROCESS || OP == OP_GENERATE)
                v[k] = g;
            else if (OP == OP_PROCESS_MUL)
                v[k] = d[k] * g;
            else if (OP == OP_GENERATE_MUL)                     // :443-444, :452-456, :481-482: a store, nothing, a store
                v[k] = outside ? 0.0f : hold ? d[k] : d[k] * g;
            else                                                // :493-494, :504-505, :531-532
                v[k] = outside ? 0.0f : hold ? s[k] : s[k] * g;
        }
        if (VEC && whole)
            *reinterpret_cast<float4 *>(out) = make_float4(v[0], v[1], v[2], v[3]);
        else
        {
            #pragma unroll
            for (uint32_t k = 0; k < PER; ++k)
                if (k < left)
                    out[k] = v[k];
        }
    }

    __global__ __launch_bounds__(BLOCK) void adsr_gen_kernel(float2 *__restrict__ gen, uint32_t n, const gen_pairs pairs)
    {
        const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
        if (i < n)
            gen[i] = pairs.v[i];
    }
} // namespace

struct mi_adsr_bank : mi_bank::tables<record, no_state>
{
    std::vector<mi_adsr_settings_t> cfg;
    std::vector<uint8_t>            enabled;
    uint32_t                        disabled = 0;
    float2                         *d_gen = nullptr;            // [channels] { start, step } of the generate call in flight
};

namespace
{
    constexpr const char *NAME = "mi_adsr_bank";

    // update_settings of every channel that asks for it; changed records go to the device
    int update(mi_adsr_bank *b, hipStream_t st)
    {
        for (uint32_t ch = 0; ch < b->channels; ++ch)
        {
            mi_adsr_settings_t &c = b->cfg[ch];
            if (c.flags & MI_ADSR_RECONFIGURE)
                mi_adsr_settings_update(&c);
            const record r = mi_adsr::record_of(c, b->enabled[ch]);
            if (memcmp(&r, &b->params[ch], sizeof(r)) != 0)
                b->params[ch] = r, b->up.touch(ch);
        }
        return mi_bank::upload(*b, NAME, st);
    }

    // rows a[c] = a + c * as and b[c] = b + c * bs of `count` floats: does any row of one meet a row of the other?  Exact for one
    // channel and for equal strides (up to the number of rows); rows with different strides are taken as two blocks.
    bool rows_meet(const float *a, size_t as, const float *b, size_t bs, uint32_t channels, size_t count)
    {
        const uintptr_t a0 = reinterpret_cast<uintptr_t>(a) / sizeof(float), b0 = reinterpret_cast<uintptr_t>(b) / sizeof(float);
        if (channels == 1)
            as = bs = count;
        const uintptr_t a1 = a0 + size_t(channels - 1) * as + count, b1 = b0 + size_t(channels - 1) * bs + count;
        if (a1 <= b0 || b1 <= a0)
            return false;
        if (as != bs || as < count)
            return true;
        const size_t r = ((a0 > b0) ? a0 - b0 : b0 - a0) % as;
        return r < count || as - r < count;
    }

    template <int OP> void launch(mi_adsr_bank *b, float *dst, const float *src, size_t dst_stride, size_t src_stride, uint32_t count, bool vec,
                                  hipStream_t st, hipEvent_t ev0, hipEvent_t ev1)
    {
        const dim3 grid((count + TILE - 1) / TILE, b->channels), block(BLOCK);
        if (vec)
            MI_LAUNCH((adsr_kernel<OP, true>), grid, block, 0, st, ev0, ev1, dst, src, dst_stride, src_stride, count, b->d_params, b->d_gen);
        else
            MI_LAUNCH((adsr_kernel<OP, false>), grid, block, 0, st, ev0, ev1, dst, src, dst_stride, src_stride, count, b->d_params, b->d_gen);
    }

    int run(mi_adsr_bank *b, const char *entry, int op, float *dst, const float *src, const float *start, const float *step, size_t count,
            size_t dst_stride, size_t src_stride, void *stream)
    {
        MI_REQUIRE(b != nullptr, MI_ESTATE, "%s: NULL bank", entry);
        if (count == 0)
            return MI_OK;
        const bool gen = op >= OP_GENERATE, needs_src = op == OP_PROCESS || op == OP_PROCESS_MUL || op == OP_GENERATE_MUL_SRC;
        if (!needs_src)
            src = nullptr, src_stride = 0;
        int r = mi_bank::check_rows(entry, b->channels, count, COUNT_LIMIT,
                                    { { dst, dst_stride, count, mi_bank::REQUIRED | mi_bank::OUTPUT },
                                      { src, src_stride, count, needs_src ? uint32_t(mi_bank::REQUIRED) : 0u } });
        if (r != MI_OK)
            return r;
        MI_REQUIRE(!gen || (start != nullptr && step != nullptr), MI_EINVAL, "%s: NULL start or step", entry);
        MI_REQUIRE(src == nullptr || (src == dst && (src_stride == dst_stride || b->channels == 1)) ||
                   !rows_meet(dst, dst_stride, src, src_stride, b->channels, count), MI_EINVAL,
                   "%s: dst and src overlap without being the same rows", entry);
        hipStream_t st = mi::as_stream(stream);
        r = update(b, st);                                      // :336, :344, :387, :437, :487
        if (r != MI_OK)
            return r;
        if (b->disabled == b->channels)
            return MI_OK;
        if (gen)
        {
            gen_pairs pairs;
            for (uint32_t first = 0; first < b->channels; first += PAIRS)
            {
                const uint32_t n = (b->channels - first < PAIRS) ? b->channels - first : PAIRS;
                for (uint32_t k = 0; k < n; ++k)
                    pairs.v[k] = make_float2(start[first + k], step[first + k]);
                for (uint32_t k = n; k < PAIRS; ++k)
                    pairs.v[k] = make_float2(0.0f, 0.0f);
                hipLaunchKernelGGL(adsr_gen_kernel, dim3((n + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, st, b->d_gen + first, n, pairs);
                MI_HIP_CHECK(hipGetLastError());
            }
        }
        const bool vec = mi::aligned16(dst, dst_stride, b->channels) && (src == nullptr || mi::aligned16(src, src_stride, b->channels));
        const uint32_t n = uint32_t(count);
        hipEvent_t ev0 = nullptr, ev1 = nullptr;
        mi::take_profile_events(&ev0, &ev1);
        switch (op)
        {
            case OP_PROCESS:        launch<OP_PROCESS>(b, dst, src, dst_stride, src_stride, n, vec, st, ev0, ev1); break;
            case OP_PROCESS_MUL:    launch<OP_PROCESS_MUL>(b, dst, src, dst_stride, src_stride, n, vec, st, ev0, ev1); break;
            case OP_GENERATE:       launch<OP_GENERATE>(b, dst, src, dst_stride, src_stride, n, vec, st, ev0, ev1); break;
            case OP_GENERATE_MUL:   launch<OP_GENERATE_MUL>(b, dst, src, dst_stride, src_stride, n, vec, st, ev0, ev1); break;
            default:                launch<OP_GENERATE_MUL_SRC>(b, dst, src, dst_stride, src_stride, n, vec, st, ev0, ev1); break;
        }
        MI_HIP_CHECK(hipGetLastError());
        return MI_OK;
    }
} // namespace

extern "C" {

int mi_adsr_bank_create(mi_adsr_bank_t **bank, uint32_t channels)
{
    int r = mi_bank::open(bank, "mi_adsr_bank_create", channels, 65535u);
    if (r != MI_OK)
        return r;
    mi_adsr_bank *b = *bank;
    *bank = nullptr;
    b->channels = channels;
    mi_adsr_settings_t fresh;
    mi_adsr_settings_init(&fresh);
    b->cfg.assign(channels, fresh);
    b->enabled.assign(channels, 1);
    record p = mi_adsr::record_of(fresh, 1);
    p.enabled = ~0u;                                        // no channel's record is what update_settings will make: all are sent
    r = mi_bank::alloc(*b, "mi_adsr_bank_create", p, no_state{ 0 });
    if (r == MI_OK)
    {
        const hipError_t e = hipMalloc(reinterpret_cast<void **>(&b->d_gen), size_t(channels) * sizeof(float2));
        if (e == hipSuccess)
            (void)hipMemset(b->d_gen, 0, size_t(channels) * sizeof(float2));
        else
            r = mi::fail(MI_EHIP, "mi_adsr_bank_create: %s", hipGetErrorString(e));
    }
    if (r != MI_OK)
    {
        mi_adsr_bank_destroy(b);
        return r;
    }
    *bank = b;
    return MI_OK;
}

int mi_adsr_bank_destroy(mi_adsr_bank_t *b)
{
    if (b == nullptr)
        return MI_OK;
    (void)hipFree(b->d_gen);
    return mi_bank::destroy(b);
}

int mi_adsr_bank_set(mi_adsr_bank_t *b, uint32_t channel, uint32_t setter, double x, double y, double z)
{
    MI_BANK_SETTER("adsr", "set");
    return mi_adsr_settings_set(&c, setter, x, y, z);
}

#define ADSR_SETTER(name, args, setter, x, y, z) \
    int mi_adsr_bank_##name args \
    { \
        MI_BANK_SETTER("adsr", #name); \
        return mi_adsr_settings_set(&c, setter, x, y, z); \
    }
#define ADSR_B mi_adsr_bank_t *b, uint32_t channel
ADSR_SETTER(set_attack_time, (ADSR_B, float v), MI_ADSR_SET_ATTACK_TIME, v, 0, 0)
ADSR_SETTER(set_hold_time, (ADSR_B, float v), MI_ADSR_SET_HOLD_TIME, v, 0, 0)
ADSR_SETTER(set_decay_time, (ADSR_B, float v), MI_ADSR_SET_DECAY_TIME, v, 0, 0)
ADSR_SETTER(set_slope_time, (ADSR_B, float v), MI_ADSR_SET_SLOPE_TIME, v, 0, 0)
ADSR_SETTER(set_release_time, (ADSR_B, float v), MI_ADSR_SET_RELEASE_TIME, v, 0, 0)
ADSR_SETTER(set_attack_curve, (ADSR_B, float v), MI_ADSR_SET_ATTACK_CURVE, v, 0, 0)
ADSR_SETTER(set_decay_curve, (ADSR_B, float v), MI_ADSR_SET_DECAY_CURVE, v, 0, 0)
ADSR_SETTER(set_slope_curve, (ADSR_B, float v), MI_ADSR_SET_SLOPE_CURVE, v, 0, 0)
ADSR_SETTER(set_release_curve, (ADSR_B, float v), MI_ADSR_SET_RELEASE_CURVE, v, 0, 0)
ADSR_SETTER(set_attack_function, (ADSR_B, uint32_t v), MI_ADSR_SET_ATTACK_FUNCTION, v, 0, 0)
ADSR_SETTER(set_decay_function, (ADSR_B, uint32_t v), MI_ADSR_SET_DECAY_FUNCTION, v, 0, 0)
ADSR_SETTER(set_slope_function, (ADSR_B, uint32_t v), MI_ADSR_SET_SLOPE_FUNCTION, v, 0, 0)
ADSR_SETTER(set_release_function, (ADSR_B, uint32_t v), MI_ADSR_SET_RELEASE_FUNCTION, v, 0, 0)
ADSR_SETTER(set_break_level, (ADSR_B, float v), MI_ADSR_SET_BREAK_LEVEL, v, 0, 0)
ADSR_SETTER(set_sustain_level, (ADSR_B, float v), MI_ADSR_SET_SUSTAIN_LEVEL, v, 0, 0)
ADSR_SETTER(set_hold_enabled, (ADSR_B, int v), MI_ADSR_SET_HOLD_ENABLED, v != 0, 0, 0)
ADSR_SETTER(set_break_enabled, (ADSR_B, int v), MI_ADSR_SET_BREAK_ENABLED, v != 0, 0, 0)
ADSR_SETTER(set_attack, (ADSR_B, float t, float v, uint32_t f), MI_ADSR_SET_ATTACK, t, v, f)
ADSR_SETTER(set_hold, (ADSR_B, float t, int on), MI_ADSR_SET_HOLD, t, on != 0, 0)
ADSR_SETTER(set_decay, (ADSR_B, float t, float v, uint32_t f), MI_ADSR_SET_DECAY, t, v, f)
ADSR_SETTER(set_break, (ADSR_B, float l, int on), MI_ADSR_SET_BREAK, l, on != 0, 0)
ADSR_SETTER(set_slope, (ADSR_B, float t, float v, uint32_t f), MI_ADSR_SET_SLOPE, t, v, f)
ADSR_SETTER(set_release, (ADSR_B, float t, float v, uint32_t f), MI_ADSR_SET_RELEASE, t, v, f)
#undef ADSR_B
#undef ADSR_SETTER

int mi_adsr_bank_set_settings(mi_adsr_bank_t *b, uint32_t channel, const mi_adsr_settings_t *settings)
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_adsr_bank_set_settings: NULL bank");
    MI_REQUIRE(channel < b->channels && settings != nullptr, MI_EINVAL, "mi_adsr_bank_set_settings: bad argument");
    bool nan = std::isnan(settings->hold_time) || std::isnan(settings->break_level) || std::isnan(settings->sustain_level);
    for (int k = 0; k < MI_ADSR_PARTS; ++k)
        nan = nan || std::isnan(settings->curve[k].time) || std::isnan(settings->curve[k].curve);
    MI_REQUIRE(!nan, MI_EINVAL, "mi_adsr_bank_set_settings: a NaN time, curve or level");
    b->cfg[channel] = *settings;
    return MI_OK;
}

int mi_adsr_bank_get_settings(const mi_adsr_bank_t *b, uint32_t channel, mi_adsr_settings_t *settings)
{
    const int r = mi_bank::get_checks(b, "mi_adsr_bank_get_settings", channel, settings);
    if (r == MI_OK)
        *settings = b->cfg[channel];
    return r;
}

int mi_adsr_bank_needs_update(const mi_adsr_bank_t *b, uint32_t channel, int *yes)
{
    const int r = mi_bank::get_checks(b, "mi_adsr_bank_needs_update", channel, yes);
    if (r == MI_OK)
        *yes = (b->cfg[channel].flags & MI_ADSR_RECONFIGURE) ? 1 : 0;
    return r;
}

int mi_adsr_bank_update_settings(mi_adsr_bank_t *b, void *stream)
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_adsr_bank_update_settings: NULL bank");
    return update(b, mi::as_stream(stream));
}

int mi_adsr_bank_set_row_enabled(mi_adsr_bank_t *b, uint32_t channel, int enabled)
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_adsr_bank_set_row_enabled: NULL bank");
    MI_REQUIRE(channel < b->channels, MI_EINVAL, "mi_adsr_bank_set_row_enabled: channel %u out of range", channel);
    const uint8_t on = enabled != 0;
    if (b->enabled[channel] != on)
        b->disabled += uint32_t(b->enabled[channel]) - on, b->enabled[channel] = on;
    return MI_OK;
}

int mi_adsr_bank_process(mi_adsr_bank_t *b, float *dst, const float *src, size_t count, size_t dst_stride, size_t src_stride, void *stream)
{
    return run(b, "mi_adsr_bank_process", OP_PROCESS, dst, src, nullptr, nullptr, count, dst_stride, src_stride, stream);
}

int mi_adsr_bank_process_mul(mi_adsr_bank_t *b, float *dst, const float *src, size_t count, size_t dst_stride, size_t src_stride, void *stream)
{
    return run(b, "mi_adsr_bank_process_mul", OP_PROCESS_MUL, dst, src, nullptr, nullptr, count, dst_stride, src_stride, stream);
}

int mi_adsr_bank_generate(mi_adsr_bank_t *b, float *dst, const float *start, const float *step, size_t count, size_t dst_stride, void *stream)
{
    return run(b, "mi_adsr_bank_generate", OP_GENERATE, dst, nullptr, start, step, count, dst_stride, 0, stream);
}

int mi_adsr_bank_generate_mul(mi_adsr_bank_t *b, float *dst, const float *src, const float *start, const float *step, size_t count,
                              size_t dst_stride, size_t src_stride, void *stream)
{
    return run(b, "mi_adsr_bank_generate_mul", (src != nullptr) ? OP_GENERATE_MUL_SRC : OP_GENERATE_MUL, dst, src, start, step, count,
               dst_stride, src_stride, stream);
}

} // extern "C"
