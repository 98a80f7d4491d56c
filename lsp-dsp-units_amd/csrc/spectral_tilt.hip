// mi_spectral_tilt_bank -- `channels` x lsp::dspu::SpectralTilt (reference: src/main/filters/SpectralTilt.cpp): an exponentially spaced
// pole / zero cascade of up to 64 biquads per channel.  The design is the host's (csrc/host/spectral_tilt.cpp); the cascade runs on a
// mi_biquad_bank of 64 sections that this bank owns, in that bank's exact or fast mode.  What is here is what the reference's three
// process entries make of their operands -- the second operand is dst itself --:
//   overwrite   dst = filter(src); a NULL src: zero fill; a bypassed channel: copy
//   add         dst = dst + filter(src); a NULL src: nothing; a bypassed channel: dst += src
//   mul         dst = dst * filter(src); a NULL src: zero fill; a bypassed channel: dst *= src
// A bypassed channel's row is switched off in the biquad bank -- the reference does not touch sFilter there, so the filter memory and
// the sections stay -- and tilt_combine_kernel serves it.  Add and mul filter into a scratch row and then combine.
//
//   tilt_combine_kernel<OP, VEC>   grid (tiles of 1024 samples, channels), four adjacent samples per lane: dst = a OP b, where b is
//       the scratch row of a filtering channel and the source row of a bypassed one; everything is read before anything is stored, so
//       dst may be a or b.  OP overwrite copies b (bypassed channels only).  The NoiseGenerator bank uses it for dst = src OP noise.
#include "bank_core.h"

#include <vector>

#pragma clang fp contract(off)

namespace
{
    constexpr int      BLOCK = 256;
    constexpr uint32_t PER = 4;
    constexpr uint32_t SECTIONS = MI_STLT_MAX_SECTIONS;
    constexpr size_t   COUNT_LIMIT = size_t(1) << 31;           // sample indices are 32-bit
    enum { TILT_OFF, TILT_FILTER, TILT_BYPASS };

    template <int OP, bool VEC>
    __global__ __launch_bounds__(BLOCK) void tilt_combine_kernel(float *dst, const float *a, const float *filtered, const float *bypassed,
                                                                 size_t dst_stride, size_t a_stride, size_t filtered_stride, size_t bypassed_stride,
                                                                 uint32_t count, const uint32_t *__restrict__ mode)
    {
        const uint32_t ch = blockIdx.y, m = (mode != nullptr) ? mode[ch] : uint32_t(TILT_FILTER);
        if (m == TILT_OFF || (OP == MI_OSC_OVERWRITE && m != TILT_BYPASS))
            return;
        const uint32_t i0 = (blockIdx.x * BLOCK + threadIdx.x) * PER;
        if (i0 >= count)
            return;
        const float *b = ((m == TILT_BYPASS) ? bypassed + size_t(ch) * bypassed_stride : filtered + size_t(ch) * filtered_stride) + i0;
        float *out = dst + size_t(ch) * dst_stride + i0;
        const bool whole = i0 + PER <= count;
        float v[PER] = { 0.0f, 0.0f, 0.0f, 0.0f }, s[PER] = { 0.0f, 0.0f, 0.0f, 0.0f };
        if (VEC && whole)
        {
            const float4 q = *reinterpret_cast<const float4 *>(b);
            v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
        }
        else
            for (uint32_t k = 0; k < PER && i0 + k < count; ++k)
                v[k] = b[k];
        if (OP != MI_OSC_OVERWRITE)
        {
            const float *in = a + size_t(ch) * a_stride + i0;
            if (VEC && whole)
            {
                const float4 q = *reinterpret_cast<const float4 *>(in);
                s[0] = q.x, s[1] = q.y, s[2] = q.z, s[3] = q.w;
            }
            else
                for (uint32_t k = 0; k < PER && i0 + k < count; ++k)
                    s[k] = in[k];
            #pragma unroll
            for (uint32_t k = 0; k < PER; ++k)
                v[k] = (OP == MI_OSC_ADD) ? s[k] + v[k] : s[k] * v[k];
        }
        if (VEC && whole)
            *reinterpret_cast<float4 *>(out) = make_float4(v[0], v[1], v[2], v[3]);
        else
            for (uint32_t k = 0; k < PER && i0 + k < count; ++k)
                out[k] = v[k];
    }
} // namespace

namespace mi
{
    // dst = a OP b over `channels` rows of `count` samples (count != 0); b: `filtered`, or `bypassed` where mode[ch] says so, and
    // channels whose mode is off are left out; mode == NULL: every channel takes `filtered`.  A NULL row pointer is one no channel takes.
    int rows_combine(float *dst, const float *a, const float *filtered, const float *bypassed, size_t dst_stride, size_t a_stride,
                     size_t filtered_stride, size_t bypassed_stride, size_t count, uint32_t op, const uint32_t *d_mode, uint32_t channels,
                     hipStream_t st)
    {
        const bool vec = aligned16(dst, dst_stride, channels) && (a == nullptr || aligned16(a, a_stride, channels)) &&
                         (filtered == nullptr || aligned16(filtered, filtered_stride, channels)) &&
                         (bypassed == nullptr || aligned16(bypassed, bypassed_stride, channels));
        const dim3 grid(uint32_t((count + BLOCK * PER - 1) / (BLOCK * PER)), channels), block(BLOCK);
        hipEvent_t ev0 = nullptr, ev1 = nullptr;
        take_profile_events(&ev0, &ev1);
        #define TILT_COMBINE(OP, VEC) \
            MI_LAUNCH((tilt_combine_kernel<OP, VEC>), grid, block, 0, st, ev0, ev1, dst, a, filtered, bypassed, dst_stride, a_stride, \
                      filtered_stride, bypassed_stride, uint32_t(count), d_mode)
        if (op == MI_OSC_ADD && vec)        TILT_COMBINE(MI_OSC_ADD, true);
        else if (op == MI_OSC_ADD)          TILT_COMBINE(MI_OSC_ADD, false);
        else if (op == MI_OSC_MUL && vec)   TILT_COMBINE(MI_OSC_MUL, true);
        else if (op == MI_OSC_MUL)          TILT_COMBINE(MI_OSC_MUL, false);
        else if (vec)                       TILT_COMBINE(MI_OSC_OVERWRITE, true);
        else                                TILT_COMBINE(MI_OSC_OVERWRITE, false);
        #undef TILT_COMBINE
        MI_HIP_CHECK(hipGetLastError());
        return MI_OK;
    }

    // rows of a bank's scratch: [channels][stride], stride a multiple of four floats and at least count; grown outside a capture
    int scratch_reserve(const char *bank, float **d_scratch, size_t *stride, uint32_t channels, size_t count, hipStream_t st)
    {
        if (count <= *stride)
            return MI_OK;
        bool cap = false;
        const int r = capturing(st, &cap);
        if (r != MI_OK)
            return r;
        MI_REQUIRE(!cap, MI_ESTATE, "%s: the scratch rows have to grow to %zu samples; call reserve() before capturing", bank, count);
        const size_t want = (count + 3) & ~size_t(3);
        float *fresh = nullptr;
        MI_HIP_CHECK(hipMalloc(reinterpret_cast<void **>(&fresh), size_t(channels) * want * sizeof(float)));
        if (*d_scratch != nullptr)
        {
            MI_HIP_CHECK(hipDeviceSynchronize());               // launches that still read the old rows
            (void)hipFree(*d_scratch);
        }
        *d_scratch = fresh, *stride = want;
        return MI_OK;
    }
} // namespace mi

struct mi_spectral_tilt_bank
{
    uint32_t                                    channels = 0;
    std::vector<mi_spectral_tilt_settings_t>    cfg;
    std::vector<uint8_t>                        enabled;
    std::vector<uint32_t>                       mode;           // TILT_*: what the device table holds, or will after the upload
    mi::dirty_range                             up;
    uint32_t                                   *d_mode = nullptr;
    uint32_t                                    filtering = 0, bypassed = 0;    // channels of either mode
    bool                                        touched = true;                 // a setter ran since the modes were last made
    mi_biquad_bank_t                           *biquads = nullptr;
    float                                      *d_scratch = nullptr;            // [channels][scratch_stride]
    size_t                                      scratch_stride = 0;
};

namespace
{
    // update_settings() of one channel; a new design goes to the biquad bank with end(true)
    int update_channel(mi_spectral_tilt_bank *b, uint32_t ch)
    {
        mi_spectral_tilt_settings_t &c = b->cfg[ch];
        if (!c.sync)
            return MI_OK;
        int designed = 0;
        int r = mi_spectral_tilt_settings_update(&c, &designed);
        if (r == MI_OK && designed)
            r = mi_biquad_bank_set_chains(b->biquads, ch, c.sections, c.n_sections, 1);
        b->touched = true;
        return r;
    }

    // update_settings() of every channel, or (running: the process entries open with it) of those that are switched on; then every
    // channel's mode, the biquad bank's rows to match, and the changed modes and sections go to the device
    int tilt_update(mi_spectral_tilt_bank *b, hipStream_t st, bool running)
    {
        if (b->touched)
        {
            b->touched = false;
            bool left = false;
            b->filtering = b->bypassed = 0;
            for (uint32_t ch = 0; ch < b->channels; ++ch)
            {
                if (!running || b->enabled[ch])
                {
                    const int r = update_channel(b, ch);
                    if (r != MI_OK)
                        return r;
                }
                else
                    left |= b->cfg[ch].sync != 0;
                const uint32_t m = !b->enabled[ch] ? uint32_t(TILT_OFF) : b->cfg[ch].bypass ? uint32_t(TILT_BYPASS) : uint32_t(TILT_FILTER);
                b->filtering += m == TILT_FILTER, b->bypassed += m == TILT_BYPASS;
                if (m == b->mode[ch])
                    continue;
                b->mode[ch] = m, b->up.touch(ch);
                const int r = mi_biquad_bank_set_row_enabled(b->biquads, ch, m == TILT_FILTER);
                if (r != MI_OK)
                    return r;
            }
            b->touched = left;
        }
        const int r = mi::upload_dirty("mi_spectral_tilt_bank", b->d_mode, b->mode.data(), b->up, st);
        return (r != MI_OK) ? r : mi_biquad_bank_commit(b->biquads, st);
    }

    int zero_rows(mi_spectral_tilt_bank *b, float *dst, size_t count, size_t dst_stride, hipStream_t st)
    {
        if (b->channels == 1)                                   // one row: its stride says nothing
            MI_HIP_CHECK(hipMemsetAsync(dst, 0, count * sizeof(float), st));
        else if (b->filtering + b->bypassed == b->channels)
            MI_HIP_CHECK(hipMemset2DAsync(dst, dst_stride * sizeof(float), 0, count * sizeof(float), b->channels, st));
        else
            for (uint32_t ch = 0; ch < b->channels; ++ch)
                if (b->enabled[ch])
                    MI_HIP_CHECK(hipMemsetAsync(dst + size_t(ch) * dst_stride, 0, count * sizeof(float), st));
        return MI_OK;
    }
} // namespace

extern "C" {

int mi_spectral_tilt_bank_create(mi_spectral_tilt_bank_t **bank, uint32_t channels)
{
    int r = mi_bank::open(bank, "mi_spectral_tilt_bank_create", channels, 65535u);     // tilt_combine_kernel's grid.y
    if (r != MI_OK)
        return r;
    mi_spectral_tilt_bank *b = *bank;
    *bank = nullptr;
    b->channels = channels;
    mi_spectral_tilt_settings_t fresh;
    mi_spectral_tilt_settings_init(&fresh);
    b->cfg.assign(channels, fresh);
    b->enabled.assign(channels, 1);
    b->mode.assign(channels, TILT_FILTER);
    b->filtering = channels;
    r = mi_biquad_bank_create(&b->biquads, channels, SECTIONS);        // init(): sFilter.init(MAX_ORDER)
    if (r == MI_OK)
    {
        hipError_t e = hipMalloc(reinterpret_cast<void **>(&b->d_mode), size_t(channels) * sizeof(uint32_t));
        if (e == hipSuccess)
            e = hipMemcpy(b->d_mode, b->mode.data(), size_t(channels) * sizeof(uint32_t), hipMemcpyHostToDevice);
        if (e != hipSuccess)
            r = mi::fail(MI_EHIP, "mi_spectral_tilt_bank_create: %s", hipGetErrorString(e));
    }
    if (r != MI_OK)
    {
        mi_spectral_tilt_bank_destroy(b);
        return r;
    }
    *bank = b;
    return MI_OK;
}

int mi_spectral_tilt_bank_destroy(mi_spectral_tilt_bank_t *b)
{
    if (b == nullptr)
        return MI_OK;
    mi_biquad_bank_destroy(b->biquads);
    (void)hipFree(b->d_mode); (void)hipFree(b->d_scratch);
    delete b;
    return MI_OK;
}

#define TILT_SETTER(name, call) \
    MI_BANK_SETTER("spectral_tilt", name); \
    b->touched = true; \
    return call

int mi_spectral_tilt_bank_set_order(mi_spectral_tilt_bank_t *b, uint32_t channel, size_t order)
{
    TILT_SETTER("set_order", mi_spectral_tilt_settings_set_order(&c, order));
}

int mi_spectral_tilt_bank_set_slope(mi_spectral_tilt_bank_t *b, uint32_t channel, float slope, uint32_t unit)
{
    TILT_SETTER("set_slope", mi_spectral_tilt_settings_set_slope(&c, slope, unit));
}

int mi_spectral_tilt_bank_set_norm(mi_spectral_tilt_bank_t *b, uint32_t channel, uint32_t norm)
{
    TILT_SETTER("set_norm", mi_spectral_tilt_settings_set_norm(&c, norm));
}

int mi_spectral_tilt_bank_set_lower_frequency(mi_spectral_tilt_bank_t *b, uint32_t channel, float lower)
{
    TILT_SETTER("set_lower_frequency", mi_spectral_tilt_settings_set_lower_frequency(&c, lower));
}

int mi_spectral_tilt_bank_set_upper_frequency(mi_spectral_tilt_bank_t *b, uint32_t channel, float upper)
{
    TILT_SETTER("set_upper_frequency", mi_spectral_tilt_settings_set_upper_frequency(&c, upper));
}

int mi_spectral_tilt_bank_set_frequency_range(mi_spectral_tilt_bank_t *b, uint32_t channel, float lower, float upper)
{
    TILT_SETTER("set_frequency_range", mi_spectral_tilt_settings_set_frequency_range(&c, lower, upper));
}

int mi_spectral_tilt_bank_set_sample_rate(mi_spectral_tilt_bank_t *b, uint32_t channel, size_t sample_rate)
{
    TILT_SETTER("set_sample_rate", mi_spectral_tilt_settings_set_sample_rate(&c, sample_rate));
}

int mi_spectral_tilt_bank_set_row_enabled(mi_spectral_tilt_bank_t *b, uint32_t channel, int enabled)
{
    MI_BANK_SETTER("spectral_tilt", "set_row_enabled");
    (void)c;
    if (b->enabled[channel] != uint8_t(enabled != 0))
        b->enabled[channel] = enabled != 0, b->touched = true;
    return MI_OK;
}

int mi_spectral_tilt_bank_set_exact(mi_spectral_tilt_bank_t *b, int on)
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_spectral_tilt_bank_set_exact: NULL bank");
    return mi_biquad_bank_set_exact(b->biquads, on);
}

int mi_spectral_tilt_bank_update_settings(mi_spectral_tilt_bank_t *b, void *stream)
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_spectral_tilt_bank_update_settings: NULL bank");
    return tilt_update(b, mi::as_stream(stream), false);
}

int mi_spectral_tilt_bank_commit(mi_spectral_tilt_bank_t *b, void *stream)
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_spectral_tilt_bank_commit: NULL bank");
    return tilt_update(b, mi::as_stream(stream), true);
}

int mi_spectral_tilt_bank_reserve(mi_spectral_tilt_bank_t *b, size_t count, void *stream)
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_spectral_tilt_bank_reserve: NULL bank");
    MI_REQUIRE(count < COUNT_LIMIT, MI_EINVAL, "mi_spectral_tilt_bank_reserve: count %zu too large", count);
    return mi::scratch_reserve("mi_spectral_tilt_bank", &b->d_scratch, &b->scratch_stride, b->channels, count, mi::as_stream(stream));
}

int mi_spectral_tilt_bank_process(mi_spectral_tilt_bank_t *b, float *dst, const float *src, size_t count, size_t dst_stride, size_t src_stride,
                                  uint32_t op, void *stream)
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_spectral_tilt_bank_process: NULL bank");
    MI_REQUIRE(op <= MI_OSC_MUL, MI_EINVAL, "mi_spectral_tilt_bank_process: no operation %u", op);
    if (count == 0)
        return MI_OK;
    int r = mi_bank::check_rows("mi_spectral_tilt_bank_process", b->channels, count, COUNT_LIMIT,
                                { { dst, dst_stride, count, mi_bank::REQUIRED | mi_bank::OUTPUT }, { src, src_stride, count, 0 } });
    if (r != MI_OK)
        return r;
    if (b->channels == 1)                                       // one row: its strides say nothing (the biquad bank asks for them all the same)
        dst_stride = src_stride = count;
    hipStream_t st = mi::as_stream(stream);
    r = tilt_update(b, st, true);                               // every process entry opens with update_settings()
    if (r != MI_OK || b->filtering + b->bypassed == 0)
        return r;
    if (src == nullptr)                                         // :381-386, :413-418, :445-446
        return (op == MI_OSC_ADD) ? MI_OK : zero_rows(b, dst, count, dst_stride, st);
    if (op == MI_OSC_OVERWRITE)
    {
        if (b->filtering != 0)
            r = mi_biquad_bank_process(b->biquads, dst, src, count, dst_stride, src_stride, stream);
        if (r == MI_OK && b->bypassed != 0 && dst != src)
            r = mi::rows_combine(dst, nullptr, nullptr, src, dst_stride, 0, 0, src_stride, count, op, b->d_mode, b->channels, st);
        return r;
    }
    if (b->filtering != 0)
    {
        r = mi::scratch_reserve("mi_spectral_tilt_bank", &b->d_scratch, &b->scratch_stride, b->channels, count, st);
        if (r == MI_OK)
            r = mi_biquad_bank_process(b->biquads, b->d_scratch, src, count, b->scratch_stride, src_stride, stream);
        if (r != MI_OK)
            return r;
    }
    return mi::rows_combine(dst, dst, b->d_scratch, src, dst_stride, dst_stride, b->scratch_stride, src_stride, count, op, b->d_mode, b->channels, st);
}

int mi_spectral_tilt_bank_get_chains(const mi_spectral_tilt_bank_t *b, uint32_t channel, mi_biquad_x1_t *chains, uint32_t *count)
{
    const int r = mi_bank::get_checks(b, "mi_spectral_tilt_bank_get_chains", channel, count);
    if (r != MI_OK)
        return r;
    const mi_spectral_tilt_settings_t &c = b->cfg[channel];
    *count = c.n_sections;
    if (chains != nullptr)
        memcpy(chains, c.sections, size_t(c.n_sections) * sizeof(mi_biquad_x1_t));
    return MI_OK;
}

int mi_spectral_tilt_bank_get_settings(const mi_spectral_tilt_bank_t *b, uint32_t channel, mi_spectral_tilt_settings_t *settings)
{
    const int r = mi_bank::get_checks(b, "mi_spectral_tilt_bank_get_settings", channel, settings);
    if (r == MI_OK)
        *settings = b->cfg[channel];
    return r;
}

static int tilt_chart(mi_spectral_tilt_bank_t *b, const char *entry, uint32_t channel, float *re, float *im, float *c, const float *f, size_t count)
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "%s: NULL bank", entry);
    MI_REQUIRE(channel < b->channels, MI_EINVAL, "%s: channel %u out of range", entry, channel);
    const int r = update_channel(b, channel);                   // freq_chart() opens with update_settings(): :507, :515
    return (r != MI_OK) ? r : mi_spectral_tilt_settings_freq_chart(&b->cfg[channel], re, im, c, f, count);
}

int mi_spectral_tilt_bank_freq_chart(mi_spectral_tilt_bank_t *b, uint32_t channel, float *re, float *im, const float *f, size_t count)
{
    MI_REQUIRE(count == 0 || (re != nullptr && im != nullptr), MI_EINVAL, "mi_spectral_tilt_bank_freq_chart: NULL buffer");
    return tilt_chart(b, "mi_spectral_tilt_bank_freq_chart", channel, re, im, nullptr, f, count);
}

int mi_spectral_tilt_bank_freq_chart_packed(mi_spectral_tilt_bank_t *b, uint32_t channel, float *c, const float *f, size_t count)
{
    MI_REQUIRE(count == 0 || c != nullptr, MI_EINVAL, "mi_spectral_tilt_bank_freq_chart_packed: NULL buffer");
    return tilt_chart(b, "mi_spectral_tilt_bank_freq_chart_packed", channel, nullptr, nullptr, c, f, count);
}

int mi_spectral_tilt_bank_reset(mi_spectral_tilt_bank_t *b, uint32_t channel, void *stream)
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_spectral_tilt_bank_reset: NULL bank");
    MI_REQUIRE(channel < b->channels || channel == UINT32_MAX, MI_EINVAL, "mi_spectral_tilt_bank_reset: channel %u out of range", channel);
    return mi_biquad_bank_reset(b->biquads, channel, stream);
}

// one channel's filter memory out of (into) the biquad bank's, whose accessors move the whole bank's
static int tilt_state(mi_spectral_tilt_bank_t *b, const char *entry, uint32_t channel, float *get, const float *set, void *stream)
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "%s: NULL bank", entry);
    MI_REQUIRE(channel < b->channels && (get != nullptr || set != nullptr), MI_EINVAL, "%s: bad argument", entry);
    int r = mi::refuse_state_access(mi::as_stream(stream));
    if (r != MI_OK)
        return r;
    std::vector<float> all(size_t(b->channels) * SECTIONS * 2);
    r = mi_biquad_bank_get_state(b->biquads, all.data(), stream);
    if (r != MI_OK)
        return r;
    float *mine = all.data() + size_t(channel) * SECTIONS * 2;
    if (get != nullptr)
        memcpy(get, mine, SECTIONS * 2 * sizeof(float));
    if (set == nullptr)
        return MI_OK;
    memcpy(mine, set, SECTIONS * 2 * sizeof(float));
    return mi_biquad_bank_set_state(b->biquads, all.data(), stream);
}

int mi_spectral_tilt_bank_get_state(mi_spectral_tilt_bank_t *b, uint32_t channel, float *memory, void *stream)
{
    return tilt_state(b, "mi_spectral_tilt_bank_get_state", channel, memory, nullptr, stream);
}

int mi_spectral_tilt_bank_set_state(mi_spectral_tilt_bank_t *b, uint32_t channel, const float *memory, void *stream)
{
    return tilt_state(b, "mi_spectral_tilt_bank_set_state", channel, nullptr, memory, stream);
}

} // extern "C"
