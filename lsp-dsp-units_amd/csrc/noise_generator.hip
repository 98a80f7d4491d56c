// mi_noise_generator_bank -- `channels` x lsp::dspu::NoiseGenerator (reference: src/main/noise/Generator.cpp): the three noise sources
// behind one interface and a SpectralTilt that colours them.  The bank owns a mi_mls_bank, a mi_lcg_bank, a mi_velvet_bank and a
// mi_spectral_tilt_bank of `channels` rows each; it has no kernel of its own but the combine launch it shares with the tilt bank
// (mi::rows_combine, spectral_tilt.hip).  What is here is NoiseGenerator::update_settings() per channel on the host, and the routing
// of a call: the channels sorted by enGenerator, exactly those rows switched on in each source bank, source banks without a row not
// launched, white rows switched off in the tilt bank.
//   overwrite, add with src == NULL    sources -> dst (one segment of count), tilt in place on dst
//   add, mul with a source             sources -> scratch (Velvet in segments of 256: every chunk of the reference's loop restarts its
//                                      window scan), tilt in place on scratch, dst = src OP scratch.  The scratch is never "0 + noise":
//                                      (+0) + (-0) would lose the sign that add3(dst, vTemp, src) keeps.
//   mul with src == NULL               zero fill
#include "bank_core.h"

#include <cmath>
#include <vector>

#pragma clang fp contract(off)

namespace
{
    constexpr size_t COUNT_LIMIT = MI_VN_MAX_COUNT + 1;         // the Velvet bank's

    bool coloured(uint32_t color)                               // do_process()'s second switch, Generator.cpp:365-378
    {
        return color >= MI_NG_COLOR_PINK && color <= MI_NG_COLOR_ARBITRARY;
    }
    uint32_t source_of(uint32_t generator)                      // ... and its first, :349-363: default: is the LCG
    {
        return (generator == MI_NG_GEN_MLS || generator == MI_NG_GEN_VELVET) ? generator : uint32_t(MI_NG_GEN_LCG);
    }
} // namespace

struct mi_noise_generator_bank
{
    uint32_t                                    channels = 0;
    std::vector<mi_noise_generator_settings_t>  cfg;
    mi_mls_bank_t                              *mls = nullptr;
    mi_lcg_bank_t                              *lcg = nullptr;
    mi_velvet_bank_t                           *velvet = nullptr;
    mi_spectral_tilt_bank_t                    *tilt = nullptr;
    uint32_t                                    uninited = 0;                   // channels without an init()
    bool                                        pending = true;                 // some channel's nUpdate is not 0
    bool                                        rerouted = true;                // a generator or a colour changed since the rows were sorted
    uint32_t                                    rows[3] = { 0, 0, 0 };          // rows of MLS, LCG, Velvet
    uint32_t                                    coloured_rows = 0;
    float                                      *d_scratch = nullptr;            // [channels][scratch_stride]
    size_t                                      scratch_stride = 0;
};

namespace
{
    #define NG_TRY(call) do { const int r_ = (call); if (r_ != MI_OK) return r_; } while (0)

    // update_settings() of one channel, Generator.cpp:259-345
    int update_channel(mi_noise_generator_bank *b, uint32_t ch)
    {
        mi_noise_generator_settings_t &c = b->cfg[ch];
        if (!c.update)
            return MI_OK;
        NG_TRY(mi_mls_bank_set_amplitude(b->mls, ch, c.amplitude));
        NG_TRY(mi_mls_bank_set_offset(b->mls, ch, c.offset));
        if (c.update & MI_NG_UPD_MLS)
        {
            NG_TRY(mi_mls_bank_set_n_bits(b->mls, ch, c.mls_n_bits));
            NG_TRY(mi_mls_bank_set_state(b->mls, ch, c.mls_seed));
        }
        NG_TRY(mi_lcg_bank_set_amplitude(b->lcg, ch, c.amplitude));
        NG_TRY(mi_lcg_bank_set_offset(b->lcg, ch, c.offset));
        if (c.update & MI_NG_UPD_LCG)
            NG_TRY(mi_lcg_bank_set_distribution(b->lcg, ch, c.lcg_distribution));
        NG_TRY(mi_velvet_bank_set_amplitude(b->velvet, ch, c.amplitude));
        NG_TRY(mi_velvet_bank_set_offset(b->velvet, ch, c.offset));
        if (c.update & MI_NG_UPD_VELVET)
        {
            const float sr = c.sample_rate;                     // seconds_to_samples(float sr, float time)
            NG_TRY(mi_velvet_bank_set_core_type(b->velvet, ch, c.velvet_core));
            NG_TRY(mi_velvet_bank_set_velvet_type(b->velvet, ch, c.velvet_type));
            NG_TRY(mi_velvet_bank_set_velvet_window_width(b->velvet, ch, c.velvet_window_width_s * sr));
            NG_TRY(mi_velvet_bank_set_delta_value(b->velvet, ch, c.velvet_arn_delta));
            NG_TRY(mi_velvet_bank_set_crush(b->velvet, ch, int(c.velvet_crush)));
            NG_TRY(mi_velvet_bank_set_crush_probability(b->velvet, ch, c.velvet_crush_prob));
        }
        if (c.update & MI_NG_UPD_COLOR)
        {
            NG_TRY(mi_spectral_tilt_bank_set_sample_rate(b->tilt, ch, c.sample_rate));
            float slope = 0.0f;
            uint32_t unit = MI_STLT_SLOPE_UNIT_NEPER_PER_NEPER;
            switch (c.color)
            {
                case MI_NG_COLOR_PINK:      slope = -0.5f; break;
                case MI_NG_COLOR_RED:       slope = -1.0f; break;
                case MI_NG_COLOR_BLUE:      slope = 0.5f; break;
                case MI_NG_COLOR_VIOLET:    slope = 1.0f; break;
                case MI_NG_COLOR_ARBITRARY: slope = c.color_slope, unit = c.color_slope_unit; break;
                default:                    break;
            }
            NG_TRY(mi_spectral_tilt_bank_set_order(b->tilt, ch, c.color_order));
            NG_TRY(mi_spectral_tilt_bank_set_slope(b->tilt, ch, slope, unit));
            NG_TRY(mi_spectral_tilt_bank_set_lower_frequency(b->tilt, ch, 10.0f));
            NG_TRY(mi_spectral_tilt_bank_set_upper_frequency(b->tilt, ch, 0.9f * 0.5f * c.sample_rate));
        }
        c.update = 0;
        return MI_OK;
    }

    int update_all(mi_noise_generator_bank *b)
    {
        for (uint32_t ch = 0; b->pending && ch < b->channels; ++ch)
            NG_TRY(update_channel(b, ch));
        b->pending = false;
        return MI_OK;
    }

    // exactly the rows of a generator are on in its bank; exactly the coloured rows are on in the tilt bank
    int route(mi_noise_generator_bank *b)
    {
        if (!b->rerouted)
            return MI_OK;
        b->rows[0] = b->rows[1] = b->rows[2] = b->coloured_rows = 0;
        for (uint32_t ch = 0; ch < b->channels; ++ch)
        {
            const uint32_t g = source_of(b->cfg[ch].generator);
            const bool col = coloured(b->cfg[ch].color);
            b->rows[g] += 1, b->coloured_rows += col;
            NG_TRY(mi_mls_bank_set_row_enabled(b->mls, ch, g == MI_NG_GEN_MLS));
            NG_TRY(mi_lcg_bank_set_row_enabled(b->lcg, ch, g == MI_NG_GEN_LCG));
            NG_TRY(mi_velvet_bank_set_row_enabled(b->velvet, ch, g == MI_NG_GEN_VELVET));
            NG_TRY(mi_spectral_tilt_bank_set_row_enabled(b->tilt, ch, col));
        }
        b->rerouted = false;
        return MI_OK;
    }

    // do_process(rows, count) of every channel, Generator.cpp:347-379
    int draw(mi_noise_generator_bank *b, float *rows, size_t count, size_t stride, bool segmented, void *stream)
    {
        if (b->rows[MI_NG_GEN_MLS] != 0)
            NG_TRY(mi_mls_bank_process(b->mls, rows, nullptr, count, stride, 0, MI_OSC_OVERWRITE, stream));
        if (b->rows[MI_NG_GEN_LCG] != 0)
            NG_TRY(mi_lcg_bank_process(b->lcg, rows, nullptr, count, stride, 0, MI_OSC_OVERWRITE, stream));
        if (b->rows[MI_NG_GEN_VELVET] != 0)
            NG_TRY(segmented ? mi_velvet_bank_process_segmented(b->velvet, rows, count, stride, stream)
                             : mi_velvet_bank_process(b->velvet, rows, nullptr, count, stride, 0, MI_OSC_OVERWRITE, stream));
        if (b->coloured_rows != 0)
            NG_TRY(mi_spectral_tilt_bank_process(b->tilt, rows, rows, count, stride, stride, MI_OSC_OVERWRITE, stream));
        return MI_OK;
    }
} // namespace

extern "C" {

int mi_noise_generator_bank_create(mi_noise_generator_bank_t **bank, uint32_t channels)
{
    int r = mi_bank::open(bank, "mi_noise_generator_bank_create", channels, 65535u);       // the MLS bank's
    if (r != MI_OK)
        return r;
    mi_noise_generator_bank *b = *bank;
    *bank = nullptr;
    b->channels = channels;
    mi_noise_generator_settings_t c = mi_noise_generator_settings_t();     // construct(), Generator.cpp:44-78
    c.lcg_distribution = MI_LCG_UNIFORM;
    c.velvet_core = MI_VN_CORE_LCG, c.velvet_type = MI_VN_VELVET_OVN;
    c.velvet_window_width_s = 0.1f, c.velvet_arn_delta = 0.5f, c.velvet_crush = 0, c.velvet_crush_prob = 0.5f;
    c.color = MI_NG_COLOR_WHITE, c.color_order = 50, c.color_slope = 0.0f, c.color_slope_unit = MI_STLT_SLOPE_UNIT_NEPER_PER_NEPER;
    c.sample_rate = 0, c.generator = MI_NG_GEN_LCG, c.amplitude = 1.0f, c.offset = 0.0f;
    c.update = MI_NG_UPD_ALL;
    b->cfg.assign(channels, c);
    b->uninited = channels;
    r = mi_mls_bank_create(&b->mls, channels);
    if (r == MI_OK) r = mi_lcg_bank_create(&b->lcg, channels);
    if (r == MI_OK) r = mi_velvet_bank_create(&b->velvet, channels);
    if (r == MI_OK) r = mi_spectral_tilt_bank_create(&b->tilt, channels);
    if (r != MI_OK)
    {
        mi_noise_generator_bank_destroy(b);
        return r;
    }
    *bank = b;
    return MI_OK;
}

int mi_noise_generator_bank_destroy(mi_noise_generator_bank_t *b)
{
    if (b == nullptr)
        return MI_OK;
    mi_mls_bank_destroy(b->mls);
    mi_lcg_bank_destroy(b->lcg);
    mi_velvet_bank_destroy(b->velvet);
    mi_spectral_tilt_bank_destroy(b->tilt);
    (void)hipFree(b->d_scratch);
    delete b;
    return MI_OK;
}

int mi_noise_generator_bank_init(mi_noise_generator_bank_t *b, uint32_t channel, uint32_t mls_n_bits, uint64_t mls_seed, uint32_t lcg_seed,
                                 uint32_t velvet_rand_seed, uint32_t velvet_mls_n_bits, uint64_t velvet_mls_seed)      // :88-108
{
    MI_BANK_SETTER("noise_generator", "init");
    c.mls_n_bits = uint8_t(mls_n_bits), c.mls_seed = mls_seed;
    c.lcg_seed = lcg_seed;
    NG_TRY(mi_lcg_bank_init(b->lcg, channel, lcg_seed));
    c.velvet_rand_seed = velvet_rand_seed, c.velvet_mls_n_bits = uint8_t(velvet_mls_n_bits), c.velvet_mls_seed = velvet_mls_seed;
    NG_TRY(mi_velvet_bank_init(b->velvet, channel, velvet_rand_seed, uint8_t(velvet_mls_n_bits), velvet_mls_seed));
    NG_TRY(mi_spectral_tilt_bank_set_norm(b->tilt, channel, MI_STLT_NORM_AUTO));
    c.update = MI_NG_UPD_ALL, b->pending = true;
    b->uninited -= c.inited ? 0u : 1u, c.inited = 1;
    return MI_OK;
}

int mi_noise_generator_bank_init_auto(mi_noise_generator_bank_t *b, uint32_t channel)       // :110-122
{
    MI_BANK_SETTER("noise_generator", "init_auto");
    c.mls_n_bits = 64, c.mls_seed = 0;                          // maximum_number_of_bits(); 0 forces the default seed
    NG_TRY(mi_lcg_bank_init_time(b->lcg, channel));
    NG_TRY(mi_velvet_bank_init_time(b->velvet, channel));
    NG_TRY(mi_spectral_tilt_bank_set_norm(b->tilt, channel, MI_STLT_NORM_AUTO));
    c.update = MI_NG_UPD_ALL, b->pending = true;
    b->uninited -= c.inited ? 0u : 1u, c.inited = 1;
    return MI_OK;
}

// a setter of the reference: nothing happens if the value is the member's, otherwise the member is set and `bits` are raised
#define NG_SETTER(name, same, assign, bits) \
    MI_BANK_SETTER("noise_generator", name); \
    if (same) \
        return MI_OK; \
    assign; \
    c.update |= (bits), b->pending = true; \
    return MI_OK

int mi_noise_generator_bank_set_sample_rate(mi_noise_generator_bank_t *b, uint32_t channel, size_t sample_rate)
{
    NG_SETTER("set_sample_rate", c.sample_rate == sample_rate, c.sample_rate = sample_rate, MI_NG_UPD_COLOR | MI_NG_UPD_VELVET);
}

int mi_noise_generator_bank_set_mls_n_bits(mi_noise_generator_bank_t *b, uint32_t channel, uint32_t n_bits)
{
    NG_SETTER("set_mls_n_bits", uint8_t(n_bits) == c.mls_n_bits, c.mls_n_bits = uint8_t(n_bits), MI_NG_UPD_MLS);
}

int mi_noise_generator_bank_set_mls_seed(mi_noise_generator_bank_t *b, uint32_t channel, uint64_t seed)
{
    NG_SETTER("set_mls_seed", seed == c.mls_seed, c.mls_seed = seed, MI_NG_UPD_MLS);
}

int mi_noise_generator_bank_set_lcg_distribution(mi_noise_generator_bank_t *b, uint32_t channel, uint32_t distribution)
{
    NG_SETTER("set_lcg_distribution", distribution == c.lcg_distribution, c.lcg_distribution = distribution, MI_NG_UPD_LCG);
}

int mi_noise_generator_bank_set_velvet_type(mi_noise_generator_bank_t *b, uint32_t channel, uint32_t type)
{
    NG_SETTER("set_velvet_type", type == c.velvet_type, c.velvet_type = type, MI_NG_UPD_VELVET);
}

int mi_noise_generator_bank_set_velvet_window_width(mi_noise_generator_bank_t *b, uint32_t channel, float seconds)
{
    MI_REQUIRE(std::isfinite(seconds), MI_EINVAL, "mi_noise_generator_bank_set_velvet_window_width: the width is not finite");
    NG_SETTER("set_velvet_window_width", seconds == c.velvet_window_width_s, c.velvet_window_width_s = seconds, MI_NG_UPD_VELVET);
}

int mi_noise_generator_bank_set_velvet_arn_delta(mi_noise_generator_bank_t *b, uint32_t channel, float delta)
{
    NG_SETTER("set_velvet_arn_delta", delta == c.velvet_arn_delta, c.velvet_arn_delta = delta, MI_NG_UPD_VELVET);
}

int mi_noise_generator_bank_set_velvet_crush(mi_noise_generator_bank_t *b, uint32_t channel, int crush)
{
    NG_SETTER("set_velvet_crush", uint32_t(crush != 0) == c.velvet_crush, c.velvet_crush = crush != 0, MI_NG_UPD_VELVET);
}

int mi_noise_generator_bank_set_velvet_crushing_probability(mi_noise_generator_bank_t *b, uint32_t channel, float prob)
{
    NG_SETTER("set_velvet_crushing_probability", prob == c.velvet_crush_prob, c.velvet_crush_prob = prob, MI_NG_UPD_VELVET);
}

int mi_noise_generator_bank_set_generator(mi_noise_generator_bank_t *b, uint32_t channel, uint32_t generator)      // raises nothing, :205-211
{
    MI_BANK_SETTER("noise_generator", "set_generator");
    if (generator != c.generator)
        c.generator = generator, b->rerouted = true;
    return MI_OK;
}

int mi_noise_generator_bank_set_noise_color(mi_noise_generator_bank_t *b, uint32_t channel, uint32_t color)
{
    NG_SETTER("set_noise_color", color == c.color, (c.color = color, b->rerouted = true), MI_NG_UPD_COLOR);
}

int mi_noise_generator_bank_set_coloring_order(mi_noise_generator_bank_t *b, uint32_t channel, size_t order)
{
    NG_SETTER("set_coloring_order", order == c.color_order, c.color_order = order, MI_NG_UPD_COLOR);
}

int mi_noise_generator_bank_set_color_slope(mi_noise_generator_bank_t *b, uint32_t channel, float slope, uint32_t unit)
{
    NG_SETTER("set_color_slope", (slope == c.color_slope) && (unit == c.color_slope_unit), (c.color_slope = slope, c.color_slope_unit = unit),
              MI_NG_UPD_COLOR);
}

int mi_noise_generator_bank_set_amplitude(mi_noise_generator_bank_t *b, uint32_t channel, float amplitude)
{
    NG_SETTER("set_amplitude", amplitude == c.amplitude, c.amplitude = amplitude, MI_NG_UPD_OTHER);
}

int mi_noise_generator_bank_set_offset(mi_noise_generator_bank_t *b, uint32_t channel, float offset)
{
    NG_SETTER("set_offset", offset == c.offset, c.offset = offset, MI_NG_UPD_OTHER);
}

int mi_noise_generator_bank_set_exact(mi_noise_generator_bank_t *b, int on)
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_noise_generator_bank_set_exact: NULL bank");
    return mi_spectral_tilt_bank_set_exact(b->tilt, on);
}

int mi_noise_generator_bank_update_settings(mi_noise_generator_bank_t *b, void *stream)
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_noise_generator_bank_update_settings: NULL bank");
    NG_TRY(update_all(b));
    NG_TRY(route(b));
    // what the units would send with their next launch goes now.  Their own update_settings() are those of the rows that are on: an
    // idle MLS and the colour filter of a white channel keep theirs pending, as in the reference
    NG_TRY(mi_mls_bank_commit(b->mls, stream));
    NG_TRY(mi_lcg_bank_commit(b->lcg, stream));
    NG_TRY(mi_velvet_bank_commit(b->velvet, stream));
    return mi_spectral_tilt_bank_commit(b->tilt, stream);
}

int mi_noise_generator_bank_reserve(mi_noise_generator_bank_t *b, size_t count, void *stream)
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_noise_generator_bank_reserve: NULL bank");
    MI_REQUIRE(count < COUNT_LIMIT, MI_EINVAL, "mi_noise_generator_bank_reserve: count %zu too large", count);
    return mi::scratch_reserve("mi_noise_generator_bank", &b->d_scratch, &b->scratch_stride, b->channels, count, mi::as_stream(stream));
}

int mi_noise_generator_bank_process(mi_noise_generator_bank_t *b, float *dst, const float *src, size_t count, size_t dst_stride,
                                    size_t src_stride, uint32_t op, void *stream)
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_noise_generator_bank_process: NULL bank");
    MI_REQUIRE(op <= MI_OSC_MUL, MI_EINVAL, "mi_noise_generator_bank_process: no operation %u", op);
    if (op == MI_OSC_OVERWRITE)
        src = nullptr;
    if (count == 0)
        return MI_OK;
    NG_TRY(mi_bank::check_rows("mi_noise_generator_bank_process", b->channels, count, COUNT_LIMIT,
                               { { dst, dst_stride, count, mi_bank::REQUIRED | mi_bank::OUTPUT }, { src, src_stride, count, 0 } }));
    for (uint32_t ch = 0; (b->uninited != 0 || b->pending) && ch < b->channels; ++ch)
    {
        const mi_noise_generator_settings_t &c = b->cfg[ch];
        MI_REQUIRE(c.inited, MI_ESTATE, "mi_noise_generator_bank_process: channel %u was never init()ed", ch);
        MI_REQUIRE(!coloured(c.color) || c.sample_rate != 0, MI_ESTATE,
                   "mi_noise_generator_bank_process: channel %u is coloured and has sample rate 0; the colour filter cannot be designed", ch);
    }
    NG_TRY(update_all(b));
    hipStream_t st = mi::as_stream(stream);
    if (src == nullptr && op == MI_OSC_MUL)                     // noise * 0: fill_zero and not a draw, :411-416
    {
        if (b->channels == 1)                                   // one row: its stride says nothing
            MI_HIP_CHECK(hipMemsetAsync(dst, 0, count * sizeof(float), st));
        else
            MI_HIP_CHECK(hipMemset2DAsync(dst, dst_stride * sizeof(float), 0, count * sizeof(float), b->channels, st));
        return MI_OK;
    }
    NG_TRY(route(b));
    if (src == nullptr)                                         // process_overwrite(), and process_add() without a source, :385-390
        return draw(b, dst, count, dst_stride, false, stream);
    NG_TRY(mi::scratch_reserve("mi_noise_generator_bank", &b->d_scratch, &b->scratch_stride, b->channels, count, st));
    NG_TRY(draw(b, b->d_scratch, count, b->scratch_stride, true, stream));
    return mi::rows_combine(dst, src, b->d_scratch, nullptr, dst_stride, src_stride, b->scratch_stride, 0, count, op, nullptr, b->channels, st);
}

static int ng_chart(mi_noise_generator_bank_t *b, const char *entry, uint32_t channel, float *re, float *im, float *c, const float *f, size_t count)
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "%s: NULL bank", entry);
    MI_REQUIRE(channel < b->channels, MI_EINVAL, "%s: channel %u out of range", entry, channel);
    MI_REQUIRE(count == 0 || (f != nullptr && (c != nullptr || (re != nullptr && im != nullptr))), MI_EINVAL, "%s: NULL buffer", entry);
    if (coloured(b->cfg[channel].color))                        // :440-477
        return (c != nullptr) ? mi_spectral_tilt_bank_freq_chart_packed(b->tilt, channel, c, f, count)
                              : mi_spectral_tilt_bank_freq_chart(b->tilt, channel, re, im, f, count);
    for (size_t i = 0; i < count; ++i)
        if (c != nullptr)
            c[2 * i] = 1.0f, c[2 * i + 1] = 0.0f;
        else
            re[i] = 1.0f, im[i] = 0.0f;
    return MI_OK;
}

int mi_noise_generator_bank_freq_chart(mi_noise_generator_bank_t *b, uint32_t channel, float *re, float *im, const float *f, size_t count)
{
    return ng_chart(b, "mi_noise_generator_bank_freq_chart", channel, re, im, nullptr, f, count);
}

int mi_noise_generator_bank_freq_chart_packed(mi_noise_generator_bank_t *b, uint32_t channel, float *c, const float *f, size_t count)
{
    return ng_chart(b, "mi_noise_generator_bank_freq_chart_packed", channel, nullptr, nullptr, c, f, count);
}

int mi_noise_generator_bank_get_settings(const mi_noise_generator_bank_t *b, uint32_t channel, mi_noise_generator_settings_t *settings)
{
    const int r = mi_bank::get_checks(b, "mi_noise_generator_bank_get_settings", channel, settings);
    if (r == MI_OK)
        *settings = b->cfg[channel];
    return r;
}

int mi_noise_generator_bank_get_tilt_settings(const mi_noise_generator_bank_t *b, uint32_t channel, mi_spectral_tilt_settings_t *settings)
{
    const int r = mi_bank::get_checks(b, "mi_noise_generator_bank_get_tilt_settings", channel, settings);
    return (r != MI_OK) ? r : mi_spectral_tilt_bank_get_settings(b->tilt, channel, settings);
}

int mi_noise_generator_bank_get_state(mi_noise_generator_bank_t *b, uint32_t channel, mi_noise_generator_state_t *state, void *stream)
{
    const int r = mi_bank::get_checks(b, "mi_noise_generator_bank_get_state", channel, state);
    if (r != MI_OK)
        return r;
    NG_TRY(mi::refuse_state_access(mi::as_stream(stream)));
    *state = mi_noise_generator_state_t();
    mi_mls_settings_t ms;
    NG_TRY(mi_lcg_bank_get_state(b->lcg, channel, &state->lcg, stream));
    NG_TRY(mi_mls_bank_get_state(b->mls, channel, &state->mls_state, stream));
    NG_TRY(mi_mls_bank_get_settings(b->mls, channel, &ms));
    state->mls_n_bits = ms.n_bits;
    NG_TRY(mi_velvet_bank_get_state(b->velvet, channel, &state->velvet, stream));
    return mi_spectral_tilt_bank_get_state(b->tilt, channel, state->filter, stream);
}

int mi_noise_generator_bank_set_state(mi_noise_generator_bank_t *b, uint32_t channel, const mi_noise_generator_state_t *state, void *stream)
{
    const int r = mi_bank::get_checks(b, "mi_noise_generator_bank_set_state", channel, state);
    if (r != MI_OK)
        return r;
    NG_TRY(mi::refuse_state_access(mi::as_stream(stream)));
    NG_TRY(mi_lcg_bank_set_state(b->lcg, channel, &state->lcg, stream));
    NG_TRY(mi_mls_bank_set_n_bits(b->mls, channel, state->mls_n_bits));
    NG_TRY(mi_mls_bank_set_state(b->mls, channel, state->mls_state));
    NG_TRY(mi_velvet_bank_set_state(b->velvet, channel, &state->velvet, stream));
    return mi_spectral_tilt_bank_set_state(b->tilt, channel, state->filter, stream);
}

} // extern "C"
