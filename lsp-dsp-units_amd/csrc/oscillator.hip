// mi_oscillator_bank -- `channels` x lsp::dspu::Oscillator (reference: src/main/util/Oscillator.cpp:359-633): waveforms from a
// uint32_t phase accumulator that a constant advances, nPhaseAcc = (nPhaseAcc + nFreqCtrlWord) & nPhaseAccMask.  The phase of
// sample i of a call is therefore (p0 + i w) & mask in closed form -- the multiplication wraps as the additions would, and the
// mask keeps the low bits -- and the value of a sample depends on its phase alone: every sample of every channel is independent.
//
//   oscillator_kernel<OP, VEC>   grid (tiles of TILE samples, channels); a lane owns 4 consecutive samples and, where the rows
//       allow it (VEC), stores them as 16 bytes.  The channel's record (function, words, coefficients; osc_params) is read through
//       a pointer that depends on blockIdx alone: uniform, so it sits in SGPRs, and the switch on the function is a scalar branch.
//       OP is overwrite, add or mul; add and mul read their four src values before anything is stored, so dst may be src.  A
//       channel with a BL function writes N x count values with the step nFreqCtrlWord / N into the bank's scratch rows instead.
//   oscillator_advance_kernel    one thread per channel, behind the tiles on the stream: nPhaseAcc = (p0 + n w) & mask, and the
//       pending phase change is marked as taken.  A follow-up launch and not a last-tile-done counter: the stream orders it
//       behind every tile with no atomics and no fence, it is capturable like any launch, and it costs a launch of `channels`
//       threads.
//   oscillator_combine_kernel<OP>  BL only: dst = src OP (the downsampled row) for the BL channels, where the downsampler could
//       not write to dst itself (add, mul, or a bank with both kinds of channels).
//
// A pending phase change (update_settings :164-166, reset_phase_accumulator, a new accumulator width or rate) travels in the
// record: known == 1: nPhaseAcc is `phase`; known == 0: it is (the device's + phase) & mask.  The host never reads the phase.
//
// Sinusoids: the argument is the reference's float product; the value is the float64 sine of it rounded once to float32 (S*):
// sin(double) is good to under an ulp of double, so its rounding differs from S* only where the true sine lies within about
// 2^-29 ulp(float) of a rounding boundary.  Everything else is float arithmetic in the reference's order, contraction off.
#include "bank_core.h"

#include <cmath>
#include <vector>

#pragma clang fp contract(off)

namespace
{
    constexpr int      BLOCK = 256;
    constexpr uint32_t PER = 4, TILE = BLOCK * PER;
    constexpr size_t   COUNT_LIMIT = size_t(1) << 27;           // N * count stays below 2^30: sample indices are 32-bit
    constexpr uint32_t MAX_TIMES = 8;
    constexpr uint32_t PERIODS_BUF = 12 * 1024;                 // PROCESS_BUF_LIMIT_SIZE, Oscillator.cpp:26

    // what the kernel needs of one channel; n[] and f[] by function:
    //   sine, cosine            f = { A, dc, fAcc2Phase }
    //   squared sine, cosine    f = { sq.fAmplitude, dc, 0.5f * fAcc2Phase }
    //   rectangular             n = { nDutyWord }           f = { A, dc, fBLPeakAtten }
    //   sawtooth                n = { nWidthWord }          f = { c0, c1, c2, c3, dc, fBLPeakAtten }
    //   trapezoid               n = nPoints                 f = { c0, c1, c2, c3, dc, A, fBLPeakAtten }
    //   pulsetrain              n = nTrainPoints            f = { A, dc, fBLPeakAtten }
    //   parabolic               n = { nWidthWord }          f = { par.fAmplitude, dc, 2.0f / nWidthWord, fBLPeakAtten }
    struct osc_params
    {
        uint32_t function, mask, step, times;                   // step: nFreqCtrlWord, or nFreqCtrlWord_Over for a BL function
        uint32_t n[4];
        float    f[8];
        uint32_t known, phase;                                  // the pending phase change
        uint32_t pad[2];
    };
    struct osc_state { uint32_t acc; };

    __device__ __forceinline__ bool bl(uint32_t fn) { return fn >= MI_FG_BL_RECTANGULAR; }

    __device__ __forceinline__ uint32_t start_phase(const osc_params &P, const osc_state *state, uint32_t ch)
    {
        return P.known ? P.phase : (state[ch].acc + P.phase) & P.mask;
    }

    __device__ __forceinline__ float sine_star(float x)   { return float(sin(double(x))); }
    __device__ __forceinline__ float cosine_star(float x) { return float(cos(double(x))); }

    // one branch of do_process, :367-632, at one phase
    template <int FN> __device__ __forceinline__ float wave(const osc_params &P, uint32_t ph)
    {
        const float pf = __uint2float_rn(ph);
        const float *f = P.f;
        if (FN == MI_FG_SINE)                                   // :372
            return f[0] * sine_star(f[2] * pf) + f[1];
        if (FN == MI_FG_COSINE)                                 // :380
            return f[0] * cosine_star(f[2] * pf) + f[1];
        if (FN == MI_FG_SQUARED_SINE || FN == MI_FG_SQUARED_COSINE)     // :390-391, :401-402
        {
            const float x = (FN == MI_FG_SQUARED_SINE) ? sine_star(f[2] * pf) : cosine_star(f[2] * pf);
            return f[0] * x * x + f[1];
        }
        if (FN == MI_FG_RECTANGULAR)                            // :410
            return ((ph < P.n[0]) ? f[0] : -f[0]) + f[1];
        if (FN == MI_FG_BL_RECTANGULAR)                         // :490
            return f[2] * (((ph < P.n[0]) ? f[0] : -f[0]) + f[1]);
        if (FN == MI_FG_SAWTOOTH || FN == MI_FG_BL_SAWTOOTH)    // :418-421, :514-517
        {
            const float v = (ph < P.n[0]) ? f[0] * pf + f[1] + f[4] : f[2] * pf + f[3] + f[4];
            return (FN == MI_FG_BL_SAWTOOTH) ? f[5] * v : v;
        }
        if (FN == MI_FG_TRAPEZOID || FN == MI_FG_BL_TRAPEZOID)  // :430-443, :542-555: the first branch that holds
        {
            float v;
            if (ph < P.n[0])
                v = f[0] * pf + f[4];
            else if (ph <= P.n[1])
                v = f[5] + f[4];
            else if (ph < P.n[2])                               // ph > n[1] here
                v = f[1] * pf + f[2] + f[4];
            else if (ph <= P.n[3])                              // ph >= n[2] here
                v = f[4] - f[5];
            else
                v = f[0] * pf + f[3] + f[4];
            return (FN == MI_FG_BL_TRAPEZOID) ? f[6] * v : v;
        }
        if (FN == MI_FG_PULSETRAIN)                             // :453-458
            return (ph <= P.n[0]) ? f[0] + f[1] : ((ph >= P.n[1]) && (ph <= P.n[2])) ? f[1] - f[0] : 0.0f + f[1];
        if (FN == MI_FG_BL_PULSETRAIN)                          // :580-585: the else branch is not scaled
            return (ph <= P.n[0]) ? f[2] * (f[0] + f[1]) : ((ph >= P.n[1]) && (ph <= P.n[2])) ? f[2] * (f[1] - f[0]) : 0.0f + f[1];
        if (FN == MI_FG_PARABOLIC || FN == MI_FG_BL_PARABOLIC)  // :467-473, :610-616: the else branch is not scaled
        {
            if (ph < P.n[0])
            {
                const float x = f[2] * pf - 1.0f;
                const float v = f[0] * (1.0f - x * x) + f[1];
                return (FN == MI_FG_BL_PARABOLIC) ? f[3] * v : v;
            }
            return 0.0f + f[1];
        }
        return 0.0f;
    }

    template <int FN> __device__ __forceinline__ void wave4(const osc_params &P, uint32_t p, float (&v)[PER])
    {
        #pragma unroll
        for (uint32_t k = 0; k < PER; ++k)
            v[k] = wave<FN>(P, (p + k * P.step) & P.mask);
    }

    template <int OP, bool VEC>
    __global__ __launch_bounds__(BLOCK) void oscillator_kernel(float *dst, const float *src, size_t dst_stride, size_t src_stride,
                                                               uint32_t count, const osc_params *__restrict__ params,
                                                               const osc_state *__restrict__ state, float *__restrict__ synth,
                                                               size_t synth_stride)
    {
        const uint32_t ch = blockIdx.y;
        const osc_params P = params[ch];
        const bool to_synth = bl(P.function);
        const uint32_t n = to_synth ? P.times * count : count;
        const uint32_t i0 = (blockIdx.x * BLOCK + threadIdx.x) * PER;
        if (i0 >= n)
            return;
        const uint32_t p = start_phase(P, state, ch) + i0 * P.step;     // wraps as the additions would; masked per sample
        float v[PER];
        switch (P.function)
        {
            case MI_FG_SINE:            wave4<MI_FG_SINE>(P, p, v); break;
            case MI_FG_COSINE:          wave4<MI_FG_COSINE>(P, p, v); break;
            case MI_FG_SQUARED_SINE:    wave4<MI_FG_SQUARED_SINE>(P, p, v); break;
            case MI_FG_SQUARED_COSINE:  wave4<MI_FG_SQUARED_COSINE>(P, p, v); break;
            case MI_FG_RECTANGULAR:     wave4<MI_FG_RECTANGULAR>(P, p, v); break;
            case MI_FG_SAWTOOTH:        wave4<MI_FG_SAWTOOTH>(P, p, v); break;
            case MI_FG_TRAPEZOID:       wave4<MI_FG_TRAPEZOID>(P, p, v); break;
            case MI_FG_PULSETRAIN:      wave4<MI_FG_PULSETRAIN>(P, p, v); break;
            case MI_FG_PARABOLIC:       wave4<MI_FG_PARABOLIC>(P, p, v); break;
            case MI_FG_BL_RECTANGULAR:  wave4<MI_FG_BL_RECTANGULAR>(P, p, v); break;
            case MI_FG_BL_SAWTOOTH:     wave4<MI_FG_BL_SAWTOOTH>(P, p, v); break;
            case MI_FG_BL_TRAPEZOID:    wave4<MI_FG_BL_TRAPEZOID>(P, p, v); break;
            case MI_FG_BL_PULSETRAIN:   wave4<MI_FG_BL_PULSETRAIN>(P, p, v); break;
            default:                    wave4<MI_FG_BL_PARABOLIC>(P, p, v); break;
        }
        if (to_synth)                                           // rows of the bank: 16-byte aligned, a stride that is a multiple of 4
        {
            float *row = synth + size_t(ch) * synth_stride + i0;
            if (i0 + PER <= n)
                *reinterpret_cast<float4 *>(row) = make_float4(v[0], v[1], v[2], v[3]);
            else
                for (uint32_t k = 0; i0 + k < n; ++k)
                    row[k] = v[k];
            return;
        }
        float *out = dst + size_t(ch) * dst_stride + i0;
        const float *in = (OP != MI_OSC_OVERWRITE && src != nullptr) ? src + size_t(ch) * src_stride + i0 : nullptr;
        const bool whole = i0 + PER <= n;
        float s[PER] = { 0.0f, 0.0f, 0.0f, 0.0f };              // src == NULL: fill_zero, :698, :719
        if (OP != MI_OSC_OVERWRITE && in != nullptr)
        {
            if (VEC && whole)
            {
                const float4 q = *reinterpret_cast<const float4 *>(in);
                s[0] = q.x, s[1] = q.y, s[2] = q.z, s[3] = q.w;
            }
            else
                for (uint32_t k = 0; k < PER && i0 + k < n; ++k)
                    s[k] = in[k];
        }
        #pragma unroll
        for (uint32_t k = 0; k < PER; ++k)
            v[k] = (OP == MI_OSC_ADD) ? s[k] + v[k] : (OP == MI_OSC_MUL) ? s[k] * v[k] : v[k];     // add2 / mul2: dst OP synth
        if (VEC && whole)
            *reinterpret_cast<float4 *>(out) = make_float4(v[0], v[1], v[2], v[3]);
        else
            for (uint32_t k = 0; k < PER && i0 + k < n; ++k)
                out[k] = v[k];
    }

    __global__ __launch_bounds__(BLOCK) void oscillator_advance_kernel(osc_params *params, osc_state *state, uint32_t channels, uint32_t count)
    {
        const uint32_t ch = blockIdx.x * BLOCK + threadIdx.x;
        if (ch >= channels)
            return;
        osc_params &P = params[ch];
        const uint32_t n = bl(P.function) ? P.times * count : count;
        state[ch].acc = (start_phase(P, state, ch) + n * P.step) & P.mask;
        P.known = 0, P.phase = 0;
    }

    template <int OP>
    __global__ __launch_bounds__(BLOCK) void oscillator_combine_kernel(float *dst, const float *src, size_t dst_stride, size_t src_stride,
                                                                       uint32_t count, const osc_params *__restrict__ params,
                                                                       const float *__restrict__ down, size_t down_stride)
    {
        const uint32_t ch = blockIdx.y, i = blockIdx.x * BLOCK + threadIdx.x;
        if (!bl(params[ch].function) || i >= count)
            return;
        const float s = (OP != MI_OSC_OVERWRITE && src != nullptr) ? src[size_t(ch) * src_stride + i] : 0.0f;
        const float v = down[size_t(ch) * down_stride + i];
        dst[size_t(ch) * dst_stride + i] = (OP == MI_OSC_ADD) ? s + v : (OP == MI_OSC_MUL) ? s * v : v;
    }

    // get_periods' picks, :668: dst[k] = row[index[k]], 0.0f for a position outside the buffer (index < 0)
    __global__ __launch_bounds__(BLOCK) void oscillator_gather_kernel(float *__restrict__ dst, const float *__restrict__ row,
                                                                      const int32_t *__restrict__ index, uint32_t n)
    {
        const uint32_t k = blockIdx.x * BLOCK + threadIdx.x;
        if (k >= n)
            return;
        const int32_t at = index[k];
        dst[k] = (at >= 0 && at < int32_t(PERIODS_BUF)) ? row[at] : 0.0f;
    }

    inline size_t round4(size_t v) { return (v + 3) & ~size_t(3); }
} // namespace

struct mi_oscillator_bank : mi_bank::tables<osc_params, osc_state>
{
    std::vector<mi_oscillator_settings_t> cfg;
    mi_oversampler_bank_t  *over = nullptr;                 // sOver
    float                  *d_synth = nullptr, *d_down = nullptr;   // [channels][synth_stride], [channels][down_stride]
    size_t                  synth_stride = 0, down_stride = 0;      // floats per row, multiples of 4
    size_t                  last_count = 0;                         // of the last BL call
    // get_periods(): per channel, made at its first call: sOverGetPeriods and vSynthBuffer of that oscillator
    struct periods_unit { mi_oversampler_bank_t *over = nullptr; float *d_row = nullptr; };
    std::vector<periods_unit> periods;
    osc_params             *d_pparams = nullptr;                    // one record and one phase for the fills, a row of N x 12 Ki
    osc_state              *d_pstate = nullptr;                     // for their oversampled samples, the picks' indices
    float                  *d_psynth = nullptr;
    int32_t                *d_pindex = nullptr;
    size_t                  pindex_cap = 0;
    int                     exact = -1;                             // set_exact(), -1: the process-wide default
    bool                    any_bl = false, all_bl = false;
    uint32_t                times = 1;                              // of the BL channels
};

namespace
{
    constexpr const char *NAME = "mi_oscillator_bank";

    osc_params record_of(const mi_oscillator_settings_t &s)
    {
        osc_params p = osc_params();
        p.function = s.function, p.mask = s.mask;
        const bool over = s.function >= MI_FG_BL_RECTANGULAR;
        p.step = over ? s.freq_word_over : s.freq_word;
        p.times = over ? s.oversampling : 1;
        p.known = s.phase_known, p.phase = s.phase;
        switch (s.function)
        {
            case MI_FG_SINE: case MI_FG_COSINE:
                p.f[0] = s.amplitude, p.f[1] = s.referenced_dc, p.f[2] = s.acc2phase;
                break;
            case MI_FG_SQUARED_SINE: case MI_FG_SQUARED_COSINE:
                p.f[0] = s.sq_amplitude, p.f[1] = s.referenced_dc, p.f[2] = 0.5f * s.acc2phase;     // :390: the product comes first
                break;
            case MI_FG_RECTANGULAR: case MI_FG_BL_RECTANGULAR:
                p.n[0] = s.duty_word;
                p.f[0] = s.amplitude, p.f[1] = s.referenced_dc, p.f[2] = s.rect_atten;
                break;
            case MI_FG_SAWTOOTH: case MI_FG_BL_SAWTOOTH:
                p.n[0] = s.width_word;
                for (int k = 0; k < 4; ++k)
                    p.f[k] = s.saw_coeffs[k];
                p.f[4] = s.referenced_dc, p.f[5] = s.saw_atten;
                break;
            case MI_FG_TRAPEZOID: case MI_FG_BL_TRAPEZOID:
                for (int k = 0; k < 4; ++k)
                    p.n[k] = s.points[k], p.f[k] = s.trap_coeffs[k];
                p.f[4] = s.referenced_dc, p.f[5] = s.amplitude, p.f[6] = s.trap_atten;
                break;
            case MI_FG_PULSETRAIN: case MI_FG_BL_PULSETRAIN:
                for (int k = 0; k < 3; ++k)
                    p.n[k] = s.train[k];
                p.f[0] = s.amplitude, p.f[1] = s.referenced_dc, p.f[2] = s.pulse_atten;
                break;
            default:                                            // parabolic; :469: 2.0f / nWidthWord, an IEEE division on the host
                p.n[0] = s.par_word;
                p.f[0] = s.par_amplitude, p.f[1] = s.referenced_dc, p.f[2] = 2.0f / float(s.par_word), p.f[3] = s.par_atten;
                break;
        }
        return p;
    }

    int grow(mi_oscillator_bank *b, size_t count, uint32_t times, hipStream_t st)
    {
        const size_t ss = round4(count * times), ds = round4(count);
        if (ss <= b->synth_stride && ds <= b->down_stride)
            return MI_OK;
        bool cap = false;
        const int r = mi::capturing(st, &cap);
        if (r != MI_OK)
            return r;
        MI_REQUIRE(!cap, MI_ESTATE, "mi_oscillator_bank: the scratch rows have to grow; call reserve() before capturing");
        MI_HIP_CHECK(hipDeviceSynchronize());                   // launches in flight may still use the old rows
        const size_t ns = (ss > b->synth_stride) ? ss : b->synth_stride, nd = (ds > b->down_stride) ? ds : b->down_stride;
        (void)hipFree(b->d_synth); (void)hipFree(b->d_down);
        b->d_synth = nullptr, b->d_down = nullptr, b->synth_stride = 0, b->down_stride = 0;
        MI_HIP_CHECK(hipMalloc(reinterpret_cast<void **>(&b->d_synth), size_t(b->channels) * ns * sizeof(float)));
        MI_HIP_CHECK(hipMalloc(reinterpret_cast<void **>(&b->d_down), size_t(b->channels) * nd * sizeof(float)));
        // rows of channels without a BL function go through the downsampler unused: zeros, not whatever the memory held (a call's
        // rows are always synth_stride apart, so nothing else is ever written there)
        MI_HIP_CHECK(hipMemset(b->d_synth, 0, size_t(b->channels) * ns * sizeof(float)));
        MI_HIP_CHECK(hipMemset(b->d_down, 0, size_t(b->channels) * nd * sizeof(float)));
        MI_HIP_CHECK(hipDeviceSynchronize());                   // ... before a launch on any stream
        b->synth_stride = ns, b->down_stride = nd;
        return MI_OK;
    }

    // update_settings of every channel, the oversampler's part (:343-354) and the upload
    int update(mi_oscillator_bank *b, hipStream_t st)
    {
        for (uint32_t ch = 0; ch < b->channels; ++ch)
        {
            mi_oscillator_settings_t &c = b->cfg[ch];
            if (c.sync)
                mi_oscillator_settings_update(&c);
            const osc_params p = record_of(c);
            if (memcmp(&p, &b->params[ch], sizeof(p)) != 0)
                b->params[ch] = p, b->up.touch(ch);
        }
        uint32_t lead = 0, bls = 0;
        for (uint32_t ch = b->channels; ch-- > 0; )
            if (b->cfg[ch].function >= MI_FG_BL_RECTANGULAR)
                lead = ch, ++bls;
        const mi_oscillator_settings_t &l = b->cfg[lead];
        for (uint32_t ch = 0; ch < b->channels; ++ch)
            MI_REQUIRE(b->cfg[ch].function < MI_FG_BL_RECTANGULAR || (b->cfg[ch].over_mode == l.over_mode && b->cfg[ch].sample_rate == l.sample_rate),
                       MI_EINVAL, "mi_oscillator_bank_update_settings: channels %u and %u have band-limited functions but differ in sample "
                       "rate or oversampler mode; the bank has one oversampler", lead, ch);
        b->any_bl = bls != 0, b->all_bl = bls == b->channels, b->times = l.oversampling ? l.oversampling : 1;
        if (l.sample_rate <= UINT32_MAX)                          // (a rate that was never set is size_t(-1))
        {
            int r = mi_oversampler_bank_set_sample_rate(b->over, uint32_t(l.sample_rate));      // :343
            if (r == MI_OK) r = mi_oversampler_bank_set_mode(b->over, l.over_mode);             // :344
            int modified = 0;
            if (r == MI_OK) r = mi_oversampler_bank_modified(b->over, &modified);               // :345-346
            if (r == MI_OK && modified) r = mi_oversampler_bank_update_settings(b->over, st);
            if (r != MI_OK)
                return r;
        }
        return mi_bank::upload(*b, NAME, st);
    }

    template <int OP> void launch_main(mi_oscillator_bank *b, float *dst, const float *src, size_t dst_stride, size_t src_stride, uint32_t count,
                                       uint32_t tiles, bool vec, hipStream_t st, hipEvent_t ev0, hipEvent_t ev1)
    {
        const dim3 grid(tiles, b->channels), block(BLOCK);
        if (vec)
            MI_LAUNCH((oscillator_kernel<OP, true>), grid, block, 0, st, ev0, ev1, dst, src, dst_stride, src_stride, count, b->d_params, b->d_state,
                      b->d_synth, b->synth_stride);
        else
            MI_LAUNCH((oscillator_kernel<OP, false>), grid, block, 0, st, ev0, ev1, dst, src, dst_stride, src_stride, count, b->d_params, b->d_state,
                      b->d_synth, b->synth_stride);
    }
} // namespace

extern "C" {

int mi_oscillator_bank_create(mi_oscillator_bank_t **bank, uint32_t channels)
{
    int r = mi_bank::open(bank, "mi_oscillator_bank_create", channels, 65535u);
    if (r != MI_OK)
        return r;
    mi_oscillator_bank *b = *bank;
    *bank = nullptr;
    b->channels = channels;
    mi_oscillator_settings_t fresh;
    mi_oscillator_settings_init(&fresh);
    b->cfg.assign(channels, fresh);
    osc_params p = record_of(fresh);
    p.function = ~0u;                                       // no channel's record is what update_settings will make: all are sent
    r = mi_bank::alloc(*b, "mi_oscillator_bank_create", p, osc_state{ 0 });
    if (r == MI_OK)
        r = mi_oversampler_bank_create(&b->over, channels);
    if (r != MI_OK)
    {
        mi_oscillator_bank_destroy(b);
        return r;
    }
    *bank = b;
    return MI_OK;
}

int mi_oscillator_bank_destroy(mi_oscillator_bank_t *b)
{
    if (b == nullptr)
        return MI_OK;
    mi_oversampler_bank_destroy(b->over);
    for (mi_oscillator_bank::periods_unit &u : b->periods)
    {
        mi_oversampler_bank_destroy(u.over);
        (void)hipFree(u.d_row);
    }
    (void)hipFree(b->d_synth); (void)hipFree(b->d_down); (void)hipFree(b->d_pparams); (void)hipFree(b->d_pstate);
    (void)hipFree(b->d_psynth); (void)hipFree(b->d_pindex);
    return mi_bank::destroy(b);
}

int mi_oscillator_bank_set(mi_oscillator_bank_t *b, uint32_t channel, uint32_t setter, double x, double y)
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_oscillator_bank_set: NULL bank");
    MI_REQUIRE(channel < b->channels, MI_EINVAL, "mi_oscillator_bank_set: channel %u out of range", channel);
    return mi_oscillator_settings_set(&b->cfg[channel], setter, x, y);
}

#define OSC_SETTER(name, args, setter, x, y) \
    int mi_oscillator_bank_##name args \
    { \
        MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_oscillator_bank_" #name ": NULL bank"); \
        MI_REQUIRE(channel < b->channels, MI_EINVAL, "mi_oscillator_bank_" #name ": channel %u out of range", channel); \
        return mi_oscillator_settings_set(&b->cfg[channel], setter, x, y); \
    }
OSC_SETTER(set_function, (mi_oscillator_bank_t *b, uint32_t channel, uint32_t v), MI_OSC_SET_FUNCTION, v, 0)
OSC_SETTER(set_frequency, (mi_oscillator_bank_t *b, uint32_t channel, float v), MI_OSC_SET_FREQUENCY, v, 0)
OSC_SETTER(set_sample_rate, (mi_oscillator_bank_t *b, uint32_t channel, size_t v), MI_OSC_SET_SAMPLE_RATE, double(v), 0)
OSC_SETTER(set_phase, (mi_oscillator_bank_t *b, uint32_t channel, float v), MI_OSC_SET_PHASE, v, 0)
OSC_SETTER(set_phase_accumulator_bits, (mi_oscillator_bank_t *b, uint32_t channel, uint32_t v), MI_OSC_SET_PHASE_ACCUMULATOR_BITS, v, 0)
OSC_SETTER(set_dc_offset, (mi_oscillator_bank_t *b, uint32_t channel, float v), MI_OSC_SET_DC_OFFSET, v, 0)
OSC_SETTER(set_dc_reference, (mi_oscillator_bank_t *b, uint32_t channel, uint32_t v), MI_OSC_SET_DC_REFERENCE, v, 0)
OSC_SETTER(set_amplitude, (mi_oscillator_bank_t *b, uint32_t channel, float v), MI_OSC_SET_AMPLITUDE, v, 0)
OSC_SETTER(set_duty_ratio, (mi_oscillator_bank_t *b, uint32_t channel, float v), MI_OSC_SET_DUTY_RATIO, v, 0)
OSC_SETTER(set_width, (mi_oscillator_bank_t *b, uint32_t channel, float v), MI_OSC_SET_WIDTH, v, 0)
OSC_SETTER(set_trapezoid_ratios, (mi_oscillator_bank_t *b, uint32_t channel, float v, float w), MI_OSC_SET_TRAPEZOID_RATIOS, v, w)
OSC_SETTER(set_pulsetrain_ratios, (mi_oscillator_bank_t *b, uint32_t channel, float v, float w), MI_OSC_SET_PULSETRAIN_RATIOS, v, w)
OSC_SETTER(set_parabolic_width, (mi_oscillator_bank_t *b, uint32_t channel, float v), MI_OSC_SET_PARABOLIC_WIDTH, v, 0)
OSC_SETTER(set_squared_sinusoid_inversion, (mi_oscillator_bank_t *b, uint32_t channel, int v), MI_OSC_SET_SQUARED_SINUSOID_INVERSION, v != 0, 0)
OSC_SETTER(set_parabolic_inversion, (mi_oscillator_bank_t *b, uint32_t channel, int v), MI_OSC_SET_PARABOLIC_INVERSION, v != 0, 0)
OSC_SETTER(set_oversampler_mode, (mi_oscillator_bank_t *b, uint32_t channel, uint32_t v), MI_OSC_SET_OVERSAMPLER_MODE, v, 0)
OSC_SETTER(reset_phase_accumulator, (mi_oscillator_bank_t *b, uint32_t channel), MI_OSC_RESET_PHASE_ACCUMULATOR, 0, 0)
#undef OSC_SETTER

int mi_oscillator_bank_needs_update(const mi_oscillator_bank_t *b, uint32_t channel, int *yes)
{
    const int r = mi_bank::get_checks(b, "mi_oscillator_bank_needs_update", channel, yes);
    if (r == MI_OK)
        *yes = b->cfg[channel].sync ? 1 : 0;
    return r;
}

int mi_oscillator_bank_update_settings(mi_oscillator_bank_t *b, void *stream)
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_oscillator_bank_update_settings: NULL bank");
    return update(b, mi::as_stream(stream));
}

int mi_oscillator_bank_get_settings(const mi_oscillator_bank_t *b, uint32_t channel, mi_oscillator_settings_t *settings)
{
    const int r = mi_bank::get_checks(b, "mi_oscillator_bank_get_settings", channel, settings);
    if (r == MI_OK)
        *settings = b->cfg[channel];
    return r;
}

int mi_oscillator_bank_set_settings(mi_oscillator_bank_t *b, uint32_t channel, const mi_oscillator_settings_t *settings)
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_oscillator_bank_set_settings: NULL bank");
    MI_REQUIRE(channel < b->channels && settings != nullptr, MI_EINVAL, "mi_oscillator_bank_set_settings: bad argument");
    const uint32_t n = settings->oversampling;
    MI_REQUIRE(settings->function <= MI_FG_BL_PARABOLIC && settings->over_mode <= MI_OM_LANCZOS_8X24BIT && settings->bits <= 32 &&
               (n == 0 || n == 1 || n == 2 || n == 3 || n == 4 || n == 6 || n == 8), MI_EINVAL,
               "mi_oscillator_bank_set_settings: function %u, oversampler mode %u, %u bits or oversampling %u out of range",
               settings->function, settings->over_mode, settings->bits, n);
    b->cfg[channel] = *settings;
    return MI_OK;
}

int mi_oscillator_bank_get_exact_frequency(const mi_oscillator_bank_t *b, uint32_t channel, float *frequency)
{
    const int r = mi_bank::get_checks(b, "mi_oscillator_bank_get_exact_frequency", channel, frequency);
    if (r != MI_OK)
        return r;
    const mi_oscillator_settings_t &c = b->cfg[channel];
    *frequency = c.sample_rate * c.freq_word * (1.0f / (c.mask + 1.0f));                // .h:264: float(size_t * uint32_t) * float
    return MI_OK;
}

int mi_oscillator_bank_get_exact_phase(const mi_oscillator_bank_t *b, uint32_t channel, float *phase)
{
    const int r = mi_bank::get_checks(b, "mi_oscillator_bank_get_exact_phase", channel, phase);
    if (r != MI_OK)
        return r;
    const mi_oscillator_settings_t &c = b->cfg[channel];
    const double x = (c.mask + 1.0);                                                    // :761-762
    *phase = round(x * c.init_phase * 0.5f * 0.31830988618379067154) * (2.0 * 3.14159265358979323846 / x);
    return MI_OK;
}

int mi_oscillator_bank_reserve(mi_oscillator_bank_t *b, size_t count)
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_oscillator_bank_reserve: NULL bank");
    MI_REQUIRE(count < COUNT_LIMIT, MI_EINVAL, "mi_oscillator_bank_reserve: count %zu too large", count);
    const int r = grow(b, count, MAX_TIMES, nullptr);
    return (r != MI_OK) ? r : mi_oversampler_bank_reserve(b->over, count);
}

int mi_oscillator_bank_set_exact(mi_oscillator_bank_t *b, int on)
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_oscillator_bank_set_exact: NULL bank");
    b->exact = on != 0;
    for (mi_oscillator_bank::periods_unit &u : b->periods)
        if (u.over != nullptr)
            mi_oversampler_bank_set_exact(u.over, on);
    return mi_oversampler_bank_set_exact(b->over, on);
}

int mi_oscillator_bank_process(mi_oscillator_bank_t *b, float *dst, const float *src, size_t count, size_t dst_stride, size_t src_stride,
                               uint32_t op, void *stream)
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_oscillator_bank_process: NULL bank");
    MI_REQUIRE(op <= MI_OSC_MUL, MI_EINVAL, "mi_oscillator_bank_process: no operation %u", op);
    if (op == MI_OSC_OVERWRITE)
        src = nullptr;
    int r = (count == 0) ? MI_OK : mi_bank::check_rows("mi_oscillator_bank_process", b->channels, count, COUNT_LIMIT,
                                { { dst, dst_stride, count, mi_bank::REQUIRED | mi_bank::OUTPUT }, { src, src_stride, count, 0 } });
    if (r != MI_OK)
        return r;
    hipStream_t st = mi::as_stream(stream);
    r = update(b, st);                                      // :693, :714, :735
    if (r != MI_OK)
        return r;
    for (uint32_t ch = 0; ch < b->channels; ++ch)
        MI_REQUIRE(b->cfg[ch].sample_rate != UINT64_MAX || b->cfg[ch].unset_rate_ok, MI_ESTATE, "mi_oscillator_bank_process: the sample rate of channel %u was never set", ch);
    if (count == 0)
        return MI_OK;
    const uint32_t times = b->any_bl ? b->times : 1;
    if (b->any_bl)
    {
        r = grow(b, count, times, st);
        if (r != MI_OK)
            return r;
        b->last_count = count * times;
    }
    const uint32_t n = uint32_t(count), tiles = uint32_t((count * times + TILE - 1) / TILE);
    const bool vec = mi::aligned16(dst, dst_stride, b->channels) && (src == nullptr || mi::aligned16(src, src_stride, b->channels));
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    mi::take_profile_events(&ev0, &ev1);
    if (op == MI_OSC_ADD)
        launch_main<MI_OSC_ADD>(b, dst, src, dst_stride, src_stride, n, tiles, vec, st, ev0, ev1);
    else if (op == MI_OSC_MUL)
        launch_main<MI_OSC_MUL>(b, dst, src, dst_stride, src_stride, n, tiles, vec, st, ev0, ev1);
    else
        launch_main<MI_OSC_OVERWRITE>(b, dst, src, dst_stride, src_stride, n, tiles, vec, st, ev0, ev1);
    MI_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(oscillator_advance_kernel, dim3((b->channels + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, st, b->d_params, b->d_state, b->channels, n);
    MI_HIP_CHECK(hipGetLastError());
    for (uint32_t ch = 0; ch < b->channels; ++ch)           // as the advance kernel leaves the records
    {
        b->cfg[ch].phase_known = 0, b->cfg[ch].phase = 0;
        b->params[ch].known = 0, b->params[ch].phase = 0;
    }
    if (!b->any_bl)
        return MI_OK;
    // one downsample per call (:494 and its siblings chunk by PROCESS_BUF_LIMIT_SIZE / N; the filter's state runs on)
    if (b->all_bl && op == MI_OSC_OVERWRITE)
        return mi_oversampler_bank_downsample(b->over, dst, b->d_synth, count, dst_stride, b->synth_stride, stream);
    r = mi_oversampler_bank_downsample(b->over, b->d_down, b->d_synth, count, b->down_stride, b->synth_stride, stream);
    if (r != MI_OK)
        return r;
    const dim3 grid(uint32_t((count + BLOCK - 1) / BLOCK), b->channels);
    if (op == MI_OSC_ADD)
        hipLaunchKernelGGL(oscillator_combine_kernel<MI_OSC_ADD>, grid, dim3(BLOCK), 0, st, dst, src, dst_stride, src_stride, n, b->d_params, b->d_down, b->down_stride);
    else if (op == MI_OSC_MUL)
        hipLaunchKernelGGL(oscillator_combine_kernel<MI_OSC_MUL>, grid, dim3(BLOCK), 0, st, dst, src, dst_stride, src_stride, n, b->d_params, b->d_down, b->down_stride);
    else
        hipLaunchKernelGGL(oscillator_combine_kernel<MI_OSC_OVERWRITE>, grid, dim3(BLOCK), 0, st, dst, src, dst_stride, src_stride, n, b->d_params, b->d_down, b->down_stride);
    MI_HIP_CHECK(hipGetLastError());
    return MI_OK;
}

int mi_oscillator_bank_get_state(mi_oscillator_bank_t *b, uint32_t channel, mi_oscillator_state_t *state, void *stream)
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_oscillator_bank_get_state: NULL bank");
    MI_REQUIRE(state != nullptr, MI_EINVAL, "mi_oscillator_bank_get_state: NULL state");
    MI_REQUIRE(channel < b->channels, MI_EINVAL, "mi_oscillator_bank_get_state: channel %u out of range", channel);
    hipStream_t st = mi::as_stream(stream);
    int r = mi::refuse_state_access(st);
    if (r == MI_OK)
        r = update(b, st);                                  // a pending update_settings moves the phase (:164-166)
    if (r != MI_OK)
        return r;
    const mi_oscillator_settings_t &c = b->cfg[channel];
    if (c.phase_known)
    {
        state->phase = c.phase;
        return MI_OK;
    }
    osc_state s;
    r = mi_bank::get_state(b, "mi_oscillator_bank_get_state", channel, &s, stream);
    if (r == MI_OK)
        state->phase = (s.acc + c.phase) & c.mask;
    return r;
}

int mi_oscillator_bank_set_state(mi_oscillator_bank_t *b, uint32_t channel, const mi_oscillator_state_t *state, void *stream)
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_oscillator_bank_set_state: NULL bank");
    MI_REQUIRE(state != nullptr, MI_EINVAL, "mi_oscillator_bank_set_state: NULL state");
    MI_REQUIRE(channel < b->channels, MI_EINVAL, "mi_oscillator_bank_set_state: channel %u out of range", channel);
    const int r = mi::refuse_state_access(mi::as_stream(stream));
    if (r != MI_OK)
        return r;
    mi_oscillator_settings_t &c = b->cfg[channel];
    if (c.sync)
        mi_oscillator_settings_update(&c);                  // the mask that the phase lives under
    c.phase_known = 1, c.phase = state->phase & c.mask;     // travels with the next launch, like a reset
    return MI_OK;
}

int mi_oscillator_bank_get_periods(mi_oscillator_bank_t *b, uint32_t channel, float *dst, size_t periods, size_t periods_skip,
                                   size_t samples, void *stream)                             // :635-689
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_oscillator_bank_get_periods: NULL bank");
    MI_REQUIRE(channel < b->channels, MI_EINVAL, "mi_oscillator_bank_get_periods: channel %u out of range", channel);
    MI_REQUIRE(dst != nullptr || samples == 0, MI_EINVAL, "mi_oscillator_bank_get_periods: NULL buffer");
    MI_REQUIRE(samples < COUNT_LIMIT, MI_EINVAL, "mi_oscillator_bank_get_periods: %zu samples are too many", samples);
    hipStream_t st = mi::as_stream(stream);
    int r = mi::refuse_state_access(st);
    if (r == MI_OK)
        r = update(b, st);
    if (r != MI_OK || samples == 0)
        return r;
    const mi_oscillator_settings_t &c = b->cfg[channel];
    MI_REQUIRE(c.sample_rate != UINT64_MAX || c.unset_rate_ok, MI_ESTATE, "mi_oscillator_bank_get_periods: the sample rate of channel %u was never set",
               channel);
    const float duration = float(c.sample_rate) / c.frequency;                              // :640
    MI_REQUIRE(duration > 0.0f && !std::isinf(duration), MI_EINVAL,
               "mi_oscillator_bank_get_periods: a period of %g samples (the reference's loops do not end for it)", double(duration));
    const bool over = c.function >= MI_FG_BL_RECTANGULAR;
    const uint32_t times = over ? c.oversampling : 1;

    if (b->periods.empty())
        b->periods.resize(b->channels);
    mi_oscillator_bank::periods_unit &u = b->periods[channel];
    if (b->d_pparams == nullptr)
    {
        MI_HIP_CHECK(hipMalloc(reinterpret_cast<void **>(&b->d_pparams), sizeof(osc_params)));
        MI_HIP_CHECK(hipMalloc(reinterpret_cast<void **>(&b->d_pstate), sizeof(osc_state)));
        MI_HIP_CHECK(hipMalloc(reinterpret_cast<void **>(&b->d_psynth), size_t(MAX_TIMES) * PERIODS_BUF * sizeof(float)));
        MI_HIP_CHECK(hipMemset(b->d_pstate, 0, sizeof(osc_state)));
    }
    if (u.d_row == nullptr)
    {
        MI_HIP_CHECK(hipMalloc(reinterpret_cast<void **>(&u.d_row), PERIODS_BUF * sizeof(float)));
        MI_HIP_CHECK(hipMemset(u.d_row, 0, PERIODS_BUF * sizeof(float)));
        MI_HIP_CHECK(hipDeviceSynchronize());
    }
    if (over)
    {
        if (u.over == nullptr)
        {
            r = mi_oversampler_bank_create(&u.over, 1);
            if (r == MI_OK && b->exact >= 0)
                r = mi_oversampler_bank_set_exact(u.over, b->exact);
            if (r != MI_OK)
                return r;
        }
        if (c.sample_rate <= UINT32_MAX)                    // :348-351, here at the first use and whenever they changed
        {
            r = mi_oversampler_bank_set_sample_rate(u.over, uint32_t(c.sample_rate));
            if (r == MI_OK) r = mi_oversampler_bank_set_mode(u.over, c.over_mode);
            int modified = 0;
            if (r == MI_OK) r = mi_oversampler_bank_modified(u.over, &modified);
            if (r == MI_OK && modified) r = mi_oversampler_bank_update_settings(u.over, stream);
            if (r == MI_OK) r = mi_oversampler_bank_reserve(u.over, PERIODS_BUF);
            if (r != MI_OK)
                return r;
        }
    }
    if (samples > b->pindex_cap)
    {
        (void)hipFree(b->d_pindex);
        b->d_pindex = nullptr, b->pindex_cap = 0;
        MI_HIP_CHECK(hipMalloc(reinterpret_cast<void **>(&b->d_pindex), samples * sizeof(int32_t)));
        b->pindex_cap = samples;
    }

    // the fills run from a phase of their own that starts at nInitPhaseWord (:637-638); the streaming phase is not touched
    osc_params rec = b->params[channel];
    rec.known = 1, rec.phase = c.init_word;
    MI_HIP_CHECK(hipMemcpyAsync(b->d_pparams, &rec, sizeof(rec), hipMemcpyHostToDevice, st));
    MI_HIP_CHECK(hipStreamSynchronize(st));

    auto fill = [&](size_t to_do) -> int                    // do_process(&sOverGetPeriods, vSynthBuffer, to_do)
    {
        if (to_do == 0)
            return MI_OK;
        const uint32_t tiles = uint32_t((to_do * times + TILE - 1) / TILE);
        hipLaunchKernelGGL((oscillator_kernel<MI_OSC_OVERWRITE, true>), dim3(tiles, 1), dim3(BLOCK), 0, st, u.d_row, static_cast<const float *>(nullptr),
                           size_t(PERIODS_BUF), size_t(0), uint32_t(to_do), b->d_pparams, b->d_pstate, b->d_psynth, size_t(MAX_TIMES) * PERIODS_BUF);
        MI_HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(oscillator_advance_kernel, dim3(1), dim3(BLOCK), 0, st, b->d_pparams, b->d_pstate, 1u, uint32_t(to_do));
        MI_HIP_CHECK(hipGetLastError());
        return over ? mi_oversampler_bank_downsample(u.over, u.d_row, b->d_psynth, to_do, PERIODS_BUF, size_t(MAX_TIMES) * PERIODS_BUF, stream) : MI_OK;
    };
    std::vector<int32_t> index;
    size_t done = 0;
    auto flush = [&]() -> int                               // the picks out of the row as it stands
    {
        if (index.empty())
            return MI_OK;
        MI_HIP_CHECK(hipMemcpyAsync(b->d_pindex, index.data(), index.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(oscillator_gather_kernel, dim3(uint32_t((index.size() + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, st, dst + done, u.d_row,
                           b->d_pindex, uint32_t(index.size()));
        MI_HIP_CHECK(hipGetLastError());
        MI_HIP_CHECK(hipStreamSynchronize(st));
        done += index.size();
        index.clear();
        return MI_OK;
    };
    auto limited = [](float want) -> size_t                 // :652-654, :675-677: at most one buffer, none for a negative count
    {
        return (want >= float(PERIODS_BUF)) ? size_t(PERIODS_BUF) : (want > 0.0f) ? size_t(want) : 0;
    };

    float out_samples = duration * float(periods);          // :641-643
    float skip_samples = duration * float(periods_skip);
    const float step = out_samples / float(samples);
    ptrdiff_t buf_size = 0;
    while (skip_samples > 0.0f)                             // :649-660
    {
        const size_t to_do = limited(ceilf(out_samples + skip_samples + step));
        r = fill(to_do);
        if (r != MI_OK)
            return r;
        buf_size = ptrdiff_t(to_do);
        skip_samples -= to_do;
    }
    float t = buf_size + skip_samples;                      // :662
    size_t left = samples;
    while (left > 0)                                        // :664-686
    {
        if (t < buf_size)
        {
            // :668 reads vSynthBuffer[size_t(t)] whatever t is; a position in front of the buffer reads 0.0f here
            index.push_back((t >= 0.0f && t < float(PERIODS_BUF)) ? int32_t(t) : -1);
            t += step;
            left--;
        }
        else
        {
            r = flush();
            if (r != MI_OK)
                return r;
            const size_t to_do = limited(ceilf(out_samples + step));
            r = fill(to_do);
            if (r != MI_OK)
                return r;
            out_samples -= to_do;
            buf_size = PERIODS_BUF;
            t -= buf_size;
        }
    }
    return flush();
}

int mi_oscillator_bank_synth_rows(const mi_oscillator_bank_t *b, const float **rows, size_t *stride)
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_oscillator_bank_synth_rows: NULL bank");
    MI_REQUIRE(rows != nullptr && stride != nullptr, MI_EINVAL, "mi_oscillator_bank_synth_rows: NULL result pointer");
    *rows = b->d_synth, *stride = b->last_count ? b->synth_stride : 0;
    return MI_OK;
}

} // extern "C"
