// lsp::dspu::AutoGain and lsp::dspu::SimpleAutoGain as banks of `channels` units (src/main/dynamics/AutoGain.cpp,
// SimpleAutoGain.cpp): the kernels, and the two banks around them on the shared host core (bank_core.h): update() in host
// float32, the setters with the reference's rules and the entries.  The classes are host/autogain.cpp.
//
// Both are serial recurrences per channel whose branches depend on the running gain, with element-wise work beside them:
// the tile walk of tile_chain_device.h.  autogain_kernel keeps THREE input rows per channel in LDS (llong, lshort, lexp; two
// with a level per channel), the chain lane reads all of them and writes the VCA gain over llong; the helper waves load three
// rows and emit one, multiplied by the audio where there is one.  A tile is whole in LDS before anything of it is stored, so
// vca may be any of the input rows.  simple_autogain_kernel has one row and applies the recorded changes of the gain limits
// ahead of its first sample.
//
// Per sample there is nothing but *, /, +, - and compares: every one rounds on its own (no fused multiply-add; the division
// is the correctly rounded sequence and subnormals are kept), so gain and state match tests/autogain_ref.py bit for bit.
// Inputs are finite and lexp > 0: NaN is out of scope.
#include "autogain_bank.h"
#include "bank_core.h"
#include "tile_chain_device.h"

#include <cmath>

#pragma clang fp contract(off)      // every product and every sum below rounds on its own, in the kernels and in update()

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
}

namespace
{
    using namespace mi_tile_chain;

    enum { VEC_VCA = 1, VEC_LONG = 2, VEC_SHORT = 4, VEC_EXP = 8, VEC_AUDIO = 16 };
    enum { VEC_DST = 1, VEC_SRC = 2 };

    constexpr int PITCH = GROUP * ROW;          // floats between a channel's llong, lshort and lexp rows of a tile in LDS
    constexpr int QUAD  = 4;                    // samples of every row the chain reads ahead of itself

    // AutoGain.cpp:197-211: eval_curve(c, x) / x
    __device__ __forceinline__ float eval_gain(const mi_autogain_curve_t &c, float x)
    {
        const float v = x - c.x1;
        const float y = ((c.a * v + c.b) * v + c.c * v) + c.d;
        return ((x >= c.x2) ? c.t : (x <= c.x1) ? x : y) / x;
    }

    // what the chain's lane keeps of its channel
    struct gain_state { float gain, out; uint32_t surge; };
    struct gain_consts
    {
        float skg, skf, lkg, lkf;               // sShort.fKGrow, fKFall, sLong.fKGrow, fKFall
        float silence, dev, max;
        bool quick, limit;                      // F_QUICK_AMP, F_MAX_GAIN
        mi_autogain_curve_t sc, oc;             // sShortComp, sOutComp
    };

    // process_sample, AutoGain.cpp:223-276, with apply_gain_limiting, :213-221
    __device__ __forceinline__ float gain_step(float sl, float ss, float le, gain_state &s, const gain_consts &p)
    {
        float gain = s.gain;
        if (!(ss <= p.silence))
        {
            const float nl = sl * gain, ns = ss * gain;
            uint32_t f = s.surge;
            if (f == MI_AG_SURGE_UP)                                    // :234-246
                f = (ns <= le * p.dev) ? 0 : f;
            else if (p.quick && f == MI_AG_SURGE_DOWN)
                f = (ns * p.dev > le) ? 0 : f;
            else
                f = 0;
            const float red = eval_gain(p.sc, ns / le);                 // :249-253
            if (red * p.dev < 1.0f)
                f |= MI_AG_SURGE_UP;
            else if (p.quick && ns * p.dev <= le)
                f |= MI_AG_SURGE_DOWN;
            const float k = (f & MI_AG_SURGE_UP) ? p.skf : (f & MI_AG_SURGE_DOWN) ? p.skg :
                            (nl > le) ? p.lkf : (nl < le) ? p.lkg : 1.0f;   // :258-268 (gain * 1 is gain)
            gain = gain * k;
            gain = gain * eval_gain(p.oc, (ss * gain) / le);            // :271-272
            s.surge = f;
            s.gain = gain;
        }
        if (p.limit)                                                    // :215-218
            s.out = (gain >= p.max) ? p.max / gain : 1.0f;
        else
        {
            const float grown = s.out * p.lkg;
            s.out = (grown < 1.0f) ? grown : 1.0f;
        }
        return gain * s.out;
    }

    // The chain over samples [0, n) of a channel's ROWS rows of a tile in LDS (base, base + PITCH, base + 2 PITCH): row 0
    // becomes step(row 0, row 1, row 2), in order.  What chain_batches is for one row: the next four samples of every row are
    // read before this four's chain, one 16-byte write after it.
    template <int ROWS, class Step> __device__ __forceinline__ void chain_rows(lds_float *base, uint32_t n, Step step)
    {
        uint32_t i = 0;
        if (QUAD <= n)
        {
            f32x4 q[ROWS];
            #pragma unroll
            for (int j = 0; j < ROWS; ++j)
                q[j] = *reinterpret_cast<lds_f32x4 *>(base + j * PITCH);
            for (; i + QUAD <= n; i += QUAD)
            {
                float v[3][QUAD] = {};
                #pragma unroll
                for (int j = 0; j < ROWS; ++j)
                    v[j][0] = q[j].x, v[j][1] = q[j].y, v[j][2] = q[j].z, v[j][3] = q[j].w;
                const uint32_t next = (i + 2 * QUAD <= n) ? i + QUAD : i;
                #pragma unroll
                for (int j = 0; j < ROWS; ++j)
                    q[j] = *reinterpret_cast<lds_f32x4 *>(base + j * PITCH + next);
                float g[QUAD];
                #pragma unroll
                for (int t = 0; t < QUAD; ++t)
                    g[t] = step(v[0][t], v[1][t], v[2][t]);
                *reinterpret_cast<lds_f32x4 *>(base + i) = f32x4{ g[0], g[1], g[2], g[3] };
            }
        }
        for (; i < n; ++i)
            base[i] = step(base[i], base[PITCH + i], (ROWS > 2) ? base[2 * PITCH + i] : 0.0f);
    }

    // a lane's four samples c .. c + 3 of tile t of a row in memory into LDS
    __device__ __forceinline__ void load_quad(float *l, const float *row, bool wide, uint32_t c, extent t)
    {
        if (wide && c + 4 <= t.n)
            *reinterpret_cast<float4 *>(l) = *reinterpret_cast<const float4 *>(row + t.t0 + c);
        else
        {
            #pragma unroll
            for (uint32_t j = 0; j < 4; ++j)
                if (c + j < t.n)
                    l[j] = row[t.t0 + c + j];
        }
    }

    // ... out of LDS, times the audio where there is one, into memory
    __device__ __forceinline__ void emit_quad(float *out, const float *l, const float *audio, bool wide_out, bool wide_audio,
                                              uint32_t c, extent t)
    {
        if (c >= t.n)
            return;
        const float4 g4 = *reinterpret_cast<const float4 *>(l);
        float g[4] = { g4.x, g4.y, g4.z, g4.w };
        if (audio != nullptr)
        {
            float a[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
            if (wide_audio && c + 4 <= t.n)
            {
                const float4 a4 = *reinterpret_cast<const float4 *>(audio + t.t0 + c);
                a[0] = a4.x, a[1] = a4.y, a[2] = a4.z, a[3] = a4.w;
            }
            else
            {
                #pragma unroll
                for (uint32_t j = 0; j < 4; ++j)
                    if (c + j < t.n)
                        a[j] = audio[t.t0 + c + j];
            }
            #pragma unroll
            for (uint32_t j = 0; j < 4; ++j)
                g[j] = a[j] * g[j];
        }
        store_quad(out + t.t0 + c, g, wide_out, c, t.n);
    }

    // vca (audio == NULL) or audio * vca.  LEVEL: lexp is levels[channels], otherwise rows.  vec: which buffers have 16-byte
    // aligned rows.
    template <bool LEVEL>
    __global__ __launch_bounds__(BLOCK) void autogain_kernel(float *vca, const float *llong, const float *lshort, const float *lexp,
                                                             const float *audio, size_t vca_stride, size_t long_stride,
                                                             size_t short_stride, size_t exp_stride, size_t audio_stride,
                                                             uint32_t count, uint32_t channels, const mi_autogain_params_t *params,
                                                             mi::autogain_state *state, uint32_t vec)
    {
        constexpr int ROWS = LEVEL ? 2 : 3;
        __shared__ __attribute__((aligned(16))) float tile[2][ROWS][GROUP][ROW];
        const role me = my_role(channels);
        const uint32_t r = me.r, ch = me.ch, c = me.c;

        gain_state gs = { 1.0f, 1.0f, 0 };
        gain_consts p = {};
        float level = 1.0f;
        if (me.valid && me.chain)
        {
            const mi::autogain_state s = state[ch];
            gs = gain_state{ s.gain, s.out, s.surge };
            const mi_autogain_params_t q = params[ch];
            p.skg = q.short_kgrow, p.skf = q.short_kfall, p.lkg = q.long_kgrow, p.lkf = q.long_kfall;
            p.silence = q.silence, p.dev = q.deviation, p.max = q.max_gain;
            p.quick = (q.flags & MI_AG_QUICK_AMP) != 0, p.limit = (q.flags & MI_AG_MAX_GAIN) != 0;
            p.sc = q.short_comp, p.oc = q.out_comp;
            if (LEVEL)
                level = lexp[ch];
        }
        const float *ls = llong + size_t(ch) * long_stride, *ss = lshort + size_t(ch) * short_stride;
        const float *es = LEVEL ? nullptr : lexp + size_t(ch) * exp_stride;
        const float *as = (audio != nullptr) ? audio + size_t(ch) * audio_stride : nullptr;
        float *vs = vca + size_t(ch) * vca_stride;

        auto load_tile = [&](uint32_t k)
        {
            const extent t = tile_extent(count, k);
            load_quad(&tile[k & 1][0][r][c], ls, vec & VEC_LONG, c, t);
            load_quad(&tile[k & 1][1][r][c], ss, vec & VEC_SHORT, c, t);
            if (!LEVEL)
                load_quad(&tile[k & 1][ROWS - 1][r][c], es, vec & VEC_EXP, c, t);
        };
        auto chain_tile = [&](uint32_t k)
        {
            chain_rows<ROWS>((lds_float *)&tile[k & 1][0][r][0], tile_extent(count, k).n,
                             [&](float sl, float sh, float le) { return gain_step(sl, sh, LEVEL ? level : le, gs, p); });
        };
        auto emit_tile = [&](uint32_t k)
        {
            emit_quad(vs, &tile[k & 1][0][r][c], as, vec & VEC_VCA, vec & VEC_AUDIO, c, tile_extent(count, k));
        };

        MI_TILE_CHAIN_WALK(me, count, k, load_tile(k), chain_tile(k), emit_tile(k));
        if (me.valid && me.chain)
            state[ch] = mi::autogain_state{ gs.gain, gs.out, gs.surge, 0 };
    }

    // SimpleAutoGain::process, SimpleAutoGain.cpp:155-175
    __global__ __launch_bounds__(BLOCK) void simple_autogain_kernel(float *dst, const float *src, size_t dst_stride, size_t src_stride,
                                                                    uint32_t count, uint32_t channels,
                                                                    const mi_simple_autogain_params_t *params, float *gain,
                                                                    mi::simple_autogain_pending *pending,
                                                                    const mi::simple_autogain_op *ops, uint32_t vec)
    {
        __shared__ __attribute__((aligned(16))) float tile[2][GROUP][ROW];
        const role me = my_role(channels);
        const uint32_t r = me.r, ch = me.ch, c = me.c;

        float g = 1.0f, kg = 0.0f, kf = 0.0f, thr = 0.0f, lo = 0.0f, hi = 0.0f;
        if (me.valid && me.chain)
        {
            g = gain[ch];
            const mi::simple_autogain_pending pd = pending[ch];         // the limits' changes since the last launch, in order
            for (uint32_t j = 0; j < pd.count; ++j)
                g = mi::simple_autogain_apply(g, ops[pd.first + j]);
            if (pd.count != 0)
                pending[ch].count = 0;
            const mi_simple_autogain_params_t q = params[ch];
            kg = q.kgrow, kf = q.kfall, thr = q.threshold, lo = q.min_gain, hi = q.max_gain;
        }
        const float *xs = src + size_t(ch) * src_stride;
        float *ds = dst + size_t(ch) * dst_stride;

        auto chain_tile = [&](uint32_t k)
        {
            chain_batches((lds_float *)&tile[k & 1][r][0], 0, tile_extent(count, k).n, [&](float x)
            {
                const float s = x * g;
                g = g * ((s < thr) ? kg : (s > thr) ? kf : 1.0f);      // :166-169 (g * 1 is g)
                g = (g < lo) ? lo : (g > hi) ? hi : g;                  // lsp_limit
                return g;
            });
        };

        MI_TILE_CHAIN_WALK(me, count, k, load_quad(&tile[k & 1][r][c], xs, vec & VEC_SRC, c, tile_extent(count, k)), chain_tile(k),
                           emit_quad(ds, &tile[k & 1][r][c], nullptr, vec & VEC_DST, false, c, tile_extent(count, k)));
        if (me.valid && me.chain)
            gain[ch] = g;
    }
} // namespace

/* ---- the host side ---------------------------------------------------------------------------------------------------- */

namespace
{
    constexpr uint32_t SWITCHES = MI_AG_QUICK_AMP | MI_AG_MAX_GAIN;
    constexpr uint32_t SURGES   = MI_AG_SURGE_UP | MI_AG_SURGE_DOWN;

    // AutoGain::calc_compressor, AutoGain.cpp:180-195; c.a goes through double as the reference's expression does
    void calc_curve(mi_autogain_curve_t &c, float x1, float x2, float y2)
    {
        c.x1 = x1;
        c.x2 = x2;
        const float dy = y2 - c.x1;
        const float dx = c.x2 - c.x1;
        const float dx1 = 1.0f / dx;
        const float dx2 = dx1 * dx1;
        c.t = y2;
        c.d = c.x1;
        c.c = 1.0f;
        c.b = 3.0f * dy * dx2 - 2.0f * dx1;
        c.a = float((1.0f - 2.0 * dy * dx1) * dx2);
    }

    // AutoGain::update, :155-173
    void compute_params(const mi_autogain_settings_t &s, mi_autogain_params_t &p)
    {
        const float ksr = float((M_LN10 / 20.0f) / double(s.sample_rate));
        p.short_kgrow = expf(s.short_grow * ksr);
        p.short_kfall = expf(-s.short_fall * ksr);
        p.long_kgrow = expf(s.long_grow * ksr);
        p.long_kfall = expf(-s.long_fall * ksr);
        const float q = sqrtf(s.deviation);
        calc_curve(p.short_comp, 1.0f / s.deviation, s.deviation, 1.0f);
        calc_curve(p.out_comp, q, s.deviation * q, s.deviation);
        p.silence = s.silence;
        p.deviation = s.deviation;
        p.max_gain = s.max_gain;
        p.flags = s.flags & SWITCHES;
    }

    // SimpleAutoGain::update, SimpleAutoGain.cpp:142-153
    void compute_params(const mi_simple_autogain_settings_t &s, mi_simple_autogain_params_t &p)
    {
        const float ksr = float((M_LN10 * 0.05f) / double(s.sample_rate));
        p.kgrow = expf(s.grow * ksr);
        p.kfall = expf(-s.fall * ksr);
        p.threshold = s.threshold;
        p.min_gain = s.min_gain;
        p.max_gain = s.max_gain;
    }
} // namespace

struct mi_autogain_bank : mi_bank::settings_bank<mi_autogain_settings_t, mi_autogain_params_t, mi::autogain_state>
{
    static constexpr const char *NAME = "mi_autogain_bank";

    static mi_autogain_settings_t fresh_settings()              // construct(), AutoGain.cpp:43-66
    {
        mi_autogain_settings_t s = {};
        s.silence = float(2.5119e-4);                           // GAIN_AMP_M_72_DB
        s.deviation = float(1.99526);                           // GAIN_AMP_P_6_DB
        s.max_gain = float(3.98107);                            // GAIN_AMP_P_12_DB
        return s;
    }
    static mi_autogain_params_t fresh_params()                  // ... with init_compressor, :72-81
    {
        mi_autogain_params_t p = {};
        p.short_comp.x1 = p.short_comp.x2 = p.short_comp.t = 1.0f;
        p.out_comp = p.short_comp;
        const mi_autogain_settings_t s = fresh_settings();
        p.silence = s.silence, p.deviation = s.deviation, p.max_gain = s.max_gain;
        return p;
    }
    static mi::autogain_state fresh_state() { return mi::autogain_state{ 1.0f, 1.0f, 0, 0 }; }  // fCurrGain, fOutGain
    static void compute(const mi_autogain_settings_t &s, mi_autogain_params_t &p) { compute_params(s, p); }
};

struct mi_simple_autogain_bank : mi_bank::settings_bank<mi_simple_autogain_settings_t, mi_simple_autogain_params_t, float>
{
    static constexpr const char *NAME = "mi_simple_autogain_bank";

    static mi_simple_autogain_settings_t fresh_settings()       // construct(), SimpleAutoGain.cpp:43-56
    {
        mi_simple_autogain_settings_t s = {};
        s.min_gain = 0.000001f;
        s.max_gain = 1.0f;
        return s;
    }
    static mi_simple_autogain_params_t fresh_params()
    {
        mi_simple_autogain_params_t p = {};
        p.min_gain = 0.000001f;
        p.max_gain = 1.0f;
        return p;
    }
    static float fresh_state() { return 1.0f; }                 // d_state is fCurrGain
    static void compute(const mi_simple_autogain_settings_t &s, mi_simple_autogain_params_t &p) { compute_params(s, p); }

    struct recorded { uint32_t channel; mi::simple_autogain_op op; };
    std::vector<recorded>                       ops;        // the limits' changes since the last launch, in order
    mi::simple_autogain_pending                *d_pending = nullptr;    // [channels]
    mi::simple_autogain_op                     *d_ops = nullptr;        // [ops_cap], a channel's side by side
    size_t                                      ops_cap = 0;
};

namespace
{
    int autogain_launch(float *vca, const float *llong, const float *lshort, const float *lexp, bool level, const float *audio,
                        size_t vca_stride, size_t long_stride, size_t short_stride, size_t exp_stride, size_t audio_stride,
                        uint32_t count, uint32_t channels, const mi_autogain_params_t *params, mi::autogain_state *state, hipStream_t st)
    {
        const uint32_t vec = (mi::aligned16(vca, vca_stride, channels) ? VEC_VCA : 0) | (mi::aligned16(llong, long_stride, channels) ? VEC_LONG : 0) |
                             (mi::aligned16(lshort, short_stride, channels) ? VEC_SHORT : 0) |
                             (!level && mi::aligned16(lexp, exp_stride, channels) ? VEC_EXP : 0) |
                             (mi::aligned16(audio, audio_stride, channels) ? VEC_AUDIO : 0);
        hipEvent_t ev0 = nullptr, ev1 = nullptr;
        mi::take_profile_events(&ev0, &ev1);
        const dim3 grid((channels + GROUP - 1) / GROUP), block(BLOCK);
        if (level)
            MI_LAUNCH(autogain_kernel<true>, grid, block, 0, st, ev0, ev1, vca, llong, lshort, lexp, audio, vca_stride, long_stride,
                      short_stride, exp_stride, audio_stride, count, channels, params, state, vec);
        else
            MI_LAUNCH(autogain_kernel<false>, grid, block, 0, st, ev0, ev1, vca, llong, lshort, lexp, audio, vca_stride, long_stride,
                      short_stride, exp_stride, audio_stride, count, channels, params, state, vec);
        MI_HIP_CHECK(hipGetLastError());
        return MI_OK;
    }

    int simple_autogain_launch(float *dst, const float *src, size_t dst_stride, size_t src_stride, uint32_t count, uint32_t channels,
                               const mi_simple_autogain_params_t *params, float *gain, mi::simple_autogain_pending *pending,
                               const mi::simple_autogain_op *ops, hipStream_t st)
    {
        const uint32_t vec = (mi::aligned16(dst, dst_stride, channels) ? VEC_DST : 0) | (mi::aligned16(src, src_stride, channels) ? VEC_SRC : 0);
        hipEvent_t ev0 = nullptr, ev1 = nullptr;
        mi::take_profile_events(&ev0, &ev1);
        MI_LAUNCH(simple_autogain_kernel, dim3((channels + GROUP - 1) / GROUP), dim3(BLOCK), 0, st, ev0, ev1, dst, src, dst_stride,
                  src_stride, count, channels, params, gain, pending, ops, vec);
        MI_HIP_CHECK(hipGetLastError());
        return MI_OK;
    }

    // the recorded changes of the limits go to the device, every channel's side by side and in their order
    int sag_send_ops(mi_simple_autogain_bank *b, hipStream_t st)
    {
        if (b->ops.empty())
            return MI_OK;
        const int r = mi::refuse_capture("mi_simple_autogain_bank", st);
        if (r != MI_OK)
            return r;
        const size_t n = b->ops.size();
        if (n > b->ops_cap)
        {
            (void)hipFree(b->d_ops);
            b->d_ops = nullptr;
            b->ops_cap = 0;
            MI_HIP_CHECK(hipMalloc(reinterpret_cast<void **>(&b->d_ops), 2 * n * sizeof(mi::simple_autogain_op)));
            b->ops_cap = 2 * n;
        }
        std::vector<mi::simple_autogain_pending> where(b->channels, mi::simple_autogain_pending{ 0, 0 });
        for (const auto &o : b->ops)
            ++where[o.channel].count;
        uint32_t first = 0;
        for (auto &w : where)
            w.first = first, first += w.count, w.count = 0;
        std::vector<mi::simple_autogain_op> sorted(n);
        for (const auto &o : b->ops)
            sorted[where[o.channel].first + where[o.channel].count++] = o.op;
        MI_HIP_CHECK(hipMemcpyAsync(b->d_ops, sorted.data(), n * sizeof(mi::simple_autogain_op), hipMemcpyHostToDevice, st));
        MI_HIP_CHECK(hipMemcpyAsync(b->d_pending, where.data(), where.size() * sizeof(mi::simple_autogain_pending), hipMemcpyHostToDevice, st));
        MI_HIP_CHECK(hipStreamSynchronize(st));                 // the host tables go away
        b->ops.clear();
        return MI_OK;
    }

    void sag_record(mi_simple_autogain_bank *b, uint32_t channel, uint32_t kind, float lo, float hi)
    {
        b->ops.push_back({ channel, mi::simple_autogain_op{ kind, lo, hi, 0 } });
    }

    // AutoGain::set_timing, :90-98
    void set_timing(mi_autogain_bank *b, uint32_t channel, float &slot, float value)
    {
        value = (value > 0.0f) ? value : 0.0f;
        if (slot == value)
            return;
        slot = value;
        b->update[channel] = 1;
    }

    void set_switch(mi_autogain_bank *b, uint32_t channel, uint32_t flag, int enable)
    {
        uint32_t &f = b->cfg[channel].flags;
        f = enable ? (f | flag) : (f & ~flag);
        b->params[channel].flags = f & SWITCHES;
        b->up.touch(channel);
    }

    // the checks and the launch of the three process entries.  level: lexp is one float per channel
    int ag_process(mi_autogain_bank *b, const char *who, float *vca, const float *audio, const float *llong, const float *lshort,
                   const float *lexp, bool level, size_t count, size_t vca_stride, size_t audio_stride, size_t long_stride,
                   size_t short_stride, size_t exp_stride, bool with_audio, void *stream)
    {
        MI_REQUIRE(b != nullptr, MI_ESTATE, "%s: NULL bank", who);
        hipStream_t st = mi::as_stream(stream);
        const int r = mi_bank::update(b, st);
        if (r != MI_OK || count == 0)
            return r;
        MI_REQUIRE(!level || lexp != nullptr, MI_EINVAL, "%s: NULL buffer (the levels)", who);
        const int k = mi_bank::check_rows(who, b->channels, count, size_t(1) << 31,
                                          { { vca, vca_stride, count, mi_bank::REQUIRED | mi_bank::OUTPUT },
                                            { llong, long_stride, count, mi_bank::REQUIRED }, { lshort, short_stride, count, mi_bank::REQUIRED },
                                            { level ? nullptr : lexp, exp_stride, count, level ? 0u : mi_bank::REQUIRED },
                                            { audio, audio_stride, count, with_audio ? mi_bank::REQUIRED : 0u } });
        if (k != MI_OK)
            return k;
        MI_REQUIRE(!level || static_cast<const void *>(lexp) != static_cast<const void *>(vca), MI_EINVAL,
                   "%s: the levels are the output buffer", who);
        return autogain_launch(vca, llong, lshort, lexp, level, audio, vca_stride, long_stride, short_stride, level ? 0 : exp_stride,
                               audio_stride, uint32_t(count), b->channels, b->d_params, b->d_state, st);
    }
} // namespace

namespace mi
{
    int autogain_bank_set_params(mi_autogain_bank_t *b, uint32_t channel, const mi_autogain_params_t *p)
    {
        return mi_bank::set_params(b, "autogain_bank_set_params", channel, p);
    }

    int autogain_bank_set_state(mi_autogain_bank_t *b, uint32_t channel, float curr_gain, float out_gain, uint32_t surge, hipStream_t st)
    {
        return mi_bank::set_state(b, "autogain_bank_set_state", channel, autogain_state{ curr_gain, out_gain, surge & SURGES, 0 }, true, st);
    }

    int simple_autogain_bank_set_params(mi_simple_autogain_bank_t *b, uint32_t channel, const mi_simple_autogain_params_t *p)
    {
        return mi_bank::set_params(b, "simple_autogain_bank_set_params", channel, p);
    }

    // ... the gain as it stands: changes of the limits recorded for the channel before are dropped
    int simple_autogain_bank_set_state(mi_simple_autogain_bank_t *b, uint32_t channel, float curr_gain, hipStream_t st)
    {
        const int r = mi_bank::set_state(b, "simple_autogain_bank_set_state", channel, curr_gain, true, st);
        if (r != MI_OK)
            return r;
        std::vector<mi_simple_autogain_bank::recorded> kept;
        for (const auto &o : b->ops)
            if (o.channel != channel)
                kept.push_back(o);
        b->ops.swap(kept);
        return MI_OK;
    }
}

extern "C" {

/* ---- AutoGain ------------------------------------------------------------------------------------------------------- */

int mi_autogain_compute_params(const mi_autogain_settings_t *settings, mi_autogain_params_t *params)
{
    MI_REQUIRE(settings != nullptr && params != nullptr, MI_EINVAL, "mi_autogain_compute_params: NULL argument");
    *params = mi_autogain_bank::fresh_params();
    compute_params(*settings, *params);
    return MI_OK;
}

int mi_autogain_bank_create(mi_autogain_bank_t **bank, uint32_t channels)                // AutoGain.cpp:43-66
{
    return mi_bank::create(bank, "mi_autogain_bank_create", channels);
}

int mi_autogain_bank_destroy(mi_autogain_bank_t *b)
{
    return mi_bank::destroy(b);
}

int mi_autogain_bank_set_sample_rate(mi_autogain_bank_t *b, uint32_t channel, uint32_t sample_rate)          // :100-109
{
    MI_BANK_SETTER("autogain", "set_sample_rate");
    if (c.sample_rate == sample_rate)
        return MI_OK;
    c.sample_rate = sample_rate;
    b->update[channel] = 1;
    return MI_OK;
}

int mi_autogain_bank_set_silence_threshold(mi_autogain_bank_t *b, uint32_t channel, float threshold)         // :111-115
{
    MI_BANK_SETTER("autogain", "set_silence_threshold");
    c.silence = (0.0f > threshold) ? 0.0f : threshold;
    b->params[channel].silence = c.silence;
    b->up.touch(channel);
    return MI_OK;
}

int mi_autogain_bank_set_deviation(mi_autogain_bank_t *b, uint32_t channel, float deviation)                 // :117-125
{
    MI_BANK_SETTER("autogain", "set_deviation");
    deviation = (1.0f > deviation) ? 1.0f : deviation;
    if (deviation == c.deviation)
        return MI_OK;
    c.deviation = deviation;
    b->update[channel] = 1;
    return MI_OK;
}


int mi_autogain_bank_set_short_grow(mi_autogain_bank_t *b, uint32_t channel, float value)
{
    MI_BANK_SETTER("autogain", "set_short_grow");
    set_timing(b, channel, c.short_grow, value);
    return MI_OK;
}

int mi_autogain_bank_set_short_fall(mi_autogain_bank_t *b, uint32_t channel, float value)
{
    MI_BANK_SETTER("autogain", "set_short_fall");
    set_timing(b, channel, c.short_fall, value);
    return MI_OK;
}

int mi_autogain_bank_set_short_speed(mi_autogain_bank_t *b, uint32_t channel, float grow, float fall)        // :127-131
{
    MI_BANK_SETTER("autogain", "set_short_speed");
    set_timing(b, channel, c.short_grow, grow);
    set_timing(b, channel, c.short_fall, fall);
    return MI_OK;
}

int mi_autogain_bank_set_long_grow(mi_autogain_bank_t *b, uint32_t channel, float value)
{
    MI_BANK_SETTER("autogain", "set_long_grow");
    set_timing(b, channel, c.long_grow, value);
    return MI_OK;
}

int mi_autogain_bank_set_long_fall(mi_autogain_bank_t *b, uint32_t channel, float value)
{
    MI_BANK_SETTER("autogain", "set_long_fall");
    set_timing(b, channel, c.long_fall, value);
    return MI_OK;
}

int mi_autogain_bank_set_long_speed(mi_autogain_bank_t *b, uint32_t channel, float grow, float fall)         // :133-137
{
    MI_BANK_SETTER("autogain", "set_long_speed");
    set_timing(b, channel, c.long_grow, grow);
    set_timing(b, channel, c.long_fall, fall);
    return MI_OK;
}

int mi_autogain_bank_set_max_gain(mi_autogain_bank_t *b, uint32_t channel, float value)                      // :145-148
{
    MI_BANK_SETTER("autogain", "set_max_gain");
    c.max_gain = (0.0f > value) ? 0.0f : value;
    b->params[channel].max_gain = c.max_gain;
    b->up.touch(channel);
    return MI_OK;
}

int mi_autogain_bank_set_max_gain_control(mi_autogain_bank_t *b, uint32_t channel, float value, int enable)  // :139-143
{
    MI_BANK_SETTER("autogain", "set_max_gain_control");
    c.max_gain = (0.0f > value) ? 0.0f : value;
    b->params[channel].max_gain = c.max_gain;
    set_switch(b, channel, MI_AG_MAX_GAIN, enable);
    return MI_OK;
}

int mi_autogain_bank_enable_max_gain(mi_autogain_bank_t *b, uint32_t channel, int enable)                    // :150-153
{
    MI_BANK_SETTER("autogain", "enable_max_gain");
    (void)c;
    set_switch(b, channel, MI_AG_MAX_GAIN, enable);
    return MI_OK;
}

int mi_autogain_bank_enable_quick_amplifier(mi_autogain_bank_t *b, uint32_t channel, int enable)             // :175-178
{
    MI_BANK_SETTER("autogain", "enable_quick_amplifier");
    (void)c;
    set_switch(b, channel, MI_AG_QUICK_AMP, enable);
    return MI_OK;
}

int mi_autogain_bank_update_settings(mi_autogain_bank_t *b, void *stream)                                    // :155-173
{
    return mi_bank::update_settings(b, "mi_autogain_bank_update_settings", stream);
}

int mi_autogain_bank_get_params(const mi_autogain_bank_t *b, uint32_t channel, mi_autogain_params_t *params)
{
    return mi_bank::get_params(b, "mi_autogain_bank_get_params", channel, params);
}

int mi_autogain_bank_get_state(mi_autogain_bank_t *b, uint32_t channel, float *curr_gain, float *out_gain, uint32_t *flags,
                               void *stream)
{
    mi::autogain_state s;
    const int r = mi_bank::get_state(b, "mi_autogain_bank_get_state", channel, &s, stream);
    if (r != MI_OK)
        return r;
    if (curr_gain != nullptr) *curr_gain = s.gain;
    if (out_gain != nullptr) *out_gain = s.out;
    if (flags != nullptr) *flags = (b->params[channel].flags & SWITCHES) | (s.surge & SURGES);
    return MI_OK;
}

int mi_autogain_bank_process(mi_autogain_bank_t *b, float *vca, const float *llong, const float *lshort, const float *lexp,
                             size_t count, size_t vca_stride, size_t long_stride, size_t short_stride, size_t exp_stride,
                             void *stream)                                                                   // :278-286
{
    return ag_process(b, "mi_autogain_bank_process", vca, nullptr, llong, lshort, lexp, false, count, vca_stride, 0, long_stride,
                      short_stride, exp_stride, false, stream);
}

int mi_autogain_bank_process_level(mi_autogain_bank_t *b, float *vca, const float *llong, const float *lshort, const float *levels,
                                   size_t count, size_t vca_stride, size_t long_stride, size_t short_stride, void *stream)   // :288-296
{
    return ag_process(b, "mi_autogain_bank_process_level", vca, nullptr, llong, lshort, levels, true, count, vca_stride, 0, long_stride,
                      short_stride, 0, false, stream);
}

int mi_autogain_bank_process_apply(mi_autogain_bank_t *b, float *dst, const float *audio, const float *llong, const float *lshort,
                                   const float *lexp, size_t count, size_t dst_stride, size_t audio_stride, size_t long_stride,
                                   size_t short_stride, size_t exp_stride, void *stream)
{
    return ag_process(b, "mi_autogain_bank_process_apply", dst, audio, llong, lshort, lexp, false, count, dst_stride, audio_stride,
                      long_stride, short_stride, exp_stride, true, stream);
}

/* ---- SimpleAutoGain ------------------------------------------------------------------------------------------------- */

int mi_simple_autogain_compute_params(const mi_simple_autogain_settings_t *settings, mi_simple_autogain_params_t *params)
{
    MI_REQUIRE(settings != nullptr && params != nullptr, MI_EINVAL, "mi_simple_autogain_compute_params: NULL argument");
    compute_params(*settings, *params);
    return MI_OK;
}


int mi_simple_autogain_bank_create(mi_simple_autogain_bank_t **bank, uint32_t channels)   // SimpleAutoGain.cpp:43-56
{
    const int r = mi_bank::create(bank, "mi_simple_autogain_bank_create", channels);
    if (r != MI_OK)
        return r;
    mi_simple_autogain_bank *b = *bank;
    hipError_t e = hipMalloc(reinterpret_cast<void **>(&b->d_pending), size_t(channels) * sizeof(mi::simple_autogain_pending));
    if (e == hipSuccess) e = hipMemset(b->d_pending, 0, size_t(channels) * sizeof(mi::simple_autogain_pending));
    if (e == hipSuccess) e = hipDeviceSynchronize();            // the memset, whatever stream the first call comes on
    if (e != hipSuccess)
    {
        *bank = nullptr;
        mi_simple_autogain_bank_destroy(b);
        return mi::fail(MI_EHIP, "mi_simple_autogain_bank_create: %s", hipGetErrorString(e));
    }
    return MI_OK;
}

int mi_simple_autogain_bank_destroy(mi_simple_autogain_bank_t *b)
{
    if (b == nullptr)
        return MI_OK;
    (void)hipFree(b->d_pending); (void)hipFree(b->d_ops);
    return mi_bank::destroy(b);
}

int mi_simple_autogain_bank_set_sample_rate(mi_simple_autogain_bank_t *b, uint32_t channel, uint32_t sample_rate)     // :68-77
{
    MI_BANK_SETTER("simple_autogain", "set_sample_rate");
    if (c.sample_rate == sample_rate)
        return MI_OK;
    c.sample_rate = sample_rate;
    b->update[channel] = 1;
    return MI_OK;
}

int mi_simple_autogain_bank_set_grow(mi_simple_autogain_bank_t *b, uint32_t channel, float value)             // :79-86
{
    MI_BANK_SETTER("simple_autogain", "set_grow");
    if (c.grow == value)
        return MI_OK;
    c.grow = value;
    b->update[channel] = 1;
    return MI_OK;
}

int mi_simple_autogain_bank_set_fall(mi_simple_autogain_bank_t *b, uint32_t channel, float value)             // :88-95
{
    MI_BANK_SETTER("simple_autogain", "set_fall");
    if (c.fall == value)
        return MI_OK;
    c.fall = value;
    b->update[channel] = 1;
    return MI_OK;
}

int mi_simple_autogain_bank_set_speed(mi_simple_autogain_bank_t *b, uint32_t channel, float grow, float fall) // :97-106
{
    MI_BANK_SETTER("simple_autogain", "set_speed");
    if (c.grow == grow && c.fall == fall)
        return MI_OK;
    c.grow = grow, c.fall = fall;
    b->update[channel] = 1;
    return MI_OK;
}

int mi_simple_autogain_bank_set_max_gain(mi_simple_autogain_bank_t *b, uint32_t channel, float value)         // :108-115
{
    MI_BANK_SETTER("simple_autogain", "set_max_gain");
    if (c.max_gain == value)
        return MI_OK;
    c.max_gain = value;
    b->params[channel].max_gain = value;
    b->up.touch(channel);
    sag_record(b, channel, mi::SAG_MIN, 0.0f, value);
    return MI_OK;
}

int mi_simple_autogain_bank_set_min_gain(mi_simple_autogain_bank_t *b, uint32_t channel, float value)         // :117-124
{
    MI_BANK_SETTER("simple_autogain", "set_min_gain");
    if (c.min_gain == value)
        return MI_OK;
    c.min_gain = value;
    b->params[channel].min_gain = value;
    b->up.touch(channel);
    sag_record(b, channel, mi::SAG_MAX, value, 0.0f);
    return MI_OK;
}

int mi_simple_autogain_bank_set_gain(mi_simple_autogain_bank_t *b, uint32_t channel, float min, float max)    // :126-135
{
    MI_BANK_SETTER("simple_autogain", "set_gain");
    if (c.min_gain == min && c.max_gain == max)
        return MI_OK;
    c.min_gain = min, c.max_gain = max;
    b->params[channel].min_gain = min, b->params[channel].max_gain = max;
    b->up.touch(channel);
    sag_record(b, channel, mi::SAG_LIMIT, min, max);
    return MI_OK;
}

int mi_simple_autogain_bank_set_threshold(mi_simple_autogain_bank_t *b, uint32_t channel, float threshold)    // :137-140
{
    MI_BANK_SETTER("simple_autogain", "set_threshold");
    c.threshold = threshold;
    b->params[channel].threshold = threshold;
    b->up.touch(channel);
    return MI_OK;
}

int mi_simple_autogain_bank_update_settings(mi_simple_autogain_bank_t *b, void *stream)                       // :142-153
{
    return mi_bank::update_settings(b, "mi_simple_autogain_bank_update_settings", stream);
}

int mi_simple_autogain_bank_get_params(const mi_simple_autogain_bank_t *b, uint32_t channel, mi_simple_autogain_params_t *params)
{
    return mi_bank::get_params(b, "mi_simple_autogain_bank_get_params", channel, params);
}

int mi_simple_autogain_bank_get_state(mi_simple_autogain_bank_t *b, uint32_t channel, float *curr_gain, void *stream)
{
    float g = 0.0f;
    const int r = mi_bank::get_state(b, "mi_simple_autogain_bank_get_state", channel, &g, stream);
    if (r != MI_OK)
        return r;
    for (const auto &o : b->ops)                                // what the next launch will do first
        if (o.channel == channel)
            g = mi::simple_autogain_apply(g, o.op);
    if (curr_gain != nullptr) *curr_gain = g;
    return MI_OK;
}

int mi_simple_autogain_bank_process(mi_simple_autogain_bank_t *b, float *dst, const float *src, size_t count, size_t dst_stride,
                                    size_t src_stride, void *stream)                                          // :155-175
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_simple_autogain_bank_process: NULL bank");
    hipStream_t st = mi::as_stream(stream);
    const int r = mi_bank::update(b, st);
    if (r != MI_OK || count == 0)
        return r;
    const int k = mi_bank::check_rows("mi_simple_autogain_bank_process", b->channels, count, size_t(1) << 31,
                                      { { dst, dst_stride, count, mi_bank::REQUIRED | mi_bank::OUTPUT },
                                        { src, src_stride, count, mi_bank::REQUIRED } });
    if (k != MI_OK)
        return k;
    const int s = sag_send_ops(b, st);
    if (s != MI_OK)
        return s;
    return simple_autogain_launch(dst, src, dst_stride, src_stride, uint32_t(count), b->channels, b->d_params, b->d_state, b->d_pending,
                                  b->d_ops, st);
}

} // extern "C"
