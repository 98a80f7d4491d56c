// lsp::dspu::AutoGain and lsp::dspu::SimpleAutoGain as banks of `channels` units (src/main/dynamics/AutoGain.cpp,
// SimpleAutoGain.cpp): the kernels and their launches; the banks' host side is host/autogain.cpp.
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
#include "tile_chain_device.h"

#pragma clang fp contract(off)      // every product and every sum below rounds on its own

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

namespace mi
{
    int autogain_launch(float *vca, const float *llong, const float *lshort, const float *lexp, bool level, const float *audio,
                        size_t vca_stride, size_t long_stride, size_t short_stride, size_t exp_stride, size_t audio_stride,
                        uint32_t count, uint32_t channels, const mi_autogain_params_t *params, autogain_state *state, hipStream_t st)
    {
        const uint32_t vec = (aligned16(vca, vca_stride, channels) ? VEC_VCA : 0) | (aligned16(llong, long_stride, channels) ? VEC_LONG : 0) |
                             (aligned16(lshort, short_stride, channels) ? VEC_SHORT : 0) |
                             (!level && aligned16(lexp, exp_stride, channels) ? VEC_EXP : 0) |
                             (aligned16(audio, audio_stride, channels) ? VEC_AUDIO : 0);
        hipEvent_t ev0 = nullptr, ev1 = nullptr;
        take_profile_events(&ev0, &ev1);
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
                               const mi_simple_autogain_params_t *params, float *gain, simple_autogain_pending *pending,
                               const simple_autogain_op *ops, hipStream_t st)
    {
        const uint32_t vec = (aligned16(dst, dst_stride, channels) ? VEC_DST : 0) | (aligned16(src, src_stride, channels) ? VEC_SRC : 0);
        hipEvent_t ev0 = nullptr, ev1 = nullptr;
        take_profile_events(&ev0, &ev1);
        MI_LAUNCH(simple_autogain_kernel, dim3((channels + GROUP - 1) / GROUP), dim3(BLOCK), 0, st, ev0, ev1, dst, src, dst_stride,
                  src_stride, count, channels, params, gain, pending, ops, vec);
        MI_HIP_CHECK(hipGetLastError());
        return MI_OK;
    }
} // namespace mi
