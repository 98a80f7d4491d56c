// lsp::dspu::DynamicProcessor as a bank of `channels` processors (src/main/dynamics/DynamicProcessor.cpp): the envelope follower
// of process() (:404-430) -- the Compressor's three-variable recurrence with tau looked up per sample from the running envelope
// (solve_reaction, :195-202) -- and the array reduction() (:562-584): the sum of up to four splines of ln |e|, then expf.
//
// dynproc_kernel runs on the tile walk of tile_chain_device.h as follow_kernel of dynamics_device.h does: prepare loads the
// input tile, the chain is the follower in place in LDS (dynproc_follow_tile, a function of its own so that its instructions
// can be looked at, tests/test_dynproc_host.py), emit computes the gain from the envelope and stores.  It is a kernel of its
// own because emit reads the row's table anew for every tile through a wave-uniform pointer and the follower takes two
// tables, not two taus, which nobody else in the walk would use; the flags, the follower's state, the end of its step and the
// bank around the kernel (dynamics_bank_core.h) are the shared ones.  The parameters are computed in host/dynproc.cpp
// (mi_dynproc_compute_params).
//
// Both tables of a channel are PADDED to their full length where they are loaded: a reaction level of +inf is never reached
// by a finite envelope, so the look-up is four compares and four selects on every lane; a spline with knee_start = +inf and
// everything else 0 adds 0 * (lx - 0) = +-0 to the sum, so the sum has four terms on every row and `no spline` is expf(+0) = 1.
//
// Inputs are finite: NaN is out of scope.  Subnormal envelopes are kept (the float32 denormal mode is on).
#include "dynproc_bank.h"
#include "dynamics_bank_core.h"

#include <cmath>

#pragma clang fp contract(off)      // every product and every sum below rounds on its own

namespace
{
    using namespace mi_dynamics;

    constexpr int DOTS = MI_DYNPROC_DOTS, RANGES = MI_DYNPROC_RANGES;

    // vAttack or vRelease in a lane's registers: t0 is the default, t1 .. t4 hold from l1 .. l4 on; +inf where unused.  Named
    // scalars, not arrays: of `r = (x >= lvl[i]) ? tau[i + 1] : r` over arrays the compiler makes a selected INDEX and a load
    // through it, which puts the tables into scratch.
    struct reactions { float l1, l2, l3, l4, t0, t1, t2, t3, t4; };

    __device__ __forceinline__ reactions load_reactions(const mi_dynproc_reaction_t *r, uint32_t count)
    {
        reactions t;
        t.t0 = r[0].tau;
        t.l1 = (1 < count) ? r[1].level : INFINITY, t.t1 = (1 < count) ? r[1].tau : 0.0f;
        t.l2 = (2 < count) ? r[2].level : INFINITY, t.t2 = (2 < count) ? r[2].tau : 0.0f;
        t.l3 = (3 < count) ? r[3].level : INFINITY, t.t3 = (3 < count) ? r[3].tau : 0.0f;
        t.l4 = (4 < count) ? r[4].level : INFINITY, t.t4 = (4 < count) ? r[4].tau : 0.0f;
        return t;
    }

    // solve_reaction, :195-202: the tau of the last level <= x.  Nine scalars by value: through a reference to a struct the
    // compiler selects an ADDRESS and loads through it, which puts the table into scratch.
    __device__ __forceinline__ float solve_reaction(float x, float l1, float l2, float l3, float l4, float t0, float t1, float t2,
                                                    float t3, float t4)
    {
        float r = t0;
        r = (x >= l1) ? t1 : r;
        r = (x >= l2) ? t2 : r;
        r = (x >= l3) ? t3 : r;
        r = (x >= l4) ? t4 : r;
        return r;
    }

    // DynamicProcessor.cpp:406-427, one sample, given the two taus that were looked up from e BEFORE the step
    __device__ __forceinline__ void follow_step(float s, float &e, float &peak, uint32_t &hold, float ta, float tr, uint32_t nhold)
    {
        const float d = s - e;
        const bool neg = d < 0.0f;
        const float tau = neg ? tr : ta;
        const float en = e + d * tau;
        MI_FOLLOW_SETTLE(e, peak, hold, neg, en, nhold);
    }

    // ... over samples [0, n) of one row in LDS, in place: row[i] becomes the envelope.  The two tables come as eighteen
    // scalars: a struct by value would travel through the stack, and the kernel has no scratch.
    __device__ __noinline__ follow_state dynproc_follow_tile(lds_float *row, uint32_t n, follow_state s, uint32_t nhold,
                                                             float al1, float al2, float al3, float al4,
                                                             float at0, float at1, float at2, float at3, float at4,
                                                             float rl1, float rl2, float rl3, float rl4,
                                                             float rt0, float rt1, float rt2, float rt3, float rt4)
    {
        float e = s.e, peak = s.peak;
        uint32_t hold = s.hold;
        chain_batches(row, 0, n, [=, &e, &peak, &hold](float v)
        {
            const float ta = solve_reaction(e, al1, al2, al3, al4, at0, at1, at2, at3, at4);
            const float tr = solve_reaction(e, rl1, rl2, rl3, rl4, rt0, rt1, rt2, rt3, rt4);
            follow_step(v, e, peak, hold, ta, tr, nhold);
            return e;
        });
        return follow_state{ e, peak, hold };
    }

    // vSplines of a row, padded to four
    struct splines { mi_dynproc_spline_t s[DOTS]; };

    // The padding works on the words, with a mask: a select between two floats is done by the vector unit even where both
    // are uniform, and the row's table would leave the scalar registers for it.
    __device__ __forceinline__ float keep_or(float v, uint32_t keep, uint32_t otherwise)
    {
        return __uint_as_float((__float_as_uint(v) & keep) | (otherwise & ~keep));
    }

    __device__ __forceinline__ splines load_splines(const mi_dynproc_params_t &p)
    {
        constexpr uint32_t INF = 0x7f800000u;
        splines t;
        #pragma unroll
        for (uint32_t j = 0; j < uint32_t(DOTS); ++j)
        {
            const uint32_t on = (j < p.splines) ? ~0u : 0u;
            const mi_dynproc_spline_t &q = p.spline[j];
            t.s[j].pre_ratio = keep_or(q.pre_ratio, on, 0);
            t.s[j].post_ratio = keep_or(q.post_ratio, on, 0);
            t.s[j].knee_start = keep_or(q.knee_start, on, INF);
            t.s[j].knee_stop = keep_or(q.knee_stop, on, INF);
            t.s[j].thresh = keep_or(q.thresh, on, 0);
            t.s[j].makeup = keep_or(q.makeup, on, 0);
            t.s[j].herm[0] = keep_or(q.herm[0], on, 0);
            t.s[j].herm[1] = keep_or(q.herm[1], on, 0);
            t.s[j].herm[2] = keep_or(q.herm[2], on, 0);
            t.s[j].herm[3] = 0.0f;
        }
        return t;
    }

    // spline_amp, :173-183
    __device__ __forceinline__ float spline_amp(const mi_dynproc_spline_t &s, float lx)
    {
        if (lx <= s.knee_start)
            return s.makeup + s.pre_ratio * (lx - s.thresh);
        if (lx >= s.knee_stop)
            return s.makeup + s.post_ratio * (lx - s.thresh);
        return (s.herm[0] * lx + s.herm[1]) * lx + s.herm[2];
    }

    // spline_model, :185-193
    __device__ __forceinline__ float spline_model(const mi_dynproc_spline_t &s, float lx)
    {
        return s.makeup + ((lx <= s.thresh) ? s.pre_ratio : s.post_ratio) * (lx - s.thresh);
    }

    // the body of reduction() / curve() / model() for the limited level x: expf of the sum over the splines, in order
    template <bool MODEL> __device__ __forceinline__ float spline_gain(const splines &t, float x)
    {
        const float lx = logf(x);
        float gain = 0.0f;
        #pragma unroll
        for (int j = 0; j < DOTS; ++j)
            gain += MODEL ? spline_model(t.s[j], lx) : spline_amp(t.s[j], lx);
        return expf(gain);
    }

    // reduction(float *, const float *, size_t), :562-584, one sample: the lower limit is GAIN_AMP_MIN
    __device__ __forceinline__ float reduction(const splines &t, float e)
    {
        float x = fabsf(e);
        x = (x < 1e-6f) ? 1e-6f : (x > 1e+10f) ? 1e+10f : x;
        return spline_gain<false>(t, x);
    }

    // gain (audio == NULL) or dst = audio * gain into `gain`, the envelope into `env` unless NULL.  vec: which of the buffers
    // have 16-byte aligned rows.
    __global__ __launch_bounds__(BLOCK) void dynproc_kernel(float *gain, float *env, const float *in, const float *audio,
                                                            size_t gain_stride, size_t env_stride, size_t in_stride,
                                                            size_t audio_stride, uint32_t count, uint32_t channels,
                                                            const mi_dynproc_params_t *__restrict__ params,
                                                            device_state *state, uint32_t vec)
    {
        __shared__ __attribute__((aligned(16))) float tile[2][GROUP][ROW];
        const role me = my_role(channels);
        const uint32_t r = me.r, ch = me.ch, c = me.c;

        // A helper's row's table, by a wave-uniform index: the row comes from the wave's number alone (the role's r merges it
        // with the chain's lane number, which is not uniform, and the table then travels through vector loads).  Whatever the
        // index, the pointer stays inside the table: a helper wave whose row has no channel gets the last channel's; wave 0
        // has "row -1", which is the previous workgroup's last channel, and in workgroup 0 wraps and is clamped to the last
        // channel as well.  Neither reads it: only emit does, and only for a row that has a channel.
        const uint32_t wave_ch = blockIdx.x * GROUP + uint32_t(__builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6) - 1));
        const mi_dynproc_params_t *row_params = params + ((wave_ch < channels) ? wave_ch : channels - 1);

        // the follower's lane: its channel's state and reaction tables
        follow_state fs = { 0.0f, 0.0f, 0 };
        reactions att = {}, rel = {};
        uint32_t nhold = 0;
        if (me.valid && me.chain)
        {
            const device_state s = state[ch];
            fs = follow_state{ s.e, s.peak, s.hold };
            att = load_reactions(params[ch].attack, params[ch].attacks);
            rel = load_reactions(params[ch].release, params[ch].releases);
            nhold = params[ch].hold;
        }
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
            // the row's 40 spline floats, read anew for every tile with scalar loads: held over the walk they would be live
            // across the call of the follower, which keeps no scalar registers, and the compiler parks them in 36 VGPRs
            const splines sp = load_splines(*row_params);
            const float4 e4 = *reinterpret_cast<const float4 *>(&tile[k & 1][r][c]);
            const float e[4] = { e4.x, e4.y, e4.z, e4.w };
            float g[4];
            #pragma unroll
            for (uint32_t j = 0; j < 4; ++j)
                g[j] = (c + j < t.n) ? reduction(sp, e[j]) : 0.0f;
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
                           fs = dynproc_follow_tile((lds_float *)&tile[k & 1][r][0], tile_extent(count, k).n, fs, nhold,
                                                    att.l1, att.l2, att.l3, att.l4,
                                                    att.t0, att.t1, att.t2, att.t3, att.t4,
                                                    rel.l1, rel.l2, rel.l3, rel.l4,
                                                    rel.t0, rel.t1, rel.t2, rel.t3, rel.t4),
                           emit_tile(k));
        if (me.valid && me.chain)
            state[ch] = device_state{ fs.e, fs.peak, fs.hold, 0 };
    }

    // curve(float *, const float *, size_t), :474-496, or with MODEL model(...), :518-540, over rows: the lower limit is
    // FLOAT_SAT_M_INF, the result the gain times the limited level
    template <bool MODEL>
    __global__ __launch_bounds__(CURVE_BLOCK) void dynproc_curve_kernel(float *out, const float *in, size_t out_stride,
                                                                        size_t in_stride, uint32_t dots,
                                                                        const mi_dynproc_params_t *params)
    {
        const uint32_t ch = blockIdx.y, i = blockIdx.x * CURVE_BLOCK + threadIdx.x;
        if (i >= dots)
            return;
        const splines sp = load_splines(params[ch]);
        float x = fabsf(in[size_t(ch) * in_stride + i]);
        x = (x < 1e-10f) ? 1e-10f : (x > 1e+10f) ? 1e+10f : x;
        out[size_t(ch) * out_stride + i] = spline_gain<MODEL>(sp, x) * x;
    }

} // namespace

struct mi_dynproc_bank : mi_bank::settings_bank<mi_dynproc_settings_t, mi_dynproc_params_t, device_state>
{
    static constexpr const char *NAME = "mi_dynproc_bank";

    static mi_dynproc_settings_t fresh_settings()                               // DynamicProcessor::construct, :43-74
    {
        mi_dynproc_settings_t s = {};
        s.in_ratio = 1.0f;
        s.out_ratio = 1.0f;
        return s;
    }
    static mi_dynproc_params_t fresh_params()       // what the kernel may read before the first update: nothing but defaults
    {
        mi_dynproc_params_t p = {};
        p.attacks = p.releases = 1;
        return p;
    }
    static device_state fresh_state() { return device_state{}; }
    static void compute(const mi_dynproc_settings_t &s, mi_dynproc_params_t &p) { mi_dynproc_compute_params(&s, &p); }
    template <class... Args> static void launch(dim3 grid, hipStream_t st, hipEvent_t ev0, hipEvent_t ev1, Args... args)
    {
        MI_LAUNCH(dynproc_kernel, grid, dim3(BLOCK), 0, st, ev0, ev1, args...);
    }
};

namespace
{
    int dyn_curve(mi_dynproc_bank *b, const char *entry, bool model, float *out, const float *in, size_t dots, size_t out_stride,
                  size_t in_stride, void *stream)
    {
        return mi_dynamics::curve(b, entry, out, in, dots, out_stride, in_stride, stream,
                                  [&](dim3 grid, hipStream_t st, hipEvent_t ev0, hipEvent_t ev1)
        {
            if (model)
                MI_LAUNCH(dynproc_curve_kernel<true>, grid, dim3(CURVE_BLOCK), 0, st, ev0, ev1, out, in, out_stride, in_stride,
                          uint32_t(dots), b->d_params);
            else
                MI_LAUNCH(dynproc_curve_kernel<false>, grid, dim3(CURVE_BLOCK), 0, st, ev0, ev1, out, in, out_stride, in_stride,
                          uint32_t(dots), b->d_params);
        });
    }
} // namespace

namespace mi
{
    int dynproc_bank_set_params(mi_dynproc_bank_t *b, uint32_t channel, const mi_dynproc_params_t *p)
    {
        const int r = mi_bank::set_params_checks(b, "dynproc_bank_set_params", channel, p);
        if (r != MI_OK)
            return r;
        MI_REQUIRE(p->splines <= uint32_t(DOTS) && p->attacks >= 1 && p->attacks <= uint32_t(RANGES) && p->releases >= 1 &&
                   p->releases <= uint32_t(RANGES), MI_EINVAL, "dynproc_bank_set_params: counts out of range");
        return mi_bank::set_params_store(b, channel, p);
    }

    int dynproc_bank_set_state(mi_dynproc_bank_t *b, uint32_t channel, float envelope, float peak, uint32_t hold, hipStream_t st)
    {
        return mi_bank::set_state(b, "dynproc_bank_set_state", channel, device_state{ envelope, peak, hold, 0 }, true, st);
    }
}

extern "C" {

int mi_dynproc_bank_create(mi_dynproc_bank_t **bank, uint32_t channels)                 // DynamicProcessor.cpp:43-74
{
    return mi_bank::create(bank, "mi_dynproc_bank_create", channels);
}

int mi_dynproc_bank_destroy(mi_dynproc_bank_t *b)
{
    return mi_bank::destroy(b);
}

int mi_dynproc_bank_set_sample_rate(mi_dynproc_bank_t *b, uint32_t channel, uint32_t sample_rate)         // :80-86
{
    MI_BANK_SETTER("dynproc", "set_sample_rate");
    if (c.sample_rate == sample_rate)
        return MI_OK;
    c.sample_rate = sample_rate;
    b->update[channel] = 1;
    return MI_OK;
}

int mi_dynproc_bank_set_in_ratio(mi_dynproc_bank_t *b, uint32_t channel, float ratio)                     // :88-94
{
    MI_BANK_SETTER("dynproc", "set_in_ratio");
    if (c.in_ratio == ratio)
        return MI_OK;
    c.in_ratio = ratio;
    b->update[channel] = 1;
    return MI_OK;
}

int mi_dynproc_bank_set_out_ratio(mi_dynproc_bank_t *b, uint32_t channel, float ratio)                    // :96-102
{
    MI_BANK_SETTER("dynproc", "set_out_ratio");
    if (c.out_ratio == ratio)
        return MI_OK;
    c.out_ratio = ratio;
    b->update[channel] = 1;
    return MI_OK;
}

int mi_dynproc_bank_set_dot(mi_dynproc_bank_t *b, uint32_t channel, uint32_t id, const mi_dynproc_dot_t *dot)   // :287-337
{
    MI_BANK_SETTER("dynproc", "set_dot");
    MI_REQUIRE(id < uint32_t(DOTS), MI_EINVAL, "mi_dynproc_bank_set_dot: dot %u out of range", id);
    mi_dynproc_dot_t &d = c.dot[id];
    if (dot == nullptr)
    {
        if (d.input >= 0.0f || d.output >= 0.0f || d.knee >= 0.0f)
            b->update[channel] = 1;
        d.input = d.output = d.knee = -1.0f;
    }
    else
    {
        if (d.input != dot->input || d.output != dot->output || d.knee != dot->knee)
            b->update[channel] = 1;
        d = *dot;
    }
    return MI_OK;
}

int mi_dynproc_bank_set_attack_level(mi_dynproc_bank_t *b, uint32_t channel, uint32_t id, float level)    // :117-123
{
    MI_BANK_SETTER("dynproc", "set_attack_level");
    MI_REQUIRE(id < uint32_t(DOTS), MI_EINVAL, "mi_dynproc_bank_set_attack_level: level %u out of range", id);
    if (c.attack_level[id] == level)
        return MI_OK;
    c.attack_level[id] = level;
    b->update[channel] = 1;
    return MI_OK;
}

int mi_dynproc_bank_set_release_level(mi_dynproc_bank_t *b, uint32_t channel, uint32_t id, float level)   // :130-136
{
    MI_BANK_SETTER("dynproc", "set_release_level");
    MI_REQUIRE(id < uint32_t(DOTS), MI_EINVAL, "mi_dynproc_bank_set_release_level: level %u out of range", id);
    if (c.release_level[id] == level)
        return MI_OK;
    c.release_level[id] = level;
    b->update[channel] = 1;
    return MI_OK;
}

int mi_dynproc_bank_set_attack_time(mi_dynproc_bank_t *b, uint32_t channel, uint32_t id, float time)      // :143-149
{
    MI_BANK_SETTER("dynproc", "set_attack_time");
    MI_REQUIRE(id < uint32_t(RANGES), MI_EINVAL, "mi_dynproc_bank_set_attack_time: range %u out of range", id);
    if (c.attack_time[id] == time)
        return MI_OK;
    c.attack_time[id] = time;
    b->update[channel] = 1;
    return MI_OK;
}

int mi_dynproc_bank_set_release_time(mi_dynproc_bank_t *b, uint32_t channel, uint32_t id, float time)     // :156-162
{
    MI_BANK_SETTER("dynproc", "set_release_time");
    MI_REQUIRE(id < uint32_t(RANGES), MI_EINVAL, "mi_dynproc_bank_set_release_time: range %u out of range", id);
    if (c.release_time[id] == time)
        return MI_OK;
    c.release_time[id] = time;
    b->update[channel] = 1;
    return MI_OK;
}

int mi_dynproc_bank_set_hold(mi_dynproc_bank_t *b, uint32_t channel, float hold)                          // :164-171
{
    MI_BANK_SETTER("dynproc", "set_hold");
    hold = (hold > 0.0f) ? hold : 0.0f;
    if (c.hold == hold)
        return MI_OK;
    c.hold = hold;
    b->update[channel] = 1;
    return MI_OK;
}

int mi_dynproc_bank_update_settings(mi_dynproc_bank_t *b, void *stream)                                    // :339-395
{
    return mi_bank::update_settings(b, "mi_dynproc_bank_update_settings", stream);
}

int mi_dynproc_bank_clear(mi_dynproc_bank_t *b, void *stream)
{
    return mi_bank::clear(b, "mi_dynproc_bank_clear", stream);
}

int mi_dynproc_bank_get_params(const mi_dynproc_bank_t *b, uint32_t channel, mi_dynproc_params_t *params)
{
    return mi_bank::get_params(b, "mi_dynproc_bank_get_params", channel, params);
}

int mi_dynproc_bank_get_state(mi_dynproc_bank_t *b, uint32_t channel, float *envelope, float *peak, uint32_t *hold,
                              void *stream)
{
    return mi_dynamics::get_follow_state(b, "mi_dynproc_bank_get_state", channel, envelope, peak, hold, stream);
}

int mi_dynproc_bank_process(mi_dynproc_bank_t *b, float *gain, float *env, const float *in, size_t count,
                            size_t gain_stride, size_t env_stride, size_t in_stride, void *stream)        // :397-442
{
    return mi_dynamics::process(b, "mi_dynproc_bank_process", gain, env, in, count, gain_stride, env_stride, in_stride, stream);
}

int mi_dynproc_bank_process_apply(mi_dynproc_bank_t *b, float *dst, const float *audio, const float *sc, size_t count,
                                  size_t dst_stride, size_t audio_stride, size_t sc_stride, void *stream)
{
    return mi_dynamics::process_apply(b, "mi_dynproc_bank_process_apply", dst, audio, sc, count, dst_stride, audio_stride, sc_stride,
                                      stream);
}

int mi_dynproc_bank_curve(mi_dynproc_bank_t *b, float *out, const float *in, size_t dots, size_t out_stride,
                          size_t in_stride, void *stream)                                                  // :474-496
{
    return dyn_curve(b, "mi_dynproc_bank_curve", false, out, in, dots, out_stride, in_stride, stream);
}

int mi_dynproc_bank_model(mi_dynproc_bank_t *b, float *out, const float *in, size_t dots, size_t out_stride,
                          size_t in_stride, void *stream)                                                  // :518-540
{
    return dyn_curve(b, "mi_dynproc_bank_model", true, out, in, dots, out_stride, in_stride, stream);
}

} // extern "C"
