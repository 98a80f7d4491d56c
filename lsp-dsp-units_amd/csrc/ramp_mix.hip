// lsp::dspu::Bypass and lsp::dspu::Crossfade as banks of `channels` units (src/main/ctl/Bypass.cpp, Crossfade.cpp): a gain that
// runs as the float32 sum fGain += fDelta, one step per sample, a mix of two rows under it, and after the ramp a copy or a
// scale of the one row that is left.  The two classes differ in the test that ends the ramp (fGain < 1 or fGain > 0 against
// nCounter > 0), in the formula and in what the tail is; ramp_mix_kernel<KIND> is the same walk for both.
//
// A workgroup of BLOCK threads owns one channel and takes its row in chunks of CHUNK samples for as long as the ramp runs:
//     chain    thread 0 alone writes the chunk's gains into LDS, gains[i] = the gain BEFORE the step of sample i, and one more:
//              a chain of dependent adds, four to a 16-byte store, that looks once per 32 whether the ramp is behind it
//     end      every thread holds its four gains against the end test; the lowest sample that fails is where the ramp ends
//              (the crossfade knows it beforehand: min(nCounter, n))
//     mix      a thread's four samples, 16 bytes per row where the row allows it
// Once the ramp is over -- from sample 0 on for a steady channel -- nothing serial runs and no barrier but the one behind the
// state's load is met: the rest of the row is a 16-byte copy or scale that reads only the input the tail needs, 8 bytes per
// sample.  The channels of a launch are in different states; every decision is taken per workgroup from its own channel's state.
//
// INVARIANTS.  A thread reads every input of its four samples before it stores them, and no other thread touches those
// samples, so dst may be any input row with the same stride.  Chunks start at multiples of four samples of the row, so the
// 16-byte accesses of the ramp and of the tail are the same quads.  Thread 0 owns the chain and the state: every thread reads
// the state before the first barrier, thread 0 writes it back after its last use.  A ramp that uses up the block leaves fGain
// and nState as the loop left them; the clamp happens only where samples remain, as in the reference.
//
// The setters act on device state, so both banks record them in call order and send them in front of the next launch or
// state access (as surge.hip does); inside a stream capture that is refused.
#include "bank_core.h"
#include "tile_chain_device.h"

#include <cmath>
#include <vector>

#pragma clang fp contract(off)

namespace
{
    using mi_tile_chain::store_quad;

    enum { BYPASS, BYPASS_WET, BYPASS_DRYWET, CROSSFADE };
    enum { VEC_DST = 1, VEC_A = 2, VEC_B = 4 };
    enum { TAIL_ZERO, TAIL_COPY, TAIL_SCALE };
    constexpr int BLOCK = 256;
    constexpr int CHUNK = 4 * BLOCK;                    // samples of a ramp per trip through LDS: one quad per thread
    constexpr uint32_t WALK = 32;                       // gains between two looks of the chain at whether the ramp has ended
    constexpr size_t COUNT_LIMIT = size_t(1) << 31;     // the kernel counts samples in 32 bits

    // nState | nCounter, fDelta, fGain
    struct device_state { uint32_t word; float delta, gain; };

    // a thread's four samples q .. q + 3 of a row, those in [lo, hi); the others read as 0
    __device__ __forceinline__ void load_quad(float (&v)[4], const float *row, bool wide, uint32_t q, uint32_t lo, uint32_t hi)
    {
        if (wide && q >= lo && q + 4 <= hi)
        {
            const float4 t = *reinterpret_cast<const float4 *>(row + q);
            v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
        }
        else
        {
            #pragma unroll
            for (uint32_t j = 0; j < 4; ++j)
                v[j] = (q + j >= lo && q + j < hi) ? row[q + j] : 0.0f;
        }
    }

    // ... and back: store_quad's rule, with a lower bound as well
    __device__ __forceinline__ void save_quad(float *row, const float (&v)[4], bool wide, uint32_t q, uint32_t lo, uint32_t hi)
    {
        if (q >= lo)
            store_quad(row + q, v, wide, q, hi);
        else
        {
            #pragma unroll
            for (uint32_t j = 0; j < 4; ++j)
                if (q + j >= lo && q + j < hi)
                    row[q + j] = v[j];
        }
    }

    // one ramp sample: a = dry | fade_out, b = wet | fade_in (has_a, has_b: the row is there), g = the gain before the step
    template <int KIND>
    __device__ __forceinline__ float mix(float a, float b, float g, bool has_a, bool has_b, float dry_gain, float wet_gain)
    {
        if (KIND == CROSSFADE)
        {
            if (has_a && has_b)
                return a + (b - a) * g;                             // Crossfade.cpp:141
            return has_b ? b * g : a * (1.0f - g);                  // :97, :120
        }
        if (!has_a)
            return (KIND == BYPASS) ? b * g : (b * g) * wet_gain;   // Bypass.cpp:168, :270, :372
        if (KIND == BYPASS)
            return a + (b - a) * g;                                 // :120
        if (KIND == BYPASS_WET)
            return a + (b * wet_gain - a) * g;                      // :222
        return a + (b * wet_gain - a * dry_gain) * g;               // :324
    }

    // does the ramp go on at a sample whose gain before the step is g?  (the crossfade counts instead)
    __device__ __forceinline__ bool ramps(bool up, float g)
    {
        return up ? (g < 1.0f) : (g > 0.0f);                        // Bypass.cpp:118, :140
    }

    template <int KIND>
    __global__ __launch_bounds__(BLOCK) void ramp_mix_kernel(float *dst, const float *a, const float *b, size_t dst_stride,
                                                             size_t a_stride, size_t b_stride, uint32_t count, float dry_gain,
                                                             float wet_gain, device_state *state, uint32_t vec)
    {
        __shared__ __attribute__((aligned(16))) float gains[CHUNK + WALK];
        __shared__ uint32_t ramp_end;
        const uint32_t tid = threadIdx.x, ch = blockIdx.x;
        device_state s = state[ch];
        s.word = __builtin_amdgcn_readfirstlane(s.word);
        s.delta = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(s.delta)));
        s.gain = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(s.gain)));
        __syncthreads();                                            // everybody has the state before thread 0 may write it
        const bool has_a = a != nullptr, has_b = b != nullptr;
        float *d = dst + size_t(ch) * dst_stride;
        const float *ra = has_a ? a + size_t(ch) * a_stride : nullptr, *rb = has_b ? b + size_t(ch) * b_stride : nullptr;
        const bool up = s.delta > 0.0f;                             // anything else, NaN too, goes down: Bypass.cpp:115

        uint32_t pos = 0;
        if (KIND == CROSSFADE && !has_a && !has_b)
        {
            // Crossfade.cpp:86-88: the fade moves on without a loop, one product and one sum
            const uint32_t n = (s.word < count) ? s.word : count;
            s.word -= n;
            s.gain += s.delta * float(n);
        }
        else
        {
            bool ramping = (KIND == CROSSFADE) ? s.word > 0 : ramps(up, s.gain);
            while (ramping && pos < count)
            {
                const uint32_t n = (count - pos < uint32_t(CHUNK)) ? count - pos : uint32_t(CHUNK);
                const uint32_t steps = (KIND == CROSSFADE && s.word < n) ? s.word : n;
                if (tid == 0)
                {
                    // gains[0 .. steps], rounded up to whole runs of WALK (at most CHUNK + WALK floats)
                    float g = s.gain;
                    const float dl = s.delta;
                    for (uint32_t i = 0; i <= steps; i += WALK)
                    {
                        float last = g;
                        #pragma unroll
                        for (uint32_t k = 0; k < WALK; k += 4)
                        {
                            float4 v;
                            v.x = g; g += dl;
                            v.y = g; g += dl;
                            v.z = g; g += dl;
                            v.w = g; g += dl;
                            *reinterpret_cast<float4 *>(&gains[i + k]) = v;
                            last = v.w;
                        }
                        // The gains of a ramp never come back once they have left it (fDelta > 0 keeps them at or above 1,
                        // anything else at or below 0 or NaN), so a run whose last gain is outside holds the ramp's end and
                        // the walk stops there: a ramp of 240 samples is not walked for a chunk's 1024.  One look per run:
                        // the compare and its branch cost the lane as much as a dozen of the adds.
                        if (KIND != CROSSFADE && !ramps(up, last))
                            break;
                    }
                    ramp_end = steps;
                }
                __syncthreads();
                if (KIND != CROSSFADE)
                {
                    const float4 g4 = *reinterpret_cast<const float4 *>(&gains[4 * tid]);
                    const float g[4] = { g4.x, g4.y, g4.z, g4.w };
                    uint32_t first = n;
                    #pragma unroll
                    for (int j = 3; j >= 0; --j)
                        if (4 * tid + j < n && !ramps(up, g[j]))
                            first = 4 * tid + j;
                    if (first < n)
                        atomicMin(&ramp_end, first);
                    __syncthreads();
                }
                const uint32_t len = __builtin_amdgcn_readfirstlane(ramp_end);
                const float g_end = gains[len];
                const uint32_t q = 4 * tid;
                if (q < len)
                {
                    float va[4] = { 0.0f, 0.0f, 0.0f, 0.0f }, vb[4] = { 0.0f, 0.0f, 0.0f, 0.0f }, o[4];
                    if (has_a)
                        load_quad(va, ra + pos, vec & VEC_A, q, 0, len);
                    if (has_b)
                        load_quad(vb, rb + pos, vec & VEC_B, q, 0, len);
                    const float4 g4 = *reinterpret_cast<const float4 *>(&gains[q]);
                    const float g[4] = { g4.x, g4.y, g4.z, g4.w };
                    #pragma unroll
                    for (int j = 0; j < 4; ++j)
                        o[j] = mix<KIND>(va[j], vb[j], g[j], has_a, has_b, dry_gain, wet_gain);
                    store_quad(d + pos + q, o, vec & VEC_DST, q, len);
                }
                pos += len;
                s.gain = g_end;
                if (KIND == CROSSFADE)
                    s.word -= len;
                ramping = (len == n) && ((KIND == CROSSFADE) ? s.word > 0 : ramps(up, s.gain));
                __syncthreads();                                    // the gains are read before the next chunk's are written
            }
        }

        if (pos < count)
        {
            // what is left after the ramp: the clamp (Bypass.cpp:132-133, :154-155) and one row, scaled, copied or zeroed
            int tail = TAIL_ZERO;
            const float *src = nullptr;
            bool wide = false;
            float k = 0.0f;
            if (KIND == CROSSFADE)
            {
                const bool in_side = s.gain > 0.0f;                 // Crossfade.cpp:108, :131, :153
                src = in_side ? rb : ra;
                wide = in_side ? (vec & VEC_B) : (vec & VEC_A);
                tail = (src != nullptr) ? TAIL_COPY : TAIL_ZERO;
            }
            else if (up)
            {
                s.gain = 1.0f, s.word = MI_BYPASS_OFF;
                src = rb, wide = vec & VEC_B, k = wet_gain;
                tail = (KIND == BYPASS) ? TAIL_COPY : TAIL_SCALE;
            }
            else
            {
                s.gain = 0.0f, s.word = MI_BYPASS_ON;
                src = ra, wide = vec & VEC_A, k = dry_gain;
                tail = !has_a ? TAIL_ZERO : (KIND == BYPASS_DRYWET) ? TAIL_SCALE : TAIL_COPY;
            }
            for (uint32_t q = (pos & ~3u) + 4 * tid; q < count; q += CHUNK)
            {
                float v[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
                if (tail != TAIL_ZERO)
                    load_quad(v, src, wide, q, pos, count);
                if (tail == TAIL_SCALE)
                {
                    #pragma unroll
                    for (int j = 0; j < 4; ++j)
                        v[j] = v[j] * k;                            // dsp::mul_k3
                }
                save_quad(d, v, vec & VEC_DST, q, pos, count);
            }
        }
        if (tid == 0)
            state[ch] = s;
    }

    // what a setter left for the device: `bytes` of `s` over the head of the channel's state
    struct recorded_op { uint32_t channel, bytes; device_state s; };

    // float(sample_rate) * time as init() of both classes forms it; false where the reference's conversion is undefined
    bool ramp_length(int sample_rate, float time, float *length)
    {
        const float l = float(sample_rate) * time;
        if (std::isnan(time) || std::isnan(l) || l >= 4294967296.0f)
            return false;
        *length = (l < 1.0f) ? 1.0f : l;
        return true;
    }
} // namespace

// The host's record of a channel.  Bypass: fDelta, which no kernel changes, and whether bypassing() is known to be
// fDelta < 0.  Crossfade: nSamples, and nCounter as the device will hold it after what is enqueued.
struct ramp_channel { float delta = 0.0f; bool known = false; uint32_t samples = 0, counter = 0; };

struct ramp_bank : mi_bank::tables<ramp_channel, device_state>
{
    std::vector<recorded_op>    ops;                // what the setters do to the state, in call order
    hipStream_t                 last = nullptr;     // the stream of the last process or state call
};
struct mi_bypass_bank : ramp_bank { static constexpr const char *NAME = "mi_bypass_bank"; };
struct mi_crossfade_bank : ramp_bank { static constexpr const char *NAME = "mi_crossfade_bank"; };

namespace
{
    template <class Bank> int ramp_create(Bank **bank, const char *entry, uint32_t channels, const device_state &fresh)
    {
        int r = mi_bank::open(bank, entry, channels);
        if (r != MI_OK)
            return r;
        Bank *b = *bank;
        b->channels = channels;
        b->params.assign(channels, ramp_channel());
        // the state array alone: these banks have no parameter table on the device
        const std::vector<device_state> states(channels, fresh);
        hipError_t e = hipMalloc(reinterpret_cast<void **>(&b->d_state), states.size() * sizeof(device_state));
        if (e == hipSuccess)
            e = hipMemcpy(b->d_state, states.data(), states.size() * sizeof(device_state), hipMemcpyHostToDevice);
        if (e == hipSuccess)
            return MI_OK;
        *bank = nullptr;
        mi_bank::destroy(b);
        return mi::fail(MI_EHIP, "%s: %s", entry, hipGetErrorString(e));
    }

    // the recorded operations onto the device state, in order
    template <class Bank> int ramp_update(Bank *b, hipStream_t st)
    {
        b->last = st;
        if (b->ops.empty())
            return MI_OK;
        const int r = mi::refuse_capture(Bank::NAME, st);
        if (r != MI_OK)
            return r;
        for (const recorded_op &op : b->ops)
            MI_HIP_CHECK(hipMemcpyAsync(b->d_state + op.channel, &op.s, op.bytes, hipMemcpyHostToDevice, st));
        MI_HIP_CHECK(hipStreamSynchronize(st));                     // the list is cleared after this
        b->ops.clear();
        return MI_OK;
    }

    template <class Bank> int ramp_get_state(Bank *b, const char *entry, uint32_t channel, device_state *s, void *stream)
    {
        int r = mi_bank::get_checks(b, entry, channel, s);
        if (r == MI_OK)
            r = mi::refuse_state_access(mi::as_stream(stream));
        if (r == MI_OK)
            r = ramp_update(b, mi::as_stream(stream));              // the setters have acted by now
        if (r == MI_OK)
            r = mi_bank::get_state(b, entry, channel, s, stream);
        return r;
    }

    template <class Bank> int ramp_set_state(Bank *b, const char *entry, uint32_t channel, const void *state, void *stream)
    {
        MI_REQUIRE(b != nullptr, MI_ESTATE, "%s: NULL bank", entry);
        MI_REQUIRE(state != nullptr, MI_EINVAL, "%s: NULL state", entry);
        MI_REQUIRE(channel < b->channels, MI_EINVAL, "%s: channel %u out of range", entry, channel);
        hipStream_t st = mi::as_stream(stream);
        int r = mi::refuse_state_access(st);
        if (r == MI_OK)
            r = ramp_update(b, st);                                 // what was recorded before this call does not undo it
        if (r != MI_OK)
            return r;
        device_state s;
        memcpy(&s, state, sizeof(s));
        return mi_bank::set_state(b, entry, channel, s, true, st);
    }

    // Bypass::bypassing() (Bypass.cpp:84-93) of a state
    bool bypassing_of(const device_state &s)
    {
        return s.word == MI_BYPASS_ON || (s.word == MI_BYPASS_ACTIVE && s.delta < 0.0f);
    }

    // Is bypassing() of a channel with this state fDelta < 0 whatever the kernels do to it?  For a finite fDelta that is not 0:
    // S_ACTIVE says so itself (Bypass.cpp:90), and a ramp only ever ends in S_OFF with fDelta > 0 and in S_ON otherwise
    // (:133, :155), which init() and set_bypass() keep; so it holds for as long as it held at the last set_state().
    bool sign_tells(const device_state &s)
    {
        if (!std::isfinite(s.delta) || s.delta == 0.0f)
            return false;
        return s.word == MI_BYPASS_ACTIVE || (s.word == MI_BYPASS_ON && s.delta < 0.0f) || (s.word == MI_BYPASS_OFF && s.delta > 0.0f);
    }

    // set_bypass() of one channel, Bypass.cpp:53-82
    int bypass_switch(mi_bypass_bank *b, uint32_t ch, bool bypass, bool *changed)
    {
        ramp_channel &c = b->params[ch];
        if (c.known)
            *changed = bypass != (c.delta < 0.0f);
        else
        {
            device_state s;
            const int r = ramp_get_state(b, "mi_bypass_bank_set_bypass", ch, &s, b->last);
            if (r != MI_OK)
                return r;
            const bool valid = s.word <= MI_BYPASS_OFF;
            *changed = valid && bypass != bypassing_of(s);
            c.delta = s.delta;
        }
        if (!*changed)
            return MI_OK;
        c.delta = -c.delta;
        c.known = sign_tells(device_state{ MI_BYPASS_ACTIVE, c.delta, 0.0f });
        b->ops.push_back(recorded_op{ ch, 8, device_state{ MI_BYPASS_ACTIVE, c.delta, 0.0f } });    // fGain stays
        return MI_OK;
    }

    template <int KIND>
    int ramp_process(ramp_bank *b, int r, const char *entry, float *dst, const float *a, const float *bb, float dry_gain,
                     float wet_gain, size_t count, size_t dst_stride, size_t a_stride, size_t b_stride, hipStream_t st)
    {
        if (r != MI_OK || count == 0)
            return r;
        const uint32_t second = (KIND == CROSSFADE) ? 0 : mi_bank::REQUIRED;
        const int k = mi_bank::check_rows(entry, b->channels, count, COUNT_LIMIT,
                                          { { dst, dst_stride, count, mi_bank::REQUIRED | mi_bank::OUTPUT },
                                            { a, a_stride, count, 0 }, { bb, b_stride, count, second } });
        if (k != MI_OK)
            return k;
        const uint32_t vec = (mi::aligned16(dst, dst_stride, b->channels) ? VEC_DST : 0) |
                             (mi::aligned16(a, a_stride, b->channels) ? VEC_A : 0) | (mi::aligned16(bb, b_stride, b->channels) ? VEC_B : 0);
        hipEvent_t ev0 = nullptr, ev1 = nullptr;
        mi::take_profile_events(&ev0, &ev1);
        MI_LAUNCH(ramp_mix_kernel<KIND>, dim3(b->channels), dim3(BLOCK), 0, st, ev0, ev1, dst, a, bb, dst_stride, a_stride, b_stride,
                  uint32_t(count), dry_gain, wet_gain, b->d_state, vec);
        MI_HIP_CHECK(hipGetLastError());
        return MI_OK;
    }

    template <int KIND>
    int bypass_process(mi_bypass_bank *b, const char *entry, float *dst, const float *dry, const float *wet, float dry_gain,
                       float wet_gain, size_t count, size_t dst_stride, size_t dry_stride, size_t wet_stride, void *stream)
    {
        MI_REQUIRE(b != nullptr, MI_ESTATE, "%s: NULL bank", entry);
        hipStream_t st = mi::as_stream(stream);
        return ramp_process<KIND>(b, ramp_update(b, st), entry, dst, dry, wet, dry_gain, wet_gain, count, dst_stride, dry_stride,
                                  wet_stride, st);
    }

    // the counters' copies, for mi::capture_touch
    uint64_t crossfade_positions(const void *bank)
    {
        uint64_t h = 0;
        for (const ramp_channel &c : static_cast<const mi_crossfade_bank *>(bank)->params)
            h = mi::position_mix(h, c.counter);
        return h;
    }
} // namespace

extern "C" {

int mi_bypass_bank_create(mi_bypass_bank_t **bank, uint32_t channels)                                        // Bypass.cpp:39-44
{
    return ramp_create(bank, "mi_bypass_bank_create", channels, device_state{ MI_BYPASS_OFF, 0.0f, 0.0f });
}

int mi_bypass_bank_destroy(mi_bypass_bank_t *b)
{
    return mi_bank::destroy(b);
}

int mi_bypass_bank_init(mi_bypass_bank_t *b, uint32_t channel, int sample_rate, float time)                  // :95-104
{
    float length = 0.0f;
    MI_REQUIRE(ramp_length(sample_rate, time, &length), MI_EINVAL, "mi_bypass_bank_init: %d Hz x %g s is no ramp length", sample_rate,
               double(time));
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_bypass_bank_init: NULL bank");
    MI_REQUIRE(channel < b->channels || channel == UINT32_MAX, MI_EINVAL, "mi_bypass_bank_init: channel %u out of range", channel);
    const device_state s = { MI_BYPASS_OFF, 1.0f / length, 1.0f };
    for (uint32_t ch = 0; ch < b->channels; ++ch)
        if (channel == UINT32_MAX || ch == channel)
        {
            b->params[ch].delta = s.delta, b->params[ch].known = sign_tells(s);
            b->ops.push_back(recorded_op{ ch, sizeof(device_state), s });
        }
    return MI_OK;
}

int mi_bypass_bank_set_bypass(mi_bypass_bank_t *b, uint32_t channel, int bypass, int *changed)               // :53-82
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_bypass_bank_set_bypass: NULL bank");
    MI_REQUIRE(channel < b->channels || channel == UINT32_MAX, MI_EINVAL, "mi_bypass_bank_set_bypass: channel %u out of range", channel);
    MI_REQUIRE(changed != nullptr || channel == UINT32_MAX, MI_EINVAL, "mi_bypass_bank_set_bypass: NULL result pointer");
    int n = 0;
    for (uint32_t ch = 0; ch < b->channels; ++ch)
        if (channel == UINT32_MAX || ch == channel)
        {
            bool one = false;
            const int r = bypass_switch(b, ch, bypass != 0, &one);
            if (r != MI_OK)
                return r;
            n += one ? 1 : 0;
        }
    if (changed != nullptr)
        *changed = n;
    return MI_OK;
}

int mi_bypass_bank_bypassing(mi_bypass_bank_t *b, uint32_t channel, int *bypassing, void *stream)            // :84-93
{
    int r = mi_bank::get_checks(b, "mi_bypass_bank_bypassing", channel, bypassing);
    if (r != MI_OK)
        return r;
    if (b->params[channel].known)
    {
        *bypassing = b->params[channel].delta < 0.0f;
        return MI_OK;
    }
    device_state s;
    r = ramp_get_state(b, "mi_bypass_bank_bypassing", channel, &s, stream);
    if (r == MI_OK)
        *bypassing = bypassing_of(s);
    return r;
}

int mi_bypass_bank_get_state(mi_bypass_bank_t *b, uint32_t channel, mi_bypass_state_t *state, void *stream)
{
    device_state s;
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_bypass_bank_get_state: NULL bank");
    MI_REQUIRE(state != nullptr, MI_EINVAL, "mi_bypass_bank_get_state: NULL state");
    const int r = ramp_get_state(b, "mi_bypass_bank_get_state", channel, &s, stream);
    if (r == MI_OK)
        state->state = s.word, state->delta = s.delta, state->gain = s.gain;
    return r;
}

int mi_bypass_bank_set_state(mi_bypass_bank_t *b, uint32_t channel, const mi_bypass_state_t *state, void *stream)
{
    const int r = ramp_set_state(b, "mi_bypass_bank_set_state", channel, state, stream);
    if (r == MI_OK)
    {
        const device_state s = { state->state, state->delta, state->gain };
        b->params[channel].delta = s.delta, b->params[channel].known = sign_tells(s);
    }
    return r;
}

int mi_bypass_bank_process(mi_bypass_bank_t *b, float *dst, const float *dry, const float *wet, size_t count, size_t dst_stride,
                           size_t dry_stride, size_t wet_stride, void *stream)                               // :106-206
{
    return bypass_process<BYPASS>(b, "mi_bypass_bank_process", dst, dry, wet, 1.0f, 1.0f, count, dst_stride, dry_stride, wet_stride,
                                  stream);
}

int mi_bypass_bank_process_wet(mi_bypass_bank_t *b, float *dst, const float *dry, const float *wet, float wet_gain, size_t count,
                               size_t dst_stride, size_t dry_stride, size_t wet_stride, void *stream)        // :208-308
{
    return bypass_process<BYPASS_WET>(b, "mi_bypass_bank_process_wet", dst, dry, wet, 1.0f, wet_gain, count, dst_stride, dry_stride,
                                      wet_stride, stream);
}

int mi_bypass_bank_process_drywet(mi_bypass_bank_t *b, float *dst, const float *dry, const float *wet, float dry_gain,
                                  float wet_gain, size_t count, size_t dst_stride, size_t dry_stride, size_t wet_stride,
                                  void *stream)                                                              // :310-410
{
    return bypass_process<BYPASS_DRYWET>(b, "mi_bypass_bank_process_drywet", dst, dry, wet, dry_gain, wet_gain, count, dst_stride,
                                         dry_stride, wet_stride, stream);
}

int mi_crossfade_bank_create(mi_crossfade_bank_t **bank, uint32_t channels)                                  // Crossfade.cpp:39-45
{
    return ramp_create(bank, "mi_crossfade_bank_create", channels, device_state{ 0, 0.0f, 1.0f });
}

int mi_crossfade_bank_destroy(mi_crossfade_bank_t *b)
{
    return mi_bank::destroy(b);
}

int mi_crossfade_bank_init(mi_crossfade_bank_t *b, uint32_t channel, int sample_rate, float time)            // :51-55
{
    float length = 0.0f;
    MI_REQUIRE(ramp_length(sample_rate, time, &length), MI_EINVAL, "mi_crossfade_bank_init: %d Hz x %g s is no fade length", sample_rate,
               double(time));
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_crossfade_bank_init: NULL bank");
    MI_REQUIRE(channel < b->channels || channel == UINT32_MAX, MI_EINVAL, "mi_crossfade_bank_init: channel %u out of range", channel);
    for (uint32_t ch = 0; ch < b->channels; ++ch)
        if (channel == UINT32_MAX || ch == channel)
            b->params[ch].samples = uint32_t(length);               // 1 <= length < 2^32
    return MI_OK;
}

int mi_crossfade_bank_toggle(mi_crossfade_bank_t *b, uint32_t channel, int *toggled)                         // :57-67
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_crossfade_bank_toggle: NULL bank");
    MI_REQUIRE(channel < b->channels || channel == UINT32_MAX, MI_EINVAL, "mi_crossfade_bank_toggle: channel %u out of range", channel);
    MI_REQUIRE(toggled != nullptr || channel == UINT32_MAX, MI_EINVAL, "mi_crossfade_bank_toggle: NULL result pointer");
    int n = 0;
    for (uint32_t ch = 0; ch < b->channels; ++ch)
        if ((channel == UINT32_MAX || ch == channel) && b->params[ch].counter == 0)
        {
            ramp_channel &c = b->params[ch];
            c.counter = c.samples;
            b->ops.push_back(recorded_op{ ch, sizeof(device_state), device_state{ c.samples, 1.0f / float(c.samples), 0.0f } });
            ++n;
        }
    if (toggled != nullptr)
        *toggled = n;
    return MI_OK;
}

int mi_crossfade_bank_reset(mi_crossfade_bank_t *b, uint32_t channel)                                        // :69-74
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_crossfade_bank_reset: NULL bank");
    MI_REQUIRE(channel < b->channels || channel == UINT32_MAX, MI_EINVAL, "mi_crossfade_bank_reset: channel %u out of range", channel);
    for (uint32_t ch = 0; ch < b->channels; ++ch)
        if (channel == UINT32_MAX || ch == channel)
        {
            b->params[ch].counter = 0;
            b->ops.push_back(recorded_op{ ch, sizeof(device_state), device_state{ 0, 0.0f, 0.0f } });
        }
    return MI_OK;
}

int mi_crossfade_bank_remaining(const mi_crossfade_bank_t *b, uint32_t channel, size_t *remaining)
{
    const int r = mi_bank::get_checks(b, "mi_crossfade_bank_remaining", channel, remaining);
    if (r == MI_OK)
        *remaining = b->params[channel].counter;
    return r;
}

int mi_crossfade_bank_get_state(mi_crossfade_bank_t *b, uint32_t channel, mi_crossfade_state_t *state, void *stream)
{
    device_state s;
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_crossfade_bank_get_state: NULL bank");
    MI_REQUIRE(state != nullptr, MI_EINVAL, "mi_crossfade_bank_get_state: NULL state");
    const int r = ramp_get_state(b, "mi_crossfade_bank_get_state", channel, &s, stream);
    if (r == MI_OK)
        state->counter = s.word, state->delta = s.delta, state->gain = s.gain;
    return r;
}

int mi_crossfade_bank_set_state(mi_crossfade_bank_t *b, uint32_t channel, const mi_crossfade_state_t *state, void *stream)
{
    const int r = ramp_set_state(b, "mi_crossfade_bank_set_state", channel, state, stream);
    if (r == MI_OK)
        b->params[channel].counter = state->counter;
    return r;
}

int mi_crossfade_bank_process(mi_crossfade_bank_t *b, float *dst, const float *fade_out, const float *fade_in, size_t count,
                              size_t dst_stride, size_t out_stride, size_t in_stride, void *stream)          // :76-156
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_crossfade_bank_process: NULL bank");
    hipStream_t st = mi::as_stream(stream);
    int r = mi::capture_touch(st, b, "crossfade", crossfade_positions);
    if (r == MI_OK)
        r = ramp_update(b, st);
    r = ramp_process<CROSSFADE>(b, r, "mi_crossfade_bank_process", dst, fade_out, fade_in, 1.0f, 1.0f, count, dst_stride, out_stride,
                                in_stride, st);
    if (r == MI_OK)
        for (ramp_channel &c : b->params)
            c.counter -= (c.counter < count) ? c.counter : uint32_t(count);     // every variant takes min(nCounter, count)
    return r;
}

} // extern "C"
