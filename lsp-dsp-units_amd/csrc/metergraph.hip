// lsp::dspu::MeterGraph as a bank of `channels` graphs (src/main/util/MeterGraph.cpp): a full-rate row cut into frames of nPeriod
// samples, each reduced by the channel's method and appended to a ring of display frames on the device.
//
// metergraph_kernel: a workgroup per channel.  The chunk boundaries of a call are a closed form of nCount, nPeriod and count
// (metergraph_bank.h), so nothing in a call depends on anything but the carry into its first chunk:
//     the first chunk          by the whole workgroup; folds into fCurrent where the frame is open (the ABS_MAXIMUM quirk lives
//                              there); closes a frame or ends the call
//     the whole periods        independent of each other: period >= 1024 by the workgroup in turn, period >= 256 a wave per
//                              frame, period >= 64 sixteen lanes per frame, below that a lane per frame
//     the tail                 by the workgroup: opens the frame that the next call goes on with
// The row is read once, 16 bytes per lane on the 16-byte grid whatever the row's base is (metergraph_device.h).  A call may append
// more frames than the ring holds: only the last `frames` of them are stored (and, of the whole periods, computed), each by one
// lane into a slot of its own, so no two stores of a call meet.  The kernel writes fCurrent, nCount and nHead back: a captured
// call appends again at every replay.
//
// metergraph_value_kernel is process(float) (:70-111), a lane per channel; metergraph_read_kernel is read() (:246-258) and
// metergraph_level_kernel level() (.h:173).  Everything is the reference's in every bit: there is no arithmetic but fabsf,
// compares and the product with the gain.
#include "bank_core.h"
#include "metergraph_device.h"

#pragma clang fp contract(off)

namespace
{
    using namespace mi_metergraph;

    constexpr int BLOCK = 256, WAVE = 64, WAVES = BLOCK / WAVE;
    constexpr uint32_t BLOCK_PERIOD = 1024;             // whole periods from here on take the workgroup, one after another
    constexpr uint32_t GROUP_PERIOD = 256, SMALL_GROUP = 16;    // ... from here on a wave each, below that 16 lanes, below 64 a lane
    constexpr size_t COUNT_LIMIT = size_t(1) << 31;     // the kernel counts samples in 32 bits
    constexpr uint32_t FRAMES_LIMIT = 1u << 20;

    struct device_state { float current; uint32_t count, head; };               // fCurrent, nCount, nHead
    enum { OP_FILL = 1, OP_RESET = 2 };
    struct fill_op { uint32_t flags; float value; };                            // what init(), fill() and clear() left to do

    // the best key of the workgroup in every thread; `part` is scratch of WAVES keys
    __device__ __forceinline__ mkey block_best(mkey k, mkey *part)
    {
        k = wave_best(k);
        __syncthreads();                                                        // the scratch's last readers are through
        if ((threadIdx.x & (WAVE - 1)) == 0)
            part[threadIdx.x / WAVE] = k;
        __syncthreads();
        mkey best = part[0];
        #pragma unroll
        for (int w = 1; w < WAVES; ++w)
            best = better(best, part[w]);
        return best;
    }

    __global__ __launch_bounds__(BLOCK) void metergraph_kernel(const float *src, const float *gains, size_t stride, uint32_t n,
                                                               const mi_metergraph_params_t *params, device_state *state, float *ring,
                                                               uint32_t max_frames)
    {
        __shared__ mkey part[WAVES];
        const uint32_t ch = blockIdx.x, t = threadIdx.x;
        const mi_metergraph_params_t p = params[ch];
        const device_state s = state[ch];
        __syncthreads();                                                        // every thread has the state before one writes it
        const float *xs = src + size_t(ch) * stride;
        float *rg = ring + size_t(ch) * max_frames;
        const bool has_gain = gains != nullptr;
        const float gain = has_gain ? gains[ch] : 1.0f;
        const uint32_t method = p.method, period = p.period, frames = p.frames;

        const plan pl = make_plan(s.count, period, n);
        // frame j of the call goes to slot (nHead + j) % nCapacity (RingBuffer.cpp:102-106); only the last `frames` are stored
        const uint32_t keep_from = (pl.frames > frames) ? pl.frames - frames : 0;
        auto store_frame = [&](uint32_t j, float v)
        {
            if (j >= keep_from)
                rg[(s.head + j) % frames] = v;
        };

        float current = s.current;
        uint32_t j = 0;
        if (pl.pre)                                                             // nCount == nPeriod: a frame before any sample
        {
            if (t == 0)
                store_frame(j, current);
            ++j;
        }
        {
            const mkey k = block_best(chunk_key(xs, pl.first_len, method, t, BLOCK), part);
            const float v = chunk_value(xs, key_index(k), method, has_gain, gain);
            current = (pl.pre || s.count == 0) ? v : fold_block(method, current, v);
            if (pl.first_frame)
            {
                if (t == 0)
                    store_frame(j, current);
                ++j;
            }
        }
        const float *fs = xs + pl.first_len;                                    // the whole periods start here
        const uint32_t f0 = (keep_from > j) ? keep_from - j : 0;                // the first of them that is stored
        if (period >= BLOCK_PERIOD)
        {
            for (uint32_t f = f0; f < pl.full; ++f)
            {
                const float *cs = fs + size_t(f) * period;
                const mkey k = block_best(chunk_key(cs, period, method, t, BLOCK), part);
                current = chunk_value(cs, key_index(k), method, has_gain, gain);
                if (t == 0)
                    store_frame(j + f, current);
            }
        }
        else if (period >= WAVE)
        {
            // a group of lanes per frame: a wave, or 16 lanes where a period is too short to give 64 lanes 16 bytes each (the
            // lanes of a group run the same number of frames, so a shuffle never reads a lane that has left the loop)
            const uint32_t group = (period >= GROUP_PERIOD) ? WAVE : SMALL_GROUP;
            const uint32_t gl = t & (group - 1);
            for (uint32_t f = f0 + t / group; f < pl.full; f += BLOCK / group)
            {
                const float *cs = fs + size_t(f) * period;
                const mkey k = group_best(chunk_key(cs, period, method, gl, group), group);
                const float v = chunk_value(cs, key_index(k), method, has_gain, gain);
                if (gl == 0)
                {
                    store_frame(j + f, v);
                    if (f + 1 == pl.full && pl.tail == 0)
                        state[ch].current = v;                                  // the call ends with this frame
                }
            }
        }
        else
        {
            for (uint32_t f = f0 + t; f < pl.full; f += BLOCK)
            {
                const float *cs = fs + size_t(f) * period;
                mkey k = 0;
                if (method != MI_MM_PEAK)
                    for (uint32_t i = 0; i < period; ++i)
                        k = better(k, is_max(method) ? element_key<true>(cs[i], i) : element_key<false>(cs[i], i));
                else
                    k = element_key<true>(0.0f, 0);
                const float v = chunk_value(cs, key_index(k), method, has_gain, gain);
                store_frame(j + f, v);
                if (f + 1 == pl.full && pl.tail == 0)
                    state[ch].current = v;
            }
        }
        const bool written = pl.full != 0 && pl.tail == 0 && period < BLOCK_PERIOD;     // fCurrent is the last whole period's
        if (pl.tail != 0)
        {
            const float *cs = fs + size_t(pl.full) * period;
            const mkey k = block_best(chunk_key(cs, pl.tail, method, t, BLOCK), part);
            current = chunk_value(cs, key_index(k), method, has_gain, gain);
        }
        if (t == 0)
        {
            if (!written)
                state[ch].current = current;
            state[ch].count = pl.count_after;
            state[ch].head = uint32_t((size_t(s.head) + pl.frames) % frames);
        }
    }

    // process(float sample) of every channel, :70-111
    __global__ __launch_bounds__(BLOCK) void metergraph_value_kernel(const float *values, uint32_t channels,
                                                                     const mi_metergraph_params_t *params, device_state *state, float *ring,
                                                                     uint32_t max_frames)
    {
        const uint32_t ch = blockIdx.x * BLOCK + threadIdx.x;
        if (ch >= channels)
            return;
        const mi_metergraph_params_t p = params[ch];
        device_state s = state[ch];
        const float x = values[ch];
        s.current = (s.count == 0) ? first_single(p.method, x) : fold_single(p.method, s.current, x);
        if (++s.count >= p.period)                                              // :105
        {
            ring[size_t(ch) * max_frames + s.head] = s.current;                 // RingBuffer.cpp:102-106
            s.head = (s.head + 1) % p.frames;
            s.count = 0;
        }
        state[ch] = s;
    }

    // read(dst, count), :246-258: fDefault ahead of the frames where count exceeds the capacity, then get(dst, count - 1, count)
    __global__ __launch_bounds__(BLOCK) void metergraph_read_kernel(float *dst, size_t stride, uint32_t count,
                                                                    const mi_metergraph_params_t *params, const device_state *state,
                                                                    const float *ring, uint32_t max_frames)
    {
        const uint32_t ch = blockIdx.y, i = blockIdx.x * BLOCK + threadIdx.x;
        if (i >= count)
            return;
        const mi_metergraph_params_t p = params[ch];
        const uint32_t lead = (count > p.frames) ? count - p.frames : 0;        // delta, :249
        float v = p.default_value;
        if (i >= lead)
        {
            const uint32_t offset = count - 1 - i;                              // frames behind the newest, below nCapacity
            v = ring[size_t(ch) * max_frames + (state[ch].head + p.frames - offset - 1) % p.frames];   // RingBuffer.cpp:166
        }
        dst[size_t(ch) * stride + i] = v;
    }

    // level(), .h:173: sBuffer.get(0)
    __global__ __launch_bounds__(BLOCK) void metergraph_level_kernel(float *levels, uint32_t channels, const mi_metergraph_params_t *params,
                                                                     const device_state *state, const float *ring, uint32_t max_frames)
    {
        const uint32_t ch = blockIdx.x * BLOCK + threadIdx.x;
        if (ch >= channels)
            return;
        const uint32_t frames = params[ch].frames;
        levels[ch] = ring[size_t(ch) * max_frames + (state[ch].head + frames - 1) % frames];           // RingBuffer.cpp:127
    }

    // what init(), fill() and clear() left: the ring's words and nHead = 0 (RingBuffer.cpp:115-120); init() also fCurrent and nCount
    __global__ __launch_bounds__(BLOCK) void metergraph_fill_kernel(const fill_op *ops, const mi_metergraph_params_t *params,
                                                                    device_state *state, float *ring, uint32_t max_frames)
    {
        const uint32_t ch = blockIdx.x;
        const fill_op op = ops[ch];
        if (!(op.flags & OP_FILL))
            return;
        const uint32_t frames = params[ch].frames;
        for (uint32_t i = threadIdx.x; i < frames; i += BLOCK)
            ring[size_t(ch) * max_frames + i] = op.value;
        if (threadIdx.x == 0)
        {
            state[ch].head = 0;
            if (op.flags & OP_RESET)
                state[ch].current = 0.0f, state[ch].count = 0;
        }
    }
} // namespace

struct mi_metergraph_bank : mi_bank::tables<mi_metergraph_params_t, device_state>
{
    static constexpr const char *NAME = "mi_metergraph_bank";

    uint32_t                max_frames = 0;
    float                  *d_ring = nullptr;       // [channels][max_frames]
    fill_op                *d_ops = nullptr;        // [channels]
    std::vector<fill_op>    ops;                    // pending init() / fill() / clear() of every channel
    bool                    work = false;           // ... of some channel
};

namespace
{
    int mg_destroy(mi_metergraph_bank *b)
    {
        if (b == nullptr)
            return MI_OK;
        (void)hipFree(b->d_ring); (void)hipFree(b->d_ops);
        return mi_bank::destroy(b);
    }

    // the changed settings, then the pending fills
    int mg_update(mi_metergraph_bank *b, hipStream_t st)
    {
        const int r = mi_bank::upload(*b, mi_metergraph_bank::NAME, st);
        if (r != MI_OK || !b->work)
            return r;
        const int k = mi::refuse_capture(mi_metergraph_bank::NAME, st);
        if (k != MI_OK)
            return k;
        MI_HIP_CHECK(hipMemcpyAsync(b->d_ops, b->ops.data(), size_t(b->channels) * sizeof(fill_op), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(metergraph_fill_kernel, dim3(b->channels), dim3(BLOCK), 0, st, b->d_ops, b->d_params, b->d_state, b->d_ring,
                           b->max_frames);
        MI_HIP_CHECK(hipGetLastError());
        MI_HIP_CHECK(hipStreamSynchronize(st));                 // the host's list may change again after this returns
        b->ops.assign(b->channels, fill_op{ 0, 0.0f });
        b->work = false;
        return MI_OK;
    }

    // update, and every channel has a ring
    int mg_ready(mi_metergraph_bank *b, const char *entry, hipStream_t st)
    {
        const int r = mg_update(b, st);
        if (r != MI_OK)
            return r;
        for (uint32_t ch = 0; ch < b->channels; ++ch)
            MI_REQUIRE(b->params[ch].frames != 0 && b->params[ch].period != 0, MI_ESTATE, "%s: channel %u has no ring: call init() first",
                       entry, ch);
        return MI_OK;
    }

    int mg_channel(const mi_metergraph_bank *b, const char *entry, uint32_t channel)
    {
        MI_REQUIRE(b != nullptr, MI_ESTATE, "%s: NULL bank", entry);
        MI_REQUIRE(channel < b->channels, MI_EINVAL, "%s: channel %u out of range", entry, channel);
        return MI_OK;
    }

    bool period_ok(size_t period)   { return period >= 1 && period <= size_t(UINT32_MAX); }

    void pend_fill(mi_metergraph_bank *b, uint32_t ch, uint32_t flags, float value)
    {
        b->ops[ch].flags |= flags;
        b->ops[ch].value = value;
        b->work = true;
    }
} // namespace

extern "C" {

int mi_metergraph_bank_create(mi_metergraph_bank_t **bank, uint32_t channels, uint32_t max_frames)           // construct(), :40-48
{
    int r = mi_bank::open_checks(bank, "mi_metergraph_bank_create", channels);
    if (r != MI_OK)
        return r;
    MI_REQUIRE(max_frames >= 1 && max_frames <= FRAMES_LIMIT, MI_EINVAL, "mi_metergraph_bank_create: max_frames must be 1 .. %u", FRAMES_LIMIT);
    r = mi_bank::open_new(bank, "mi_metergraph_bank_create");
    if (r != MI_OK)
        return r;
    mi_metergraph_bank *b = *bank;
    b->channels = channels;
    b->max_frames = max_frames;
    b->ops.assign(channels, fill_op{ 0, 0.0f });
    r = mi_bank::alloc(*b, "mi_metergraph_bank_create", mi_metergraph_params_t{ MI_MM_ABS_MAXIMUM, 1, 0, 0.0f }, device_state{ 0.0f, 0, 0 });
    if (r == MI_OK)
    {
        hipError_t e = hipMalloc(reinterpret_cast<void **>(&b->d_ring), size_t(channels) * max_frames * sizeof(float));
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&b->d_ops), size_t(channels) * sizeof(fill_op));
        if (e == hipSuccess) e = hipMemset(b->d_ring, 0, size_t(channels) * max_frames * sizeof(float));
        if (e != hipSuccess)
            r = mi::fail(MI_EHIP, "mi_metergraph_bank_create: %s", hipGetErrorString(e));
    }
    if (r != MI_OK)
    {
        *bank = nullptr;
        mg_destroy(b);
    }
    return r;
}

int mi_metergraph_bank_destroy(mi_metergraph_bank_t *b)
{
    return mg_destroy(b);
}

int mi_metergraph_bank_init(mi_metergraph_bank_t *b, uint32_t channel, size_t frames, size_t period, float default_value)    // :55-68
{
    const int r = mg_channel(b, "mi_metergraph_bank_init", channel);
    if (r != MI_OK)
        return r;
    MI_REQUIRE(period_ok(period), MI_EINVAL, "mi_metergraph_bank_init: a period of %zu: the reference refuses 0, and counts in 32 bits", period);
    MI_REQUIRE(frames >= 1 && frames <= b->max_frames, MI_EINVAL, "mi_metergraph_bank_init: frames must be 1 .. %u (max_frames)", b->max_frames);
    mi_metergraph_params_t &p = b->params[channel];
    p.frames = uint32_t(frames), p.period = uint32_t(period), p.default_value = default_value;
    b->up.touch(channel);
    b->ops[channel].flags = 0;                                  // whatever was pending is overwritten
    pend_fill(b, channel, OP_FILL | OP_RESET, default_value);
    return MI_OK;
}

int mi_metergraph_bank_set_method(mi_metergraph_bank_t *b, uint32_t channel, uint32_t method)                // .h:128
{
    const int r = mg_channel(b, "mi_metergraph_bank_set_method", channel);
    if (r != MI_OK)
        return r;
    if (b->params[channel].method != method)
        b->params[channel].method = method, b->up.touch(channel);
    return MI_OK;
}

int mi_metergraph_bank_set_period(mi_metergraph_bank_t *b, uint32_t channel, size_t period)                  // .h:141
{
    const int r = mg_channel(b, "mi_metergraph_bank_set_period", channel);
    if (r != MI_OK)
        return r;
    // with a period of 0 the reference's process() never returns (:118: can_do is 0 for ever once nCount is 0)
    MI_REQUIRE(period_ok(period), MI_EINVAL, "mi_metergraph_bank_set_period: a period of %zu: 0 hangs the reference, and it counts in 32 bits", period);
    if (b->params[channel].period != uint32_t(period))
        b->params[channel].period = uint32_t(period), b->up.touch(channel);
    return MI_OK;
}

int mi_metergraph_bank_set_default_value(mi_metergraph_bank_t *b, uint32_t channel, float value)             // .h:122
{
    const int r = mg_channel(b, "mi_metergraph_bank_set_default_value", channel);
    if (r != MI_OK)
        return r;
    if (memcmp(&b->params[channel].default_value, &value, sizeof(float)) != 0)
        b->params[channel].default_value = value, b->up.touch(channel);
    return MI_OK;
}

int mi_metergraph_bank_fill(mi_metergraph_bank_t *b, uint32_t channel, float level)                          // .h:179
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_metergraph_bank_fill: NULL bank");
    MI_REQUIRE(channel < b->channels || channel == UINT32_MAX, MI_EINVAL, "mi_metergraph_bank_fill: channel %u out of range", channel);
    for (uint32_t ch = 0; ch < b->channels; ++ch)
        if (channel == UINT32_MAX || ch == channel)
            pend_fill(b, ch, OP_FILL, level);
    return MI_OK;
}

int mi_metergraph_bank_clear(mi_metergraph_bank_t *b, uint32_t channel)                                      // .h:184
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_metergraph_bank_clear: NULL bank");
    MI_REQUIRE(channel < b->channels || channel == UINT32_MAX, MI_EINVAL, "mi_metergraph_bank_clear: channel %u out of range", channel);
    for (uint32_t ch = 0; ch < b->channels; ++ch)
        if (channel == UINT32_MAX || ch == channel)
            pend_fill(b, ch, OP_FILL, b->params[ch].default_value);             // fDefault as it is now
    return MI_OK;
}

int mi_metergraph_bank_update_settings(mi_metergraph_bank_t *b, void *stream)
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_metergraph_bank_update_settings: NULL bank");
    return mg_update(b, mi::as_stream(stream));
}

int mi_metergraph_bank_get_params(const mi_metergraph_bank_t *b, uint32_t channel, mi_metergraph_params_t *params)
{
    return mi_bank::get_params(b, "mi_metergraph_bank_get_params", channel, params);
}

int mi_metergraph_bank_get_state(mi_metergraph_bank_t *b, uint32_t channel, mi_metergraph_state_t *state, float *ring, void *stream)
{
    int r = mi_bank::get_checks(b, "mi_metergraph_bank_get_state", channel, state);
    hipStream_t st = mi::as_stream(stream);
    if (r == MI_OK)
        r = mi::refuse_state_access(st);
    if (r == MI_OK)
        r = mg_update(b, st);
    if (r != MI_OK)
        return r;
    if (ring != nullptr && b->params[channel].frames != 0)
        MI_HIP_CHECK(hipMemcpyAsync(ring, b->d_ring + size_t(channel) * b->max_frames, size_t(b->params[channel].frames) * sizeof(float),
                                    hipMemcpyDeviceToHost, st));
    device_state s;
    r = mi::read_state(&s, b->d_state + channel, st);           // synchronises
    if (r != MI_OK)
        return r;
    state->current = s.current, state->count = s.count, state->head = s.head;
    return MI_OK;
}

int mi_metergraph_bank_set_state(mi_metergraph_bank_t *b, uint32_t channel, const mi_metergraph_state_t *state, const float *ring,
                                 void *stream)
{
    int r = mg_channel(b, "mi_metergraph_bank_set_state", channel);
    if (r != MI_OK)
        return r;
    MI_REQUIRE(state != nullptr, MI_EINVAL, "mi_metergraph_bank_set_state: NULL state");
    hipStream_t st = mi::as_stream(stream);
    r = mi::refuse_state_access(st);
    if (r == MI_OK)
        r = mg_update(b, st);                                   // an init() or a fill() before this call does not undo it
    if (r != MI_OK)
        return r;
    const uint32_t frames = b->params[channel].frames;
    MI_REQUIRE(frames != 0, MI_ESTATE, "mi_metergraph_bank_set_state: channel %u has no ring: call init() first", channel);
    MI_REQUIRE(state->head < frames, MI_EINVAL, "mi_metergraph_bank_set_state: head %u outside the ring of %u frames", state->head, frames);
    if (ring != nullptr)
        MI_HIP_CHECK(hipMemcpyAsync(b->d_ring + size_t(channel) * b->max_frames, ring, size_t(frames) * sizeof(float), hipMemcpyHostToDevice, st));
    return mi::write_state(b->d_state + channel, device_state{ state->current, state->count, state->head }, st);
}

int mi_metergraph_bank_process(mi_metergraph_bank_t *b, const float *src, const float *gains, size_t count, size_t stride, void *stream)
{                                                                                                            // :113-244
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_metergraph_bank_process: NULL bank");
    hipStream_t st = mi::as_stream(stream);
    const int r = mg_ready(b, "mi_metergraph_bank_process", st);
    if (r != MI_OK || count == 0)
        return r;
    const int k = mi_bank::check_rows("mi_metergraph_bank_process", b->channels, count, COUNT_LIMIT, { { src, stride, count, mi_bank::REQUIRED } });
    if (k != MI_OK)
        return k;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    mi::take_profile_events(&ev0, &ev1);
    MI_LAUNCH(metergraph_kernel, dim3(b->channels), dim3(BLOCK), 0, st, ev0, ev1, src, gains, stride, uint32_t(count), b->d_params, b->d_state,
              b->d_ring, b->max_frames);
    MI_HIP_CHECK(hipGetLastError());
    return MI_OK;
}

int mi_metergraph_bank_process_value(mi_metergraph_bank_t *b, const float *values, void *stream)            // :70-111
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_metergraph_bank_process_value: NULL bank");
    MI_REQUIRE(values != nullptr, MI_EINVAL, "mi_metergraph_bank_process_value: NULL buffer");
    hipStream_t st = mi::as_stream(stream);
    const int r = mg_ready(b, "mi_metergraph_bank_process_value", st);
    if (r != MI_OK)
        return r;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    mi::take_profile_events(&ev0, &ev1);
    MI_LAUNCH(metergraph_value_kernel, dim3((b->channels + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, st, ev0, ev1, values, b->channels, b->d_params,
              b->d_state, b->d_ring, b->max_frames);
    MI_HIP_CHECK(hipGetLastError());
    return MI_OK;
}

int mi_metergraph_bank_read(mi_metergraph_bank_t *b, float *dst, size_t count, size_t stride, void *stream)  // :246-258
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_metergraph_bank_read: NULL bank");
    hipStream_t st = mi::as_stream(stream);
    const int r = mg_ready(b, "mi_metergraph_bank_read", st);
    if (r != MI_OK || count == 0)
        return r;
    const int k = mi_bank::check_rows("mi_metergraph_bank_read", b->channels, count, COUNT_LIMIT, { { dst, stride, count, mi_bank::REQUIRED } });
    if (k != MI_OK)
        return k;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    mi::take_profile_events(&ev0, &ev1);
    MI_LAUNCH(metergraph_read_kernel, dim3(uint32_t((count + BLOCK - 1) / BLOCK), b->channels), dim3(BLOCK), 0, st, ev0, ev1, dst, stride,
              uint32_t(count), b->d_params, b->d_state, b->d_ring, b->max_frames);
    MI_HIP_CHECK(hipGetLastError());
    return MI_OK;
}

int mi_metergraph_bank_level(mi_metergraph_bank_t *b, float *levels, void *stream)                           // .h:173
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_metergraph_bank_level: NULL bank");
    MI_REQUIRE(levels != nullptr, MI_EINVAL, "mi_metergraph_bank_level: NULL buffer");
    hipStream_t st = mi::as_stream(stream);
    const int r = mg_ready(b, "mi_metergraph_bank_level", st);
    if (r != MI_OK)
        return r;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    mi::take_profile_events(&ev0, &ev1);
    MI_LAUNCH(metergraph_level_kernel, dim3((b->channels + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, st, ev0, ev1, levels, b->channels, b->d_params,
              b->d_state, b->d_ring, b->max_frames);
    MI_HIP_CHECK(hipGetLastError());
    return MI_OK;
}

} // extern "C"
