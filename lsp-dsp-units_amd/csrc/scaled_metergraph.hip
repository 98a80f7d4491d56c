// lsp::dspu::ScaledMeterGraph as a bank of `channels` graphs (src/main/util/ScaledMeterGraph.cpp): a full-rate row sampled twice,
// into a history of sub-samples of `subsampling` samples each and into a ring of display frames of the period last taken over; a
// new period re-decimates the history into the frame ring (update_period(), :269-342).
//
// scaled_metergraph_kernel: a workgroup per channel, one launch per process() (:351-363):
//     the history sampler      over the row, as metergraph_kernel cuts it (first chunk by the workgroup into the open frame, the
//                              whole periods independent of each other, the tail by the workgroup); the carry into an open frame
//                              is this class's (scaled_metergraph_bank.h)
//     the decision             nPeriod != sFrames.nPeriod, from the uploaded target and the sampler state ON THE DEVICE: a captured
//                              call re-decimates at the replay where the two differ and at no other
//     either the re-decimation the pending push, then a lane per output frame with the serial sentinel fold of its group; the
//                              groups are a closed form (scaled_metergraph_bank.h), so the frames are independent of each other
//     or the frames sampler    over the same row
// The row is read twice in one launch; a channel's row stays in the cache for the second pass (fusing the passes
// would cut every chunk at both samplers' boundaries; not measured yet).  Of more frames than a ring holds only the last are stored, each by one lane into a slot of its own: both rings.  The
// kernel writes both samplers' fCurrent and nCount, both heads and sFrames.nPeriod back: a captured call appends again at every
// replay.
//
// scaled_metergraph_value_kernel is process(float) (:344-349) with its update_period(), a lane per channel;
// scaled_metergraph_read_kernel is read() (:365-369), scaled_metergraph_level_kernel level() (:371-374).  Everything is the
// reference's in every bit: there is no arithmetic but fabsf, compares and the product with the gain.
#include "bank_core.h"
#include "metergraph_device.h"
#include "scaled_metergraph_bank.h"

#pragma clang fp contract(off)

namespace
{
    using namespace mi_metergraph;
    namespace sm = mi_scaled_metergraph;

    constexpr int BLOCK = 256, WAVE = 64, WAVES = BLOCK / WAVE;
    constexpr uint32_t BLOCK_PERIOD = 1024;             // whole periods from here on take the workgroup, one after another
    constexpr uint32_t GROUP_PERIOD = 256, SMALL_GROUP = 16;    // ... from here on a wave each, below that 16 lanes, below 64 a lane
    constexpr size_t COUNT_LIMIT = size_t(1) << 31;     // the kernel counts samples in 32 bits
    constexpr uint32_t FRAMES_LIMIT = 1u << 20, SUBFRAMES_LIMIT = 1u << 24;

    // what the table holds of a channel: enMethod, the target nPeriod (0: none set yet), nMaxPeriod, sHistory.nPeriod,
    // sFrames.nFrames, sHistory.nFrames
    typedef mi_scaled_metergraph_params_t params_t;
    // sHistory's fCurrent, nCount, nHead, then sFrames' and sFrames.nPeriod
    typedef mi_scaled_metergraph_state_t device_state;
    enum { OP_FILL = 1, OP_RESET = 2 };
    struct fill_op { uint32_t flags; float value; };                            // what init() and fill() left to do

    struct sampler { float current; uint32_t count, head; };

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

    // process_sampler(sampler, src, count) (:147-206) or (sampler, src, gain, count) (:208-267) of one sampler by the workgroup:
    // n samples of xs into the ring rg of `cap` words.  Every thread gets the sampler as the call leaves it.  `last` is a word
    // of shared scratch.  s.count < period, so make_plan's `pre` is not set (scaled_metergraph_bank.h).
    __device__ sampler run_sampler(const float *xs, uint32_t n, uint32_t method, bool has_gain, float gain, sampler s, uint32_t period,
                                   float *rg, uint32_t cap, mkey *part, float *last)
    {
        const uint32_t t = threadIdx.x;
        const plan pl = make_plan(s.count, period, n);
        // frame j of the call goes to slot (nHead + j) % nCapacity (RawRingBuffer.cpp:127-131); only the last `cap` are stored
        const uint32_t keep_from = (pl.frames > cap) ? pl.frames - cap : 0;
        auto store_frame = [&](uint32_t j, float v)
        {
            if (j >= keep_from)
                rg[(s.head + j) % cap] = v;
        };

        float current = s.current;
        uint32_t j = 0;
        {
            const mkey k = block_best(chunk_key(xs, pl.first_len, method, t, BLOCK), part);
            const float v = chunk_value(xs, key_index(k), method, has_gain, gain);
            current = (s.count == 0) ? v : sm::fold_block(method, current, v);
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
                    if (f + 1 == pl.full)
                        *last = v;
                }
            }
        }
        else
        {
            // a lane per frame, 16 bytes at a time where the frame's words are on the 16-byte grid
            for (uint32_t f = f0 + t; f < pl.full; f += BLOCK)
            {
                const float *cs = fs + size_t(f) * period;
                const mkey k = chunk_key(cs, period, method, 0, 1);
                const float v = chunk_value(cs, key_index(k), method, has_gain, gain);
                store_frame(j + f, v);
                if (f + 1 == pl.full)
                    *last = v;
            }
        }
        if (pl.tail != 0)
        {
            const float *cs = fs + size_t(pl.full) * period;
            const mkey k = block_best(chunk_key(cs, pl.tail, method, t, BLOCK), part);
            current = chunk_value(cs, key_index(k), method, has_gain, gain);
        }
        else if (pl.full != 0 && period < BLOCK_PERIOD)                         // fCurrent is the last whole period's
        {
            __syncthreads();                                                    // *last is written
            current = *last;
        }
        return sampler{ current, pl.count_after, uint32_t((size_t(s.head) + pl.frames) % cap) };
    }

    // frame k of the re-decimation (:294-339): the serial sentinel fold of its sub-samples first .. last (1-based, oldest first);
    // sub-sample i is sHistory.sBuffer.read(subsamples - i + 1), RawRingBuffer.cpp:151-155
    __device__ __forceinline__ float redecimated(const float *hist, uint32_t hcap, uint32_t hhead, uint32_t subs, uint32_t k, uint32_t method,
                                                 uint32_t period, uint32_t hp)
    {
        const uint32_t first = sm::group_first(k, period, hp), last = sm::group_last(k, period, hp);
        uint32_t at = (hhead + hcap - (subs - first + 1)) % hcap;              // subs < hcap
        float current = -1.0f;                                                  // :285, :337
        for (uint32_t i = first; i <= last; ++i)
        {
            current = sm::fold_sub(method, current, hist[at]);
            at = (at + 1 == hcap) ? 0 : at + 1;
        }
        return current;
    }

    __global__ __launch_bounds__(BLOCK) void scaled_metergraph_kernel(const float *src, const float *gains, size_t stride, uint32_t n,
                                                                      const params_t *params, device_state *state, float *history,
                                                                      float *ring, uint32_t max_subframes, uint32_t max_frames)
    {
        __shared__ mkey part[WAVES];
        __shared__ float last;
        const uint32_t ch = blockIdx.x, t = threadIdx.x;
        const params_t p = params[ch];
        if (p.period == 0 || p.frames == 0)                                     // the host refuses these; a replayed graph may meet an init() since
            return;
        const device_state s = state[ch];
        __syncthreads();                                                        // every thread has the state before one writes it
        const float *xs = src + size_t(ch) * stride;
        float *hist = history + size_t(ch) * (size_t(max_subframes) + sm::FRAMES_GAP);
        float *rg = ring + size_t(ch) * (size_t(max_frames) + sm::FRAMES_GAP);
        const uint32_t hcap = p.subframes + sm::FRAMES_GAP, fcap = p.frames + sm::FRAMES_GAP;
        const bool has_gain = gains != nullptr;
        const float gain = has_gain ? gains[ch] : 1.0f;

        sampler h = run_sampler(xs, n, p.method, has_gain, gain, sampler{ s.history_current, s.history_count, s.history_head },
                                p.subsampling, hist, hcap, part, &last);
        sampler f = { s.frames_current, s.frames_count, s.frames_head };
        uint32_t frames_period = s.frames_period;
        if (p.period != frames_period)                                          // update_period(), :271
        {
            if (h.count > 0)                                                    // :275-279
            {
                if (t == 0)
                    hist[h.head] = h.current;
                h.head = (h.head + 1 == hcap) ? 0 : h.head + 1;
                h.count = 0;
            }
            else if (f.count > 0)                                               // :280-281
            {
                if (t == 0)
                    hist[h.head] = f.current;
                h.head = (h.head + 1 == hcap) ? 0 : h.head + 1;
            }
            // The history words that this launch has pushed -- by whichever lanes of the workgroup -- are read below by other
            // lanes.  They are plain global stores: a release fence at workgroup scope in every writer, the workgroup's barrier,
            // then an acquire fence at workgroup scope in every reader order them (the HIP memory model asks for no more between
            // threads of one workgroup; __syncthreads() carries both fences, the explicit one says so).
            __threadfence_block();
            __syncthreads();
            frames_period = p.period;                                           // :284
            const uint32_t subs = sm::subsamples(frames_period, p.frames, p.subsampling);
            // sBuffer.reset(), :291: the head at 0, the words stay; exactly `frames` pushes follow, into slots 0 .. frames - 1
            for (uint32_t k = t; k < p.frames; k += BLOCK)
                rg[k] = redecimated(hist, hcap, h.head, subs, k, p.method, frames_period, p.subsampling);
            f = sampler{ -1.0f, sm::leftover(frames_period, p.frames, p.subsampling), p.frames };      // frames < fcap
        }
        else
            f = run_sampler(xs, n, p.method, has_gain, gain, f, frames_period, rg, fcap, part, &last);
        if (t == 0)
            state[ch] = device_state{ h.current, h.count, h.head, f.current, f.count, f.head, frames_period };
    }

    // process(float sample) of every channel, :344-349, with update_period() as the reference counts it
    __global__ __launch_bounds__(BLOCK) void scaled_metergraph_value_kernel(const float *values, uint32_t channels, const params_t *params,
                                                                            device_state *state, float *history, float *ring,
                                                                            uint32_t max_subframes, uint32_t max_frames)
    {
        const uint32_t ch = blockIdx.x * BLOCK + threadIdx.x;
        if (ch >= channels)
            return;
        const params_t p = params[ch];
        if (p.period == 0 || p.frames == 0)                                     // as in scaled_metergraph_kernel
            return;
        device_state s = state[ch];
        float *hist = history + size_t(ch) * (size_t(max_subframes) + sm::FRAMES_GAP);
        float *rg = ring + size_t(ch) * (size_t(max_frames) + sm::FRAMES_GAP);
        const uint32_t hcap = p.subframes + sm::FRAMES_GAP, fcap = p.frames + sm::FRAMES_GAP;
        const float x = values[ch];
        float pushed;
        s.history_current = sm::fold_single(p.method, s.history_current, s.history_count, x, &pushed);
        if (++s.history_count >= p.subsampling)                                 // :140
        {
            hist[s.history_head] = pushed;
            s.history_head = (s.history_head + 1) % hcap;
            s.history_count = 0;
        }
        if (p.period != s.frames_period)                                        // update_period(), :269-342
        {
            if (s.history_count > 0)
            {
                hist[s.history_head] = s.history_current;
                s.history_head = (s.history_head + 1) % hcap;
                s.history_count = 0;
            }
            else if (s.frames_count > 0)
            {
                hist[s.history_head] = s.frames_current;
                s.history_head = (s.history_head + 1) % hcap;
            }
            s.frames_period = p.period;
            const uint32_t subs = sm::subsamples(s.frames_period, p.frames, p.subsampling);
            for (uint32_t k = 0; k < p.frames; ++k)                             // this lane's own stores above are in program order
                rg[k] = redecimated(hist, hcap, s.history_head, subs, k, p.method, s.frames_period, p.subsampling);
            s.frames_current = -1.0f;
            s.frames_count = sm::leftover(s.frames_period, p.frames, p.subsampling);
            s.frames_head = p.frames;
        }
        else
        {
            s.frames_current = sm::fold_single(p.method, s.frames_current, s.frames_count, x, &pushed);
            if (++s.frames_count >= s.frames_period)
            {
                rg[s.frames_head] = pushed;
                s.frames_head = (s.frames_head + 1) % fcap;
                s.frames_count = 0;
            }
        }
        state[ch] = s;
    }

    // read(dst, count), :365-369: the newest min(count, nFrames) frames, oldest first; nothing behind them
    __global__ __launch_bounds__(BLOCK) void scaled_metergraph_read_kernel(float *dst, size_t stride, uint32_t count, const params_t *params,
                                                                           const device_state *state, const float *ring, uint32_t max_frames)
    {
        const uint32_t ch = blockIdx.y, i = blockIdx.x * BLOCK + threadIdx.x;
        const params_t p = params[ch];
        const uint32_t take = (count < p.frames) ? count : p.frames;
        if (i >= take)
            return;
        const uint32_t fcap = p.frames + sm::FRAMES_GAP;
        const uint32_t tail = (state[ch].frames_head + fcap - take) % fcap;     // RawRingBuffer.cpp:136
        dst[size_t(ch) * stride + i] = ring[size_t(ch) * (size_t(max_frames) + sm::FRAMES_GAP) + (tail + i) % fcap];
    }

    // level(), :371-374: sFrames.sBuffer.read(1)
    __global__ __launch_bounds__(BLOCK) void scaled_metergraph_level_kernel(float *levels, uint32_t channels, const params_t *params,
                                                                            const device_state *state, const float *ring, uint32_t max_frames)
    {
        const uint32_t ch = blockIdx.x * BLOCK + threadIdx.x;
        if (ch >= channels)
            return;
        const uint32_t fcap = params[ch].frames + sm::FRAMES_GAP;
        levels[ch] = ring[size_t(ch) * (size_t(max_frames) + sm::FRAMES_GAP) + (state[ch].frames_head + fcap - 1) % fcap];
    }

    // what init() and fill() left.  fill(), :376-383: every word of both rings and both counts; heads and fCurrent stay.  init(),
    // :67-91: zeroed rings (OP_FILL with 0) and every state word 0
    __global__ __launch_bounds__(BLOCK) void scaled_metergraph_fill_kernel(const fill_op *ops, const params_t *params, device_state *state,
                                                                           float *history, float *ring, uint32_t max_subframes,
                                                                           uint32_t max_frames)
    {
        const uint32_t ch = blockIdx.x;
        const fill_op op = ops[ch];
        if (!(op.flags & OP_FILL))
            return;
        const uint32_t hcap = params[ch].subframes + sm::FRAMES_GAP, fcap = params[ch].frames + sm::FRAMES_GAP;
        for (uint32_t i = threadIdx.x; i < hcap; i += BLOCK)
            history[size_t(ch) * (size_t(max_subframes) + sm::FRAMES_GAP) + i] = op.value;
        for (uint32_t i = threadIdx.x; i < fcap; i += BLOCK)
            ring[size_t(ch) * (size_t(max_frames) + sm::FRAMES_GAP) + i] = op.value;
        if (threadIdx.x == 0)
        {
            if (op.flags & OP_RESET)
                state[ch] = device_state{ 0.0f, 0, 0, 0.0f, 0, 0, 0 };
            else
                state[ch].history_count = 0, state[ch].frames_count = 0;
        }
    }
} // namespace

struct mi_scaled_metergraph_bank : mi_bank::tables<params_t, device_state>
{
    static constexpr const char *NAME = "mi_scaled_metergraph_bank";

    uint32_t                max_frames = 0, max_subframes = 0;
    float                  *d_history = nullptr;    // [channels][max_subframes + FRAMES_GAP]
    float                  *d_ring = nullptr;       // [channels][max_frames + FRAMES_GAP]
    fill_op                *d_ops = nullptr;        // [channels]
    std::vector<fill_op>    ops;                    // pending init() / fill() of every channel
    bool                    work = false;           // ... of some channel
};

namespace
{
    typedef mi_scaled_metergraph_bank bank_t;

    int sg_destroy(bank_t *b)
    {
        if (b == nullptr)
            return MI_OK;
        (void)hipFree(b->d_history); (void)hipFree(b->d_ring); (void)hipFree(b->d_ops);
        return mi_bank::destroy(b);
    }

    // the changed settings, then the pending fills
    int sg_update(bank_t *b, hipStream_t st)
    {
        const int r = mi_bank::upload(*b, bank_t::NAME, st);
        if (r != MI_OK || !b->work)
            return r;
        const int k = mi::refuse_capture(bank_t::NAME, st);
        if (k != MI_OK)
            return k;
        MI_HIP_CHECK(hipMemcpyAsync(b->d_ops, b->ops.data(), size_t(b->channels) * sizeof(fill_op), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(scaled_metergraph_fill_kernel, dim3(b->channels), dim3(BLOCK), 0, st, b->d_ops, b->d_params, b->d_state,
                           b->d_history, b->d_ring, b->max_subframes, b->max_frames);
        MI_HIP_CHECK(hipGetLastError());
        MI_HIP_CHECK(hipStreamSynchronize(st));                 // the host's list may change again after this returns
        b->ops.assign(b->channels, fill_op{ 0, 0.0f });
        b->work = false;
        return MI_OK;
    }

    // update, and every channel has its rings; `period`: and a period to run at (with sFrames.nPeriod == 0 the reference's
    // process() never returns, :152)
    int sg_ready(bank_t *b, const char *entry, hipStream_t st)
    {
        const int r = sg_update(b, st);
        if (r != MI_OK)
            return r;
        for (uint32_t ch = 0; ch < b->channels; ++ch)
        {
            MI_REQUIRE(b->params[ch].frames != 0, MI_ESTATE, "%s: channel %u has no rings: call init() first", entry, ch);
            MI_REQUIRE(b->params[ch].period != 0, MI_ESTATE, "%s: channel %u has no period: call set_period() first", entry, ch);
        }
        return MI_OK;
    }

    int sg_channel(const bank_t *b, const char *entry, uint32_t channel)
    {
        MI_REQUIRE(b != nullptr, MI_ESTATE, "%s: NULL bank", entry);
        MI_REQUIRE(channel < b->channels, MI_EINVAL, "%s: channel %u out of range", entry, channel);
        return MI_OK;
    }

    void pend_fill(bank_t *b, uint32_t ch, uint32_t flags, float value)
    {
        b->ops[ch].flags |= flags;
        b->ops[ch].value = value;
        b->work = true;
    }

    size_t history_words(const bank_t *b)   { return size_t(b->max_subframes) + mi_scaled_metergraph::FRAMES_GAP; }
    size_t ring_words(const bank_t *b)      { return size_t(b->max_frames) + mi_scaled_metergraph::FRAMES_GAP; }
} // namespace

extern "C" {

int mi_scaled_metergraph_bank_create(mi_scaled_metergraph_bank_t **bank, uint32_t channels, uint32_t max_frames, uint32_t max_subframes)
{
    const char *entry = "mi_scaled_metergraph_bank_create";
    int r = mi_bank::open_checks(bank, entry, channels);
    if (r != MI_OK)
        return r;
    MI_REQUIRE(max_frames >= 1 && max_frames <= FRAMES_LIMIT, MI_EINVAL, "%s: max_frames must be 1 .. %u", entry, FRAMES_LIMIT);
    MI_REQUIRE(max_subframes >= max_frames && max_subframes <= SUBFRAMES_LIMIT, MI_EINVAL, "%s: max_subframes must be max_frames .. %u", entry,
               SUBFRAMES_LIMIT);
    r = mi_bank::open_new(bank, entry);
    if (r != MI_OK)
        return r;
    bank_t *b = *bank;
    b->channels = channels;
    b->max_frames = max_frames, b->max_subframes = max_subframes;
    b->ops.assign(channels, fill_op{ 0, 0.0f });
    r = mi_bank::alloc(*b, entry, params_t{ MI_MM_ABS_MAXIMUM, 0, 0, 0, 0, 0 }, device_state{ 0.0f, 0, 0, 0.0f, 0, 0, 0 });     // construct(), :42-59
    if (r == MI_OK)
    {
        const size_t hbytes = size_t(channels) * history_words(b) * sizeof(float), fbytes = size_t(channels) * ring_words(b) * sizeof(float);
        hipError_t e = hipMalloc(reinterpret_cast<void **>(&b->d_history), hbytes);
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&b->d_ring), fbytes);
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&b->d_ops), size_t(channels) * sizeof(fill_op));
        if (e == hipSuccess) e = hipMemset(b->d_history, 0, hbytes);
        if (e == hipSuccess) e = hipMemset(b->d_ring, 0, fbytes);
        if (e != hipSuccess)
            r = mi::fail(MI_EHIP, "%s: %s", entry, hipGetErrorString(e));
    }
    if (r != MI_OK)
    {
        *bank = nullptr;
        sg_destroy(b);
    }
    return r;
}

int mi_scaled_metergraph_bank_destroy(mi_scaled_metergraph_bank_t *b)
{
    return sg_destroy(b);
}

int mi_scaled_metergraph_bank_init(mi_scaled_metergraph_bank_t *b, uint32_t channel, size_t frames, size_t subsampling, size_t max_period)   // :67-91
{
    const char *entry = "mi_scaled_metergraph_bank_init";
    const int r = sg_channel(b, entry, channel);
    if (r != MI_OK)
        return r;
    // where the reference is undefined: a division by 0 (:70), no frames, a limit that inverts (:95) with a history read further
    // back than it is long (:289, :297)
    MI_REQUIRE(subsampling >= 1, MI_EINVAL, "%s: a subsampling of 0: the reference divides by it", entry);
    MI_REQUIRE(frames >= 1 && frames <= b->max_frames, MI_EINVAL, "%s: frames must be 1 .. %u (max_frames)", entry, b->max_frames);
    MI_REQUIRE(max_period >= subsampling, MI_EINVAL, "%s: max_period %zu below the subsampling %zu", entry, max_period, subsampling);
    MI_REQUIRE(max_period < COUNT_LIMIT && frames * max_period < COUNT_LIMIT, MI_EINVAL,
               "%s: frames * max_period must be below 2^31: the reference counts it in 32 bits (:288)", entry);
    const size_t subframes = (frames * max_period + subsampling - 1) / subsampling;                     // :69-70
    MI_REQUIRE(subframes <= b->max_subframes, MI_EINVAL, "%s: %zu sub-frames, the bank has room for %u (max_subframes)", entry, subframes,
               b->max_subframes);
    params_t &p = b->params[channel];
    p.period = 0, p.max_period = uint32_t(max_period), p.subsampling = uint32_t(subsampling), p.frames = uint32_t(frames);
    p.subframes = uint32_t(subframes);
    b->up.touch(channel);
    b->ops[channel].flags = 0;                                  // whatever was pending is overwritten
    pend_fill(b, channel, OP_FILL | OP_RESET, 0.0f);
    return MI_OK;
}

int mi_scaled_metergraph_bank_set_method(mi_scaled_metergraph_bank_t *b, uint32_t channel, uint32_t method)                 // :98-101
{
    const int r = sg_channel(b, "mi_scaled_metergraph_bank_set_method", channel);
    if (r != MI_OK)
        return r;
    if (b->params[channel].method != method)
        b->params[channel].method = method, b->up.touch(channel);
    return MI_OK;
}

int mi_scaled_metergraph_bank_set_period(mi_scaled_metergraph_bank_t *b, uint32_t channel, size_t period)                   // :93-96
{
    const char *entry = "mi_scaled_metergraph_bank_set_period";
    const int r = sg_channel(b, entry, channel);
    if (r != MI_OK)
        return r;
    params_t &p = b->params[channel];
    MI_REQUIRE(p.frames != 0, MI_ESTATE, "%s: channel %u has no rings: call init() first", entry, channel);
    const uint32_t target = mi_scaled_metergraph::limit_period(period, p.subsampling, p.max_period);
    if (p.period != target)
        p.period = target, b->up.touch(channel);
    return MI_OK;
}

int mi_scaled_metergraph_bank_fill(mi_scaled_metergraph_bank_t *b, uint32_t channel, float level)                           // :376-383
{
    const char *entry = "mi_scaled_metergraph_bank_fill";
    MI_REQUIRE(b != nullptr, MI_ESTATE, "%s: NULL bank", entry);
    MI_REQUIRE(channel < b->channels || channel == UINT32_MAX, MI_EINVAL, "%s: channel %u out of range", entry, channel);
    for (uint32_t ch = 0; ch < b->channels; ++ch)
        if ((channel == UINT32_MAX || ch == channel) && b->params[ch].frames != 0)      // without rings there is nothing to fill
            pend_fill(b, ch, OP_FILL, level);
    return MI_OK;
}

int mi_scaled_metergraph_bank_update_settings(mi_scaled_metergraph_bank_t *b, void *stream)
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_scaled_metergraph_bank_update_settings: NULL bank");
    return sg_update(b, mi::as_stream(stream));
}

int mi_scaled_metergraph_bank_get_params(const mi_scaled_metergraph_bank_t *b, uint32_t channel, mi_scaled_metergraph_params_t *params)
{
    return mi_bank::get_params(b, "mi_scaled_metergraph_bank_get_params", channel, params);
}

int mi_scaled_metergraph_bank_get_state(mi_scaled_metergraph_bank_t *b, uint32_t channel, mi_scaled_metergraph_state_t *state, float *history,
                                        float *ring, void *stream)
{
    int r = mi_bank::get_checks(b, "mi_scaled_metergraph_bank_get_state", channel, state);
    hipStream_t st = mi::as_stream(stream);
    if (r == MI_OK)
        r = mi::refuse_state_access(st);
    if (r == MI_OK)
        r = sg_update(b, st);
    if (r != MI_OK)
        return r;
    const params_t &p = b->params[channel];
    if (history != nullptr && p.frames != 0)
        MI_HIP_CHECK(hipMemcpyAsync(history, b->d_history + size_t(channel) * history_words(b),
                                    (size_t(p.subframes) + mi_scaled_metergraph::FRAMES_GAP) * sizeof(float), hipMemcpyDeviceToHost, st));
    if (ring != nullptr && p.frames != 0)
        MI_HIP_CHECK(hipMemcpyAsync(ring, b->d_ring + size_t(channel) * ring_words(b),
                                    (size_t(p.frames) + mi_scaled_metergraph::FRAMES_GAP) * sizeof(float), hipMemcpyDeviceToHost, st));
    return mi::read_state(state, b->d_state + channel, st);    // synchronises
}

int mi_scaled_metergraph_bank_set_state(mi_scaled_metergraph_bank_t *b, uint32_t channel, const mi_scaled_metergraph_state_t *state,
                                        const float *history, const float *ring, void *stream)
{
    const char *entry = "mi_scaled_metergraph_bank_set_state";
    int r = sg_channel(b, entry, channel);
    if (r != MI_OK)
        return r;
    MI_REQUIRE(state != nullptr, MI_EINVAL, "%s: NULL state", entry);
    hipStream_t st = mi::as_stream(stream);
    r = mi::refuse_state_access(st);
    if (r == MI_OK)
        r = sg_update(b, st);                                   // an init() or a fill() before this call does not undo it
    if (r != MI_OK)
        return r;
    const params_t &p = b->params[channel];
    MI_REQUIRE(p.frames != 0, MI_ESTATE, "%s: channel %u has no rings: call init() first", entry, channel);
    const uint32_t hcap = p.subframes + mi_scaled_metergraph::FRAMES_GAP, fcap = p.frames + mi_scaled_metergraph::FRAMES_GAP;
    MI_REQUIRE(state->history_head < hcap && state->frames_head < fcap, MI_EINVAL, "%s: heads %u, %u outside the rings of %u and %u words", entry,
               state->history_head, state->frames_head, hcap, fcap);
    // what the samplers keep (scaled_metergraph_bank.h): nCount below the period; sFrames.nPeriod is 0 or a period set_period() can give
    MI_REQUIRE(state->history_count < p.subsampling, MI_EINVAL, "%s: sHistory.nCount %u not below the subsampling %u", entry, state->history_count,
               p.subsampling);
    MI_REQUIRE(state->frames_period == 0 || (state->frames_period >= p.subsampling && state->frames_period <= p.max_period), MI_EINVAL,
               "%s: sFrames.nPeriod %u is neither 0 nor in %u .. %u", entry, state->frames_period, p.subsampling, p.max_period);
    MI_REQUIRE(state->frames_count < ((state->frames_period != 0) ? state->frames_period : p.max_period), MI_EINVAL,
               "%s: sFrames.nCount %u not below its period", entry, state->frames_count);
    if (history != nullptr)
        MI_HIP_CHECK(hipMemcpyAsync(b->d_history + size_t(channel) * history_words(b), history, size_t(hcap) * sizeof(float), hipMemcpyHostToDevice, st));
    if (ring != nullptr)
        MI_HIP_CHECK(hipMemcpyAsync(b->d_ring + size_t(channel) * ring_words(b), ring, size_t(fcap) * sizeof(float), hipMemcpyHostToDevice, st));
    return mi::write_state(b->d_state + channel, *state, st);
}

int mi_scaled_metergraph_bank_process(mi_scaled_metergraph_bank_t *b, const float *src, const float *gains, size_t count, size_t stride,
                                      void *stream)                                                      // :351-363
{
    const char *entry = "mi_scaled_metergraph_bank_process";
    MI_REQUIRE(b != nullptr, MI_ESTATE, "%s: NULL bank", entry);
    hipStream_t st = mi::as_stream(stream);
    const int r = sg_ready(b, entry, st);
    if (r != MI_OK || count == 0)
        return r;
    const int k = mi_bank::check_rows(entry, b->channels, count, COUNT_LIMIT, { { src, stride, count, mi_bank::REQUIRED } });
    if (k != MI_OK)
        return k;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    mi::take_profile_events(&ev0, &ev1);
    MI_LAUNCH(scaled_metergraph_kernel, dim3(b->channels), dim3(BLOCK), 0, st, ev0, ev1, src, gains, stride, uint32_t(count), b->d_params,
              b->d_state, b->d_history, b->d_ring, b->max_subframes, b->max_frames);
    MI_HIP_CHECK(hipGetLastError());
    return MI_OK;
}

int mi_scaled_metergraph_bank_process_value(mi_scaled_metergraph_bank_t *b, const float *values, void *stream)              // :344-349
{
    const char *entry = "mi_scaled_metergraph_bank_process_value";
    MI_REQUIRE(b != nullptr, MI_ESTATE, "%s: NULL bank", entry);
    MI_REQUIRE(values != nullptr, MI_EINVAL, "%s: NULL buffer", entry);
    hipStream_t st = mi::as_stream(stream);
    const int r = sg_ready(b, entry, st);
    if (r != MI_OK)
        return r;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    mi::take_profile_events(&ev0, &ev1);
    MI_LAUNCH(scaled_metergraph_value_kernel, dim3((b->channels + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, st, ev0, ev1, values, b->channels,
              b->d_params, b->d_state, b->d_history, b->d_ring, b->max_subframes, b->max_frames);
    MI_HIP_CHECK(hipGetLastError());
    return MI_OK;
}

int mi_scaled_metergraph_bank_read(mi_scaled_metergraph_bank_t *b, float *dst, size_t count, size_t stride, void *stream)   // :365-369
{
    const char *entry = "mi_scaled_metergraph_bank_read";
    MI_REQUIRE(b != nullptr, MI_ESTATE, "%s: NULL bank", entry);
    hipStream_t st = mi::as_stream(stream);
    const int r = sg_ready(b, entry, st);
    if (r != MI_OK || count == 0)
        return r;
    const int k = mi_bank::check_rows(entry, b->channels, count, COUNT_LIMIT, { { dst, stride, count, mi_bank::REQUIRED } });
    if (k != MI_OK)
        return k;
    const size_t most = (count < b->max_frames) ? count : b->max_frames;       // no channel has more frames to give
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    mi::take_profile_events(&ev0, &ev1);
    MI_LAUNCH(scaled_metergraph_read_kernel, dim3(uint32_t((most + BLOCK - 1) / BLOCK), b->channels), dim3(BLOCK), 0, st, ev0, ev1, dst, stride,
              uint32_t(most), b->d_params, b->d_state, b->d_ring, b->max_frames);
    MI_HIP_CHECK(hipGetLastError());
    return MI_OK;
}

int mi_scaled_metergraph_bank_level(mi_scaled_metergraph_bank_t *b, float *levels, void *stream)                            // :371-374
{
    const char *entry = "mi_scaled_metergraph_bank_level";
    MI_REQUIRE(b != nullptr, MI_ESTATE, "%s: NULL bank", entry);
    MI_REQUIRE(levels != nullptr, MI_EINVAL, "%s: NULL buffer", entry);
    hipStream_t st = mi::as_stream(stream);
    const int r = sg_ready(b, entry, st);
    if (r != MI_OK)
        return r;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    mi::take_profile_events(&ev0, &ev1);
    MI_LAUNCH(scaled_metergraph_level_kernel, dim3((b->channels + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, st, ev0, ev1, levels, b->channels,
              b->d_params, b->d_state, b->d_ring, b->max_frames);
    MI_HIP_CHECK(hipGetLastError());
    return MI_OK;
}

} // extern "C"
