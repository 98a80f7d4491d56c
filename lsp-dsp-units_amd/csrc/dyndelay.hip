// mi_dyndelay_bank -- `channels` x lsp::dspu::DynamicDelay (reference: src/main/util/DynamicDelay.cpp:65-148): a delay line whose
// delay, feedback gain and feedback delay come per sample from three rows.  Per sample, in this order (:101-116):
//     shift = clamp(ssize_t(delay[i]), 0, nMaxDelay)          tail = nHead - shift (+ nCapacity)
//     feed  = size_t(float(tail) + clamp(fdelay[i], 0.0f, float(shift)))  (- nCapacity)      -- a float32 sum, then truncated
//     vDelay[nHead] = in[i];  s = vDelay[tail];  vDelay[feed] += s * fgain[i];  out[i] = vDelay[tail];  ++nHead (wrap)
// The recurrence runs through the ring at addresses that depend on the delay rows and the position only, never on the audio.
//
// A workgroup of BLOCK threads owns one channel and takes its rows in tiles of at most TILE = 0x400 samples:
//     index    every thread loads its four samples of the four rows and forms shift / tail / feed; the tile's largest shift is
//              reduced.  All of a tile's inputs are in registers before anything of the tile is stored: out may be any input row.
//     place    the ring is at least nMaxDelay + 0x402 long, so a head of this tile is no tail and no feed of an earlier step of
//              it: the tile's inputs go to their head positions at once.  If [h0 - largest shift, h0 + tile) fits WINDOW floats
//              it is staged in LDS, worked on there and written back; otherwise the steps work on the ring in global memory.
//     runs     the tile is cut into runs.  A run whose feed positions are pairwise distinct and in which no step's tail is
//              another step's feed touches, step by step, cells no other step of it touches: its steps execute one per lane,
//              without a barrier between them.  The test is a pair of tag arrays in LDS indexed by position modulo TAGS (the
//              lowest lane that feeds / reads a slot); a lane is "bad" if a lower lane's feed shares its feed's or its tail's
//              slot, or a lower lane's tail shares its feed's slot; the run ends in front of the lowest bad lane.  A collision
//              of two positions in a slot only shortens a run (conservative, never optimistic).
//     serial   where a run would be shorter than MIN_RUN, lane 0 walks the next steps (16, and twice as many after every look
//              that found no run, up to 128) as the reference's loop does, relying on program order to its own addresses, before
//              the next look.  This path is correct alone (MI_DSPU_TEST_PATH=dyndelay_serial takes it
//              for every step; dyndelay_parallel never takes it).
// out[i] is the cell at tail AFTER the feedback was added: s + s * g where feed == tail, s otherwise -- no other step of a run
// writes that cell -- so the re-read of the reference is a select here.  The product and the sum round separately.
//
// Above 2^24 the float32 sum of the feed index may round UP, past the head.  Such a step ("ahead") could feed a cell that a
// later input of the tile overwrites, so a tile that has one is walked by lane 0 on the ring with the inputs placed step by
// step: the reference's loop as it stands.  Capacities above 2^24 floats are refused at create, so tail itself is exact.
//
// Where the reference has no defined behaviour the bank defines it: delay converts with saturation and NaN as 0 (what
// v_cvt_i32_f32 does), a NaN fdelay counts as 0.  in and fgain may be anything and follow IEEE bit for bit.
#include "bank_core.h"

#include <vector>

#pragma clang fp contract(off)

namespace
{
    constexpr int      BLOCK = 256;
    constexpr uint32_t TILE = 0x400;                    // DynamicDelay.cpp:30; the ring's slack is built from it (:68)
    constexpr uint32_t PER = TILE / BLOCK;              // samples of a tile per thread
    constexpr uint32_t WINDOW = 5120;                   // floats of the ring a workgroup stages in LDS: shifts up to 4096
    // Slots of each tag array (a power of two).  A run's feeds and a run's tails are each within some 256 cells of one another
    // where the rows are smooth, so the two stretches share slots only where the delay is within 256 of a multiple of TAGS.
    constexpr uint32_t TAGS = 2048;
    constexpr uint32_t MIN_RUN = 8;                     // a parallel run costs about as much as five steps of lane 0's walk
    // steps lane 0 walks before the next look for a parallel run: WALK_MIN after a parallel run, twice as many after every look
    // that found none, WALK_MAX at the most -- rows that never run in parallel pay for a look every 128 steps
    constexpr uint32_t WALK_MIN = 16, WALK_MAX = 128;
    constexpr uint32_t NONE = 0xffffffffu;
    constexpr size_t   COUNT_LIMIT = size_t(1) << 31;   // the kernel counts samples in 32 bits
    constexpr size_t   CAPACITY_LIMIT = size_t(1) << 24;
    enum { PATH_AUTO, PATH_SERIAL, PATH_PARALLEL };

    struct device_state { uint32_t head; };

    __device__ __forceinline__ uint32_t wave_max(uint32_t v)
    {
        #pragma unroll
        for (int d = 32; d > 0; d >>= 1)
        {
            const uint32_t o = __shfl_xor(v, d);
            v = (o > v) ? o : v;
        }
        return v;
    }

    // one step on cells t and f of R (the window or the ring): the value out[i] takes
    __device__ __forceinline__ float step(float *R, uint32_t t, uint32_t f, float g)
    {
        const float s = R[t];
        const float v = R[f] + s * g;
        R[f] = v;
        return (f == t) ? v : s;
    }

    // steps [a, b) on lane 0, in order.  place: the inputs are not at their heads yet (io[k] is in[k]; positions are the ring's)
    __device__ __forceinline__ void walk(float *R, const uint32_t *tail, const uint32_t *feed, const float *gain, float *io,
                                         uint32_t a, uint32_t b, bool place, uint32_t h0, uint32_t cap)
    {
        for (uint32_t k = a; k < b; ++k)
        {
            if (place)
            {
                const uint32_t h = h0 + k;
                R[(h >= cap) ? h - cap : h] = io[k];
            }
            io[k] = step(R, tail[k], feed[k], gain[k]);
        }
    }

    // The runs of a tile of n steps whose inputs are placed.  R: the window in LDS or the ring; positions as stored in tail / feed.
    // Returns the number of steps that ran one per lane.
    __device__ __forceinline__ uint32_t runs(float *R, const uint32_t *tail, const uint32_t *feed, const float *gain, float *io,
                                             uint32_t *feed_tag, uint32_t *tail_tag, uint32_t *run_len, uint32_t n, int path)
    {
        const uint32_t tid = threadIdx.x;
        uint32_t parallel = 0;
        if (path == PATH_SERIAL)
        {
            if (tid == 0)
                walk(R, tail, feed, gain, io, 0, n, false, 0, 0);
            __syncthreads();
            return 0;
        }
        uint32_t stride = WALK_MIN;
        for (uint32_t a = 0; a < n; )
        {
            const uint32_t m = (n - a < uint32_t(BLOCK)) ? n - a : uint32_t(BLOCK);
            const bool mine = tid < m;
            const uint32_t t = mine ? tail[a + tid] : 0, f = mine ? feed[a + tid] : 0;
            const uint32_t ts = t & (TAGS - 1), fs = f & (TAGS - 1);
            if (mine)
            {
                atomicMin(&feed_tag[fs], tid);
                atomicMin(&tail_tag[ts], tid);
            }
            if (tid == 0)
                *run_len = m;
            __syncthreads();
            if (mine && (feed_tag[fs] < tid || feed_tag[ts] < tid || tail_tag[fs] < tid))
                atomicMin(run_len, tid);
            __syncthreads();
            const uint32_t len = *run_len;                          // >= 1: lane 0 has no lower lane
            if (mine)
                feed_tag[fs] = NONE, tail_tag[ts] = NONE;
            if (len >= MIN_RUN || len == m || path == PATH_PARALLEL)
            {
                if (tid < len)
                    io[a + tid] = step(R, t, f, gain[a + tid]);
                parallel += len;
                a += len;
                stride = WALK_MIN;
            }
            else
            {
                const uint32_t b = (n - a < stride) ? n : a + stride;
                if (tid == 0)
                    walk(R, tail, feed, gain, io, a, b, false, 0, 0);
                a = b;
                stride = (2 * stride < WALK_MAX) ? 2 * stride : WALK_MAX;
            }
            __syncthreads();                                        // the run's cells, the tags and run_len are settled
        }
        return parallel;
    }

    __global__ __launch_bounds__(BLOCK) void dyndelay_kernel(float *out, const float *in, const float *delay, const float *fgain,
                                                             const float *fdelay, size_t out_stride, size_t in_stride,
                                                             size_t delay_stride, size_t fgain_stride, size_t fdelay_stride,
                                                             uint32_t count, float *rings, device_state *state, uint32_t cap,
                                                             uint32_t max_delay, int path, unsigned long long *counters)
    {
        __shared__ float    win[WINDOW];
        __shared__ uint32_t s_tail[TILE], s_feed[TILE];
        __shared__ float    s_gain[TILE], s_io[TILE];
        __shared__ uint32_t feed_tag[TAGS], tail_tag[TAGS];
        __shared__ uint32_t s_max, s_ahead, run_len;

        const uint32_t tid = threadIdx.x, ch = blockIdx.x;
        float *ring = rings + size_t(ch) * cap;
        const float *x = in + size_t(ch) * in_stride, *dl = delay + size_t(ch) * delay_stride;
        const float *fg = fgain + size_t(ch) * fgain_stride, *fd = fdelay + size_t(ch) * fdelay_stride;
        float *y = out + size_t(ch) * out_stride;
        uint32_t h0 = __builtin_amdgcn_readfirstlane(state[ch].head);
        const float max_f = float(max_delay);                       // exact: max_delay < 2^24
        uint32_t parallel = 0;

        for (uint32_t k = tid; k < TAGS; k += BLOCK)
            feed_tag[k] = NONE, tail_tag[k] = NONE;

        for (uint32_t pos = 0; pos < count; pos += TILE)
        {
            const uint32_t n = (count - pos < TILE) ? count - pos : TILE;
            if (tid == 0)
                s_max = 0, s_ahead = 0;
            __syncthreads();                                        // and the previous tile's arrays are free

            // index: this thread's samples tid, tid + BLOCK, ..
            uint32_t tl[PER], fe[PER], hd[PER], top = 0;
            float g[PER], v[PER];
            bool ahead = false;
            #pragma unroll
            for (uint32_t q = 0; q < PER; ++q)
            {
                const uint32_t j = tid + q * BLOCK;
                tl[q] = fe[q] = hd[q] = 0, g[q] = v[q] = 0.0f;
                if (j < n)
                {
                    const float d = dl[pos + j], b = fd[pos + j];
                    g[q] = fg[pos + j], v[q] = x[pos + j];
                    // ssize_t(delay) limited to [0, nMaxDelay]; NaN and what is below 1 give 0, what is beyond the range nMaxDelay
                    const uint32_t shift = !(d > 0.0f) ? 0 : (d >= max_f) ? max_delay : uint32_t(int32_t(d));
                    const uint32_t h = (h0 + j >= cap) ? h0 + j - cap : h0 + j;
                    const uint32_t t = (h >= shift) ? h - shift : h + cap - shift;
                    const float lim = float(shift);
                    const float back = (b < 0.0f) ? 0.0f : (b > lim) ? lim : (b != b) ? 0.0f : b;       // lsp_limit; NaN: 0
                    uint32_t f = uint32_t(float(t) + back);         // the float32 sum, truncated
                    f = (f >= cap) ? f - cap : f;
                    const uint32_t behind = (h >= f) ? h - f : h + cap - f;
                    ahead = ahead || behind > shift;
                    top = (shift > top) ? shift : top;
                    tl[q] = t, fe[q] = f, hd[q] = h;
                }
            }
            top = wave_max(top);
            if ((tid & 63) == 0)
                atomicMax(&s_max, top);
            if (ahead)
                s_ahead = 1;
            __syncthreads();
            const uint32_t reach = s_max;
            const bool plain = s_ahead != 0;                        // the reference's loop as it stands, on the ring
            const bool staged = !plain && reach + n <= WINDOW;
            const uint32_t base = (h0 >= reach) ? h0 - reach : h0 + cap - reach;   // the window's first cell

            #pragma unroll
            for (uint32_t q = 0; q < PER; ++q)
            {
                const uint32_t j = tid + q * BLOCK;
                if (j < n)
                {
                    // staged: positions relative to the window's first cell (below reach + n <= WINDOW)
                    s_tail[j] = !staged ? tl[q] : (tl[q] >= base) ? tl[q] - base : tl[q] + cap - base;
                    s_feed[j] = !staged ? fe[q] : (fe[q] >= base) ? fe[q] - base : fe[q] + cap - base;
                    s_gain[j] = g[q];
                    s_io[j] = v[q];
                    if (staged)
                        win[reach + j] = v[q];
                    else if (!plain)
                        ring[hd[q]] = v[q];
                }
            }
            if (staged)
                for (uint32_t k = tid; k < reach; k += BLOCK)
                    win[k] = ring[(base + k >= cap) ? base + k - cap : base + k];
            __syncthreads();

            if (plain)
            {
                if (tid == 0)
                    walk(ring, s_tail, s_feed, s_gain, s_io, 0, n, true, h0, cap);
                __syncthreads();
            }
            else if (staged)
                parallel += runs(win, s_tail, s_feed, s_gain, s_io, feed_tag, tail_tag, &run_len, n, path);
            else
                parallel += runs(ring, s_tail, s_feed, s_gain, s_io, feed_tag, tail_tag, &run_len, n, path);

            if (staged)
                for (uint32_t k = tid; k < reach + n; k += BLOCK)
                    ring[(base + k >= cap) ? base + k - cap : base + k] = win[k];
            for (uint32_t j = tid; j < n; j += BLOCK)
                y[pos + j] = s_io[j];
            h0 = (h0 + n >= cap) ? h0 + n - cap : h0 + n;
        }
        if (tid == 0)
        {
            state[ch].head = h0;
            if (counters != nullptr)
            {
                atomicAdd(&counters[0], (unsigned long long)parallel);
                atomicAdd(&counters[1], (unsigned long long)count);
            }
        }
    }

    // DynamicDelay::copy (DynamicDelay.cpp:124-148): the newest min(capacities) samples of the source line to the end of the
    // destination line, zeros in front of them, the destination's head to 0.  The two lines are different lines.
    __global__ __launch_bounds__(BLOCK) void dyndelay_copy_kernel(float *dst, uint32_t dst_cap, device_state *dst_state, const float *src,
                                                                  uint32_t src_cap, const device_state *src_state)
    {
        const uint32_t count = (dst_cap < src_cap) ? dst_cap : src_cap;
        const uint32_t dt = dst_cap - count;
        const uint32_t sh = src_state->head;
        const uint32_t st = (sh >= count) ? sh - count : sh + src_cap - count;
        for (uint32_t i = blockIdx.x * BLOCK + threadIdx.x; i < dst_cap; i += gridDim.x * BLOCK)
        {
            const uint32_t k = st + (i - dt);                       // used where i >= dt: < 2 * src_cap
            dst[i] = (i < dt) ? 0.0f : src[(k >= src_cap) ? k - src_cap : k];
        }
        if (blockIdx.x == 0 && threadIdx.x == 0)
            dst_state->head = 0;
    }
} // namespace

struct mi_dyndelay_bank
{
    uint32_t            channels = 0, max_delay = 0, capacity = 0;
    float              *d_ring = nullptr;           // [channels][capacity]
    device_state       *d_state = nullptr;          // [channels]
    unsigned long long *d_counters = nullptr;       // steps one per lane, steps in all: the kernel is handed them while counting
    bool                counting = false;
};

namespace
{
    int line_checks(const mi_dyndelay_bank *b, const char *entry, uint32_t channel, const void *host, size_t offset, size_t count)
    {
        MI_REQUIRE(b != nullptr, MI_ESTATE, "%s: NULL bank", entry);
        MI_REQUIRE(channel < b->channels, MI_EINVAL, "%s: channel %u out of range", entry, channel);
        MI_REQUIRE(count == 0 || host != nullptr, MI_EINVAL, "%s: NULL buffer", entry);
        MI_REQUIRE(offset <= b->capacity && count <= b->capacity - offset, MI_EINVAL, "%s: %zu floats at %zu do not fit the line's %u", entry,
                   count, offset, b->capacity);
        return MI_OK;
    }
} // namespace

extern "C" {

int mi_dyndelay_bank_create(mi_dyndelay_bank_t **bank, uint32_t channels, size_t max_size)
{
    int r = mi_bank::open_checks(bank, "mi_dyndelay_bank_create", channels);
    if (r != MI_OK)
        return r;
    MI_REQUIRE(max_size < CAPACITY_LIMIT, MI_EINVAL, "mi_dyndelay_bank_create: a line for %zu samples is longer than 2^24 floats", max_size);
    const size_t d = max_size + 1, capacity = d - d % TILE + 2 * TILE;          // DynamicDelay.cpp:67-68
    MI_REQUIRE(capacity <= CAPACITY_LIMIT, MI_EINVAL, "mi_dyndelay_bank_create: a line of %zu floats is longer than 2^24", capacity);
    r = mi_bank::open_new(bank, "mi_dyndelay_bank_create");
    if (r != MI_OK)
        return r;
    mi_dyndelay_bank *b = *bank;
    b->channels = channels, b->max_delay = uint32_t(max_size), b->capacity = uint32_t(capacity);
    const size_t bytes = size_t(channels) * capacity * sizeof(float);
    hipError_t e = hipMalloc(reinterpret_cast<void **>(&b->d_ring), bytes);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&b->d_state), channels * sizeof(device_state));
    if (e == hipSuccess) e = hipMemset(b->d_ring, 0, bytes);
    if (e == hipSuccess) e = hipMemset(b->d_state, 0, channels * sizeof(device_state));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&b->d_counters), 2 * sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMemset(b->d_counters, 0, 2 * sizeof(unsigned long long));
    if (e == hipSuccess)
        return MI_OK;
    *bank = nullptr;
    mi_dyndelay_bank_destroy(b);
    return mi::fail(e == hipErrorOutOfMemory ? MI_ENOMEM : MI_EHIP, "mi_dyndelay_bank_create: %s", hipGetErrorString(e));
}

int mi_dyndelay_bank_destroy(mi_dyndelay_bank_t *b)
{
    if (b == nullptr)
        return MI_OK;
    (void)hipFree(b->d_ring); (void)hipFree(b->d_state); (void)hipFree(b->d_counters);
    delete b;
    return MI_OK;
}

int mi_dyndelay_bank_get(const mi_dyndelay_bank_t *b, uint32_t channel, uint32_t *max_delay, uint32_t *capacity, uint32_t *head)
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_dyndelay_bank_get: NULL bank");
    MI_REQUIRE(channel < b->channels, MI_EINVAL, "mi_dyndelay_bank_get: channel %u out of range", channel);
    if (max_delay) *max_delay = b->max_delay;
    if (capacity)  *capacity = b->capacity;
    if (head)
    {
        device_state s;
        const int r = mi::read_state(&s, b->d_state + channel, nullptr);
        if (r != MI_OK)
            return r;
        *head = s.head;
    }
    return MI_OK;
}

int mi_dyndelay_bank_get_state(mi_dyndelay_bank_t *b, uint32_t channel, mi_dyndelay_state_t *state, void *stream)
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_dyndelay_bank_get_state: NULL bank");
    MI_REQUIRE(state != nullptr, MI_EINVAL, "mi_dyndelay_bank_get_state: NULL state");
    device_state s;
    const int r = mi_bank::get_state(b, "mi_dyndelay_bank_get_state", channel, &s, stream);
    if (r == MI_OK)
        state->head = s.head;
    return r;
}

int mi_dyndelay_bank_set_state(mi_dyndelay_bank_t *b, uint32_t channel, const mi_dyndelay_state_t *state, void *stream)
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_dyndelay_bank_set_state: NULL bank");
    MI_REQUIRE(state != nullptr, MI_EINVAL, "mi_dyndelay_bank_set_state: NULL state");
    MI_REQUIRE(channel < b->channels, MI_EINVAL, "mi_dyndelay_bank_set_state: channel %u out of range", channel);
    MI_REQUIRE(state->head < b->capacity, MI_EINVAL, "mi_dyndelay_bank_set_state: head %u outside the line's %u floats", state->head, b->capacity);
    return mi::write_state(b->d_state + channel, device_state{ state->head }, mi::as_stream(stream));
}

int mi_dyndelay_bank_clear(mi_dyndelay_bank_t *b, void *stream)                                              // :91-95
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_dyndelay_bank_clear: NULL bank");
    MI_HIP_CHECK(hipMemsetAsync(b->d_ring, 0, size_t(b->channels) * b->capacity * sizeof(float), mi::as_stream(stream)));
    MI_HIP_CHECK(hipMemsetAsync(b->d_state, 0, b->channels * sizeof(device_state), mi::as_stream(stream)));
    return MI_OK;
}

int mi_dyndelay_bank_process(mi_dyndelay_bank_t *b, float *out, const float *in, const float *delay, const float *fgain,
                             const float *fdelay, size_t count, size_t out_stride, size_t in_stride, size_t delay_stride,
                             size_t fgain_stride, size_t fdelay_stride, void *stream)                        // :97-118
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_dyndelay_bank_process: NULL bank");
    if (count == 0)
        return MI_OK;
    const uint32_t in_row = mi_bank::REQUIRED;
    const int r = mi_bank::check_rows("mi_dyndelay_bank_process", b->channels, count, COUNT_LIMIT,
                                      { { out, out_stride, count, mi_bank::REQUIRED | mi_bank::OUTPUT }, { in, in_stride, count, in_row },
                                        { delay, delay_stride, count, in_row }, { fgain, fgain_stride, count, in_row },
                                        { fdelay, fdelay_stride, count, in_row } });
    if (r != MI_OK)
        return r;
    const int path = mi::test_path("dyndelay_serial") ? PATH_SERIAL : mi::test_path("dyndelay_parallel") ? PATH_PARALLEL : PATH_AUTO;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    mi::take_profile_events(&ev0, &ev1);
    MI_LAUNCH(dyndelay_kernel, dim3(b->channels), dim3(BLOCK), 0, mi::as_stream(stream), ev0, ev1, out, in, delay, fgain, fdelay,
              out_stride, in_stride, delay_stride, fgain_stride, fdelay_stride, uint32_t(count), b->d_ring, b->d_state, b->capacity,
              b->max_delay, path, b->counting ? b->d_counters : nullptr);
    MI_HIP_CHECK(hipGetLastError());
    return MI_OK;
}

int mi_dyndelay_bank_copy(mi_dyndelay_bank_t *dst, uint32_t dst_channel, mi_dyndelay_bank_t *src, uint32_t src_channel, void *stream)   // :124-148
{
    MI_REQUIRE(dst != nullptr && src != nullptr, MI_ESTATE, "mi_dyndelay_bank_copy: NULL bank");
    MI_REQUIRE(dst_channel < dst->channels, MI_EINVAL, "mi_dyndelay_bank_copy: channel %u out of range", dst_channel);
    MI_REQUIRE(src_channel < src->channels, MI_EINVAL, "mi_dyndelay_bank_copy: source channel %u out of range", src_channel);
    MI_REQUIRE(dst != src || dst_channel != src_channel, MI_EINVAL, "mi_dyndelay_bank_copy: a line cannot be copied onto itself");
    const uint32_t blocks = (dst->capacity + BLOCK - 1) / BLOCK;
    hipLaunchKernelGGL(dyndelay_copy_kernel, dim3(blocks > 256 ? 256 : blocks), dim3(BLOCK), 0, mi::as_stream(stream),
                       dst->d_ring + size_t(dst_channel) * dst->capacity, dst->capacity, dst->d_state + dst_channel,
                       src->d_ring + size_t(src_channel) * src->capacity, src->capacity, src->d_state + src_channel);
    MI_HIP_CHECK(hipGetLastError());
    return MI_OK;
}

int mi_dyndelay_bank_read_line(mi_dyndelay_bank_t *b, uint32_t channel, float *host, size_t offset, size_t count, void *stream)
{
    int r = line_checks(b, "mi_dyndelay_bank_read_line", channel, host, offset, count);
    if (r == MI_OK)
        r = mi::refuse_state_access(mi::as_stream(stream));
    if (r != MI_OK || count == 0)
        return r;
    MI_HIP_CHECK(hipMemcpyAsync(host, b->d_ring + size_t(channel) * b->capacity + offset, count * sizeof(float), hipMemcpyDeviceToHost,
                                mi::as_stream(stream)));
    MI_HIP_CHECK(hipStreamSynchronize(mi::as_stream(stream)));
    return MI_OK;
}

int mi_dyndelay_bank_write_line(mi_dyndelay_bank_t *b, uint32_t channel, const float *host, size_t offset, size_t count, void *stream)
{
    int r = line_checks(b, "mi_dyndelay_bank_write_line", channel, host, offset, count);
    if (r == MI_OK)
        r = mi::refuse_state_access(mi::as_stream(stream));
    if (r != MI_OK || count == 0)
        return r;
    MI_HIP_CHECK(hipMemcpyAsync(b->d_ring + size_t(channel) * b->capacity + offset, host, count * sizeof(float), hipMemcpyHostToDevice,
                                mi::as_stream(stream)));
    MI_HIP_CHECK(hipStreamSynchronize(mi::as_stream(stream)));
    return MI_OK;
}

int mi_dyndelay_bank_count_steps(mi_dyndelay_bank_t *b, int on, void *stream)
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_dyndelay_bank_count_steps: NULL bank");
    hipStream_t st = mi::as_stream(stream);
    const int r = mi::refuse_state_access(st);
    if (r != MI_OK)
        return r;
    // The counters live as long as the bank: a launch in flight or in a captured graph keeps a valid address (a graph captured
    // while counting goes on counting).  Switching on zeroes them behind what the stream holds.
    b->counting = on != 0;
    if (!b->counting)
        return MI_OK;
    MI_HIP_CHECK(hipMemsetAsync(b->d_counters, 0, 2 * sizeof(unsigned long long), st));
    MI_HIP_CHECK(hipStreamSynchronize(st));
    return MI_OK;
}

int mi_dyndelay_bank_steps(mi_dyndelay_bank_t *b, uint64_t *parallel, uint64_t *total, void *stream)
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_dyndelay_bank_steps: NULL bank");
    MI_REQUIRE(parallel != nullptr && total != nullptr, MI_EINVAL, "mi_dyndelay_bank_steps: NULL result pointer");
    MI_REQUIRE(b->counting, MI_ESTATE, "mi_dyndelay_bank_steps: the bank is not counting (mi_dyndelay_bank_count_steps)");
    unsigned long long c[2] = { 0, 0 };
    hipStream_t st = mi::as_stream(stream);
    const int r = mi::refuse_state_access(st);
    if (r != MI_OK)
        return r;
    MI_HIP_CHECK(hipMemcpyAsync(c, b->d_counters, sizeof(c), hipMemcpyDeviceToHost, st));
    MI_HIP_CHECK(hipStreamSynchronize(st));
    *parallel = c[0], *total = c[1];
    return MI_OK;
}

} // extern "C"
