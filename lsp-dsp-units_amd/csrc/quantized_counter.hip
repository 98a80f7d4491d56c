// lsp::dspu::QuantizedCounter as a bank of `channels` counters (src/main/stat/QuantizedCounter.cpp): the histogram of the last
// nPeriod samples of a row over nLevels quantisation levels, with one counter for what lies below the range and one for above.
// History ring, counters, nHead and nCount of every channel live on the device.
//
// qcounter_kernel: a workgroup per channel, one launch per process().  The result is a vector of integers, so the order of the
// increments does not matter and every sample is independent.  A call is a closed form of nHead, nCount, nPeriod, nCapacity and
// count (quantized_counter_bank.h):
//     the history samples that leave    read from the ring before the row overwrites them, -1 each
//     the row's suffix that stays       the last min(count, nPeriod) samples, +1 each
// Both are spans of floats read 16 bytes per lane on the 16-byte grid whatever their base.  A lane folds the equal bins of its
// four consecutive samples into one add; a wave whose lanes all hold one and the same bin (silence, DC, a clipped row) hands the
// whole count to one lane, so a constant row costs one add per wave and not a 64-way serialised one.  The deltas gather in an
// LDS histogram of nLevels + 2 signed words and the non-zero ones are then added to the channel's counters by the one workgroup
// that owns them: no global atomic.  Where nLevels + 2 words do not fit the launch's LDS (LDS_WORDS) the same code adds to the
// channel's counters in global memory with workgroup-scope atomics.
//
// A pending settings change (update_settings(), :162-187) is decided on the device: the table holds a serial number that every
// setter that changes something advances, the state the serial that the counters were last counted under.  Where they differ the
// kernel zeroes all nMaxLevels + 2 counters and counts the history that remains under the new step -- the reference's recount of
// the old nCount samples followed by its evictions, whose intermediate nothing can observe inside one launch.  The kernel writes
// nHead, nCount and the serial back: a captured call counts its row again at every replay and recounts at the first only.
//
// The same kernel with OP_UPDATE is update_settings() on its own: the recount of all nCount samples, nothing evicted, so that a
// window longer than a period that was reduced stays visible as it does in the reference.
#include "bank_core.h"
#include "quantized_counter_bank.h"

#pragma clang fp contract(off)

namespace
{
    using namespace mi_qcounter;

    constexpr int BLOCK = 256, WAVE = 64;
    // The LDS histogram's budget: 8192 words = 32 KiB, so five workgroups (20 waves) of the largest histogram still share a CU's
    // 160 KiB.  A launch takes only what its largest channel needs.
    constexpr uint32_t LDS_WORDS = 8192;
    constexpr size_t COUNT_LIMIT = size_t(1) << 31;             // the kernel counts samples in 32 bits
    constexpr uint32_t LEVELS_LIMIT = 1u << 24;                 // float(nLevels) stays exact
    enum { OP_PROCESS = 0, OP_UPDATE = 1 };

    struct device_state { uint32_t head, count, serial; };      // nHead, nCount, the serial of the settings the counters hold

    // where the deltas of one channel go: LDS words [0, levels + 2) or the channel's counters
    template <bool LDS> struct sink
    {
        int32_t    *hist;                                       // LDS
        uint32_t   *counters;                                   // global
        uint32_t    levels, max_levels;

        __device__ __forceinline__ void add(uint32_t word, int32_t d) const
        {
            if (LDS)
                atomicAdd(&hist[(word < max_levels) ? word : word - max_levels + levels], d);
            else
                (void)__hip_atomic_fetch_add(&counters[word], uint32_t(d), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
    };

    // xs[0 .. len) counted with `sign` each by the whole workgroup: single words up to the 16-byte grid, then 16 bytes per lane,
    // then the rest.  Every thread of the workgroup calls this with the same arguments.
    template <bool LDS, bool COMBINE>
    __device__ __forceinline__ void count_span(const sink<LDS> &to, const float *xs, uint32_t len, int32_t sign, float min_value, float rstep)
    {
        const uint32_t t = threadIdx.x, lane = t & (WAVE - 1);
        uint32_t head = (4u - (uint32_t(reinterpret_cast<uintptr_t>(xs) >> 2) & 3u)) & 3u;
        head = (head < len) ? head : len;
        const uint32_t quads = (len - head) >> 2;
        if (t < head)
            to.add(bin_of(scaled(xs[t], min_value, rstep), to.levels, to.max_levels), sign);
        const uint32_t rest = head + 4u * quads + t;
        if (rest < len)
            to.add(bin_of(scaled(xs[rest], min_value, rstep), to.levels, to.max_levels), sign);

        const float4 *q = reinterpret_cast<const float4 *>(xs + head);
        for (uint32_t base = 0; base < quads; base += BLOCK)    // the bound is the workgroup's: every lane of a wave is in the loop
        {
            const uint32_t j = base + t;
            const bool valid = j < quads;
            uint32_t b0 = 0, b1 = 0, b2 = 0, b3 = 0;
            if (valid)
            {
                const float4 v = q[j];
                b0 = bin_of(scaled(v.x, min_value, rstep), to.levels, to.max_levels);
                b1 = bin_of(scaled(v.y, min_value, rstep), to.levels, to.max_levels);
                b2 = bin_of(scaled(v.z, min_value, rstep), to.levels, to.max_levels);
                b3 = bin_of(scaled(v.w, min_value, rstep), to.levels, to.max_levels);
            }
            if (COMBINE)
            {
                // one bin in the whole wave: its first lane with samples adds the lot
                const unsigned long long with = __ballot(valid);
                if (with == 0)
                    continue;
                const int first = __ffsll(with) - 1;
                const uint32_t fb = __shfl(b0, first, WAVE);
                const bool one = !valid || (b0 == fb && b1 == fb && b2 == fb && b3 == fb);
                if (__all(one))
                {
                    if (int(lane) == first)
                        to.add(fb, sign * 4 * int32_t(__popcll(with)));
                    continue;
                }
            }
            if (valid)
            {
                // the lane's runs of equal bins
                uint32_t cur = b0;
                int32_t c = 1;
                if (b1 == cur) ++c; else { to.add(cur, sign * c); cur = b1; c = 1; }
                if (b2 == cur) ++c; else { to.add(cur, sign * c); cur = b2; c = 1; }
                if (b3 == cur) ++c; else { to.add(cur, sign * c); cur = b3; c = 1; }
                to.add(cur, sign * c);
            }
        }
    }

    // `len` samples of the ring from position `pos` on, in at most two spans
    template <bool LDS, bool COMBINE>
    __device__ __forceinline__ void count_ring(const sink<LDS> &to, const float *ring, uint32_t capacity, uint32_t pos, uint32_t len, int32_t sign,
                                               float min_value, float rstep)
    {
        const uint32_t first = (len < capacity - pos) ? len : capacity - pos;
        count_span<LDS, COMBINE>(to, ring + pos, first, sign, min_value, rstep);
        count_span<LDS, COMBINE>(to, ring, len - first, sign, min_value, rstep);
    }

    template <bool LDS, bool COMBINE>
    __device__ __forceinline__ void count_call(const sink<LDS> &to, const float *xs, uint32_t n, const float *ring, uint32_t capacity, const plan &pl,
                                               bool pending, const mi_qcounter_params_t &p)
    {
        if (pending)                                            // the history that remains, counted anew
            count_ring<LDS, COMBINE>(to, ring, capacity, uint32_t((uint64_t(pl.tail) + pl.evict) % capacity), pl.remain, 1, p.min_value, p.rstep);
        else                                                    // the history that leaves
            count_ring<LDS, COMBINE>(to, ring, capacity, pl.tail, pl.evict, -1, p.min_value, p.rstep);
        count_span<LDS, COMBINE>(to, xs + pl.keep_from, n - pl.keep_from, 1, p.min_value, p.rstep);
    }

    template <bool COMBINE>
    __global__ __launch_bounds__(BLOCK) void qcounter_kernel(const float *src, size_t stride, uint32_t n, uint32_t op, uint32_t lds_words,
                                                             const mi_qcounter_params_t *params, device_state *state, float *rings,
                                                             uint32_t *all_counters, uint32_t capacity, uint32_t max_levels)
    {
        extern __shared__ int32_t hist[];                       // lds_words of them
        const uint32_t ch = blockIdx.x, t = threadIdx.x;
        const mi_qcounter_params_t p = params[ch];
        const device_state s = state[ch];
        const bool pending = p.update != s.serial;
        if (op == OP_UPDATE && !pending)                        // the whole workgroup leaves
            return;
        const float *xs = src + size_t(ch) * stride;
        float *ring = rings + size_t(ch) * capacity;
        uint32_t *counters = all_counters + size_t(ch) * (max_levels + 2);
        const uint32_t levels = p.levels, words = levels + 2;

        plan pl = make_plan(s.head, s.count, p.period, capacity, n);
        if (op == OP_UPDATE)                                    // all nCount samples, none evicted
            pl.evict = 0, pl.remain = s.count;
        const bool lds = words <= lds_words;

        if (lds)
            for (uint32_t i = t; i < words; i += BLOCK)
                hist[i] = 0;
        else if (pending)
            for (uint32_t i = t; i < max_levels + 2; i += BLOCK)
                counters[i] = 0;
        __syncthreads();
        if (lds)
            count_call<true, COMBINE>(sink<true>{ hist, counters, levels, max_levels }, xs, n, ring, capacity, pl, pending, p);
        else
            count_call<false, COMBINE>(sink<false>{ hist, counters, levels, max_levels }, xs, n, ring, capacity, pl, pending, p);
        __syncthreads();                                        // the deltas are complete and the ring's leaving samples are read
        if (lds)
        {
            if (pending)                                        // :170: every word, those beyond nLevels too
            {
                for (uint32_t i = t; i < max_levels + 2; i += BLOCK)
                    counters[i] = (i < levels) ? uint32_t(hist[i]) : (i >= max_levels) ? uint32_t(hist[i - max_levels + levels]) : 0u;
            }
            else
                for (uint32_t i = t; i < words; i += BLOCK)
                {
                    const int32_t d = hist[i];
                    if (d != 0)
                        counters[(i < levels) ? i : i - levels + max_levels] += uint32_t(d);
                }
        }
        if (op == OP_UPDATE)
        {
            if (t == 0)
                state[ch].serial = p.update;
            return;
        }
        // the row into the ring: [store_from, n) to store_pos on, around the ring's end
        const uint32_t len = n - pl.store_from;
        const uint32_t first = (len < capacity - pl.store_pos) ? len : capacity - pl.store_pos;
        const float *from = xs + pl.store_from;
        for (uint32_t i = t; i < first; i += BLOCK)
            ring[pl.store_pos + i] = from[i];
        for (uint32_t i = first + t; i < len; i += BLOCK)
            ring[i - first] = from[i];
        if (t == 0)
            state[ch] = device_state{ pl.head_after, pl.count_after, p.update };
    }

    // clear(), :189-196: the counters, nHead and nCount of the flagged channels; the ring's words and the serial stay
    __global__ __launch_bounds__(BLOCK) void qcounter_clear_kernel(const uint8_t *flags, device_state *state, uint32_t *all_counters,
                                                                   uint32_t max_levels)
    {
        const uint32_t ch = blockIdx.x;
        if (!flags[ch])
            return;
        for (uint32_t i = threadIdx.x; i < max_levels + 2; i += BLOCK)
            all_counters[size_t(ch) * (max_levels + 2) + i] = 0;
        if (threadIdx.x == 0)
            state[ch].head = 0, state[ch].count = 0;
    }

    // counters(), below() and above() of every channel: dst[ch][0 .. levels) the bins, then below, then above
    __global__ __launch_bounds__(BLOCK) void qcounter_read_kernel(uint32_t *dst, size_t stride, uint32_t levels, const uint32_t *all_counters,
                                                                  uint32_t max_levels)
    {
        const uint32_t ch = blockIdx.y, i = blockIdx.x * BLOCK + threadIdx.x;
        if (i >= levels + 2)
            return;
        dst[size_t(ch) * stride + i] = all_counters[size_t(ch) * (max_levels + 2) + ((i < levels) ? i : i - levels + max_levels)];
    }
} // namespace

struct mi_qcounter_bank : mi_bank::tables<mi_qcounter_params_t, device_state>
{
    static constexpr const char *NAME = "mi_qcounter_bank";

    uint32_t                max_period = 0, max_levels = 0, capacity = 0;
    float                  *d_ring = nullptr;       // [channels][capacity]
    uint32_t               *d_counters = nullptr;   // [channels][max_levels + 2]
    uint8_t                *d_flags = nullptr;      // [channels]: the channels of a pending clear()
    std::vector<uint8_t>    clears;                 // clear() of every channel, pending
    bool                    work = false;           // ... of some channel
    std::vector<uint8_t>    update;                 // bUpdate of every channel as the host follows it
    std::vector<float>      rstep;                  // fRStep of every channel: that of the last update
    bool                    combine = true;         // the wave-level combining; off for measurements only
};

namespace
{
    int qc_destroy(mi_qcounter_bank *b)
    {
        if (b == nullptr)
            return MI_OK;
        (void)hipFree(b->d_ring); (void)hipFree(b->d_counters); (void)hipFree(b->d_flags);
        return mi_bank::destroy(b);
    }

    // the changed settings go to the device, then the pending clears.  Nothing is recounted here.
    int qc_upload(mi_qcounter_bank *b, hipStream_t st)
    {
        const int r = mi_bank::upload(*b, mi_qcounter_bank::NAME, st);
        if (r != MI_OK || !b->work)
            return r;
        const int k = mi::refuse_capture(mi_qcounter_bank::NAME, st);
        if (k != MI_OK)
            return k;
        MI_HIP_CHECK(hipMemcpyAsync(b->d_flags, b->clears.data(), size_t(b->channels), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(qcounter_clear_kernel, dim3(b->channels), dim3(BLOCK), 0, st, b->d_flags, b->d_state, b->d_counters, b->max_levels);
        MI_HIP_CHECK(hipGetLastError());
        MI_HIP_CHECK(hipStreamSynchronize(st));                 // the host's list may change again after this returns
        b->clears.assign(b->channels, 0);
        b->work = false;
        return MI_OK;
    }

    int qc_channel(const mi_qcounter_bank *b, const char *entry, uint32_t channel)
    {
        MI_REQUIRE(b != nullptr, MI_ESTATE, "%s: NULL bank", entry);
        MI_REQUIRE(channel < b->channels, MI_EINVAL, "%s: channel %u out of range", entry, channel);
        return MI_OK;
    }

    // lsp_limit(v, 1, most), :102, :111, :150
    uint32_t limited(size_t v, uint32_t most)      { return (v < 1) ? 1u : (v > most) ? most : uint32_t(v); }

    void changed(mi_qcounter_bank *b, uint32_t ch)              // bUpdate = true
    {
        ++b->params[ch].update;
        b->params[ch].rstep = rstep_of(b->params[ch].levels, b->params[ch].min_value, b->params[ch].max_value);
        b->update[ch] = 1;
        b->up.touch(ch);
    }

    // OP_PROCESS or OP_UPDATE of every channel; the host's bUpdate of the channels it covers falls
    int qc_launch(mi_qcounter_bank *b, const char *entry, const float *src, size_t count, size_t stride, uint32_t op, hipStream_t st)
    {
        const int r = qc_upload(b, st);
        if (r != MI_OK)
            return r;
        uint32_t most = 0;
        for (uint32_t ch = 0; ch < b->channels; ++ch)
        {
            const mi_qcounter_params_t &p = b->params[ch];
            if (op == OP_UPDATE && !b->update[ch])
                continue;
            // with nLevels == 0 the reference's step is 0 / 0 and with nPeriod == 0 its window holds nothing: defined, meaningless
            MI_REQUIRE(p.levels != 0 && (op == OP_UPDATE || p.period != 0), MI_ESTATE,
                       "%s: channel %u has no %s yet: call set_range() and set_period() first", entry, ch, (p.levels == 0) ? "range" : "period");
            most = (p.levels > most) ? p.levels : most;
        }
        const uint32_t words = (most + 2 <= LDS_WORDS) ? most + 2 : LDS_WORDS;      // channels beyond the budget count in global memory
        hipEvent_t ev0 = nullptr, ev1 = nullptr;
        mi::take_profile_events(&ev0, &ev1);
        if (b->combine)
            MI_LAUNCH(qcounter_kernel<true>, dim3(b->channels), dim3(BLOCK), words * sizeof(int32_t), st, ev0, ev1, src, stride, uint32_t(count), op,
                      words, b->d_params, b->d_state, b->d_ring, b->d_counters, b->capacity, b->max_levels);
        else
            MI_LAUNCH(qcounter_kernel<false>, dim3(b->channels), dim3(BLOCK), words * sizeof(int32_t), st, ev0, ev1, src, stride, uint32_t(count), op,
                      words, b->d_params, b->d_state, b->d_ring, b->d_counters, b->capacity, b->max_levels);
        MI_HIP_CHECK(hipGetLastError());
        for (uint32_t ch = 0; ch < b->channels; ++ch)
            if (b->update[ch])
                b->update[ch] = 0, b->rstep[ch] = b->params[ch].rstep;
        return MI_OK;
    }
} // namespace

extern "C" {

int mi_qcounter_bank_create(mi_qcounter_bank_t **bank, uint32_t channels, size_t max_period, size_t max_levels)  // construct(), init(), :42-98
{
    int r = mi_bank::open_checks(bank, "mi_qcounter_bank_create", channels);
    if (r != MI_OK)
        return r;
    MI_REQUIRE(max_period >= 1 && max_levels >= 1, MI_EINVAL, "mi_qcounter_bank_create: max_period and max_levels must be at least 1");
    MI_REQUIRE(max_levels <= LEVELS_LIMIT, MI_EINVAL, "mi_qcounter_bank_create: max_levels must be 1 .. %u", LEVELS_LIMIT);
    MI_REQUIRE(max_period <= size_t(UINT32_MAX) - 2 * BUFFER_GAP, MI_EINVAL,
               "mi_qcounter_bank_create: a ring of max_period + %zu samples does not fit the reference's 32-bit nCapacity", BUFFER_GAP);
    r = mi_bank::open_new(bank, "mi_qcounter_bank_create");
    if (r != MI_OK)
        return r;
    mi_qcounter_bank *b = *bank;
    b->channels = channels;
    b->max_period = uint32_t(max_period), b->max_levels = uint32_t(max_levels), b->capacity = uint32_t(capacity_of(max_period));
    b->clears.assign(channels, 0);
    b->update.assign(channels, 1);                              // bUpdate = true, :56
    b->rstep.assign(channels, 0.0f);
    // the serial in the table is 1 and in the state 0: the first call counts under its settings, as bUpdate = true has it
    r = mi_bank::alloc(*b, "mi_qcounter_bank_create", mi_qcounter_params_t{ 0, 0, 0.0f, 0.0f, 0.0f, 1 }, device_state{ 0, 0, 0 });
    if (r == MI_OK)
    {
        const size_t ring_bytes = size_t(channels) * b->capacity * sizeof(float), counter_bytes = size_t(channels) * (max_levels + 2) * sizeof(uint32_t);
        hipError_t e = hipMalloc(reinterpret_cast<void **>(&b->d_ring), ring_bytes);
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&b->d_counters), counter_bytes);
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&b->d_flags), size_t(channels));
        if (e == hipSuccess) e = hipMemset(b->d_ring, 0, ring_bytes);
        if (e == hipSuccess) e = hipMemset(b->d_counters, 0, counter_bytes);
        if (e != hipSuccess)
            r = mi::fail(MI_EHIP, "mi_qcounter_bank_create: %s", hipGetErrorString(e));
    }
    if (r != MI_OK)
    {
        *bank = nullptr;
        qc_destroy(b);
    }
    return r;
}

int mi_qcounter_bank_destroy(mi_qcounter_bank_t *b)
{
    return qc_destroy(b);
}

int mi_qcounter_bank_set_period(mi_qcounter_bank_t *b, uint32_t channel, size_t period)                      // :100-107: no bUpdate
{
    const int r = qc_channel(b, "mi_qcounter_bank_set_period", channel);
    if (r != MI_OK)
        return r;
    const uint32_t v = limited(period, b->max_period);
    if (b->params[channel].period != v)
        b->params[channel].period = v, b->up.touch(channel);
    return MI_OK;
}

int mi_qcounter_bank_set_levels(mi_qcounter_bank_t *b, uint32_t channel, size_t levels)                      // :109-117
{
    const int r = qc_channel(b, "mi_qcounter_bank_set_levels", channel);
    if (r != MI_OK)
        return r;
    const uint32_t v = limited(levels, b->max_levels);
    if (b->params[channel].levels != v)
        b->params[channel].levels = v, changed(b, channel);
    return MI_OK;
}

int mi_qcounter_bank_set_min_value(mi_qcounter_bank_t *b, uint32_t channel, float min_value)                 // :119-126
{
    const int r = qc_channel(b, "mi_qcounter_bank_set_min_value", channel);
    if (r != MI_OK)
        return r;
    if (!(b->params[channel].min_value == min_value))
        b->params[channel].min_value = min_value, changed(b, channel);
    return MI_OK;
}

int mi_qcounter_bank_set_max_value(mi_qcounter_bank_t *b, uint32_t channel, float max_value)                 // :128-135
{
    const int r = qc_channel(b, "mi_qcounter_bank_set_max_value", channel);
    if (r != MI_OK)
        return r;
    if (!(b->params[channel].max_value == max_value))
        b->params[channel].max_value = max_value, changed(b, channel);
    return MI_OK;
}

int mi_qcounter_bank_set_value_range(mi_qcounter_bank_t *b, uint32_t channel, float min_value, float max_value)  // :137-146
{
    const int r = qc_channel(b, "mi_qcounter_bank_set_value_range", channel);
    if (r != MI_OK)
        return r;
    mi_qcounter_params_t &p = b->params[channel];
    if (p.min_value == min_value && p.max_value == max_value)
        return MI_OK;
    p.min_value = min_value, p.max_value = max_value;
    changed(b, channel);
    return MI_OK;
}

int mi_qcounter_bank_set_range(mi_qcounter_bank_t *b, uint32_t channel, float min_value, float max_value, size_t levels)  // :148-160
{
    const int r = qc_channel(b, "mi_qcounter_bank_set_range", channel);
    if (r != MI_OK)
        return r;
    mi_qcounter_params_t &p = b->params[channel];
    const uint32_t v = limited(levels, b->max_levels);
    if (p.levels == v && p.min_value == min_value && p.max_value == max_value)
        return MI_OK;
    p.levels = v, p.min_value = min_value, p.max_value = max_value;
    changed(b, channel);
    return MI_OK;
}

int mi_qcounter_bank_set_wave_combining(mi_qcounter_bank_t *b, int on)
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_qcounter_bank_set_wave_combining: NULL bank");
    b->combine = on != 0;
    return MI_OK;
}

int mi_qcounter_bank_needs_update(const mi_qcounter_bank_t *b, uint32_t channel, int *needs)                 // .h:141
{
    const int r = mi_bank::get_checks(b, "mi_qcounter_bank_needs_update", channel, needs);
    if (r == MI_OK)
        *needs = b->update[channel];
    return r;
}

int mi_qcounter_bank_update_settings(mi_qcounter_bank_t *b, void *stream)                                    // :162-187
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_qcounter_bank_update_settings: NULL bank");
    return qc_launch(b, "mi_qcounter_bank_update_settings", nullptr, 0, 0, OP_UPDATE, mi::as_stream(stream));
}

int mi_qcounter_bank_clear(mi_qcounter_bank_t *b, uint32_t channel)                                          // :189-196
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_qcounter_bank_clear: NULL bank");
    MI_REQUIRE(channel < b->channels || channel == UINT32_MAX, MI_EINVAL, "mi_qcounter_bank_clear: channel %u out of range", channel);
    for (uint32_t ch = 0; ch < b->channels; ++ch)
        if (channel == UINT32_MAX || ch == channel)
            b->clears[ch] = 1, b->work = true;
    return MI_OK;
}

int mi_qcounter_bank_process(mi_qcounter_bank_t *b, const float *src, size_t count, size_t stride, void *stream) // :242-266
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_qcounter_bank_process: NULL bank");
    // a call of no samples still takes the settings over and evicts (:245-248)
    const int k = mi_bank::check_rows("mi_qcounter_bank_process", b->channels, count, COUNT_LIMIT,
                                      { { src, stride, count, (count != 0) ? uint32_t(mi_bank::REQUIRED) : 0u } });
    if (k != MI_OK)
        return k;
    return qc_launch(b, "mi_qcounter_bank_process", src, count, stride, OP_PROCESS, mi::as_stream(stream));
}

int mi_qcounter_bank_read(mi_qcounter_bank_t *b, uint32_t *counters, size_t stride, void *stream)           // .h:164-178
{
    MI_REQUIRE(b != nullptr, MI_ESTATE, "mi_qcounter_bank_read: NULL bank");
    hipStream_t st = mi::as_stream(stream);
    const int r = qc_upload(b, st);
    if (r != MI_OK)
        return r;
    uint32_t most = 0;
    for (uint32_t ch = 0; ch < b->channels; ++ch)
        most = (b->params[ch].levels > most) ? b->params[ch].levels : most;
    const size_t words = size_t(most) + 2;
    const int k = mi_bank::check_rows("mi_qcounter_bank_read", b->channels, words, COUNT_LIMIT, { { counters, stride, words, mi_bank::REQUIRED } });
    if (k != MI_OK)
        return k;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    mi::take_profile_events(&ev0, &ev1);
    MI_LAUNCH(qcounter_read_kernel, dim3(uint32_t((words + BLOCK - 1) / BLOCK), b->channels), dim3(BLOCK), 0, st, ev0, ev1, counters, stride, most,
              b->d_counters, b->max_levels);
    MI_HIP_CHECK(hipGetLastError());
    return MI_OK;
}

int mi_qcounter_bank_get_params(const mi_qcounter_bank_t *b, uint32_t channel, mi_qcounter_params_t *params)
{
    const int r = mi_bank::get_params(b, "mi_qcounter_bank_get_params", channel, params);
    if (r == MI_OK)
        params->rstep = b->rstep[channel], params->update = b->update[channel];     // fRStep and bUpdate as the reference has them
    return r;
}

int mi_qcounter_bank_get_state(mi_qcounter_bank_t *b, uint32_t channel, mi_qcounter_state_t *state, float *ring, uint32_t *counters, void *stream)
{
    int r = mi_bank::get_checks(b, "mi_qcounter_bank_get_state", channel, state);
    hipStream_t st = mi::as_stream(stream);
    if (r == MI_OK)
        r = mi::refuse_state_access(st);
    if (r == MI_OK)
        r = qc_upload(b, st);
    if (r != MI_OK)
        return r;
    if (ring != nullptr)
        MI_HIP_CHECK(hipMemcpyAsync(ring, b->d_ring + size_t(channel) * b->capacity, size_t(b->capacity) * sizeof(float), hipMemcpyDeviceToHost, st));
    if (counters != nullptr)
        MI_HIP_CHECK(hipMemcpyAsync(counters, b->d_counters + size_t(channel) * (b->max_levels + 2), size_t(b->max_levels + 2) * sizeof(uint32_t),
                                    hipMemcpyDeviceToHost, st));
    device_state s;
    r = mi::read_state(&s, b->d_state + channel, st);           // synchronises
    if (r != MI_OK)
        return r;
    state->head = s.head, state->count = s.count, state->capacity = b->capacity;
    return MI_OK;
}

int mi_qcounter_bank_set_state(mi_qcounter_bank_t *b, uint32_t channel, const mi_qcounter_state_t *state, const float *ring, const uint32_t *counters,
                               void *stream)
{
    int r = qc_channel(b, "mi_qcounter_bank_set_state", channel);
    if (r != MI_OK)
        return r;
    MI_REQUIRE(state != nullptr, MI_EINVAL, "mi_qcounter_bank_set_state: NULL state");
    hipStream_t st = mi::as_stream(stream);
    r = mi::refuse_state_access(st);
    if (r == MI_OK)
        r = qc_upload(b, st);                                   // a clear() before this call does not undo it
    if (r != MI_OK)
        return r;
    MI_REQUIRE(state->head < b->capacity && state->count <= b->capacity, MI_EINVAL,
               "mi_qcounter_bank_set_state: head %u or count %u outside the ring of %u samples", state->head, state->count, b->capacity);
    if (ring != nullptr)
        MI_HIP_CHECK(hipMemcpyAsync(b->d_ring + size_t(channel) * b->capacity, ring, size_t(b->capacity) * sizeof(float), hipMemcpyHostToDevice, st));
    if (counters != nullptr)
        MI_HIP_CHECK(hipMemcpyAsync(b->d_counters + size_t(channel) * (b->max_levels + 2), counters, size_t(b->max_levels + 2) * sizeof(uint32_t),
                                    hipMemcpyHostToDevice, st));
    // head and count only: the serial of the settings that the counters hold stays
    const uint32_t words[2] = { state->head, state->count };
    MI_HIP_CHECK(hipMemcpyAsync(b->d_state + channel, words, sizeof(words), hipMemcpyHostToDevice, st));
    MI_HIP_CHECK(hipStreamSynchronize(st));
    return MI_OK;
}

} // extern "C"
