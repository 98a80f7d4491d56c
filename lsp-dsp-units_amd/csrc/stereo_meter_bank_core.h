// What the banks of correlometer.hip and panometer.hip share on the host: the setters' rules, update_settings(), the checks of
// process() and the device tables.  Both banks keep, per channel, two rings of the bank's capacity, the sums, nHead and
// nWindow on the device (no host positions: calls replay from a captured graph) and period, capacity, norm, law and default
// in a device table uploaded by dirty range (the tables of bank_core.h).  A setter only notes what the reference's setter does
// to the state; it reaches the device at update_settings(), outside the hot path and never inside a capture.
#pragma once
#include "bank_core.h"
#include "stereo_meter_device.h"

namespace mi_stereo_meter
{
    enum { P_WINDOW = 1, P_ZERO_SUMS = 2, P_CLEAR = 4 };    // pending: nWindow = nPeriod; the sums = 0; the rings = 0 and nHead = head

    struct channel_cfg
    {
        uint32_t period = 0, law = 1;
        float    norm = 0.0f, dflt = 0.5f;
        uint32_t head = 0;                  // nPeriod when clear() was called
        uint8_t  pend = 0;
    };

    struct bank_core : mi_bank::tables<meter_params, meter_state>
    {
        const char                 *name = "";              // in messages
        uint32_t                    max_period = 0, capacity = 0;
        uint32_t                    unset = 0;              // channels whose period is still 0
        std::vector<channel_cfg>    cfg;
        bool                        work = false;           // some channel has something pending
        float                      *d_rings = nullptr;      // [channels][2][ring_stride]
        size_t                      ring_stride = 0;
    };

    template <class Bank> int core_destroy(Bank *b)
    {
        if (b != nullptr)
            (void)hipFree(b->d_rings);
        return mi_bank::destroy(b);
    }

    // init(max_period) of every channel of a new, empty bank: period 0, nHead 0, the sums and the rings zero
    inline int core_init(bank_core &b, const char *entry, const char *name, uint32_t channels, uint32_t max_period)
    {
        b.name = name, b.channels = channels, b.max_period = max_period, b.capacity = ring_capacity(max_period);
        b.ring_stride = b.capacity;
        MI_REQUIRE(b.ring_stride * 2 * channels < (size_t(1) << 33), MI_ENOMEM, "%s: %u pairs of rings of %u samples are too much",
                   entry, channels, b.capacity);
        b.unset = channels;
        b.cfg.assign(channels, channel_cfg());
        meter_params p = {};
        p.period = 0, p.capacity = b.capacity, p.norm = 0.0f, p.law = 1, p.dflt = 0.5f;
        b.up.lo = 0, b.up.hi = channels;
        const int r = mi_bank::alloc(b, entry, p, meter_state{});
        if (r != MI_OK)
            return r;
        const size_t ring_bytes = b.ring_stride * 2 * channels * sizeof(float);
        hipError_t e = hipMalloc(reinterpret_cast<void **>(&b.d_rings), ring_bytes);
        if (e == hipSuccess) e = hipMemset(b.d_rings, 0, ring_bytes);
        MI_REQUIRE(e == hipSuccess, MI_EHIP, "%s: %s", entry, hipGetErrorString(e));
        return MI_OK;
    }

    // create(): the bank, and its channels as init(max_period) leaves them
    template <class Bank> int core_create(Bank **bank, const char *entry, const char *name, uint32_t channels, uint32_t max_period)
    {
        int r = mi_bank::open_checks(bank, entry, channels);
        if (r != MI_OK)
            return r;
        MI_REQUIRE(max_period > 0 && max_period <= MAX_PERIOD, MI_EINVAL, "%s: a longest period of %u samples (1 .. %u)", entry,
                   max_period, MAX_PERIOD);
        r = mi_bank::open_new(bank, entry);
        if (r != MI_OK)
            return r;
        r = core_init(**bank, entry, name, channels, max_period);
        if (r != MI_OK)
        {
            core_destroy(*bank);
            *bank = nullptr;
        }
        return r;
    }

    // set_period(): clamped, an unchanged value ignored.  pend: what a change leaves to do (P_WINDOW for the Correlometer's
    // update flag, P_WINDOW | P_ZERO_SUMS for the Panometer, which acts at once).  0 is refused: the reference's process() never
    // ends with it.
    inline int core_set_period(bank_core &b, uint32_t channel, uint32_t period, uint8_t pend)
    {
        MI_REQUIRE(channel < b.channels, MI_EINVAL, "%s_set_period: channel %u out of range", b.name, channel);
        MI_REQUIRE(period > 0, MI_EINVAL, "%s_set_period: a period of 0 samples", b.name);
        channel_cfg &c = b.cfg[channel];
        period = (period < b.max_period) ? period : b.max_period;
        if (period == c.period)
            return MI_OK;
        b.unset -= (c.period == 0) ? 1 : 0;
        c.period = period;
        c.norm = 1.0f / float(period);
        c.pend |= pend;
        b.work = true;
        return MI_OK;
    }

    // clear() of one channel or of all (UINT32_MAX): the rings zero, nHead = nPeriod as it is now, and (zero_sums) the sums
    inline int core_clear(bank_core &b, uint32_t channel, bool zero_sums)
    {
        MI_REQUIRE(channel < b.channels || channel == UINT32_MAX, MI_EINVAL, "%s_clear: channel %u out of range", b.name, channel);
        for (uint32_t ch = 0; ch < b.channels; ++ch)
            if (channel == UINT32_MAX || ch == channel)
            {
                b.cfg[ch].pend |= uint8_t(P_CLEAR | (zero_sums ? P_ZERO_SUMS : 0));
                b.cfg[ch].head = b.cfg[ch].period;
            }
        b.work = true;
        return MI_OK;
    }

    inline int core_update(bank_core &b, hipStream_t st)
    {
        if (!b.work && !b.up.any())
            return MI_OK;
        const int r = mi::refuse_capture(b.name, st);
        if (r != MI_OK)
            return r;
        if (b.work)
        {
            std::vector<meter_state> hs(b.channels);
            MI_HIP_CHECK(hipMemcpyAsync(hs.data(), b.d_state, hs.size() * sizeof(meter_state), hipMemcpyDeviceToHost, st));
            MI_HIP_CHECK(hipStreamSynchronize(st));
            for (uint32_t ch = 0; ch < b.channels; ++ch)
            {
                channel_cfg &c = b.cfg[ch];
                if (c.pend == 0)
                    continue;
                if (c.pend & P_CLEAR)
                {
                    MI_HIP_CHECK(hipMemsetAsync(b.d_rings + size_t(ch) * 2 * b.ring_stride, 0, 2 * b.ring_stride * sizeof(float), st));
                    hs[ch].head = c.head % b.capacity;
                }
                if (c.pend & P_ZERO_SUMS)
                    hs[ch].sum[0] = hs[ch].sum[1] = hs[ch].sum[2] = 0.0f;
                if (c.pend & P_WINDOW)
                    hs[ch].window = c.period;
                c.pend = 0;
                b.up.touch(ch);
            }
            MI_HIP_CHECK(hipMemcpyAsync(b.d_state, hs.data(), hs.size() * sizeof(meter_state), hipMemcpyHostToDevice, st));
            MI_HIP_CHECK(hipStreamSynchronize(st));                     // `hs` is gone after this returns
            b.work = false;
        }
        for (uint32_t ch = b.up.lo; ch < b.up.hi; ++ch)
        {
            const channel_cfg &c = b.cfg[ch];
            meter_params &p = b.params[ch];
            p.period = c.period, p.capacity = b.capacity, p.norm = c.norm, p.law = c.law, p.dflt = c.dflt;
        }
        return mi_bank::upload(b, b.name, st);
    }

    // the state of one channel as given: nHead inside the ring, nWindow at most the period
    inline int core_set_state(bank_core &b, uint32_t channel, meter_state s, bool zero_rings, hipStream_t st)
    {
        MI_REQUIRE(channel < b.channels, MI_EINVAL, "%s_set_state: channel %u out of range", b.name, channel);
        int r = mi::refuse_state_access(st);                        // before the rings' memset below could go into a capture
        if (r == MI_OK)
            r = core_update(b, st);
        if (r != MI_OK)
            return r;
        s.head %= b.capacity;
        s.window = (s.window < b.cfg[channel].period) ? s.window : b.cfg[channel].period;
        if (zero_rings)
            MI_HIP_CHECK(hipMemsetAsync(b.d_rings + size_t(channel) * 2 * b.ring_stride, 0, 2 * b.ring_stride * sizeof(float), st));
        return mi::write_state(b.d_state + channel, s, st);
    }

    // what process() checks once the settings are on the device and count > 0; vec: where 16-byte accesses are allowed
    inline int core_check(const bank_core &b, const char *entry, const float *out, const float *a, const float *in_b, size_t count,
                          size_t out_stride, size_t a_stride, size_t b_stride, uint32_t *vec)
    {
        if (b.unset > 0)
            for (uint32_t ch = 0; ch < b.channels; ++ch)
                MI_REQUIRE(b.cfg[ch].period > 0, MI_ESTATE, "%s: channel %u has no period yet (the reference's process() never "
                                                            "ends with a period of 0); call set_period() first", entry, ch);
        const int r = mi_bank::check_rows(entry, b.channels, count, size_t(1) << 31,
                                          { { out, out_stride, count, mi_bank::REQUIRED | mi_bank::OUTPUT },
                                            { a, a_stride, count, mi_bank::REQUIRED }, { in_b, b_stride, count, mi_bank::REQUIRED } });
        if (r != MI_OK)
            return r;
        *vec = (mi::aligned16(out, out_stride, b.channels) ? VEC_OUT : 0) | (mi::aligned16(a, a_stride, b.channels) ? VEC_A : 0) |
               (mi::aligned16(in_b, b_stride, b.channels) ? VEC_B : 0);
        return MI_OK;
    }
} // namespace mi_stereo_meter
