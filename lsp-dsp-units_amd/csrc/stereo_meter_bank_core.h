// What the banks of correlometer.hip and panometer.hip share on the host: the setters' rules, update_settings(), the checks of
// process() and the device tables.  Both banks keep, per channel, two rings of the bank's capacity, the sums, nHead and
// nWindow on the device (no host positions: calls replay from a captured graph) and period, capacity, norm, law and default
// in a device table uploaded by dirty range.  A setter only notes what the reference's setter does to the state; it reaches
// the device at update_settings(), outside the hot path and never inside a capture.
#pragma once
#include "stereo_meter_device.h"

#include <new>
#include <vector>

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

    struct bank_core
    {
        const char                 *name = "";              // in messages
        uint32_t                    channels = 0, max_period = 0, capacity = 0;
        uint32_t                    unset = 0;              // channels whose period is still 0
        std::vector<channel_cfg>    cfg;
        std::vector<meter_params>   params;                 // what the device table holds, or will after the upload
        mi::dirty_range             up;
        bool                        work = false;           // some channel has something pending
        meter_params               *d_params = nullptr;     // [channels]
        meter_state                *d_state = nullptr;      // [channels]
        float                      *d_rings = nullptr;      // [channels][2][ring_stride]
        size_t                      ring_stride = 0;
    };

    inline void core_destroy(bank_core &b)
    {
        (void)hipFree(b.d_params); (void)hipFree(b.d_state); (void)hipFree(b.d_rings);
        b.d_params = nullptr, b.d_state = nullptr, b.d_rings = nullptr;
    }

    // init(max_period) of every channel: period 0, nHead 0, the sums and the rings zero
    inline int core_create(bank_core &b, const char *name, uint32_t channels, uint32_t max_period)
    {
        MI_REQUIRE(channels > 0 && channels <= (1u << 20), MI_EINVAL, "%s_create: channels must be 1 .. 1048576", name);
        MI_REQUIRE(max_period > 0 && max_period <= MAX_PERIOD, MI_EINVAL, "%s_create: a longest period of %u samples (1 .. %u)", name,
                   max_period, MAX_PERIOD);
        MI_REQUIRE(mi_dspu_device_count() > 0, MI_ENODEV, "no HIP device available (there is no CPU fallback)");
        b.name = name, b.channels = channels, b.max_period = max_period, b.capacity = ring_capacity(max_period);
        b.ring_stride = b.capacity;
        MI_REQUIRE(b.ring_stride * 2 * channels < (size_t(1) << 33), MI_ENOMEM, "%s_create: %u pairs of rings of %u samples are too much",
                   name, channels, b.capacity);
        b.unset = channels;
        b.cfg.assign(channels, channel_cfg());
        meter_params p = {};
        p.period = 0, p.capacity = b.capacity, p.norm = 0.0f, p.law = 1, p.dflt = 0.5f;
        b.params.assign(channels, p);
        b.up.lo = 0, b.up.hi = channels;
        const size_t ring_bytes = b.ring_stride * 2 * channels * sizeof(float);
        hipError_t e = hipMalloc(reinterpret_cast<void **>(&b.d_params), size_t(channels) * sizeof(meter_params));
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&b.d_state), size_t(channels) * sizeof(meter_state));
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&b.d_rings), ring_bytes);
        if (e == hipSuccess) e = hipMemset(b.d_state, 0, size_t(channels) * sizeof(meter_state));
        if (e == hipSuccess) e = hipMemset(b.d_rings, 0, ring_bytes);
        if (e != hipSuccess)
        {
            core_destroy(b);
            return mi::fail(MI_EHIP, "%s_create: %s", name, hipGetErrorString(e));
        }
        return MI_OK;
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
        return mi::upload_dirty(b.name, b.d_params, b.params.data(), b.up, st);
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
    inline int core_check(const bank_core &b, const float *out, const float *a, const float *in_b, size_t count, size_t out_stride,
                          size_t a_stride, size_t b_stride, uint32_t *vec)
    {
        if (b.unset > 0)
            for (uint32_t ch = 0; ch < b.channels; ++ch)
                MI_REQUIRE(b.cfg[ch].period > 0, MI_ESTATE, "%s_process: channel %u has no period yet (the reference's process() never "
                                                            "ends with a period of 0); call set_period() first", b.name, ch);
        MI_REQUIRE(out != nullptr && a != nullptr && in_b != nullptr, MI_EINVAL, "%s_process: NULL output or input", b.name);
        MI_REQUIRE(count < (size_t(1) << 31), MI_EINVAL, "%s_process: count %zu too large", b.name, count);
        MI_REQUIRE(b.channels == 1 || (out_stride >= count && a_stride >= count && b_stride >= count), MI_EINVAL,
                   "%s_process: strides (%zu, %zu, %zu) shorter than count %zu", b.name, out_stride, a_stride, b_stride, count);
        MI_REQUIRE((out != a || out_stride == a_stride) && (out != in_b || out_stride == b_stride), MI_EINVAL,
                   "%s_process: in place with different strides", b.name);
        *vec = (mi::aligned16(out, out_stride, b.channels) ? VEC_OUT : 0) | (mi::aligned16(a, a_stride, b.channels) ? VEC_A : 0) |
               (mi::aligned16(in_b, b_stride, b.channels) ? VEC_B : 0);
        return MI_OK;
    }
} // namespace mi_stereo_meter
