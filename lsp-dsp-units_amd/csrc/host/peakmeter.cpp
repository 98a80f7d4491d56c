// lsp::dspu::PeakMeter (src/main/meters/PeakMeter.cpp) on a mi_peakmeter_bank of one channel kept beside the object (beside.h).
// The object's fields are what counts: before every device call update_settings() runs on the host as in the reference (fTau,
// nHold, nCounter clamped), the bank is handed fTau and nHold where they differ from its own, and fPeak and nCounter where they
// are not what the previous call read back; afterwards the two are read back.
#include <lsp-plug.in/dsp-units/meters/PeakMeter.h>
#include <lsp-plug.in/dsp-units/units.h>

#include <cmath>
#include <cstddef>

#include "beside.h"

#pragma clang fp contract(off)

namespace lsp
{
namespace dspu
{
namespace
{
    struct peak_held { float peak = 0.0f; uint32_t counter = 0; };
    typedef mi_host::registry<mi_host::beside<mi_peakmeter_bank_t, peak_held, mi_peakmeter_bank_destroy> > peakmeters;

    int send_state(mi_peakmeter_bank_t *bank, const peak_held &now)
    {
        const mi_peakmeter_state_t s = { now.peak, now.counter };
        return mi_peakmeter_bank_set_state(bank, 0, &s, nullptr);
    }

    static_assert(sizeof(PeakMeter) == 32, "sizeof(PeakMeter)");
}

PeakMeter::PeakMeter()  { construct(); }
PeakMeter::~PeakMeter() { destroy(); }

void PeakMeter::construct()                                     // :40-50
{
    peakmeters::drop(this);                                     // whatever lived at this address before
    fPeak = 0.0f;
    fTau = 1.0f;
    fHold = 5.0f;
    fRelease = 0.0f;
    nHold = 0;
    nCounter = 0;
    nSampleRate = 0;
    bUpdate = true;
}

void PeakMeter::destroy()                                       // :52-55
{
    peakmeters::drop(this);
}

void PeakMeter::set_sample_rate(size_t sample_rate)             // :57-63
{
    if (nSampleRate == sample_rate)
        return;
    nSampleRate = uint32_t(sample_rate);
    bUpdate = true;
}

size_t PeakMeter::sample_rate() const   { return nSampleRate; }

void PeakMeter::set_hold_time(float value)                      // :70-76
{
    if (fHold == value)
        return;
    fHold = value;
    bUpdate = true;
}

float PeakMeter::hold_time() const      { return fHold; }

void PeakMeter::set_release_time(float value)                   // :83-89
{
    if (fRelease == value)
        return;
    fRelease = value;
    bUpdate = true;
}

float PeakMeter::release_time() const   { return fRelease; }

void PeakMeter::set_time(float hold, float release)             // :96-103
{
    if (fHold == hold && fRelease == release)
        return;
    fHold = hold;
    fRelease = release;
    bUpdate = true;
}

float PeakMeter::value() const          { return fPeak; }

void PeakMeter::clear()                                         // :110-114
{
    nCounter = 0;
    fPeak = 0.0f;
}

void PeakMeter::update_settings()                               // :116-125
{
    if (!bUpdate)
        return;
    bUpdate = false;
    // uint32_t(float) is undefined below 0, for NaN and from 2^32 on: clamped here
    const float m = millis_to_samples(float(nSampleRate), fHold);
    nHold = !(m >= 0.0f) ? 0u : (m >= 4294967296.0f) ? UINT32_MAX : uint32_t(m);
    fTau = expf(logf(1.0f - float(M_SQRT1_2)) / millis_to_samples(float(nSampleRate), fRelease));
    nCounter = (nCounter < nHold) ? nCounter : nHold;
}

namespace
{
    // the bank of `self` with the object's fTau, nHold, fPeak and nCounter on the device
    peakmeters::entry *ready(const void *self, float tau, uint32_t hold, float peak, uint32_t counter)
    {
        peakmeters::entry *p = peakmeters::of_one(self, mi_peakmeter_bank_create);
        if (p == nullptr)
            return nullptr;
        mi_peakmeter_params_t q;
        if (mi_peakmeter_bank_get_params(p->bank, 0, &q) != MI_OK)
            return nullptr;
        if (memcmp(&q.tau, &tau, sizeof(float)) != 0 || q.hold != hold)
        {
            q.tau = tau, q.hold = hold;
            if (mi_peakmeter_bank_set_params(p->bank, 0, &q) != MI_OK)
                return nullptr;
        }
        return p->hand_over_state(peak_held{ peak, counter }, send_state) ? p : nullptr;
    }
}

float PeakMeter::process(float *dst, const float *src, size_t count)       // :127-155
{
    update_settings();
    if (count == 0)
        return fPeak;
    peakmeters::entry *p = ready(this, fTau, nHold, fPeak, nCounter);
    if (p == nullptr || !p->buf.reserve(count, 2))
        return fPeak;
    float *d_src = p->buf.row(0), *d_dst = p->buf.row(1);
    mi_peakmeter_state_t s;
    if (!p->buf.up(0, src, count) ||
        mi_peakmeter_bank_process(p->bank, (dst != NULL) ? d_dst : NULL, d_src, NULL, count, count, count, nullptr) != MI_OK ||
        (dst != NULL && !p->buf.down(dst, 1, count)) ||
        mi_peakmeter_bank_get_state(p->bank, 0, &s, nullptr) != MI_OK)
        return fPeak;
    p->held = peak_held{ s.peak, s.counter };
    fPeak = s.peak;
    nCounter = s.counter;
    return fPeak;
}

float PeakMeter::process(const float *data, size_t count)                  // :157-183
{
    return process(NULL, data, count);
}

float PeakMeter::process(float value, size_t count)                        // :185-205
{
    update_settings();
    peakmeters::entry *p = ready(this, fTau, nHold, fPeak, nCounter);
    if (p == nullptr || !p->buf.reserve(1, 2))
        return fPeak;
    // a count beyond 32 bits is beyond every counter: UINT32_MAX decays as far (the factor underflows to 0 or is 1 long before)
    const size_t n = (count < size_t(UINT32_MAX)) ? count : size_t(UINT32_MAX);
    mi_peakmeter_state_t s;
    if (!p->buf.up(0, &value, 1) ||
        mi_peakmeter_bank_process_value(p->bank, NULL, p->buf.row(0), n, nullptr) != MI_OK ||
        mi_peakmeter_bank_get_state(p->bank, 0, &s, nullptr) != MI_OK)
        return fPeak;
    p->held = peak_held{ s.peak, s.counter };
    fPeak = s.peak;
    nCounter = s.counter;
    return fPeak;
}

void PeakMeter::dump(IStateDumper *v) const                                // :207-217
{
    v->write("fPeak", fPeak);
    v->write("fTau", fTau);
    v->write("fHold", fHold);
    v->write("fRelease", fRelease);
    v->write("nHold", nHold);
    v->write("nCounter", nCounter);
    v->write("nSampleRate", nSampleRate);
    v->write("bUpdate", bUpdate);
}

} // namespace dspu
} // namespace lsp
