// lsp::dspu::TruePeakMeter (src/main/meters/TruePeakMeter.cpp) on a mi_truepeak_bank of one channel.  process() stages the
// caller's host block through device memory, like the other compatibility classes (dspu_classes.cpp): correct, but many
// meters belong in one bank with the samples kept in HBM.
#include <lsp-plug.in/dsp-units/meters/TruePeakMeter.h>

#include <algorithm>
#include <cmath>
#include <new>

#include "beside.h"

namespace lsp
{
namespace dspu
{
namespace
{
    struct truepeak_impl
    {
        mi_truepeak_bank_t *bank = nullptr;
        mi_host::rows buf;                  // [1][cap]: the staged block (process() runs in place on it)
        float  *d_peak = nullptr;
    };

    inline truepeak_impl *impl_of(uint8_t *p) { return reinterpret_cast<truepeak_impl *>(p); }

    template <size_t N>
    inline void reduce(float *dst, const float *src, size_t count)
    {
        for (size_t i = 0; i < count; ++i, src += N)
        {
            float m = std::fabs(src[0]);
            for (size_t k = 1; k < N; ++k)
                m = std::max(m, std::fabs(src[k]));
            dst[i] = m;
        }
    }
}

TruePeakMeter::TruePeakMeter()  { construct(); }
TruePeakMeter::~TruePeakMeter() { destroy(); }

void TruePeakMeter::construct()                                 // TruePeakMeter.cpp:47-57
{
    nSampleRate = 0;
    nHead = 0;
    nTimes = 0;
    bUpdate = true;
    pFunc = nullptr;
    pReduce = nullptr;
    vBuffer = nullptr;
    pData = nullptr;
}

void TruePeakMeter::destroy()                                   // :59-67
{
    if (truepeak_impl *p = impl_of(pData))
    {
        mi_truepeak_bank_destroy(p->bank);
        p->buf.release();
        mi_dspu_free(p->d_peak);
        delete p;
    }
    pFunc = nullptr;
    vBuffer = nullptr;
    pData = nullptr;
}

bool TruePeakMeter::init()                                      // :69-82
{
    destroy();
    truepeak_impl *p = new (std::nothrow) truepeak_impl();
    if (p == nullptr)
        return false;
    if (mi_truepeak_bank_create(&p->bank, 1) != MI_OK ||
        mi_dspu_malloc(reinterpret_cast<void **>(&p->d_peak), sizeof(float)) != MI_OK)
    {
        mi_truepeak_bank_destroy(p->bank);
        delete p;
        return false;
    }
    pData = reinterpret_cast<uint8_t *>(p);
    // the bank starts as the reference object after construct(): rate 0, an update pending; mirror its rate and flag
    if (nSampleRate != 0)
        mi_truepeak_bank_set_sample_rate(p->bank, nSampleRate);
    clear();
    return true;
}

uint8_t TruePeakMeter::calc_oversampling_multiplier(size_t sample_rate)     // :85-100
{
    const size_t f = 4 * 44100;
    if (sample_rate >= f)       return 0;
    if (sample_rate * 2 >= f)   return 2;
    if (sample_rate * 3 >= f)   return 3;
    if (sample_rate * 4 >= f)   return 4;
    if (sample_rate * 6 >= f)   return 6;
    return 8;
}

void TruePeakMeter::set_sample_rate(uint32_t sr)                // :102-109
{
    if (nSampleRate == sr)
        return;
    nSampleRate = sr;
    bUpdate = true;
    if (truepeak_impl *p = impl_of(pData))
        mi_truepeak_bank_set_sample_rate(p->bank, sr);
}

size_t TruePeakMeter::sample_rate() const
{
    return nSampleRate;
}

void TruePeakMeter::reduce_2x(float *dst, const float *src, size_t count) { reduce<2>(dst, src, count); }     // :115-147
void TruePeakMeter::reduce_3x(float *dst, const float *src, size_t count) { reduce<3>(dst, src, count); }
void TruePeakMeter::reduce_4x(float *dst, const float *src, size_t count) { reduce<4>(dst, src, count); }
void TruePeakMeter::reduce_6x(float *dst, const float *src, size_t count) { reduce<6>(dst, src, count); }
void TruePeakMeter::reduce_8x(float *dst, const float *src, size_t count) { reduce<8>(dst, src, count); }

void TruePeakMeter::update_settings()                           // :149-189
{
    if (!bUpdate)
        return;
    bUpdate = false;
    truepeak_impl *p = impl_of(pData);
    if (p != nullptr)
        mi_truepeak_bank_update_settings(p->bank, nullptr);
    const uint8_t times = calc_oversampling_multiplier(nSampleRate);
    if (nTimes == times)
        return;
    nTimes = times;
    switch (times)
    {
        case 2:  pReduce = reduce_2x; break;
        case 3:  pReduce = reduce_3x; break;
        case 4:  pReduce = reduce_4x; break;
        case 6:  pReduce = reduce_6x; break;
        case 8:  pReduce = reduce_8x; break;
        default: pReduce = nullptr; break;
    }
    nHead = 0;                                                  // the bank cleared its state
}

void TruePeakMeter::clear()                                     // :191-195
{
    nHead = 0;
    if (truepeak_impl *p = impl_of(pData))
        mi_truepeak_bank_clear(p->bank, nullptr);
}

void TruePeakMeter::process(float *dst, const float *src, size_t count)    // :197-236
{
    update_settings();
    truepeak_impl *p = impl_of(pData);
    if (p == nullptr || count == 0 || !p->buf.reserve(count))
        return;
    if (p->buf.up(0, src, count) &&
        mi_truepeak_bank_process(p->bank, p->buf.row(0), p->buf.row(0), count, count, count, nullptr) == MI_OK &&
        p->buf.down(dst, 0, count))
        mi_dspu_stream_synchronize(nullptr);
}

void TruePeakMeter::process(float *buf, size_t count)
{
    process(buf, buf, count);
}

// The largest value process() would have written (see the header): the reference's returns 0.0f.
float TruePeakMeter::process_max(const float *src, size_t count)
{
    update_settings();
    truepeak_impl *p = impl_of(pData);
    if (p == nullptr || count == 0 || !p->buf.reserve(count))
        return 0.0f;
    float peak = 0.0f;
    if (!p->buf.up(0, src, count) ||
        mi_truepeak_bank_process_max(p->bank, p->d_peak, p->buf.row(0), count, count, nullptr) != MI_OK ||
        mi_dspu_copy_d2h(&peak, p->d_peak, sizeof(float), nullptr) != MI_OK ||
        mi_dspu_stream_synchronize(nullptr) != MI_OK)
        return 0.0f;
    return peak;
}

size_t TruePeakMeter::latency() const                           // :274-277
{
    return (nTimes != 0) ? 10 : 0;
}

void TruePeakMeter::dump(IStateDumper *v) const                 // :279-291
{
    v->write("nSampleRate", nSampleRate);
    v->write("nHead", nHead);
    v->write("nTimes", nTimes);
    v->write("bUpdate", bUpdate);
    v->write("pFunc", reinterpret_cast<const void *>(pFunc));
    v->write("pReduce", reinterpret_cast<const void *>(pReduce));
    v->write("vBuffer", vBuffer);
    v->write("pData", pData);
}

} // namespace dspu
} // namespace lsp
