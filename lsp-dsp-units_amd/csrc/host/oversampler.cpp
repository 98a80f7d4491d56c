// lsp::dspu::Oversampler (src/main/util/Oversampler.cpp) on a mi_oversampler_bank of one channel.  The host-pointer
// methods stage the caller's block through device memory, like the other compatibility classes (dspu_classes.cpp):
// correct, but many channels belong in one bank with the samples kept in HBM.  The class's callbacks are host functions:
// process() brings the oversampled block to the host for them and sends it back for the filter and the decimation.
#include <lsp-plug.in/dsp-units/util/Oversampler.h>

#include <cstring>
#include <new>
#include <vector>

#include "beside.h"

namespace lsp
{
namespace dspu
{
namespace
{
    struct oversampler_impl
    {
        mi_oversampler_bank_t *bank = nullptr;
        mi_host::rows over;                 // [1][cap]: the staged oversampled block; two buffers, their lengths differ
        mi_host::rows base;                 // [1][cap]: the staged base-rate block (declared last: released first, as ever)
        std::vector<float> h_over;
    };

    inline oversampler_impl *impl_of(uint8_t *p) { return reinterpret_cast<oversampler_impl *>(p); }

    // the object's mode and filtering flag are the truth; the bank follows before every call
    inline oversampler_impl *synced(uint8_t *p, size_t mode, bool filter)
    {
        oversampler_impl *im = impl_of(p);
        if (im != nullptr)
        {
            mi_oversampler_bank_set_mode(im->bank, uint32_t(mode));
            mi_oversampler_bank_set_filtering(im->bank, filter ? 1 : 0);
        }
        return im;
    }

    struct plain_callback
    {
        oversampler_callback_t  func;
        void                   *arg;
    };
}

IOversamplerCallback::~IOversamplerCallback()
{
}

void IOversamplerCallback::process(float *out, const float *in, size_t samples)        // Oversampler.cpp:38-41
{
    if (out != in)
        memmove(out, in, samples * sizeof(float));
}

Oversampler::Oversampler()  { construct(); }
Oversampler::~Oversampler() { destroy(); }

void Oversampler::construct()                                   // Oversampler.cpp:53-68
{
    pCallback = nullptr;
    fUpBuffer = nullptr;
    fDownBuffer = nullptr;
    pFunc = nullptr;
    nUpHead = 0;
    nMode = OM_NONE;
    nSampleRate = 0;
    nUpdate = UP_ALL;
    sFilter.construct();
    bData = nullptr;
    bFilter = true;
}

bool Oversampler::init()                                        // :70-93
{
    if (!sFilter.init(nullptr))
        return false;
    if (bData == nullptr)
    {
        oversampler_impl *p = new (std::nothrow) oversampler_impl();
        if (p == nullptr)
            return false;
        if (mi_oversampler_bank_create(&p->bank, 1) != MI_OK)
        {
            delete p;
            return false;
        }
        bData = reinterpret_cast<uint8_t *>(p);
        if (nSampleRate != 0)
            mi_oversampler_bank_set_sample_rate(p->bank, uint32_t(nSampleRate));
    }
    nUpHead = 0;
    return true;
}

void Oversampler::destroy()                                     // :95-106
{
    sFilter.destroy();
    if (oversampler_impl *p = impl_of(bData))
    {
        mi_oversampler_bank_destroy(p->bank);
        delete p;
    }
    fUpBuffer = nullptr;
    fDownBuffer = nullptr;
    bData = nullptr;
    pCallback = nullptr;
}

void Oversampler::set_sample_rate(size_t sr)                    // :108-126
{
    if (sr == nSampleRate)
        return;
    nSampleRate = sr;
    nUpdate |= UP_SAMPLE_RATE;
    const size_t os = get_oversampling();

    filter_params_t fp;
    const float cutoff = sr * 0.42f;
    fp.fFreq = (cutoff < 20000.0f) ? cutoff : 20000.0f;
    fp.fFreq2 = fp.fFreq;
    fp.fGain = 1.0f;
    fp.fQuality = 0.1f;
    fp.nSlope = 30;
    fp.nType = FLT_BT_BWC_LOPASS;
    sFilter.update(nSampleRate * os, &fp);
    if (oversampler_impl *p = synced(bData, nMode, bFilter))
        mi_oversampler_bank_set_sample_rate(p->bank, uint32_t(sr));
}

void Oversampler::update_settings()                             // :128-144
{
    if (nUpdate & (UP_MODE | UP_SAMPLE_RATE))
    {
        nUpHead = 0;
        sFilter.clear();
    }
    const size_t os = get_oversampling();
    filter_params_t fp;
    sFilter.get_params(&fp);
    sFilter.update(nSampleRate * os, &fp);
    if (oversampler_impl *p = synced(bData, nMode, bFilter))
        mi_oversampler_bank_update_settings(p->bank, nullptr);
    nUpdate = 0;
}

size_t Oversampler::get_oversampling() const                    // :146-195
{
    static const uint8_t times[5] = { 2, 3, 4, 6, 8 };
    return (nMode >= OM_LANCZOS_2X2 && nMode <= OM_LANCZOS_8X24BIT) ? times[(nMode - 1) / 6] : 1;
}

size_t Oversampler::latency() const                             // :955-1006
{
    static const uint8_t a[6] = { 2, 3, 4, 4, 10, 62 };
    return (nMode >= OM_LANCZOS_2X2 && nMode <= OM_LANCZOS_8X24BIT) ? a[(nMode - 1) % 6] : 0;
}

Oversampler::resample_func_t Oversampler::get_function(size_t)  // :1008-1052
{
    return nullptr;
}

void Oversampler::set_mode(over_mode_t mode)                    // :1055-1063
{
    if (nMode == size_t(mode))
        return;
    nMode = mode;
    pFunc = get_function(mode);
    nUpdate |= UP_MODE;
}

over_mode_t Oversampler::mode() const       { return over_mode_t(nMode); }      // :1065-1068
bool Oversampler::filtering() const         { return bFilter; }                 // :1070-1073

void Oversampler::upsample(float *dst, const float *src, size_t samples)       // :197-367
{
    oversampler_impl *p = synced(bData, nMode, bFilter);
    const size_t os = get_oversampling();
    if (p == nullptr || samples == 0 || !p->base.reserve(samples) || !p->over.reserve(samples * os))
        return;
    if (p->base.up(0, src, samples) &&
        mi_oversampler_bank_upsample(p->bank, p->over.row(0), p->base.row(0), samples, samples * os, samples, nullptr) == MI_OK &&
        p->over.down(dst, 0, samples * os))
        mi_dspu_stream_synchronize(nullptr);
}

void Oversampler::downsample(float *dst, const float *src, size_t samples)     // :369-525
{
    oversampler_impl *p = synced(bData, nMode, bFilter);
    const size_t os = get_oversampling();
    if (p == nullptr || samples == 0 || !p->base.reserve(samples) || !p->over.reserve(samples * os))
        return;
    if (p->over.up(0, src, samples * os) &&
        mi_oversampler_bank_downsample(p->bank, p->base.row(0), p->over.row(0), samples, samples, samples * os, nullptr) == MI_OK &&
        p->base.down(dst, 0, samples))
        mi_dspu_stream_synchronize(nullptr);
}

void Oversampler::process(float *dst, const float *src, size_t samples, IOversamplerCallback *callback)    // :527-739
{
    if (nMode == OM_NONE || callback == nullptr)
    {
        if (nMode == OM_NONE && callback != nullptr)            // :731-737
        {
            callback->process(dst, src, samples);
            return;
        }
        // nothing between up and down: the bank's process() keeps the oversampled block on the device
        oversampler_impl *p = synced(bData, nMode, bFilter);
        if (p == nullptr || samples == 0 || !p->base.reserve(samples))
            return;
        if (p->base.up(0, src, samples) &&
            mi_oversampler_bank_process(p->bank, p->base.row(0), p->base.row(0), samples, samples, samples, nullptr, nullptr, nullptr) == MI_OK &&
            p->base.down(dst, 0, samples))
            mi_dspu_stream_synchronize(nullptr);
        return;
    }
    oversampler_impl *p = impl_of(bData);
    if (p == nullptr || samples == 0)
        return;
    const size_t over = samples * get_oversampling();
    try { p->h_over.resize(over); } catch (...) { return; }
    upsample(p->h_over.data(), src, samples);
    callback->process(p->h_over.data(), p->h_over.data(), over);
    downsample(dst, p->h_over.data(), samples);
}

void Oversampler::process(float *dst, const float *src, size_t samples, oversampler_callback_t callback, void *arg)    // :741-953
{
    struct adapter: public IOversamplerCallback
    {
        plain_callback cb;
        void process(float *out, const float *in, size_t n) override { cb.func(out, in, n, cb.arg); }
    } a;
    a.cb.func = callback;
    a.cb.arg = arg;
    process(dst, src, samples, (callback != nullptr) ? &a : static_cast<IOversamplerCallback *>(nullptr));
}

void Oversampler::dump(IStateDumper *v) const                   // :1075-1088
{
    v->write("pCallback", static_cast<const void *>(pCallback));
    v->write("fUpBuffer", fUpBuffer);
    v->write("fDownBuffer", fDownBuffer);
    v->write("pFunc", reinterpret_cast<const void *>(pFunc));
    v->write("nUpHead", nUpHead);
    v->write("nMode", nMode);
    v->write("nSampleRate", nSampleRate);
    v->write("nUpdate", nUpdate);
    v->write_object("sFilter", &sFilter);
    v->write("bData", bData);
    v->write("bFilter", bFilter);
}

} // namespace dspu
} // namespace lsp
