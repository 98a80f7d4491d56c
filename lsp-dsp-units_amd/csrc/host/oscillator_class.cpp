// lsp::dspu::Oscillator (src/main/util/Oscillator.cpp) on a mi_oscillator_bank of one channel.  The members are the truth: the
// setters and update_settings() work on them (update_settings through mi_oscillator_settings_update, the arithmetic the bank
// uses), and a call hands them to the bank where they differ from what it holds.  nPhaseAcc moves on the host by the call's
// samples, as on the device.  pData is the handle: the bank, two staging rows, and what the bank was given last.
#include <lsp-plug.in/dsp-units/util/Oscillator.h>

#include <cmath>
#include <cstddef>
#include <cstring>
#include <new>
#include <vector>

#include "beside.h"

#define PROCESS_BUF_LIMIT_SIZE  (12 * 1024)                     // :26

namespace lsp
{
namespace dspu
{
namespace
{
    struct handle
    {
        mi_oscillator_bank_t       *bank = nullptr;
        mi_host::rows               buf;                        // [2][cap]: dst, src
        mi_oscillator_settings_t    given = {};                 // what the bank is to hold
        bool                        built = false, any = false; // given was made by update_settings(); the bank has it
        uint32_t                    acc = 0;                    // nPhaseAcc on the device

        ~handle() { mi_oscillator_bank_destroy(bank); }
    };

    handle *of(uint8_t *p) { return reinterpret_cast<handle *>(p); }

    // the members and the phase go to the bank where it does not hold them
    bool hand_over(handle *h, uint32_t acc)
    {
        if (!h->built)
            return false;
        if (h->any && h->acc == acc)
            return true;
        h->given.phase_known = 1, h->given.phase = acc, h->given.sync = 0;
        if (mi_oscillator_bank_set_settings(h->bank, 0, &h->given) != MI_OK)
            return false;
        h->any = true, h->acc = acc;
        return true;
    }

    static_assert(sizeof(Oscillator) == 608, "sizeof(Oscillator)");
}

Oscillator::Oscillator()    { construct(); }
Oscillator::~Oscillator()   { destroy(); }

void Oscillator::construct()                                    // :42-117
{
    enFunction = FG_SINE;
    fAmplitude = 1.0f;
    fFrequency = 0.0f;
    fDCOffset = 0.0f;
    enDCReference = DC_WAVEDC;
    fReferencedDC = 0.0f;
    fInitPhase = 0.0f;
    nSampleRate = -1;
    nPhaseAcc = 0;
    nPhaseAccBits = sizeof(phacc_t) * 8;
    nPhaseAccMaxBits = sizeof(phacc_t) * 8;
    nPhaseAccMask = 0;
    fAcc2Phase = 0.0f;
    nFreqCtrlWord = 0;
    nInitPhaseWord = 0;
    memset(&sSquaredSinusoid, 0, sizeof(sSquaredSinusoid));
    memset(&sRectangular, 0, sizeof(sRectangular));
    memset(&sSawtooth, 0, sizeof(sSawtooth));
    memset(&sTrapezoid, 0, sizeof(sTrapezoid));
    memset(&sPulse, 0, sizeof(sPulse));
    memset(&sParabolic, 0, sizeof(sParabolic));
    sRectangular.fDutyRatio = 0.5f;
    sSawtooth.fWidth = 1.0f;
    sTrapezoid.fRaiseRatio = 0.25f;
    sTrapezoid.fFallRatio = 0.25f;
    sParabolic.fAmplitude = 1.0f;
    sOver.construct();                                          // nothing is owned yet: valid on raw memory, harmless twice
    sOverGetPeriods.construct();
    nOversampling = 0;
    enOverMode = OM_NONE;
    vProcessBuffer = NULL;
    vSynthBuffer = NULL;
    pData = NULL;
    nFreqCtrlWord_Over = 0;
    bSync = true;
}

bool Oscillator::init()                                         // :119-135
{
    if (pData == NULL)
    {
        handle *h = new (std::nothrow) handle();
        if (h == nullptr)
            return false;
        if (mi_oscillator_bank_create(&h->bank, 1) != MI_OK)
        {
            delete h;
            return false;
        }
        pData = reinterpret_cast<uint8_t *>(h);
    }
    const bool over = sOver.init(), periods = sOverGetPeriods.init();
    return over && periods;
}

void Oscillator::destroy()                                      // :137-149
{
    sOver.destroy();
    sOverGetPeriods.destroy();
    if (pData != NULL)
    {
        delete of(pData);
        pData = NULL;
    }
    vProcessBuffer = NULL;
    vSynthBuffer = NULL;
}

void Oscillator::update_settings()                              // :151-357
{
    if (!bSync)
        return;
    mi_oscillator_settings_t s;
    mi_oscillator_settings_init(&s);
    s.function = enFunction, s.amplitude = fAmplitude, s.frequency = fFrequency, s.dc_offset = fDCOffset;
    s.dc_reference = enDCReference, s.referenced_dc = fReferencedDC, s.init_phase = fInitPhase;
    s.sample_rate = nSampleRate, s.bits = nPhaseAccBits, s.mask = nPhaseAccMask, s.acc2phase = fAcc2Phase;
    s.freq_word = nFreqCtrlWord, s.init_word = nInitPhaseWord;
    s.sq_invert = sSquaredSinusoid.bInvert, s.sq_amplitude = sSquaredSinusoid.fAmplitude, s.sq_wave_dc = sSquaredSinusoid.fWaveDC;
    s.duty = sRectangular.fDutyRatio, s.duty_word = sRectangular.nDutyWord, s.rect_wave_dc = sRectangular.fWaveDC;
    s.rect_atten = sRectangular.fBLPeakAtten;
    s.width = sSawtooth.fWidth, s.width_word = sSawtooth.nWidthWord, s.saw_wave_dc = sSawtooth.fWaveDC, s.saw_atten = sSawtooth.fBLPeakAtten;
    s.raise_ratio = sTrapezoid.fRaiseRatio, s.fall_ratio = sTrapezoid.fFallRatio, s.trap_wave_dc = sTrapezoid.fWaveDC;
    s.trap_atten = sTrapezoid.fBLPeakAtten;
    for (int k = 0; k < 4; ++k)
        s.saw_coeffs[k] = sSawtooth.fCoeffs[k], s.points[k] = sTrapezoid.nPoints[k], s.trap_coeffs[k] = sTrapezoid.fCoeffs[k];
    s.pos_ratio = sPulse.fPosWidthRatio, s.neg_ratio = sPulse.fNegWidthRatio, s.pulse_wave_dc = sPulse.fWaveDC, s.pulse_atten = sPulse.fBLPeakAtten;
    for (int k = 0; k < 3; ++k)
        s.train[k] = sPulse.nTrainPoints[k];
    s.par_invert = sParabolic.bInvert, s.par_amplitude = sParabolic.fAmplitude, s.par_width = sParabolic.fWidth;
    s.par_word = sParabolic.nWidthWord, s.par_wave_dc = sParabolic.fWaveDC, s.par_atten = sParabolic.fBLPeakAtten;
    s.oversampling = uint32_t(nOversampling), s.over_mode = enOverMode, s.freq_word_over = nFreqCtrlWord_Over;
    s.sync = 1, s.phase_known = 1, s.phase = nPhaseAcc;

    mi_oscillator_settings_update(&s);

    nPhaseAccMask = s.mask, fAcc2Phase = s.acc2phase, nFreqCtrlWord = s.freq_word, nInitPhaseWord = s.init_word, nPhaseAcc = s.phase;
    fReferencedDC = s.referenced_dc;
    sSquaredSinusoid.fAmplitude = s.sq_amplitude, sSquaredSinusoid.fWaveDC = s.sq_wave_dc;
    sRectangular.nDutyWord = s.duty_word, sRectangular.fWaveDC = s.rect_wave_dc, sRectangular.fBLPeakAtten = s.rect_atten;
    sSawtooth.nWidthWord = s.width_word, sSawtooth.fWaveDC = s.saw_wave_dc, sSawtooth.fBLPeakAtten = s.saw_atten;
    sTrapezoid.fWaveDC = s.trap_wave_dc, sTrapezoid.fBLPeakAtten = s.trap_atten;
    for (int k = 0; k < 4; ++k)
        sSawtooth.fCoeffs[k] = s.saw_coeffs[k], sTrapezoid.nPoints[k] = s.points[k], sTrapezoid.fCoeffs[k] = s.trap_coeffs[k];
    for (int k = 0; k < 3; ++k)
        sPulse.nTrainPoints[k] = s.train[k];
    sPulse.fWaveDC = s.pulse_wave_dc, sPulse.fBLPeakAtten = s.pulse_atten;
    sParabolic.fAmplitude = s.par_amplitude, sParabolic.nWidthWord = s.par_word, sParabolic.fWaveDC = s.par_wave_dc;
    sParabolic.fBLPeakAtten = s.par_atten;

    sOver.set_sample_rate(nSampleRate);                         // :343-351
    sOver.set_mode(enOverMode);
    if (sOver.modified())
        sOver.update_settings();
    sOverGetPeriods.set_sample_rate(nSampleRate);
    sOverGetPeriods.set_mode(enOverMode);
    if (sOverGetPeriods.modified())
        sOverGetPeriods.update_settings();

    nOversampling = sOver.get_oversampling();                   // :353-354
    nFreqCtrlWord_Over = nFreqCtrlWord / nOversampling;
    bSync = false;

    // what the bank is given: the members as they stand.  A rate that was never set stays size_t(-1) in the arithmetic above; the
    // bank would refuse to process, and the reference does not
    s.oversampling = uint32_t(nOversampling), s.freq_word_over = nFreqCtrlWord_Over;
    s.unset_rate_ok = 1;
    if (handle *h = of(pData))
    {
        h->given = s;
        h->built = true, h->any = false;                        // goes to the bank with the next call
    }
}

void Oscillator::do_process(Oversampler *os, float *dst, size_t count)      // :359-633, host dst
{
    handle *h = of(pData);
    (void)os;                                                   // the bank runs the band-limited functions through its own
    if (h == nullptr || count == 0 || !h->buf.reserve(count, 2))
        return;
    if (!h->built)                                              // init() after the last update_settings(): the same members again
    {
        bSync = true;
        update_settings();
    }
    if (!hand_over(h, nPhaseAcc))
        return;
    if (mi_oscillator_bank_process(h->bank, h->buf.row(0), nullptr, count, h->buf.capacity(), h->buf.capacity(), MI_OSC_OVERWRITE, nullptr) != MI_OK)
        return;
    const bool over = enFunction >= FG_BL_RECTANGULAR;
    const phacc_t n = phacc_t(over ? nOversampling * count : count), w = over ? nFreqCtrlWord_Over : nFreqCtrlWord;
    nPhaseAcc = (nPhaseAcc + n * w) & nPhaseAccMask;            // what the advance kernel leaves on the device
    h->acc = nPhaseAcc;
    h->buf.down(dst, 0, count);
}

void Oscillator::get_periods(float *dst, size_t periods, size_t periodsSkip, size_t samples)   // :635-689
{
    // the bank's: the reference's loop on the host, every fill a launch from a phase of its own through an oversampler of its
    // own (sOverGetPeriods' part), the picks gathered on the device.  nPhaseAcc stays (:637, :688).  A period that is not positive
    // and finite is refused there, and nothing is written.
    handle *h = of(pData);
    if (h == nullptr || samples == 0 || !hand_over(h, nPhaseAcc) || !h->buf.reserve(samples, 2))
        return;
    if (mi_oscillator_bank_get_periods(h->bank, 0, h->buf.row(0), periods, periodsSkip, samples, nullptr) != MI_OK)
        return;
    h->buf.down(dst, 0, samples);
}

void Oscillator::process_add(float *dst, const float *src, size_t count)       // :691-710
{
    update_settings();
    std::vector<float> synth(count);
    do_process(&sOver, synth.data(), count);
    for (size_t i = 0; i < count; ++i)
        dst[i] = ((src != NULL) ? src[i] : 0.0f) + synth[i];    // copy or fill_zero, then add2
}

void Oscillator::process_mul(float *dst, const float *src, size_t count)       // :712-731
{
    update_settings();
    std::vector<float> synth(count);
    do_process(&sOver, synth.data(), count);
    for (size_t i = 0; i < count; ++i)
        dst[i] = ((src != NULL) ? src[i] : 0.0f) * synth[i];    // copy or fill_zero, then mul2
}

void Oscillator::process_overwrite(float *dst, size_t count)                   // :733-747
{
    update_settings();
    do_process(&sOver, dst, count);
}

void Oscillator::set_phase(float phase)                         // :749-757
{
    if (fInitPhase == phase)
        return;
    fInitPhase = phase;
    bSync = true;
}

float Oscillator::get_exact_phase() const                       // :759-763
{
    double x = (nPhaseAccMask + 1.0);
    return round(x * fInitPhase * 0.5f * M_1_PI) * (2.0 * M_PI / x);
}

void Oscillator::set_dc_offset(float dcOffset)                  // :765-771
{
    if (fDCOffset == dcOffset)
        return;
    fDCOffset = dcOffset;
}

void Oscillator::set_dc_reference(dc_reference_t dcReference)   // :773-777
{
    enDCReference = dcReference;
    bSync = true;
}

void Oscillator::set_squared_sinusoid_inversion(bool invert)    // :779-786
{
    if (sSquaredSinusoid.bInvert == invert)
        return;
    sSquaredSinusoid.bInvert = invert;
    bSync = true;
}

void Oscillator::set_parabolic_inversion(bool invert)           // :788-795
{
    if (sParabolic.bInvert == invert)
        return;
    sParabolic.bInvert = invert;
    bSync = true;
}

// the ratios' clamps and refusals are mi_oscillator_settings_set's, on a scratch record
#define OSC_RATIO_SETTER(setter, a, b, ...) \
    mi_oscillator_settings_t s; \
    mi_oscillator_settings_init(&s); \
    s.sync = 0; \
    __VA_ARGS__; \
    mi_oscillator_settings_set(&s, setter, a, b)

void Oscillator::set_duty_ratio(float dutyRatio)                // :797-804
{
    OSC_RATIO_SETTER(MI_OSC_SET_DUTY_RATIO, dutyRatio, 0, s.duty = sRectangular.fDutyRatio);
    sRectangular.fDutyRatio = s.duty;
    bSync = bSync || s.sync;
}

void Oscillator::set_width(float width)                         // :806-817
{
    OSC_RATIO_SETTER(MI_OSC_SET_WIDTH, width, 0, s.width = sSawtooth.fWidth);
    sSawtooth.fWidth = s.width;
    bSync = bSync || s.sync;
}

void Oscillator::set_trapezoid_ratios(float raise, float fall)  // :819-838
{
    OSC_RATIO_SETTER(MI_OSC_SET_TRAPEZOID_RATIOS, raise, fall, s.raise_ratio = sTrapezoid.fRaiseRatio, s.fall_ratio = sTrapezoid.fFallRatio);
    sTrapezoid.fRaiseRatio = s.raise_ratio, sTrapezoid.fFallRatio = s.fall_ratio;
    bSync = bSync || s.sync;
}

void Oscillator::set_pulsetrain_ratios(float posWidthRatio, float negWidthRatio)   // :840-858
{
    OSC_RATIO_SETTER(MI_OSC_SET_PULSETRAIN_RATIOS, posWidthRatio, negWidthRatio, s.pos_ratio = sPulse.fPosWidthRatio, s.neg_ratio = sPulse.fNegWidthRatio);
    sPulse.fPosWidthRatio = s.pos_ratio, sPulse.fNegWidthRatio = s.neg_ratio;
    bSync = bSync || s.sync;
}

void Oscillator::set_parabolic_width(float width)               // :860-872
{
    OSC_RATIO_SETTER(MI_OSC_SET_PARABOLIC_WIDTH, width, 0, s.par_width = sParabolic.fWidth);
    sParabolic.fWidth = s.par_width;
    bSync = bSync || s.sync;
}
#undef OSC_RATIO_SETTER

void Oscillator::set_oversampler_mode(over_mode_t mode)         // :874-881
{
    if (mode == enOverMode)
        return;
    enOverMode = mode;
    bSync = true;
}

void Oscillator::set_amplitude(float amplitude)                 // :883-890
{
    if (fAmplitude == amplitude)
        return;
    fAmplitude = amplitude;
    bSync = true;
}

void Oscillator::dump(IStateDumper *v) const                    // :892-983
{
    v->write("enFunction", enFunction);
    v->write("fAmplitude", fAmplitude);
    v->write("fFrequency", fFrequency);
    v->write("fDCOffset", fDCOffset);
    v->write("enDCReference", enDCReference);
    v->write("fReferencedDC", fReferencedDC);
    v->write("fInitPhase", fInitPhase);

    v->write("nSampleRate", nSampleRate);
    v->write("nPhaseAcc", nPhaseAcc);
    v->write("nPhaseAccBits", nPhaseAccBits);
    v->write("nPhaseAccMaxBits", nPhaseAccMaxBits);
    v->write("nPhaseAccMask", nPhaseAccMask);
    v->write("fAcc2Phase", fAcc2Phase);

    v->write("nFreqCtrlWord", nFreqCtrlWord);
    v->write("nInitPhaseWord", nInitPhaseWord);

    v->begin_object("sSquaredSinusoid", &sSquaredSinusoid, sizeof(sSquaredSinusoid));
    {
        v->write("bInvert", sSquaredSinusoid.bInvert);
        v->write("fAmplitude", sSquaredSinusoid.fAmplitude);
        v->write("fWaveDC", sSquaredSinusoid.fWaveDC);
    }
    v->end_object();

    v->begin_object("sRectangular", &sRectangular, sizeof(sRectangular));
    {
        v->write("fDutyRatio", sRectangular.fDutyRatio);
        v->write("nDutyWord", sRectangular.nDutyWord);
        v->write("fWaveDC", sRectangular.fWaveDC);
        v->write("fBLPeakAtten", sRectangular.fBLPeakAtten);
    }
    v->end_object();

    v->begin_object("sSawtooth", &sSawtooth, sizeof(sSawtooth));
    {
        v->write("fWidth", sSawtooth.fWidth);
        v->write("nWidthWord", sSawtooth.nWidthWord);
        v->writev("fCoeffs", sSawtooth.fCoeffs, 4);
        v->write("fWaveDC", sSawtooth.fWaveDC);
        v->write("fBLPeakAtten", sSawtooth.fBLPeakAtten);
    }
    v->end_object();

    v->begin_object("sTrapezoid", &sTrapezoid, sizeof(sTrapezoid));
    {
        v->write("fRaiseRatio", sTrapezoid.fRaiseRatio);
        v->write("fFallRatio", sTrapezoid.fFallRatio);
        v->writev("nPoints", sTrapezoid.nPoints, 4);
        v->writev("fCoeffs", sTrapezoid.fCoeffs, 4);
        v->write("fWaveDC", sTrapezoid.fWaveDC);
        v->write("fBLPeakAtten", sTrapezoid.fBLPeakAtten);
    }
    v->end_object();

    v->begin_object("sPulse", &sPulse, sizeof(sPulse));
    {
        v->write("fPosWidthRatio", sPulse.fPosWidthRatio);
        v->write("fNegWidthRatio", sPulse.fNegWidthRatio);
        v->writev("nTrainPoints", sPulse.nTrainPoints, 3);
        v->write("fWaveDC", sPulse.fWaveDC);
        v->write("fBLPeakAtten", sPulse.fBLPeakAtten);
    }
    v->end_object();

    v->begin_object("sParabolic", &sParabolic, sizeof(sParabolic));
    {
        v->write("bInvert", sParabolic.bInvert);
        v->write("fAmplitude", sParabolic.fAmplitude);
        v->write("fWidth", sParabolic.fWidth);
        v->write("nWidthWord", sParabolic.nWidthWord);
        v->write("fWaveDC", sParabolic.fWaveDC);
        v->write("fBLPeakAtten", sParabolic.fBLPeakAtten);
    }
    v->end_object();

    v->write("vProcessBuffer", vProcessBuffer);
    v->write("vSynthBuffer", vSynthBuffer);
    v->write("pData", pData);

    v->write_object("sOver", &sOver);
    v->write_object("sOverGetPeriods", &sOverGetPeriods);

    v->write("nOversampling", nOversampling);
    v->write("enOverMode", enOverMode);
    v->write("nFreqCtrlWord_Over", nFreqCtrlWord_Over);
    v->write("bSync", bSync);
}

} // namespace dspu
} // namespace lsp
