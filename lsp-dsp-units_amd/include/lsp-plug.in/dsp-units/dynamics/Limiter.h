// lsp::dspu::Limiter on the GPU library (one limiter, host pointers; the device-resident form for many channels is
// mi_limiter_bank_*).  The setters, update_settings() and dump() are host arithmetic on the object's fields; init() makes a
// bank of one channel beside the object and process() runs on it: the gain buffer lives on the device, so vGainBuf, vTmpBuf
// and vData stay NULL, and nHead and sALR.fEnvelope are read back after every call.  Inputs are finite: NaN is out of scope.
//
// Unlike the reference: init() refuses a maximum look-ahead above MI_LIMITER_MAX_LOOKAHEAD samples and set_sample_rate() a rate
// above init()'s; the patch loop of a chunk of n samples ends after 2 n patches (see mi_limiter_bank in mi_dspu.h); process()
// does not read back its own output where gain == sc: the arithmetic is the out-of-place call's.
#ifndef MI_LSP_PLUG_IN_DSP_UNITS_DYNAMICS_LIMITER_H_
#define MI_LSP_PLUG_IN_DSP_UNITS_DYNAMICS_LIMITER_H_

#include <lsp-plug.in/dsp-units/version.h>
#include <lsp-plug.in/dsp-units/iface/IStateDumper.h>

#include <sys/types.h>

#define LIMITER_PEAKS_MAX           32

namespace lsp
{
    namespace dspu
    {
        enum limiter_mode_t
        {
            LM_HERM_THIN, LM_HERM_WIDE, LM_HERM_TAIL, LM_HERM_DUCK,
            LM_EXP_THIN,  LM_EXP_WIDE,  LM_EXP_TAIL,  LM_EXP_DUCK,
            LM_LINE_THIN, LM_LINE_WIDE, LM_LINE_TAIL, LM_LINE_DUCK
        };

        class LSP_DSP_UNITS_PUBLIC Limiter
        {
            // Binary layout: data members and their order as in the reference class
            // (include/lsp-plug.in/dsp-units/dynamics/Limiter.h:57-147 of lsp-dsp-units), 216 bytes.  There is no spare member:
            // the GPU bank is kept beside the object, keyed by its address, and goes away in destroy().
            protected:
                enum update_t
                {
                    UP_SR = 1 << 0, UP_LK = 1 << 1, UP_MODE = 1 << 2, UP_OTHER = 1 << 3, UP_THRESH = 1 << 4, UP_ALR = 1 << 5,
                    UP_ALL = UP_SR | UP_LK | UP_MODE | UP_OTHER | UP_THRESH | UP_ALR
                };

                typedef struct alr_t
                {
                    float       fKS, fKE, fGain, fTauAttack, fTauRelease, vHermite[3], fAttack, fRelease, fEnvelope, fKnee;
                    bool        bEnable;
                } alr_t;

                typedef struct sat_t  { int32_t nAttack, nPlane, nRelease, nMiddle; float vAttack[4], vRelease[4]; } sat_t;
                typedef struct exp_t  { int32_t nAttack, nPlane, nRelease, nMiddle; float vAttack[4], vRelease[4]; } exp_t;
                typedef struct line_t { int32_t nAttack, nPlane, nRelease, nMiddle; float vAttack[2], vRelease[2]; } line_t;

            protected:
                float       fThreshold;
                float       fReqThreshold;
                float       fLookahead;
                float       fMaxLookahead;
                float       fAttack;
                float       fRelease;
                float       fKnee;
                size_t      nMaxLookahead;
                size_t      nLookahead;
                size_t      nHead;
                size_t      nMaxSampleRate;
                size_t      nSampleRate;
                size_t      nUpdate;
                size_t      nMode;
                alr_t       sALR;

                float      *vGainBuf;
                float      *vTmpBuf;
                uint8_t    *vData;

                union
                {
                    sat_t       sSat;
                    exp_t       sExp;
                    line_t      sLine;
                };

            public:
                explicit Limiter();
                Limiter(const Limiter &) = delete;
                Limiter(Limiter &&) = delete;
                ~Limiter();

                Limiter & operator = (const Limiter &) = delete;
                Limiter & operator = (Limiter &&) = delete;

                void        construct();            // valid on raw (e.g. zeroed) memory
                void        destroy();

            public:
                bool                init(size_t max_sr, float max_lookahead);       // ms
                inline bool         modified() const            { return nUpdate != 0; }
                void                update_settings();

                inline limiter_mode_t get_mode() const          { return limiter_mode_t(nMode); }
                void                set_mode(limiter_mode_t mode);
                void                set_sample_rate(size_t sr);
                inline size_t       sample_rate() const         { return nSampleRate; }
                inline size_t       max_sample_rate() const     { return nMaxSampleRate; }

                inline float        get_threshold() const       { return fReqThreshold; }
                float               set_threshold(float thresh, bool immediate);
                inline float        get_attack() const          { return fAttack; }
                float               set_attack(float attack);                       // ms
                inline float        get_release() const         { return fRelease; }
                float               set_release(float release);                     // ms
                inline float        get_lookahead() const       { return fLookahead; }
                float               set_lookahead(float lk_ahead);                  // ms, limited to init()'s maximum
                inline size_t       max_latency() const         { return nMaxLookahead; }
                inline float        get_knee() const            { return fKnee; }
                float               set_knee(float knee);
                inline size_t       get_latency() const         { return nLookahead; }

                inline float        get_alr_attack() const      { return sALR.fAttack; }
                float               set_alr_attack(float attack);
                inline float        get_alr_release() const     { return sALR.fRelease; }
                float               set_alr_release(float attack);
                inline bool         get_alr() const             { return sALR.bEnable; }
                bool                set_alr(bool enable);
                float               set_alr_knee(float knee);                       // stored as 1 / knee above 1
                inline float        alr_knee() const            { return sALR.fKnee; }

                // gain: the gain for the VCA, sc: the sidechain signal; applies pending settings first
                void                process(float *gain, const float *sc, size_t samples);

                void                dump(IStateDumper *v) const;
        };
    }
}

#endif
