// lsp::dspu::ADSREnvelope on the GPU library (one envelope, host pointers; the device-resident form for many channels is
// mi_adsr_bank_*).  The object's bytes are the reference's.  The setters and update_settings() are host work on the object's
// fields (the designer is mi_adsr_settings_update, no device); the scalar process(float) is control-rate and evaluates on the host
// from the designed curves, with the device's rule for expf in EXP segments; the four array methods stage the caller's rows on
// the device and run the bank's kernel through a bank of one channel that the object makes at its first such call.  pGenerator
// names the curve's generator as in the reference; the kernel branches on enFunction.
#ifndef MI_LSP_PLUG_IN_DSP_UNITS_UTIL_ADSRENVELOPE_H_
#define MI_LSP_PLUG_IN_DSP_UNITS_UTIL_ADSRENVELOPE_H_

#include <stddef.h>
#include <stdint.h>

#include <lsp-plug.in/dsp-units/version.h>
#include <lsp-plug.in/dsp-units/iface/IStateDumper.h>

namespace lsp
{
    namespace dspu
    {
        class LSP_DSP_UNITS_PUBLIC ADSREnvelope
        {
            public:
                enum function_t { ADSR_NONE, ADSR_LINE, ADSR_LINE2, ADSR_CUBIC, ADSR_QUADRO, ADSR_EXP };

            protected:
                enum flags_t { F_USE_HOLD = 1 << 0, F_USE_BREAK = 1 << 1, F_RECONFIGURE = 1 << 2 };
                enum part_t { P_ATTACK, P_DECAY, P_SLOPE, P_RELEASE, P_TOTAL };

                struct gen_none_t       { float fT, fK, fB; };
                struct gen_line_t       { float fT2, fK1, fB1, fK2, fB2; };
                struct gen_hermite_t    { float fT0, fK[5]; };
                struct gen_exp_t        { float fT0, fKT, fA[2], fB[2]; };
                union gen_params_t
                {
                    gen_none_t      sNone;
                    gen_line_t      sLine;
                    gen_hermite_t   sHermite;
                    gen_exp_t       sExp;
                };
                typedef float (*generator_t)(float t, const gen_params_t *params);
                struct curve_t
                {
                    float           fTime;
                    float           fCurve;
                    function_t      enFunction;
                    generator_t     pGenerator;
                    gen_params_t    sParams;
                };

            protected:
                curve_t             vCurve[P_TOTAL];
                float               fHoldTime;
                float               fBreakLevel;
                float               fSustainLevel;
                uint32_t            nFlags;

            protected:
                static float        none_generator(float t, const gen_params_t *params);
                static float        line_generator(float t, const gen_params_t *params);
                static float        cubic_generator(float t, const gen_params_t *params);
                static float        quadro_generator(float t, const gen_params_t *params);
                static float        exp_generator(float t, const gen_params_t *params);

            protected:
                void                set_param(float &param, float value);
                void                set_function(function_t &func, function_t value);
                void                set_flag(uint32_t flag, bool set);
                void                set_curve(part_t part, float time, float curve, function_t func);
                float               do_process(float value);

            public:
                ADSREnvelope();
                ~ADSREnvelope();
                ADSREnvelope(const ADSREnvelope &) = delete;
                ADSREnvelope(ADSREnvelope &&) = delete;
                ADSREnvelope & operator = (const ADSREnvelope &) = delete;
                ADSREnvelope & operator = (ADSREnvelope &&) = delete;

                void                construct();
                void                destroy();

            public:
                // values are clamped to [0, 1]; a NaN is refused (the value stays)
                inline void         set_attack_time(float value)        { set_param(vCurve[P_ATTACK].fTime, value); }
                inline void         set_hold_time(float value)          { set_param(fHoldTime, value); }
                inline void         set_decay_time(float value)         { set_param(vCurve[P_DECAY].fTime, value); }
                inline void         set_slope_time(float value)         { set_param(vCurve[P_SLOPE].fTime, value); }
                inline void         set_relese_time(float value)        { set_param(vCurve[P_RELEASE].fTime, value); }

                inline void         set_attack_curve(float value)       { set_param(vCurve[P_ATTACK].fCurve, value); }
                inline void         set_decay_curve(float value)        { set_param(vCurve[P_DECAY].fCurve, value); }
                inline void         set_slope_curve(float value)        { set_param(vCurve[P_SLOPE].fCurve, value); }
                inline void         set_release_curve(float value)      { set_param(vCurve[P_RELEASE].fCurve, value); }

                inline void         set_attack_function(function_t f)   { set_function(vCurve[P_ATTACK].enFunction, f); }
                inline void         set_decay_function(function_t f)    { set_function(vCurve[P_DECAY].enFunction, f); }
                inline void         set_slope_function(function_t f)    { set_function(vCurve[P_SLOPE].enFunction, f); }
                inline void         set_release_function(function_t f)  { set_function(vCurve[P_RELEASE].enFunction, f); }

                inline void         set_break_level(float value)        { set_param(fBreakLevel, value); }
                inline void         set_sustain_level(float value)      { set_param(fSustainLevel, value); }

                inline void         set_hold_enabled(bool enabled)      { set_flag(F_USE_HOLD, enabled); }
                inline void         set_break_enabled(bool enabled)     { set_flag(F_USE_BREAK, enabled); }

                inline void         set_attack(float time, float curve, function_t func)    { set_curve(P_ATTACK, time, curve, func); }
                void                set_hold(float time, bool enabled);
                inline void         set_decay(float time, float curve, function_t func)     { set_curve(P_DECAY, time, curve, func); }
                void                set_break(float level, bool enabled);
                inline void         set_slope(float time, float curve, function_t func)     { set_curve(P_SLOPE, time, curve, func); }
                inline void         set_release(float time, float curve, function_t func)   { set_curve(P_RELEASE, time, curve, func); }

                inline float        attack_time() const                 { return vCurve[P_ATTACK].fTime; }
                inline float        hold_time() const                   { return fHoldTime; }
                inline float        decay_time() const                  { return vCurve[P_DECAY].fTime; }
                inline float        slope_time() const                  { return vCurve[P_SLOPE].fTime; }
                inline float        release_time() const                { return vCurve[P_RELEASE].fTime; }

                inline float        attack_curve() const                { return vCurve[P_ATTACK].fCurve; }
                inline float        decay_curve() const                 { return vCurve[P_DECAY].fCurve; }
                inline float        slope_curve() const                 { return vCurve[P_SLOPE].fCurve; }
                inline float        release_curve() const               { return vCurve[P_RELEASE].fCurve; }

                inline function_t   attack_function() const             { return vCurve[P_ATTACK].enFunction; }
                inline function_t   decay_function() const              { return vCurve[P_DECAY].enFunction; }
                inline function_t   slope_function() const              { return vCurve[P_SLOPE].enFunction; }
                inline function_t   release_function() const            { return vCurve[P_RELEASE].enFunction; }

                inline float        break_level() const                 { return fBreakLevel; }
                inline float        sustain_level() const               { return fSustainLevel; }

                inline float        hold_enabled() const                { return nFlags & F_USE_HOLD; }
                inline float        break_enabled() const               { return nFlags & F_USE_BREAK; }

            public:
                void                update_settings();

                // the envelope at one normalized time, on the host; 0 outside (0, 1)
                float               process(float value);

                // host rows, staged on the device: dst[i] = the envelope at src[i]; dst[i] *= it
                void                process(float *dst, const float *src, size_t count);
                void                process_mul(float *dst, const float *src, size_t count);

                // the envelope at start + i * step: stored; applied to dst in place; applied to src and stored
                void                generate(float *dst, float start, float step, size_t count);
                void                generate_mul(float *dst, float start, float step, size_t count);
                void                generate_mul(float *dst, const float *src, float start, float step, size_t count);

                void                dump(IStateDumper *v) const;
        };
    } /* namespace dspu */
} /* namespace lsp */

#endif /* MI_LSP_PLUG_IN_DSP_UNITS_UTIL_ADSRENVELOPE_H_ */
