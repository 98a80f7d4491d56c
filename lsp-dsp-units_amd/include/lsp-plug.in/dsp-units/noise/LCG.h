// lsp::dspu::LCG on the GPU library (one generator, host pointers; the device-resident form for many channels is mi_lcg_bank_*).
// The members are the state: process_single() runs on the host with the reference's arithmetic; process_add / process_mul /
// process_overwrite hand the members to a bank of one channel (mi_lcg_bank_set_state and the setters), stage the caller's rows on
// the device, run the bank's kernel and take the Randomizer back (mi_lcg_bank_get_state), so single samples and rows mix freely
// and stay one stream.  Uniform and triangular rows have the reference's bits; in exponential and Gaussian rows expf, logf and
// cosf are the float64 function rounded once, in single samples the host C library's (mi_dspu.h).
// Where the reference's behaviour is undefined: before init() process_add / _mul / _overwrite leave the rows untouched and
// process_single() works on draws of 0.0f (Randomizer.h); a distribution above LCG_GAUSSIAN is uniform, as the reference's
// default: has it.
#ifndef MI_LSP_PLUG_IN_DSP_UNITS_NOISE_LCG_H_
#define MI_LSP_PLUG_IN_DSP_UNITS_NOISE_LCG_H_

#include <lsp-plug.in/dsp-units/version.h>
#include <lsp-plug.in/dsp-units/util/Randomizer.h>
#include <lsp-plug.in/dsp-units/iface/IStateDumper.h>

namespace lsp
{
    namespace dspu
    {
        enum lcg_dist_t
        {
            LCG_UNIFORM,        // uniform over [-1, 1), x fAmplitude + fOffset
            LCG_EXPONENTIAL,    // double sided exponential over [-1, 1], x fAmplitude + fOffset
            LCG_TRIANGULAR,     // triangular over [-1, 1], x fAmplitude + fOffset
            LCG_GAUSSIAN        // Gaussian of mean 0 and standard deviation 1, x fAmplitude + fOffset
        };

        class LSP_DSP_UNITS_PUBLIC LCG
        {
            // Binary layout: data members and their order as in the reference class, 88 bytes on LP64 (tests/cpp/noise_layout.cpp).
            private:
                lcg_dist_t  enDistribution;

                float       fAmplitude;
                float       fOffset;

                Randomizer  sRand;

            private:
                void run(float *dst, const float *src, size_t count, unsigned op);

            public:
                explicit LCG();
                LCG(const LCG &) = delete;
                LCG(LCG &&) = delete;
                ~LCG();

                LCG & operator = (const LCG &) = delete;
                LCG & operator = (LCG &) = delete;

                void construct();
                void destroy();

            public:
                void init(uint32_t seed);
                void init();

                inline void set_distribution(lcg_dist_t dist)   { enDistribution = dist; }

                inline void set_amplitude(float amplitude)
                {
                    if (amplitude == fAmplitude)
                        return;
                    fAmplitude = amplitude;
                }

                inline void set_offset(float offset)
                {
                    if (offset == fOffset)
                        return;
                    fOffset = offset;
                }

                float process_single();
                void process_add(float *dst, const float *src, size_t count);
                void process_mul(float *dst, const float *src, size_t count);
                void process_overwrite(float *dst, size_t count);

                void dump(IStateDumper *v) const;
        };
    }
}

#endif
