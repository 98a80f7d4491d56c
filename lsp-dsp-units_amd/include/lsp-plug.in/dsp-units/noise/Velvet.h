// lsp::dspu::Velvet on the GPU library (one generator, host pointers; the device-resident form for many channels is
// mi_velvet_bank_*).  The members are the state: process_add / process_mul / process_overwrite hand sRandomizer, sMLS and the
// settings to a bank of one channel (mi_velvet_bank_set_state and the setters), stage the caller's rows on the device, run the
// bank's kernel and take both states back (mi_velvet_bank_get_state).  Every sample and every state word has the reference's
// bits; a call is the reference's call: one segment for process_overwrite and process_add(dst, NULL, n), segments of 256 with a
// source, a zero fill and no draw for process_mul(dst, NULL, n).
// Where the reference's behaviour is undefined: before init() the rows stay untouched (Randomizer.h); so does a call without a
// source of more than 2^24 samples (mi_dspu.h); a window width that is not finite is not taken (the width stays as it is).
#ifndef MI_LSP_PLUG_IN_DSP_UNITS_NOISE_VELVET_H_
#define MI_LSP_PLUG_IN_DSP_UNITS_NOISE_VELVET_H_

#include <lsp-plug.in/dsp-units/version.h>
#include <lsp-plug.in/dsp-units/util/Randomizer.h>
#include <lsp-plug.in/dsp-units/noise/MLS.h>
#include <lsp-plug.in/dsp-units/iface/IStateDumper.h>

namespace lsp
{
    namespace dspu
    {
        enum vn_core_t
        {
            VN_CORE_MLS,        // spikes from the MLS: OVN, OVNA and ARN, not crushed
            VN_CORE_LCG
        };

        enum vn_velvet_type_t
        {
            VN_VELVET_OVN,      // one spike per window
            VN_VELVET_OVNA,     // ... whose place may reach into the next window
            VN_VELVET_ARN,      // additive random steps between spikes
            VN_VELVET_TRN       // dense: a rounded uniform draw per sample
        };

        class LSP_DSP_UNITS_PUBLIC Velvet
        {
            protected:
                typedef struct crush_t
                {
                    bool    bCrush;
                    float   fCrushProb;
                } crush_t;

            // Binary layout: data members and their order as in the reference class, 176 bytes on LP64 (tests/cpp/velvet_layout.cpp).
            private:
                Randomizer          sRandomizer;

                MLS                 sMLS;

                vn_core_t           enCore;

                vn_velvet_type_t    enVelvetType;

                crush_t             sCrushParams;

                float               fWindowWidth;
                float               fARNdelta;
                float               fAmplitude;
                float               fOffset;

            private:
                void run(float *dst, const float *src, size_t count, unsigned op);

            public:
                explicit Velvet();
                Velvet(const Velvet &) = delete;
                Velvet(Velvet &&) = delete;
                ~Velvet();

                void construct();
                void destroy();

                Velvet & operator = (const Velvet &) = delete;
                Velvet & operator = (Velvet &&) = delete;

            protected:
                float get_random_value();
                float get_spike();
                float get_crushed_spike();

            public:
                void init(uint32_t randseed, uint8_t mlsnbits, MLS::mls_t mlsseed);
                void init();                                    // the Randomizer's seed is the host clock; the MLS keeps what it has

                void set_core_type(vn_core_t core);
                void set_velvet_type(vn_velvet_type_t type);
                void set_velvet_window_width(float width);      // clamped up to 2
                void set_delta_value(float delta);              // clamped to 0 .. 1
                void set_amplitude(float amplitude);
                void set_offset(float offset);
                void set_crush(bool crush);
                void set_crush_probability(float prob);         // clamped to 0 .. 1

                void process_add(float *dst, const float *src, size_t count);
                void process_mul(float *dst, const float *src, size_t count);
                void process_overwrite(float *dst, size_t count);

                void dump(IStateDumper *v) const;
        };
    }
}

#endif
