// lsp::dspu::MLS on the GPU library (one register, host pointers; the device-resident form for many channels is mi_mls_bank_*),
// with mls_t = uint64_t: the reference's LP64 build.  The members are the state: update_settings() is mi_mls_settings_update on
// them, process_single() runs the register on the host; process_add / process_mul / process_overwrite hand nBits and nState to a
// bank of one channel, stage the caller's rows on the device, run the bank's kernels and take nState back
// (mi_mls_bank_get_state), so single samples and rows mix freely and stay one stream.  Every sample has the reference's bits.
#ifndef MI_LSP_PLUG_IN_DSP_UNITS_NOISE_MLS_H_
#define MI_LSP_PLUG_IN_DSP_UNITS_NOISE_MLS_H_

#include <lsp-plug.in/dsp-units/version.h>
#include <lsp-plug.in/dsp-units/iface/IStateDumper.h>

namespace lsp
{
    namespace dspu
    {
        class LSP_DSP_UNITS_PUBLIC MLS
        {
            public:
                typedef uint64_t mls_t;                         // umword_t of a 64-bit build

            // Binary layout: data members and their order as in the reference class, 72 bytes on LP64 (tests/cpp/noise_layout.cpp).
            private:
                size_t      nBits;
                size_t      nFeedbackBit;
                mls_t       nFeedbackMask;
                mls_t       nActiveMask;
                mls_t       nTapsMask;
                mls_t       nOutputMask;
                mls_t       nState;

                float       fAmplitude;
                float       fOffset;

                bool        bSync;

            private:
                void run(float *dst, const float *src, size_t count, unsigned op);

            public:
                explicit MLS();
                MLS(const MLS &) = delete;
                MLS(MLS &&) = delete;
                ~MLS();

                MLS & operator = (const MLS &) = delete;
                MLS & operator = (MLS &&) = delete;

                void construct();
                void destroy();

            protected:
                mls_t xor_gate(mls_t value);
                mls_t progress();
                void update_settings();

            public:
                size_t maximum_number_of_bits() const;
                bool needs_update() const;

                void set_n_bits(size_t nbits);
                void set_state(mls_t targetstate);
                void set_amplitude(float amplitude);
                void set_offset(float offset);

                mls_t get_period() const;                       // all ones from 64 bits on (mi_dspu.h)

                float process_single();
                void process_add(float *dst, const float *src, size_t count);
                void process_mul(float *dst, const float *src, size_t count);
                void process_overwrite(float *dst, size_t count);

                void dump(IStateDumper *v) const;

            friend class Velvet;
        };
    }
}

#endif
