// lsp::dspu::Randomizer on the host (reference: util/Randomizer.h, src/main/util/Randomizer.cpp): random() is one float per call,
// so the class is plain host C++ with the reference's arithmetic and its C library's expf, logf and cosf; the device form of the
// same generators is csrc/randomizer_device.h under mi_lcg_bank_*.  init(seed) is mi_lcg_seed_words.
// Where the reference's behaviour is undefined: a Randomizer that was never init()ed has nBufID == size_t(-1) and the reference
// indexes vRandom[-1]; here the draw is 0.0f then (random() shapes it as any other) and nothing changes.
#ifndef MI_LSP_PLUG_IN_DSP_UNITS_UTIL_RANDOMIZER_H_
#define MI_LSP_PLUG_IN_DSP_UNITS_UTIL_RANDOMIZER_H_

#include <lsp-plug.in/dsp-units/version.h>
#include <lsp-plug.in/dsp-units/iface/IStateDumper.h>

namespace lsp
{
    namespace dspu
    {
        enum random_function_t
        {
            RND_LINEAR,     // uniform over [0, 1]
            RND_EXP,        // decaying exponential over [0, 1]
            RND_TRIANGLE,   // triangle over [0, 1]
            RND_GAUSSIAN,   // Gaussian of mean 0 and standard deviation 1
            RND_MAX
        };

        class LSP_DSP_UNITS_PUBLIC Randomizer
        {
            // Binary layout: data members and their order as in the reference class, 72 bytes on LP64 (tests/cpp/noise_layout.cpp).
            private:
                static const uint32_t vMul1[];
                static const uint32_t vMul2[];
                static const uint32_t vAdders[];

                typedef struct randgen_t
                {
                    uint32_t    vLast;
                    uint32_t    vMul1;
                    uint32_t    vMul2;
                    uint32_t    vAdd;
                } randgen_t;

                randgen_t   vRandom[4];
                size_t      nBufID;

            protected:
                float generate_linear();

            public:
                explicit Randomizer();
                Randomizer(const Randomizer &) = delete;
                Randomizer(Randomizer &&) = delete;
                ~Randomizer();

                Randomizer &operator = (const Randomizer &) = delete;
                Randomizer &operator = (Randomizer &&) = delete;

                void construct();
                void destroy();

                void init(uint32_t seed);
                void init();                                    // the seed is the host clock

            public:
                float random(random_function_t func = RND_LINEAR);

                void dump(IStateDumper *v) const;

            friend class LCG;
            friend class Velvet;
        };
    }
}

#endif
