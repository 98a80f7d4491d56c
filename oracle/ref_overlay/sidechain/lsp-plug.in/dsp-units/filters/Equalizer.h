// STAND-IN placed ahead of the reference's <lsp-plug.in/dsp-units/filters/Equalizer.h> for oracle/_ref/sidechain_ref only:
// Sidechain.cpp names the pre-equalizer's process() and reset(), and the real class would pull the whole filter tree in.  No
// recorded case sets a pre-equalizer (pPreEq stays NULL), so neither is ever called; both abort if they are.
#ifndef ORACLE_REF_OVERLAY_SIDECHAIN_EQUALIZER_H_
#define ORACLE_REF_OVERLAY_SIDECHAIN_EQUALIZER_H_

#include <cstdlib>
#include <lsp-plug.in/common/types.h>
#include <lsp-plug.in/dsp/dsp.h>                 // Sidechain.cpp gets dsp:: through this header

namespace lsp
{
    namespace dspu
    {
        class Equalizer
        {
            public:
                void process(float *, const float *, size_t)    { abort(); }
                void reset()                                    { abort(); }
        };
    }
}

#endif
