// lsp::dspu::interpolation on the GPU library's host side (mi_interpolation_* of mi_dspu.h): the two Hermite designs that
// ADSREnvelope's update_settings() calls (src/main/misc/interpolation.cpp:112-177 of the reference), float arguments with
// double intermediates as there.
#ifndef MI_LSP_PLUG_IN_DSP_UNITS_MISC_INTERPOLATION_H_
#define MI_LSP_PLUG_IN_DSP_UNITS_MISC_INTERPOLATION_H_

#include <lsp-plug.in/dsp-units/version.h>

namespace lsp
{
    namespace dspu
    {
        namespace interpolation
        {
            // y = p[0] x^3 + p[1] x^2 + p[2] x + p[3] through (x0, y0) and (x1, y1) with the slopes k0 and k1
            LSP_DSP_UNITS_PUBLIC void hermite_cubic(float *p, float x0, float y0, float k0, float x1, float y1, float k1);
            // y = p[0] x^4 + ... + p[4] through (x0, y0) and (x1, y1) with the slopes k0 and k1, and through (x2, y2)
            LSP_DSP_UNITS_PUBLIC void hermite_quadro(float *p, float x0, float y0, float k0, float x1, float y1, float k1, float x2, float y2);
        }
    }
}

#endif /* MI_LSP_PLUG_IN_DSP_UNITS_MISC_INTERPOLATION_H_ */
