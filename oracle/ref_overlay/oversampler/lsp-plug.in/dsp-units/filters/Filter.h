// RECORDING STAND-IN placed ahead of the reference's <lsp-plug.in/dsp-units/filters/Filter.h> for oracle/_ref/oversampler_ref
// only.  The real filter is held to the biquad oracle by the Oversampler's own tests; what the recordings pin is what the
// Oversampler ASKS of it and when it clears it.  update(sr, fp) stores what it was asked and logs it, clear() logs a call,
// process() copies.  filter_params_t and the filter types are the reference's own (filters/common.h).
#ifndef ORACLE_REF_OVERLAY_OVERSAMPLER_FILTER_H_
#define ORACLE_REF_OVERLAY_OVERSAMPLER_FILTER_H_

#include <cstring>
#include <vector>
#include <lsp-plug.in/dsp-units/filters/common.h>

namespace lsp
{
    namespace dspu
    {
        struct filter_call_t { bool clear; size_t rate; filter_params_t fp; };
        extern std::vector<filter_call_t> filter_log;           // defined by the driver

        class FilterBank;
        class IStateDumper;

        class Filter
        {
            protected:
                filter_params_t     sParams;

            public:
                void construct()                    { memset(&sParams, 0, sizeof(sParams)); }
                bool init(FilterBank *)             { construct(); return true; }
                void destroy()                      { }
                void dump(IStateDumper *) const     { }
                void get_params(filter_params_t *fp) const  { *fp = sParams; }
                void clear()
                {
                    filter_call_t c;
                    c.clear = true; c.rate = 0; c.fp = sParams;
                    filter_log.push_back(c);
                }
                void update(size_t sr, const filter_params_t *fp)
                {
                    filter_call_t c;
                    sParams = *fp;
                    c.clear = false; c.rate = sr; c.fp = *fp;
                    filter_log.push_back(c);
                }
                void process(float *dst, const float *src, size_t count)
                {
                    if (dst != src)
                        memmove(dst, src, count * sizeof(float));
                }
        };
    }
}

#endif
