/*
 * ORACLE -- test infrastructure only. Nothing under lsp-dsp-units_amd/ may
 * include, link or call this file; tests/, __graft_entry__.smoke() and the
 * cpu_baseline leg of bench.py are its only users.
 *
 * CPU restatement of the reference's IIR streaming path:
 *   FilterBank::process      /root/reference/src/main/filters/FilterBank.cpp:256-291
 *   FilterBank::reset        FilterBank.cpp:238-254
 *   FilterBank::impulse_response  FilterBank.cpp:293-330
 * and of the lsp-dsp-lib 1.0.36 primitives it calls, dsp::biquad_process_x1/x2/x4/x8
 * (un-vendored dependency, modules.mk:29-33).  Their published algorithm is a
 * transposed direct form II section with pre-negated denominator signs
 * (Filter.cpp:2261-2262 "Sign negated", Filter.cpp:1628-1634):
 *
 *      y    = b0*x + d0
 *      d0'  = d1 + (b1*x + a1*y)
 *      d1'  =       b2*x + a2*y
 *
 * The x2/x4/x8 variants run 2/4/8 such sections in series on the same sample
 * stream (software-pipelined over SIMD lanes upstream); the arithmetic seen by
 * each section is the one above, so the oracle runs sections one after another.
 *
 * Parity pin: no reference test asserts IIR output, so the
 * streaming arithmetic is pinned through what the reference documents about it:
 *  (1) the sign convention + the BS.1770 table in Filter.cpp:2103-2111
 *      (tests/test_filter_design.py::test_anchor_k_weighting_table);
 *  (2) tests/test_oracle_filters.py: for every filter type the spectrum of THIS
 *      file's impulse response equals the transfer function Filter::freq_chart
 *      evaluates from the analog prototype (Filter.cpp:500-696) -- a wrong sign,
 *      section order, state update or delay in the recurrence below breaks it;
 *  (3) on the device, tests/hip/serial_biquad.hip runs this recurrence operation for operation and equals this
 *      file bit for bit (tests/test_biquad_gpu.py::test_device_twin_equals_the_oracle): the GPU's float32
 *      arithmetic is the one written here.
 * The README filter values in tests/golden/filter_anchors.json are a regression check of the designer, not a pin of this
 * arithmetic; they now also follow from tests/golden/filter_ref_designs.npz and filter_ref_streams.npz, recorded from the
 * reference's own Filter and FilterBank over a stand-in that IS this recurrence (oracle/ref_overlay/filters).
 *
 * Build: see oracle/Makefile (gcc -O2 -ffp-contract=off so the rounding is the
 * same on every host).
 */
#include <stddef.h>
#include <string.h>

/* One channel: `ns` sections in series. coef = ns x {b0,b1,b2,a1,a2}; state = ns x {d0,d1}. */
void orc_biquad_cascade(float *dst, const float *src, size_t n,
                        const float *coef, float *state, size_t ns)
{
    if (ns == 0)                     /* FilterBank.cpp:261-265: empty bank copies */
    {
        if (dst != src)
            memmove(dst, src, n * sizeof(float));
        return;
    }
    for (size_t s = 0; s < ns; ++s)
    {
        const float b0 = coef[5*s+0], b1 = coef[5*s+1], b2 = coef[5*s+2];
        const float a1 = coef[5*s+3], a2 = coef[5*s+4];
        float d0 = state[2*s+0], d1 = state[2*s+1];
        const float *in = (s == 0) ? src : dst;     /* later banks run in place, FilterBank.cpp:270 */
        for (size_t i = 0; i < n; ++i)
        {
            const float x  = in[i];
            const float y  = b0*x + d0;
            const float p1 = b1*x + a1*y;
            const float p2 = b2*x + a2*y;
            d0      = d1 + p1;
            d1      = p2;
            dst[i]  = y;
        }
        state[2*s+0] = d0;
        state[2*s+1] = d1;
    }
}

/* A bank of independent channels ([channels][stride] layout), optionally threaded. */
void orc_biquad_bank(float *dst, const float *src, size_t channels, size_t n,
                     size_t dst_stride, size_t src_stride,
                     const float *coef, float *state, const unsigned *nsec, size_t max_sections)
{
#ifdef _OPENMP
#pragma omp parallel for schedule(static)
#endif
    for (long c = 0; c < (long)channels; ++c)
        orc_biquad_cascade(dst + c*dst_stride, src + c*src_stride, n,
                           coef + (size_t)c*max_sections*5, state + (size_t)c*max_sections*2, nsec[c]);
}

/* FilterBank::impulse_response: save state, zero it, run a unit impulse, restore. */
void orc_biquad_impulse_response(float *out, size_t n, const float *coef, float *state, size_t ns)
{
    float backup[2*1024];
    if (ns > 1024)
        ns = 1024;
    memcpy(backup, state, 2*ns*sizeof(float));
    memset(state, 0, 2*ns*sizeof(float));
    memset(out, 0, n*sizeof(float));
    if (n > 0)
        out[0] = 1.0f;
    orc_biquad_cascade(out, out, n, coef, state, ns);
    memcpy(state, backup, 2*ns*sizeof(float));
}

/*
 * Time-varying sections: lsp-dsp-lib's dsp::dyn_biquad_process_x1/x2/x4/x8 as DynamicFilters::process calls them
 * (/root/reference/src/main/filters/DynamicFilters.cpp:255-305): the same transposed direct form II recurrence with
 * one coefficient set per SAMPLE and section.  Upstream pipelines the sections over SIMD lanes (sample n reaches
 * section j at step n + j, with its own coefficients travelling along: the diagonal cascade layout of
 * DynamicFilters.cpp:320-369); what each section computes for sample n is what is written here.
 * coef: [ns][n][5] = {b0, b1, b2, a1, a2} per section and sample, state: ns x {d0, d1}.
 * Pin: with the same coefficients for every sample this IS orc_biquad_cascade, bit for bit
 * (tests/test_oracle_dynamic_filters.py); no reference test or vector exists for the unit.
 */
void orc_dyn_biquad_cascade(float *dst, const float *src, size_t n, const float *coef, float *state, size_t ns)
{
    if (ns == 0)
    {
        if (dst != src)
            memmove(dst, src, n * sizeof(float));
        return;
    }
    for (size_t s = 0; s < ns; ++s)
    {
        const float *q = coef + s * n * 5;
        float d0 = state[2*s+0], d1 = state[2*s+1];
        const float *in = (s == 0) ? src : dst;
        for (size_t i = 0; i < n; ++i, q += 5)
        {
            const float x  = in[i];
            const float y  = q[0]*x + d0;
            const float p1 = q[1]*x + q[3]*y;
            const float p2 = q[2]*x + q[4]*y;
            d0      = d1 + p1;
            d1      = p2;
            dst[i]  = y;
        }
        state[2*s+0] = d0;
        state[2*s+1] = d1;
    }
}

/* The same in double arithmetic on the float coefficients: the round-off yardstick of the parity tests. */
void orc_dyn_biquad_cascade_f64(double *dst, const float *src, size_t n, const float *coef, double *state, size_t ns)
{
    for (size_t i = 0; i < n; ++i)
        dst[i] = src[i];
    for (size_t s = 0; s < ns; ++s)
    {
        const float *q = coef + s * n * 5;
        double d0 = state[2*s+0], d1 = state[2*s+1];
        for (size_t i = 0; i < n; ++i, q += 5)
        {
            const double x  = dst[i];
            const double y  = (double)q[0]*x + d0;
            const double p1 = (double)q[1]*x + (double)q[3]*y;
            const double p2 = (double)q[2]*x + (double)q[4]*y;
            d0      = d1 + p1;
            d1      = p2;
            dst[i]  = y;
        }
        state[2*s+0] = d0;
        state[2*s+1] = d1;
    }
}
