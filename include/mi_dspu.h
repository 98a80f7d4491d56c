/*
 * mi_dspu.h -- C-ABI of the MI355X (gfx950) implementation of the lsp-dsp-units
 * block-streaming hot path.
 *
 * This is the drop-in boundary: plain C, plain pointers and sizes, no C++ or
 * torch types.  Every entry point names the reference interface it replaces
 * (paths relative to the reference tree, lsp-plugins/lsp-dsp-units 1.0.36).
 *
 * Conventions
 *   - every function returns MI_OK (0) or a negative MI_E* code;
 *     mi_dspu_last_error() returns a thread-local human-readable message;
 *   - sample buffers are DEVICE pointers to float32, laid out
 *     [channel][stride] (one reference object == one channel == one row);
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); no
 *     entry point synchronises the stream unless its name says so;
 *   - objects are opaque handles created/destroyed by the library; they are
 *     not thread-safe (same contract as the reference objects).
 *   - there is NO CPU fallback: without a usable HIP device every compute
 *     entry point fails with MI_ENODEV.
 */
#ifndef MI_DSPU_H_
#define MI_DSPU_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MI_DSPU_ABI_VERSION     1

enum
{
    MI_OK            =  0,
    MI_EINVAL        = -1,   /* bad argument (reference: silently clamped or `false`)   */
    MI_ENOMEM        = -2,   /* allocation failure (reference: init() returns false)     */
    MI_ENODEV        = -3,   /* no HIP device / kernel image not loadable                 */
    MI_EHIP          = -4,   /* a HIP runtime call failed; see mi_dspu_last_error()       */
    MI_ESTATE        = -5    /* object not initialised (reference: STATUS_BAD_STATE)      */
};

/* ---- library / device plumbing ------------------------------------------------------- */

int         mi_dspu_abi_version(void);
const char *mi_dspu_last_error(void);
/* Number of visible HIP devices (0 when none; never fails). */
int         mi_dspu_device_count(void);
/* Select the device used by the calling thread (hipSetDevice). */
int         mi_dspu_set_device(int device);

int         mi_dspu_malloc(void **dev_ptr, size_t bytes);
int         mi_dspu_free(void *dev_ptr);
int         mi_dspu_memset(void *dev_ptr, int value, size_t bytes, void *stream);
int         mi_dspu_copy_h2d(void *dev_dst, const void *host_src, size_t bytes, void *stream);
int         mi_dspu_copy_d2h(void *host_dst, const void *dev_src, size_t bytes, void *stream);
int         mi_dspu_copy_d2d(void *dev_dst, const void *dev_src, size_t bytes, void *stream);
int         mi_dspu_stream_create(void **stream);
int         mi_dspu_stream_destroy(void *stream);
int         mi_dspu_stream_synchronize(void *stream);

/* Timing helper used by bench.py: runs `fn`-less event pairs on `stream`. */
int         mi_dspu_event_create(void **event);
int         mi_dspu_event_destroy(void *event);
int         mi_dspu_event_record(void *event, void *stream);
int         mi_dspu_event_synchronize(void *event);
int         mi_dspu_event_elapsed_ms(float *ms, void *start, void *stop);
/*
 * Environment switches -- the library reads exactly these five, at every call:
 *   MI_DSPU_COMPAT_BITS=1     runs of 4096-point blocks (Equalizer FIR/FFT, SpectralProcessor with a mask, SpectralSplitter at
 *                             rank 12) stay on the workgroup kernels, whose results are the block-by-block calls' BIT FOR BIT,
 *                             instead of the wave-resident transform kernels (1.3 - 1.7 x faster, within 1e-6 of the calls)
 *   MI_DSPU_EXACT_IIR=1       biquad banks START in the exact mode (mi_biquad_bank_set_exact below): the reference's serial recurrence,
 *                             its output bit for bit, for hosts that cannot be changed to call mi_dspu_set_exact_iir_default
 *   MI_CONV_TWO_LAUNCH=1      Convolver: frame launch + tail launch instead of the one-launch step   } fall-backs behind two
 *   MI_ILUFS_TWO_LAUNCHES=1   ILUFSMeter: bookkeeping in a launch of its own                         } in-launch hand-overs that
 *                             rest on gfx950's dispatch order / memory-side atomics (a wait that does not end raises a fault)
 *   MI_DSPU_TEST_PATH=a,b,..  TEST HOOK, not a tuning knob: sends calls down another LIVE path of the library -- one that other
 *                             inputs take anyway -- so that differential tests can hold two paths against each other:
 *                             blocks_loop, conv_batch_finish, conv_frame_per_launch, crossover_unfused, ilufs_rows_apart,
 *                             loudness_scalar, splitter_hop_launches, analyzer_strobe_per_launch, dyndelay_serial,
 *                             dyndelay_parallel
 */
/*
 * Arm a pair of events for the calling thread: the next hot-path kernel this
 * thread launches (the dominant kernel of the next process() call) records them
 * at its own begin and end (hipExtLaunchKernelGGL), so their elapsed time is the
 * kernel's launch duration as a profiler reports it.  One-shot.
 */
int         mi_dspu_profile_next_launch(void *start_event, void *stop_event);
/*
 * The hot-path kernel the calling thread launched last (its name as the library spells it, template arguments included;
 * "" before the first one).  For tests and profiles that must know WHICH launch a call took -- a run of blocks riding its
 * one-launch kernel or the block-by-block fallback -- not only that the result is right.  No reference counterpart.
 */
const char *mi_dspu_last_launch(void);
/*
 * The first 16 hex digits of the SHA-256 of a source file of csrc/ (e.g. "biquad.hip") as it was when THIS library was built,
 * or NULL for a name the build did not see.  Counter summaries under profiles/ carry the hashes of the sources they were
 * measured on; bench.py quotes a committed counter only while the library it loaded was built from the same source.
 */
const char *mi_dspu_source_sha(const char *file);
/*
 * hipGraph helpers for launch-bound inner loops: a run of steady-state *_process() calls on `stream` is captured once
 * and replayed (hipStreamBeginCapture / hipStreamEndCapture + hipGraphInstantiate / hipGraphLaunch).
 * begin: `stream` must be a created (non-NULL) stream.  end: returns an executable graph handle.
 * Banks without ring positions (biquad, crossover, dynamic filters) replay any run.  The others (delay, ring buffer,
 * convolver, equalizer, spectral processor, analyzer, splitter, loudness meters) hand ring positions kept on the host to
 * their kernels by value: end_capture() checks that the captured calls bring every such bank back to the positions it
 * started from and returns MI_ESTATE otherwise (capture a whole number of position periods: one lap of a delay line,
 * an even number of analyzer strobes, ...).  A refused capture is not lost work and leaves no inconsistent state: the
 * captured calls are executed ONCE inside end_capture() (synchronising the stream), so device rings and host positions
 * agree as after eager calls; no graph is returned.  Dynamic filters refuse capture (MI_ESTATE) while a clear of their
 * filter memory is pending (right after init / set_sample_rate): make one eager call first.  On a stream captured with
 * hipStreamBeginCapture directly those banks' process() returns MI_ESTATE and changes nothing.
 * launch: a bank that has re-made device buffers since the capture (the convolver's ring of frames is grown once, by
 * the bank's first mi_convolver_bank_process_blocks batch) makes the graph stale: MI_ESTATE, nothing is launched --
 * capture again.
 */
int         mi_dspu_graph_begin_capture(void *stream);
int         mi_dspu_graph_end_capture(void *stream, void **graph_exec);
int         mi_dspu_graph_launch(void *graph_exec, void *stream);
int         mi_dspu_graph_destroy(void *graph_exec);

/* ---- biquad cascade bank -------------------------------------------------------------- */
/*
 * One digital section, same field order/size as dsp::biquad_x1_t used by
 * FilterBank::add_chain() (include/lsp-plug.in/dsp-units/filters/FilterBank.h:86,
 * fields as written in src/main/filters/Filter.cpp:2254-2265):
 *      y[n] = b0 x[n] + b1 x[n-1] + b2 x[n-2] + a1 y[n-1] + a2 y[n-2]
 * (denominator signs pre-negated).  p0..p2 are padding.
 */
typedef struct mi_biquad_x1
{
    float b0, b1, b2;
    float a1, a2;
    float p0, p1, p2;
} mi_biquad_x1_t;

/*
 * mi_biquad_bank: `channels` independent lsp::dspu::FilterBank objects
 * (filters/FilterBank.h:34-139), each holding up to `max_sections` biquads that
 * run strictly in series (src/main/filters/FilterBank.cpp:256-291).
 */
typedef struct mi_biquad_bank mi_biquad_bank_t;

/* FilterBank::init(filters), FilterBank.cpp:62-92, for every channel. */
int mi_biquad_bank_create(mi_biquad_bank_t **bank, uint32_t channels, uint32_t max_sections);
/* FilterBank::destroy(), FilterBank.cpp:51-60. */
int mi_biquad_bank_destroy(mi_biquad_bank_t *bank);
/*
 * FilterBank::begin() + add_chain() x count + end(clear) for one channel
 * (FilterBank.h:78-82, FilterBank.cpp:94-99,106-236).  As in the reference the
 * delay memory of the channel is cleared when `clear` is non-zero or when the
 * number of sections changed (FilterBank.cpp:233-235).  count > max_sections
 * is clamped the way add_chain() clamps (the last slot keeps the last chain).
 * Host-side only; the device tables are refreshed by the next process()/commit().
 */
int mi_biquad_bank_set_chains(mi_biquad_bank_t *bank, uint32_t channel,
                              const mi_biquad_x1_t *chains, uint32_t count, int clear);
/* Same for all channels at once: chains is [channels][count]. */
int mi_biquad_bank_set_all_chains(mi_biquad_bank_t *bank, const mi_biquad_x1_t *chains,
                                  uint32_t count, int clear);
/* FilterBank::size() of one channel. */
int mi_biquad_bank_size(const mi_biquad_bank_t *bank, uint32_t channel, uint32_t *count);
/* A channel that is switched off is skipped by process(): its delay memory stays as it is and its output row is not
 * written -- what a caller gets by not calling FilterBank::process() for that object (the meters do this for disabled
 * channels, LoudnessMeter.cpp:420-422, ILUFSMeter.cpp:370). */
int mi_biquad_bank_set_row_enabled(mi_biquad_bank_t *bank, uint32_t channel, int enabled);
/*
 * The bank's arithmetic.  0 (default): the time-parallel kernels -- the reference's recurrence inside chunks of 16 samples,
 * the chunks joined by a scan: the same filter in another order of roundings, within the recursion's own float32 noise of the
 * reference's output (DESIGN.md section 4 states the bound), 550 000 Msamples/s at 1024 channels x 8 sections.
 * 1: FilterBank::process's serial recurrence (/root/reference/src/main/filters/FilterBank.cpp:256-291; lsp-dsp-lib's
 * biquad_process_x1 form, every product and sum rounded on its own) sample after sample, a section per lane: the reference's
 * output and filter memory BIT FOR BIT, at the price of the recursion's latency chain (32 000 Msamples/s at that size).
 * The filter memory is the same in both modes: calls may alternate.  process(), process_blocks() and impulse_response()
 * follow the mode, and chains of banks (Crossover, the Equalizer's IIR mode) then run bank by bank instead of through their
 * fused launch; the meters' fused sums (LoudnessMeter / ILUFSMeter) keep the fast kernels.
 * mi_dspu_set_exact_iir_default (or MI_DSPU_EXACT_IIR=1 in the environment): the mode banks created from now on start in (process-wide; how the class layer's
 * dspu::Filter / FilterBank / Equalizer objects are put into the exact mode: set it before constructing them).
 */
int mi_biquad_bank_set_exact(mi_biquad_bank_t *bank, int on);
int mi_dspu_set_exact_iir_default(int on);
/*
 * Measurement aid: the shader clock (GHz) the last run-of-blocks launch of the biquad bank (mi_biquad_bank_process_blocks)
 * held, from the cycle counter and the 100 MHz wall clock its first workgroup stamps at entry and exit, and that workgroup's
 * life in microseconds.  The part lowers its clock under dense packed arithmetic: an issue-rate roof priced at the nominal
 * 2.4 GHz is not the one the launch met (bench.py prices valu_issue_frac at this clock).  Synchronises with the device.
 */
int mi_dspu_last_stream_clock(double *ghz, double *microseconds);
/* Push pending coefficient tables / state clears to the device (async on stream). */
int mi_biquad_bank_commit(mi_biquad_bank_t *bank, void *stream);
/* FilterBank::reset(), FilterBank.cpp:238-254; channel = UINT32_MAX for all. */
int mi_biquad_bank_reset(mi_biquad_bank_t *bank, uint32_t channel, void *stream);
/*
 * FilterBank::process(out, in, samples) for every channel, FilterBank.cpp:256-291.
 * out/in: device float32 [channels][*_stride]; out may be the same buffer as in
 * (exact alias only, as in the reference).  A channel with 0 sections copies.
 */
int mi_biquad_bank_process(mi_biquad_bank_t *bank, float *out, const float *in,
                           size_t samples, size_t out_stride, size_t in_stride, void *stream);
/*
 * `blocks` consecutive FilterBank::process() calls in one C call: block k reads in[k] and writes out[k] (HOST arrays of
 * `blocks` DEVICE pointers, each [channels][*_stride]); the filter memory is carried from block to block exactly as by
 * `blocks` separate calls -- it IS `blocks` launches, issued back to back without returning to the caller in between
 * (a host language whose call overhead is of the order of the 12 us a 1024 x 4096 block takes keeps the GPU busy this way).
 */
int mi_biquad_bank_process_blocks(mi_biquad_bank_t *bank, float *const *out, const float *const *in, size_t blocks,
                                  size_t samples, size_t out_stride, size_t in_stride, void *stream);
/*
 * FilterBank::impulse_response(out, samples), FilterBank.cpp:293-330: delay
 * memory is saved, zeroed, a unit impulse is run and the memory restored.
 */
int mi_biquad_bank_impulse_response(mi_biquad_bank_t *bank, float *out, size_t samples,
                                    size_t out_stride, void *stream);
/* Delay memory access (biquad_t::d[], FilterBank.cpp:248-252): host arrays of
 * [channels][max_sections][2] floats {d0,d1}.  Synchronise the stream. */
int mi_biquad_bank_get_state(mi_biquad_bank_t *bank, float *host_state, void *stream);
int mi_biquad_bank_set_state(mi_biquad_bank_t *bank, const float *host_state, void *stream);

/* ---- filter designer (host side) --------------------------------------------------------- */
/*
 * filter_params_t, field for field (include/lsp-plug.in/dsp-units/filters/common.h:137-145).
 */
typedef struct mi_filter_params
{
    uint32_t    nType;      /* enum mi_filter_type */
    uint32_t    nSlope;
    float       fFreq;
    float       fFreq2;
    float       fGain;
    float       fQuality;
} mi_filter_params_t;

/* filter_type_t with the same enumerator values (filters/common.h:38-135). */
enum mi_filter_type
{
    MI_FLT_NONE = 0,
    MI_FLT_BT_AMPLIFIER = 1,
    MI_FLT_MT_AMPLIFIER = 2,
    MI_FLT_BT_RLC_LOPASS = 3,
    MI_FLT_MT_RLC_LOPASS = 4,
    MI_FLT_BT_RLC_HIPASS = 5,
    MI_FLT_MT_RLC_HIPASS = 6,
    MI_FLT_BT_RLC_LOSHELF = 7,
    MI_FLT_MT_RLC_LOSHELF = 8,
    MI_FLT_BT_RLC_HISHELF = 9,
    MI_FLT_MT_RLC_HISHELF = 10,
    MI_FLT_BT_RLC_BELL = 11,
    MI_FLT_MT_RLC_BELL = 12,
    MI_FLT_BT_RLC_RESONANCE = 13,
    MI_FLT_MT_RLC_RESONANCE = 14,
    MI_FLT_BT_RLC_NOTCH = 15,
    MI_FLT_MT_RLC_NOTCH = 16,
    MI_FLT_BT_RLC_ALLPASS = 17,
    MI_FLT_MT_RLC_ALLPASS = 18,
    MI_FLT_BT_RLC_ALLPASS2 = 19,
    MI_FLT_MT_RLC_ALLPASS2 = 20,
    MI_FLT_BT_RLC_LADDERPASS = 21,
    MI_FLT_MT_RLC_LADDERPASS = 22,
    MI_FLT_BT_RLC_LADDERREJ = 23,
    MI_FLT_MT_RLC_LADDERREJ = 24,
    MI_FLT_BT_RLC_BANDPASS = 25,
    MI_FLT_MT_RLC_BANDPASS = 26,
    MI_FLT_BT_RLC_ENVELOPE = 27,
    MI_FLT_MT_RLC_ENVELOPE = 28,
    MI_FLT_BT_BWC_LOPASS = 29,
    MI_FLT_MT_BWC_LOPASS = 30,
    MI_FLT_BT_BWC_HIPASS = 31,
    MI_FLT_MT_BWC_HIPASS = 32,
    MI_FLT_BT_BWC_LOSHELF = 33,
    MI_FLT_MT_BWC_LOSHELF = 34,
    MI_FLT_BT_BWC_HISHELF = 35,
    MI_FLT_MT_BWC_HISHELF = 36,
    MI_FLT_BT_BWC_BELL = 37,
    MI_FLT_MT_BWC_BELL = 38,
    MI_FLT_BT_BWC_LADDERPASS = 39,
    MI_FLT_MT_BWC_LADDERPASS = 40,
    MI_FLT_BT_BWC_LADDERREJ = 41,
    MI_FLT_MT_BWC_LADDERREJ = 42,
    MI_FLT_BT_BWC_BANDPASS = 43,
    MI_FLT_MT_BWC_BANDPASS = 44,
    MI_FLT_BT_BWC_ALLPASS = 45,
    MI_FLT_MT_BWC_ALLPASS = 46,
    MI_FLT_BT_LRX_LOPASS = 47,
    MI_FLT_MT_LRX_LOPASS = 48,
    MI_FLT_BT_LRX_HIPASS = 49,
    MI_FLT_MT_LRX_HIPASS = 50,
    MI_FLT_BT_LRX_LOSHELF = 51,
    MI_FLT_MT_LRX_LOSHELF = 52,
    MI_FLT_BT_LRX_HISHELF = 53,
    MI_FLT_MT_LRX_HISHELF = 54,
    MI_FLT_BT_LRX_BELL = 55,
    MI_FLT_MT_LRX_BELL = 56,
    MI_FLT_BT_LRX_LADDERPASS = 57,
    MI_FLT_MT_LRX_LADDERPASS = 58,
    MI_FLT_BT_LRX_LADDERREJ = 59,
    MI_FLT_MT_LRX_LADDERREJ = 60,
    MI_FLT_BT_LRX_BANDPASS = 61,
    MI_FLT_MT_LRX_BANDPASS = 62,
    MI_FLT_BT_LRX_ALLPASS = 63,
    MI_FLT_MT_LRX_ALLPASS = 64,
    MI_FLT_DR_APO_LOPASS = 65,
    MI_FLT_DR_APO_HIPASS = 66,
    MI_FLT_DR_APO_BANDPASS = 67,
    MI_FLT_DR_APO_NOTCH = 68,
    MI_FLT_DR_APO_ALLPASS = 69,
    MI_FLT_DR_APO_ALLPASS2 = 70,
    MI_FLT_DR_APO_PEAKING = 71,
    MI_FLT_DR_APO_LOSHELF = 72,
    MI_FLT_DR_APO_HISHELF = 73,
    MI_FLT_DR_APO_LADDERPASS = 74,
    MI_FLT_DR_APO_LADDERREJ = 75,
    MI_FLT_A_WEIGHTED = 76,
    MI_FLT_B_WEIGHTED = 77,
    MI_FLT_C_WEIGHTED = 78,
    MI_FLT_D_WEIGHTED = 79,
    MI_FLT_K_WEIGHTED = 80
};

/* dsp::f_cascade_t: numerator t[] and denominator b[] of one analog (or plot) cascade. */
typedef struct mi_filter_cascade
{
    float t[4];
    float b[4];
} mi_filter_cascade_t;

/* Filter::filter_mode_t (filters/Filter.h:41-47). */
enum { MI_FM_BYPASS = 0, MI_FM_BILINEAR = 1, MI_FM_MATCHED = 2, MI_FM_APO = 3 };

/*
 * Filter::update() + Filter::rebuild() without a bank (src/main/filters/Filter.cpp:141-167,208-403):
 * limits the parameters, builds the prototype cascades and transforms them into digital sections
 * exactly as they would be handed to FilterBank::add_chain().  Host-only, no GPU needed.
 * chains/cascades may be NULL to query the counts; at most max_* entries are written.
 */
int mi_filter_design(const mi_filter_params_t *params, uint32_t sample_rate,
                     mi_biquad_x1_t *chains, uint32_t max_chains, uint32_t *n_chains,
                     mi_filter_cascade_t *cascades, uint32_t max_cascades, uint32_t *n_cascades, int *mode);
/* Filter::limit(), Filter.cpp:161-167. */
int mi_filter_limit(mi_filter_params_t *params, uint32_t sample_rate);
/*
 * Filter::freq_chart(c, f, count), packed-complex form (Filter.cpp:602-696): c[2i], c[2i+1] = H(f[i]).
 */
int mi_filter_freq_chart(const mi_filter_params_t *params, uint32_t sample_rate, float *c, const float *f, size_t count);

/* ---- partitioned FFT convolver bank ------------------------------------------------------ */
/*
 * mi_convolver_bank: `channels` independent lsp::dspu::Convolver objects
 * (include/lsp-plug.in/dsp-units/util/Convolver.h:35-114): exact linear
 * convolution of each channel with its own impulse response, zero added
 * latency, any call size.
 */
typedef struct mi_convolver_bank mi_convolver_bank_t;

/*
 * Convolver::init(data, count, rank, phase) for every channel
 * (src/main/util/Convolver.cpp:77-215).  irs: HOST float32 [channels][ir_stride];
 * channel c uses counts[c] taps (counts == NULL: `count` for all).  rank is
 * clamped to [8,16] (Convolver.h:28-29, Convolver.cpp:87) and sets the frame
 * 2^(rank-1) at which whole-frame calls take the FFT path; frames above 4096
 * are processed as 4096-sample partitions.  phase only staggers the
 * reference's CPU load (Convolver.cpp:139) and has no effect on the output; it
 * is accepted and ignored.  All counts == 0 leaves the bank uninitialised:
 * process() then writes zeros (Convolver.cpp:80-84,219-223).  Synchronises `stream`.
 */
int mi_convolver_bank_create(mi_convolver_bank_t **bank, uint32_t channels, const float *irs, size_t ir_stride,
                             const uint32_t *counts, uint32_t count, uint32_t rank, float phase, void *stream);
/* Replace the impulse response of the named channels (`channels`: HOST flags, NULL = every channel) by `count` taps read
 * from DEVICE memory [channels][ir_stride] (count within the capacity the bank was created with); input history is kept.
 * Used by the equalizer bank when it retunes (the reference re-parses its FIR the same way, Equalizer.cpp:342-345).
 * Single-partition banks (taps <= frame) take the new response at the next frame boundary: the frame being received keeps
 * the one it began with.  Synchronises `stream`. */
int mi_convolver_bank_set_irs_device(mi_convolver_bank_t *bank, const float *irs, size_t ir_stride, uint32_t count,
                                     const uint8_t *channels, void *stream);
/*
 * Single-partition banks: the new responses of the named channels wait for the next frame boundary and are cross-faded in
 * over that frame -- weight of the new response 0 up to B/2, a linear ramp over the next B output positions of the frame's
 * 2B-long result, 1 after that (what Equalizer::process does for a "smooth" retune, Equalizer.cpp:486-501).  Every
 * channel behaves like one reference Equalizer object with its vConv, vNewConv and EF_XFADE: a later call for a channel
 * that is still waiting replaces its target; a channel that is not named takes no part (the reference's cross-fade is not a
 * no-op for an unchanged response -- it also scales the overlap tail of the previous blocks, Equalizer.cpp:496,499);
 * mi_convolver_bank_set_irs_device() for a waiting channel changes the response the fade starts from, not its target
 * (after the fade the target, i.e. the older request, is in force -- Equalizer.cpp:491).
 */
int mi_convolver_bank_crossfade_irs_device(mi_convolver_bank_t *bank, const float *irs, size_t ir_stride, uint32_t count,
                                           const uint8_t *channels, void *stream);
/* Convolver::destroy(), Convolver.cpp:71-75.  MI_EHIP (the bank is freed all the same) if a hand-over had timed out, see
 * mi_convolver_bank_faults. */
int mi_convolver_bank_destroy(mi_convolver_bank_t *bank);
/* Diagnostic (synchronises the stream): how often the two roles of the one-launch frame step gave up waiting for each other
 * (about a second each; 0 on a healthy device -- DESIGN.md 3.2).  A fault is not silent: it raises a host-visible flag, and
 * from then on mi_convolver_bank_process (without synchronising), this call and mi_convolver_bank_destroy return MI_EHIP
 * until mi_convolver_bank_reset -- the frame in which it happened and everything after it is invalid.  The one-launch step
 * is used on gfx950 only; MI_CONV_TWO_LAUNCH=1 in the environment selects the two-launch form (no in-launch waiting). */
int mi_convolver_bank_faults(mi_convolver_bank_t *bank, uint32_t *count, void *stream);
/* Forget all input history (state right after init); clears a recorded fault. */
int mi_convolver_bank_reset(mi_convolver_bank_t *bank, void *stream);
/* Convolver::rank() / data_size() (Convolver.h:100-106) plus the partition geometry in use. */
int mi_convolver_bank_info(const mi_convolver_bank_t *bank, uint32_t *rank, uint32_t *frame,
                           uint32_t *partitions, uint32_t *data_size);
/*
 * Convolver::process(dst, src, count) for every channel, Convolver.cpp:217-313.
 * out/in: device float32 [channels][*_stride]; out may be the same buffer as in.
 */
int mi_convolver_bank_process(mi_convolver_bank_t *bank, float *out, const float *in, size_t samples,
                              size_t out_stride, size_t in_stride, void *stream);
/*
 * `blocks` consecutive mi_convolver_bank_process calls in one C call (Convolver.cpp:217-313 per block): block k reads in[k]
 * and writes out[k] (HOST tables of DEVICE pointers).  Whole frames of a partitioned bank go in batches of up to 16 frames
 * whose tails come out of ONE pass over the partitions' images; samples and state are those of the calls one by one.
 */
int mi_convolver_bank_process_blocks(mi_convolver_bank_t *bank, float *const *out, const float *const *in, size_t blocks,
                                     size_t samples, size_t out_stride, size_t in_stride, void *stream);

/* ---- windows and spectral envelopes (host side) ---------------------------------------- */
/* windows::window_t with the same enumerator values (include/lsp-plug.in/dsp-units/misc/windows.h:34-62). */
enum mi_window
{
    MI_WINDOW_HANN, MI_WINDOW_HAMMING, MI_WINDOW_BLACKMAN, MI_WINDOW_LANCZOS, MI_WINDOW_GAUSSIAN,
    MI_WINDOW_POISSON, MI_WINDOW_PARZEN, MI_WINDOW_TUKEY, MI_WINDOW_WELCH, MI_WINDOW_NUTTALL,
    MI_WINDOW_BLACKMAN_NUTTALL, MI_WINDOW_BLACKMAN_HARRIS, MI_WINDOW_HANN_POISSON, MI_WINDOW_BARTLETT_HANN,
    MI_WINDOW_BARTLETT_FEJER, MI_WINDOW_TRIANGULAR, MI_WINDOW_RECTANGULAR, MI_WINDOW_FLAT_TOP,
    MI_WINDOW_COSINE, MI_WINDOW_SQR_COSINE, MI_WINDOW_CUBIC, MI_WINDOW_TOTAL
};
/* envelope::envelope_t (include/lsp-plug.in/dsp-units/misc/envelope.h:36-50). */
enum mi_envelope
{
    MI_ENVELOPE_VIOLET_NOISE, MI_ENVELOPE_BLUE_NOISE, MI_ENVELOPE_WHITE_NOISE, MI_ENVELOPE_PINK_NOISE,
    MI_ENVELOPE_BROWN_NOISE, MI_ENVELOPE_MINUS_4_5_DB, MI_ENVELOPE_PLUS_4_5_DB, MI_ENVELOPE_TOTAL
};
/* windows::window(dst, n, type), src/main/misc/windows.cpp:62-98 (host memory). */
int mi_window(float *dst, size_t n, int type);
/*
 * The parameterised families, windows::*_general of misc/windows.h:71,86,95,101,113,128,134,143,146,155:
 *   TRIANGULAR {dn}   HAMMING {a, b}   BLACKMAN {a}   NUTTALL {a0..a3}   FLAT_TOP {a0..a4}   GAUSSIAN {s}
 *   POISSON {t}   BARTLETT_HANN {a0, a1, a2}   HANN_POISSON {a}   TUKEY {a}
 * (HANN, BLACKMAN_NUTTALL, BLACKMAN_HARRIS and BARTLETT_FEJER are members of those families and take the same lists).
 */
int mi_window_general(float *dst, size_t n, int type, const float *params, uint32_t count);
/* envelope::noise_lin / reverse_noise_lin(dst, first, last, center, n, type), src/main/misc/envelope.cpp:63-123 (host
 * memory): the colour's spectral envelope (f / center)^k on n linearly spaced frequencies, or the opposite colour's. */
int mi_envelope_noise_lin(float *dst, float first, float last, float center, size_t n, int type);
int mi_envelope_reverse_noise_lin(float *dst, float first, float last, float center, size_t n, int type);
/* envelope::noise_log / reverse_noise_log (envelope.cpp:170-268: logarithmic frequency grid) and noise_list /
 * reverse_noise_list (:272-344: an explicit list of frequencies); reverse != 0 selects the compensating colour. */
int mi_envelope_noise_log(float *dst, float first, float last, float center, size_t n, int type, int reverse);
int mi_envelope_noise_list(float *dst, const float *freqs, float center, size_t n, int type, int reverse);

/* ---- spectral processor bank -------------------------------------------------------------- */
/*
 * mi_spectral_bank: `channels` lsp::dspu::SpectralProcessor objects sharing rank and phase, equivalently one
 * lsp::dspu::MultiSpectralProcessor with `channels` channels (util/SpectralProcessor.h:45-175,
 * util/MultiSpectralProcessor.h:47-247): 50 %-overlap sine-window STFT -> operation -> ISTFT overlap-add,
 * latency 2^rank samples.
 */
typedef struct mi_spectral_bank mi_spectral_bank_t;
enum { MI_SPECTRAL_OP_NONE = 0, MI_SPECTRAL_OP_MASK = 1, MI_SPECTRAL_OP_CALLBACK = 2 };
/*
 * spectral_processor_func_t / multi_spectral_processor_func_t on the device
 * (util/SpectralProcessor.h:39, util/MultiSpectralProcessor.h:41): `spectrum` is a DEVICE pointer to
 * [channels][2 * 2^rank] floats (packed complex, all 2^rank bins); the function runs on the host and may enqueue
 * work on `stream` (including collectives); the inverse transform is ordered after it on the same stream.
 */
typedef void (*mi_spectral_func_t)(void *object, void *subject, float *spectrum, size_t rank, size_t channels, void *stream);

/* SpectralProcessor::init(max_rank), SpectralProcessor.cpp:59-75 (ranks 5..18: frames up to 2^14 samples are transformed
 * in LDS in one launch per hop, longer ones through global memory in several). */
int mi_spectral_bank_create(mi_spectral_bank_t **bank, uint32_t channels, uint32_t max_rank);
int mi_spectral_bank_destroy(mi_spectral_bank_t *bank);
/* set_rank / set_phase, SpectralProcessor.cpp:127-145 (a rank above max_rank is ignored, phase is clamped to 0..1). */
int mi_spectral_bank_set_rank(mi_spectral_bank_t *bank, uint32_t rank);
int mi_spectral_bank_set_phase(mi_spectral_bank_t *bank, float phase);
/* Analysis / synthesis windows (enum mi_window, or -1 for none).  The reference processor always uses the sine
 * window on both sides (SpectralProcessor.cpp:118); the Equalizer's SPM mode uses none / squared cosine
 * (Equalizer.cpp:352-353,535-540) and is built on this. */
int mi_spectral_bank_set_windows(mi_spectral_bank_t *bank, int in_window, int out_window);
/* get_rank(), latency(), remaining() (SpectralProcessor.h:128,142, SpectralProcessor.cpp:251-255). */
int mi_spectral_bank_get(const mi_spectral_bank_t *bank, uint32_t *rank, uint32_t *latency, uint32_t *remaining);
/* bind(func, object, subject) / unbind(), SpectralProcessor.cpp:91-105. */
int mi_spectral_bank_bind(mi_spectral_bank_t *bank, mi_spectral_func_t func, void *object, void *subject);
int mi_spectral_bank_unbind(mi_spectral_bank_t *bank);
/*
 * Built-in callback: spectrum[k] *= mask[k], k = 0..2^(rank-1) (real gains, applied to both halves of the
 * spectrum), fused into the transform kernel.  mask is HOST memory, one row shared by all channels
 * (mask_stride == 0) or [channels][mask_stride].
 */
int mi_spectral_bank_bind_mask(mi_spectral_bank_t *bank, const float *mask, size_t mask_stride, void *stream);
/* MultiSpectralProcessor::bind_in/bind_out (MultiSpectralProcessor.cpp:160-227): which channels have an input /
 * an output bound (HOST byte arrays, NULL = unchanged; default all bound). Callback mode only. */
int mi_spectral_bank_bind_channels(mi_spectral_bank_t *bank, const uint8_t *has_in, const uint8_t *has_out, void *stream);
/* reset(), SpectralProcessor.cpp:257-266. */
int mi_spectral_bank_reset(mi_spectral_bank_t *bank, void *stream);
/* process(dst, src, count), SpectralProcessor.cpp:147-199.  With out == NULL: process(src, count), :201-249 -- analysis
 * only: the function is called on every frame, nothing is transformed back and the output buffer is shifted and its
 * tail zeroed instead of overlap-added (MultiSpectralProcessor timing: out == NULL just skips the copy-out).
 * Throughput note: a call that hands over whole frames from rows whose pointers are 8-byte aligned and whose strides are
 * even is one launch per hop for the operations NONE and MASK at ranks 8..13 (two around the function for CALLBACK with
 * MultiSpectralProcessor's timing); anything else adds two strided copies per piece. */
int mi_spectral_bank_process(mi_spectral_bank_t *bank, float *out, const float *in, size_t count,
                             size_t out_stride, size_t in_stride, void *stream);
/*
 * `blocks` consecutive mi_spectral_bank_process calls in one C call (SpectralProcessor.cpp:143-199 per block): block k reads
 * in[k] and writes out[k] (HOST tables of DEVICE pointers).  Runs of blocks of whole frames whose buffers lie apart go out as
 * one launch; the samples and the state are those of the calls one by one.
 */
int mi_spectral_bank_process_blocks(mi_spectral_bank_t *bank, float *const *out, const float *const *in, size_t blocks,
                                    size_t count, size_t out_stride, size_t in_stride, void *stream);
/* When a complete frame is transformed: eager == 0 (default) when the next sample arrives, as SpectralProcessor does
 * (SpectralProcessor.cpp:159: remaining() can read 0, the function runs at the start of the following call); eager != 0
 * as soon as the frame is complete, as MultiSpectralProcessor does (MultiSpectralProcessor.cpp:324). */
int mi_spectral_bank_set_timing(mi_spectral_bank_t *bank, int eager);

/* ---- spectrum analyzer bank ---------------------------------------------------------------- */
/*
 * mi_analyzer_bank: one lsp::dspu::Analyzer with `channels` channels (util/Analyzer.h:53-361): ring-buffer
 * ingest, windowed FFT magnitude per channel once per refresh period, exponential smoothing, envelope.
 */
typedef struct mi_analyzer_bank mi_analyzer_bank_t;
enum { MI_ANALYZER_SAMPLE_RATE, MI_ANALYZER_RATE, MI_ANALYZER_WINDOW, MI_ANALYZER_ENVELOPE, MI_ANALYZER_SHIFT,
       MI_ANALYZER_REACTIVITY, MI_ANALYZER_RANK, MI_ANALYZER_ACTIVE };
enum { MI_ANALYZER_CH_FREEZE, MI_ANALYZER_CH_ENABLE, MI_ANALYZER_CH_DELAY };

/* Analyzer::init(channels, max_rank, max_sr, min_rate, max_delay), Analyzer.cpp:83-152 (ranks 5..18; above 14 through global memory). */
int mi_analyzer_bank_create(mi_analyzer_bank_t **bank, uint32_t channels, uint32_t max_rank, uint32_t max_sample_rate,
                            float min_rate, uint32_t max_delay);
int mi_analyzer_bank_destroy(mi_analyzer_bank_t *bank);
/* set_sample_rate/set_rate/set_window/set_envelope/set_shift/set_reactivity/set_rank/set_activity, Analyzer.cpp:154-211. */
/* Analyzer::reset(): the smoothed and the published spectra are cleared at the next reconfigure (Analyzer.cpp:274-281) */
int mi_analyzer_bank_reset(mi_analyzer_bank_t *bank);
int mi_analyzer_bank_configure(mi_analyzer_bank_t *bank, int what, double value);
/* freeze_channel/enable_channel/set_channel_delay, Analyzer.cpp:213-249. */
int mi_analyzer_bank_channel(mi_analyzer_bank_t *bank, uint32_t channel, int what, uint32_t value);
/*
 * Analyzer::process(in, samples), Analyzer.cpp:299-409.  in: device [channels][in_stride] or NULL (zeros).
 * Unlike the reference (which divides by zero, Analyzer.cpp:258-260,315) a refresh rate above
 * sample_rate / channels is rejected with MI_EINVAL.
 */
int mi_analyzer_bank_process(mi_analyzer_bank_t *bank, const float *in, size_t samples, size_t in_stride, void *stream);
/* Analyzer::get_spectrum for every channel at once, Analyzer.cpp:443-456: out[c][i] = vData[c][idx[i]] * envelope[idx[i]]
 * (out and idx are DEVICE pointers). */
int mi_analyzer_bank_get_spectrum(mi_analyzer_bank_t *bank, float *out, size_t out_stride, const uint32_t *idx,
                                  uint32_t count, void *stream);
/* Per-bin sum over this bank's channels of the smoothed magnitudes (2^(rank-1)+1 floats, DEVICE): the local half
 * of the cross-channel per-bin reduction; the caller all-reduces it across GPUs. */
int mi_analyzer_bank_reduce_bins(mi_analyzer_bank_t *bank, float *out, int with_envelope, void *stream);
/*
 * mi_analyzer_bank_process followed by mi_analyzer_bank_reduce_bins in one call: the two launches.  (The reduction as a second
 * role of the analysis launch -- round 3, 20.3 against 17.2 us per step -- was removed in round 6.)
 */
int mi_analyzer_bank_process_reduce(mi_analyzer_bank_t *bank, const float *in, size_t samples, size_t in_stride,
                                    float *out, int with_envelope, void *stream);
/*
 * `frames` consecutive mi_analyzer_bank_process_reduce calls in one C call: frame k takes in[k] (HOST array of DEVICE
 * pointers, each [channels][in_stride]) and leaves its per-bin sums in out + k * out_stride.  Where every call is exactly
 * one strobe (samples == period) the spectra of up to 16 frames are kept and their reductions run as ONE launch; the
 * sums and the state left behind are those of `frames` separate calls, bit for bit.
 */
int mi_analyzer_bank_process_reduce_frames(mi_analyzer_bank_t *bank, const float *const *in, size_t frames, size_t samples,
                                           size_t in_stride, float *out, size_t out_stride, int with_envelope, void *stream);
int mi_analyzer_bank_info(const mi_analyzer_bank_t *bank, uint32_t *rank, uint32_t *bins, uint32_t *period, uint32_t *step);

/*
 * Multi-GPU: the one exchange step of the path.  Channels are sharded over the GPUs of a node, one process per GPU;
 * the per-bin sum over ALL channels (the MultiSpectralProcessor-style callback stage, util/MultiSpectralProcessor.h:41,
 * BASELINE config 5) is each rank's mi_analyzer_bank_reduce_bins followed by one RCCL all-reduce over xGMI, issued
 * from the library's C++ host side on the caller's stream.  A communicator is created like an ncclComm_t: one rank
 * makes the 128-byte id and hands it to the others by whatever means the host has (a file, MPI, torch.distributed).
 * mi_dspu_comm_adopt wraps an ncclComm_t the host already owns (not destroyed with the wrapper).
 * reduce_bins adds the channels in a shard-composable order (blocks of 16 channels, then a binary tree aligned to
 * powers of two), so the halves of a channel set reduce to partial sums whose sum is the reduction of the whole set.
 */
#define MI_DSPU_COMM_ID_BYTES 128
typedef struct mi_dspu_comm mi_dspu_comm_t;
int mi_dspu_comm_unique_id(void *id128);
int mi_dspu_comm_create(mi_dspu_comm_t **comm, const void *id128, int nranks, int rank);
int mi_dspu_comm_adopt(mi_dspu_comm_t **comm, void *nccl_comm);
int mi_dspu_comm_destroy(mi_dspu_comm_t *comm);
int mi_dspu_comm_info(const mi_dspu_comm_t *comm, int *nranks, int *rank);
/* bins: DEVICE [frames][2^(rank-1)+1], summed in place over the ranks of `comm` (float32, ncclSum). */
int mi_analyzer_bank_allreduce_bins(mi_analyzer_bank_t *bank, float *bins, size_t frames, mi_dspu_comm_t *comm, void *stream);
/*
 * The same exchange step beside the caller's stream, for callers that double-buffer the sums: begin() issues the collective on
 * the communicator's own (least urgent: it takes the CUs the next batch's launches leave) side stream behind everything `stream` has enqueued so far -- `partial` summed over the
 * ranks into `total` (may be the same buffer) -- and returns; `stream` goes on with the next batch of frames, whose reduction
 * writes ANOTHER buffer.  mi_dspu_comm_wait() makes `stream` wait, on the device, for the slot's collective: call it in front of
 * whatever reads `total` and in front of the work that overwrites the slot's buffers again.  Slots: 0 .. MI_DSPU_COMM_SLOTS - 1.
 * The result is the serial call's bit for bit (the same ncclAllReduce on the same data).  Not capturable into a hipGraph.
 * Reference for the semantic: the cross-channel callback of MultiSpectralProcessor
 * (/root/reference/include/lsp-plug.in/dsp-units/util/MultiSpectralProcessor.h:41).
 */
#define MI_DSPU_COMM_SLOTS 4
int mi_analyzer_bank_allreduce_bins_begin(mi_analyzer_bank_t *bank, const float *partial, float *total, size_t frames,
                                          mi_dspu_comm_t *comm, int slot, void *stream);
int mi_dspu_comm_wait(mi_dspu_comm_t *comm, int slot, void *stream);

/* ---- dynamic filter bank --------------------------------------------------- */
/*
 * mi_dynfilter_bank: `channels` x lsp::dspu::DynamicFilters(filters) that share their filter settings
 * (filters/DynamicFilters.h:41-189, src/main/filters/DynamicFilters.cpp): filters whose gain follows a per-sample
 * gain vector.  set_params / set_filter_active / process / freq_chart have the reference's meaning (:127-181, .h:147-153,
 * :204-318, :1774-1970); process() takes DEVICE rows [channels][stride] for the samples AND the gains (every channel its
 * own gain curve) and is a copy for an inactive / FLT_NONE / slope-0 filter (:207-212).  A change of a filter's type clears
 * the memory of every filter at the next process() (:132-133,214-219).  FLT_*_RLC_ENVELOPE has no dynamic form here (the
 * reference's builder reads unset fields, :1022-1085) and is refused with MI_EINVAL, as are the static-only types.
 */
typedef struct mi_dynfilter_bank mi_dynfilter_bank_t;
int mi_dynfilter_bank_create(mi_dynfilter_bank_t **bank, uint32_t channels, uint32_t filters);
int mi_dynfilter_bank_destroy(mi_dynfilter_bank_t *bank);
int mi_dynfilter_bank_set_sample_rate(mi_dynfilter_bank_t *bank, uint32_t sample_rate);
int mi_dynfilter_bank_set_params(mi_dynfilter_bank_t *bank, uint32_t id, const mi_filter_params_t *params);
/* the parameters as set_params left them (fFreq2 transformed, DynamicFilters.cpp:170-178) */
int mi_dynfilter_bank_get_params(const mi_dynfilter_bank_t *bank, uint32_t id, mi_filter_params_t *params, int *active);
int mi_dynfilter_bank_set_filter_active(mi_dynfilter_bank_t *bank, uint32_t id, int active);
int mi_dynfilter_bank_process(mi_dynfilter_bank_t *bank, uint32_t id, float *out, const float *in, const float *gain,
                              size_t samples, size_t out_stride, size_t in_stride, size_t gain_stride, void *stream);
/*
 * Host-only (no device needed, like mi_filter_design): `params` are what set_params() receives.
 * sections: the digital sections the filter has at a fixed gain -- what every sample of a constant gain vector is
 * filtered with.  freq_chart: DynamicFilters::freq_chart(id, c, f, gain, count), packed complex.
 */
int mi_dynfilter_sections(const mi_filter_params_t *params, uint32_t sample_rate, float gain, mi_biquad_x1_t *sections,
                          uint32_t max_sections, uint32_t *count);
int mi_dynfilter_freq_chart(const mi_filter_params_t *params, uint32_t sample_rate, float *c, const float *f, float gain, size_t count);

/* ---- equalizer bank --------------------------------------------------------------------------- */
/*
 * mi_equalizer_bank: `channels` x lsp::dspu::Equalizer(filters, fir_rank)
 * (include/lsp-plug.in/dsp-units/filters/Equalizer.h:47-289).  equalizer_mode_t values as in Equalizer.h:35-42.
 */
typedef struct mi_equalizer_bank mi_equalizer_bank_t;
enum { MI_EQM_BYPASS = 0, MI_EQM_IIR = 1, MI_EQM_FIR = 2, MI_EQM_FFT = 3, MI_EQM_SPM = 4 };

/* Equalizer::init(filters, fir_rank), src/main/filters/Equalizer.cpp:67-160 (fir_rank 0 or 5..13). */
int mi_equalizer_bank_create(mi_equalizer_bank_t **bank, uint32_t channels, uint32_t filters, uint32_t fir_rank);
int mi_equalizer_bank_destroy(mi_equalizer_bank_t *bank);
/* set_params(id, params) of one channel (or UINT32_MAX: all), Equalizer.cpp:210-218; MI_EINVAL for a bad id
 * where the reference returns false. */
int mi_equalizer_bank_set_params(mi_equalizer_bank_t *bank, uint32_t channel, uint32_t filter, const mi_filter_params_t *params);
int mi_equalizer_bank_get_params(const mi_equalizer_bank_t *bank, uint32_t channel, uint32_t filter, mi_filter_params_t *params);
/* set_mode / set_sample_rate / set_actual_sample_rate, Equalizer.cpp:360-375,188-203. */
int mi_equalizer_bank_set_mode(mi_equalizer_bank_t *bank, int mode);
int mi_equalizer_bank_set_sample_rate(mi_equalizer_bank_t *bank, uint32_t sample_rate);
int mi_equalizer_bank_set_actual_sample_rate(mi_equalizer_bank_t *bank, uint32_t sample_rate);
/* get_latency() (reconfigures first), Equalizer.cpp:237-241. */
int mi_equalizer_bank_get_latency(mi_equalizer_bank_t *bank, uint32_t *latency, void *stream);
/* reset(), Equalizer.cpp:573-597. */
int mi_equalizer_bank_reset(mi_equalizer_bank_t *bank, void *stream);
/* smooth() / set_smooth(), Equalizer.cpp:618-626: in FIR and FFT modes a retune is cross-faded in over the block
 * that completes next (EF_XFADE, Equalizer.cpp:339-343,486-501) instead of switching at its start. */
int mi_equalizer_bank_set_smooth(mi_equalizer_bank_t *bank, int smooth);
/* process(out, in, samples), Equalizer.cpp:460-571. */
int mi_equalizer_bank_process(mi_equalizer_bank_t *bank, float *out, const float *in, size_t samples,
                              size_t out_stride, size_t in_stride, void *stream);
/*
 * `blocks` consecutive Equalizer::process() calls in one C call: block k reads in[k] and writes out[k] (HOST arrays of
 * DEVICE pointers, each [channels][*_stride]).  In the FIR and FFT modes runs of blocks of exactly 2^fir_rank samples go
 * as ONE launch (the response's image and the overlap-add tail stay on chip from block to block); results and carried
 * state are those of `blocks` separate calls, bit for bit (Equalizer.cpp:460-571 called block after block).
 */
int mi_equalizer_bank_process_blocks(mi_equalizer_bank_t *bank, float *const *out, const float *const *in, size_t blocks,
                                     size_t samples, size_t out_stride, size_t in_stride, void *stream);
/* filter count, fir_rank(), mode(), ir_size() (Equalizer.cpp:599-616). */
int mi_equalizer_bank_info(const mi_equalizer_bank_t *bank, uint32_t *filters, uint32_t *fir_rank, int *mode, uint32_t *ir_size);

/* ---- IIR crossover bank (first caller of the filter path) ----------------------------- */
/*
 * mi_crossover_bank: one lsp::dspu::Crossover per channel, all channels sharing the split settings
 * (util/Crossover.h:97-330, src/main/util/Crossover.cpp): `bands` bands, bands-1 split points; an active split point
 * low-passes into the band on its left (+ all-pass filters of the split points above it, so that the bands sum to an
 * all-pass) and high-passes into the chain on its right.  Linkwitz-Riley slopes: 1 = LR2 (12 dB/oct) ... 9 = LR32,
 * 0 = split point off (enum crossover_slope_t).  Band outputs go to caller-owned device buffers instead of the
 * reference's per-band callback.
 */
typedef struct mi_crossover_bank mi_crossover_bank_t;
enum { MI_CROSS_MODE_BT = 0, MI_CROSS_MODE_MT = 1 };                /* crossover_mode_t */

/* Crossover::init(bands, buf_size), Crossover.cpp:71-160 (default split frequencies log-spaced over 10 Hz..24 kHz). */
int mi_crossover_bank_create(mi_crossover_bank_t **bank, uint32_t channels, uint32_t bands);
int mi_crossover_bank_destroy(mi_crossover_bank_t *bank);
/* set_sample_rate / set_slope / set_frequency / set_mode / set_gain, Crossover.cpp:185-254,327-341 */
int mi_crossover_bank_set_sample_rate(mi_crossover_bank_t *bank, uint32_t sample_rate);
int mi_crossover_bank_set_slope(mi_crossover_bank_t *bank, uint32_t split, uint32_t slope);
int mi_crossover_bank_set_frequency(mi_crossover_bank_t *bank, uint32_t split, float freq);
int mi_crossover_bank_set_mode(mi_crossover_bank_t *bank, uint32_t split, int mode);
int mi_crossover_bank_set_gain(mi_crossover_bank_t *bank, uint32_t band, float gain);
/* get_slope / get_frequency / get_mode (any pointer may be NULL) */
int mi_crossover_bank_get_split(const mi_crossover_bank_t *bank, uint32_t split, uint32_t *slope, float *freq, int *mode);
/* Crossover::needs_reconfiguration(), util/Crossover.h:352 */
int mi_crossover_bank_needs_reconfiguration(const mi_crossover_bank_t *bank, int *pending);
/* get_gain / get_band_start / get_band_end / band_active after reconfigure(), Crossover.cpp:256-325 */
int mi_crossover_bank_get_band(mi_crossover_bank_t *bank, uint32_t band, float *gain, float *start, float *end, int *active,
                               void *stream);
/*
 * Crossover::process(in, samples), Crossover.cpp:451-498.  band_out: HOST array of `bands` DEVICE pointers
 * [channels][out_stride]; NULL = no handler bound to that band (its low-pass is skipped like in the reference).
 * Inactive bands are not written.  in: [channels][in_stride].
 */
int mi_crossover_bank_process(mi_crossover_bank_t *bank, float *const *band_out, const float *in, size_t samples,
                              size_t out_stride, size_t in_stride, void *stream);
/*
 * `blocks` consecutive process() calls in one C call (Crossover.cpp:451-498 per block): block i reads in[i] and writes band k
 * to band_out[i * bands + k] (HOST tables of DEVICE pointers; a band is NULL in every block or in none).  Runs of blocks
 * whose buffers do not overlap each other go out as ONE launch; the results are bit for bit those of the calls one by one.
 */
int mi_crossover_bank_process_blocks(mi_crossover_bank_t *bank, float *const *band_out, const float *const *in, size_t blocks,
                                     size_t samples, size_t out_stride, size_t in_stride, void *stream);
/* freq_chart(band, c, f, count), packed complex (re, im interleaved), HOST memory, Crossover.cpp:500-590 */
int mi_crossover_bank_freq_chart(mi_crossover_bank_t *bank, uint32_t band, float *c, const float *f, size_t count, void *stream);

/* ---- loudness meter bank (SURVEY 8f, K-weighted cascade fused with a mean-square reduction) ------------ */
/*
 * mi_loudness_bank: `meters` x lsp::dspu::LoudnessMeter(channels) sharing one configuration
 * (meters/LoudnessMeter.h:47-330, src/main/meters/LoudnessMeter.cpp): per channel a weighting filter (K by default,
 * ITU-R BS.1770), a sliding mean square over `period` ms, the channels mixed with their BS.2051 designation weights,
 * square root.  Rows of the sample buffers: row = meter * channels + channel.
 * The weighting filters of this bank and of mi_ilufs_bank follow the process-wide exact / fast default; mi_loudness_bank_set_exact
 * and mi_ilufs_bank_set_exact choose per bank.  A meter does not always average a filter's round-off away: a window of a few
 * samples, a step through the K curve's high-pass or gating blocks of the filter's decaying memory read it; a host
 * that needs the reference's reading to 1e-5 there switches the exact mode on and pays the serial recurrence's latency.
 */
typedef struct mi_loudness_bank mi_loudness_bank_t;
enum { MI_BS_WEIGHT_NONE = 0, MI_BS_WEIGHT_A, MI_BS_WEIGHT_B, MI_BS_WEIGHT_C, MI_BS_WEIGHT_D, MI_BS_WEIGHT_K };   /* bs::weighting_t */
/* bs::channel_t (misc/broadcast.h:58-94), numeric values as in the reference: 0 NONE, 1 CENTER, 4 LEFT, 5 RIGHT,
 * 6..11 the +1.5 dB group (FRONT_LEFT .. RIGHT_SURROUND), 32/33 LFE1/LFE2 (excluded from the measurement). */
enum { MI_BS_CHANNEL_NONE = 0, MI_BS_CHANNEL_CENTER = 1, MI_BS_CHANNEL_LEFT = 4, MI_BS_CHANNEL_RIGHT = 5,
       MI_BS_CHANNEL_FRONT_LEFT = 6, MI_BS_CHANNEL_RIGHT_SURROUND = 11, MI_BS_CHANNEL_LFE1 = 32, MI_BS_CHANNEL_LFE2 = 33 };

/* LoudnessMeter::init(channels, max_period), LoudnessMeter.cpp:85-185 (mono: CENTER, stereo: LEFT/RIGHT by default). */
int mi_loudness_bank_create(mi_loudness_bank_t **bank, uint32_t meters, uint32_t channels, float max_period_ms);
int mi_loudness_bank_destroy(mi_loudness_bank_t *bank);
/* set_sample_rate (reallocates and clears the mean-square lines), set_period, set_weighting, LoudnessMeter.cpp:203-309 */
int mi_loudness_bank_set_sample_rate(mi_loudness_bank_t *bank, uint32_t sample_rate, void *stream);
int mi_loudness_bank_set_period(mi_loudness_bank_t *bank, float period_ms);
int mi_loudness_bank_set_weighting(mi_loudness_bank_t *bank, int weighting);
/* per channel index, for every meter: set_designation / set_link / set_active, LoudnessMeter.cpp:213-268 */
int mi_loudness_bank_set_designation(mi_loudness_bank_t *bank, uint32_t channel, int designation);
int mi_loudness_bank_set_link(mi_loudness_bank_t *bank, uint32_t channel, float link);
int mi_loudness_bank_set_active(mi_loudness_bank_t *bank, uint32_t channel, int active, void *stream);
/* clear(): fLoudness, the lines and running sums of the enabled channels, and the weighting filters' memory are zeroed; the
 * filters stay as they are.  A DELIBERATE DEVIATION from LoudnessMeter.cpp:274-289, whose sFilter.clear() on a Filter with an
 * external bank makes the next process() add the cascades to the bank a second time (sBank.nItems 2 -> 4 with the K curve) over
 * stale packed sections and delays that were not zeroed, until the next filter update: ill-defined there.
 * This is what the reference computes for clear() followed by a forced filter update.  latency() in samples, :326-329 */
int mi_loudness_bank_clear(mi_loudness_bank_t *bank, void *stream);
/* bind(id, out, in) with / without an input: an enabled channel without an input is left out of the blocks (its filter does
 * not run, its squares line is not written, it is not mixed: LoudnessMeter.cpp:421-422) but keeps taking part in
 * refresh_rms() and clear(); binding it again continues where it stopped (unlike set_active(1), which clears). */
int mi_loudness_bank_set_bound(mi_loudness_bank_t *bank, uint32_t channel, int bound);
/* LoudnessMeter::needs_update() / update_settings(), meters/LoudnessMeter.h:264-269 */
int mi_loudness_bank_needs_update(const mi_loudness_bank_t *bank, int *pending);
int mi_loudness_bank_update_settings(mi_loudness_bank_t *bank, void *stream);
int mi_loudness_bank_latency(const mi_loudness_bank_t *bank, uint32_t *samples);
/*
 * process(out, count) / process(out, count, gain), LoudnessMeter.cpp:462-564.  in: [meters*channels][in_stride];
 * out: [meters][out_stride] or NULL; ch_out: [meters*channels][out_stride] or NULL (the reference's per-channel vOut with
 * linking: link 0 = the channel's own RMS, 1 = the mixed loudness).  The second form multiplies every output by gain and,
 * like the reference's, leaves loudness() alone (only the first form records fLoudness, LoudnessMeter.cpp:485).
 */
int mi_loudness_bank_process(mi_loudness_bank_t *bank, float *out, float *ch_out, const float *in, size_t count,
                             size_t out_stride, size_t in_stride, void *stream);
int mi_loudness_bank_process_gain(mi_loudness_bank_t *bank, float *out, float *ch_out, const float *in, size_t count,
                                  size_t out_stride, size_t in_stride, float gain, void *stream);
/* loudness(): the last value of the mixed loudness recorded by process() (HOST array of `meters` floats; synchronises) */
int mi_loudness_bank_loudness(mi_loudness_bank_t *bank, float *loudness, void *stream);
/* mi_biquad_bank_set_exact of the weighting filters (the bank starts with the process-wide default) */
int mi_loudness_bank_set_exact(mi_loudness_bank_t *bank, int on);

/*
 * mi_ilufs_bank: `meters` x lsp::dspu::ILUFSMeter(channels) sharing one configuration
 * (meters/ILUFSMeter.h:41-260, src/main/meters/ILUFSMeter.cpp): integrated loudness per ITU-R BS.1770-4 -- weighting
 * filter, gating blocks of `block_period` ms overlapping by 75 %, absolute (-70 LKFS) and relative (-10 LU) gating over
 * the integration period (0 = since the last clear()).  The output is the integrated loudness as a gain, held between
 * block boundaries.  Rows of the input: row = meter * channels + channel.
 */
typedef struct mi_ilufs_bank mi_ilufs_bank_t;
/* ILUFSMeter::init(channels, max_int_time [s], block_period [ms]), ILUFSMeter.cpp:113-211 */
int mi_ilufs_bank_create(mi_ilufs_bank_t **bank, uint32_t meters, uint32_t channels, float max_int_time, float block_period_ms);
int mi_ilufs_bank_destroy(mi_ilufs_bank_t *bank);
/* set_sample_rate / set_integration_period [s] / set_weighting, ILUFSMeter.cpp:258-322 */
int mi_ilufs_bank_set_sample_rate(mi_ilufs_bank_t *bank, uint32_t sample_rate, void *stream);
int mi_ilufs_bank_set_integration_period(mi_ilufs_bank_t *bank, float period, void *stream);
int mi_ilufs_bank_set_weighting(mi_ilufs_bank_t *bank, int weighting);
/* per channel index, for every meter: set_designation / set_active, ILUFSMeter.cpp:223-256 */
int mi_ilufs_bank_set_designation(mi_ilufs_bank_t *bank, uint32_t channel, int designation);
int mi_ilufs_bank_set_active(mi_ilufs_bank_t *bank, uint32_t channel, int active);
int mi_ilufs_bank_clear(mi_ilufs_bank_t *bank, void *stream);                      /* ILUFSMeter.cpp:547-560 */
/* process(out, count, gain), ILUFSMeter.cpp:355-470.  in: [meters*channels][in_stride]; out: [meters][out_stride] or NULL. */
int mi_ilufs_bank_process(mi_ilufs_bank_t *bank, float *out, const float *in, size_t count, size_t out_stride,
                          size_t in_stride, float gain, void *stream);
/* loudness() of every meter (HOST array of `meters` floats; synchronises) */
/* ILUFSMeter::needs_update() / update_settings(), meters/ILUFSMeter.h:244-249 */
int mi_ilufs_bank_needs_update(const mi_ilufs_bank_t *bank, int *pending);
int mi_ilufs_bank_update_settings(mi_ilufs_bank_t *bank, void *stream);
int mi_ilufs_bank_loudness(mi_ilufs_bank_t *bank, float *loudness, void *stream);
/* The gating-block history as the meters hold it (vLoudness / nMSHead / nMSCount of ILUFSMeter.h): hist is HOST memory
 * [meters][*size] (NULL: only the size is wanted), head / count HOST [meters] or NULL.  *size is nMSSize: max(int_count, 64)
 * floats rounded up to DEFAULT_ALIGN = 0x40 bytes (ILUFSMeter.cpp:299; the constant is lsp-common-lib's and unpinned). */
int mi_ilufs_bank_history(mi_ilufs_bank_t *bank, float *hist, uint32_t *size, uint32_t *head, uint32_t *count, void *stream);
/* mi_biquad_bank_set_exact of the weighting filters (the bank starts with the process-wide default); on: reserves the buffer
 * of the exact path, so that process() never allocates.  In the exact mode the bookkeeping is always a launch of its own. */
int mi_ilufs_bank_set_exact(mi_ilufs_bank_t *bank, int on);

/* ---- true-peak meter bank (ITU-R BS.1770-4 Annex 2) ------------------------------------------------------------------ */
/*
 * mi_truepeak_bank: `channels` x lsp::dspu::TruePeakMeter (meters/TruePeakMeter.h:36-155, src/main/meters/TruePeakMeter.cpp):
 * every input upsampled N times by a Lanczos kernel (a = 10, lsp-dsp-lib's lanczos_resample_Nx16bit), every output the
 * largest magnitude of its N oversampled values.  N from the sample rate (:85-100): 0 (plain |x|) at 176400 Hz and above,
 * 2 from 88200, 3 from 58800, 4 from 44100, 6 from 29400, 8 below.  The state is the last 20 inputs of each channel, kept
 * on the device; the bank has no positions, so its process calls can be captured into a graph and replayed.
 * Rows of the sample buffers: [channels][stride].
 */
typedef struct mi_truepeak_bank mi_truepeak_bank_t;
/* TruePeakMeter::init(), TruePeakMeter.cpp:69-82: sample rate 0 as constructed, so the first update picks N = 8 */
int mi_truepeak_bank_create(mi_truepeak_bank_t **bank, uint32_t channels);
int mi_truepeak_bank_destroy(mi_truepeak_bank_t *bank);                                 /* :59-67 */
/* set_sample_rate(sr), :102-109: takes effect at the next update_settings() */
int mi_truepeak_bank_set_sample_rate(mi_truepeak_bank_t *bank, uint32_t sample_rate);
/* update_settings(), :149-189: clears the state only when N changes.  On a stream being captured an update that changes N
 * is refused (MI_ESTATE): call it before the capture. */
int mi_truepeak_bank_update_settings(mi_truepeak_bank_t *bank, void *stream);
int mi_truepeak_bank_clear(mi_truepeak_bank_t *bank, void *stream);                     /* :191-195 */
/* latency(), :274-277: 10 samples while N != 0, else 0; oversampling(): the current N (nTimes) */
int mi_truepeak_bank_latency(const mi_truepeak_bank_t *bank, uint32_t *samples);
int mi_truepeak_bank_oversampling(const mi_truepeak_bank_t *bank, uint32_t *times);
/* process(dst, src, count), :197-236, update_settings() first.  dst may equal src (in place, same stride); otherwise the
 * two must not overlap. */
int mi_truepeak_bank_process(mi_truepeak_bank_t *bank, float *dst, const float *src, size_t count, size_t dst_stride,
                             size_t src_stride, void *stream);
/* process_max(src, count), :238-272, update_settings() first: peaks is a DEVICE array of `channels` floats, each the largest
 * value process() would have written for that channel; the state advances as process() advances it.  (The reference's
 * returns 0.0f and looks at only part of the oversampled block; its header documents the maximum, which is what this is.) */
int mi_truepeak_bank_process_max(mi_truepeak_bank_t *bank, float *peaks, const float *src, size_t count, size_t src_stride,
                                 void *stream);
/* The coefficients the kernels use for `times` = 2, 3, 4, 6, 8 (0: none): h is HOST memory [times][20] or NULL, row k the
 * phase k / times, h_k[t] = float(L(t - 10 + k / times)) with L(x) = sinc(x) sinc(x / 10) computed in double; row 0 is the
 * unit impulse at t = 10.  *count = times * 20.  No device needed. */
int mi_truepeak_coefficients(uint32_t times, float *h, size_t *count);

/* ---- oversampler bank (Lanczos resampling with anti-alias filter) ----------------------------------------------------- */
/*
 * mi_oversampler_bank: `channels` x lsp::dspu::Oversampler (util/Oversampler.h:107-288, src/main/util/Oversampler.cpp):
 * every input upsampled N times by a Lanczos kernel of half-width a, the caller's work on the oversampled rows, the
 * anti-alias low-pass (FLT_BT_BWC_LOPASS, slope 30, min(20 kHz, 0.42 sr), designed at sr N; :108-126) and the decimation.
 * The upsample state is the last 2a inputs of each channel on the device; the bank has no positions (no nUpHead), so its
 * calls can be captured into a graph and replayed.  The filter is an ordinary mi_biquad_bank the bank owns: it follows the
 * process-wide exact / fast default (mi_dspu_set_exact_iir_default) and mi_oversampler_bank_set_exact.
 * Rows of the sample buffers: [channels][stride]; oversampled rows hold N * count samples.
 */
typedef struct mi_oversampler_bank mi_oversampler_bank_t;
/* over_mode_t with the same enumerator values (util/Oversampler.h:62-100).  N = 2, 3, 4, 6, 8 by group; a = 2, 3, 4 for
 * *X2, *X3, *X4, 4 for *12BIT (the reference says only "latency 4": the *X4 table is used),
 * 10 for *16BIT (the true-peak table), 62 for *24BIT. */
enum mi_over_mode
{
    MI_OM_NONE = 0,
    MI_OM_LANCZOS_2X2 = 1, MI_OM_LANCZOS_2X3 = 2, MI_OM_LANCZOS_2X4 = 3, MI_OM_LANCZOS_2X12BIT = 4, MI_OM_LANCZOS_2X16BIT = 5, MI_OM_LANCZOS_2X24BIT = 6,
    MI_OM_LANCZOS_3X2 = 7, MI_OM_LANCZOS_3X3 = 8, MI_OM_LANCZOS_3X4 = 9, MI_OM_LANCZOS_3X12BIT = 10, MI_OM_LANCZOS_3X16BIT = 11, MI_OM_LANCZOS_3X24BIT = 12,
    MI_OM_LANCZOS_4X2 = 13, MI_OM_LANCZOS_4X3 = 14, MI_OM_LANCZOS_4X4 = 15, MI_OM_LANCZOS_4X12BIT = 16, MI_OM_LANCZOS_4X16BIT = 17, MI_OM_LANCZOS_4X24BIT = 18,
    MI_OM_LANCZOS_6X2 = 19, MI_OM_LANCZOS_6X3 = 20, MI_OM_LANCZOS_6X4 = 21, MI_OM_LANCZOS_6X12BIT = 22, MI_OM_LANCZOS_6X16BIT = 23, MI_OM_LANCZOS_6X24BIT = 24,
    MI_OM_LANCZOS_8X2 = 25, MI_OM_LANCZOS_8X3 = 26, MI_OM_LANCZOS_8X4 = 27, MI_OM_LANCZOS_8X12BIT = 28, MI_OM_LANCZOS_8X16BIT = 29, MI_OM_LANCZOS_8X24BIT = 30
};
/* IOversamplerCallback::process / oversampler_callback_t (util/Oversampler.h:36-60) for a bank: called on the HOST once per
 * process() call, it enqueues the caller's work on `stream` over the oversampled rows -- buf is DEVICE memory
 * [channels][stride] with `samples` = N * count samples per row, worked on in place -- and returns an MI_* status. */
typedef int (*mi_oversampler_callback_t)(float *buf, size_t samples, size_t stride, uint32_t channels, void *stream, void *arg);
/* Oversampler::construct() + init(), Oversampler.cpp:53-93: OM_NONE, rate 0, filtering on, every update pending */
int mi_oversampler_bank_create(mi_oversampler_bank_t **bank, uint32_t channels);
int mi_oversampler_bank_destroy(mi_oversampler_bank_t *bank);                           /* :95-106 */
/* set_sample_rate(sr), :108-126: the only call that sets the filter's parameters (a bank whose rate was never set filters
 * with FLT_NONE).  The sections are designed and sent at the next update_settings(). */
int mi_oversampler_bank_set_sample_rate(mi_oversampler_bank_t *bank, uint32_t sample_rate);
/* set_mode(mode), :1055-1063: the resampling kernels follow the mode at once (as pFunc does), state and filter at the next
 * update_settings(); mode(), :1065-1068 */
int mi_oversampler_bank_set_mode(mi_oversampler_bank_t *bank, uint32_t mode);
int mi_oversampler_bank_mode(const mi_oversampler_bank_t *bank, uint32_t *mode);
/* set_filtering(filter), util/Oversampler.h:191-197; filtering(), :1070-1073; modified(), util/Oversampler.h:209-212 */
int mi_oversampler_bank_set_filtering(mi_oversampler_bank_t *bank, int on);
int mi_oversampler_bank_filtering(const mi_oversampler_bank_t *bank, int *on);
int mi_oversampler_bank_modified(const mi_oversampler_bank_t *bank, int *yes);
/* update_settings(), :128-144: zeroes the upsample state and clears the filter when the mode, the filtering flag or the
 * sample rate changed, and designs the filter at sr N for the current N.  The caller runs it, as in the reference; the
 * process entries do not.  On a stream being captured an update that changes anything is refused (MI_ESTATE). */
int mi_oversampler_bank_update_settings(mi_oversampler_bank_t *bank, void *stream);
/* get_oversampling(), :146-195; latency(), :955-1006 (a); max_latency(), util/Oversampler.h:281 (62) */
int mi_oversampler_bank_oversampling(const mi_oversampler_bank_t *bank, uint32_t *times);
int mi_oversampler_bank_latency(const mi_oversampler_bank_t *bank, uint32_t *samples);
int mi_oversampler_bank_max_latency(const mi_oversampler_bank_t *bank, uint32_t *samples);
/* The scratch rows [channels][N count] of process() and of a filtered downsample() (fUpBuffer / fDownBuffer, :70-93) for
 * calls of up to `count` samples at the current mode.  A call that would have to grow them on a stream being captured
 * returns MI_ESTATE: reserve before capturing. */
int mi_oversampler_bank_reserve(mi_oversampler_bank_t *bank, size_t count);
/* mi_biquad_bank_set_exact of the anti-alias filter's bank (sFilter, util/Oversampler.h:131) */
int mi_oversampler_bank_set_exact(mi_oversampler_bank_t *bank, int on);
/* upsample(dst, src, count), :197-367: dst rows of N * count samples; dst and src must not overlap.  OM_NONE copies. */
int mi_oversampler_bank_upsample(mi_oversampler_bank_t *bank, float *dst, const float *src, size_t count, size_t dst_stride,
                                 size_t src_stride, void *stream);
/* downsample(dst, src, count), :369-525: src rows of N * count samples through the filter (when filtering is on), every
 * N-th kept; dst and src must not overlap.  OM_NONE copies. */
int mi_oversampler_bank_downsample(mi_oversampler_bank_t *bank, float *dst, const float *src, size_t count, size_t dst_stride,
                                   size_t src_stride, void *stream);
/* process(dst, src, count, callback, arg), :527-953: upsample into the scratch rows, the callback (NULL: none), the filter
 * in place, the decimation.  dst may equal src (same stride).  It shares the upsample state with upsample() and the filter
 * state with downsample().  OM_NONE (:731-737, :945-951): a copy, then the callback on the dst rows. */
int mi_oversampler_bank_process(mi_oversampler_bank_t *bank, float *dst, const float *src, size_t count, size_t dst_stride,
                                size_t src_stride, mi_oversampler_callback_t callback, void *arg, void *stream);
/* The filter_params_t the bank holds (:117-125, limited as Filter::update limits them) and the rate it designs them at */
int mi_oversampler_bank_get_filter(const mi_oversampler_bank_t *bank, mi_filter_params_t *params, uint32_t *sample_rate);
/* The coefficients the kernels of `mode` use (lanczos_resample_NxK of lsp-dsp-lib as get_function() picks them, :1008-1052;
 * inferred): h is HOST memory [N][2a] or NULL, row k the phase k / N, h_k[t] = float(L(t - a + k / N)) with
 * L(x) = sinc(x) sinc(x / a) computed in double; row 0 is the unit impulse at t = a.  *count = N * 2a, 0 for OM_NONE.
 * No device needed. */
int mi_oversampler_coefficients(uint32_t mode, float *h, size_t *count);

/* ---- compressor bank (envelope follower and two-knee gain curve) ------------------------------------------------------ */
/*
 * mi_compressor_bank: `channels` x lsp::dspu::Compressor (dynamics/Compressor.h:44-289, src/main/dynamics/Compressor.cpp),
 * every channel with settings of its own.  process() is the reference's: the envelope follower (:226-259), a serial
 * recurrence over (fEnvelope, fPeak, nHoldCounter), then the gain curve of two knees (dsp::compressor_x2_gain, as the scalar
 * overload states it, :297-310).  The envelope, the peak and the hold counter are the reference's bit for bit in float32
 * (each product and each sum rounds once); the gain goes through the device's logf / expf and is within the bound
 * DESIGN.md section 3.10 derives.  The state lives on the device; the bank has no positions, so its process calls can be
 * captured into a graph and replayed.  Inputs are finite: NaN is out of scope.  Subnormal envelopes are kept.
 * Rows of the sample buffers: [channels][stride].
 */
typedef struct mi_compressor_bank mi_compressor_bank_t;
enum mi_compressor_mode { MI_CM_DOWNWARD = 0, MI_CM_UPWARD = 1, MI_CM_BOOSTING = 2 };     /* compressor_mode_t */
/* dsp::compressor_knee_t / compressor_x2_t of lsp-dsp-lib: below start the constant gain, above end
 * exp(tilt[0] ln x + tilt[1]), between them exp((herm[0] ln x + herm[1]) ln x + herm[2]) */
typedef struct { float start, end, gain, herm[3], tilt[2]; } mi_compressor_knee_t;
/* what update_settings() computes: fTauAttack, fTauRelease, fReleaseThresh as set, nHold, sComp */
typedef struct { float tau_attack, tau_release, release_threshold; uint32_t hold; mi_compressor_knee_t k[2]; } mi_compressor_params_t;
/* the setters' values: times in ms, thresholds, knee and ratio as the reference takes them */
typedef struct
{
    uint32_t sample_rate, mode;
    float attack_threshold, release_threshold, boost_threshold, attack, release, hold, knee, ratio;
} mi_compressor_settings_t;
/* update_settings(), :89-220, of one compressor in host float32 (expf, logf): all three modes, boosting with its two cases
 * on boost_threshold >= 1.  No device needed. */
int mi_compressor_compute_params(const mi_compressor_settings_t *settings, mi_compressor_params_t *params);
/* construct(), :46-83: every channel DOWNWARD, ratio 1, boost threshold -72 dB, everything else 0, an update pending */
int mi_compressor_bank_create(mi_compressor_bank_t **bank, uint32_t channels);
int mi_compressor_bank_destroy(mi_compressor_bank_t *bank);
/* The setters of one channel (:362-461): each returns early on an unchanged value, otherwise the channel's update is
 * pending until update_settings().  set_knee limits to [0, 1], set_hold to >= 0, as the reference does. */
int mi_compressor_bank_set_sample_rate(mi_compressor_bank_t *bank, uint32_t channel, uint32_t sample_rate);
int mi_compressor_bank_set_mode(mi_compressor_bank_t *bank, uint32_t channel, uint32_t mode);
int mi_compressor_bank_set_threshold(mi_compressor_bank_t *bank, uint32_t channel, float attack, float release);
int mi_compressor_bank_set_boost_threshold(mi_compressor_bank_t *bank, uint32_t channel, float boost);
int mi_compressor_bank_set_timings(mi_compressor_bank_t *bank, uint32_t channel, float attack, float release);
int mi_compressor_bank_set_hold(mi_compressor_bank_t *bank, uint32_t channel, float hold);
int mi_compressor_bank_set_knee(mi_compressor_bank_t *bank, uint32_t channel, float knee);
int mi_compressor_bank_set_ratio(mi_compressor_bank_t *bank, uint32_t channel, float ratio);
/* update_settings() of every channel with an update pending; the changed stretch of the parameter table goes to the device
 * (and the call waits for it).  The process entries run it first, as the reference's do.  On a stream being captured a
 * pending update is refused (MI_ESTATE): call it before the capture.  clear(): envelope, peak and hold counter to zero. */
int mi_compressor_bank_update_settings(mi_compressor_bank_t *bank, void *stream);
int mi_compressor_bank_clear(mi_compressor_bank_t *bank, void *stream);
/* What the last update_settings() computed for the channel (HOST memory); fEnvelope, fPeak, nHoldCounter of the channel as
 * the work enqueued on `stream` leaves them (HOST memory, each may be NULL; waits for the stream) */
int mi_compressor_bank_get_params(const mi_compressor_bank_t *bank, uint32_t channel, mi_compressor_params_t *params);
int mi_compressor_bank_get_state(mi_compressor_bank_t *bank, uint32_t channel, float *envelope, float *peak, uint32_t *hold,
                                 void *stream);
/* process(out, env, in, samples), :222-267: gain receives the VCA gain, env (NULL: not wanted) the envelope.  gain or env
 * may be the input rows (in place, same stride); gain and env differ. */
int mi_compressor_bank_process(mi_compressor_bank_t *bank, float *gain, float *env, const float *in, size_t count,
                               size_t gain_stride, size_t env_stride, size_t in_stride, void *stream);
/* dst = audio * gain(sc) in the same launch: process() on the sidechain rows sc followed by one float32 multiply, bit for
 * bit.  dst may be audio or sc (same stride). */
int mi_compressor_bank_process_apply(mi_compressor_bank_t *bank, float *dst, const float *audio, const float *sc, size_t count,
                                     size_t dst_stride, size_t audio_stride, size_t sc_stride, void *stream);
/* curve(out, in, dots), :313-334: out = gain(|in|) |in| of every channel's curve, stateless; update_settings() first */
int mi_compressor_bank_curve(mi_compressor_bank_t *bank, float *out, const float *in, size_t dots, size_t out_stride,
                             size_t in_stride, void *stream);

/* ---- expander bank (envelope follower and one-knee gain curve with a floor or a ceiling) -------------------------------- */
/*
 * mi_expander_bank: `channels` x lsp::dspu::Expander (dynamics/Expander.h:40-283, src/main/dynamics/Expander.cpp), every
 * channel with settings and a mode of its own.  process() is the reference's: the Compressor's envelope follower (:252-284),
 * then Expander::amplification(float) (:375-407), which stands for dsp::uexpander_x1_gain / dexpander_x1_gain of the absent
 * lsp-dsp-lib.  Envelope, peak and hold counter are the reference's bit for bit in float32; the gain is within the bound
 * DESIGN.md section 3.12 derives.  State on the device, no positions: calls can be captured and replayed.  Inputs are
 * finite; subnormal envelopes are kept.  Rows of the sample buffers: [channels][stride].
 */
typedef struct mi_expander_bank mi_expander_bank_t;
enum mi_expander_mode { MI_EM_DOWNWARD = 0, MI_EM_UPWARD = 1 };                           /* expander_mode_t */
/* dsp::expander_knee_t of lsp-dsp-lib.  Upward: |x| is limited to threshold, above start the gain is exp(tilt[0] ln x +
 * tilt[1]) from end on and exp((herm[0] ln x + herm[1]) ln x + herm[2]) below it, otherwise 1.  Downward: 0 below
 * threshold, below end the tilt line up to start and the knee above it, otherwise 1. */
typedef struct { float start, end, threshold, herm[3], tilt[2]; } mi_expander_knee_t;
/* what update_settings() computes: fTauAttack, fTauRelease, fReleaseThresh as set, nHold, sExp, bUpward */
typedef struct { float tau_attack, tau_release, release_threshold; uint32_t hold; mi_expander_knee_t k; uint32_t upward; } mi_expander_params_t;
/* the setters' values: times in ms; mode is kept as the reference keeps it, upward or not */
typedef struct
{
    uint32_t sample_rate, mode;
    float attack_threshold, release_threshold, attack, release, hold, knee, ratio;
} mi_expander_settings_t;
/* update_settings(), :200-245, of one expander in host float32, with square_roots (:44-57) and the UPPER_ / LOWER_THRESHOLD
 * limits.  No device needed. */
int mi_expander_compute_params(const mi_expander_settings_t *settings, mi_expander_params_t *params);
/* construct(), :70-101: every channel UPWARD, ratio 1, everything else 0, an update pending */
int mi_expander_bank_create(mi_expander_bank_t **bank, uint32_t channels);
int mi_expander_bank_destroy(mi_expander_bank_t *bank);
/* The setters of one channel (:107-198): each returns early on an unchanged value.  set_hold limits to >= 0; nothing else
 * is limited (set_knee is not, unlike the Compressor's).  set_mode compares "upward or not", as the reference does. */
int mi_expander_bank_set_sample_rate(mi_expander_bank_t *bank, uint32_t channel, uint32_t sample_rate);
int mi_expander_bank_set_mode(mi_expander_bank_t *bank, uint32_t channel, uint32_t mode);
int mi_expander_bank_set_threshold(mi_expander_bank_t *bank, uint32_t channel, float attack, float release);
int mi_expander_bank_set_timings(mi_expander_bank_t *bank, uint32_t channel, float attack, float release);
int mi_expander_bank_set_hold(mi_expander_bank_t *bank, uint32_t channel, float hold);
int mi_expander_bank_set_knee(mi_expander_bank_t *bank, uint32_t channel, float knee);
int mi_expander_bank_set_ratio(mi_expander_bank_t *bank, uint32_t channel, float ratio);
/* as mi_compressor_bank_update_settings / _clear / _get_params / _get_state */
int mi_expander_bank_update_settings(mi_expander_bank_t *bank, void *stream);
int mi_expander_bank_clear(mi_expander_bank_t *bank, void *stream);
int mi_expander_bank_get_params(const mi_expander_bank_t *bank, uint32_t channel, mi_expander_params_t *params);
int mi_expander_bank_get_state(mi_expander_bank_t *bank, uint32_t channel, float *envelope, float *peak, uint32_t *hold,
                               void *stream);
/* process(out, env, in, samples), :247-292; gain or env may be the input rows (same stride); gain and env differ */
int mi_expander_bank_process(mi_expander_bank_t *bank, float *gain, float *env, const float *in, size_t count,
                             size_t gain_stride, size_t env_stride, size_t in_stride, void *stream);
/* dst = audio * gain(sc) in the same launch; dst may be audio or sc (same stride) */
int mi_expander_bank_process_apply(mi_expander_bank_t *bank, float *dst, const float *audio, const float *sc, size_t count,
                                   size_t dst_stride, size_t audio_stride, size_t sc_stride, void *stream);
/* curve(out, in, dots), as the scalar overload :333-365 states it, stateless; update_settings() first */
int mi_expander_bank_curve(mi_expander_bank_t *bank, float *out, const float *in, size_t dots, size_t out_stride,
                           size_t in_stride, void *stream);

/* ---- gate bank (envelope follower, two cubic curves and the hysteresis between them) ------------------------------------ */
/*
 * mi_gate_bank: `channels` x lsp::dspu::Gate (dynamics/Gate.h:34-288, src/main/dynamics/Gate.cpp), every channel with
 * settings of its own.  process() restates the block overload (:267-367): the follower without a release threshold, and per
 * sample the curve in force, open (0) or close (1).  When the envelope leaves the curve in force (above sCurves[0].sKnee.end
 * on curve 0, below sCurves[1].sKnee.start on curve 1) the reference runs the follower a second time on the same input
 * sample under the other curve; that sample's envelope and gain are the second step's.  The arithmetic is that of the
 * reference's out-of-place call whichever buffers alias.  ONE DIFFERENCE: a sample is stepped again at most once, then the
 * walk advances; with close start <= open end and taus in [0, 1] the reference never does more, with inverted thresholds
 * it may not return.  Unlike Gate::process, the bank's process entries apply pending settings first.
 * Envelope, peak, hold counter and curve index bit for bit; the gain within the bound section 3.13 derives.
 */
typedef struct mi_gate_bank mi_gate_bank_t;
/* dsp::gate_knee_t of lsp-dsp-lib: gain_start up to start, gain_end from end on, between them
 * exp(((herm[0] ln x + herm[1]) ln x + herm[2]) ln x + herm[3]) */
typedef struct { float start, end, gain_start, gain_end, herm[4]; } mi_gate_knee_t;
/* what update_settings() computes: fTauAttack, fTauRelease, nHold, sCurves[0..1].sKnee */
typedef struct { float tau_attack, tau_release; uint32_t hold, reserved; mi_gate_knee_t k[2]; } mi_gate_params_t;
/* the setters' values: [0] the open curve, [1] the close curve; times in ms */
typedef struct { uint32_t sample_rate; float threshold[2], zone[2], reduction, attack, release, hold; } mi_gate_settings_t;
/* update_settings(), :180-205, in host float32; interpolation::hermite_cubic with its double intermediates on float32
 * differences and products (interpolation.cpp:112-131).  A zone of 1 gives non-finite coefficients that no sample reaches.
 * No device needed. */
int mi_gate_compute_params(const mi_gate_settings_t *settings, mi_gate_params_t *params);
/* construct(), :41-74: both zones 1, everything else 0, curve 0, an update pending */
int mi_gate_bank_create(mi_gate_bank_t **bank, uint32_t channels);
int mi_gate_bank_destroy(mi_gate_bank_t *bank);
/* The setters of one channel (:80-178): early return on unchanged values; set_hold limits to >= 0, nothing else is limited */
int mi_gate_bank_set_sample_rate(mi_gate_bank_t *bank, uint32_t channel, uint32_t sample_rate);
int mi_gate_bank_set_threshold(mi_gate_bank_t *bank, uint32_t channel, float open, float close);
int mi_gate_bank_set_zone(mi_gate_bank_t *bank, uint32_t channel, float open, float close);
int mi_gate_bank_set_reduction(mi_gate_bank_t *bank, uint32_t channel, float reduction);
int mi_gate_bank_set_timings(mi_gate_bank_t *bank, uint32_t channel, float attack, float release);
int mi_gate_bank_set_hold(mi_gate_bank_t *bank, uint32_t channel, float hold);
int mi_gate_bank_update_settings(mi_gate_bank_t *bank, void *stream);
/* clear(): envelope, peak, hold counter and curve index to zero */
int mi_gate_bank_clear(mi_gate_bank_t *bank, void *stream);
int mi_gate_bank_get_params(const mi_gate_bank_t *bank, uint32_t channel, mi_gate_params_t *params);
/* fEnvelope, fPeak, nHoldCounter, nCurve of the channel (HOST memory, each may be NULL; waits for the stream) */
int mi_gate_bank_get_state(mi_gate_bank_t *bank, uint32_t channel, float *envelope, float *peak, uint32_t *hold,
                           uint32_t *curve, void *stream);
int mi_gate_bank_process(mi_gate_bank_t *bank, float *gain, float *env, const float *in, size_t count,
                         size_t gain_stride, size_t env_stride, size_t in_stride, void *stream);
int mi_gate_bank_process_apply(mi_gate_bank_t *bank, float *dst, const float *audio, const float *sc, size_t count,
                               size_t dst_stride, size_t audio_stride, size_t sc_stride, void *stream);
/* curve(out, in, dots, hyst), :207-226: the open curve, or with hyst != 0 the close curve, stateless */
int mi_gate_bank_curve(mi_gate_bank_t *bank, float *out, const float *in, size_t dots, int hyst, size_t out_stride,
                       size_t in_stride, void *stream);

/* ---- dynamic processor bank (envelope follower with level-dependent reaction times, curve through up to four dots) ------ */
/*
 * mi_dynproc_bank: `channels` x lsp::dspu::DynamicProcessor (dynamics/DynamicProcessor.h:42-333,
 * src/main/dynamics/DynamicProcessor.cpp), every channel with settings of its own.  process() is the reference's block overload
 * (:397-442): the follower over (fEnvelope, fPeak, nHoldCounter) whose tau is looked up per sample from the envelope BEFORE the
 * step (solve_reaction, :195-202), then the array reduction() (:562-584): |e| limited to [GAIN_AMP_MIN = 1e-6, 1e10], the sum
 * of spline_amp (:173-183) over the channel's splines in the reference's order, expf of it.  The scalar reduction(float), curve
 * and model limit at 1e-10 instead (FLOAT_SAT_M_INF); curve and model here are the array forms (:474-496, :518-540), which do
 * so too.  Envelope, peak and hold counter are the reference's bit for bit in float32; the gain is within the bound DESIGN.md
 * section 3.14 derives; no spline enabled gives exactly 1.  State on the device, no positions: calls can be captured and
 * replayed.  Inputs are finite.  Rows of the sample buffers: [channels][stride].
 */
typedef struct mi_dynproc_bank mi_dynproc_bank_t;
#define MI_DYNPROC_DOTS   4                                                                 /* DYNAMIC_PROCESSOR_DOTS */
#define MI_DYNPROC_RANGES 5                                                                 /* DYNAMIC_PROCESSOR_RANGES */
typedef struct { float input, output, knee; } mi_dynproc_dot_t;                             /* dyndot_t: a negative field is "off" */
/* spline_t (DynamicProcessor.h:49-58): up to knee_start makeup + pre_ratio (ln x - thresh), from knee_stop on makeup +
 * post_ratio (ln x - thresh), between them (herm[0] ln x + herm[1]) ln x + herm[2]; herm[3] is never written */
typedef struct { float pre_ratio, post_ratio, knee_start, knee_stop, thresh, makeup, herm[4]; } mi_dynproc_spline_t;
typedef struct { float level, tau; } mi_dynproc_reaction_t;                                 /* reaction_t, sorted by level */
/* what update_settings() computes: fCount[CT_SPLINES / CT_ATTACK / CT_RELEASE], nHold, vAttack, vRelease, vSplines; entries
 * from the count on are zero */
typedef struct
{
    uint32_t splines, attacks, releases, hold;
    mi_dynproc_reaction_t attack[MI_DYNPROC_RANGES], release[MI_DYNPROC_RANGES];
    mi_dynproc_spline_t spline[MI_DYNPROC_DOTS];
} mi_dynproc_params_t;
/* the setters' values: times in ms; a negative level switches the range above it off */
typedef struct
{
    uint32_t sample_rate;
    float hold, in_ratio, out_ratio;
    mi_dynproc_dot_t dot[MI_DYNPROC_DOTS];
    float attack_level[MI_DYNPROC_DOTS], release_level[MI_DYNPROC_DOTS];
    float attack_time[MI_DYNPROC_RANGES], release_time[MI_DYNPROC_RANGES];
} mi_dynproc_settings_t;
/* update_settings(), :339-395, of one processor in host float32 with sort_reactions (:204-227), sort_splines (:229-285) and
 * interpolation::hermite_quadratic (interpolation.cpp:103-109).  Two dots with one input divide by zero, as in the reference.
 * No device needed. */
int mi_dynproc_compute_params(const mi_dynproc_settings_t *settings, mi_dynproc_params_t *params);
/* construct(), :43-74: both ratios 1, everything else 0 -- so all four dots are ON at (0, 0, 0), which update_settings() cannot
 * evaluate to finite numbers (logf(0), 0 / 0), as in the reference: set every dot before use.  An update is pending. */
int mi_dynproc_bank_create(mi_dynproc_bank_t **bank, uint32_t channels);
int mi_dynproc_bank_destroy(mi_dynproc_bank_t *bank);
/* The setters of one channel (:80-171, :287-337): each returns early on an unchanged value; an id out of range is MI_EINVAL
 * (the reference ignores it).  set_hold limits to >= 0.  set_dot with dot == NULL switches the dot off (-1, -1, -1). */
int mi_dynproc_bank_set_sample_rate(mi_dynproc_bank_t *bank, uint32_t channel, uint32_t sample_rate);
int mi_dynproc_bank_set_in_ratio(mi_dynproc_bank_t *bank, uint32_t channel, float ratio);
int mi_dynproc_bank_set_out_ratio(mi_dynproc_bank_t *bank, uint32_t channel, float ratio);
int mi_dynproc_bank_set_dot(mi_dynproc_bank_t *bank, uint32_t channel, uint32_t id, const mi_dynproc_dot_t *dot);
int mi_dynproc_bank_set_attack_level(mi_dynproc_bank_t *bank, uint32_t channel, uint32_t id, float level);
int mi_dynproc_bank_set_release_level(mi_dynproc_bank_t *bank, uint32_t channel, uint32_t id, float level);
int mi_dynproc_bank_set_attack_time(mi_dynproc_bank_t *bank, uint32_t channel, uint32_t id, float time);
int mi_dynproc_bank_set_release_time(mi_dynproc_bank_t *bank, uint32_t channel, uint32_t id, float time);
int mi_dynproc_bank_set_hold(mi_dynproc_bank_t *bank, uint32_t channel, float hold);
/* as mi_compressor_bank_update_settings / _clear / _get_params / _get_state */
int mi_dynproc_bank_update_settings(mi_dynproc_bank_t *bank, void *stream);
int mi_dynproc_bank_clear(mi_dynproc_bank_t *bank, void *stream);
int mi_dynproc_bank_get_params(const mi_dynproc_bank_t *bank, uint32_t channel, mi_dynproc_params_t *params);
int mi_dynproc_bank_get_state(mi_dynproc_bank_t *bank, uint32_t channel, float *envelope, float *peak, uint32_t *hold,
                              void *stream);
/* process(out, env, in, samples), :397-442; gain or env may be the input rows (same stride); gain and env differ */
int mi_dynproc_bank_process(mi_dynproc_bank_t *bank, float *gain, float *env, const float *in, size_t count,
                            size_t gain_stride, size_t env_stride, size_t in_stride, void *stream);
/* dst = audio * gain(sc) in the same launch; dst may be audio or sc (same stride) */
int mi_dynproc_bank_process_apply(mi_dynproc_bank_t *bank, float *dst, const float *audio, const float *sc, size_t count,
                                  size_t dst_stride, size_t audio_stride, size_t sc_stride, void *stream);
/* curve(out, in, dots), :474-496, and model(out, in, dots), :518-540 (the curve without its knees: spline_model, :185-193):
 * out = gain(|in|) |in| with |in| limited to [1e-10, 1e10], stateless; update_settings() first */
int mi_dynproc_bank_curve(mi_dynproc_bank_t *bank, float *out, const float *in, size_t dots, size_t out_stride,
                          size_t in_stride, void *stream);
int mi_dynproc_bank_model(mi_dynproc_bank_t *bank, float *out, const float *in, size_t dots, size_t out_stride,
                          size_t in_stride, void *stream);

/* ---- limiter bank (look-ahead peak search and multiplicative gain patches) ----------------------------------------------- */
/*
 * mi_limiter_bank: `channels` x lsp::dspu::Limiter (dynamics/Limiter.h:55-381, src/main/dynamics/Limiter.cpp), every channel
 * with settings and mode of its own; the maximum look-ahead is the bank's.  process() is the reference's (:695-784): the call is
 * cut into chunks of at most 8192 samples counted from its first sample; per chunk the gain window (ML = nMaxLookahead behind,
 * the chunk, 3 ML ahead) takes ones at its end, the ALR follower if enabled, and then patches: the first index of the maximum
 * of gain |sc| is found, and while it exceeds the threshold the gains around it are multiplied by 1 - k shape(t), the knee
 * lowered by 0.9886 after every 32 patches.  The gain, nHead, the ALR envelope and the number of patches are the bits of that
 * loop in float32 (every product, sum and quotient rounded on its own) with shape(t) from the host's table
 * (mi_limiter_compute_patch) and dsp::max_index / dsp::abs_mul3 of the absent lsp-dsp-lib taken as "first index of the
 * maximum" and a |b| (DESIGN.md sections 3.15 and 4).  TWO DIFFERENCES: the patch loop of a chunk of n samples ends after 2 n
 * patches at the latest and then sets the channel's sticky overrun flag (the reference does not return on NaN); and a patch
 * that reaches outside the window, which happens only with a look-ahead under 8 samples, is cut at the window's ends, where the
 * reference multiplies floats it never reads again (or, with ML < 8, floats outside its allocation).  The gain window, nHead,
 * the ALR envelope, the audio history of process_apply and the counters live on the device: calls can be captured and
 * replayed.  Inputs are finite.  Unlike Limiter::process, the results depend on how the stream is cut into calls exactly as the
 * reference's do.  Rows of the sample buffers: [channels][stride].
 */
typedef struct mi_limiter_bank mi_limiter_bank_t;
#define MI_LIMITER_MAX_LOOKAHEAD 4064   /* the largest nMaxLookahead in samples: window, |sc| and gain |sc| of a chunk fill the LDS */
#define MI_LIMITER_MODES 12             /* limiter_mode_t: LM_HERM_, LM_EXP_, LM_LINE_ x THIN, WIDE, TAIL, DUCK */
/* the setters' values: times in ms; threshold is fReqThreshold; alr_knee as set_alr_knee stored it */
typedef struct
{
    uint32_t sample_rate, mode;
    float threshold, lookahead, attack, release, knee, alr_attack, alr_release, alr_knee;
} mi_limiter_settings_t;
/* what update_settings() computes: nLookahead; nAttack, nPlane, nRelease, nMiddle, vAttack, vRelease of sSat / sExp / sLine
 * (entries the mode does not write are 0); fThreshold; sALR.fKS, fKE, fGain, vHermite, fTauAttack, fTauRelease */
typedef struct
{
    uint32_t lookahead, mode;
    int32_t attack, plane, release, middle;
    float v_attack[4], v_release[4];
    float threshold, ks, ke, gain, hermite[3], tau_attack, tau_release;
} mi_limiter_params_t;
/* update_settings(), :396-548, with init_sat / init_exp / init_line (:278-394) in host float32; interpolation::hermite_cubic
 * and ::exponent with their double stretches (interpolation.cpp:112-131, :224-230).  As in the reference init_exp compares
 * the mode with the LM_HERM_ values, so the four LM_EXP_ modes share the WIDE widths.  No device needed. */
int mi_limiter_compute_params(const mi_limiter_settings_t *settings, mi_limiter_params_t *params);
/* shape[t], t in [0, params->release): what apply_*_patch (:609-673) multiplies amp with, in float32, every operation rounded
 * on its own, expf the host's; exactly 1 on the plane.  capacity: floats at shape; MI_EINVAL if params->release exceeds it. */
int mi_limiter_compute_patch(const mi_limiter_params_t *params, float *shape, size_t capacity);
/* construct() and init(max_sample_rate, max_lookahead_ms), :47-109, of every channel: gains 1, nHead 0, an update pending.
 * MI_EINVAL if millis_to_samples(max_sample_rate, max_lookahead_ms) exceeds MI_LIMITER_MAX_LOOKAHEAD. */
int mi_limiter_bank_create(mi_limiter_bank_t **bank, uint32_t channels, uint32_t max_sample_rate, float max_lookahead_ms);
int mi_limiter_bank_destroy(mi_limiter_bank_t *bank);
/* The setters of one channel (:111-229): early return on unchanged values; set_lookahead limits to the maximum;
 * set_threshold without `immediate` leaves fThreshold for update_settings() to lower (which scales ML gains);
 * set_alr_knee stores 1 / knee for a knee above 1; set_alr(0) zeroes the envelope before the next launch */
int mi_limiter_bank_set_sample_rate(mi_limiter_bank_t *bank, uint32_t channel, uint32_t sample_rate);
int mi_limiter_bank_set_mode(mi_limiter_bank_t *bank, uint32_t channel, uint32_t mode);
int mi_limiter_bank_set_threshold(mi_limiter_bank_t *bank, uint32_t channel, float threshold, int immediate);
int mi_limiter_bank_set_attack(mi_limiter_bank_t *bank, uint32_t channel, float attack);
int mi_limiter_bank_set_release(mi_limiter_bank_t *bank, uint32_t channel, float release);
int mi_limiter_bank_set_lookahead(mi_limiter_bank_t *bank, uint32_t channel, float lookahead);
int mi_limiter_bank_set_knee(mi_limiter_bank_t *bank, uint32_t channel, float knee);
int mi_limiter_bank_set_alr(mi_limiter_bank_t *bank, uint32_t channel, int enable);
int mi_limiter_bank_set_alr_attack(mi_limiter_bank_t *bank, uint32_t channel, float attack);
int mi_limiter_bank_set_alr_release(mi_limiter_bank_t *bank, uint32_t channel, float release);
int mi_limiter_bank_set_alr_knee(mi_limiter_bank_t *bank, uint32_t channel, float knee);
/* update_settings(), :396-548, of every channel with changes, its work on the gain window included; not during a capture */
int mi_limiter_bank_update_settings(mi_limiter_bank_t *bank, void *stream);
/* every channel as after create(): gains 1, nHead 0, envelope 0, audio history 0, counters and overrun flag 0 */
int mi_limiter_bank_clear(mi_limiter_bank_t *bank, void *stream);
int mi_limiter_bank_get_params(const mi_limiter_bank_t *bank, uint32_t channel, mi_limiter_params_t *params);
/* the channel's shape table as the device has it (HOST memory, *count entries; capacity: floats at shape; waits for the
 * stream; not during a capture) */
int mi_limiter_bank_get_patch(mi_limiter_bank_t *bank, uint32_t channel, float *shape, size_t capacity, uint32_t *count,
                              void *stream);
/* nLookahead of the channel after pending settings */
int mi_limiter_bank_get_latency(mi_limiter_bank_t *bank, uint32_t channel, uint32_t *latency);
/* nHead, sALR.fEnvelope, the patches and the chunks of the last call, the sticky overrun flag (HOST memory, each may be NULL;
 * waits for the stream; not during a capture) */
int mi_limiter_bank_get_state(mi_limiter_bank_t *bank, uint32_t channel, uint32_t *head, float *envelope, uint32_t *patches,
                              uint32_t *chunks, uint32_t *overrun, void *stream);
/* process(gain, sc, samples), :695-784; gain may be the sc rows (same stride) */
int mi_limiter_bank_process(mi_limiter_bank_t *bank, float *gain, const float *sc, size_t count, size_t gain_stride,
                            size_t sc_stride, void *stream);
/* dst[i] = audio_stream[i - nLookahead] * gain[i] in the same launch: the Delay and the multiply a caller puts behind
 * process().  The last ML samples of every channel's audio are kept between calls (zero at the start); a changed look-ahead
 * moves the read offset at the next call.  dst may be audio or sc (same stride). */
int mi_limiter_bank_process_apply(mi_limiter_bank_t *bank, float *dst, const float *audio, const float *sc, size_t count,
                                  size_t dst_stride, size_t audio_stride, size_t sc_stride, void *stream);

/* ---- autogain bank (loudness gain riding: two levels in, one VCA gain out) ------------------------------------------------ */
/*
 * mi_autogain_bank: `channels` x lsp::dspu::AutoGain (dynamics/AutoGain.h:42-303, src/main/dynamics/AutoGain.cpp), every channel
 * with settings of its own: what takes the loudness meter's per-sample output.  process() is the reference's (:223-296): a
 * serial recurrence over (fCurrGain, fOutGain, the two surge flags) with up to five divisions per sample and no transcendental,
 * so the gain and the state are the reference's bit for bit in float32 (every product, sum and quotient rounded on its own,
 * division correctly rounded, subnormals kept).  The state lives on the device; the bank has no positions, so its process calls
 * can be captured into a graph and replayed.  lexp > 0 and every input is finite: NaN is out of scope, and a gain that has
 * underflowed to zero makes 0 / 0 here as it does in the reference.  Rows of the sample buffers: [channels][stride].
 */
typedef struct mi_autogain_bank mi_autogain_bank_t;
/* AutoGain::flags_t without F_UPDATE: two switches and the two surge flags of the state */
enum mi_autogain_flags { MI_AG_QUICK_AMP = 2, MI_AG_MAX_GAIN = 4, MI_AG_SURGE_UP = 8, MI_AG_SURGE_DOWN = 16 };
/* AutoGain::compressor_t: x below x1, t above x2, between them ((a v + b) v + c v) + d of v = x - x1, as
 * eval_curve (:197-206) writes it */
typedef struct { float x1, x2, t, a, b, c, d; } mi_autogain_curve_t;
/* the setters' values: speeds in dB/s, silence, deviation and max_gain as gains, flags of QUICK_AMP | MAX_GAIN */
typedef struct
{
    uint32_t sample_rate, flags;
    float short_grow, short_fall, long_grow, long_fall, silence, deviation, max_gain;
} mi_autogain_settings_t;
/* what update() computes (sShort.fKGrow, fKFall, sLong.fKGrow, fKFall, sShortComp, sOutComp) and, as set, fSilence,
 * fDeviation, fMaxGain and the two switches */
typedef struct
{
    float short_kgrow, short_kfall, long_kgrow, long_kfall;
    mi_autogain_curve_t short_comp, out_comp;
    float silence, deviation, max_gain;
    uint32_t flags;
} mi_autogain_params_t;
/* update(), :155-173, with calc_compressor (:180-195) in host float32 (expf, sqrtf; ksr and c.a through double as the
 * reference's expressions go).  No device needed. */
int mi_autogain_compute_params(const mi_autogain_settings_t *settings, mi_autogain_params_t *params);
/* construct(), :43-66: silence -72 dB, deviation +6 dB, max gain +12 dB, both gains 1, no switch, an update pending */
int mi_autogain_bank_create(mi_autogain_bank_t **bank, uint32_t channels);
int mi_autogain_bank_destroy(mi_autogain_bank_t *bank);
/* The setters of one channel (:90-153, :175-178, AutoGain.h:166-215).  The speeds (limited to >= 0), the deviation (to >= 1)
 * and the sample rate return early on an unchanged value and otherwise leave an update pending.  set_silence_threshold (limited
 * to >= 0), set_max_gain (to >= 0), set_max_gain_control (the reference's set_max_gain(value, enable)), enable_max_gain and
 * enable_quick_amplifier raise no update, as in the reference: their values go into the parameter table as they are and reach
 * the device with the next update_settings() or process entry. */
int mi_autogain_bank_set_sample_rate(mi_autogain_bank_t *bank, uint32_t channel, uint32_t sample_rate);
int mi_autogain_bank_set_silence_threshold(mi_autogain_bank_t *bank, uint32_t channel, float threshold);
int mi_autogain_bank_set_deviation(mi_autogain_bank_t *bank, uint32_t channel, float deviation);
int mi_autogain_bank_set_short_grow(mi_autogain_bank_t *bank, uint32_t channel, float value);
int mi_autogain_bank_set_short_fall(mi_autogain_bank_t *bank, uint32_t channel, float value);
int mi_autogain_bank_set_short_speed(mi_autogain_bank_t *bank, uint32_t channel, float grow, float fall);
int mi_autogain_bank_set_long_grow(mi_autogain_bank_t *bank, uint32_t channel, float value);
int mi_autogain_bank_set_long_fall(mi_autogain_bank_t *bank, uint32_t channel, float value);
int mi_autogain_bank_set_long_speed(mi_autogain_bank_t *bank, uint32_t channel, float grow, float fall);
int mi_autogain_bank_set_max_gain(mi_autogain_bank_t *bank, uint32_t channel, float value);
int mi_autogain_bank_set_max_gain_control(mi_autogain_bank_t *bank, uint32_t channel, float value, int enable);
int mi_autogain_bank_enable_max_gain(mi_autogain_bank_t *bank, uint32_t channel, int enable);
int mi_autogain_bank_enable_quick_amplifier(mi_autogain_bank_t *bank, uint32_t channel, int enable);
/* update() of every channel with an update pending; the changed stretch of the parameter table goes to the device (and the
 * call waits for it).  The process entries run it first.  On a stream being captured a pending upload is refused (MI_ESTATE) */
int mi_autogain_bank_update_settings(mi_autogain_bank_t *bank, void *stream);
/* The channel's parameter table entry (HOST memory); fCurrGain, fOutGain and nFlags without F_UPDATE (the switches as set,
 * the surge flags of the state) as the work enqueued on `stream` leaves them (HOST memory, each may be NULL; waits for the
 * stream; not during a capture) */
int mi_autogain_bank_get_params(const mi_autogain_bank_t *bank, uint32_t channel, mi_autogain_params_t *params);
int mi_autogain_bank_get_state(mi_autogain_bank_t *bank, uint32_t channel, float *curr_gain, float *out_gain, uint32_t *flags,
                               void *stream);
/* process(vca, llong, lshort, lexp, count), :278-286.  vca may be any of the three input rows (same stride). */
int mi_autogain_bank_process(mi_autogain_bank_t *bank, float *vca, const float *llong, const float *lshort, const float *lexp,
                             size_t count, size_t vca_stride, size_t long_stride, size_t short_stride, size_t exp_stride,
                             void *stream);
/* process(vca, llong, lshort, float lexp, count), :288-296: the expected level of channel ch is levels[ch], read from DEVICE
 * memory by the launch, so that a captured call replays with new levels */
int mi_autogain_bank_process_level(mi_autogain_bank_t *bank, float *vca, const float *llong, const float *lshort,
                                   const float *levels, size_t count, size_t vca_stride, size_t long_stride, size_t short_stride,
                                   void *stream);
/* dst = audio * vca in the same launch: process() followed by one float32 multiply, bit for bit.  dst may be audio or any of
 * the three level rows (same stride). */
int mi_autogain_bank_process_apply(mi_autogain_bank_t *bank, float *dst, const float *audio, const float *llong,
                                   const float *lshort, const float *lexp, size_t count, size_t dst_stride, size_t audio_stride,
                                   size_t long_stride, size_t short_stride, size_t exp_stride, void *stream);

/*
 * mi_simple_autogain_bank: `channels` x lsp::dspu::SimpleAutoGain (dynamics/SimpleAutoGain.h:41-212,
 * src/main/dynamics/SimpleAutoGain.cpp): one measured level in, the gain grows by fKGrow below the threshold, falls by fKFall
 * above it, stays where the two are equal, and is limited with lsp_limit(g, min, max) after every sample.  Bit for bit in
 * float32, subnormal gains kept.  fCurrGain lives on the device.  set_max_gain, set_min_gain and set_gain change fCurrGain at
 * once in the reference (lsp_min, lsp_max, lsp_limit); here they are recorded IN ORDER and applied by the next process launch
 * ahead of its first sample (get_state applies them to what it read); with min > max lsp_limit is no clamp, so nothing is
 * merged.  Sending them is an upload: refused on a stream being captured (MI_ESTATE).  Inputs are finite.
 */
typedef struct mi_simple_autogain_bank mi_simple_autogain_bank_t;
typedef struct { uint32_t sample_rate; float grow, fall, threshold, min_gain, max_gain; } mi_simple_autogain_settings_t;
/* fKGrow, fKFall as update() computes them; fThreshold, fMinGain, fMaxGain as set */
typedef struct { float kgrow, kfall, threshold, min_gain, max_gain; } mi_simple_autogain_params_t;
/* update(), :142-153, in host float32.  No device needed. */
int mi_simple_autogain_compute_params(const mi_simple_autogain_settings_t *settings, mi_simple_autogain_params_t *params);
/* construct(), :43-56: gain 1, min gain 1e-6, max gain 1, everything else 0, an update pending */
int mi_simple_autogain_bank_create(mi_simple_autogain_bank_t **bank, uint32_t channels);
int mi_simple_autogain_bank_destroy(mi_simple_autogain_bank_t *bank);
/* The setters of one channel (:68-140): sample rate, grow, fall and speed leave an update pending unless unchanged; the gain
 * limits return early on unchanged values and otherwise act on fCurrGain as said above; set_threshold just sets */
int mi_simple_autogain_bank_set_sample_rate(mi_simple_autogain_bank_t *bank, uint32_t channel, uint32_t sample_rate);
int mi_simple_autogain_bank_set_grow(mi_simple_autogain_bank_t *bank, uint32_t channel, float value);
int mi_simple_autogain_bank_set_fall(mi_simple_autogain_bank_t *bank, uint32_t channel, float value);
int mi_simple_autogain_bank_set_speed(mi_simple_autogain_bank_t *bank, uint32_t channel, float grow, float fall);
int mi_simple_autogain_bank_set_max_gain(mi_simple_autogain_bank_t *bank, uint32_t channel, float value);
int mi_simple_autogain_bank_set_min_gain(mi_simple_autogain_bank_t *bank, uint32_t channel, float value);
int mi_simple_autogain_bank_set_gain(mi_simple_autogain_bank_t *bank, uint32_t channel, float min, float max);
int mi_simple_autogain_bank_set_threshold(mi_simple_autogain_bank_t *bank, uint32_t channel, float threshold);
/* as mi_autogain_bank_update_settings / _get_params; fCurrGain of the channel with the recorded limit changes applied */
int mi_simple_autogain_bank_update_settings(mi_simple_autogain_bank_t *bank, void *stream);
int mi_simple_autogain_bank_get_params(const mi_simple_autogain_bank_t *bank, uint32_t channel, mi_simple_autogain_params_t *params);
int mi_simple_autogain_bank_get_state(mi_simple_autogain_bank_t *bank, uint32_t channel, float *curr_gain, void *stream);
/* process(dst, src, count), :155-175; dst may be src (same stride) */
int mi_simple_autogain_bank_process(mi_simple_autogain_bank_t *bank, float *dst, const float *src, size_t count,
                                    size_t dst_stride, size_t src_stride, void *stream);

/* ---- sidechain bank (source selection, pre-amplification and the peak / RMS / low-pass / uniform detectors) ------------- */
/*
 * mi_sidechain_bank: `channels` x lsp::dspu::Sidechain (util/Sidechain.h:59-205, src/main/util/Sidechain.cpp), every channel
 * with settings of its own: what produces the signal a compressor bank takes.  process() is the reference's block overload
 * (:439-554): a source out of one or two inputs (:183-333), its magnitude times the gain, pushed into the channel's ring of
 * capacity max(millis_to_samples(sr, max_reactivity), 1) + 0x200, and one of four detectors over it; every 0x2000 samples
 * fRmsValue is formed anew from the ring (refresh_processing, :144-181, with its two partial sums where the window wraps).
 * out, fRmsValue, nRefresh and the ring position are the reference's bit for bit in float32 (each product and each sum rounds
 * once, the square root is correctly rounded); the sums of the refresh are taken serially, oldest sample first (DESIGN.md
 * section 4).  Ring, fRmsValue, nRefresh and the ring position live on the device; the bank has no host positions, so its
 * process calls can be captured into a graph and replayed.  Inputs are finite: NaN is out of scope.  Subnormals are kept.
 * The magnitude of a negative zero is +0 (fabsf), where the class's scalar text, (s < 0.0f) ? -s : s (:435), keeps -0: in PEAK
 * mode the output's sign bit differs there.  lsp-dsp-lib's abs1 / abs2 are not in the reference tree, so this is unpinned.
 * Rows of the sample buffers: [channels][stride].
 */
typedef struct mi_sidechain_bank mi_sidechain_bank_t;
enum mi_sidechain_source { MI_SCS_MIDDLE = 0, MI_SCS_SIDE = 1, MI_SCS_LEFT = 2, MI_SCS_RIGHT = 3, MI_SCS_AMIN = 4, MI_SCS_AMAX = 5 };
enum mi_sidechain_mode { MI_SCM_PEAK = 0, MI_SCM_RMS = 1, MI_SCM_LPF = 2, MI_SCM_UNIFORM = 3 };
enum mi_sidechain_stereo_mode { MI_SCSM_STEREO = 0, MI_SCSM_MIDSIDE = 1 };
enum mi_sidechain_flags { MI_SCF_MIDSIDE = 1, MI_SCF_UPDATE = 2, MI_SCF_CLEAR = 4 };        /* Sidechain::flags_t */
/* nReactivity, fTau, 1.0f / nReactivity and the ring's capacity as update_settings() and set_sample_rate() compute them;
 * nMode, nSource, nFlags and fGain as set */
typedef struct { uint32_t reactivity; float tau, interval; uint32_t capacity, mode, source, flags; float gain; } mi_sidechain_params_t;
/* The arithmetic of update_settings() (:119-131) and of set_sample_rate() (:88-93) in host float32: reactivity, tau, interval
 * and capacity; mode, source and flags 0, gain 1.  A reactivity outside [0, max_reactivity] is MI_EINVAL.  No device needed. */
int mi_sidechain_compute_params(uint32_t sample_rate, float max_reactivity, float reactivity, mi_sidechain_params_t *params);
/* init(inputs, max_reactivity), :67-86, of every channel: MIDDLE, RMS, gain 1, sample rate and reactivity 0, an update and
 * a clear pending.  inputs: 1 or 2 */
int mi_sidechain_bank_create(mi_sidechain_bank_t **bank, uint32_t channels, uint32_t inputs, float max_reactivity_ms);
int mi_sidechain_bank_destroy(mi_sidechain_bank_t *bank);
/* The setters of one channel with the reference's rules (:88-117, Sidechain.h:146-175): set_sample_rate re-makes the ring
 * (zeroed, position 0) and raises UPDATE and CLEAR; set_reactivity ignores an unchanged value and values outside
 * [0, max_reactivity] and raises UPDATE (which forces a refresh at the next sample); set_sample_rate also takes the channel
 * back to the stereo mode STEREO, as the reference's assignment to nFlags does (:91); set_stereo_mode raises CLEAR when the
 * mode changes; set_mode zeroes fRmsValue WITHOUT a refresh when the mode changes; set_source and set_gain just set.
 * Nothing reaches the device before update_settings().  A source above AMAX, a mode above UNIFORM and a stereo mode above
 * MIDSIDE are MI_EINVAL. */
int mi_sidechain_bank_set_sample_rate(mi_sidechain_bank_t *bank, uint32_t channel, uint32_t sample_rate);
int mi_sidechain_bank_set_reactivity(mi_sidechain_bank_t *bank, uint32_t channel, float reactivity);
int mi_sidechain_bank_set_stereo_mode(mi_sidechain_bank_t *bank, uint32_t channel, uint32_t mode);
int mi_sidechain_bank_set_source(mi_sidechain_bank_t *bank, uint32_t channel, uint32_t source);
int mi_sidechain_bank_set_mode(mi_sidechain_bank_t *bank, uint32_t channel, uint32_t mode);
int mi_sidechain_bank_set_gain(mi_sidechain_bank_t *bank, uint32_t channel, float gain);
/* clear(), :114-117: raises CLEAR of one channel, or of every channel (channel = UINT32_MAX).  At update_settings() it zeroes
 * fRmsValue, nRefresh and the ring's samples; the ring position stays, as in the reference. */
int mi_sidechain_bank_clear(mi_sidechain_bank_t *bank, uint32_t channel);
/* update_settings(), :119-142, of every channel with something pending: the changed stretch of the parameter table and the
 * changed state go to the device (and the call waits for them); rings grow, keeping the other channels' samples, when a
 * sample rate asks for more.  The process entries run it first.  On a stream being captured pending work is refused
 * (MI_ESTATE): call it before the capture. */
int mi_sidechain_bank_update_settings(mi_sidechain_bank_t *bank, void *stream);
/* The channel's parameters as the last update_settings() left them, flags with what is pending now (HOST memory); fRmsValue,
 * nRefresh and the ring position (RawRingBuffer::position()) as the work enqueued on `stream` leaves them (HOST memory, each
 * may be NULL; waits for the stream).  The position is 0 only before the first sample of a ring: after samples it lies in
 * (0, capacity], AT the capacity where a call ended at the ring's end (RawRingBuffer.cpp:106-125) */
int mi_sidechain_bank_get_params(const mi_sidechain_bank_t *bank, uint32_t channel, mi_sidechain_params_t *params);
int mi_sidechain_bank_get_state(mi_sidechain_bank_t *bank, uint32_t channel, float *rms_value, uint32_t *refresh, uint32_t *position,
                                void *stream);
/* process(out, in, samples), :439-554.  in1: the second input's rows, NULL for a bank of one input; in0 == NULL: silence, which
 * still runs through gain, ring and detector.  out may be in0 or in1 (same stride). */
int mi_sidechain_bank_process(mi_sidechain_bank_t *bank, float *out, const float *in0, const float *in1, size_t count,
                              size_t out_stride, size_t in0_stride, size_t in1_stride, void *stream);
/* The two halves of process() for a caller with a pre-equalizer between them: premix() writes the SIGNED selected source
 * (psmin3 / psmax3 where process() takes pamin3 / pamax3), stateless; process_premixed() runs magnitude, gain, ring and detector
 * on such rows.  process() equals premix() followed by process_premixed() bit for bit.  out may be an input (same stride). */
int mi_sidechain_bank_premix(mi_sidechain_bank_t *bank, float *out, const float *in0, const float *in1, size_t count,
                             size_t out_stride, size_t in0_stride, size_t in1_stride, void *stream);
int mi_sidechain_bank_process_premixed(mi_sidechain_bank_t *bank, float *out, const float *in, size_t count, size_t out_stride,
                                       size_t in_stride, void *stream);

/* ---- stereo-field meters: correlometer and panometer banks --------------------------------------------------------------- */
/*
 * mi_correlometer_bank: `channels` x lsp::dspu::Correlometer (meters/Correlometer.h, src/main/meters/Correlometer.cpp), every
 * channel with a period of its own: the normalised correlation of two rows, out = v / sqrt(a * b) over a sliding window of
 * `period` samples (0 where a * b < 1e-10), v, a, b the window sums of x*y, x*x, y*y.  Per channel two rings of
 * align(max_period + 0x400, 0x40) samples; per sample each sum takes in the head's term and gives up the tail's
 * (sum += head - tail: product, product, difference, sum), and every `period` samples the three sums are formed anew from the
 * rings, serially, oldest sample first, in two partial sums where the window wraps in the ring.  out,
 * the sums, nHead and nWindow are the reference's bit for bit in float32; there is no clamp to [-1, 1], as there is none in the
 * reference.  Rings, sums, nHead and nWindow live on the device: no host positions, so process calls can be captured into a
 * graph and replayed.  Inputs are finite: NaN is out of scope.  Subnormals are kept.  Rows: [channels][stride].
 */
typedef struct mi_correlometer_bank mi_correlometer_bank_t;
typedef struct { uint32_t period, capacity, max_period; } mi_correlometer_params_t;
typedef struct { float v, a, b; uint32_t head, window; } mi_correlometer_state_t;          /* sCorr, nHead, nWindow */
/* init(max_period) of every channel: period 0, nHead 0, sums and rings zero */
int mi_correlometer_bank_create(mi_correlometer_bank_t **bank, uint32_t channels, uint32_t max_period);
int mi_correlometer_bank_destroy(mi_correlometer_bank_t *bank);
/* set_period(): clamped to max_period; an unchanged value is ignored, a changed one makes the next process() start with a
 * refresh (nWindow = nPeriod).  A period of 0 is MI_EINVAL: the reference's process() never ends with it. */
int mi_correlometer_bank_set_period(mi_correlometer_bank_t *bank, uint32_t channel, uint32_t period);
/* clear() of one channel, or of every channel (channel = UINT32_MAX): rings and sums zero, nHead = nPeriod; nWindow stays */
int mi_correlometer_bank_clear(mi_correlometer_bank_t *bank, uint32_t channel);
/* What the setters left goes to the device (and the call waits for it).  process() runs it first.  On a stream being captured
 * pending work is refused (MI_ESTATE): call it before the capture. */
int mi_correlometer_bank_update_settings(mi_correlometer_bank_t *bank, void *stream);
/* The channel's settings as set (HOST memory); its state as the work enqueued on `stream` leaves it (HOST memory; waits for
 * the stream; not on a stream being captured: MI_ESTATE).  set_state writes the state as given (nHead modulo the capacity,
 * nWindow at most the period) after the pending work, zero_rings != 0: with both rings zeroed. */
int mi_correlometer_bank_get_params(const mi_correlometer_bank_t *bank, uint32_t channel, mi_correlometer_params_t *params);
int mi_correlometer_bank_get_state(mi_correlometer_bank_t *bank, uint32_t channel, mi_correlometer_state_t *state, void *stream);
int mi_correlometer_bank_set_state(mi_correlometer_bank_t *bank, uint32_t channel, const mi_correlometer_state_t *state,
                                   uint32_t zero_rings, void *stream);
/* process(dst, a, b, count).  out may be a or b (same stride).  While a channel still has period 0: MI_ESTATE naming it, and
 * nothing is launched. */
int mi_correlometer_bank_process(mi_correlometer_bank_t *bank, float *out, const float *a, const float *b, size_t count,
                                 size_t out_stride, size_t a_stride, size_t b_stride, void *stream);

/*
 * mi_panometer_bank: `channels` x lsp::dspu::Panometer (meters/Panometer.h, src/main/meters/Panometer.cpp): the balance of two
 * rows out of the window sums va, vb of their squares, which are what the two rings hold.  Per sample v = (v + head) - tail,
 * two roundings; every `period` samples both sums are formed anew from the rings as in the correlometer bank.  Linear law:
 * sl = sqrt(|va| * norm), sr = sqrt(|vb| * norm), out = sr / (sl + sr) where sl + sr > 1e-18, the default otherwise; equal
 * power: the same without the roots and with 1e-36.  norm = 1 / period.  Bit for bit the reference's in float32 (the roots and
 * the quotient correctly rounded).  Device state, capture, inputs and rows as for the correlometer bank.
 */
typedef struct mi_panometer_bank mi_panometer_bank_t;
enum mi_pan_law { MI_PAN_LAW_LINEAR = 0, MI_PAN_LAW_EQUAL_POWER = 1 };                     /* pan_law_t */
typedef struct { uint32_t period, capacity, max_period, law; float norm, default_pan; } mi_panometer_params_t;
typedef struct { float value_a, value_b; uint32_t head, window; } mi_panometer_state_t;    /* fValueA, fValueB, nHead, nWindow */
/* init(max_period) of every channel: period 0, equal power, default 0.5 */
int mi_panometer_bank_create(mi_panometer_bank_t **bank, uint32_t channels, uint32_t max_period);
int mi_panometer_bank_destroy(mi_panometer_bank_t *bank);
/* set_period(): clamped; an unchanged value is ignored, a changed one zeroes both sums, sets norm and makes the next sample
 * start with a refresh.  0 is MI_EINVAL.  set_pan_law (a law above EQUAL_POWER is MI_EINVAL) and set_default_pan just set. */
int mi_panometer_bank_set_period(mi_panometer_bank_t *bank, uint32_t channel, uint32_t period);
int mi_panometer_bank_set_pan_law(mi_panometer_bank_t *bank, uint32_t channel, uint32_t law);
int mi_panometer_bank_set_default_pan(mi_panometer_bank_t *bank, uint32_t channel, float default_pan);
/* clear(): the rings zero, nHead = nPeriod; the sums and nWindow stay */
int mi_panometer_bank_clear(mi_panometer_bank_t *bank, uint32_t channel);
int mi_panometer_bank_update_settings(mi_panometer_bank_t *bank, void *stream);
int mi_panometer_bank_get_params(const mi_panometer_bank_t *bank, uint32_t channel, mi_panometer_params_t *params);
int mi_panometer_bank_get_state(mi_panometer_bank_t *bank, uint32_t channel, mi_panometer_state_t *state, void *stream);
int mi_panometer_bank_set_state(mi_panometer_bank_t *bank, uint32_t channel, const mi_panometer_state_t *state, uint32_t zero_rings,
                                void *stream);
int mi_panometer_bank_process(mi_panometer_bank_t *bank, float *out, const float *a, const float *b, size_t count,
                              size_t out_stride, size_t a_stride, size_t b_stride, void *stream);

/* ---- peak hold/decay meter and surge protector banks ---------------------------------------------------------------------- */
/*
 * mi_peakmeter_bank: `channels` x lsp::dspu::PeakMeter (meters/PeakMeter.h, src/main/meters/PeakMeter.cpp), every channel with
 * settings of its own.  Per sample, with s = |x|: s >= peak: peak = s and the hold counter restarts; otherwise the counter runs
 * down; otherwise peak *= tau.  fPeak and nCounter live on the device: calls can be captured into a graph and replayed.  The
 * peak is the reference's bit for bit in float32; NaN and Inf samples behave as there; subnormals are kept.  A fresh meter has a
 * release of 0 and with it tau = expf(-inf) = 0: the peak drops to 0 once the hold has run out.  Rows: [channels][stride].
 */
typedef struct mi_peakmeter_bank mi_peakmeter_bank_t;
/* fTau, nHold; factor = expf(logf(fTau) * float(count)), formed on the host for the `count` of the last process_value() */
typedef struct { float tau; uint32_t hold; float factor; uint32_t count; } mi_peakmeter_params_t;
typedef struct { float peak; uint32_t counter; } mi_peakmeter_state_t;                     /* fPeak, nCounter */
/* update_settings() of one meter without a bank or a device (times in milliseconds): fTau and nHold in host float32 with the C
 * library's expf and logf, as the reference forms them; the factor is that of count 0.  MI_EINVAL where nHold is undefined (below). */
int mi_peakmeter_compute_params(uint32_t sample_rate, float hold, float release, mi_peakmeter_params_t *params);
int mi_peakmeter_bank_create(mi_peakmeter_bank_t **bank, uint32_t channels);               /* construct(): hold 5 ms, release 0 */
int mi_peakmeter_bank_destroy(mi_peakmeter_bank_t *bank);
/* The setters (times in milliseconds); an unchanged value is ignored.  nHold = uint32_t(millis_to_samples(rate, hold)) is
 * undefined in the reference for a product that is negative, NaN or at least 2^32: a setter that would leave such a pair of rate
 * and hold time is MI_EINVAL and changes nothing. */
int mi_peakmeter_bank_set_sample_rate(mi_peakmeter_bank_t *bank, uint32_t channel, uint32_t sample_rate);
int mi_peakmeter_bank_set_hold_time(mi_peakmeter_bank_t *bank, uint32_t channel, float hold);
int mi_peakmeter_bank_set_release_time(mi_peakmeter_bank_t *bank, uint32_t channel, float release);
int mi_peakmeter_bank_set_time(mi_peakmeter_bank_t *bank, uint32_t channel, float hold, float release);
/* clear() of one channel, or of every channel (channel = UINT32_MAX): fPeak = 0, nCounter = 0, before the next launch */
int mi_peakmeter_bank_clear(mi_peakmeter_bank_t *bank, uint32_t channel);
/* What the setters and clear() left goes to the device (and the call waits for it).  Every process entry runs it first.  On a
 * stream being captured pending work is refused (MI_ESTATE): call it before the capture. */
int mi_peakmeter_bank_update_settings(mi_peakmeter_bank_t *bank, void *stream);
/* fTau and nHold as update_settings() computes them (HOST memory); set_params() sets the two as given (factor and count of
 * *params are not looked at).  The state as the work enqueued on `stream` leaves it, after what is pending (HOST memory; waits
 * for the stream; not on a stream being captured: MI_ESTATE).  A counter above the hold is taken down to it by the next launch,
 * as update_settings() does in the reference. */
int mi_peakmeter_bank_get_params(const mi_peakmeter_bank_t *bank, uint32_t channel, mi_peakmeter_params_t *params);
int mi_peakmeter_bank_set_params(mi_peakmeter_bank_t *bank, uint32_t channel, const mi_peakmeter_params_t *params);
int mi_peakmeter_bank_get_state(mi_peakmeter_bank_t *bank, uint32_t channel, mi_peakmeter_state_t *state, void *stream);
int mi_peakmeter_bank_set_state(mi_peakmeter_bank_t *bank, uint32_t channel, const mi_peakmeter_state_t *state, void *stream);
/* process(dst, src, count) and process(src, count): dst NULL updates the state only; dst may be src (same stride).  peaks: NULL,
 * or a DEVICE array of `channels` floats that receives every channel's return value, the peak after the last sample. */
int mi_peakmeter_bank_process(mi_peakmeter_bank_t *bank, float *dst, const float *src, float *peaks, size_t count,
                              size_t dst_stride, size_t src_stride, void *stream);
/* process(value, count), one block-rate step of every channel: values is a DEVICE array of `channels` floats, peaks as above.
 * The decay factor expf(logf(fTau) * float(count)) is formed on the host, with the libm the reference uses, and kept in the
 * parameter table: a call whose count differs from the last one's uploads it, and is refused inside a stream capture like a
 * setter (MI_ESTATE).  count is at most UINT32_MAX. */
int mi_peakmeter_bank_process_value(mi_peakmeter_bank_t *bank, float *peaks, const float *values, size_t count, void *stream);

/*
 * mi_surge_bank: `channels` x lsp::dspu::SurgeProtector (dynamics/SurgeProtector.h, src/main/dynamics/SurgeProtector.cpp): a gain
 * that fades in (square root of a linear ramp over transition_max samples) once the level row reaches on_threshold, and out
 * once it stayed below off_threshold for shutdown_max samples.  The compares are >=, so a NaN level never passes.  fGain, both
 * counters and the flag live on the device; the gain is the reference's bit for bit.  The reference's counters are size_t, the
 * bank's are 32 bits wide.  Rows: [channels][stride].
 */
typedef struct mi_surge_bank mi_surge_bank_t;
typedef struct { uint32_t transition_max, shutdown_max; float on_threshold, off_threshold; } mi_surge_params_t;
typedef struct { float gain; uint32_t transition_time, shutdown_time, on; } mi_surge_state_t;   /* fGain, nTransitionTime, nShutdownTime, bOn */
int mi_surge_bank_create(mi_surge_bank_t **bank, uint32_t channels);                       /* construct(): everything 0 */
int mi_surge_bank_destroy(mi_surge_bank_t *bank);
/* The setters (times in samples).  set_transition_time and set_shutdown_time clamp the live counter at once in the reference,
 * and reset() clears bOn and nTransitionTime: the bank records these in call order and applies them to the device state before
 * the next launch or state access, so set_transition_time(5) followed by (100) leaves a counter of at most 5.  reset() takes a
 * channel, or UINT32_MAX for all. */
int mi_surge_bank_set_transition_time(mi_surge_bank_t *bank, uint32_t channel, uint32_t samples);
int mi_surge_bank_set_shutdown_time(mi_surge_bank_t *bank, uint32_t channel, uint32_t samples);
int mi_surge_bank_set_on_threshold(mi_surge_bank_t *bank, uint32_t channel, float threshold);
int mi_surge_bank_set_off_threshold(mi_surge_bank_t *bank, uint32_t channel, float threshold);
int mi_surge_bank_set_threshold(mi_surge_bank_t *bank, uint32_t channel, float on, float off);
int mi_surge_bank_reset(mi_surge_bank_t *bank, uint32_t channel);
/* The settings as set (HOST memory).  The state after what is recorded and enqueued (HOST memory; waits for the stream; not on
 * a stream being captured: MI_ESTATE).  set_state refuses a transition counter above transition_max, a shutdown counter above
 * shutdown_max and a flag above 1 (MI_EINVAL).  There is no update_settings(): a process call (one of count 0 will do) sends
 * what the setters left, and inside a stream capture refuses to (MI_ESTATE); get_state() before the capture sends it too. */
int mi_surge_bank_get_params(const mi_surge_bank_t *bank, uint32_t channel, mi_surge_params_t *params);
int mi_surge_bank_get_state(mi_surge_bank_t *bank, uint32_t channel, mi_surge_state_t *state, void *stream);
int mi_surge_bank_set_state(mi_surge_bank_t *bank, uint32_t channel, const mi_surge_state_t *state, void *stream);
/* process(out, in, count): the gain into out; out NULL (process(in, count)) moves the state only; out may be in (same stride).
 * process_mul: out[i] *= gain, out read and written; out may be in. */
int mi_surge_bank_process(mi_surge_bank_t *bank, float *out, const float *in, size_t count, size_t out_stride, size_t in_stride,
                          void *stream);
int mi_surge_bank_process_mul(mi_surge_bank_t *bank, float *out, const float *in, size_t count, size_t out_stride,
                              size_t in_stride, void *stream);

/* ---- depopper bank: RMS-gated fades with look-ahead --------------------------------------------------------------------------- */
/*
 * mi_depopper_bank: `channels` x lsp::dspu::Depopper (util/Depopper.h, src/main/util/Depopper.cpp), every channel with settings of
 * its own.  Per sample: the sliding RMS of the input over nRmsLen samples (env); a four-state automaton on it (closed, fade,
 * opened, wait) with a fade-in threshold and a fade-out threshold; and a look-ahead gain buffer into which a fade-out is patched
 * backwards, so the gain leaves nLookCount = (fade-out samples) + nRmsLen samples late.  fRms, nState, nCounter, nDelay, nRmsOff,
 * nLookOff and both buffers live on the device: process() reads nothing back and can be captured into a graph.  env, gain and the
 * state are the reference's bit for bit in float32 (NaN and Inf samples behave as there, subnormals are kept); the two fade
 * curves are tabulated on the host with the C library's sinf and expf, the device evaluates no transcendental.  The output does
 * not depend on how a stream is cut into calls.  Rows: [channels][stride].
 *
 * Refused with MI_EINVAL and a message by update_settings(), process(), get_state() and set_state() -- where the reference reads
 * or writes outside its buffers, divides by zero or converts an undefined float to an integer:
 *   - a channel that was never init()ed;
 *   - nRmsLen == 0 (an RMS length of less than one sample: the default);
 *   - a fade-out time above max_fade or below 0;
 *   - a time or delay that is not a number or at least 2^30 samples; init() maxima that are negative, not a number or at least
 *     2^24 samples (init() itself refuses these);
 * and, the bank's own bound, a fade-in of more than 2^20 samples (one table entry per sample).  An RMS length outside
 * [0, max_rms] is clamped, as the reference clamps it.  A refused bank stays refused until a setter has mended the channel.
 */
typedef struct mi_depopper_bank mi_depopper_bank_t;
enum { MI_DEPOPPER_LINEAR = 0, MI_DEPOPPER_CUBIC = 1, MI_DEPOPPER_SINE = 2, MI_DEPOPPER_GAUSSIAN = 3, MI_DEPOPPER_PARABOLIC = 4 };  /* depopper_mode_t */
enum { MI_DEPOPPER_CLOSED = 0, MI_DEPOPPER_FADE = 1, MI_DEPOPPER_OPENED = 2, MI_DEPOPPER_WAIT = 3 };          /* Depopper::state_t */
/* Depopper::fade_t: enMode, fThresh, fTime, fDelay, nSamples, nDelay, fPoly */
typedef struct { uint32_t mode; float threshold, time, delay; int64_t samples, delay_samples; float poly[4]; } mi_depopper_fade_t;
/* sFadeIn, sFadeOut, nSampleRate, fLookMax, fRmsMax, fRmsLength, fRmsNorm, nLookMin, nLookMax, nLookCount, nRmsMin, nRmsMax,
 * nRmsLen as the last update_settings() left them, and bReconfigure */
typedef struct
{
    mi_depopper_fade_t fade_in, fade_out;
    uint64_t sample_rate;
    float look_max, rms_max, rms_length, rms_norm;
    int64_t look_min_off, look_max_off, look_count, rms_min_off, rms_max_off, rms_len;
    uint32_t reconfigure;
} mi_depopper_params_t;
typedef struct { float rms; uint32_t state; int64_t counter, delay, rms_off, look_off; } mi_depopper_state_t;  /* fRms, nState, nCounter, nDelay, nRmsOff, nLookOff */
/* init() and reconfigure() of one depopper without a bank or a device: the settings are read from *settings as they stand, not
 * through the setters (sample_rate, look_max, rms_max, rms_length -- clamped to [0, rms_max] -- and of both fades mode, threshold,
 * time, delay), *designed receives them with the designed values, the tables (HOST memory, each may be NULL) at most their
 * capacity of entries.  MI_EINVAL where the bank would refuse the settings; designed->reconfigure then says what was written: 0,
 * the designed values as the reference computes them (nRmsLen == 0, a fade-out time outside [0, max_fade], a fade-in too long for
 * the bank); 1, nothing, because the reference's own conversions are undefined (times that are no numbers, bad maxima or modes). */
int mi_depopper_compute_params(const mi_depopper_params_t *settings, mi_depopper_params_t *designed, float *table_in, size_t in_capacity,
                               float *table_out, size_t out_capacity);
/* init() alone: *extents receives sample_rate, look_max, rms_max and the four offsets nLookMin, nLookMax, nRmsMin, nRmsMax of
 * these maxima (times in milliseconds); everything else in it is the constructor's.  MI_EINVAL for maxima that init() refuses. */
int mi_depopper_compute_extents(uint64_t sample_rate, float max_fade, float max_rms, mi_depopper_params_t *extents);
/* A threshold on the envelope taken to the domain of squares, as the device compares it: *square receives the smallest q >= 0
 * with sqrtf(q) >= threshold, so that  sqrtf(q) < threshold  is  q < *square  for every q >= 0 and for NaN (-Inf for a threshold
 * that is not above 0, NaN for NaN: neither compare ever holds). */
int mi_depopper_square_threshold(float threshold, float *square);
int mi_depopper_bank_create(mi_depopper_bank_t **bank, uint32_t channels);                 /* construct(): no buffers yet */
int mi_depopper_bank_destroy(mi_depopper_bank_t *bank);
/* init(srate, max_fade, max_rms) of one channel (times in milliseconds): nothing happens where the three are what they were;
 * otherwise the next update_settings() makes the channel's buffers, zeroes them and sets nState, nRmsOff and nLookOff. */
int mi_depopper_bank_init(mi_depopper_bank_t *bank, uint32_t channel, uint64_t sample_rate, float max_fade, float max_rms);
/* The setters (times in milliseconds), line for line the reference's: each compares the new value with the (clamped) old one,
 * stores it unclamped and asks for a reconfiguration where they differ; *old (may be NULL) receives what the reference returns.
 * A changed setting acts with the next process() that is issued.  The reference declares a tenth setter, set_release(), and
 * defines it nowhere: there is nothing to restate. */
int mi_depopper_bank_set_fade_in_mode(mi_depopper_bank_t *bank, uint32_t channel, uint32_t mode, uint32_t *old);
int mi_depopper_bank_set_fade_out_mode(mi_depopper_bank_t *bank, uint32_t channel, uint32_t mode, uint32_t *old);
int mi_depopper_bank_set_fade_in_time(mi_depopper_bank_t *bank, uint32_t channel, float value, float *old);
int mi_depopper_bank_set_fade_out_time(mi_depopper_bank_t *bank, uint32_t channel, float value, float *old);
int mi_depopper_bank_set_fade_in_threshold(mi_depopper_bank_t *bank, uint32_t channel, float value, float *old);
int mi_depopper_bank_set_fade_out_threshold(mi_depopper_bank_t *bank, uint32_t channel, float value, float *old);
int mi_depopper_bank_set_fade_in_delay(mi_depopper_bank_t *bank, uint32_t channel, float value, float *old);
int mi_depopper_bank_set_fade_out_delay(mi_depopper_bank_t *bank, uint32_t channel, float value, float *old);
int mi_depopper_bank_set_rms_length(mi_depopper_bank_t *bank, uint32_t channel, float value, float *old);
/* init() and every setter's field of one channel as they stand in *settings (read as compute_params reads them; the RMS length
 * is clamped): what a caller that keeps the reference's fields itself hands over.  A reconfiguration is asked for where a field
 * differs from the channel's, or where settings->reconfigure is not 0. */
int mi_depopper_bank_set_settings(mi_depopper_bank_t *bank, uint32_t channel, const mi_depopper_params_t *settings);
/* reconfigure() of every channel that asks for it: the designer, the tables and the settings to the device, fRms re-summed over
 * the new nRmsLen (and the call waits for the copies).  Every process entry runs it first.  On a stream being captured pending
 * work is refused (MI_ESTATE): call it before the capture.  Where one channel's settings are refused no channel is touched:
 * get_params(), get_fade_table() and latency() go on reporting what the device runs, with reconfigure still 1. */
int mi_depopper_bank_update_settings(mi_depopper_bank_t *bank, void *stream);
/* The designed values (HOST memory).  The fade tables, crossfade(fade, x) for x = 0 .. nSamples - 1 (fade_out 0: sFadeIn, 1:
 * sFadeOut): *count receives the length, table (HOST memory, may be NULL) at most `capacity` entries.  latency(): sFadeOut.nSamples. */
int mi_depopper_bank_get_params(const mi_depopper_bank_t *bank, uint32_t channel, mi_depopper_params_t *params);
int mi_depopper_bank_get_fade_table(const mi_depopper_bank_t *bank, uint32_t channel, uint32_t fade_out, float *table, size_t capacity,
                                    size_t *count);
int mi_depopper_bank_latency(const mi_depopper_bank_t *bank, uint32_t channel, int64_t *samples);
/* The state after what is pending and enqueued (HOST memory; waits for the stream; not on a stream being captured: MI_ESTATE).
 * rms_buf / gain_buf (HOST memory, each may be NULL): the logical contents of the buffers, the last nRmsMin squares and the last
 * nLookMin gains, oldest first.  set_state refuses a state above 3, a counter below 0, counters of 2^30 and more and offsets
 * outside [nRmsMin, nRmsMax] / [nLookMin, nLookMax] (MI_EINVAL). */
int mi_depopper_bank_get_state(mi_depopper_bank_t *bank, uint32_t channel, mi_depopper_state_t *state, float *rms_buf, float *gain_buf,
                               void *stream);
int mi_depopper_bank_set_state(mi_depopper_bank_t *bank, uint32_t channel, const mi_depopper_state_t *state, const float *rms_buf,
                               const float *gain_buf, void *stream);
/* process(env, gain, src, count): env may be NULL; env or gain may be src (same stride); env and gain are different buffers. */
int mi_depopper_bank_process(mi_depopper_bank_t *bank, float *env, float *gain, const float *src, size_t count, size_t env_stride,
                             size_t gain_stride, size_t src_stride, void *stream);

/* ---- bypass and crossfade banks: click-free switching ------------------------------------------------------------------------ */
/*
 * mi_bypass_bank: `channels` x lsp::dspu::Bypass (ctl/Bypass.h, src/main/ctl/Bypass.cpp).  The gain runs from 0 (dry) to 1 (wet)
 * as the running float32 sum fGain += fDelta, one step per sample, and every ramp sample is mixed with the gain before the
 * step; once the ramp is over the rest of the block is a copy or a scale of the one input that is left.  nState, fDelta and
 * fGain live on the device and are the reference's bit for bit, as is the output.  The channels of a call may be in different
 * states.  Rows: [channels][stride].
 */
typedef struct mi_bypass_bank mi_bypass_bank_t;
enum { MI_BYPASS_ON = 0, MI_BYPASS_ACTIVE = 1, MI_BYPASS_OFF = 2 };                        /* Bypass::state_t */
typedef struct { uint32_t state; float delta; float gain; } mi_bypass_state_t;             /* nState, fDelta, fGain */
int mi_bypass_bank_create(mi_bypass_bank_t **bank, uint32_t channels);                     /* construct(): S_OFF, 0, 0 */
int mi_bypass_bank_destroy(mi_bypass_bank_t *bank);
/* init(sample_rate, time) of a channel, or of all (channel = UINT32_MAX): S_OFF, fDelta = 1 / max(float(sample_rate) * time, 1),
 * fGain = 1, in host float32.  A NaN time, or a product of 2^32 and more, is MI_EINVAL and changes nothing. */
int mi_bypass_bank_init(mi_bypass_bank_t *bank, uint32_t channel, int sample_rate, float time);
/* set_bypass(bypass) of a channel, or of all.  *changed: the reference's return value; for all channels the number of
 * channels that changed, and changed may then be NULL.  init and set_bypass are recorded in call order and reach the device
 * state in front of the next launch or state access.  For a channel whose fDelta is finite and not 0 the answer is known on
 * the host; for any other (never initialised, or set so by set_state) the state is read back on the stream of the bank's
 * last process or state call: that waits for the stream, and is MI_ESTATE while the stream is being captured. */
int mi_bypass_bank_set_bypass(mi_bypass_bank_t *bank, uint32_t channel, int bypass, int *changed);
int mi_bypass_bank_bypassing(mi_bypass_bank_t *bank, uint32_t channel, int *bypassing, void *stream);
/* The state after what is recorded and enqueued (HOST memory; waits for the stream; not on a stream being captured:
 * MI_ESTATE).  set_state takes any bits: the kernel's comparisons are the reference's, NaN and 0 included. */
int mi_bypass_bank_get_state(mi_bypass_bank_t *bank, uint32_t channel, mi_bypass_state_t *state, void *stream);
int mi_bypass_bank_set_state(mi_bypass_bank_t *bank, uint32_t channel, const mi_bypass_state_t *state, void *stream);
/* process, process_wet, process_drywet: dry may be NULL; dst may be dry or wet (same stride); the gains are scalars of the
 * call.  A call with nothing recorded can be captured into a graph and replayed: a replay goes on with the ramp.  What is
 * recorded is refused inside a capture (MI_ESTATE); count 0 changes nothing. */
int mi_bypass_bank_process(mi_bypass_bank_t *bank, float *dst, const float *dry, const float *wet, size_t count, size_t dst_stride,
                           size_t dry_stride, size_t wet_stride, void *stream);
int mi_bypass_bank_process_wet(mi_bypass_bank_t *bank, float *dst, const float *dry, const float *wet, float wet_gain, size_t count,
                               size_t dst_stride, size_t dry_stride, size_t wet_stride, void *stream);
int mi_bypass_bank_process_drywet(mi_bypass_bank_t *bank, float *dst, const float *dry, const float *wet, float dry_gain,
                                  float wet_gain, size_t count, size_t dst_stride, size_t dry_stride, size_t wet_stride,
                                  void *stream);

/*
 * mi_crossfade_bank: `channels` x lsp::dspu::Crossfade (ctl/Crossfade.h, src/main/ctl/Crossfade.cpp): after toggle() the output
 * goes from fade_out to fade_in over nSamples samples, with the same running sum.  nCounter, fDelta and fGain live on the
 * device; nSamples and an exact copy of nCounter (every process call takes min(nCounter, count) off it) are kept on the host,
 * so toggle() and remaining() never wait.  The reference's counters are size_t, the bank's are 32 bits wide.
 */
typedef struct mi_crossfade_bank mi_crossfade_bank_t;
typedef struct { uint32_t counter; float delta; float gain; } mi_crossfade_state_t;        /* nCounter, fDelta, fGain */
int mi_crossfade_bank_create(mi_crossfade_bank_t **bank, uint32_t channels);               /* construct(): 0, 0, 0, 1 */
int mi_crossfade_bank_destroy(mi_crossfade_bank_t *bank);
/* init(sample_rate, time): nSamples = max(ssize_t(float(sample_rate) * time), 1); MI_EINVAL as for the bypass bank */
int mi_crossfade_bank_init(mi_crossfade_bank_t *bank, uint32_t channel, int sample_rate, float time);
/* toggle() and reset() of a channel, or of all (UINT32_MAX): recorded, and on the device in front of the next launch or state
 * access.  *toggled: whether the channel was idle and now fades; for all channels how many do (toggled may then be NULL). */
int mi_crossfade_bank_toggle(mi_crossfade_bank_t *bank, uint32_t channel, int *toggled);
int mi_crossfade_bank_reset(mi_crossfade_bank_t *bank, uint32_t channel);
int mi_crossfade_bank_remaining(const mi_crossfade_bank_t *bank, uint32_t channel, size_t *remaining);
int mi_crossfade_bank_get_state(mi_crossfade_bank_t *bank, uint32_t channel, mi_crossfade_state_t *state, void *stream);
int mi_crossfade_bank_set_state(mi_crossfade_bank_t *bank, uint32_t channel, const mi_crossfade_state_t *state, void *stream);
/* process(dst, fade_out, fade_in, count): either input may be NULL, or both (silence; the fade moves on all the same); dst
 * may be either input (same stride).  The counters are positions held on the host: capture a call through
 * mi_dspu_graph_begin_capture / end_capture, which refuse a capture during which a fade ran (a replay would not move them). */
int mi_crossfade_bank_process(mi_crossfade_bank_t *bank, float *dst, const float *fade_out, const float *fade_in, size_t count,
                              size_t dst_stride, size_t out_stride, size_t in_stride, void *stream);

/*
 * mi_splitter_bank: lsp::dspu::SpectralSplitter for `channels` channels sharing the settings
 * (util/SpectralSplitter.h:62-250, src/main/util/SpectralSplitter.cpp:62-361) -- the engine of lsp::dspu::FFTCrossover.
 * The last 2^rank samples of every channel are transformed once per 2^(chunk_rank-1) samples; each handler shapes that
 * spectrum, returns to the time domain and overlap-adds the last 2^chunk_rank samples (sin^2 window) into its output.
 * A handler is bound as COPY (no spectral function), MASK (2^rank real gains in FFT order: FFTCrossover::spectral_func,
 * FFTCrossover.cpp:124-140) or CALLBACK; its sink is the device buffer passed to process().
 */
typedef struct mi_splitter_bank mi_splitter_bank_t;
/* spectral_splitter_func_t on the device (util/SpectralSplitter.h:41-46): in/out are DEVICE pointers to
 * [channels][2 * 2^rank] floats (packed complex); the function runs on the host and may enqueue work on `stream`. */
typedef void (*mi_splitter_func_t)(void *object, void *subject, float *out, const float *in, size_t rank, size_t channels, void *stream);
/* init(max_rank, handlers), SpectralSplitter.cpp:62-127 (max_rank 5..18; frames above 2^14 samples go through global memory,
 * one plain launch per step of the hop instead of the fused kernel) */
int mi_splitter_bank_create(mi_splitter_bank_t **bank, uint32_t channels, uint32_t max_rank, uint32_t handlers);
int mi_splitter_bank_destroy(mi_splitter_bank_t *bank);
/* set_rank / set_chunk_rank / set_phase, SpectralSplitter.cpp:260-282 */
int mi_splitter_bank_set_rank(mi_splitter_bank_t *bank, uint32_t rank);
int mi_splitter_bank_set_chunk_rank(mi_splitter_bank_t *bank, int32_t rank);
int mi_splitter_bank_set_phase(mi_splitter_bank_t *bank, float phase);
/* rank(), chunk_rank(), latency() (:284-293) and the samples left until the next transform */
int mi_splitter_bank_get(const mi_splitter_bank_t *bank, uint32_t *rank, uint32_t *chunk_rank, uint32_t *latency, uint32_t *remaining);
/* bind(id, object, subject, func, sink) in its three forms, unbind(id) (:143-180).  mask: HOST memory, one row of 2^rank
 * gains for all channels (mask_stride == 0) or [channels][mask_stride]; binding a mask to a handler that already has
 * one only replaces the gains. */
int mi_splitter_bank_bind_copy(mi_splitter_bank_t *bank, uint32_t handler, void *stream);
int mi_splitter_bank_bind_mask(mi_splitter_bank_t *bank, uint32_t handler, const float *mask, size_t mask_stride, void *stream);
int mi_splitter_bank_bind_callback(mi_splitter_bank_t *bank, uint32_t handler, mi_splitter_func_t func, void *object, void *subject, void *stream);
int mi_splitter_bank_unbind(mi_splitter_bank_t *bank, uint32_t handler);
int mi_splitter_bank_clear(mi_splitter_bank_t *bank, void *stream);                /* SpectralSplitter.cpp:246-258 */
/* process(src, count), :295-361.  in: [channels][in_stride] or NULL (silence); outs: HOST array of `handlers` device
 * pointers, each [channels][out_stride] or NULL (no sink).  An output buffer must not overlap the input rows (MI_EINVAL): the
 * reference hands bands to sink functions, never back into the block being read. */
int mi_splitter_bank_process(mi_splitter_bank_t *bank, float *const *outs, const float *in, size_t count, size_t out_stride,
                             size_t in_stride, void *stream);
/*
 * `blocks` consecutive mi_splitter_bank_process calls in one C call (SpectralSplitter.cpp:295-361 per block): block k reads
 * in[k] and hands band i to outs[k * handlers + i] (HOST tables of DEVICE pointers; a band is NULL in every block of a run
 * or in none).  Runs of blocks of whole frames go out as one launch where the several-hops kernel applies; the samples and
 * the state are those of the calls one by one.
 */
int mi_splitter_bank_process_blocks(mi_splitter_bank_t *bank, float *const *outs, const float *const *in, size_t blocks,
                                    size_t count, size_t out_stride, size_t in_stride, void *stream);

/*
 * crossover::* of misc/fft_crossover.h:47-154 (src/main/misc/fft_crossover.cpp): magnitude of the FFT crossover's high-
 * and low-pass at single frequencies, on frequency lists and on FFT-ordered bins.  Host functions, host memory.
 */
float mi_crossover_hipass(float f, float f0, float slope);
float mi_crossover_lopass(float f, float f0, float slope);
void  mi_crossover_hipass_set(float *gain, const float *f, float f0, float slope, size_t count);
void  mi_crossover_hipass_apply(float *gain, const float *f, float f0, float slope, size_t count);
void  mi_crossover_lopass_set(float *gain, const float *f, float f0, float slope, size_t count);
void  mi_crossover_lopass_apply(float *gain, const float *f, float f0, float slope, size_t count);
void  mi_crossover_hipass_fft_set(float *mag, float f0, float slope, float sample_rate, size_t rank);
void  mi_crossover_hipass_fft_apply(float *mag, float f0, float slope, float sample_rate, size_t rank);
void  mi_crossover_lopass_fft_set(float *mag, float f0, float slope, float sample_rate, size_t rank);
void  mi_crossover_lopass_fft_apply(float *mag, float f0, float slope, float sample_rate, size_t rank);

/* ---- delay line and ring buffer banks ----------------------------------------------------- */
/*
 * mi_delay_bank: `channels` x lsp::dspu::Delay (include/lsp-plug.in/dsp-units/util/Delay.h:35-209).  The delay is
 * per channel.  Calls on the whole bank move every line by the same amount; the *_rows calls move the listed lines
 * only, each line then keeps a write position of its own (every reference object has its nHead, Delay.h:35).
 * Index arithmetic is the reference's (uint32 head/tail/size, src/main/util/Delay.cpp:76-102,434,569-574):
 * outputs are bit-exact.
 */
typedef struct mi_delay_bank mi_delay_bank_t;
enum { MI_GAIN_NONE = 0, MI_GAIN_SCALAR = 1, MI_GAIN_VECTOR = 2 };

/* Delay::init(max_size), Delay.cpp:51-66: line length = align(max_size + 0x200, 0x200). */
int mi_delay_bank_create(mi_delay_bank_t **bank, uint32_t channels, size_t max_size);
int mi_delay_bank_destroy(mi_delay_bank_t *bank);
/* Delay::set_delay(delay) (delay %= size), Delay.cpp:569-574; channel = UINT32_MAX for all. */
int mi_delay_bank_set_delay(mi_delay_bank_t *bank, uint32_t channel, size_t delay);
/* get_delay() and the raw nSize / nHead / nTail of one channel. */
int mi_delay_bank_get(const mi_delay_bank_t *bank, uint32_t channel, uint32_t *delay, uint32_t *size, uint32_t *head, uint32_t *tail);
/* Delay::clear(), Delay.cpp:576-582. */
int mi_delay_bank_clear(mi_delay_bank_t *bank, void *stream);
/* Delay::append(src, count), Delay.cpp:76-102. */
int mi_delay_bank_append(mi_delay_bank_t *bank, const float *in, size_t count, size_t in_stride, void *stream);
/*
 * Delay::process / process_add and their gain variants (Delay.cpp:104-397): out (+)= gain * delayed(in).
 * add != 0 selects process_add; gain_mode MI_GAIN_NONE / MI_GAIN_SCALAR (gain) / MI_GAIN_VECTOR
 * (gain_vec: device [channels][gain_stride]).  out may be the same buffer as in.
 */
int mi_delay_bank_process(mi_delay_bank_t *bank, float *out, const float *in, size_t count, size_t out_stride,
                          size_t in_stride, int add, int gain_mode, float gain, const float *gain_vec,
                          size_t gain_stride, void *stream);
/*
 * Delay::process_ramping(dst, src, [gain,] delay, count), Delay.cpp:399-546: the delay of channel c slides
 * linearly to new_delays[c] (HOST array) over the block; tail index (old_tail + ssize_t(delta * offset)) % size.
 */
int mi_delay_bank_process_ramping(mi_delay_bank_t *bank, float *out, const float *in, const uint32_t *new_delays,
                                  size_t count, size_t out_stride, size_t in_stride, int gain_mode, float gain,
                                  const float *gain_vec, size_t gain_stride, void *stream);
/*
 * The same calls for a SUBSET of the bank's lines -- Delay objects with different call histories in one bank:
 * rows (HOST array of n_rows distinct channel indices) names the line behind every row of the call's buffers
 * (row r of in / out / gain_vec belongs to channel rows[r]); only those lines are written and move on.  One launch
 * however the lines' positions differ (they are read from a per-line table on the device).  The first *_rows call
 * switches the bank's kernels to that table; whole-bank calls keep working and move every line.
 */
int mi_delay_bank_append_rows(mi_delay_bank_t *bank, const uint32_t *rows, uint32_t n_rows, const float *in, size_t count,
                              size_t in_stride, void *stream);
int mi_delay_bank_process_rows(mi_delay_bank_t *bank, const uint32_t *rows, uint32_t n_rows, float *out, const float *in,
                               size_t count, size_t out_stride, size_t in_stride, int add, int gain_mode, float gain,
                               const float *gain_vec, size_t gain_stride, void *stream);
/* Delay::process_ramping for the listed lines only: new_delays[r] is the delay line rows[r] slides to (HOST array of n_rows). */
int mi_delay_bank_process_ramping_rows(mi_delay_bank_t *bank, const uint32_t *rows, uint32_t n_rows, float *out, const float *in,
                                       const uint32_t *new_delays, size_t count, size_t out_stride, size_t in_stride, int gain_mode,
                                       float gain, const float *gain_vec, size_t gain_stride, void *stream);

/* mi_ring_bank: `channels` x lsp::dspu::RingBuffer (util/RingBuffer.h:35-179, src/main/util/RingBuffer.cpp:48-209). */
typedef struct mi_ring_bank mi_ring_bank_t;
/* RingBuffer::init(size, fill), RingBuffer.cpp:48-63. */
int mi_ring_bank_create(mi_ring_bank_t **bank, uint32_t channels, size_t size, float fill);
/* The same with the storage in pinned host memory mapped into the device: *host_view ([channels][size]) is the raw
 * storage as RingBuffer::data() exposes it (util/RingBuffer.h:130); valid after the stream of a call has been synchronised. */
int mi_ring_bank_create_shared(mi_ring_bank_t **bank, uint32_t channels, size_t size, float fill, float **host_view);
int mi_ring_bank_destroy(mi_ring_bank_t *bank);
/* clear() / fill(value), RingBuffer.cpp:108-120 (head returns to 0). */
int mi_ring_bank_fill(mi_ring_bank_t *bank, float value, void *stream);
/* append(data, count) -> *appended = min(count, capacity), RingBuffer.cpp:76-106. */
int mi_ring_bank_append(mi_ring_bank_t *bank, const float *in, size_t count, size_t in_stride, size_t *appended, void *stream);
/* get(dst, offset, count) -> *read, zero-filled where nothing is stored, RingBuffer.cpp:147-183.
 * The single-sample get(offset) (RingBuffer.cpp:122-129) is get(dst, offset, 1). */
int mi_ring_bank_get(mi_ring_bank_t *bank, float *out, size_t offset, size_t count, size_t out_stride, size_t *read, void *stream);
/* size(), head position and tail_position(offset), RingBuffer.cpp:140-145. */
int mi_ring_bank_info(const mi_ring_bank_t *bank, size_t offset, uint32_t *capacity, uint32_t *head, uint32_t *tail_position);

/*
 * mi_dyndelay_bank: `channels` x lsp::dspu::DynamicDelay (util/DynamicDelay.h, src/main/util/DynamicDelay.cpp): a delay line
 * whose delay, feedback gain and feedback delay come per sample from three rows.  Per sample (DynamicDelay.cpp:101-116):
 *     shift = clamp(ssize_t(delay[i]), 0, max_size);  tail = head - shift;  feed = size_t(float(tail) + clamp(fdelay[i], 0, shift))
 *     line[head] = in[i];  s = line[tail];  line[feed] += s * fgain[i];  out[i] = line[tail];  ++head
 * (positions modulo the capacity).  The feed index is the reference's float32 sum; the product and the sum round separately; out
 * is read after the feedback was added.  out, the line and the head have the reference's bits.  nHead lives per channel on
 * the device, so a process call takes no decision on the host and can be captured in a graph.
 * Where the reference's behaviour is undefined the bank defines it: delay converts with saturation (a NaN delay is 0, a delay
 * beyond the range of ssize_t is max_size), and a NaN fdelay counts as 0.  in and fgain may hold anything (Inf, NaN,
 * subnormals, -0) and follow IEEE arithmetic bit for bit.
 */
typedef struct mi_dyndelay_bank mi_dyndelay_bank_t;
typedef struct { uint32_t head; } mi_dyndelay_state_t;                                      /* nHead */
/* init(max_size), DynamicDelay.cpp:65-89: capacity = d - d % 0x400 + 0x800 floats with d = max_size + 1, zeroed; head 0.
 * MI_EINVAL for a capacity above 2^24 floats: the feed index is formed as float32(tail) + ..., and a tail of 2^24 or more
 * would no longer be exact in float32, in the reference as here. */
int mi_dyndelay_bank_create(mi_dyndelay_bank_t **bank, uint32_t channels, size_t max_size);
int mi_dyndelay_bank_destroy(mi_dyndelay_bank_t *bank);
/* max_delay(), capacity() and nHead of one channel; any of the three may be NULL.  The head is read with a synchronised copy
 * on the NULL stream (use get_state for another stream). */
int mi_dyndelay_bank_get(const mi_dyndelay_bank_t *bank, uint32_t channel, uint32_t *max_delay, uint32_t *capacity, uint32_t *head);
/* nHead of a channel, read and written with a synchronised copy: MI_ESTATE on a stream that is being captured.
 * set_state: MI_EINVAL for a head outside the line. */
int mi_dyndelay_bank_get_state(mi_dyndelay_bank_t *bank, uint32_t channel, mi_dyndelay_state_t *state, void *stream);
int mi_dyndelay_bank_set_state(mi_dyndelay_bank_t *bank, uint32_t channel, const mi_dyndelay_state_t *state, void *stream);
/* clear(), DynamicDelay.cpp:91-95: every line and every head to zero, on the stream */
int mi_dyndelay_bank_clear(mi_dyndelay_bank_t *bank, void *stream);
/* process(out, in, delay, fgain, fdelay, samples), DynamicDelay.cpp:97-118: five device arrays [channels][stride], all required.
 * All inputs of a stretch of 0x400 samples are read before any of its outputs is stored: out may be any of the four inputs,
 * with the same stride. */
int mi_dyndelay_bank_process(mi_dyndelay_bank_t *bank, float *out, const float *in, const float *delay, const float *fgain,
                             const float *fdelay, size_t count, size_t out_stride, size_t in_stride, size_t delay_stride,
                             size_t fgain_stride, size_t fdelay_stride, void *stream);
/* copy(s), DynamicDelay.cpp:124-148, on the device: the newest min(capacities) samples of the source line go to the end of the
 * destination line, zeros in front of them, the destination's head to 0.  The banks may be the same; the lines may not. */
int mi_dyndelay_bank_copy(mi_dyndelay_bank_t *dst_bank, uint32_t dst_channel, mi_dyndelay_bank_t *src_bank, uint32_t src_channel,
                          void *stream);
/* `count` floats of a channel's line from position `offset` on, to and from HOST memory (dump(), tests, a caller that seeds a
 * line); synchronised copies, MI_ESTATE on a capturing stream */
int mi_dyndelay_bank_read_line(mi_dyndelay_bank_t *bank, uint32_t channel, float *host, size_t offset, size_t count, void *stream);
int mi_dyndelay_bank_write_line(mi_dyndelay_bank_t *bank, uint32_t channel, const float *host, size_t offset, size_t count, void *stream);
/* Debug counters, written by the kernel only while counting is on: how many steps ran one per lane (parallel) out of how
 * many in all, over every channel since counting was switched on (which zeroes them).  Both calls synchronise the stream and
 * are refused on a capturing one; a graph captured while counting goes on counting.  steps: MI_ESTATE while not counting. */
int mi_dyndelay_bank_count_steps(mi_dyndelay_bank_t *bank, int on, void *stream);
int mi_dyndelay_bank_steps(mi_dyndelay_bank_t *bank, uint64_t *parallel, uint64_t *total, void *stream);

/* ---- oscillator bank (phase-accumulator waveforms) --------------------------------------------------------------------- */
/*
 * mi_oscillator_bank: `channels` x lsp::dspu::Oscillator (util/Oscillator.h, src/main/util/Oscillator.cpp): nine plain and five
 * band-limited (BL) waveforms from a uint32_t phase accumulator, nPhaseAcc = (nPhaseAcc + nFreqCtrlWord) & nPhaseAccMask
 * (:373).  The phase of sample i of a call is (p0 + i w) & mask in closed form, so a row splits along time as well as across
 * channels; the value of a sample depends on its phase alone.  nPhaseAcc lives per channel on the device: process takes no
 * decision on the host and can be captured in a graph.  The settings words and coefficients are computed on the host as the
 * reference computes them (update_settings, :151-357, its mix of double and float kept), loop-invariant divisions included.
 *
 * All non-sinusoid functions, and everything behind the sine (the product by the amplitude, the DC, add and mul), have the
 * reference's bits.  SINUSOIDS: the reference's sin(fAcc2Phase * nPhaseAcc) is the float overload, so its bits are those of its
 * C library's sinf.  The bank forms the argument as the reference does (float(phase) rounded to nearest even, one float
 * product; the squared functions (0.5f * fAcc2Phase) * float(phase)) and takes the float64 sine of that float32 argument,
 * rounded once to float32 (S*).  glibc's sinf is within one ulp of S*.
 *
 * The BL functions synthesise N * count samples with the step nFreqCtrlWord / N into scratch rows and go through
 * mi_oversampler_bank_downsample of an oversampler bank that the oscillator bank owns (:479-628; one downsample per call: the
 * reference's chunks of PROCESS_BUF_LIMIT_SIZE / N change no value, the filter's state runs on).  That bank has one mode and one
 * rate: the channels with a BL function must agree in sample rate and oversampler mode (update_settings: MI_EINVAL otherwise;
 * use two banks).  The oversampler follows the first BL channel, or channel 0 where there is none.
 *
 * What the bank defines where the reference does not:
 *   - trapezoid, :430-443: with fFallRatio == 0, nPoints[1] == nPoints[2], and a phase exactly there satisfies two of the
 *     five ifs (:433 and :439); the reference then writes two values for one sample and runs past its buffer.  The bank
 *     writes exactly one value per sample: the first branch, in source order, that holds.
 *   - nFreqCtrlWord (and every other word) comes from a floating-point to uint32_t conversion that is undefined for a negative,
 *     too large or NaN value.  The bank converts through int64_t and keeps the low 32 bits, NaN and what does not fit int64_t
 *     as 0: what the x86-64 build of the reference does.
 *   - nSampleRate starts at size_t(-1): a channel whose rate was never set refuses process with MI_ESTATE.
 *   - get_periods (:635-689): after a refill (:675-684, every call without skipped periods has one) the read position t has had
 *     the whole buffer size subtracted and is negative, and vSynthBuffer[size_t(t)] reads in front of the buffer, out of
 *     vProcessBuffer.  Bank and class read 0.0f for a position in front of the buffer.  A call with skipped periods that fits
 *     one buffer never refills and has the reference's values.  A period that is not positive and finite is refused (MI_EINVAL;
 *     the class writes nothing): the reference's loops do not end for it.  Positions of the buffer that no fill of the channel's
 *     get_periods calls has written read 0.0f (in the reference vSynthBuffer also holds what process_* staged there).
 */
typedef struct mi_oscillator_bank mi_oscillator_bank_t;
enum
{
    MI_FG_SINE, MI_FG_COSINE, MI_FG_SQUARED_SINE, MI_FG_SQUARED_COSINE, MI_FG_RECTANGULAR, MI_FG_SAWTOOTH, MI_FG_TRAPEZOID,
    MI_FG_PULSETRAIN, MI_FG_PARABOLIC, MI_FG_BL_RECTANGULAR, MI_FG_BL_SAWTOOTH, MI_FG_BL_TRAPEZOID, MI_FG_BL_PULSETRAIN,
    MI_FG_BL_PARABOLIC                                                                      /* fg_function_t, Oscillator.h:33-49 */
};
enum { MI_DC_WAVEDC, MI_DC_ZERO };                                                          /* dc_reference_t, Oscillator.h:51-55 */
enum { MI_OSC_OVERWRITE, MI_OSC_ADD, MI_OSC_MUL };                                          /* process_overwrite / _add / _mul */
/* The members of one oscillator (Oscillator.h:116-151) without its buffers, and what the host knows of nPhaseAcc: with
 * phase_known the accumulator IS `phase`; otherwise it is (the device's + phase) & mask.  Host only. */
typedef struct mi_oscillator_settings
{
    uint32_t    function;                                   /* enFunction */
    float       amplitude, frequency, dc_offset;
    uint32_t    dc_reference;
    float       referenced_dc, init_phase;
    uint64_t    sample_rate;                                /* nSampleRate: UINT64_MAX until set */
    uint32_t    bits, mask;                                 /* nPhaseAccBits, nPhaseAccMask */
    float       acc2phase;
    uint32_t    freq_word, init_word;
    uint32_t    sq_invert;          float sq_amplitude, sq_wave_dc;                                     /* sSquaredSinusoid */
    float       duty;               uint32_t duty_word;     float rect_wave_dc, rect_atten;             /* sRectangular */
    float       width;              uint32_t width_word;    float saw_coeffs[4], saw_wave_dc, saw_atten; /* sSawtooth */
    float       raise_ratio, fall_ratio; uint32_t points[4]; float trap_coeffs[4], trap_wave_dc, trap_atten; /* sTrapezoid */
    float       pos_ratio, neg_ratio; uint32_t train[3];    float pulse_wave_dc, pulse_atten;           /* sPulse */
    uint32_t    par_invert;         float par_amplitude, par_width; uint32_t par_word; float par_wave_dc, par_atten; /* sParabolic */
    uint32_t    oversampling, over_mode, freq_word_over;
    uint32_t    sync;                                       /* bSync */
    uint32_t    phase_known, phase;
    uint32_t    unset_rate_ok;                              /* the C++ class: a rate of size_t(-1) is processed with, as the reference does */
} mi_oscillator_settings_t;
/* The setters of Oscillator.h:207-257 and Oscillator.cpp:749-890, with the reference's clamps and refusals (a refused value
 * changes nothing and is no error) */
enum
{
    MI_OSC_SET_FUNCTION, MI_OSC_SET_FREQUENCY, MI_OSC_SET_SAMPLE_RATE, MI_OSC_SET_PHASE, MI_OSC_SET_PHASE_ACCUMULATOR_BITS,
    MI_OSC_SET_DC_OFFSET, MI_OSC_SET_DC_REFERENCE, MI_OSC_SET_AMPLITUDE, MI_OSC_SET_DUTY_RATIO, MI_OSC_SET_WIDTH,
    MI_OSC_SET_TRAPEZOID_RATIOS, MI_OSC_SET_PULSETRAIN_RATIOS, MI_OSC_SET_PARABOLIC_WIDTH, MI_OSC_SET_SQUARED_SINUSOID_INVERSION,
    MI_OSC_SET_PARABOLIC_INVERSION, MI_OSC_SET_OVERSAMPLER_MODE, MI_OSC_RESET_PHASE_ACCUMULATOR, MI_OSC_SETTERS
};
/* construct(), :42-117; one setter (a, b: its arguments; integers and flags as their value; MI_EINVAL for an unknown setter, a
 * function above MI_FG_BL_PARABOLIC, a DC reference above MI_DC_ZERO or an oversampler mode above MI_OM_LANCZOS_8X24BIT);
 * update_settings(), :151-357 without the oversamplers' part.  No device needed. */
int mi_oscillator_settings_init(mi_oscillator_settings_t *s);
int mi_oscillator_settings_set(mi_oscillator_settings_t *s, uint32_t setter, double a, double b);
int mi_oscillator_settings_update(mi_oscillator_settings_t *s);

int mi_oscillator_bank_create(mi_oscillator_bank_t **bank, uint32_t channels);              /* construct() + init(), :42-135 */
int mi_oscillator_bank_destroy(mi_oscillator_bank_t *bank);                                 /* :137-149 */
/* One setter of one channel (MI_OSC_SET_*, as mi_oscillator_settings_set), and by name */
int mi_oscillator_bank_set(mi_oscillator_bank_t *bank, uint32_t channel, uint32_t setter, double a, double b);
int mi_oscillator_bank_set_function(mi_oscillator_bank_t *bank, uint32_t channel, uint32_t function);           /* .h:240-244 */
int mi_oscillator_bank_set_frequency(mi_oscillator_bank_t *bank, uint32_t channel, float frequency);            /* .h:250-257 */
int mi_oscillator_bank_set_sample_rate(mi_oscillator_bank_t *bank, uint32_t channel, size_t sample_rate);       /* .h:221-229 */
int mi_oscillator_bank_set_phase(mi_oscillator_bank_t *bank, uint32_t channel, float phase);                    /* :749-757 */
int mi_oscillator_bank_set_phase_accumulator_bits(mi_oscillator_bank_t *bank, uint32_t channel, uint32_t bits); /* .h:207-215 */
int mi_oscillator_bank_set_dc_offset(mi_oscillator_bank_t *bank, uint32_t channel, float dc_offset);            /* :765-771 */
int mi_oscillator_bank_set_dc_reference(mi_oscillator_bank_t *bank, uint32_t channel, uint32_t reference);      /* :773-777 */
int mi_oscillator_bank_set_amplitude(mi_oscillator_bank_t *bank, uint32_t channel, float amplitude);            /* :883-890 */
int mi_oscillator_bank_set_duty_ratio(mi_oscillator_bank_t *bank, uint32_t channel, float duty);                /* :797-804 */
int mi_oscillator_bank_set_width(mi_oscillator_bank_t *bank, uint32_t channel, float width);                    /* :806-817 */
int mi_oscillator_bank_set_trapezoid_ratios(mi_oscillator_bank_t *bank, uint32_t channel, float raise, float fall);    /* :819-838 */
int mi_oscillator_bank_set_pulsetrain_ratios(mi_oscillator_bank_t *bank, uint32_t channel, float pos, float neg);      /* :840-858 */
int mi_oscillator_bank_set_parabolic_width(mi_oscillator_bank_t *bank, uint32_t channel, float width);          /* :860-872 */
int mi_oscillator_bank_set_squared_sinusoid_inversion(mi_oscillator_bank_t *bank, uint32_t channel, int invert); /* :779-786 */
int mi_oscillator_bank_set_parabolic_inversion(mi_oscillator_bank_t *bank, uint32_t channel, int invert);       /* :788-795 */
int mi_oscillator_bank_set_oversampler_mode(mi_oscillator_bank_t *bank, uint32_t channel, uint32_t mode);       /* :874-881 */
/* (set_sample_rate and set_oversampler_mode: the channels that have a BL function must agree in both, see above; the
 * disagreement is reported by update_settings and process, MI_EINVAL) */
int mi_oscillator_bank_reset_phase_accumulator(mi_oscillator_bank_t *bank, uint32_t channel);                   /* .h:234 */
/* needs_update(), .h:192-195: bSync of the channel */
int mi_oscillator_bank_needs_update(const mi_oscillator_bank_t *bank, uint32_t channel, int *yes);
/* update_settings(), :151-357, of every channel whose bSync is set.  The phase move of :164-166 depends on the device's phase:
 * the host records the pending change (subtract the old init word, add the new one; or the value itself after a reset) and the
 * next process applies it on the device; there is no read-back.  Changed records are sent to the device: MI_ESTATE on a stream
 * that is being captured if there is anything to send. */
int mi_oscillator_bank_update_settings(mi_oscillator_bank_t *bank, void *stream);
/* The channel's members as update_settings left them */
int mi_oscillator_bank_get_settings(const mi_oscillator_bank_t *bank, uint32_t channel, mi_oscillator_settings_t *settings);
/* ... and set as they stand: members that mi_oscillator_settings_* computed elsewhere (the C++ class does).  With phase_known the
 * phase goes to the device with the next process.  MI_EINVAL for a function, an oversampler mode, a width or an oversampling out
 * of range. */
int mi_oscillator_bank_set_settings(mi_oscillator_bank_t *bank, uint32_t channel, const mi_oscillator_settings_t *settings);
int mi_oscillator_bank_get_exact_frequency(const mi_oscillator_bank_t *bank, uint32_t channel, float *frequency);      /* .h:262-265 */
int mi_oscillator_bank_get_exact_phase(const mi_oscillator_bank_t *bank, uint32_t channel, float *phase);              /* :759-763 */
/* process_overwrite / process_add / process_mul, :691-747, by `op`: dst [channels][dst_stride] device rows of `count` samples.
 * update_settings() runs first, as in the reference.  src [channels][src_stride] is read by add and mul only and may be NULL:
 * 0.0f + s and 0.0f * s then, as fill_zero followed by add2 / mul2 gives.  Every lane reads its src values before it stores:
 * dst may be src, with the same stride.  A BL function needs scratch rows of N * count floats: they grow outside a capture
 * (reserve), MI_ESTATE inside one. */
int mi_oscillator_bank_process(mi_oscillator_bank_t *bank, float *dst, const float *src, size_t count, size_t dst_stride,
                               size_t src_stride, uint32_t op, void *stream);
/* Scratch rows for BL calls of up to `count` samples at the largest oversampling (8), the oversampler's own included */
int mi_oscillator_bank_reserve(mi_oscillator_bank_t *bank, size_t count);
/* mi_oversampler_bank_set_exact of the bank's oversampler */
int mi_oscillator_bank_set_exact(mi_oscillator_bank_t *bank, int on);
/* nPhaseAcc of a channel (pending changes applied), read and written with a synchronised copy: MI_ESTATE on a capturing stream */
typedef struct { uint32_t phase; } mi_oscillator_state_t;
int mi_oscillator_bank_get_state(mi_oscillator_bank_t *bank, uint32_t channel, mi_oscillator_state_t *state, void *stream);
int mi_oscillator_bank_set_state(mi_oscillator_bank_t *bank, uint32_t channel, const mi_oscillator_state_t *state, void *stream);
/* get_periods(dst, periods, periodsSkip, samples), :635-689, of one channel: dst is a DEVICE row of `samples` floats.  The loop runs
 * on the host with the reference's float arithmetic; every fill is a launch from a phase of its own that starts at
 * nInitPhaseWord, into a row of 12 * 1024 floats that the channel keeps between calls (its stale contents are read, as :683
 * has it), for a BL function through an oversampler bank of the channel's own (sOverGetPeriods; made at the first such call, it
 * follows set_exact); the picks are a gather kernel.  Synchronous; MI_ESTATE on a capturing stream.  nPhaseAcc and the
 * streaming oversampler are not touched. */
int mi_oscillator_bank_get_periods(mi_oscillator_bank_t *bank, uint32_t channel, float *dst, size_t periods, size_t periods_skip,
                                   size_t samples, void *stream);
/* The oversampled rows of the last BL call ([channels][stride] device floats, N * count of them per row; NULL before the first):
 * what went into the downsampler.  For tests that feed them to an oversampler bank of their own. */
int mi_oscillator_bank_synth_rows(const mi_oscillator_bank_t *bank, const float **rows, size_t *stride);

/* ---- noise banks (LCG white noise, maximum-length sequences) ------------------------------------------------------------------ */
/*
 * Both banks: process(dst, src, count, dst_stride, src_stride, op, stream) with op = MI_OSC_OVERWRITE / MI_OSC_ADD / MI_OSC_MUL as
 * mi_oscillator_bank_process has it (process_overwrite / process_add / process_mul of every channel).  dst [channels][dst_stride]
 * and src [channels][src_stride] are device rows; every lane reads its src values before it stores, so dst may be src with the
 * same stride.  The state lives on the device and the kernels write it back: nothing is read back, a call can be captured.
 * Defined where the reference is not:
 *   - src == NULL with add or mul (a null dereference there) is MI_EINVAL;
 *   - count == 0 succeeds and changes nothing: no state, and for MLS no pending update_settings is run either.
 *
 * mi_lcg_bank: `channels` x lsp::dspu::LCG (noise/LCG.h, src/main/noise/LCG.cpp) over lsp::dspu::Randomizer
 * (src/main/util/Randomizer.cpp): four generators vLast = vMul1 * vLast + ((vMul2 * vLast) >> 16) + vAdd in uint32_t, drawn round
 * robin from nBufID on.  The map is not affine, so a channel is four serial chains: one lane per (channel, generator) runs them in
 * chunks and leaves the raw draws in LDS in draw order; all lanes of the workgroup turn draws into samples.  A call of `count`
 * samples takes count draws (uniform, triangular) or 2 * count (exponential, Gaussian), and the next call goes on exactly there.
 * Uniform and triangular samples are the reference's bits; expf, logf and cosf are the float64 function of the reference's float32
 * argument rounded once (the reference's bits there are its C library's).
 * Defined where the reference is not:
 *   - a channel that was never init()ed has nBufID == size_t(-1) and the reference indexes vRandom[-1]: process is MI_ESTATE;
 *   - a distribution above MI_LCG_GAUSSIAN is what the reference's switch makes of it (default: uniform); the setter takes it.
 */
typedef struct mi_lcg_bank mi_lcg_bank_t;
enum { MI_LCG_UNIFORM, MI_LCG_EXPONENTIAL, MI_LCG_TRIANGULAR, MI_LCG_GAUSSIAN };            /* lcg_dist_t, LCG.h */
#define MI_LCG_UNSET 0xFFFFFFFFu                                                            /* nBufID of a Randomizer before init() */
/* The members of one Randomizer: randgen_t vRandom[4] by member, and nBufID (0 .. 3, or MI_LCG_UNSET) */
typedef struct { uint32_t last[4], mul1[4], mul2[4], add[4]; uint32_t buf_id; } mi_lcg_state_t;
/* Randomizer::init(seed), Randomizer.cpp:86-99, as words (host only, no device) */
int mi_lcg_seed_words(uint32_t seed, mi_lcg_state_t *state);
int mi_lcg_bank_create(mi_lcg_bank_t **bank, uint32_t channels);                            /* construct() */
int mi_lcg_bank_destroy(mi_lcg_bank_t *bank);
int mi_lcg_bank_init(mi_lcg_bank_t *bank, uint32_t channel, uint32_t seed);                 /* init(seed) */
int mi_lcg_bank_init_time(mi_lcg_bank_t *bank, uint32_t channel);                           /* init(): the seed is the host clock */
int mi_lcg_bank_set_distribution(mi_lcg_bank_t *bank, uint32_t channel, uint32_t distribution);
int mi_lcg_bank_set_amplitude(mi_lcg_bank_t *bank, uint32_t channel, float amplitude);
int mi_lcg_bank_set_offset(mi_lcg_bank_t *bank, uint32_t channel, float offset);
/* Changed settings and states given by init / set_state go to the device first: outside a capture (MI_ESTATE inside one).  They
 * travel with the next process() that is ISSUED: a graph captured before replays with what the device holds and does not see
 * them until a plain process() has sent them. */
int mi_lcg_bank_process(mi_lcg_bank_t *bank, float *dst, const float *src, size_t count, size_t dst_stride, size_t src_stride,
                        uint32_t op, void *stream);
/* One channel's Randomizer, read with a synchronised copy and given to the next launch: MI_ESTATE on a capturing stream.
 * set_state takes buf_id 0 .. 3, or MI_LCG_UNSET for a channel as construct() leaves it. */
int mi_lcg_bank_get_state(mi_lcg_bank_t *bank, uint32_t channel, mi_lcg_state_t *state, void *stream);
int mi_lcg_bank_set_state(mi_lcg_bank_t *bank, uint32_t channel, const mi_lcg_state_t *state, void *stream);
/* As mi_biquad_bank_set_row_enabled: a channel that is switched off is what a caller gets by not calling process() on that object.
 * Its row is not written, its Randomizer does not move, and a state given by init / set_state stays pending until the row next
 * runs; it need not have been init()ed.  Every channel is on after create(); a bank with no channel on launches nothing.  The
 * same for mi_mls_bank (a pending update_settings() waits too: needs_update, get_state and get_settings stay exact) and
 * mi_velvet_bank. */
int mi_lcg_bank_set_row_enabled(mi_lcg_bank_t *bank, uint32_t channel, int enabled);
/* What the next process() would send to the device first -- changed settings, given states; for mi_mls_bank the update_settings()
 * of the channels that are switched on -- goes now: outside a capture.  A process() after it can be captured.  The same for
 * mi_mls_bank, mi_velvet_bank and mi_spectral_tilt_bank. */
int mi_lcg_bank_commit(mi_lcg_bank_t *bank, void *stream);

/*
 * mi_mls_bank: `channels` x lsp::dspu::MLS (noise/MLS.h, src/main/noise/MLS.cpp) with mls_t = uint64_t, the reference's LP64 build.
 * The register shifts right and its output is bit 0, so the update is linear over GF(2): sample i of a call is the parity of
 * rows[i] & state with rows[i] = row 0 of the i-th power of the transition matrix M, and the state n samples on is M^n state.  The
 * kernel runs over (tile of 1024 samples, channel); a tile reaches its state through the powers M^(1024 * 2^j) over the set bits of
 * its index, and a launch of one wave per channel behind the tiles writes M^count state.  rows and the powers M^(2^p) depend on the
 * register width alone: one table for all 64 widths per device, made at the first create(): nothing is built or sent per call.
 * The host follows nState exactly (it knows count), so set_state's "unchanged: nothing happens" rule (MLS.cpp:123-130) and
 * needs_update() are the reference's with no read-back.  A sample is fAmplitude + fOffset or -fAmplitude + fOffset: two float sums.
 */
typedef struct mi_mls_bank mi_mls_bank_t;
/* The members of one MLS (MLS.h), nState as it stands after every call issued so far */
typedef struct mi_mls_settings
{
    uint64_t n_bits, feedback_bit, feedback_mask, active_mask, taps_mask, output_mask, state;
    float    amplitude, offset;
    uint32_t sync, pad;
} mi_mls_settings_t;
/* construct() and update_settings(), MLS.cpp:89-103 and :153-179, on a mi_mls_settings_t (host only, no device) */
int mi_mls_settings_init(mi_mls_settings_t *s);
int mi_mls_settings_update(mi_mls_settings_t *s);
/* The closed form of a register of n_bits (1 .. 64), host only: rows[1024] and powers[27][64] (either may be NULL), and M^count state */
int mi_mls_tables(uint32_t n_bits, uint64_t *rows, uint64_t *powers);
int mi_mls_advance(uint32_t n_bits, uint64_t state, uint64_t count, uint64_t *result);
int mi_mls_bank_create(mi_mls_bank_t **bank, uint32_t channels);                            /* construct() */
int mi_mls_bank_destroy(mi_mls_bank_t *bank);
int mi_mls_bank_set_n_bits(mi_mls_bank_t *bank, uint32_t channel, size_t n_bits);           /* :114-121; clamped to 1 .. 64 at the update */
int mi_mls_bank_set_state(mi_mls_bank_t *bank, uint32_t channel, uint64_t state);           /* :123-130 */
int mi_mls_bank_set_amplitude(mi_mls_bank_t *bank, uint32_t channel, float amplitude);      /* :132-138 */
int mi_mls_bank_set_offset(mi_mls_bank_t *bank, uint32_t channel, float offset);            /* :140-146 */
int mi_mls_bank_needs_update(const mi_mls_bank_t *bank, uint32_t channel, int *yes);        /* :109-112 */
/* update_settings() of every channel that needs it, and changed records go to the device: outside a capture (MI_ESTATE inside
 * one; process runs it first, as progress() does) */
int mi_mls_bank_update_settings(mi_mls_bank_t *bank, void *stream);
int mi_mls_bank_maximum_number_of_bits(const mi_mls_bank_t *bank, size_t *bits);            /* :148-151: 64 */
/* :199-206; 2^64 - 1 for every n_bits from 64 on (the reference shifts by n_bits there before update_settings has clamped it) */
int mi_mls_bank_get_period(const mi_mls_bank_t *bank, uint32_t channel, uint64_t *period);
int mi_mls_bank_process(mi_mls_bank_t *bank, float *dst, const float *src, size_t count, size_t dst_stride, size_t src_stride,
                        uint32_t op, void *stream);
/* What a capture of calls of `count` samples needs is there after this: the tables are (they do not depend on count), so it only
 * checks count; kept so that every generator bank is prepared for a capture alike */
int mi_mls_bank_reserve(mi_mls_bank_t *bank, size_t count);
int mi_mls_bank_get_settings(const mi_mls_bank_t *bank, uint32_t channel, mi_mls_settings_t *settings);
/* nState of a channel as the device holds it (the host's where a set_state or an update has not been launched yet), read with a
 * synchronised copy: MI_ESTATE on a capturing stream.  get_settings gives the host's copy of the same word.  The host counts the
 * calls it issues; replays of a captured graph move the device's word on without it, and this call brings the host's copy up to
 * the device's again (everything issued on other streams has to be complete).  Until then set_state's no-op rule and get_settings
 * speak of the calls that were issued, not of the replays; a set_state or set_n_bits after a capture reaches the device with the
 * next process() that is issued, not with a replay. */
int mi_mls_bank_get_state(mi_mls_bank_t *bank, uint32_t channel, uint64_t *state, void *stream);
int mi_mls_bank_set_row_enabled(mi_mls_bank_t *bank, uint32_t channel, int enabled);        /* see mi_lcg_bank_set_row_enabled */
int mi_mls_bank_commit(mi_mls_bank_t *bank, void *stream);                                  /* see mi_lcg_bank_commit */

/*
 * mi_velvet_bank: `channels` x lsp::dspu::Velvet (noise/Velvet.h, src/main/noise/Velvet.cpp): sparse-impulse noise over a
 * Randomizer and an MLS per channel.  process() is as for the two banks above, with what Velvet itself makes of a call:
 *   - overwrite, and add with src == NULL, are ONE segment of `count` samples (do_process(dst, count));
 *   - add and mul with a source cut the call into segments of 256 samples (BUF_LIM_SIZE), each of which starts its window scan
 *     anew: a call is not the sum of shorter calls;
 *   - mul with src == NULL zero-fills dst and draws nothing: no state word changes, and a state given by init / set_state stays
 *     pending.  (So src == NULL with add or mul is defined here and is not MI_EINVAL.)
 * How many draws a segment takes depends on the draws (the draw that ends a segment is consumed; ARN's spike count is data
 * dependent; the MLS advances by the number of spikes), so the host cannot follow either state: Randomizer and MLS live on the
 * device, the kernel writes them back, nothing is read back and a call can be captured; a replay goes on from the device's state.
 * A wave per channel runs the four generator chains in chunks into a ring of raw draws in LDS and interprets them: 60 windows
 * (OVN, OVNA) or 64 steps (ARN) at a time, a ballot finds the draw that ends the segment, and of two windows that hit one sample
 * the one with the higher scan index wins, as the later write does in the reference.  Every sample and every state word has the
 * reference's bits (fAmplitude and fOffset are applied as mul_k2 and add_k2: two roundings).
 * init(channel, randseed, mls_n_bits, mls_seed) is Velvet::init: Randomizer::init(randseed), then MLS::set_n_bits and
 * MLS::set_state with their "equal to the current value: nothing happens" rule (MLS.cpp:114-130) against the nState that the
 * device holds -- the pending init travels in the channel's record and the kernel applies it --, and update_settings() runs
 * lazily before the first MLS spike (mask, a zero state becomes all ones), so bSync is part of the state that comes back.
 * Settings and pending states travel with the next process() that is ISSUED, as for mi_lcg_bank.
 * Defined where the reference is not:
 *   - a channel that was never init()ed has nBufID == size_t(-1) (vRandom[-1] there): process is MI_ESTATE, for every type and
 *     core (mul with src == NULL, which draws nothing, included: one rule);
 *   - count == 0 succeeds and changes nothing;
 *   - count > 2^24 is MI_EINVAL: beyond it float(idx) is no longer exact and the reference's output degenerates;
 *   - a window width that is not finite is MI_EINVAL at the setter (a NaN compares false in lsp_max; an infinite width makes
 *     0 * inf, whose conversion to size_t is undefined);
 *   - a float-to-index conversion whose value is out of range (or NaN) saturates, which ends the segment;
 *   - a velvet type outside the enum is the reference's default: branch (zero fill, then amplitude and offset), a core outside
 *     the enum is its default: too (the LCG core); the setters take them.
 */
typedef struct mi_velvet_bank mi_velvet_bank_t;
enum { MI_VN_CORE_MLS, MI_VN_CORE_LCG };                                                    /* vn_core_t, Velvet.h */
enum { MI_VN_VELVET_OVN, MI_VN_VELVET_OVNA, MI_VN_VELVET_ARN, MI_VN_VELVET_TRN };           /* vn_velvet_type_t */
#define MI_VN_MAX_COUNT ((size_t)1 << 24)
/* sRandomizer and sMLS of one Velvet.  mls.amplitude and mls.offset are 1 and 0, as construct() and both init() leave them */
typedef struct { mi_lcg_state_t rand; uint32_t pad; mi_mls_settings_t mls; } mi_velvet_state_t;
int mi_velvet_bank_create(mi_velvet_bank_t **bank, uint32_t channels);                      /* construct() */
int mi_velvet_bank_destroy(mi_velvet_bank_t *bank);
/* mls_n_bits is Velvet::init's uint8_t mlsnbits: its low 8 bits count */
int mi_velvet_bank_init(mi_velvet_bank_t *bank, uint32_t channel, uint32_t randseed, uint32_t mls_n_bits, uint64_t mls_seed);
int mi_velvet_bank_init_time(mi_velvet_bank_t *bank, uint32_t channel);     /* init(): the seed is the host clock; the MLS keeps what it has */
int mi_velvet_bank_set_core_type(mi_velvet_bank_t *bank, uint32_t channel, uint32_t core);
int mi_velvet_bank_set_velvet_type(mi_velvet_bank_t *bank, uint32_t channel, uint32_t type);
int mi_velvet_bank_set_velvet_window_width(mi_velvet_bank_t *bank, uint32_t channel, float width);     /* clamped up to 2.0f */
int mi_velvet_bank_set_delta_value(mi_velvet_bank_t *bank, uint32_t channel, float delta);             /* clamped to 0 .. 1 */
int mi_velvet_bank_set_crush_probability(mi_velvet_bank_t *bank, uint32_t channel, float prob);        /* clamped to 0 .. 1 */
int mi_velvet_bank_set_amplitude(mi_velvet_bank_t *bank, uint32_t channel, float amplitude);
int mi_velvet_bank_set_offset(mi_velvet_bank_t *bank, uint32_t channel, float offset);
int mi_velvet_bank_set_crush(mi_velvet_bank_t *bank, uint32_t channel, int crush);
int mi_velvet_bank_process(mi_velvet_bank_t *bank, float *dst, const float *src, size_t count, size_t dst_stride, size_t src_stride,
                           uint32_t op, void *stream);
/* Nothing of the bank depends on count (the MLS tables are the device's): checks count, as mi_mls_bank_reserve does */
int mi_velvet_bank_reserve(mi_velvet_bank_t *bank, size_t count);
/* One channel's Randomizer and MLS as the device holds them (with a pending init or set_state applied), read with a synchronised
 * copy and given to the next launch: MI_ESTATE on a capturing stream.  set_state takes rand.buf_id 0 .. 3 or MI_LCG_UNSET and the
 * MLS members as they stand: n_bits, state and sync are the state, the masks follow feedback_bit (the width of the last
 * update_settings() - 1; all masks 0: never updated). */
int mi_velvet_bank_get_state(mi_velvet_bank_t *bank, uint32_t channel, mi_velvet_state_t *state, void *stream);
int mi_velvet_bank_set_state(mi_velvet_bank_t *bank, uint32_t channel, const mi_velvet_state_t *state, void *stream);
int mi_velvet_bank_set_row_enabled(mi_velvet_bank_t *bank, uint32_t channel, int enabled);  /* see mi_lcg_bank_set_row_enabled */
int mi_velvet_bank_commit(mi_velvet_bank_t *bank, void *stream);                            /* see mi_lcg_bank_commit */
/* An overwrite cut into segments of 256 samples (BUF_LIM_SIZE), each of which starts its window scan anew: what a caller's loop
 * of process_overwrite(tmp, <= 256) over a longer row makes (NoiseGenerator's process_add / process_mul with a source do this,
 * Generator.cpp), in one launch.  Everything else is as for mi_velvet_bank_process with MI_OSC_OVERWRITE. */
int mi_velvet_bank_process_segmented(mi_velvet_bank_t *bank, float *dst, size_t count, size_t dst_stride, void *stream);

/* ---- spectral tilt bank and noise generator bank (coloured noise) ------------------------------------------------------------ */
/*
 * mi_spectral_tilt_bank: `channels` x lsp::dspu::SpectralTilt (filters/SpectralTilt.h, src/main/filters/SpectralTilt.cpp): a
 * magnitude response that goes like f^slope between two frequencies, made of `order` exponentially spaced bilinear pole / zero
 * pairs joined two by two into up to 64 biquads.  The design is the host's: mi_spectral_tilt_settings_t holds the members of one
 * SpectralTilt and the sections of its sFilter, and mi_spectral_tilt_settings_update is update_settings() line for line, with the
 * reference's operand types (what it evaluates in double is evaluated in double), quirks included:
 *   - an odd order is raised to the next even one, then clamped to 128;
 *   - set_frequency_range() swaps its arguments when upper > lower -- the wrong way round --, and update_settings() then falls
 *     back to 0.1 Hz .. 20 kHz; a frequency at or above Nyquist overwrites the member with its default;
 *   - MI_STLT_SLOPE_UNIT_NONE or a slope of zero sets bBypass and leaves the sections of the last design where they are: the
 *     freq_chart of a bypassed tilt reports that stale cascade;
 *   - every new design clears the filter memory (sFilter.end(true));
 *   - order 0 designs no section (the spacing ratio is powf(u / l, 1 / float(2^64 - 1))): process copies.
 * dsp::bilinear_transform_x1 is lsp-dsp-lib's; the formulas of Filter::bilinear_transform (Filter.cpp:2225-2262) in float stand
 * for it, as in mi_dynfilter_*.
 * The cascade runs on a mi_biquad_bank of 64 sections that the bank owns: exact or fast as that bank (the process-wide default at
 * create(), mi_spectral_tilt_bank_set_exact).  process(dst, src, count, dst_stride, src_stride, op, stream) is the reference's three
 * entries, whose second operand is dst itself:
 *   MI_OSC_OVERWRITE  dst = filter(src); src == NULL: zero fill; a bypassed channel: copy
 *   MI_OSC_ADD        dst = dst + filter(src); src == NULL: nothing; a bypassed channel: dst += src
 *   MI_OSC_MUL        dst = dst * filter(src); src == NULL: zero fill; a bypassed channel: dst *= src
 * dst may be src (same stride).  Add and mul filter into scratch rows of the bank (reserve(count) makes them, outside a capture)
 * and a second launch combines.  Bypassed and filtering channels run side by side.  update_settings() of the channels that are
 * switched on opens every process (count == 0 succeeds and does nothing at all); new sections and modes go to the device outside a
 * capture only: call mi_spectral_tilt_bank_update_settings first.
 */
#define MI_STLT_MAX_SECTIONS 64u
enum { MI_STLT_SLOPE_UNIT_NEPER_PER_NEPER, MI_STLT_SLOPE_UNIT_DB_PER_OCTAVE, MI_STLT_SLOPE_UNIT_DB_PER_DECADE, MI_STLT_SLOPE_UNIT_NONE,
       MI_STLT_SLOPE_UNIT_MAX };                                                            /* stlt_slope_unit_t */
enum { MI_STLT_NORM_AT_DC, MI_STLT_NORM_AT_20_HZ, MI_STLT_NORM_AT_1_KHZ, MI_STLT_NORM_AT_20_KHZ, MI_STLT_NORM_AT_NYQUIST, MI_STLT_NORM_AUTO,
       MI_STLT_NORM_NONE, MI_STLT_NORM_MAX };                                               /* stlt_norm_t */
typedef struct mi_spectral_tilt_settings
{
    uint64_t        order;                                  /* nOrder */
    uint64_t        sample_rate;                            /* nSampleRate; 2^64 - 1 (size_t(-1)) after construct() */
    uint32_t        slope_unit, norm;                       /* enSlopeUnit, enNorm */
    float           slope_val, slope_nep_nep;               /* fSlopeVal, fSlopeNepNep */
    float           lower_frequency, upper_frequency;
    uint32_t        bypass, sync;                           /* bBypass, bSync */
    uint32_t        n_sections, pad;                        /* sFilter: the sections of the last design */
    mi_biquad_x1_t  sections[MI_STLT_MAX_SECTIONS];
} mi_spectral_tilt_settings_t;
/* construct(), the setters and update_settings() on a mi_spectral_tilt_settings_t (host only, no device).  *designed (may be
 * NULL) is set when the sections were made anew: whoever runs them clears the filter memory.  freq_chart: both forms by the
 * pointers given (re and im, or c with re and im interleaved, or both); it does not run update first. */
int mi_spectral_tilt_settings_init(mi_spectral_tilt_settings_t *s);
int mi_spectral_tilt_settings_set_order(mi_spectral_tilt_settings_t *s, uint64_t order);
int mi_spectral_tilt_settings_set_slope(mi_spectral_tilt_settings_t *s, float slope, uint32_t unit);
int mi_spectral_tilt_settings_set_norm(mi_spectral_tilt_settings_t *s, uint32_t norm);
int mi_spectral_tilt_settings_set_lower_frequency(mi_spectral_tilt_settings_t *s, float lower);
int mi_spectral_tilt_settings_set_upper_frequency(mi_spectral_tilt_settings_t *s, float upper);
int mi_spectral_tilt_settings_set_frequency_range(mi_spectral_tilt_settings_t *s, float lower, float upper);
int mi_spectral_tilt_settings_set_sample_rate(mi_spectral_tilt_settings_t *s, uint64_t sample_rate);
int mi_spectral_tilt_settings_update(mi_spectral_tilt_settings_t *s, int *designed);
int mi_spectral_tilt_settings_freq_chart(const mi_spectral_tilt_settings_t *s, float *re, float *im, float *c, const float *f, size_t count);
/* digital_biquad_gain() and normalise_digital_biquad() of one section with the members of *s (sample rate, norm, slope) */
int mi_spectral_tilt_settings_section_gain(const mi_spectral_tilt_settings_t *s, const mi_biquad_x1_t *section, float frequency, float *gain);
int mi_spectral_tilt_settings_normalise_section(const mi_spectral_tilt_settings_t *s, mi_biquad_x1_t *section);

typedef struct mi_spectral_tilt_bank mi_spectral_tilt_bank_t;
int mi_spectral_tilt_bank_create(mi_spectral_tilt_bank_t **bank, uint32_t channels);        /* construct() and init(); 1 .. 65535 channels */
int mi_spectral_tilt_bank_destroy(mi_spectral_tilt_bank_t *bank);
int mi_spectral_tilt_bank_set_order(mi_spectral_tilt_bank_t *bank, uint32_t channel, size_t order);
int mi_spectral_tilt_bank_set_slope(mi_spectral_tilt_bank_t *bank, uint32_t channel, float slope, uint32_t unit);
int mi_spectral_tilt_bank_set_norm(mi_spectral_tilt_bank_t *bank, uint32_t channel, uint32_t norm);
int mi_spectral_tilt_bank_set_lower_frequency(mi_spectral_tilt_bank_t *bank, uint32_t channel, float lower);
int mi_spectral_tilt_bank_set_upper_frequency(mi_spectral_tilt_bank_t *bank, uint32_t channel, float upper);
int mi_spectral_tilt_bank_set_frequency_range(mi_spectral_tilt_bank_t *bank, uint32_t channel, float lower, float upper);
int mi_spectral_tilt_bank_set_sample_rate(mi_spectral_tilt_bank_t *bank, uint32_t channel, size_t sample_rate);
/* As mi_biquad_bank_set_row_enabled: a channel that is switched off is an object nobody calls: row, filter memory and a pending
 * update_settings() stay.  A bank with no channel on launches nothing. */
int mi_spectral_tilt_bank_set_row_enabled(mi_spectral_tilt_bank_t *bank, uint32_t channel, int enabled);
int mi_spectral_tilt_bank_set_exact(mi_spectral_tilt_bank_t *bank, int on);                 /* mi_biquad_bank_set_exact of the cascade */
/* update_settings() of EVERY channel; new sections and modes go to the device: outside a capture */
int mi_spectral_tilt_bank_update_settings(mi_spectral_tilt_bank_t *bank, void *stream);
/* ... and of the channels that are switched on only: what the next process() would do first (see mi_lcg_bank_commit) */
int mi_spectral_tilt_bank_commit(mi_spectral_tilt_bank_t *bank, void *stream);
int mi_spectral_tilt_bank_reserve(mi_spectral_tilt_bank_t *bank, size_t count, void *stream);
int mi_spectral_tilt_bank_process(mi_spectral_tilt_bank_t *bank, float *dst, const float *src, size_t count, size_t dst_stride,
                                  size_t src_stride, uint32_t op, void *stream);
/* The sections as the last update_settings() of the channel left them (chains may be NULL: the count alone) */
int mi_spectral_tilt_bank_get_chains(const mi_spectral_tilt_bank_t *bank, uint32_t channel, mi_biquad_x1_t *chains, uint32_t *count);
int mi_spectral_tilt_bank_get_settings(const mi_spectral_tilt_bank_t *bank, uint32_t channel, mi_spectral_tilt_settings_t *settings);
/* freq_chart() in both forms, on the host in float as complex_transfer_calc has it; update_settings() of the channel runs first,
 * as in the reference, and a new design reaches the device with the next process() or update_settings() */
int mi_spectral_tilt_bank_freq_chart(mi_spectral_tilt_bank_t *bank, uint32_t channel, float *re, float *im, const float *f, size_t count);
int mi_spectral_tilt_bank_freq_chart_packed(mi_spectral_tilt_bank_t *bank, uint32_t channel, float *c, const float *f, size_t count);
/* FilterBank::reset() of one channel's sFilter; channel = UINT32_MAX for all (not in the reference's class; for hosts that seek) */
int mi_spectral_tilt_bank_reset(mi_spectral_tilt_bank_t *bank, uint32_t channel, void *stream);
/* One channel's filter memory, [MI_STLT_MAX_SECTIONS][2] floats {d0, d1}: synchronised copies, MI_ESTATE on a capturing stream.
 * The biquad bank's accessors move the whole bank's memory, so each call costs [channels][64][2] floats through the host (and
 * set_state twice that): meant for single channels and tests, not for saving a large bank channel by channel.  The same holds for
 * mi_noise_generator_bank_get_state / set_state, which go through these. */
int mi_spectral_tilt_bank_get_state(mi_spectral_tilt_bank_t *bank, uint32_t channel, float *memory, void *stream);
int mi_spectral_tilt_bank_set_state(mi_spectral_tilt_bank_t *bank, uint32_t channel, const float *memory, void *stream);

/*
 * mi_noise_generator_bank: `channels` x lsp::dspu::NoiseGenerator (noise/Generator.h, src/main/noise/Generator.cpp): an MLS, an
 * LCG and a Velvet source behind one interface, coloured by a SpectralTilt.  The bank owns a mi_mls_bank, a mi_lcg_bank, a
 * mi_velvet_bank and a mi_spectral_tilt_bank, each `channels` wide, and scratch rows.  Per call the channels are sorted by their
 * generator: exactly those rows are switched on in each source bank, and only source banks with a row are launched; the tilt bank
 * runs the coloured rows in place, white rows are switched off there.  The idle sources of a channel keep their state.
 *   overwrite, and add with src == NULL   the sources write dst as one segment of count, the tilt colours dst in place: a white
 *                                         overwrite costs exactly the source bank's launch
 *   add, mul with a source                the reference draws into a temporary in chunks of <= 256, which LCG, MLS and the filter
 *                                         cannot tell from one call and Velvet can (every chunk restarts its window scan): the
 *                                         sources overwrite the scratch rows (Velvet: mi_velvet_bank_process_segmented), the tilt
 *                                         colours them in place, and one launch forms dst = src op scratch.  dst may be src.
 *   mul with src == NULL                  zero fill; nothing drawn, nothing filtered; update_settings() still runs
 * update_settings() is the reference's: the UPD_* bits say what is applied again, amplitude and offset go to all three sources
 * whenever anything is pending, set_generator raises nothing, the velvet core is MI_VN_CORE_LCG, the window width is
 * sample_rate * width (seconds_to_samples), the colour filter runs from 10 Hz to 0.9 * 0.5 * sample_rate with MI_STLT_NORM_AUTO and
 * its own update_settings() runs only when a coloured row is processed (or charted).
 * Defined where the reference is not, or refused:
 *   - process before init() of every channel is MI_ESTATE (the Randomizers index vRandom[-1] there);
 *   - a coloured channel with sample rate 0 is MI_ESTATE at process (the reference designs NaN coefficients);
 *   - count above MI_VN_MAX_COUNT is MI_EINVAL; count == 0 succeeds and changes nothing;
 *   - a generator or colour outside its enum takes the default: branch (LCG; white);
 *   - a velvet window width that is not finite is MI_EINVAL at the setter.
 */
typedef struct mi_noise_generator_bank mi_noise_generator_bank_t;
enum { MI_NG_GEN_MLS, MI_NG_GEN_LCG, MI_NG_GEN_VELVET };                                    /* ng_generator_t */
enum { MI_NG_COLOR_WHITE, MI_NG_COLOR_PINK, MI_NG_COLOR_RED, MI_NG_COLOR_BLUE, MI_NG_COLOR_VIOLET, MI_NG_COLOR_ARBITRARY };    /* ng_color_t */
enum { MI_NG_UPD_MLS = 1, MI_NG_UPD_LCG = 2, MI_NG_UPD_VELVET = 4, MI_NG_UPD_COLOR = 8, MI_NG_UPD_OTHER = 16, MI_NG_UPD_ALL = 31 };
/* The members of one NoiseGenerator beside its four units */
typedef struct mi_noise_generator_settings
{
    uint64_t mls_seed, velvet_mls_seed, color_order, sample_rate, update;   /* sMLSParams.nSeed, sVelvetParams.nMLSseed, sColorParams.nOrder, nSampleRate, nUpdate */
    uint32_t mls_n_bits, lcg_seed, lcg_distribution;
    uint32_t velvet_rand_seed, velvet_mls_n_bits, velvet_core, velvet_type, velvet_crush;
    float    velvet_window_width_s, velvet_arn_delta, velvet_crush_prob;
    uint32_t color, color_slope_unit;
    float    color_slope;
    uint32_t generator, inited;                                             /* enGenerator; init() has run */
    float    amplitude, offset;
} mi_noise_generator_settings_t;
/* The state of one NoiseGenerator's four units */
typedef struct mi_noise_generator_state
{
    mi_lcg_state_t      lcg;
    uint32_t            pad;
    uint64_t            mls_state, mls_n_bits;              /* sMLS: nState and nBits */
    mi_velvet_state_t   velvet;
    float               filter[MI_STLT_MAX_SECTIONS * 2];   /* sColorFilter's memory */
} mi_noise_generator_state_t;
int mi_noise_generator_bank_create(mi_noise_generator_bank_t **bank, uint32_t channels);    /* construct() */
int mi_noise_generator_bank_destroy(mi_noise_generator_bank_t *bank);
/* init(mls_n_bits, mls_seed, lcg_seed, velvet_rand_seed, velvet_mls_n_bits, velvet_mls_seed); the bit counts are uint8_t there */
int mi_noise_generator_bank_init(mi_noise_generator_bank_t *bank, uint32_t channel, uint32_t mls_n_bits, uint64_t mls_seed, uint32_t lcg_seed,
                                 uint32_t velvet_rand_seed, uint32_t velvet_mls_n_bits, uint64_t velvet_mls_seed);
int mi_noise_generator_bank_init_auto(mi_noise_generator_bank_t *bank, uint32_t channel);   /* init(): time seeds, MLS of 64 bits */
int mi_noise_generator_bank_set_sample_rate(mi_noise_generator_bank_t *bank, uint32_t channel, size_t sample_rate);
int mi_noise_generator_bank_set_mls_n_bits(mi_noise_generator_bank_t *bank, uint32_t channel, uint32_t n_bits);
int mi_noise_generator_bank_set_mls_seed(mi_noise_generator_bank_t *bank, uint32_t channel, uint64_t seed);
int mi_noise_generator_bank_set_lcg_distribution(mi_noise_generator_bank_t *bank, uint32_t channel, uint32_t distribution);
int mi_noise_generator_bank_set_velvet_type(mi_noise_generator_bank_t *bank, uint32_t channel, uint32_t type);
int mi_noise_generator_bank_set_velvet_window_width(mi_noise_generator_bank_t *bank, uint32_t channel, float seconds);
int mi_noise_generator_bank_set_velvet_arn_delta(mi_noise_generator_bank_t *bank, uint32_t channel, float delta);
int mi_noise_generator_bank_set_velvet_crush(mi_noise_generator_bank_t *bank, uint32_t channel, int crush);
int mi_noise_generator_bank_set_velvet_crushing_probability(mi_noise_generator_bank_t *bank, uint32_t channel, float prob);
int mi_noise_generator_bank_set_generator(mi_noise_generator_bank_t *bank, uint32_t channel, uint32_t generator);
int mi_noise_generator_bank_set_noise_color(mi_noise_generator_bank_t *bank, uint32_t channel, uint32_t color);
int mi_noise_generator_bank_set_coloring_order(mi_noise_generator_bank_t *bank, uint32_t channel, size_t order);
int mi_noise_generator_bank_set_color_slope(mi_noise_generator_bank_t *bank, uint32_t channel, float slope, uint32_t unit);
int mi_noise_generator_bank_set_amplitude(mi_noise_generator_bank_t *bank, uint32_t channel, float amplitude);
int mi_noise_generator_bank_set_offset(mi_noise_generator_bank_t *bank, uint32_t channel, float offset);
int mi_noise_generator_bank_set_exact(mi_noise_generator_bank_t *bank, int on);             /* the colour filter's arithmetic */
/* NoiseGenerator::update_settings() of every channel (host only: it calls the units' setters), the rows sorted by generator and
 * colour, and then what the units' next launches would send first goes to the device (mi_*_bank_commit): outside a capture.  The
 * units' OWN update_settings() run for the rows that are switched on only -- an idle MLS and the colour filter of a white channel
 * keep theirs pending, as in the reference, where nobody calls them.  After it (and reserve(count) for add and mul with a source)
 * process can be captured. */
int mi_noise_generator_bank_update_settings(mi_noise_generator_bank_t *bank, void *stream);
int mi_noise_generator_bank_reserve(mi_noise_generator_bank_t *bank, size_t count, void *stream);
int mi_noise_generator_bank_process(mi_noise_generator_bank_t *bank, float *dst, const float *src, size_t count, size_t dst_stride,
                                    size_t src_stride, uint32_t op, void *stream);
/* A white channel: re = 1, im = 0; a coloured one: the colour filter's chart (NoiseGenerator::freq_chart does not run the
 * generator's own update_settings(), and neither do these) */
int mi_noise_generator_bank_freq_chart(mi_noise_generator_bank_t *bank, uint32_t channel, float *re, float *im, const float *f, size_t count);
int mi_noise_generator_bank_freq_chart_packed(mi_noise_generator_bank_t *bank, uint32_t channel, float *c, const float *f, size_t count);
int mi_noise_generator_bank_get_settings(const mi_noise_generator_bank_t *bank, uint32_t channel, mi_noise_generator_settings_t *settings);
int mi_noise_generator_bank_get_tilt_settings(const mi_noise_generator_bank_t *bank, uint32_t channel, mi_spectral_tilt_settings_t *settings);
/* The four units' states with synchronised copies: MI_ESTATE on a capturing stream.  set_state gives the Randomizers and the
 * filter memory as they stand and the MLS through set_n_bits / set_state (their "unchanged: nothing happens" rule holds). */
int mi_noise_generator_bank_get_state(mi_noise_generator_bank_t *bank, uint32_t channel, mi_noise_generator_state_t *state, void *stream);
int mi_noise_generator_bank_set_state(mi_noise_generator_bank_t *bank, uint32_t channel, const mi_noise_generator_state_t *state, void *stream);

/* ---- ADSR envelope bank (attack, hold, decay, break, slope, sustain, release curves) ------------------------------------------- */
/*
 * mi_adsr_bank: `channels` x lsp::dspu::ADSREnvelope (util/ADSREnvelope.h, src/main/util/ADSREnvelope.cpp).  The unit has no
 * stream state: a sample is a function of one time value and the channel's designed record (four curves of a function tag and the
 * six floats of gen_params_t, fHoldTime, fBreakLevel, fSustainLevel, nFlags), so one kernel over (chunk of the row, channel)
 * serves the five array entry points, writes nothing but dst, and every call can be captured.  Float arithmetic in the
 * reference's order with no contraction; expf in an EXP segment is the float64 exp of the float32 argument rounded once.
 *
 *   process          dst[i] = do_process(src[i])               :334-340   (t <= 0, t >= 1: +0; a NaN t reaches the release curve)
 *   process_mul      dst[i] *= do_process(src[i])              :342-348
 *   generate         dst[i] = the curve at t_i                 :385-433   t_0 = start, t_i = start + float(i) * step
 *   generate_mul     src == NULL: dst[i] *= the curve at t_i   :435-483   (hold leaves dst[i]; before attack and after release
 *                    src != NULL: dst[i] = src[i] * the curve  :485-533    store 0.0f in every flavour)
 *
 * The reference's generate loops only move forward through the stages 0 before attack, 1 attack, 2 hold, 3 decay, 4 slope,
 * 5 sustain, 6 release, 7 after; in closed form sample i is at stage max(floor, stage(t_i)) with floor = stage(start) for a
 * negative step and 0 otherwise, and a NaN t is at stage 7.  start and step are host arrays of one float per channel; they reach
 * the device as arguments of a small launch on the call's stream ahead of the kernel, so a captured call replays the values of
 * capture time.  A bank's calls belong on one stream at a time.
 * Defined where the reference is not:
 *   - a NaN given to a setter (lsp_limit lets it through) is MI_EINVAL and nothing changes;
 *   - a function outside MI_ADSR_NONE .. MI_ADSR_EXP runs as MI_ADSR_NONE (the reference's default: label);
 *   - count == 0 succeeds and launches nothing; dst and src may be the same rows with the same stride, and must not overlap otherwise.
 */
typedef struct mi_adsr_bank mi_adsr_bank_t;
enum { MI_ADSR_NONE, MI_ADSR_LINE, MI_ADSR_LINE2, MI_ADSR_CUBIC, MI_ADSR_QUADRO, MI_ADSR_EXP };         /* function_t, .h:41-49 */
enum { MI_ADSR_ATTACK, MI_ADSR_DECAY, MI_ADSR_SLOPE, MI_ADSR_RELEASE, MI_ADSR_PARTS };                /* part_t, .h:59-67 */
enum { MI_ADSR_USE_HOLD = 1, MI_ADSR_USE_BREAK = 2, MI_ADSR_RECONFIGURE = 4 };                      /* flags_t, .h:52-57 */
/* curve_t without pGenerator.  params by function: NONE { fT, fK, fB }; LINE, LINE2 { fT2, fK1, fB1, fK2, fB2 }; CUBIC, QUADRO
 * { fT0, fK[5] }; EXP { fT0, fKT, fA[2], fB[2] } */
typedef struct { float time, curve; uint32_t function; float params[6]; } mi_adsr_curve_t;
typedef struct mi_adsr_settings
{
    mi_adsr_curve_t curve[MI_ADSR_PARTS];
    float           hold_time, break_level, sustain_level;
    uint32_t        flags;
} mi_adsr_settings_t;
/* The setters of .h:161-188 by number: a is the value (a time, a curve, a level, a function, or != 0 for enabled); the combined
 * setters take (time, curve, function) or (time or level, enabled) in a, b, c */
enum
{
    MI_ADSR_SET_ATTACK_TIME, MI_ADSR_SET_HOLD_TIME, MI_ADSR_SET_DECAY_TIME, MI_ADSR_SET_SLOPE_TIME, MI_ADSR_SET_RELEASE_TIME,
    MI_ADSR_SET_ATTACK_CURVE, MI_ADSR_SET_DECAY_CURVE, MI_ADSR_SET_SLOPE_CURVE, MI_ADSR_SET_RELEASE_CURVE,
    MI_ADSR_SET_ATTACK_FUNCTION, MI_ADSR_SET_DECAY_FUNCTION, MI_ADSR_SET_SLOPE_FUNCTION, MI_ADSR_SET_RELEASE_FUNCTION,
    MI_ADSR_SET_BREAK_LEVEL, MI_ADSR_SET_SUSTAIN_LEVEL, MI_ADSR_SET_HOLD_ENABLED, MI_ADSR_SET_BREAK_ENABLED,
    MI_ADSR_SET_ATTACK, MI_ADSR_SET_HOLD, MI_ADSR_SET_DECAY, MI_ADSR_SET_BREAK, MI_ADSR_SET_SLOPE, MI_ADSR_SET_RELEASE
};
/* construct(), the setters and update_settings() (:40-293) on a mi_adsr_settings_t, and do_process(t) of a designed one with the
 * device's expf rule: host only, no device */
int mi_adsr_settings_init(mi_adsr_settings_t *s);
int mi_adsr_settings_set(mi_adsr_settings_t *s, uint32_t setter, double a, double b, double c);
int mi_adsr_settings_update(mi_adsr_settings_t *s);
int mi_adsr_settings_process(const mi_adsr_settings_t *s, float t, float *value);
/* interpolation::hermite_cubic and hermite_quadro (src/main/misc/interpolation.cpp:112-177): p[4] and p[5] */
int mi_interpolation_hermite_cubic(float *p, float x0, float y0, float k0, float x1, float y1, float k1);
int mi_interpolation_hermite_quadro(float *p, float x0, float y0, float k0, float x1, float y1, float k1, float x2, float y2);

int mi_adsr_bank_create(mi_adsr_bank_t **bank, uint32_t channels);                          /* construct() of every channel */
int mi_adsr_bank_destroy(mi_adsr_bank_t *bank);
/* One setter of one channel (MI_ADSR_SET_*, as mi_adsr_settings_set), and by name */
int mi_adsr_bank_set(mi_adsr_bank_t *bank, uint32_t channel, uint32_t setter, double a, double b, double c);
int mi_adsr_bank_set_attack_time(mi_adsr_bank_t *bank, uint32_t channel, float value);
int mi_adsr_bank_set_hold_time(mi_adsr_bank_t *bank, uint32_t channel, float value);
int mi_adsr_bank_set_decay_time(mi_adsr_bank_t *bank, uint32_t channel, float value);
int mi_adsr_bank_set_slope_time(mi_adsr_bank_t *bank, uint32_t channel, float value);
int mi_adsr_bank_set_release_time(mi_adsr_bank_t *bank, uint32_t channel, float value);     /* set_relese_time, .h:165 */
int mi_adsr_bank_set_attack_curve(mi_adsr_bank_t *bank, uint32_t channel, float value);
int mi_adsr_bank_set_decay_curve(mi_adsr_bank_t *bank, uint32_t channel, float value);
int mi_adsr_bank_set_slope_curve(mi_adsr_bank_t *bank, uint32_t channel, float value);
int mi_adsr_bank_set_release_curve(mi_adsr_bank_t *bank, uint32_t channel, float value);
int mi_adsr_bank_set_attack_function(mi_adsr_bank_t *bank, uint32_t channel, uint32_t function);
int mi_adsr_bank_set_decay_function(mi_adsr_bank_t *bank, uint32_t channel, uint32_t function);
int mi_adsr_bank_set_slope_function(mi_adsr_bank_t *bank, uint32_t channel, uint32_t function);
int mi_adsr_bank_set_release_function(mi_adsr_bank_t *bank, uint32_t channel, uint32_t function);
int mi_adsr_bank_set_break_level(mi_adsr_bank_t *bank, uint32_t channel, float value);
int mi_adsr_bank_set_sustain_level(mi_adsr_bank_t *bank, uint32_t channel, float value);
int mi_adsr_bank_set_hold_enabled(mi_adsr_bank_t *bank, uint32_t channel, int enabled);
int mi_adsr_bank_set_break_enabled(mi_adsr_bank_t *bank, uint32_t channel, int enabled);
int mi_adsr_bank_set_attack(mi_adsr_bank_t *bank, uint32_t channel, float time, float curve, uint32_t function);
int mi_adsr_bank_set_hold(mi_adsr_bank_t *bank, uint32_t channel, float time, int enabled);
int mi_adsr_bank_set_decay(mi_adsr_bank_t *bank, uint32_t channel, float time, float curve, uint32_t function);
int mi_adsr_bank_set_break(mi_adsr_bank_t *bank, uint32_t channel, float level, int enabled);
int mi_adsr_bank_set_slope(mi_adsr_bank_t *bank, uint32_t channel, float time, float curve, uint32_t function);
int mi_adsr_bank_set_release(mi_adsr_bank_t *bank, uint32_t channel, float time, float curve, uint32_t function);
/* A channel's settings as they stand (the C++ class designs elsewhere and sets them): a NaN member is MI_EINVAL */
int mi_adsr_bank_set_settings(mi_adsr_bank_t *bank, uint32_t channel, const mi_adsr_settings_t *settings);
int mi_adsr_bank_get_settings(const mi_adsr_bank_t *bank, uint32_t channel, mi_adsr_settings_t *settings);
int mi_adsr_bank_needs_update(const mi_adsr_bank_t *bank, uint32_t channel, int *yes);      /* nFlags & F_RECONFIGURE */
/* update_settings() of every channel that needs it, and changed records go to the device: outside a capture (MI_ESTATE inside
 * one).  The five operations run it first, as the reference's do. */
int mi_adsr_bank_update_settings(mi_adsr_bank_t *bank, void *stream);
/* A channel that is switched off is an object nobody calls: its row is neither read nor written.  Every channel is on after
 * create(); a bank with no channel on launches nothing. */
int mi_adsr_bank_set_row_enabled(mi_adsr_bank_t *bank, uint32_t channel, int enabled);
/* dst [channels][dst_stride] and src [channels][src_stride] are device rows; start and step are host arrays [channels].
 * generate_mul: src == NULL is the in-place flavour (src_stride is not looked at). */
int mi_adsr_bank_process(mi_adsr_bank_t *bank, float *dst, const float *src, size_t count, size_t dst_stride, size_t src_stride,
                         void *stream);
int mi_adsr_bank_process_mul(mi_adsr_bank_t *bank, float *dst, const float *src, size_t count, size_t dst_stride, size_t src_stride,
                             void *stream);
int mi_adsr_bank_generate(mi_adsr_bank_t *bank, float *dst, const float *start, const float *step, size_t count, size_t dst_stride,
                          void *stream);
int mi_adsr_bank_generate_mul(mi_adsr_bank_t *bank, float *dst, const float *src, const float *start, const float *step, size_t count,
                              size_t dst_stride, size_t src_stride, void *stream);

/* ---- MeterGraph bank (a full-rate row decimated into display frames) ----------------------------------------------------------- */
/*
 * mi_metergraph_bank: `channels` x lsp::dspu::MeterGraph (util/MeterGraph.h, src/main/util/MeterGraph.cpp).  Every channel cuts its
 * row into frames of `period` samples, reduces each by its method and appends the result to a ring of `frames` words on the
 * device; ring, fCurrent, nCount and nHead are the reference's in every bit (DESIGN.md 3.30 lists the quirks that are kept).
 *   - one process() call is one process(s, n) (gains == NULL) or process(s, gain, n) of every channel;
 *   - create() leaves every channel as construct() does (ABS_MAXIMUM, period 1, no ring); a channel needs init() before the bank
 *     processes: MI_ESTATE otherwise;
 *   - the reference loops forever on a period of 0: init() and set_period() refuse it with MI_EINVAL;
 *   - init(), the setters, fill() and clear() pend until update_settings(), which process(), process_value(), read(), level(),
 *     get_state() and set_state() run first; with something pending that is MI_ESTATE on a stream being captured;
 *   - process(), process_value(), read() and level() are capturable: the kernels keep the state, so a replay appends again.
 */
typedef struct mi_metergraph_bank mi_metergraph_bank_t;
enum { MI_MM_ABS_MAXIMUM, MI_MM_ABS_MINIMUM, MI_MM_SIGN_MAXIMUM, MI_MM_SIGN_MINIMUM, MI_MM_PEAK };      /* meter_method_t, .h:33-63 */
typedef struct { float current; uint32_t count; uint32_t head; } mi_metergraph_state_t;                /* fCurrent, nCount, nHead */
typedef struct { uint32_t method, period, frames; float default_value; } mi_metergraph_params_t;       /* enMethod, nPeriod, nCapacity, fDefault */
int mi_metergraph_bank_create(mi_metergraph_bank_t **bank, uint32_t channels, uint32_t max_frames);
int mi_metergraph_bank_destroy(mi_metergraph_bank_t *bank);
/* init(frames, period, default_value), :55-68: 1 <= frames <= max_frames, 1 <= period < 2^32; the ring is filled with the default */
int mi_metergraph_bank_init(mi_metergraph_bank_t *bank, uint32_t channel, size_t frames, size_t period, float default_value);
/* a method outside the enum runs as MI_MM_ABS_MAXIMUM (the reference's default: label) */
int mi_metergraph_bank_set_method(mi_metergraph_bank_t *bank, uint32_t channel, uint32_t method);
int mi_metergraph_bank_set_period(mi_metergraph_bank_t *bank, uint32_t channel, size_t period);
int mi_metergraph_bank_set_default_value(mi_metergraph_bank_t *bank, uint32_t channel, float value);
/* fill(level) and clear() = fill(fDefault): the ring's words and nHead = 0; fCurrent and nCount stay.  channel UINT32_MAX: all */
int mi_metergraph_bank_fill(mi_metergraph_bank_t *bank, uint32_t channel, float level);
int mi_metergraph_bank_clear(mi_metergraph_bank_t *bank, uint32_t channel);
int mi_metergraph_bank_update_settings(mi_metergraph_bank_t *bank, void *stream);
int mi_metergraph_bank_get_params(const mi_metergraph_bank_t *bank, uint32_t channel, mi_metergraph_params_t *params);
/* ring: NULL, or a HOST array of the channel's `frames` words in storage order.  set_state: head < frames */
int mi_metergraph_bank_get_state(mi_metergraph_bank_t *bank, uint32_t channel, mi_metergraph_state_t *state, float *ring, void *stream);
int mi_metergraph_bank_set_state(mi_metergraph_bank_t *bank, uint32_t channel, const mi_metergraph_state_t *state, const float *ring,
                                 void *stream);
/* src [channels][stride] device rows, read only; gains: NULL, or a DEVICE array of `channels` floats; count < 2^31 */
int mi_metergraph_bank_process(mi_metergraph_bank_t *bank, const float *src, const float *gains, size_t count, size_t stride,
                               void *stream);
/* process(sample) of every channel, :70-111: values is a device array of `channels` floats */
int mi_metergraph_bank_process_value(mi_metergraph_bank_t *bank, const float *values, void *stream);
/* read(dst, count), :246-258, of every channel into dst [channels][stride]: the default ahead of the frames where count exceeds
 * the channel's frames, then the newest frames, oldest first.  level(): the newest frame, levels a device array [channels]. */
int mi_metergraph_bank_read(mi_metergraph_bank_t *bank, float *dst, size_t count, size_t stride, void *stream);
int mi_metergraph_bank_level(mi_metergraph_bank_t *bank, float *levels, void *stream);

/* ---- ScaledMeterGraph bank (display frames of a period that can change: a zoomable time graph) ------------------------------------ */
/*
 * mi_scaled_metergraph_bank: `channels` x lsp::dspu::ScaledMeterGraph (util/ScaledMeterGraph.h, src/main/util/ScaledMeterGraph.cpp).
 * Every channel samples its row twice: into a history ring of sub-samples of `subsampling` samples each, and into a ring of
 * display frames of the period last taken over.  The call after a set_period() that changed the period re-decimates the history
 * into the frame ring instead (update_period(), :269-342).  Both rings, both heads and every state word are the reference's in
 * every bit (DESIGN.md 3.31 lists the quirks that are kept).
 *   - one process() call is one process(s, n) (gains == NULL) or process(s, gain, n) of every channel;
 *   - create() leaves every channel as construct() does (ABS_MAXIMUM, no rings); a channel needs init() and then set_period() before
 *     the bank processes or reads: MI_ESTATE otherwise (with sFrames.nPeriod == 0 the reference's process() never returns);
 *   - where the reference is undefined init() answers MI_EINVAL: subsampling == 0, frames == 0, max_period < subsampling; also
 *     where frames * max_period reaches 2^31 (the reference multiplies in 32 bits) or the rings are larger than create() made them;
 *   - init(), the setters and fill() pend until update_settings(), which process(), process_value(), read(), level(), get_state()
 *     and set_state() run first; with something pending that is MI_ESTATE on a stream being captured;
 *   - process(), process_value(), read() and level() are capturable: the kernels keep the state and decide on the device whether
 *     to re-decimate, so a replay appends again and re-decimates only where the periods differ.
 */
typedef struct mi_scaled_metergraph_bank mi_scaled_metergraph_bank_t;
/* sHistory's fCurrent, nCount and its ring's nHead; sFrames' three and sFrames.nPeriod (the period last taken over, 0: none) */
typedef struct { float history_current; uint32_t history_count, history_head; float frames_current; uint32_t frames_count, frames_head,
                 frames_period; } mi_scaled_metergraph_state_t;
/* enMethod, nPeriod (the target, 0: none set), nMaxPeriod, sHistory.nPeriod, sFrames.nFrames, sHistory.nFrames.  The rings hold
 * subframes + 16 and frames + 16 words (FRAMES_GAP, :30) */
typedef struct { uint32_t method, period, max_period, subsampling, frames, subframes; } mi_scaled_metergraph_params_t;
/* max_subframes: the most ceil(frames * max_period / subsampling) of any init() to come, max_frames .. 2^24 */
int mi_scaled_metergraph_bank_create(mi_scaled_metergraph_bank_t **bank, uint32_t channels, uint32_t max_frames, uint32_t max_subframes);
int mi_scaled_metergraph_bank_destroy(mi_scaled_metergraph_bank_t *bank);
/* init(frames, subsampling, max_period), :67-91: zeroed rings, every state word 0, no period; enMethod stays */
int mi_scaled_metergraph_bank_init(mi_scaled_metergraph_bank_t *bank, uint32_t channel, size_t frames, size_t subsampling, size_t max_period);
/* a method outside the enum runs as MI_MM_ABS_MAXIMUM (the reference's default: label); takes effect in mid-frame too */
int mi_scaled_metergraph_bank_set_method(mi_scaled_metergraph_bank_t *bank, uint32_t channel, uint32_t method);
/* the target only, limited to subsampling .. max_period (:95); MI_ESTATE before init() */
int mi_scaled_metergraph_bank_set_period(mi_scaled_metergraph_bank_t *bank, uint32_t channel, size_t period);
/* fill(level), :376-383: every word of both rings, both nCount = 0; heads and fCurrent stay.  channel UINT32_MAX: all */
int mi_scaled_metergraph_bank_fill(mi_scaled_metergraph_bank_t *bank, uint32_t channel, float level);
int mi_scaled_metergraph_bank_update_settings(mi_scaled_metergraph_bank_t *bank, void *stream);
int mi_scaled_metergraph_bank_get_params(const mi_scaled_metergraph_bank_t *bank, uint32_t channel, mi_scaled_metergraph_params_t *params);
/* history, ring: NULL, or HOST arrays of the channel's subframes + 16 and frames + 16 words in storage order.  set_state: heads
 * inside their rings, history_count < subsampling, frames_period 0 or in subsampling .. max_period, frames_count below it */
int mi_scaled_metergraph_bank_get_state(mi_scaled_metergraph_bank_t *bank, uint32_t channel, mi_scaled_metergraph_state_t *state,
                                        float *history, float *ring, void *stream);
int mi_scaled_metergraph_bank_set_state(mi_scaled_metergraph_bank_t *bank, uint32_t channel, const mi_scaled_metergraph_state_t *state,
                                        const float *history, const float *ring, void *stream);
/* src [channels][stride] device rows, read only; gains: NULL, or a DEVICE array of `channels` floats; count < 2^31 */
int mi_scaled_metergraph_bank_process(mi_scaled_metergraph_bank_t *bank, const float *src, const float *gains, size_t count, size_t stride,
                                      void *stream);
/* process(sample) of every channel, :344-349: values is a device array of `channels` floats */
int mi_scaled_metergraph_bank_process_value(mi_scaled_metergraph_bank_t *bank, const float *values, void *stream);
/* read(dst, count), :365-369, of every channel into dst [channels][stride]: the newest min(count, frames) frames, oldest first;
 * what lies behind them in the row is not written.  level(): the newest frame, levels a device array [channels]. */
int mi_scaled_metergraph_bank_read(mi_scaled_metergraph_bank_t *bank, float *dst, size_t count, size_t stride, void *stream);
int mi_scaled_metergraph_bank_level(mi_scaled_metergraph_bank_t *bank, float *levels, void *stream);

/* ---- QuantizedCounter bank (sliding-window histograms of full-rate rows) -------------------------------------------------------- */
/*
 * mi_qcounter_bank: `channels` x lsp::dspu::QuantizedCounter (stat/QuantizedCounter.h, src/main/stat/QuantizedCounter.cpp).  Every
 * channel keeps the histogram of the last `period` samples of its rows over `levels` quantisation levels of [min, max), with one
 * counter for what lies below the range and one for above.  History ring, counters, nHead and nCount live on the device and are
 * the reference's in every word:
 *   - the bin of a sample is trunc((v - min) * rstep) in float32; where C++ leaves the reference's conversion undefined the bank
 *     DEFINES it as the reference's compiled class has it: a NaN, a product >= 2^31 or <= -1 counts as below, one in
 *     [levels, 2^31) as above;
 *   - one process() call is one process(data, count) of every channel and leaves the window of the last min(period, samples seen)
 *     samples for ANY count.  The reference does so only while count <= nCapacity - nPeriod (always for count <= 1024); beyond
 *     that its single call corrupts its window, a defect that is not reproduced: the bank gives what the reference gives for the
 *     same row fed in pieces of at most nCapacity - nPeriod;
 *   - create() leaves every channel as construct() and init() do: no period, no levels, bUpdate set.  process() before
 *     set_period() and set_levels() or set_range() is MI_ESTATE (the reference divides by zero into a meaningless state);
 *   - the setters are host work; those that change levels, min or max set the channel's bUpdate, a setter that changes nothing
 *     does not.  The recount under the new step (update_settings(), :162-187) is decided on the device by process() or by
 *     update_settings(): it counts the nCount samples held, those beyond a reduced period included;
 *   - read(), get_state(), set_state(), update_settings() and process() send changed settings and pending clear()s to the device
 *     first; with something to send that is MI_ESTATE on a stream being captured.  read() recounts nothing;
 *   - process(), update_settings() and read() are capturable: the kernel keeps nHead, nCount and which settings the counters were
 *     counted under, so a replay counts its row again and recounts for a changed range at the first replay only.
 */
typedef struct mi_qcounter_bank mi_qcounter_bank_t;
/* nPeriod, nLevels, fMinValue, fMaxValue, fRStep (that of the last update) and bUpdate */
typedef struct { uint32_t period, levels; float min_value, max_value, rstep; uint32_t update; } mi_qcounter_params_t;
typedef struct { uint32_t head, count, capacity; } mi_qcounter_state_t;                                  /* nHead, nCount, nCapacity */
/* init(max_period, max_levels), :72-98: 1 <= max_levels <= 2^24, 1 <= max_period with a ring of max_period + 1024 samples (rounded
 * up to 64 bytes) that fits 32 bits */
int mi_qcounter_bank_create(mi_qcounter_bank_t **bank, uint32_t channels, size_t max_period, size_t max_levels);
int mi_qcounter_bank_destroy(mi_qcounter_bank_t *bank);
/* limited to 1 .. max_period; takes effect at the next process(): until then count may exceed period */
int mi_qcounter_bank_set_period(mi_qcounter_bank_t *bank, uint32_t channel, size_t period);
/* levels limited to 1 .. max_levels */
int mi_qcounter_bank_set_levels(mi_qcounter_bank_t *bank, uint32_t channel, size_t levels);
int mi_qcounter_bank_set_min_value(mi_qcounter_bank_t *bank, uint32_t channel, float min_value);
int mi_qcounter_bank_set_max_value(mi_qcounter_bank_t *bank, uint32_t channel, float max_value);
int mi_qcounter_bank_set_value_range(mi_qcounter_bank_t *bank, uint32_t channel, float min_value, float max_value);
int mi_qcounter_bank_set_range(mi_qcounter_bank_t *bank, uint32_t channel, float min_value, float max_value, size_t levels);
int mi_qcounter_bank_needs_update(const mi_qcounter_bank_t *bank, uint32_t channel, int *needs);
/* the recount of every channel whose bUpdate is set, nothing evicted; MI_ESTATE where such a channel has no levels */
int mi_qcounter_bank_update_settings(mi_qcounter_bank_t *bank, void *stream);
/* clear(), :189-196: counters, nHead and nCount; the ring's words and bUpdate stay.  channel UINT32_MAX: all */
int mi_qcounter_bank_clear(mi_qcounter_bank_t *bank, uint32_t channel);
/* src [channels][stride] device rows, read only; count < 2^31, and a count of 0 still takes settings over and evicts */
int mi_qcounter_bank_process(mi_qcounter_bank_t *bank, const float *src, size_t count, size_t stride, void *stream);
/* counters [channels][stride] DEVICE words: with L the largest levels of any channel, words [0, L) are vCounters[0 .. L), word L
 * is below() and word L + 1 above(); stride >= L + 2 */
int mi_qcounter_bank_read(mi_qcounter_bank_t *bank, uint32_t *counters, size_t stride, void *stream);
int mi_qcounter_bank_get_params(const mi_qcounter_bank_t *bank, uint32_t channel, mi_qcounter_params_t *params);
/* ring: NULL, or a HOST array of nCapacity words in storage order; counters: NULL, or a HOST array of max_levels + 2 words as
 * vCounters has them.  set_state: head < nCapacity, count <= nCapacity; state->capacity is not read */
int mi_qcounter_bank_get_state(mi_qcounter_bank_t *bank, uint32_t channel, mi_qcounter_state_t *state, float *ring, uint32_t *counters,
                               void *stream);
int mi_qcounter_bank_set_state(mi_qcounter_bank_t *bank, uint32_t channel, const mi_qcounter_state_t *state, const float *ring,
                               const uint32_t *counters, void *stream);
/* measurements only: 0 compiles the wave-level combining of equal bins out of process() (the result is the same) */
int mi_qcounter_bank_set_wave_combining(mi_qcounter_bank_t *bank, int on);

/*
 * Host-only introspection of the per-section device table (no GPU needed): the
 * chunk-parallel form of the TDF-II section used by the kernel.
 * variant 0 = 16-sample chunks (calls longer than 2048 samples), 1 = 8-sample
 * chunks; a lane owns two adjacent chunks, a wave 64 such pairs.
 * geometry[4] receives {chunk L, lanes, per-lane matrices, floats_per_row};
 * table (may be NULL) receives one row, 2x2 matrices column-major (m00 m10 m01 m11):
 *   {b0 b1 b2 a1 a2 0 0 0 | P P^2 P^4 P^8 P^16 P^32 | (p[k],q[k]) k<L | (P^2)^(i+1) i<16},  P = A^L.
 */
int mi_biquad_section_tables(const mi_biquad_x1_t *chain, int variant, float *table, uint32_t *geometry);

#ifdef __cplusplus
}
#endif

#endif /* MI_DSPU_H_ */
