// The Lanczos polyphase core of truepeak.hip and oversampler.hip, host and device.  The two banks differ only in what
// they do with an oversampled value.
//
// The arithmetic.  lsp-dsp-lib's lanczos_resample_NxK SCATTERS each input into a zero-filled buffer of pending sums:
// buf[N j + a N + d] += L(d / N) x[j], |d| < a N, zero taps skipped.  An oversampled value is final once input i has been
// added, so the same bits come out of the GATHER
//      y[N i + k] = (((+0 + h_k[2a-1] x[i-2a+1]) + h_k[2a-2] x[i-2a+2]) + ...) + h_k[0] x[i],   h_k[t] = float(L(t - a + k / N))
// in the scatter's order: oldest input first, every product and every sum rounded on its own, and y[N i] = x[i - a] copied.
//
// The state of a channel is its last 2a inputs, on the device, read at the start of a call and written at its end, so a
// bank keeps no positions on the host and a captured graph replays.
//
// The tile walk of both kernels.  A workgroup takes its inputs TILE = BLOCK x 8 at a time into lin[TAPS + p]
// (MI_LANCZOS_FILL_TILE), behind the TAPS inputs before the tile in lin[0 .. TAPS).  After the barrier a thread loads the
// window behind its 8 consecutive outputs (MI_LANCZOS_WINDOW) and makes their values phase by phase; thread tid < TAPS
// reads the next carry lin[n + tid] BEFORE the second barrier and writes it to lin[tid] AFTER the tile's stores, and the
// state at the end.
//
// The device pieces are MACROS, not functions, on purpose: the compiler optimises an inlined helper on its own before it
// inlines it, then pairs the window's LDS reads differently (ds_read_b128 against ds_read2_b64 / ds_read2_b32) and moves
// the kernels' register counts.  The same tokens in place give the same code in either kernel.
#pragma once
#include "mi_common.h"

#include <cmath>

// No tap loop may form a fused multiply-add, whatever -ffp-contract the file is compiled with: the scatter rounds every
// product and every sum (v_pk_mul_f32 / v_pk_add_f32 round each half on its own, so they keep the bits).  The two files
// repeat the pragma in front of their own loops, where a reader looks for it.
#pragma clang fp contract(off)

namespace mi_lanczos
{
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    typedef const __attribute__((address_space(4))) f32x2 *const_pairs;

    // L(x) = sinc(x) sinc(x / a) at x = num / n, in double, rounded to float once (INFERRED and unpinned, DESIGN.md
    // section 4).  |num| makes the table bit-symmetric.  At whole x the kernel is exactly 1 (x = 0) or 0, not the rounding
    // residue of sin(pi x).
    inline float tap(int num, int n, int a)
    {
        if (num % n == 0)
            return (num == 0) ? 1.0f : 0.0f;
        const double x = double(num < 0 ? -num : num) / double(n);
        const double px = M_PI * x, pxa = px / double(a);
        return float((std::sin(px) / px) * (std::sin(pxa) / pxa));
    }

    inline void make_table(int n, int a, float *h)          // [n][2a], row 0 the unit impulse at t = a
    {
        for (int k = 0; k < n; ++k)
            for (int t = 0; t < 2 * a; ++t)
                h[k * 2 * a + t] = tap(n * (t - a) + k, n, a);
    }

    // A device table holds the phases k = 1 .. N-1 of N = 2, 3, 4, 6, 8 one after the other, PHASES in all: the phases
    // before those of N (-1: no kernel for N) ...
    constexpr int FACTORS[] = { 2, 3, 4, 6, 8 };
    constexpr int PHASES = 1 + 2 + 3 + 5 + 7;
    __host__ __device__ constexpr int phases_before(int n)
    {
        return (n == 2) ? 0 : (n == 3) ? 1 : (n == 4) ? 3 : (n == 6) ? 6 : (n == 8) ? 11 : -1;
    }
    // ... each phase 2a pairs that hold a coefficient twice, the packed multiply's operand: (n - 1) * 2a pairs to dst
    inline void phase_pairs(int n, int a, f32x2 *dst)
    {
        for (int k = 1; k < n; ++k)
            for (int t = 0; t < 2 * a; ++t)
            {
                const float c = tap(n * (t - a) + k, n, a);
                *dst++ = f32x2{ c, c };
            }
    }

    // Rows of `count` inputs: enough workgroups per row to fill the device (1024 over all `channels` rows, at most
    // max_splits and one per tile), every split a whole number of tiles.  One split: the workgroup owns its row.
    struct split_plan { uint32_t splits, span; };
    inline split_plan plan_splits(uint32_t count, uint32_t tile, uint32_t channels, uint32_t max_splits)
    {
        const uint32_t tiles = (count + tile - 1) / tile;
        if (tiles < 2)
            return { 1, count };
        uint32_t want = (1024 + channels - 1) / channels;
        want = (want < max_splits) ? want : max_splits;
        want = (want < tiles) ? want : tiles;
        const uint32_t span = ((tiles + want - 1) / want) * tile;
        return { (count + span - 1) / span, span };
    }

    // What clears state or allocates cannot go into a graph: the banks ask, refuse, and name the call to make beforehand.
    using mi::capturing;
} // namespace mi_lanczos

// lin[TAPS + p] = input p of the tile that starts at xs[t0], zero beyond its n inputs; PT values per thread
#define MI_LANCZOS_FILL_TILE(lin, xs, t0, n, tid, TAPS, BLOCK, PT) \
    _Pragma("unroll") for (int j_ = 0; j_ < (PT); ++j_) \
    { \
        const uint32_t p_ = uint32_t(j_ * (BLOCK) + (tid)); \
        (lin)[(TAPS) + p_] = (p_ < (n)) ? (xs)[(t0) + p_] : 0.0f; \
    }

// float r[RL]: r[j] = lin[o + j], as float4 (RL and o multiples of 4, lin 16-byte aligned)
#define MI_LANCZOS_WINDOW(r, lin, o, RL) \
    float r[RL]; \
    _Pragma("unroll") for (int j_ = 0; j_ < (RL) / 4; ++j_) \
    { \
        const float4 v_ = *reinterpret_cast<const float4 *>(&(lin)[(o) + 4 * j_]); \
        r[4 * j_] = v_.x; r[4 * j_ + 1] = v_.y; r[4 * j_ + 2] = v_.z; r[4 * j_ + 3] = v_.w; \
    }

// The first R values of a window as pairs of neighbours, f32x2 ev[R / 2], od[R / 2 - 1]: the even-aligned ones are the
// loaded registers, the odd ones are made.
#define MI_LANCZOS_PAIRS(ev, od, r, R) \
    mi_lanczos::f32x2 ev[(R) / 2], od[(R) / 2 - 1]; \
    _Pragma("unroll") for (int j_ = 0; j_ < (R) / 2; ++j_) \
        ev[j_] = mi_lanczos::f32x2{ (r)[2 * j_], (r)[2 * j_ + 1] }; \
    _Pragma("unroll") for (int j_ = 0; j_ < (R) / 2 - 1; ++j_) \
        od[j_] = mi_lanczos::f32x2{ (r)[2 * j_ + 1], (r)[2 * j_ + 2] }

// f32x2 acc: outputs 2q, 2q + 1 of the phase with the coefficient pairs hk.  r[TAPS + j] being the newest input of
// output j, they read inputs r[TAPS + 2q - t], r[TAPS + 2q + 1 - t] and share one packed multiply and one packed add
// per tap.  The caller's loop over the phases is NOT unrolled (#pragma unroll 1): one phase's 2a coefficient pairs (4a
// SGPRs, loaded as they are stored) are all the scalar registers hold, where all phases at once would spill them into
// vector lanes.
// FROM_ZERO: the sum starts from +0.0f, as the reference's zero-filled buffer makes it, so a sum of negative zeros is +0
// (the oversampler keeps the value, sign of a zero included).  Otherwise it starts from the first product: 0 + p == p but
// for the sign of a zero, which the true-peak meter's |.| drops, and that saves a packed add per pair and phase.
#define MI_LANCZOS_PAIR_SUM(acc, hk, ev, od, TAPS, q, FROM_ZERO) \
    mi_lanczos::f32x2 acc = mi_lanczos::f32x2{ 0.0f, 0.0f }; \
    _Pragma("unroll") for (int t_ = (TAPS) - 1; t_ >= 0; --t_) \
    { \
        const int b_ = (TAPS) + 2 * (q) - t_; \
        const mi_lanczos::f32x2 p_ = (hk)[t_] * ((b_ % 2 == 0) ? ev[b_ / 2] : od[b_ / 2]); \
        acc = (!(FROM_ZERO) && t_ == (TAPS) - 1) ? p_ : acc + p_; \
    }
