// The tile walk of the envelope dynamics (dynamics_device.h, gate.hip, dynproc.hip) and sidechain.hip, device side: a serial
// per-channel chain over rows with element-wise work beside it.  The kernels differ in what they prepare, chain and emit.
//
// A workgroup of BLOCK threads owns GROUP channels and walks their rows in tiles of TILE samples through LDS, two buffers
// (tile[2][GROUP][ROW], declared by the kernel):
//     wave 0           the chain over tile k, lane c on row c, in place in LDS (chain_batches reads BATCH samples ahead)
//     waves 1 .. GROUP one row each, four samples per lane: emit(k - 1) out of LDS into memory, then prepare(k + 1) out of
//                      memory into the buffer just emptied
// one barrier per tile, all of them in MI_TILE_CHAIN_WALK.  THE INVARIANT that makes in-place calls safe: a tile is whole in
// LDS before anything of it is stored, and tile k + 1 is loaded after tile k - 1 was stored (by the same lane, in program
// order), so an output row may be an input row.  Whoever changes how many tiles are in flight changes the walk and keeps this.
//
// Functions and templates where the compiler makes the same registers, LDS and occupancy of them as of the text written
// out in place: the roles, the extents, the stores and the chain's batch loop (the two __noinline__ chains keep every
// instruction).  The walk is a MACRO, as in lanczos_device.h: as a template over three callables it moved
// compressor_kernel from 81 to 80 VGPRs (taken by value) or grew it by 200 bytes (by reference); the same tokens in place
// give the same kernel.  The LOADS of a lane's four samples stay written out in the kernels: one load_quad for them,
// tried as a function and as a macro, moved the register counts at every site but one (compressor_kernel 81 -> 77 VGPRs,
// or 58 -> 60 SGPRs with only the audio load replaced; sidechain_kernel 83 -> 79; five waves per SIMD -> six).
#pragma once
#include "mi_common.h"

// the chains round every product and every sum on their own, whatever -ffp-contract the file is compiled with; the two
// files repeat the pragma in front of their own steps
#pragma clang fp contract(off)

namespace mi_tile_chain
{
    constexpr int GROUP   = 4;                  // channels of a workgroup: 1024 channels are 256 workgroups, one per CU
    constexpr int TILE    = 256;                // samples of a row per trip through LDS
    constexpr int ROW     = TILE + 4;           // floats between rows in LDS: lane c's 16-byte reads start at bank 4c
    constexpr int HELPERS = GROUP * 64;         // one wave per row
    constexpr int BLOCK   = 64 + HELPERS;
    constexpr int BATCH   = 8;                  // samples the chain reads ahead of itself

    typedef float f32x4 __attribute__((ext_vector_type(4)));
    typedef __attribute__((address_space(3))) float lds_float;
    typedef __attribute__((address_space(3))) f32x4 lds_f32x4;

    // tile k of a row of `count` samples: samples [t0, t0 + n)
    struct extent { uint32_t t0, n; };
    __device__ __forceinline__ extent tile_extent(uint32_t count, uint32_t k)
    {
        const uint32_t t0 = k * TILE;
        return extent{ t0, (count - t0 < uint32_t(TILE)) ? count - t0 : uint32_t(TILE) };
    }

    // A lane's four samples c .. c + 3 of a tile of n into a row in memory (dst: the row at sample c): 16 bytes where the row
    // allows it (`wide`: its base and stride are 16-byte aligned) and the four are all there, otherwise those below n one by
    // one.
    __device__ __forceinline__ void store_quad(float *dst, const float (&v)[4], bool wide, uint32_t c, uint32_t n)
    {
        if (wide && c + 4 <= n)
            *reinterpret_cast<float4 *>(dst) = make_float4(v[0], v[1], v[2], v[3]);
        else
        {
            #pragma unroll
            for (uint32_t j = 0; j < 4; ++j)
                if (c + j < n)
                    dst[j] = v[j];
        }
    }

    // The chain over samples [i, to) of one row in LDS, in place: row[i] = step(row[i]), in order.  From the first multiple of
    // four on, batches of BATCH: the next batch's two 16-byte reads are issued before this batch's chain, two 16-byte writes
    // after it.
    template <class Step> __device__ __forceinline__ void chain_batches(lds_float *row, uint32_t i, uint32_t to, Step step)
    {
        for (; i < to && (i & 3u) != 0; ++i)
            row[i] = step(row[i]);
        if (i + BATCH <= to)
        {
            f32x4 a = *reinterpret_cast<lds_f32x4 *>(row + i), b = *reinterpret_cast<lds_f32x4 *>(row + i + 4);
            for (; i + BATCH <= to; i += BATCH)
            {
                float v[BATCH] = { a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w };
                const uint32_t next = (i + 2 * BATCH <= to) ? i + BATCH : i;   // the next batch, before this one's chain
                a = *reinterpret_cast<lds_f32x4 *>(row + next);
                b = *reinterpret_cast<lds_f32x4 *>(row + next + 4);
                #pragma unroll
                for (int j = 0; j < BATCH; ++j)
                    v[j] = step(v[j]);
                *reinterpret_cast<lds_f32x4 *>(row + i) = f32x4{ v[0], v[1], v[2], v[3] };
                *reinterpret_cast<lds_f32x4 *>(row + i + 4) = f32x4{ v[4], v[5], v[6], v[7] };
            }
        }
        for (; i < to; ++i)
            row[i] = step(row[i]);
    }

    // What a thread is: the chain's lane of row r (wave 0) or one of the helper wave of row r (uniform over the wave, so it
    // sits in a scalar register), with the samples c .. c + 3 of every tile.  valid: the row has a channel.
    struct role
    {
        bool chain, valid;
        uint32_t lane, r, ch, c;
    };
    __device__ __forceinline__ role my_role(uint32_t channels)
    {
        const int tid = threadIdx.x, lane = tid & 63;
        role me;
        me.chain = tid < 64;
        me.lane = uint32_t(lane);
        me.r = me.chain ? uint32_t(lane) : uint32_t(__builtin_amdgcn_readfirstlane((tid >> 6) - 1));
        me.ch = blockIdx.x * GROUP + me.r;
        me.valid = me.r < uint32_t(GROUP) && me.ch < channels;
        me.c = uint32_t(lane) * 4;
        return me;
    }
} // namespace mi_tile_chain

// The walk over the tiles of `count` > 0 samples for the thread `me` (a role): PREPARE fills buffer k & 1 of tile k, CHAIN
// runs over it, EMIT empties it -- three expressions in `k`, a name of the caller's choice.  The barriers and the k - 1 /
// k + 1 order of the invariant above are here and nowhere else.
#define MI_TILE_CHAIN_WALK(me, count, k, PREPARE, CHAIN, EMIT) \
    do { \
        const uint32_t tiles_ = ((count) + mi_tile_chain::TILE - 1) / mi_tile_chain::TILE; \
        if ((me).valid && !(me).chain) \
        { \
            const uint32_t k = 0; \
            PREPARE; \
        } \
        __syncthreads(); \
        for (uint32_t k_ = 0; k_ < tiles_; ++k_) \
        { \
            if ((me).chain) \
            { \
                if ((me).valid) \
                { \
                    const uint32_t k = k_; \
                    CHAIN; \
                } \
            } \
            else if ((me).valid) \
            { \
                if (k_ > 0) \
                { \
                    const uint32_t k = k_ - 1; \
                    EMIT; \
                } \
                if (k_ + 1 < tiles_) \
                { \
                    const uint32_t k = k_ + 1; \
                    PREPARE; \
                } \
            } \
            __syncthreads(); \
        } \
        if ((me).valid && !(me).chain) \
        { \
            const uint32_t k = tiles_ - 1; \
            EMIT; \
        } \
    } while (0)
