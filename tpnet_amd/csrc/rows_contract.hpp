// The contraction over rows of two operands parked TRANSPOSED tile by tile (mixer_channel_train.hip: k_mxc_bwd_weights;
// encoder_input_train.hip: k_eib_weights), once: out[unit][column] = sum over rows of A[row][unit] B[row][column] in the fp32 class of
// mfma_split.hpp.  A is [tiles][AS][32] and B [tiles][BS][32] floats -- element [tile][unit or column][row of the tile] -- so a lane
// loads its 8 consecutive rows of one unit (of one column) as two float4, already in operand order.  Only the walk lives
// here; a kernel keeps its own split of the work over waves, its row parts and its stores.
#pragma once
#include "mfma_split.hpp"

namespace tpnet {

// acc[tt] += sum over the tiles t0 .. t1 - 1 of A[units 32 slice ..]^T . B[columns 32 (ct0 + tt) ..] for tt < nt (nt <= WT).  Lane
// (r, h): unit 32 slice + r of A, column 32 (ct0 + tt) + r of B, rows 8 h .. 8 h + 7 of each 16-row step.  Returns the sum of the A
// operands the lane loaded: after + __shfl_xor(., 32) the sum over the rows of unit 32 slice + r.  Behind it acc[tt][q] of lane
// (r, h) is unit 32 slice + acc_row(q, h), column 32 (ct0 + tt) + r.
template <int WT>
__device__ __forceinline__ float rc_walk(const float* A, int AS, int slice, const float* B, int BS, int ct0,
                                         int nt, int64_t t0, int64_t t1, int r, int h, f32x16 (&acc)[WT]) {
    float asum = 0.0f;
    for (int64_t t = t0; t < t1; ++t) {
        const float* At = A + ((t * AS + 32 * slice + r) * 32 + 8 * h);
        const float* Bt = B + ((t * BS + 32 * ct0 + r) * 32 + 8 * h);
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const float4 a0 = *reinterpret_cast<const float4*>(At + 16 * ks), a1 = *reinterpret_cast<const float4*>(At + 16 * ks + 4);
            asum += ((a0.x + a0.y) + (a0.z + a0.w)) + ((a1.x + a1.y) + (a1.z + a1.w));
            bf16x8 ah, al;
            split8(a0, a1, ah, al);
#pragma unroll
            for (int tt = 0; tt < WT; ++tt) {
                if (tt < nt) {
                    bf16x8 bh, bl;
                    load_split8(Bt + (int64_t)tt * 32 * 32 + 16 * ks, bh, bl);
                    acc[tt] = mm3(ah, al, bh, bl, acc[tt]);
                }
            }
        }
    }
    return asum;
}

}  // namespace tpnet
