// Weight gradients of self.mlp = Linear(F, 4F) -> ReLU -> Linear(4F, F) on the matrix cores: the phases that k_mlp64_bwd
// (mlp_bwd.hip, F = 64, both arithmetic classes) and k_mlp_rows_bwd<L> (mlp_rows_bwd.hip, F = 16 and 36) share.  The mapping: per
// tile of 32 rows, wave w owns hidden units [32 w, 32 w + 32):
//   pre^T = W1[32w.., :] . X^T + b1,  H^T = relu(pre^T)          (recomputed; HOW is each kernel's own, as is how the rows arrive)
//   gH^T  = (W2^T[32w.., :] . gY^T) * (pre^T > 0)
//   gW1[32w.., :] += gH^T . X        gW2[:, 32w..] += gY^T . H      (contraction over the 32 rows: the tiles go through LDS
//                                                                   transposed, [unit][row], so that they load as operands)
//   gb1[32w..]   += sum_rows gH                                     (fp32, per-lane partial sums, reduced once per workgroup;
//                                                                    gb2 = sum_rows gY is a column sum the caller takes)
// The accumulators live in registers over all tiles of a workgroup; every workgroup writes ONE partial result
// (gW1 [H][F] | gW2 [F][H] | gb1 [H], unpadded), and the caller adds the partials in a fixed order: run-to-run identical bits.
// NP = planes of every LDS tile: 1 (bf16 operands, the opt-in 1e-2 class) or 2 (hi and lo: the fp32 class of mfma_split.hpp).
// A tile in LDS is [plane][unit][WG_QS], the 32 rows of the tile along a line; X^T and gY^T have 32 NT units (columns of x / gy,
// zero beyond F), a wave's H^T and gH^T have 32.  Nothing of the padding (H % 32, F % 32) is written into a partial, and a geometry
// without padding carries no predicate for it: they are compile-time.
#pragma once
#include "mfma_split.hpp"

namespace tpnet {

static constexpr int WG_QS = 40;           // bf16 elements per LDS row of a [unit][32 rows] tile (80 B: 16-byte aligned, bank spread)

// partial layout per workgroup (floats)
template <int F, int H>
struct WgradPartial {
    static constexpr int W1 = 0, W2 = H * F, B1 = 2 * H * F, TOT = 2 * H * F + H;
};

// workgroups of a launch = partials written (workgroups beyond do not exist: the caller sums only the first
// min(n_partial, ceil(n / 32)) partials)
inline int wgrad_grid(int64_t n, int32_t n_partial) {
    const int64_t tiles = (n + 31) / 32;
    return (int)(tiles < n_partial ? tiles : n_partial);
}

// c += A B over one 16-deep step; NP = 2: operands in two pieces [0] = hi, [1] = lo
template <int NP>
__device__ __forceinline__ f32x16 mm(const bf16x8* a, const bf16x8* b, f32x16 c) {
    if constexpr (NP == 2) return mm3(a[0], a[1], b[0], b[1], c);
    else return mfma(a[0], b[0], c);
}

// the bias of this wave's hidden slice in accumulator order (in LDS: 16 registers the fp32 class does not have):
// float 16 * (2 wave + h) + q = b1[32 wave + acc_row(q, h)], zero beyond H; read behind a barrier through the returned pointer
template <int H>
__device__ __forceinline__ const float4* wgrad_stage_bias(float* bias_l, const float* __restrict__ b1, int wave, int r, int h) {
    if (r == 0) {
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int hid = 32 * wave + acc_row(q, h);
            bias_l[16 * (2 * wave + h) + q] = (H % 32 == 0 || hid < H) ? b1[hid] : 0.0f;
        }
    }
    return reinterpret_cast<const float4*>(bias_l + 16 * (2 * wave + h));
}

// pre (bias included; register q = hidden unit acc_row(q, h), column = row r of the tile) -> which units are on (rows >= n: none)
// -> H = relu(pre) in NP pieces -> this wave's H^T tile
template <int NP>
__device__ __forceinline__ uint32_t wgrad_hidden(const f32x16& pre, bool valid, __bf16* hrow, int r, int h) {
    uint32_t on_mask = 0;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int hq = acc_row(q, h);
        const bool on = valid && pre[q] > 0.0f;
        on_mask |= (on ? 1u : 0u) << q;
        __bf16 hp[NP];
        split1(on ? pre[q] : 0.0f, hp);
#pragma unroll
        for (int pl = 0; pl < NP; ++pl) hrow[pl * 32 * WG_QS + hq * WG_QS + r] = hp[pl];
    }
    return on_mask;
}

// gH = (W2^T gY) where the unit is on -> gb1's per-lane sums -> NP pieces -> this wave's gH^T tile
template <int NP>
__device__ __forceinline__ void wgrad_ghidden(const f32x16& gh, uint32_t on_mask, float (&gb1)[16], __bf16* grow, int r, int h) {
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int hq = acc_row(q, h);
        const float gv = ((on_mask >> q) & 1u) ? gh[q] : 0.0f;
        gb1[q] += gv;
        __bf16 gp[NP];
        split1(gv, gp);
#pragma unroll
        for (int pl = 0; pl < NP; ++pl) grow[pl * 32 * WG_QS + hq * WG_QS + r] = gp[pl];
    }
}

// one tile's contraction (behind the barrier that follows the four tiles' writes):
// gW1[32w + m][32 t + r] += sum_rows gH^T[m][row] X[row][32 t + r]:  A = gH^T rows, B[k = row][n] = X^T[n][row]
// gW2[32 t + m][32w + r] += sum_rows gY^T[32 t + m][row] H[row][32w + r]: A = gY^T rows, B = H^T[r][row]
template <int NP, int NT>
__device__ __forceinline__ void wgrad_contract(const __bf16* xt, const __bf16* gyt, const __bf16* hrow, const __bf16* grow,
                                               f32x16 (&gw1)[NT], f32x16 (&gw2)[NT], int r, int h) {
    constexpr int FT = 32 * NT;                  // units of the X^T / gY^T tiles
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int ko = 16 * s + 8 * h;           // 8 consecutive rows of the tile
        bf16x8 a_gh[NP], b_h[NP];
#pragma unroll
        for (int pl = 0; pl < NP; ++pl) {
            a_gh[pl] = *reinterpret_cast<const bf16x8*>(grow + pl * 32 * WG_QS + r * WG_QS + ko);
            b_h[pl] = *reinterpret_cast<const bf16x8*>(hrow + pl * 32 * WG_QS + r * WG_QS + ko);
        }
#pragma unroll
        for (int t2 = 0; t2 < NT; ++t2) {
            bf16x8 b_x[NP], a_gy[NP];
#pragma unroll
            for (int pl = 0; pl < NP; ++pl) {
                b_x[pl] = *reinterpret_cast<const bf16x8*>(xt + pl * FT * WG_QS + (32 * t2 + r) * WG_QS + ko);
                a_gy[pl] = *reinterpret_cast<const bf16x8*>(gyt + pl * FT * WG_QS + (32 * t2 + r) * WG_QS + ko);
            }
            gw1[t2] = mm<NP>(a_gh, b_x, gw1[t2]);
            gw2[t2] = mm<NP>(a_gy, b_h, gw2[t2]);
        }
    }
}

// this workgroup's partial result: the unpadded entries only; gb1 summed over the 32 rows (lanes r) of each half h, register
// q <-> hidden unit acc_row(q, h)
template <int F, int H, int NT>
__device__ __forceinline__ void wgrad_store_partial(float* __restrict__ partial, const f32x16 (&gw1)[NT], const f32x16 (&gw2)[NT],
                                                    const float (&gb1)[16], int wave, int r, int h) {
    using PL = WgradPartial<F, H>;
    constexpr bool PH = H % 32 != 0, PF = F % 32 != 0;                    // padded hidden units / columns exist
    float* P = partial + (int64_t)blockIdx.x * PL::TOT;
#pragma unroll
    for (int t2 = 0; t2 < NT; ++t2) {
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int m = acc_row(q, h);
            if ((!PH || wave * 32 + m < H) && (!PF || 32 * t2 + r < F)) P[PL::W1 + (wave * 32 + m) * F + 32 * t2 + r] = gw1[t2][q];
            if ((!PF || 32 * t2 + m < F) && (!PH || wave * 32 + r < H)) P[PL::W2 + (32 * t2 + m) * H + wave * 32 + r] = gw2[t2][q];
        }
    }
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        float v = gb1[q];
#pragma unroll
        for (int o = 16; o >= 1; o >>= 1) v += __shfl_xor(v, o, 32);
        const int hid = wave * 32 + acc_row(q, h);
        if (r == 0 && (!PH || hid < H)) P[PL::B1 + hid] = v;
    }
}

}  // namespace tpnet
