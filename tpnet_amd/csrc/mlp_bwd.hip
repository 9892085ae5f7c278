// Backward of self.mlp = Linear(64,256) -> ReLU -> Linear(256,64) (models/TPNet.py:64-65) with respect to its four weight
// tensors, on the bf16 matrix cores ("needs a backward for training (grad w.r.t. weights only -- P has no
// grad)").  One kernel: per tile of 32 pairs, wave w (of 8) owns hidden units [32w, 32w+32); the mapping, the partial result per
// workgroup and the phases shared with mlp_rows_bwd.hip (F = 16 and 36) are stated in mlp_wgrad.hpp: the bias staging, the hidden
// tile's way to LDS, the contraction, the partial store, the launch rule.  pre^T is recomputed as the forward kernel forms it.
// Two arithmetic classes (template F32): bf16 operands with fp32 accumulation (the opt-in 1e-2 class), and -- round 4 -- the fp32
// class of the default forward paths: two-piece operands, three products per term (mfma_split.hpp), weights taken from the f32 Parameters (mlp[0].weight [256][64] and the
// prepared transpose of mlp[2].weight, tpnet_mlp::w2t [256][64]); the four LDS tiles exist twice (hi and lo planes).  What it
// replaces in a training step at the encoder level: five fp32 torch GEMMs and three elementwise passes over 80 000 x 256 floats
// per call (~1 ms).  This kernel's own: every wave loads the tile's rows itself, pre^T on the class's operands, the bf16 class.
#include "tpnet_common.h"
#include "mlp_wgrad.hpp"

namespace tpnet {

static constexpr int BB = 512;             // 8 waves = the 8 hidden tiles
static constexpr int BF = 64, BH = 256;
static constexpr int RS = WG_QS;           // bf16 elements per LDS row of a [unit][32 pairs] tile

// W1S / W2S: bf16 [256][64] (F32 = false) or f32 [256][64] (F32 = true: mlp[0].weight, and mlp[2].weight transposed)
template <bool F32>
__global__ __launch_bounds__(BB) void k_mlp64_bwd(const float* __restrict__ X, const float* __restrict__ GY, int64_t n,
                                                  const void* __restrict__ w1v, const float* __restrict__ b1,
                                                  const void* __restrict__ w2tv, float* __restrict__ partial) {
    constexpr int NP = F32 ? 2 : 1;                                       // planes: hi (and lo)
    extern __shared__ __attribute__((aligned(16))) __bf16 lds[];
    __bf16* xt = lds;                                                     // X^T   [plane][feature][pair]
    __bf16* gyt = xt + NP * BF * RS;                                      // gY^T  [plane][output][pair]
    __bf16* ht_all = gyt + NP * BF * RS;                                  // H^T   [wave][plane][hidden of the wave's tile][pair]
    __bf16* ght_all = ht_all + 8 * NP * 32 * RS;                          // gH^T
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    // this wave's rows of W1 and of W2^T as A operands (k = features / outputs)
    bf16x8 a1[4][NP], a2[4][NP];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const int off = (wave * 32 + r) * BF + 16 * s + 8 * h;
        if constexpr (F32) {
            load_split8(reinterpret_cast<const float*>(w1v) + off, a1[s][0], a1[s][NP - 1]);
            load_split8(reinterpret_cast<const float*>(w2tv) + off, a2[s][0], a2[s][NP - 1]);
        } else {
            a1[s][0] = *reinterpret_cast<const bf16x8*>(reinterpret_cast<const __bf16*>(w1v) + off);
            a2[s][0] = *reinterpret_cast<const bf16x8*>(reinterpret_cast<const __bf16*>(w2tv) + off);
        }
    }
    const float4* bias4 = wgrad_stage_bias<BH>(reinterpret_cast<float*>(ght_all + 8 * NP * 32 * RS), b1, wave, r, h);
    __syncthreads();
    f32x16 gw1[2], gw2[2];                   // gW1[32w + m][32 nt + r], nt = 0,1;  gW2[32 mt + m][32w + r], mt = 0,1
    float gb1[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) { gw1[0][q] = 0.f; gw1[1][q] = 0.f; gw2[0][q] = 0.f; gw2[1][q] = 0.f; gb1[q] = 0.f; }

    const int64_t ntiles = (n + 31) / 32;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t pair = tile * 32 + r;
        const bool valid = pair < n;
        const float* xr = X + (valid ? pair : 0) * BF;
        const float* gr = GY + (valid ? pair : 0) * BF;
        __bf16* hrow = ht_all + wave * NP * 32 * RS;
        __bf16* grow = ght_all + wave * NP * 32 * RS;
        // one operand set at a time (X, then gY: the fp32 class holds 160 registers of weights and accumulators for the whole
        // launch): rows -> pieces, the transposed tile to LDS (wave 0: X^T, wave 1: gY^T; every wave holds the same values:
        // element [16 s + 8 h + j][pair r]), then this wave's hidden tile -- register q = hidden row acc_row(q, h),
        // column = pair r
        uint32_t on_mask = 0;
        auto load_rows = [&](const float* rowp, bf16x8 (&b)[4][NP], __bf16* dst, bool store) {
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                if constexpr (F32) load_split8(rowp + 16 * s + 8 * h, b[s][0], b[s][NP - 1]);
                else b[s][0] = load_cvt8(rowp + 16 * s + 8 * h);
                if (!valid) {
#pragma unroll
                    for (int pl = 0; pl < NP; ++pl)
#pragma unroll
                        for (int j = 0; j < 8; ++j) b[s][pl][j] = (__bf16)0.0f;
                }
            }
            if (store) {
#pragma unroll
                for (int pl = 0; pl < NP; ++pl)
#pragma unroll
                    for (int s = 0; s < 4; ++s)
#pragma unroll
                        for (int j = 0; j < 8; ++j) dst[pl * BF * RS + (16 * s + 8 * h + j) * RS + r] = b[s][pl][j];
            }
        };
        {
            bf16x8 bx[4][NP];
            load_rows(xr, bx, xt, wave == 0);
            f32x16 pre;
#pragma unroll
            for (int q = 0; q < 16; ++q) pre[q] = 0.f;
#pragma unroll
            for (int s = 0; s < 4; ++s) pre = mm<NP>(a1[s], bx[s], pre);
#pragma unroll
            for (int q4 = 0; q4 < 4; ++q4) {
                const float4 bq = bias4[q4];
                pre[4 * q4] += bq.x; pre[4 * q4 + 1] += bq.y; pre[4 * q4 + 2] += bq.z; pre[4 * q4 + 3] += bq.w;
            }
            on_mask = wgrad_hidden<NP>(pre, valid, hrow, r, h);
        }
        {
            bf16x8 bg[4][NP];
            load_rows(gr, bg, gyt, wave == 1);
            f32x16 gh;
#pragma unroll
            for (int q = 0; q < 16; ++q) gh[q] = 0.f;
#pragma unroll
            for (int s = 0; s < 4; ++s) gh = mm<NP>(a2[s], bg[s], gh);
            wgrad_ghidden<NP>(gh, on_mask, gb1, grow, r, h);
        }
        __syncthreads();
        wgrad_contract<NP, 2>(xt, gyt, hrow, grow, gw1, gw2, r, h);
        __syncthreads();                          // the tiles are rewritten by the next tile
    }
    wgrad_store_partial<BF, BH, 2>(partial, gw1, gw2, gb1, wave, r, h);
}

template <bool F32>
static constexpr size_t bwd_lds_bytes() { return (size_t)(F32 ? 2 : 1) * (2 * BF * RS + 2 * 8 * 32 * RS) * sizeof(__bf16) + 256 * sizeof(float); }

}  // namespace tpnet

using namespace tpnet;

extern "C" {

int64_t tpnet_mlp64_bwd_partial_floats(void) { return (int64_t)WgradPartial<BF, BH>::TOT; }

int tpnet_mlp64_bwd_bf16(const float* x, const float* gy, int64_t n, const void* w1_bf16, const float* b1,
                         const void* w2t_bf16, float* partial, int32_t n_partial, void* stream) {
    if (n < 1 || !x || !gy || !w1_bf16 || !b1 || !w2t_bf16 || !partial || n_partial < 1) return TPNET_ERR_BAD_ARG;
    const int grid = wgrad_grid(n, n_partial);
    hipLaunchKernelGGL(k_mlp64_bwd<false>, dim3((unsigned)grid), dim3(BB), bwd_lds_bytes<false>(), (hipStream_t)stream, x, gy, n,
                       w1_bf16, b1, w2t_bf16, partial);
    TPNET_HIP_TRY(hipGetLastError());
    return grid;
}

int tpnet_mlp64_bwd_f32(const float* x, const float* gy, int64_t n, const tpnet_mlp* mlp, float* partial, int32_t n_partial,
                        void* stream) {
    if (n < 1 || !x || !gy || !mlp || !mlp->w1 || !mlp->w2t || !mlp->b1 || mlp->F != 64 || mlp->H != 256 || !partial || n_partial < 1)
        return TPNET_ERR_BAD_ARG;
    if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(gy) | reinterpret_cast<uintptr_t>(mlp->w1) |
         reinterpret_cast<uintptr_t>(mlp->w2t)) & 15)
        return TPNET_ERR_BAD_ARG;
    static LdsOptIn lds;
    if (!lds.granted({reinterpret_cast<const void*>(k_mlp64_bwd<true>)}, bwd_lds_bytes<true>())) return TPNET_ERR_BAD_ARG;
    const int grid = wgrad_grid(n, n_partial);
    hipLaunchKernelGGL(k_mlp64_bwd<true>, dim3((unsigned)grid), dim3(BB), bwd_lds_bytes<true>(), (hipStream_t)stream, x, gy, n,
                       (const void*)mlp->w1, mlp->b1, (const void*)mlp->w2t, partial);
    TPNET_HIP_TRY(hipGetLastError());
    return grid;
}

}  // extern "C"
