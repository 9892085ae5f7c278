// SURVEY.md §8 f-1 as written / BASELINE config 5: self.mlp = Linear(64,256) -> ReLU -> Linear(256,64)
// (models/TPNet.py:64-65,129) on the bf16 matrix cores INSIDE the readout kernel: a workgroup of 8 waves forms the Gram
// features of 32 pairs (models/TPNet.py:119-128) into an LDS tile, which is then the B operand (X^T) of layer 1 --
// wave w owns hidden tile w (32 of the 256 units): H^T = W1[32w.., :] . X^T by v_mfma_f32_32x32x16_bf16, bias + ReLU in
// registers, and its accumulator tile is directly the B operand of its slice of layer 2 (Y^T += W2[:, 32w..] . H^T, W2
// pre-permuted as in mlp.hip).  The eight partial Y tiles are added in a FIXED order through LDS (run-to-run identical
// bits).  The features never leave the chip; the weights of a wave (its 32 rows of W1, its 32 columns of W2: 48 VGPRs)
// are loaded once per workgroup.  bf16 operands, fp32 accumulation: 2e-2 class like tpnet_mlp64_bf16 -- opt-in.  L = 3.
// MODE 2 (the default fp32-CLASS path): the bf16 matrix cores with SPLIT operands (mfma_split.hpp: x = hi + lo, three products per
// term, fp32 accumulators: relative error ~2^-16 per product, the accuracy class of the fp32 paths), at 24 bf16 MFMAs per wave and
// tile -- the fp32 matrix cores (v_mfma_f32_32x32x2_f32) take 64 products of four times the cycles for the same class: measured
// and not kept; inputs tpnet_mlp::w1, w2f (f32: the split happens in registers), which makes ONE launch
// the default get_pair_wise_feature for lists of any length.
#include "readout.hpp"
#include "dense_tile.hpp"                 // the dense block on a 32-row LDS tile (shared with anchored_feature.hip)

namespace tpnet {

template <int LPP, int VPL, int W, bool FULL, int MODE>
__global__ __launch_bounds__(MB) void k_pair_feature_bf16(tpnet_state S, const int64_t* __restrict__ u,
                                                          const int64_t* __restrict__ v, int64_t n, double now,
                                                          double lambda, uint32_t flags, const void* __restrict__ w1v,
                                                          const float* __restrict__ b1, const void* __restrict__ w2v,
                                                          const float* __restrict__ b2, float* __restrict__ out_gram,
                                                          float* __restrict__ out, const float* __restrict__ feat_in, int tp) {
    // tp = pairs per tile: 32, or GPB (ONE readout pass per tile: a short list spreads over twice / four times the CUs and a
    // workgroup's readout is one memory round-trip chain deep instead of PT of them; columns of the matrix products beyond tp
    // compute on stale LDS rows and are never stored -- a pair is one column, nothing crosses columns)
    // feat_in != NULL: the dense layers alone on features that already exist ([n][64] f32): the tile is loaded, not formed
    // w1v / w2v: the layouts of dense_tile_weights (bf16, or f32 for the split operands)
    constexpr int L = 3;
    static_assert(MODE == 0 || MODE == 2, "k_pair_feature_bf16: bf16 operands or split operands");
    constexpr bool X3 = MODE == 2;
    constexpr int GPB = MB / LPP;             // pairs per readout pass
    constexpr int PT = 32 / GPB;              // passes per 32-pair tile
    static_assert(GPB * PT == 32 && LPP >= 16, "k_pair_feature_bf16: 16, 32 or 64 lanes per pair");
    __shared__ __attribute__((aligned(16))) float feat[32 * TS];
    __shared__ __attribute__((aligned(16))) float slab[4][32 * TS];
    __shared__ float stage1[1];
    const int tid = threadIdx.x;
    const int gl = tid % LPP, g = tid / LPP;
    const int lane = tid & 63, wave = tid >> 6;
    const bool do_scale = !(flags & TPNET_FLAG_NOT_SCALE);
    const int64_t ntiles = (n + tp - 1) / tp;
    // the first tile's ids BEFORE the weights: vector loads return in order, and the ids (host-mapped memory in the per-batch
    // calls: a PCIe round trip) are the head of the readout's dependent chain -- the weights' 128 KB arrive underneath it
    int64_t uu0 = 0, vv0 = 0;
    if (!feat_in && (int64_t)blockIdx.x < ntiles) {
        const int64_t p = (int64_t)blockIdx.x * tp + g;
        if (g < tp && p < n) { uu0 = u[p]; vv0 = v[p]; }
    }
    // ---- this wave's weights: rows [32 wave, 32 wave + 32) of W1 as A operand, the matching columns of (permuted) W2
    DenseTileW<X3> wt;
    dense_tile_weights<X3>(wt, w1v, b1, w2v, wave, lane);

    // features that already exist: a tile is 512 float4, one per thread; the NEXT tile's piece is fetched while this tile's
    // matrix products run (a tile is otherwise one global round trip + three barriers deep: 8.7 -> ~5 us per tile)
    static_assert(32 * (MF / 4) == MB, "one float4 of the feature tile per thread");
    const int frow = tid / (MF / 4), fcol = tid % (MF / 4);
    float4 fnext = make_float4(0.f, 0.f, 0.f, 0.f);
    if (feat_in && (int64_t)blockIdx.x < ntiles) {
        const int64_t p = (int64_t)blockIdx.x * 32 + frow;
        if (p < n) fnext = *reinterpret_cast<const float4*>(feat_in + p * MF + 4 * fcol);
    }
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        // ---- the features of the tile's 32 pairs -> LDS
        if (feat_in) {
            *reinterpret_cast<float4*>(feat + frow * TS + 4 * fcol) = fnext;
            const int64_t pn = (tile + gridDim.x) * 32 + frow;
            fnext = (tile + gridDim.x < ntiles && pn < n) ? *reinterpret_cast<const float4*>(feat_in + pn * MF + 4 * fcol)
                                                          : make_float4(0.f, 0.f, 0.f, 0.f);
        } else
#pragma unroll 1
        for (int pass = 0; pass * GPB < tp; ++pass) {
            const int pidx = pass * GPB + g;
            const int64_t p = tile * tp + pidx;
            const bool valid = pidx < tp && p < n;
            const bool first = pass == 0 && tile == (int64_t)blockIdx.x;
            const int64_t uu = first ? uu0 : (valid ? u[p] : 0), vv = first ? vv0 : (valid ? v[p] : 0);
            gram_pair<LPP, VPL, W, L, FULL, false, false, false>(S, uu, vv, valid, READER_BID, now, lambda, do_scale,
                                                                 feat + pidx * TS, gl, nullptr, stage1);
        }
        __syncthreads();
        const int npair = (n - tile * tp < tp) ? (int)(n - tile * tp) : tp;
        if (out_gram) {                           // the pre-mlp features, for a backward pass (training)
            for (int i = tid; i < npair * MF; i += MB) out_gram[tile * tp * MF + i] = feat[(i / MF) * TS + (i % MF)];
        }
        // ---- both layers on the tile (dense_tile.hpp), the eight partial tiles added in a fixed order
        dense_tile_partials<X3>(wt, feat, slab, wave, lane);
        {
            const int pair = tid >> 4, o = (tid & 15) * 4;      // 512 threads x 4 outputs = 32 pairs x 64
            if (pair < npair) {
                const float4 y = dense_tile_out4(slab, b2, pair, o);
                *reinterpret_cast<float4*>(out + (tile * tp + pair) * MF + o) = y;
            }
        }
        __syncthreads();                          // the tiles are reused by the next tile of this workgroup
    }
}

bool pair_feature_mfma_supported(const tpnet_state& st) {
    const Geom gm = pick_geom(st.d);
    return st.L == 3 && gm.w == 4 && gm.lpp >= 16;
}

int launch_pair_feature_bf16(const tpnet_state& st, const int64_t* u, const int64_t* v, int64_t n, double now, double lambda,
                             uint32_t flags, const void* w1, const float* b1, const void* w2p, const float* b2,
                             float* out_gram, float* out, hipStream_t s, bool split, const float* feat_in) {
    if (n == 0) return TPNET_OK;
    if (st.L != 3 || (flags & TPNET_FLAG_PACKED)) return TPNET_ERR_BAD_ARG;
    if ((reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(b2)) & 15) return TPNET_ERR_BAD_ARG;
    const Geom gm = pick_geom(st.d);
    if (gm.w != 4 || gm.lpp < 16) return TPNET_ERR_BAD_ARG;       // narrow / scalar rows: readout kernel + tpnet_mlp64_bf16
    const bool full = st.d == gm.lpp * gm.vpl * 4;
    // pairs per tile: one readout pass (GPB pairs) while the list has fewer than two 32-pair tiles per CU
    const int gpb = MB / gm.lpp;
    static const int tp_dev = TPNET_DEV_INT(FEATURE_TP, 0);
    const int tp = feat_in ? 32 : (tp_dev ? (tp_dev < gpb ? gpb : (tp_dev > 32 ? 32 : tp_dev)) : ((gpb < 32 && n <= 256 * 64) ? gpb : 32));
    const int64_t tiles = (n + tp - 1) / tp;
    // (a workgroup's first act is to load its 128 KB of weights: one workgroup per CU, each amortising them over many tiles --
    // 80 000 rows: 51 us with a workgroup per tile up to 2 048, 39 us with 768, 32.5 us with 256; 800 000 rows: 244 / 237)
    static const int grid_cap = TPNET_DEV_INT(MLP_GRID, 256);
    const int grid = (int)(tiles < grid_cap ? tiles : grid_cap);
#define TPNET_PF(LPP_, VPL_, FULL_)                                                                                          \
    do {                                                                                                                     \
        if (split)                                                                                                           \
            hipLaunchKernelGGL((k_pair_feature_bf16<LPP_, VPL_, 4, FULL_, 2>), dim3(grid), dim3(MB), 0, s, st, u, v, n, now,    \
                               lambda, flags, w1, b1, w2p, b2, out_gram, out, feat_in, tp);                                         \
        else                                                                                                                 \
            hipLaunchKernelGGL((k_pair_feature_bf16<LPP_, VPL_, 4, FULL_, 0>), dim3(grid), dim3(MB), 0, s, st, u, v, n, now,    \
                               lambda, flags, w1, b1, w2p, b2, out_gram, out, feat_in, tp);                                         \
    } while (0)
    if (gm.lpp == 16 && gm.vpl == 1) { if (full) TPNET_PF(16, 1, true); else TPNET_PF(16, 1, false); }
    else if (gm.lpp == 16) { if (full) TPNET_PF(16, 2, true); else TPNET_PF(16, 2, false); }
    else if (gm.lpp == 32 && gm.vpl == 1) { if (full) TPNET_PF(32, 1, true); else TPNET_PF(32, 1, false); }
    else if (gm.lpp == 32) { if (full) TPNET_PF(32, 2, true); else TPNET_PF(32, 2, false); }
    else if (gm.vpl == 1) { if (full) TPNET_PF(64, 1, true); else TPNET_PF(64, 1, false); }
    else { if (full) TPNET_PF(64, 2, true); else TPNET_PF(64, 2, false); }
#undef TPNET_PF
    TPNET_HIP_TRY(hipGetLastError());
    return TPNET_OK;
}

// the layouts the fused kernels read, from the Parameters of self.mlp: one launch per optimizer step (the torch expressions --
// two transposes, a contiguous copy and an index gather -- were ~100 us of a training step)
__global__ void k_mlp_prepare(const float* __restrict__ w1, const float* __restrict__ w2, int F, int H, float* __restrict__ w1t,
                              float* __restrict__ w2t, float* __restrict__ w2f) {
    const int n = F * H;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        // w1 [H][F] -> w1t [F][H];  w2 [F][H] -> w2t [H][F]   (coalesced writes)
        { const int f = i / H, h = i - f * H; w1t[i] = w1[h * F + f]; }
        { const int h = i / F, f = i - h * F; w2t[i] = w2[f * H + h]; }
        if (w2f) {            // F = 64, H = 256: i = ((w * 2 + t) * 64 + lane) * 16 + s   (include/tpnet_hip.h, tpnet_mlp::w2f)
            const int s_ = i & 15, lane = (i >> 4) & 63, t = (i >> 10) & 1, w = i >> 11;
            w2f[i] = w2[(32 * t + (lane & 31)) * H + 32 * w + acc_row(s_, lane >> 5)];
        }
    }
}

// the dense layers on existing rows: ONE route for tpnet_mlp64_f32 and the encoder's two-launch calls (encoder.hip)
int launch_mlp_rows(const tpnet_mlp* mlp, const float* x, int64_t n, float* y, hipStream_t s) {
    // long lists: every wave its own tiles, split weights in LDS (mlp_x3.hip)
    if (n >= mlp_x3_from() && mlp_x3_available() &&
        launch_mlp_rows_x3(x, n, reinterpret_cast<const float*>(mlp->w1), mlp->b1, reinterpret_cast<const float*>(mlp->w2f),
                           mlp->b2, y, s) == TPNET_OK)
        return TPNET_OK;
    tpnet_state st{};                      // (not dereferenced when the tile comes from `x`; geometry of d = 128 picks the 32-lane kernel)
    st.N = 1; st.d = 128; st.L = 3;
    return launch_pair_feature_bf16(st, nullptr, nullptr, n, 0.0, 0.0, 0, mlp->w1, mlp->b1, mlp->w2f, mlp->b2, nullptr, y, s, true, x);
}

}  // namespace tpnet

using namespace tpnet;

extern "C" int tpnet_mlp_prepare(const float* w1, const float* w2, int32_t F, int32_t H, float* w1t, float* w2t, float* w2f,
                                 void* stream) {
    if (!w1 || !w2 || !w1t || !w2t || F < 1 || H < 1 || (int64_t)F * H > (1 << 24)) return TPNET_ERR_BAD_ARG;
    if (w2f && (F != 64 || H != 256)) return TPNET_ERR_BAD_ARG;
    const int n = F * H;
    hipLaunchKernelGGL(k_mlp_prepare, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, w1, w2, (int)F, (int)H, w1t, w2t, w2f);
    TPNET_HIP_TRY(hipGetLastError());
    return TPNET_OK;
}

extern "C" int tpnet_pair_feature_bf16(const tpnet_state* st, const int64_t* u, const int64_t* v, int64_t n, double now_time,
                                       double lambda, uint32_t flags, const void* w1_bf16, const float* b1,
                                       const void* w2p_bf16, const float* b2, float* out_gram, float* out, void* stream) {
    if (check_state(st)) return TPNET_ERR_BAD_ARG;
    if (n < 0 || (n > 0 && (!u || !v || !out || !w1_bf16 || !b1 || !w2p_bf16 || !b2))) return TPNET_ERR_BAD_ARG;
    return launch_pair_feature_bf16(*st, u, v, n, now_time, lambda, flags, w1_bf16, b1, w2p_bf16, b2, out_gram, out,
                                    (hipStream_t)stream, false, nullptr);
}

extern "C" int tpnet_mlp64_f32(const float* x, int64_t n, const tpnet_mlp* mlp, float* y, void* stream) {
    if (n < 0 || !mlp || (n > 0 && (!x || !y))) return TPNET_ERR_BAD_ARG;
    if (n == 0) return TPNET_OK;
    if (mlp->F != 64 || mlp->H != 256 || !mlp->w1 || !mlp->w2f || !mlp->b1 || !mlp->b2) return TPNET_ERR_BAD_ARG;
    if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 15) return TPNET_ERR_BAD_ARG;
    return launch_mlp_rows(mlp, x, n, y, (hipStream_t)stream);
}
