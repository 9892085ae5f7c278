// Backward of self.mlp = Linear(F, 4F) -> ReLU -> Linear(4F, F) (models/TPNet.py:63-65) with respect to its four weight tensors
// for rp_num_layer L = 1 and L = 2 (F = 16 and 36, H = 64 and 144), fp32 class only, on the padded geometry of the forward
// (mlp_wave_tile.hpp).  The mapping, the partial result and the phases shared with mlp_bwd.hip (F = 64) are mlp_wgrad.hpp's: the bias
// staging, the hidden tile's way to LDS, the contraction, the partial store, the launch rule.  Same arithmetic for the three
// products that carry gradients (two-piece bf16 operands, three products per term in mm3's order on v_mfma_f32_32x32x16_bf16,
// fp32 accumulators).  This kernel's own: how the rows arrive (LOADS) and how pre^T is formed (PRE-ACTIVATIONS).
//
// GEOMETRY (RowsBwdGeo; F, H and the padded shapes are MlpRowsGeo's of mlp_wave_tile.hpp).  One wave per hidden slice:
//   L  F   H    k-steps (features / outputs)   waves = slices   tiles of gW1 columns / gW2 rows   threads   VGPRs   LDS bytes
//   1  16   64  1                              2                1 (half used)                     128      144      36 096
//   2  36  144  3 (48 columns)                 5 (160 units)    2 (64)                            320      237      81 536
// (registers of the compiled gfx950 kernels -- at L = 1 112 + 32 accumulation registers -- no scratch; the LDS is dynamic, L = 2
// needs the opt-in; 320 threads are two waves on one SIMD at most: 256 registers each.)  At L = 2 a wave
// carries 64 accumulator registers (gW1[32][64] and gW2[64][32]), 16 of gb1 and 42 of weight operands for the whole launch.
// PRE-ACTIVATIONS.  pre^T alone is formed in exact f32 (v_mfma_f32_32x32x2_f32, F / 2 instructions per tile, the accumulator
// starting at the bias), not on split operands: pre > 0 decides which (row, unit) pairs reach gW1, gb1 and gW2 at all, and at
// 2^-16 per product that decision is not always an fp32 evaluation's -- on split operands one unit among the 144 000
// pre-activations of a 1 000-row list at F = 36 moved a row of gW1 by 0.29 against autograd through the torch layers
// (tests/test_mlp_rows.py::test_gradients_through_the_module_route allows 1e-3).  H = relu(pre) is then split in two pieces like
// every other operand.
// LOADS.  A tile's 32 rows of x and of gy are 32 F consecutive floats each: the workgroup reads them ONCE, coalesced, one float4 per
// thread and input, one tile ahead of the matrix work, and parks them in LDS as fp32 rows, from which every wave takes its B
// operands.  (Every wave loading the rows itself, as mlp_bwd.hip does, measured 6.2 us per tile at L = 2 against 4.3 this way, both
// with pre^T on split operands: five waves' strided reads of the same rows.)
// PADDING RULES (the forward's, mlp_wave_tile.hpp, here for two inputs).  Columns >= F of x AND of gy are zero because the READ of the parked row is
// masked in whole float4s (F % 4 == 0), never because a zero weight multiplies them: it would take the next row's values.  Rows >= n
// of the last tile are zero because the global load is masked, in float4s that lie wholly inside or wholly outside n * F floats:
// the contraction runs over the rows, so a row read past the list would add into every gradient (and NaN * 0 = NaN).  Padded
// hidden units have zero weights and a zero bias: pre = 0 is "off", H = gH = 0.  Rows >= 16 * k-steps of the transposed X / gY
// tiles are zeroed once and never rewritten.  Nothing of the padding is written into a partial.
#include "tpnet_common.h"
#include "mlp_wgrad.hpp"

namespace tpnet {

static constexpr int QS = WG_QS;           // bf16 elements per LDS row of a [unit][32 rows] tile

template <int L>
struct RowsBwdGeo {
    static constexpr int F = (2 * L + 2) * (2 * L + 2), H = 4 * F;
    static constexpr int KS = (F + 15) / 16;          // k-steps over the features (layer 1) and over the outputs (gH)
    static constexpr int NS = (H + 31) / 32;          // hidden slices of 32 units = waves
    static constexpr int NT = (F + 31) / 32;          // 32-wide tiles of gW1's columns and of gW2's rows
    static constexpr int BLOCK = NS * 64, FT = NT * 32;
    // LDS in bf16 elements, hi plane then lo plane of every tile: X^T [FT][row], gY^T [FT][row], per wave H^T and gH^T [32][row];
    // then floats: the bias in accumulator order, and the tile's 32 rows of x and of gy as they lie in memory, row stride RS floats
    // (F or F + 4, the one with an odd number of float4s: 16 lanes' 16-byte reads of one column then cover all 64 banks)
    static constexpr int XT = 0, GYT = XT + 2 * FT * QS, HT = GYT + 2 * FT * QS, GHT = HT + NS * 2 * 32 * QS, END = GHT + NS * 2 * 32 * QS;
    static constexpr int RS = (F / 4) % 2 ? F : F + 4;
    static constexpr int BIAS = END * 2, XS = BIAS + NS * 32 * 4, GS = XS + 32 * RS * 4, BYTES = GS + 32 * RS * 4;
    static constexpr int V4 = 32 * F / 4, NLD = (V4 + BLOCK - 1) / BLOCK;   // float4s of a tile of one input; per thread
    static_assert(F % 4 == 0 && KS * 16 <= FT, "rows are whole float4s; the loaded columns fit the transposed tiles");
    static_assert((F / 2) % 2 == 0 && (RS * 4) % 8 == 0, "a lane's half of a parked row is read in 8-byte vectors");
    static_assert((END * 2) % 16 == 0 && (NS * 32 * 4) % 16 == 0 && (RS * 4) % 16 == 0, "the float tiles are read in 16-byte vectors");
};

// w1t = f32 [F][H], w2t = f32 [H][F]: the fields of tpnet_mlp that k_mlp_rows_x3 reads
template <int L>
__global__ __launch_bounds__(RowsBwdGeo<L>::BLOCK)
void k_mlp_rows_bwd(const float* __restrict__ X, const float* __restrict__ GY, int64_t n, const float* __restrict__ w1t,
                    const float* __restrict__ b1, const float* __restrict__ w2t, float* __restrict__ partial) {
    using G = RowsBwdGeo<L>;
    constexpr int F = G::F, H = G::H, KS = G::KS, NT = G::NT, FT = G::FT, FH = F / 2;
    extern __shared__ __attribute__((aligned(16))) __bf16 lds[];
    __bf16* xt = lds + G::XT;                                             // X^T   [plane][feature][row]
    __bf16* gyt = lds + G::GYT;                                           // gY^T  [plane][output][row]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    __bf16* hrow = lds + G::HT + wave * 2 * 32 * QS;                      // H^T   [plane][hidden of this wave's slice][row]
    __bf16* grow = lds + G::GHT + wave * 2 * 32 * QS;                     // gH^T
    // this wave's rows of W1 as f32 A operands of the f32 matrix instruction (lane (r, h): features FH h + i, i < FH: its two
    // k positions are ANY two features, and this choice makes a lane's B operands consecutive floats of its row), and of W2^T as
    // split A operands (k = outputs), zero beyond H and F
    float a1[FH];
    bf16x8 a2[KS][2];
    {
        const int hid = 32 * wave + r;
#pragma unroll
        for (int i = 0; i < FH; ++i) a1[i] = hid < H ? w1t[(FH * h + i) * H + hid] : 0.0f;
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            float v2[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int k = 16 * s + 8 * h + j;
                v2[j] = hid < H && k < F ? w2t[hid * F + k] : 0.0f;
            }
            split8(v2, a2[s][0], a2[s][1]);
        }
    }
    // the X^T and gY^T tiles start as zeros (PADDING RULES: their rows >= 16 KS stay so)
    for (int i = tid; i < G::HT; i += G::BLOCK) lds[i] = (__bf16)0.0f;
    char* smem = reinterpret_cast<char*>(lds);
    float* xs = reinterpret_cast<float*>(smem + G::XS);                   // x  [row][RS]
    float* gs = reinterpret_cast<float*>(smem + G::GS);                   // gy [row][RS]
    const float4* bias4 = wgrad_stage_bias<H>(reinterpret_cast<float*>(smem + G::BIAS), b1, wave, r, h);
    __syncthreads();
    f32x16 gw1[NT], gw2[NT];                 // gW1[32w + m][32 t + r];  gW2[32 t + m][32w + r]
    float gb1[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        gb1[q] = 0.f;
#pragma unroll
        for (int t2 = 0; t2 < NT; ++t2) { gw1[t2][q] = 0.f; gw2[t2][q] = 0.f; }
    }

    const int64_t ntiles = (n + 31) / 32;
    // a tile's 32 rows are 32 F consecutive floats of x and of gy: the workgroup loads them once, coalesced, float4 i of the tile
    // by thread i (and i + BLOCK ...), a float4 at or beyond n * F floats never (PADDING RULES: rows >= n are zeros), and one tile
    // ahead: the loads of the next tile are in flight during this tile's matrix work
    float4 px[G::NLD], pg[G::NLD];
    auto fetch = [&](int64_t t) {
#pragma unroll
        for (int k = 0; k < G::NLD; ++k) {
            const int i = tid + k * G::BLOCK;
            const int64_t e = t * (32 * F) + 4 * i;
            const bool ok = t < ntiles && i < G::V4 && e < n * F;
            px[k] = ok ? *reinterpret_cast<const float4*>(X + e) : make_float4(0.f, 0.f, 0.f, 0.f);
            pg[k] = ok ? *reinterpret_cast<const float4*>(GY + e) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    fetch(blockIdx.x);
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
#pragma unroll
        for (int k = 0; k < G::NLD; ++k) {
            const int i = tid + k * G::BLOCK;
            if (i < G::V4) {
                const int off = (i / (F / 4)) * G::RS + 4 * (i % (F / 4));
                *reinterpret_cast<float4*>(xs + off) = px[k];
                *reinterpret_cast<float4*>(gs + off) = pg[k];
            }
        }
        __syncthreads();                          // (the previous tile's readers of xs / gs passed the barrier below)
        fetch(tile + gridDim.x);
        const bool valid = tile * 32 + r < n;
        // one operand set at a time (X, then gY): row r -> pieces (lane (r, h) holds elements 16 s + 8 h + j of row r: the B operand
        // of k-step s; a float4 that begins at column >= F is never read), the transposed tile to LDS (wave 0: X^T, wave 1: gY^T;
        // every wave holds the same values), then this wave's hidden slice -- register q = hidden unit acc_row(q, h), column = row r
        uint32_t on_mask = 0;
        auto load_rows = [&](const float* rows, bf16x8 (&b)[KS][2], __bf16* dst, bool store) {
            const float* rowp = rows + r * G::RS;
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                const int c = 16 * s + 8 * h;
                const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
                const float4 va = c < F ? *reinterpret_cast<const float4*>(rowp + c) : z;
                const float4 vb = c + 4 < F ? *reinterpret_cast<const float4*>(rowp + c + 4) : z;
                split8(va, vb, b[s][0], b[s][1]);
            }
            if (store) {
#pragma unroll
                for (int pl = 0; pl < 2; ++pl)
#pragma unroll
                    for (int s = 0; s < KS; ++s)
#pragma unroll
                        for (int j = 0; j < 8; ++j) dst[pl * FT * QS + (16 * s + 8 * h + j) * QS + r] = b[s][pl][j];
            }
        };
        if (wave == 0) {
            bf16x8 bx[KS][2];
            load_rows(xs, bx, xt, true);
        }
        {
            // pre^T in exact f32, the bias first (PRE-ACTIVATIONS): lane (r, h) multiplies features FH h + i of row r
            f32x16 pre;
#pragma unroll
            for (int q4 = 0; q4 < 4; ++q4) {
                const float4 bq = bias4[q4];
                pre[4 * q4] = bq.x; pre[4 * q4 + 1] = bq.y; pre[4 * q4 + 2] = bq.z; pre[4 * q4 + 3] = bq.w;
            }
            const float2* xp = reinterpret_cast<const float2*>(xs + r * G::RS + FH * h);
#pragma unroll
            for (int i2 = 0; i2 < FH / 2; ++i2) {
                const float2 v = xp[i2];
                pre = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[2 * i2], v.x, pre, 0, 0, 0);
                pre = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[2 * i2 + 1], v.y, pre, 0, 0, 0);
            }
            on_mask = wgrad_hidden<2>(pre, valid, hrow, r, h);
        }
        {
            bf16x8 bg[KS][2];
            load_rows(gs, bg, gyt, wave == 1);
            f32x16 gh;
#pragma unroll
            for (int q = 0; q < 16; ++q) gh[q] = 0.f;
#pragma unroll
            for (int s = 0; s < KS; ++s) gh = mm3(a2[s][0], a2[s][1], bg[s][0], bg[s][1], gh);
            wgrad_ghidden<2>(gh, on_mask, gb1, grow, r, h);
        }
        __syncthreads();
        wgrad_contract<2, NT>(xt, gyt, hrow, grow, gw1, gw2, r, h);
        // (no barrier here: the next tile's rows go to xs / gs, which nobody reads after the barrier above, and the transposed
        // tiles are rewritten only behind the next tile's first barrier)
    }
    wgrad_store_partial<F, H, NT>(partial, gw1, gw2, gb1, wave, r, h);
}

template <int L>
static int launch_mlp_rows_bwd_l(const float* x, const float* gy, int64_t n, const tpnet_mlp* mlp, float* partial, int32_t n_partial,
                                 hipStream_t s) {
    using G = RowsBwdGeo<L>;
    static LdsOptIn lds;                               // L = 2: 81 536 bytes of dynamic LDS need the opt-in
    if (!lds.granted({reinterpret_cast<const void*>(k_mlp_rows_bwd<L>)}, G::BYTES)) return TPNET_ERR_BAD_ARG;
    const int grid = wgrad_grid(n, n_partial);
    hipLaunchKernelGGL(k_mlp_rows_bwd<L>, dim3((unsigned)grid), dim3(G::BLOCK), G::BYTES, s, x, gy, n, mlp->w1t, mlp->b1, mlp->w2t,
                       partial);
    TPNET_HIP_TRY(hipGetLastError());
    return grid;
}

}  // namespace tpnet

using namespace tpnet;

extern "C" int64_t tpnet_mlp_rows_bwd_partial_floats(int32_t F, int32_t H) {
    if (!tpnet_mlp_rows_supported(F, H)) return 0;
    return F == RowsBwdGeo<1>::F ? WgradPartial<RowsBwdGeo<1>::F, RowsBwdGeo<1>::H>::TOT : WgradPartial<RowsBwdGeo<2>::F, RowsBwdGeo<2>::H>::TOT;
}

extern "C" int tpnet_mlp_rows_bwd_f32(const float* x, const float* gy, int64_t n, const tpnet_mlp* mlp, float* partial,
                                      int32_t n_partial, void* stream) {
    if (n < 0 || !x || !gy || !mlp || !partial || n_partial < 1) return TPNET_ERR_BAD_ARG;
    if (!tpnet_mlp_rows_supported(mlp->F, mlp->H) || !mlp->w1t || !mlp->b1 || !mlp->w2t) return TPNET_ERR_BAD_ARG;
    if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(gy)) & 15) return TPNET_ERR_BAD_ARG;
    if (reinterpret_cast<uintptr_t>(partial) & 3) return TPNET_ERR_BAD_ARG;
    if (n == 0) return 0;
    return mlp->F == RowsBwdGeo<1>::F ? launch_mlp_rows_bwd_l<1>(x, gy, n, mlp, partial, n_partial, (hipStream_t)stream)
                                      : launch_mlp_rows_bwd_l<2>(x, gy, n, mlp, partial, n_partial, (hipStream_t)stream);
}
