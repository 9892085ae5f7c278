// self.mlp = Linear(F, 4F) -> ReLU -> Linear(4F, F) (models/TPNet.py:63-65, 129) for rp_num_layer L = 1 and L = 2 (F = (2L+2)^2 = 16
// and 36, H = 64 and 144) on rows of features that already exist ([n][F] f32), fp32 class, for LONG lists: what mlp_x3.hip is for
// L = 3.  Same arithmetic (two-piece bf16 operands, three products per term in the order lo*hi, hi*lo, hi*hi on
// v_mfma_f32_32x32x16_bf16, fp32 accumulators: the atoms of mfma_split.hpp) and the same mapping: every WAVE owns whole 32-row
// tiles, layer 1 is computed transposed (H^T = W1 . X^T) so a lane's accumulators are layer 2's B operand, the hidden slices are
// summed inside the output accumulators in slice order, the split weights are staged once per workgroup into LDS in exactly the
// per-lane operand order, and the next tile's rows are loaded under the current tile's matrix work.
//
// PADDED GEOMETRY (MlpRowsGeo): neither width fills the instruction's 32 x 32 x 16 shape.
//   L  F   H    k-steps of layer 1   hidden slices   output tiles    matrix instructions per tile   LDS image
//   1  16   64  1                    2               1 (half used)    18                             12 672 bytes
//   2  36  144  3 (48 columns)       5 (160 units)   2 (64 outputs)  105                             72 576 bytes
// PADDING RULES.  Columns >= F of the x operand are zero because the LOAD is masked (whole float4s: F % 4 == 0), never because a
// zero weight multiplies them: a row of 36 floats ends 12 floats into k-step 2, and reading on would take the next row's values
// (NaN * 0 = NaN) and, on the last row, memory past the list.  Padded hidden units have zero weights and a zero bias: relu(0) = 0
// adds nothing.  Padded weight columns / rows are zeros in the LDS image.  Padded output columns and rows >= n are never stored;
// stores are whole float4s of the row's F floats.
// A NaN in a row stays in that row (a column of the transposed products), but relu_split16's `x > 0 ? x : 0` maps a NaN hidden unit
// to 0 where torch's ReLU keeps it: the outputs of a row that holds a NaN are not the torch layers'.
#include "tpnet_common.h"
#include "mfma_split.hpp"

namespace tpnet {

static constexpr int RB = 512;                        // threads per workgroup: 8 waves, two per SIMD (as mlp_x3.hip)
static constexpr int RW = RB / 64;
static constexpr int R_GRID = 512;                    // workgroups per launch at most: two per CU (two LDS images of L = 2 fit a CU's 160 KB)

template <int L>
struct MlpRowsGeo {
    static constexpr int F = (2 * L + 2) * (2 * L + 2), H = 4 * F;
    static constexpr int KS = (F + 15) / 16;          // k-steps of layer 1
    static constexpr int NS = (H + 31) / 32;          // hidden slices of 32 units
    static constexpr int NT = (F + 31) / 32;          // output tiles of 32 columns
    // the LDS image: hi / lo planes of W1 (slot (w * KS + s) * 64 + lane) and W2 (slot ((w * 2 + s2) * NT + t) * 64 + lane), every
    // 16-byte slot the A operand of one lane of one matrix instruction; then b1 in accumulator order and b2, both zero-padded
    static constexpr int W1_SLOTS = NS * KS * 64, W2_SLOTS = NS * 2 * NT * 64;
    static constexpr int W1H = 0, W1L = W1H + W1_SLOTS * 16, W2H = W1L + W1_SLOTS * 16, W2L = W2H + W2_SLOTS * 16;
    static constexpr int B1 = W2L + W2_SLOTS * 16, B2 = B1 + NS * 32 * 4, BYTES = B2 + NT * 32 * 4;
    static_assert(F % 4 == 0, "rows are whole float4s");
};

// w1t = f32 [F][H] (mlp[0].weight transposed), w2t = f32 [H][F] (mlp[2].weight transposed): tpnet_mlp's fields for every F
template <int L>
__global__ __launch_bounds__(RB) __attribute__((amdgpu_waves_per_eu(4, 4)))      // two workgroups per CU: 128 registers per lane
void k_mlp_rows_x3(const float* __restrict__ X, int64_t n, const float* __restrict__ w1t, const float* __restrict__ b1,
                   const float* __restrict__ w2t, const float* __restrict__ b2, float* __restrict__ Y, int nact) {
    using G = MlpRowsGeo<L>;
    constexpr int F = G::F, H = G::H, KS = G::KS, NS = G::NS, NT = G::NT;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int64_t ntiles = (n + 31) / 32;
    // tiles of the active waves: wave v of workgroup b is wave v * grid + b of the launch (mlp_x3.hip)
    const int64_t aw = (int64_t)gridDim.x * nact;
    int64_t tile = (int64_t)wave * gridDim.x + blockIdx.x;
    const bool active = wave < nact;
    // ---- this wave's first tile ahead of the staging: lane (r, h) holds X[row r][16 s + 8 h + j], the B operand of k-step s;
    // a float4 that begins at column >= F is never read (PADDING RULES)
    float4 xa[KS], xb[KS];
    auto load_tile = [&](int64_t t) {
        const int64_t row = t * 32 + r;
        const bool ok = active && t < ntiles && row < n;
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            const int c = 16 * s + 8 * h;
            const float* p = X + row * F + c;
            xa[s] = ok && c < F ? *reinterpret_cast<const float4*>(p) : make_float4(0.f, 0.f, 0.f, 0.f);
            xb[s] = ok && c + 4 < F ? *reinterpret_cast<const float4*>(p + 4) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    load_tile(tile);
    // ---- the split weights -> LDS, walked in the order of the image (consecutive lanes write consecutive 16-byte slots and read
    // consecutive floats of a row of w1t / w2t); padded k positions, hidden units and outputs are zeros
    for (int i = tid; i < G::W1_SLOTS; i += RB) {                          // W1: slot ((w * KS + s) * 64 + lane (h, r))
        const int ws = i >> 6, w = ws / KS, s = ws - w * KS, hh = (i >> 5) & 1, rr = i & 31;
        const int hid = 32 * w + rr, k0 = 16 * s + 8 * hh;
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = (hid < H && k0 + j < F) ? w1t[(k0 + j) * H + hid] : 0.0f;
        bf16x8 hi, lo;
        split8(v, hi, lo);
        *reinterpret_cast<bf16x8*>(smem + G::W1H + i * 16) = hi;
        *reinterpret_cast<bf16x8*>(smem + G::W1L + i * 16) = lo;
    }
    for (int i = tid; i < G::W2_SLOTS; i += RB) {                          // W2: slot (((w * 2 + s2) * NT + t) * 64 + lane)
        const int g = i >> 6, t2 = g % NT, s2 = (g / NT) & 1, w = g / (2 * NT), hh = (i >> 5) & 1, rr = i & 31;
        const int o = 32 * t2 + rr;
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int hid = 32 * w + acc_row(8 * s2 + j, hh);              // (ACCUMULATOR LAYOUT, mfma_split.hpp)
            v[j] = (hid < H && o < F) ? w2t[hid * F + o] : 0.0f;
        }
        bf16x8 hi, lo;
        split8(v, hi, lo);
        *reinterpret_cast<bf16x8*>(smem + G::W2H + i * 16) = hi;
        *reinterpret_cast<bf16x8*>(smem + G::W2L + i * 16) = lo;
    }
    for (int i = tid; i < NS * 32 + NT * 32; i += RB) {
        if (i < NS * 32) {
            // bias of layer 1 in accumulator order: register q of lane half hh of slice w = hidden unit 32 w + acc_row(q, hh)
            const int w = i >> 5, hh = (i >> 4) & 1, q = i & 15, hid = 32 * w + acc_row(q, hh);
            reinterpret_cast<float*>(smem + G::B1)[i] = hid < H ? b1[hid] : 0.0f;
        } else {
            const int o = i - NS * 32;
            reinterpret_cast<float*>(smem + G::B2)[o] = o < F ? b2[o] : 0.0f;
        }
    }
    __syncthreads();
    if (!active) return;
    const bf16x8* W1H = reinterpret_cast<const bf16x8*>(smem + G::W1H) + lane;
    const bf16x8* W1L = reinterpret_cast<const bf16x8*>(smem + G::W1L) + lane;
    const bf16x8* W2H = reinterpret_cast<const bf16x8*>(smem + G::W2H) + lane;
    const bf16x8* W2L = reinterpret_cast<const bf16x8*>(smem + G::W2L) + lane;
    const float4* B1 = reinterpret_cast<const float4*>(smem + G::B1) + h * 4;
    const float4* B2 = reinterpret_cast<const float4*>(smem + G::B2);
    for (; tile < ntiles; tile += aw) {
        bf16x8 bxh[KS], bxl[KS];
#pragma unroll
        for (int s = 0; s < KS; ++s) split8(xa[s], xb[s], bxh[s], bxl[s]);
        load_tile(tile + aw);                                             // the next tile rides under this one's matrix work
        f32x16 y[NT];                                                     // the output tiles
#pragma unroll
        for (int t2 = 0; t2 < NT; ++t2)
#pragma unroll
            for (int q = 0; q < 16; ++q) y[t2][q] = 0.0f;
        // (a rolled loop: unrolled, the weight reads of every slice do not depend on the tile and are hoisted out of the tile loop
        // -- 280 registers at L = 2 -- and the kernel no longer fits the 128 registers that two workgroups per CU leave a wave)
#pragma unroll 1
        for (int w = 0; w < NS; ++w) {
            // layer 1 of hidden slice w: H^T = W1[32 w .., :] . X^T
            f32x16 acc;
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[q] = 0.0f;
#pragma unroll
            for (int s = 0; s < KS; ++s) acc = mm3(W1H[(w * KS + s) * 64], W1L[(w * KS + s) * 64], bxh[s], bxl[s], acc);
            // bias, ReLU, split -> the B operand of layer 2; then this slice's share of every output tile, the tiles taking turns
            float bv[16];
#pragma unroll
            for (int q4 = 0; q4 < 4; ++q4) {
                const float4 bb = B1[w * 8 + q4];
                bv[4 * q4] = bb.x; bv[4 * q4 + 1] = bb.y; bv[4 * q4 + 2] = bb.z; bv[4 * q4 + 3] = bb.w;
            }
            bf16x8 bhh[2], bhl[2];
            relu_split16(acc, bv, bhh, bhl);
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                bf16x8 ah[NT], al[NT];
#pragma unroll
                for (int t2 = 0; t2 < NT; ++t2) {
                    ah[t2] = W2H[((w * 2 + s2) * NT + t2) * 64];
                    al[t2] = W2L[((w * 2 + s2) * NT + t2) * 64];
                }
                mm3(ah, al, bhh[s2], bhl[s2], y);
            }
        }
        // y[t][4 i .. 4 i + 3] = outputs 32 t + 8 i + 4 h + (0..3) of row r: whole float4s, those that begin below F
        const int64_t row = tile * 32 + r;
        if (row < n) {
            float* yo = Y + row * F;
#pragma unroll
            for (int t2 = 0; t2 < NT; ++t2) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int o = 32 * t2 + 8 * i + 4 * h;
                    if (o < F) {
                        const float4 c = B2[o >> 2];
                        *reinterpret_cast<float4*>(yo + o) = make_float4(y[t2][4 * i] + c.x, y[t2][4 * i + 1] + c.y,
                                                                         y[t2][4 * i + 2] + c.z, y[t2][4 * i + 3] + c.w);
                    }
                }
            }
        }
    }
}

template <int L>
static int launch_mlp_rows_l(const float* x, int64_t n, const tpnet_mlp* mlp, float* y, hipStream_t s) {
    static LdsOptIn lds;                               // L = 2: 72 576 bytes of dynamic LDS need the opt-in
    const void* k = reinterpret_cast<const void*>(k_mlp_rows_x3<L>);
    if (!lds.granted({k}, MlpRowsGeo<L>::BYTES)) return TPNET_ERR_BAD_ARG;
    // grid rule: as many waves per workgroup take tiles as one round over R_GRID workgroups needs (mlp_x3.hip's rule, two
    // workgroups per CU); from R_GRID * RW * 32 = 131 072 rows on, a wave walks more than one tile
    const int64_t tiles = (n + 31) / 32;
    int64_t nact = (tiles + R_GRID - 1) / R_GRID;
    nact = nact > RW ? RW : nact;
    int64_t grid = (tiles + nact - 1) / nact;
    grid = grid > R_GRID ? R_GRID : grid;
    hipLaunchKernelGGL(k_mlp_rows_x3<L>, dim3((unsigned)grid), dim3(RB), MlpRowsGeo<L>::BYTES, s, x, n, mlp->w1t, mlp->b1, mlp->w2t,
                       mlp->b2, y, (int)nact);
    if (hipGetLastError() != hipSuccess) {             // (a runtime that refuses the launch: the callers fall back for good)
        lds.refused();
        return TPNET_ERR_BAD_ARG;
    }
    return TPNET_OK;
}

}  // namespace tpnet

using namespace tpnet;

extern "C" int tpnet_mlp_rows_supported(int32_t F, int32_t H) {
    return (F == MlpRowsGeo<1>::F && H == MlpRowsGeo<1>::H) || (F == MlpRowsGeo<2>::F && H == MlpRowsGeo<2>::H);
}

extern "C" int tpnet_mlp_rows_f32(const float* x, int64_t n, const tpnet_mlp* mlp, float* y, void* stream) {
    if (n < 0 || !mlp || (n > 0 && (!x || !y))) return TPNET_ERR_BAD_ARG;
    if (n == 0) return TPNET_OK;
    if (!tpnet_mlp_rows_supported(mlp->F, mlp->H) || !mlp->w1t || !mlp->b1 || !mlp->w2t || !mlp->b2) return TPNET_ERR_BAD_ARG;
    if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 15) return TPNET_ERR_BAD_ARG;
    return mlp->F == MlpRowsGeo<1>::F ? launch_mlp_rows_l<1>(x, n, mlp, y, (hipStream_t)stream)
                                      : launch_mlp_rows_l<2>(x, n, mlp, y, (hipStream_t)stream);
}
