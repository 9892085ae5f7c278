// self.mlp = Linear(F, 4F) -> ReLU -> Linear(4F, F) (models/TPNet.py:63-65, 129) on rows of features that already exist, fp32
// class, for LONG lists: the tile walk that k_mlp64_x3 (mlp_x3.hip, F = 64) and k_mlp_rows_x3<L> (mlp_rows.hip, F = 16 and 36)
// share.  Every WAVE owns whole 32-row tiles: layer 1 is computed transposed (H^T = W1 . X^T) so a lane's accumulators are layer
// 2's B operand, the hidden slices are summed inside the output accumulators in slice order, the split weights are staged once per
// workgroup into LDS in exactly the per-lane operand order, and the next tile's rows are loaded under the current tile's matrix
// work.  The arithmetic is mfma_split.hpp's (two-piece bf16 operands, three products per term in the order lo*hi, hi*lo, hi*hi on
// v_mfma_f32_32x32x16_bf16, fp32 accumulators).  A kernel brings its launch bounds, its occupancy attribute and the staging of
// the split weights from its own source layout; the launch rule stays with its host function.
//
// PADDED GEOMETRY (MlpRowsGeo): only F = 64 fills the instruction's 32 x 32 x 16 shape.
//   L  F   H    k-steps of layer 1   hidden slices   output tiles    matrix instructions per tile   LDS image
//   1  16   64  1                    2               1 (half used)    18                             12 672 bytes
//   2  36  144  3 (48 columns)       5 (160 units)   2 (64 outputs)  105                             72 576 bytes
//   3  64  256  4                    8               2               192                            132 352 bytes (IMG_BYTES)
// PADDING RULES.  Columns >= F of the x operand are zero because the LOAD is masked (whole float4s: F % 4 == 0), never because a
// zero weight multiplies them: a row of 36 floats ends 12 floats into k-step 2, and reading on would take the next row's values
// (NaN * 0 = NaN) and, on the last row, memory past the list.  Padded hidden units have zero weights and a zero bias: relu(0) = 0
// adds nothing.  Padded weight columns / rows are zeros in the LDS image.  Padded output columns and rows >= n are never stored;
// stores are whole float4s of the row's F floats.  A width without padding (F % 16 == 0 for the loads, F % 32 == 0 for the
// stores, H % 32 == 0 for the bias) carries none of these masks: they are compile-time.
// A NaN in a row stays in that row (a column of the transposed products), but relu_split16's `x > 0 ? x : 0` maps a NaN hidden unit
// to 0 where torch's ReLU keeps it: the outputs of a row that holds a NaN are not the torch layers'.
#pragma once
#include "mfma_split.hpp"

namespace tpnet {

static constexpr int WT_BLOCK = 512;                  // threads per workgroup: 8 waves, two per SIMD
static constexpr int WT_WAVES = WT_BLOCK / 64;

template <int L>
struct MlpRowsGeo {
    static constexpr int F = (2 * L + 2) * (2 * L + 2), H = 4 * F;
    static constexpr int KS = (F + 15) / 16;          // k-steps of layer 1
    static constexpr int NS = (H + 31) / 32;          // hidden slices of 32 units
    static constexpr int NT = (F + 31) / 32;          // output tiles of 32 columns
    // the slice loop's unroll.  L = 1, 2: a rolled loop -- unrolled, the weight reads of every slice do not depend on the tile and
    // are hoisted out of the tile loop (280 registers at L = 2), and the kernel no longer fits the 128 registers that two
    // workgroups per CU leave a wave.  L = 3: two slices per trip (one workgroup per CU: mlp_x3.hip)
    static constexpr int UNROLL = L == 3 ? 2 : 1;
    // the LDS image: hi / lo planes of W1 (slot (w * KS + s) * 64 + lane) and W2 (slot ((w * 2 + s2) * NT + t) * 64 + lane), every
    // 16-byte slot the A operand of one lane of one matrix instruction; then b1 in accumulator order and b2, both zero-padded
    static constexpr int W1_SLOTS = NS * KS * 64, W2_SLOTS = NS * 2 * NT * 64;
    static constexpr int W1H = 0, W1L = W1H + W1_SLOTS * 16, W2H = W1L + W1_SLOTS * 16, W2L = W2H + W2_SLOTS * 16;
    static constexpr int B1 = W2L + W2_SLOTS * 16, B2 = B1 + NS * 32 * 4, BYTES = B2 + NT * 32 * 4;
    static_assert(F % 4 == 0, "rows are whole float4s");
};

// L = 3 is the image whose offsets mfma_split.hpp names (encoder_mfma.hip's tpnet_mlp::wimg uses them in another element order)
static_assert(MlpRowsGeo<3>::W1H == IMG_W1H && MlpRowsGeo<3>::W1L == IMG_W1L && MlpRowsGeo<3>::W2H == IMG_W2H &&
              MlpRowsGeo<3>::W2L == IMG_W2L && MlpRowsGeo<3>::B1 == IMG_B1 && MlpRowsGeo<3>::B2 == IMG_B2 &&
              MlpRowsGeo<3>::BYTES == IMG_BYTES, "MlpRowsGeo<3> is the IMG_* image");

// The body of a kernel of WT_BLOCK threads: Y[n][F] = self.mlp(X[n][F]).  stage(smem, tid) writes the four weight planes of the
// image (G::W1H ... G::W2L) from the kernel's own source layout; `nact` waves per workgroup take tiles.
template <class G, class Stage>
__device__ __forceinline__ void mlp_wave_tiles(const float* __restrict__ X, int64_t n, const float* __restrict__ b1,
                                               const float* __restrict__ b2, float* __restrict__ Y, int nact, Stage stage) {
    constexpr int F = G::F, H = G::H, KS = G::KS, NS = G::NS, NT = G::NT;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int64_t ntiles = (n + 31) / 32;
    // tiles of the active waves: wave v of workgroup b is wave v * grid + b of the launch (a list's last, partial round of tiles
    // then lands on different CUs, not on the eight waves of a few)
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
            xa[s] = ok && (F % 16 == 0 || c < F) ? *reinterpret_cast<const float4*>(p) : make_float4(0.f, 0.f, 0.f, 0.f);
            xb[s] = ok && (F % 16 == 0 || c + 4 < F) ? *reinterpret_cast<const float4*>(p + 4) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    load_tile(tile);
    stage(smem, tid);
    for (int i = tid; i < NS * 32 + NT * 32; i += WT_BLOCK) {
        if (i < NS * 32) {
            // bias of layer 1 in accumulator order: register q of lane half hh of slice w = hidden unit 32 w + acc_row(q, hh)
            const int w = i >> 5, hh = (i >> 4) & 1, q = i & 15, hid = 32 * w + acc_row(q, hh);
            reinterpret_cast<float*>(smem + G::B1)[i] = (H % 32 == 0 || hid < H) ? b1[hid] : 0.0f;
        } else {
            const int o = i - NS * 32;
            reinterpret_cast<float*>(smem + G::B2)[o] = (F % 32 == 0 || o < F) ? b2[o] : 0.0f;
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
#pragma unroll G::UNROLL
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
        // y[t][4 i .. 4 i + 3] = outputs 32 t + 8 i + 4 h + (0..3) of row r: whole float4s, those that begin below F.
        // (Every tile's b2 of a step is read before the step's first store -- the image holds 32 NT floats of b2, padding included.
        // With one read in front of each store k_mlp64_x3 compiles to another schedule of the SLICE loop -- one layer-1 accumulator
        // for both slices of a trip instead of two, 154 registers instead of 167 -- and 80 000 rows take 25.8 us instead of 24.0.)
        const int64_t row = tile * 32 + r;
        if (row < n) {
            float* yo = Y + row * F;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int o = 8 * i + 4 * h;
                float4 c[NT];
#pragma unroll
                for (int t2 = 0; t2 < NT; ++t2) c[t2] = B2[(32 * t2 + o) >> 2];
#pragma unroll
                for (int t2 = 0; t2 < NT; ++t2) {
                    if (F % 32 == 0 || 32 * t2 + o < F)
                        *reinterpret_cast<float4*>(yo + 32 * t2 + o) = make_float4(y[t2][4 * i] + c[t2].x, y[t2][4 * i + 1] + c[t2].y,
                                                                                   y[t2][4 * i + 2] + c[t2].z, y[t2][4 * i + 3] + c[t2].w);
                }
            }
        }
    }
}

}  // namespace tpnet
