// self.mlp = Linear(64,256) -> ReLU -> Linear(256,64) on ONE LDS tile of 32 feature rows by a workgroup of 8 waves: the dense
// block of the readout kernels that keep the features on the chip (feature_mfma.hip: k_pair_feature_bf16; anchored_feature.hip:
// k_anchored_feature).  Wave w owns hidden tile w (32 of the 256 units): H^T = W1[32w.., :] . X^T by v_mfma_f32_32x32x16_bf16,
// bias + ReLU in registers, and its accumulator tile is directly the B operand of its slice of layer 2 (Y^T += W2[:, 32w..] . H^T).
// The eight partial Y tiles are added in a FIXED order through LDS (run-to-run identical bits).  A row of the tile is one column of
// every matrix product: nothing crosses rows, so rows that hold stale values cost nothing but their cycles.
// X3 = false: bf16 operands (the opt-in 2e-2 class); X3 = true: split operands (mfma_split.hpp), the fp32 class.
// W2LDS (X3 only): layer 2's operands and b1 wait in LDS instead of in registers, for a kernel whose readout leaves no room for
// them (k_anchored_feature: 48 registers less per lane, 8 ds_read_b128 more per tile); same operands, same order, same bits.
#pragma once
#include "mfma_split.hpp"

namespace tpnet {

static constexpr int MB = 512;            // threads per workgroup: 8 waves = the 8 hidden tiles
static constexpr int MF = 64, MH = 256;
static constexpr int TS = 68;             // floats per LDS row of the feature / partial tiles (64 + 4: bank spread)

static constexpr int DENSE_W2_LDS_BYTES = 8 * 2 * 2 * 2 * 64 * 16;      // W2LDS: [wave][s2][t2][hi, lo][lane] 16-byte operands
static constexpr int DENSE_B1_LDS_BYTES = MH * 4;

// a wave's weights: rows [32 wave, 32 wave + 32) of W1 as A operand, the matching columns of (permuted) W2 (32 VGPRs; 64 split)

template <bool X3, bool W2LDS = false>
struct DenseTileW {
    static_assert(X3 || !W2LDS, "DenseTileW: layer 2 in LDS serves the split operands");
    bf16x8 a1[4], a2[W2LDS ? 1 : 2][2];
    bf16x8 a1l[X3 ? 4 : 1], a2l[(X3 && !W2LDS) ? 2 : 1][2];          // X3: the low halves of the split weights
    float bias1[W2LDS ? 1 : 16];
    const bf16x8* w2s;                        // W2LDS: this lane's first operand of layer 2 in LDS, the others 64 elements apart
    const float* b1s;                         // W2LDS: b1 in LDS
    // A operands of layer 2's k-step s2: the two output tiles, high and low pieces
    __device__ __forceinline__ void layer2(int s2, bf16x8 (&ah)[2], bf16x8 (&al)[2]) const {
        if constexpr (W2LDS) {
#pragma unroll
            for (int t2 = 0; t2 < 2; ++t2) {
                ah[t2] = w2s[((s2 * 2 + t2) * 2 + 0) * 64];
                al[t2] = w2s[((s2 * 2 + t2) * 2 + 1) * 64];
            }
        } else {
#pragma unroll
            for (int t2 = 0; t2 < 2; ++t2) {
                ah[t2] = a2[s2][t2];
                al[t2] = a2l[X3 ? s2 : 0][t2];
            }
        }
    }
};

// bf16: w1 = bf16 [256][64], w2p = bf16 [64][256] (hidden axis permuted per 32-tile, fused_mlp.permute_w2)
// split: w1 = f32 [256][64] (mlp[0].weight as is), w2f = f32 [8 waves][2 output tiles][64 lanes][16 k-positions]
template <bool X3>
__device__ __forceinline__ void dense_tile_weights(DenseTileW<X3, false>& w, const void* __restrict__ w1v, const float* __restrict__ b1,
                                                   const void* __restrict__ w2v, int wave, int lane) {
    const __bf16* __restrict__ w1 = reinterpret_cast<const __bf16*>(w1v);
    const __bf16* __restrict__ w2p = reinterpret_cast<const __bf16*>(w2v);
    const float* __restrict__ w1f = reinterpret_cast<const float*>(w1v);
    const float* __restrict__ w2f = reinterpret_cast<const float*>(w2v);
    const int r = lane & 31, h = lane >> 5;
    if constexpr (X3) {
        // the bf16 kernel's operand layout, taken from the f32 sources: A of layer 1 = W1[32 wave + r][16 s + 8 h + j]; A of layer 2
        // = W2[32 t + r][32 wave + acc_row(8 s2 + j, h)] = w2f[..][8 s2 + j] (the gathered f32 layout lists them in order)
#pragma unroll
        for (int s = 0; s < 4; ++s) load_split8(w1f + (wave * 32 + r) * MF + 16 * s + 8 * h, w.a1[s], w.a1l[s]);
#pragma unroll
        for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) load_split8(w2f + (((wave * 2 + t2) * 64 + lane) * 16) + 8 * s2, w.a2[s2][t2], w.a2l[s2][t2]);
    } else {
#pragma unroll
        for (int s = 0; s < 4; ++s) w.a1[s] = *reinterpret_cast<const bf16x8*>(w1 + (wave * 32 + r) * MF + 16 * s + 8 * h);
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
            const int off = wave * 32 + 16 * s2 + 8 * h;          // position inside the PERMUTED hidden axis
            w.a2[s2][0] = *reinterpret_cast<const bf16x8*>(w2p + r * MH + off);
            w.a2[s2][1] = *reinterpret_cast<const bf16x8*>(w2p + (32 + r) * MH + off);
        }
    }
#pragma unroll
    for (int q = 0; q < 16; ++q) w.bias1[q] = b1[wave * 32 + acc_row(q, h)];
}

// ... with layer 2's split operands and b1 parked in LDS (w2s: DENSE_W2_LDS_BYTES, b1s: DENSE_B1_LDS_BYTES; a lane reads back
// only the operands it wrote itself, b1s is shared: a workgroup barrier before the first dense_tile_partials)
__device__ __forceinline__ void dense_tile_weights_lds(DenseTileW<true, true>& w, const float* __restrict__ w1f,
                                                       const float* __restrict__ b1, const float* __restrict__ w2f, int wave, int lane,
                                                       bf16x8* __restrict__ w2s, float* __restrict__ b1s) {
    const int r = lane & 31, h = lane >> 5;
#pragma unroll
    for (int s = 0; s < 4; ++s) load_split8(w1f + (wave * 32 + r) * MF + 16 * s + 8 * h, w.a1[s], w.a1l[s]);
    bf16x8* mine = w2s + wave * (2 * 2 * 2 * 64) + lane;
#pragma unroll
    for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
            bf16x8 hi, lo;
            load_split8(w2f + (((wave * 2 + t2) * 64 + lane) * 16) + 8 * s2, hi, lo);
            mine[((s2 * 2 + t2) * 2 + 0) * 64] = hi;
            mine[((s2 * 2 + t2) * 2 + 1) * 64] = lo;
        }
    if (lane < 32) b1s[wave * 32 + lane] = b1[wave * 32 + lane];
    w.w2s = mine;
    w.b1s = b1s + wave * 32 + 4 * h;
}

// both layers on the tile `feat` ([32][TS], complete and visible to the workgroup): afterwards -- two workgroup barriers inside --
// the four slabs hold the eight waves' partial outputs, pairwise added; dense_tile_out4 finishes them
template <bool X3, bool W2LDS>
__device__ __forceinline__ void dense_tile_partials(const DenseTileW<X3, W2LDS>& w, const float* __restrict__ feat, float (*slab)[32 * TS],
                                                    int wave, int lane) {
    const int r = lane & 31, h = lane >> 5;
    // ---- layer 1, hidden tile `wave`: H^T = W1 . X^T; lane (r, h) holds X[pair r][16 s + 8 h + j] as B operand
    f32x16 acc, y[2];                         // y: the wave's share of the two output tiles
#pragma unroll
    for (int q = 0; q < 16; ++q) { acc[q] = 0.0f; y[0][q] = 0.0f; y[1][q] = 0.0f; }
    if constexpr (X3) {
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            bf16x8 bxh, bxl;
            load_split8(feat + r * TS + 16 * s + 8 * h, bxh, bxl);
            acc = mm3(w.a1[s], w.a1l[s], bxh, bxl, acc);
        }
        bf16x8 bhh[2], bhl[2];
        if constexpr (W2LDS) {
            float bias1[16];
#pragma unroll
            for (int q = 0; q < 16; ++q) bias1[q] = w.b1s[acc_row(q, 0)];
            relu_split16(acc, bias1, bhh, bhl);
        } else
            relu_split16(acc, w.bias1, bhh, bhl);
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
            bf16x8 ah[2], al[2];
            w.layer2(s2, ah, al);
            mm3(ah, al, bhh[s2], bhl[s2], y);                                               // the two output tiles taking turns
        }
    } else {
#pragma unroll
        for (int s = 0; s < 4; ++s) acc = mfma(w.a1[s], load_cvt8(feat + r * TS + 16 * s + 8 * h), acc);
        // register q = hidden row 32 wave + acc_row(q, h), column = pair r  ->  bias, ReLU, B operand of layer 2
        bf16x8 bh[2];
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            float x = acc[q] + w.bias1[q];
            x = x > 0.0f ? x : 0.0f;
            bh[q >> 3][q & 7] = (__bf16)x;
        }
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
            y[0] = mfma(w.a2[s2][0], bh[s2], y[0]);
            y[1] = mfma(w.a2[s2][1], bh[s2], y[1]);
        }
    }
    // ---- the eight partial tiles, added in a fixed order: waves 0..3 park theirs, waves 4..7 add theirs on top, then
    // every thread sums the four slabs for its outputs.  y[0][4i..4i+3] = outputs 8i + 4h + (0..3) of pair r, y[1]: + 32
    float* sl = slab[wave & 3] + r * TS;
    if (wave < 4) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int o = 8 * i + 4 * h;
            *reinterpret_cast<float4*>(sl + o) = make_float4(y[0][4 * i], y[0][4 * i + 1], y[0][4 * i + 2], y[0][4 * i + 3]);
            *reinterpret_cast<float4*>(sl + 32 + o) = make_float4(y[1][4 * i], y[1][4 * i + 1], y[1][4 * i + 2], y[1][4 * i + 3]);
        }
    }
    __syncthreads();
    if (wave >= 4) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int o = 8 * i + 4 * h;
            float4 a = *reinterpret_cast<float4*>(sl + o), b = *reinterpret_cast<float4*>(sl + 32 + o);
            a.x += y[0][4 * i]; a.y += y[0][4 * i + 1]; a.z += y[0][4 * i + 2]; a.w += y[0][4 * i + 3];
            b.x += y[1][4 * i]; b.y += y[1][4 * i + 1]; b.z += y[1][4 * i + 2]; b.w += y[1][4 * i + 3];
            *reinterpret_cast<float4*>(sl + o) = a;
            *reinterpret_cast<float4*>(sl + 32 + o) = b;
        }
    }
    __syncthreads();
}

// outputs [o, o + 4) of the tile's row `pair`: the four slabs in their fixed order, then the bias of layer 2
__device__ __forceinline__ float4 dense_tile_out4(float (*slab)[32 * TS], const float* __restrict__ b2, int pair, int o) {
    const float4 s0 = *reinterpret_cast<const float4*>(slab[0] + pair * TS + o);
    const float4 s1 = *reinterpret_cast<const float4*>(slab[1] + pair * TS + o);
    const float4 s2 = *reinterpret_cast<const float4*>(slab[2] + pair * TS + o);
    const float4 s3 = *reinterpret_cast<const float4*>(slab[3] + pair * TS + o);
    const float4 bb = *reinterpret_cast<const float4*>(b2 + o);
    float4 y;
    y.x = ((s0.x + s1.x) + (s2.x + s3.x)) + bb.x;
    y.y = ((s0.y + s1.y) + (s2.y + s3.y)) + bb.y;
    y.z = ((s0.z + s1.z) + (s2.z + s3.z)) + bb.z;
    y.w = ((s0.w + s1.w) + (s2.w + s3.w)) + bb.w;
    return y;
}

}  // namespace tpnet
