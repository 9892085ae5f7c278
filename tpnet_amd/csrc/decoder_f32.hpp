// LinkPredictor_v1's first layer in the fp32 class for ONE 32-row tile per wave, once: the forward (k_decoder_f32) and the backward's
// row-tile kernel (k_decoder_f32_bwd_rows) in decoder_train.hip both call dec_layer1 and dec_units, so the backward's recomputed
// pre-activations are the forward's instruction sequence on the forward's operands -- the same bits, hence the same ReLU decisions.
//   a = W1 . x + b1,  x = [src_emb (D) | dst_emb (D) | feature (F)] read from its three arrays, never concatenated.
// WHY A BODY OF ITS OWN and not an instantiation of dense2_rows / dense2_bwd_rows: those stream a prepared weight IMAGE through LDS for
// a workgroup of four row tiles and end in a second matrix layer.  The decoder has one output (layer 2 is a dot product over the lane's
// accumulators), its weights change every training step (an image would be a launch per step) and its calls are 7 to 313 row tiles, so a
// tile is a workgroup of ONE wave that splits the fp32 weights as it reads them from L2: no image, no LDS, no barrier, no chunk pipeline.
// What is left is the k-loop below, built from mfma_split.hpp's atoms (split8, mm3) in its tile convention: layer 1 transposed,
// H^T = W1 . X^T, lane (r = lane & 31, h = lane >> 5) = row r of the tile, register q of accumulator t = hidden unit 32 t + acc_row(q, h).
// PADDING.  A row >= n, a hidden unit >= H and a column beyond a source's width contribute a selected 0.0f, never a product with zero:
// the lane reads an element that exists (its index clamped into the array) and the zero is selected behind the load.
// D % 4 == 0 and F % 4 == 0, so a float4 of a row lies inside one source or outside all of them.
#pragma once
#include "mfma_split.hpp"

namespace tpnet {

struct dec_dims {
    int D, F, H, K;                               // K = 2 D + F: the row length of fc1.weight
};
struct dec_src {
    const float *src, *dst, *feat;                // [n][D], [n][D] (both NULL: not_encode, the embeddings count as zeros), [n][F] (NULL: F = 0)
};

static inline bool dec_make_dims(int D, int F, int H, dec_dims& d) {
    if (D < 0 || D > 256 || D % 4 || F < 0 || F > 100 || F % 4 || D + F == 0 || H < 1 || H > 256) return false;
    d.D = D; d.F = F; d.H = H; d.K = 2 * D + F;
    return true;
}

// A masked load in two halves, BRANCH-FREE: dec_raw4 reads 16 bytes that are readable either way (the callers clamp a masked-off lane's
// INDEX to one that exists), dec_sel4 selects zeros behind it.  So all loads of a k-step are issued before the first is waited for.  As
// `on ? *p : 0` the compiler put every load into an exec branch of its own, and a k-step waited for twelve memory round trips in turn
// (profiles/decoder_f32.md)
__device__ __forceinline__ f32x4 dec_raw4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ float4 dec_sel4(const f32x4 v, bool on) {
    return make_float4(on ? v[0] : 0.0f, on ? v[1] : 0.0f, on ? v[2] : 0.0f, on ? v[3] : 0.0f);
}
__device__ __forceinline__ float4 dec_ld4(const float* p, bool on) { return dec_sel4(dec_raw4(p), on); }

// columns c .. c + 3 (c % 4 == 0) of the row's x in fc1.weight's column order; zeros for a row >= n (the caller passes row 0 for it), a
// column >= K, a missing source (those read `safe`: any 16 readable bytes)
__device__ __forceinline__ float4 dec_x4(const dec_src& s, const dec_dims& d, int64_t row, bool valid, int c, const float* safe) {
    const float* p = safe;
    bool on = false;
    if (valid && c < d.K) {
        if (c >= 2 * d.D) { p = s.feat + row * d.F + (c - 2 * d.D); on = true; }
        else if (s.src) { p = c < d.D ? s.src + row * d.D + c : s.dst + row * d.D + (c - d.D); on = true; }
    }
    return dec_ld4(p, on);
}

// acc[t] = rows 32 t .. 32 t + 31 of W1 . X^T for the lane's row tile.  A source of width w at column `off` of W1 takes ceil(w / 16)
// k-steps; the lane's B operand is x[row][16 s + 8 h .. + 7], its A operand W1[32 t + r][off + 16 s + 8 h .. + 7], both split here.
// ONE loop over the k-steps of src, dst and the feature in turn (one body, one schedule); the sources of not_encode have no steps.
template <int HT>
__device__ __forceinline__ void dec_layer1(const dec_src& s, const dec_dims& d, const float* __restrict__ w1, int64_t row, bool valid,
                                           int r, int h, f32x16 (&acc)[HT]) {
#pragma unroll
    for (int t = 0; t < HT; ++t)
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[t][q] = 0.0f;
    const int nD = s.src ? (d.D + 15) / 16 : 0, nF = (d.F + 15) / 16;          // (feat is there exactly where F > 0)
    const float* xs = s.src ? s.src + row * d.D : w1;
    const float* xd = s.src ? s.dst + row * d.D : w1;
    const float* xf = s.feat ? s.feat + row * d.F : w1;
    const float* wrow[HT];                                                      // (a unit of the padding reads unit 0's row)
#pragma unroll
    for (int t = 0; t < HT; ++t) wrow[t] = w1 + (int64_t)(32 * t + r < d.H ? 32 * t + r : 0) * d.K;
    for (int i = 0; i < 2 * nD + nF; ++i) {
        const int seg = i < nD ? 0 : i < 2 * nD ? 1 : 2;                        // (the same for the whole wave)
        const float* x = seg == 0 ? xs : seg == 1 ? xd : xf;
        const int w = seg == 2 ? d.F : d.D, off = seg * d.D;
        const int c = 16 * (i - seg * nD) + 8 * h;
        const bool in0 = c + 4 <= w, in1 = c + 8 <= w;
        const int c0 = in0 ? c : 0, c1 = in1 ? c + 4 : 0;                       // (a float4 beyond the width reads the source's first)
        const f32x4 x0 = dec_raw4(x + c0), x1 = dec_raw4(x + c1);
        f32x4 wa[HT], wb[HT];
#pragma unroll
        for (int t = 0; t < HT; ++t) {
            wa[t] = dec_raw4(wrow[t] + off + c0);
            wb[t] = dec_raw4(wrow[t] + off + c1);
        }
        bf16x8 xh, xl;
        split8(dec_sel4(x0, valid && in0), dec_sel4(x1, valid && in1), xh, xl);
#pragma unroll
        for (int t = 0; t < HT; ++t) {
            const bool real = 32 * t + r < d.H;
            bf16x8 ah, al;
            split8(dec_sel4(wa[t], real && in0), dec_sel4(wb[t], real && in1), ah, al);
            acc[t] = mm3(ah, al, xh, xl, acc[t]);
        }
    }
}

// every hidden unit the lane holds, in register order: acc = f(unit, real, a, w2 of the unit) with a = acc + b1 (the pre-activation)
// and real = unit < H; a unit of the padding has a = 0 and w2 = 0, both selected.  What f returns takes the unit's register (the
// forward's relu(a), the backward's ga: no second array of HT x 16 values)
template <int HT, class FN>
__device__ __forceinline__ void dec_units(const dec_dims& d, const float* __restrict__ b1, const float* __restrict__ w2, int h,
                                          f32x16 (&acc)[HT], FN&& f) {
#pragma unroll
    for (int t = 0; t < HT; ++t) {
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int u = 32 * t + acc_row(q, h);
            const bool real = u < d.H;
            const float a = acc[t][q] + (real ? b1[u] : 0.0f);
            acc[t][q] = f(u, real, a, real ? w2[u] : 0.0f);
        }
    }
}

}  // namespace tpnet
