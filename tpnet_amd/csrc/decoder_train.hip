// LinkPredictor_v1 (models/modules.py:73-117: concat[src_emb, dst_emb, feature] -> fc1 -> ReLU -> fc2 -> one logit) in the project's
// fp32 class, for inference and for a TRAINING step: one launch forward, two backward.  No weight image: the kernels split the fp32
// weights as they read them (decoder_f32.hpp says why), so a step has no prepare launch and no cache to invalidate.
//   k_decoder_f32             a = W1 . x + b1 on the matrix cores (dec_layer1), then logit = sum_u relu(a_u) w2_u + b2 in plain fp32
//                             over the lane's accumulators, the two lane halves added by one __shfl_xor(., 32).  Neither x nor the
//                             hidden layer is written (`hidden`, optional, is a copy of relu(a) for whoever wants it: the tests).
//   the backward from g       ga_u = a_u > 0 ? g w2_u : 0      gb2 = sum g           gw2_u = sum g relu(a_u)      gb1_u = sum ga_u
//   (g = dL/dlogit of a row)  gw1 = sum ga (x) x               gx = W1^T . ga = gsrc | gdst | gfeat               (sums over the rows)
// THE RELU'S DECISIONS ARE RECOMPUTED, not saved: k_decoder_f32_bwd_rows calls the forward's dec_layer1 and dec_units on the forward's
// operands, which is the same instruction sequence per accumulator, so its a has the forward's bits (tests/test_decoder_f32.py compares
// the backward's parked relu(a) with the forward's `hidden` bit for bit on rows built to land within a few ulp of 0).  The backward needs
// a anyway, for gw2; a saved bit per unit would add a store to the forward and spare nothing.
// THE BACKWARD'S TWO LAUNCHES:
//   k_decoder_f32_bwd_rows     a wave = a 32-row tile.  Parks x^T and g, recomputes a, parks relu(a)^T and ga^T (rows_contract.hpp's
//                              layout: [tile][unit or column][row of the tile]), keeps ga in registers as split pieces -- the accumulator
//                              layout IS the B operand of the next product, mfma_split.hpp -- and multiplies W1^T by it in groups of
//                              DEC_CG<HT> column tiles, only over the columns whose gradient is asked for (none: no product at all).
//   k_decoder_f32_bwd_weights  the contraction over rows: a wave owns a 32-unit slice and up to DEC_WT column tiles of gw1 (rc_walk);
//                              gb1 is the sum of the ga operands a wave of the first column group loads; the last workgroup of a row
//                              part adds gw2 and gb2 in plain fp32, thread = unit, rows in order.  Every row part writes ONE partial
//                              (gw1 | gb1 | gw2 | gb2, unpadded); the caller adds the partials in a fixed order.  No atomics: two calls
//                              give equal bits.
// PADDING.  decoder_f32.hpp's rule for the loads; what is parked for a row >= n, a unit >= H or a column >= K is a selected 0.0f (never a
// product with zero), and an accumulator row or column of the padding is never written to a gradient or a partial.
#include "tpnet_common.h"
#include "decoder_f32.hpp"
#include "dense2_bwd.hpp"
#include "rows_contract.hpp"

namespace tpnet {

// column tiles of gx a row-tile wave accumulates at a time: two chains take turns in the matrix pipe; at 8 hidden tiles the split ga
// alone is 128 registers and a second tile of gx would spill
template <int HT> static constexpr int DEC_CG = HT > 7 ? 1 : 2;
static constexpr int DEC_WT = 8;                 // accumulator tiles of a weight wave: 256 columns of gw1

template <int HT>
__global__ __launch_bounds__(64) void k_decoder_f32(const dec_src s, const dec_dims d, int64_t n, const float* __restrict__ w1,
                                                    const float* __restrict__ b1, const float* __restrict__ w2,
                                                    const float* __restrict__ b2, float* __restrict__ out, float* __restrict__ hidden) {
    const int r = threadIdx.x & 31, h = threadIdx.x >> 5;
    const int64_t row = (int64_t)blockIdx.x * 32 + r;
    const bool valid = row < n;
    f32x16 acc[HT];
    dec_layer1<HT>(s, d, w1, valid ? row : 0, valid, r, h, acc);
    float part = 0.0f;
    dec_units<HT>(d, b1, w2, h, acc, [&](int u, bool real, float a, float w) {
        const float v = a > 0.0f ? a : 0.0f;
        part = fmaf(v, w, part);
        if (hidden && valid && real) hidden[row * d.H + u] = v;
        return v;
    });
    part += __shfl_xor(part, 32);
    if (valid && h == 0) out[row] = part + b2[0];
}

// ---- the backward's workspace, tile by tile: hT, gaT [T][HP][32], xT [T][KP][32] (HP = pad32(H), KP = pad32(K)), g [T][32]
struct dec_ws {
    int64_t T;
    int HP, KP;
    float *hT, *gaT, *xT, *g;
};
static int64_t dec_ws_floats(int64_t n, const dec_dims& d) {
    return d2b_tiles(n) * 32 * (2 * (int64_t)d2b_pad32(d.H) + d2b_pad32(d.K) + 1);
}
static dec_ws dec_make_ws(float* base, int64_t n, const dec_dims& d) {
    dec_ws w;
    w.T = d2b_tiles(n);
    w.HP = d2b_pad32(d.H);
    w.KP = d2b_pad32(d.K);
    w.hT = base;
    w.gaT = w.hT + w.T * w.HP * 32;
    w.xT = w.gaT + w.T * w.HP * 32;
    w.g = w.xT + w.T * w.KP * 32;
    return w;
}
static __host__ __device__ inline int64_t dec_partial_floats(const dec_dims& d) { return (int64_t)d.H * d.K + 2 * (int64_t)d.H + 1; }

template <int HT>
__global__ __launch_bounds__(64) void k_decoder_f32_bwd_rows(const dec_src s, const dec_dims d, int64_t n, const float* __restrict__ w1,
                                                             const float* __restrict__ b1, const float* __restrict__ w2,
                                                             const float* __restrict__ gout, const dec_ws ws, float* __restrict__ gsrc,
                                                             float* __restrict__ gdst, float* __restrict__ gfeat) {
    const int r = threadIdx.x & 31, h = threadIdx.x >> 5;
    const int64_t tile = blockIdx.x;
    const int64_t row = tile * 32 + r;
    const bool valid = row < n;
    const int64_t prow = valid ? row : 0;
    // ---- x^T and g of the tile, parked before the accumulators are live: the lane parks the float4s 8 i + 4 h of its row
    float* xT = ws.xT + tile * ws.KP * 32 + r;
    for (int c = 4 * h; c < ws.KP; c += 8) {
        const float4 a = dec_x4(s, d, prow, valid, c, w1);
        xT[c * 32] = a.x; xT[(c + 1) * 32] = a.y; xT[(c + 2) * 32] = a.z; xT[(c + 3) * 32] = a.w;
    }
    const float g = valid ? gout[row] : 0.0f;
    if (h == 0) ws.g[tile * 32 + r] = g;
    // ---- a as the forward computed it; relu(a)^T and ga^T parked, ga kept as the split B operands of gx's k-steps: piece [t][s2] is
    // the units 32 t + acc_row(8 s2 + j, h), j = 0..7
    f32x16 acc[HT];
    dec_layer1<HT>(s, d, w1, prow, valid, r, h, acc);
    float* hT = ws.hT + tile * ws.HP * 32 + r;
    float* gaT = ws.gaT + tile * ws.HP * 32 + r;
    dec_units<HT>(d, b1, w2, h, acc, [&](int u, bool real, float a, float w) {    // (acc becomes ga)
        const bool on = valid && real && a > 0.0f;                              // (torch's rule: no gradient at a == 0)
        const float gav = on ? g * w : 0.0f;
        hT[u * 32] = on ? a : 0.0f;
        gaT[u * 32] = gav;
        return gav;
    });
    // ---- gx^T = W1^T . ga^T over the column tiles that hold a wanted gradient
    const int D = d.D, K = d.K;
    const int c_lo = gsrc ? 0 : gdst ? D : 2 * D;
    const int c_hi = gfeat ? K : gdst ? 2 * D : gsrc ? D : 0;
    if (c_hi <= c_lo) return;
    constexpr int CG = DEC_CG<HT>;
    bf16x8 bh[HT][2], bl[HT][2];
#pragma unroll
    for (int t = 0; t < HT; ++t)
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = acc[t][8 * s2 + j];
            split8(v, bh[t][s2], bl[t][s2]);
        }
#pragma unroll 1
    for (int ct0 = c_lo / 32; 32 * ct0 < c_hi; ct0 += CG) {
        f32x16 y[CG];
#pragma unroll
        for (int tt = 0; tt < CG; ++tt)
#pragma unroll
            for (int q = 0; q < 16; ++q) y[tt][q] = 0.0f;
#pragma unroll
        for (int t = 0; t < HT; ++t) {
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
#pragma unroll
                for (int tt = 0; tt < CG; ++tt) {
                    if (32 * (ct0 + tt) < c_hi) {                               // (the same for the whole wave)
                        // A operand: column c of W1 at the 8 units of piece [t][s2] of this lane half
                        const int c = 32 * (ct0 + tt) + r;
                        float v[8];
#pragma unroll
                        for (int j = 0; j < 8; ++j) {
                            const int u = 32 * t + acc_row(8 * s2 + j, h);
                            const bool on = u < d.H && c < K;                   // (branch-free as dec_ld4: clamped index, selected 0)
                            const float w = w1[(int64_t)(u < d.H ? u : 0) * K + (c < K ? c : 0)];
                            v[j] = on ? w : 0.0f;
                        }
                        bf16x8 ah, al;
                        split8(v, ah, al);
                        y[tt] = mm3(ah, al, bh[t][s2], bl[t][s2], y[tt]);
                    }
                }
            }
        }
        // register q of y[tt] = column 32 (ct0 + tt) + acc_row(q, h) of gx of the lane's row: four registers are one float4 of one array
        if (!valid) continue;
#pragma unroll
        for (int tt = 0; tt < CG; ++tt) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int o = 32 * (ct0 + tt) + 8 * i + 4 * h;
                float* p = nullptr;
                if (o < D) p = gsrc ? gsrc + row * D + o : nullptr;
                else if (o < 2 * D) p = gdst ? gdst + row * D + (o - D) : nullptr;
                else if (o < K) p = gfeat ? gfeat + row * d.F + (o - 2 * D) : nullptr;
                if (p) *reinterpret_cast<float4*>(p) = make_float4(y[tt][4 * i], y[tt][4 * i + 1], y[tt][4 * i + 2], y[tt][4 * i + 3]);
            }
        }
    }
}

// grid (ceil(NS NG / 4) + 1, row parts), NS = hidden slices, NG = column groups of gw1.  tpp: tiles per row part (every part holds one)
__global__ __launch_bounds__(256) void k_decoder_f32_bwd_weights(const dec_ws ws, int64_t n, const dec_dims d, int64_t tpp,
                                                                 float* __restrict__ partial) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int64_t t0 = (int64_t)blockIdx.y * tpp, t1 = t0 + tpp < ws.T ? t0 + tpp : ws.T;
    const int H = d.H, K = d.K;
    float* gw1 = partial + (int64_t)blockIdx.y * dec_partial_floats(d);
    float* gb1 = gw1 + (int64_t)H * K;
    float* gw2 = gb1 + H;
    float* gb2 = gw2 + H;
    if (blockIdx.x == gridDim.x - 1) {
        // ---- the sums over rows that are no matrix product: thread = unit (thread H: gb2), rows in order, rows >= n never added
        for (int u = tid; u <= H; u += 256) {
            float sum = 0.0f;
            for (int64_t t = t0; t < t1; ++t) {
                const int nr = d2b_tile_rows(n, t);
                const float* gg = ws.g + t * 32;
                if (u < H) {
                    const float* hh = ws.hT + (t * ws.HP + u) * 32;
                    for (int i = 0; i < nr; ++i) sum += gg[i] * hh[i];
                } else {
                    for (int i = 0; i < nr; ++i) sum += gg[i];
                }
            }
            if (u < H) gw2[u] = sum;
            else gb2[0] = sum;
        }
        return;
    }
    const int NS = ws.HP / 32, nti = ws.KP / 32, NG = (nti + DEC_WT - 1) / DEC_WT;
    const int item = 4 * blockIdx.x + wave;                                     // (no barrier in this kernel)
    if (item >= NS * NG) return;
    f32x16 acc[DEC_WT];
#pragma unroll
    for (int t = 0; t < DEC_WT; ++t)
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[t][q] = 0.0f;
    // gw1[slice, columns 256 grp ..] = sum_rows ga^T x
    const int slice = item / NG, grp = item % NG;
    const int ct0 = DEC_WT * grp, nt = nti - ct0 < DEC_WT ? nti - ct0 : DEC_WT;
    float asum = rc_walk(ws.gaT, ws.HP, slice, ws.xT, ws.KP, ct0, nt, t0, t1, r, h, acc);
#pragma unroll
    for (int tt = 0; tt < DEC_WT; ++tt) {
        const int c = 32 * (ct0 + tt) + r;
        if (tt < nt && c < K) {
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int j = 32 * slice + acc_row(q, h);
                if (j < H) gw1[(int64_t)j * K + c] = acc[tt][q];
            }
        }
    }
    asum += __shfl_xor(asum, 32);
    if (grp == 0 && h == 0 && 32 * slice + r < H) gb1[32 * slice + r] = asum;
}

// the kernel of HT = ceil(H / 32) hidden tiles on a grid of one wave per row tile
#define DEC_LAUNCH(KERNEL, HT_, tiles, stream, ...)                                                                        \
    do {                                                                                                                   \
        const dim3 grid_((unsigned)(tiles)), block_(64);                                                                   \
        switch (HT_) {                                                                                                     \
            case 1: hipLaunchKernelGGL(KERNEL<1>, grid_, block_, 0, stream, __VA_ARGS__); break;                           \
            case 2: hipLaunchKernelGGL(KERNEL<2>, grid_, block_, 0, stream, __VA_ARGS__); break;                           \
            case 3: hipLaunchKernelGGL(KERNEL<3>, grid_, block_, 0, stream, __VA_ARGS__); break;                           \
            case 4: hipLaunchKernelGGL(KERNEL<4>, grid_, block_, 0, stream, __VA_ARGS__); break;                           \
            case 5: hipLaunchKernelGGL(KERNEL<5>, grid_, block_, 0, stream, __VA_ARGS__); break;                           \
            case 6: hipLaunchKernelGGL(KERNEL<6>, grid_, block_, 0, stream, __VA_ARGS__); break;                           \
            case 7: hipLaunchKernelGGL(KERNEL<7>, grid_, block_, 0, stream, __VA_ARGS__); break;                           \
            default: hipLaunchKernelGGL(KERNEL<8>, grid_, block_, 0, stream, __VA_ARGS__); break;                          \
        }                                                                                                                  \
    } while (0)

// the sources of a call: src and dst come together (both NULL: not_encode), feat exactly where F > 0, and at least one is there
static bool dec_src_ok(const dec_src& s, const dec_dims& d, int64_t n) {
    if (n < 0 || n >= (1ll << 31)) return false;
    if ((s.src == nullptr) != (s.dst == nullptr) || (s.feat != nullptr) != (d.F > 0)) return false;
    if (s.src && d.D == 0) return false;
    return (s.src || s.feat) && aligned16({s.src, s.dst, s.feat});
}
static bool aligned4(std::initializer_list<const void*> ps) {
    uintptr_t a = 0;
    for (const void* p : ps) a |= reinterpret_cast<uintptr_t>(p);
    return (a & 3) == 0;
}

}  // namespace tpnet

using namespace tpnet;

extern "C" int tpnet_decoder_f32_supported(int32_t D, int32_t F, int32_t H) {
    dec_dims d;
    return dec_make_dims(D, F, H, d) ? 1 : 0;
}

extern "C" int64_t tpnet_decoder_f32_partial_floats(int32_t D, int32_t F, int32_t H) {
    dec_dims d;
    return dec_make_dims(D, F, H, d) ? dec_partial_floats(d) : 0;
}

extern "C" size_t tpnet_decoder_f32_bwd_workspace_bytes(int64_t n, int32_t D, int32_t F, int32_t H) {
    dec_dims d;
    if (n < 0 || n >= (1ll << 31) || !dec_make_dims(D, F, H, d)) return 0;
    return (size_t)dec_ws_floats(n, d) * sizeof(float);
}

extern "C" int tpnet_decoder_f32(const float* src_emb, const float* dst_emb, int32_t D, const float* feat, int32_t F, int64_t n,
                                 const float* w1, const float* b1, const float* w2, const float* b2, int32_t H, float* out,
                                 float* hidden, void* stream) {
    dec_dims d;
    const dec_src s{src_emb, dst_emb, feat};
    if (!dec_make_dims(D, F, H, d) || !dec_src_ok(s, d, n) || !w1 || !b1 || !w2 || !b2 || !out) return TPNET_ERR_BAD_ARG;
    if (!aligned16({w1}) || !aligned4({b1, w2, b2, out, hidden})) return TPNET_ERR_BAD_ARG;
    if (n == 0) return TPNET_OK;
    DEC_LAUNCH(k_decoder_f32, (H + 31) / 32, d2b_tiles(n), (hipStream_t)stream, s, d, n, w1, b1, w2, b2, out, hidden);
    TPNET_HIP_TRY(hipGetLastError());
    return TPNET_OK;
}

extern "C" int tpnet_decoder_f32_bwd(const float* src_emb, const float* dst_emb, int32_t D, const float* feat, int32_t F, int64_t n,
                                     const float* w1, const float* b1, const float* w2, int32_t H, const float* gout, void* workspace,
                                     float* gsrc, float* gdst, float* gfeat, float* partial, int32_t n_partial, void* stream) {
    dec_dims d;
    const dec_src s{src_emb, dst_emb, feat};
    if (!dec_make_dims(D, F, H, d) || !dec_src_ok(s, d, n) || !w1 || !b1 || !w2 || !gout || !workspace || !partial || n_partial < 1)
        return TPNET_ERR_BAD_ARG;
    if (((gsrc || gdst) && !src_emb) || (gfeat && !feat)) return TPNET_ERR_BAD_ARG;           // no gradient for a source that is not there
    if (!aligned16({w1, workspace, gsrc, gdst, gfeat}) || !aligned4({b1, w2, gout, partial})) return TPNET_ERR_BAD_ARG;
    if (n == 0) return 0;
    const hipStream_t st = (hipStream_t)stream;
    const dec_ws ws = dec_make_ws(static_cast<float*>(workspace), n, d);
    DEC_LAUNCH(k_decoder_f32_bwd_rows, (H + 31) / 32, ws.T, st, s, d, n, w1, b1, w2, gout, ws, gsrc, gdst, gfeat);
    int64_t tpp;
    const int parts = d2b_row_parts(ws.T, n_partial < 1024 ? n_partial : 1024, tpp);          // (the grid's second axis)
    const int items = (ws.HP / 32) * ((ws.KP / 32 + DEC_WT - 1) / DEC_WT);
    hipLaunchKernelGGL(k_decoder_f32_bwd_weights, dim3((unsigned)((items + 3) / 4 + 1), (unsigned)parts), dim3(256), 0, st, ws, n, d, tpp,
                       partial);
    TPNET_HIP_TRY(hipGetLastError());
    return parts;
}
