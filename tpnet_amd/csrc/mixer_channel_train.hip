// The channel-mixing half of an MLP-Mixer layer (models/TPNet.py:341-416) in a TRAINING step on the matrix cores: one launch forward,
// two backward.  Per row v[0 .. C) of x [n_rows][C], with s = 1 / (1 - p) and the keep masks m1 [Ch], m2 [C] of the two dropouts of
// FeedForwardNet (behind the GELU, behind the second Linear):
//   xh = ((v - m0) - dl) rstd          ln = xh gamma + beta                      (the LayerNorm rule of mixer.hip)
//   a  = W1 . ln + b1                  h  = gelu(a) m1 s
//   out = (W2 . h + b2) m2 s + v
//   k_mixer_channel_train  the forward: k_mixer_channel (dense2.hpp's two layers, the LayerNorm of the lane's row as the row source)
//                          with m1 in the activation and m2 in the epilogue -- at p = 0 nothing is drawn and the output has the
//                          bits of k_mixer_channel's.
//   the backward from gy   go = gy m2 s        gb2 = sum go          gw2 = sum go (x) h
//                          gh = W2^T . go      ga = gh m1 s gelu'(a) gb1 = sum ga       gw1 = sum ga (x) ln
//                          gln = W1^T . ga     ggamma = sum gln xh   gbeta = sum gln
//                          gt = gln gamma      gx = gy + rstd (gt - mean_c(gt) - xh mean_c(gt xh))        (every sum over the rows)
//                          Nothing but x is saved by the caller: everything is recomputed from x and the key.
// THE BACKWARD'S TWO LAUNCHES are dense2_bwd.hpp's (the transposed workspace of the call -- tpnet_mixer_channel_bwd_workspace_bytes;
// the caller allocates it for the call and frees it behind it -- the image of W1, W2^T and W1^T, the row-tile body, the padding rules):
//   k_mxc_bwd_rows     dense2_bwd_rows with ln and go = gy m2 s as the two row sources and the rule h = gelu(a) m1 s,
//                      ga = gh m1 s gelu'(a); y is gln.  The epilogue parks gln and does the LayerNorm backward on the lane pair's row
//                      (two row sums finished with __shfl_xor(., 32)).  Also parks ln, xh and go.  gx may be NULL.
//   k_mxc_bwd_weights  the contraction over rows.  A wave owns a 32-unit hidden slice j of ONE of the two products --
//                      gw1[j, :] = sum_rows ga^T ln, or gw2[:, j]^T = sum_rows h^T go -- as up to 8 accumulator tiles, and a
//                      workgroup (4 waves: two slices x two products) one part of the row tiles; gb1 is the sum of the ga operands
//                      the wave loads.  The last workgroup of a row part adds ggamma, gbeta and gb2 in plain fp32, thread = column,
//                      rows in order.  Every row part writes ONE partial (ggamma | gbeta | gw1 | gb1 | gw2 | gb2, unpadded); the
//                      caller adds the partials in a fixed order.  No atomics: two calls give equal bits.
// The weight kernel contracts parked operands; it does not recompute a and gh per hidden slice.  The workspace is
// 128 (ceil(Ch / 32) 2 + ceil(C / 32) 4) bytes per row for the time of the backward (profiles/mixer_channel_training.md).
// ARITHMETIC.  All products are the fp32 class of mfma_split.hpp (two bf16 pieces per operand, mm3's three products, fp32
// accumulators); the LayerNorm statistics, gelu, gelu', the masks and the LayerNorm backward are plain fp32.  GELU is smooth: an
// error of 2^-16 in a pre-activation moves h and gelu'(a) by as little, so a is recomputed on split operands like the forward's.
// The exact-f32 pre-activation pass that mlp_rows_bwd.hip needs to take the ReLU's decisions as the forward took them is not needed.
// DRAWS.  mixer_channel.hpp's mxc_keep4: a draw depends on (key, row, slot) alone, so the forward, the backward and the mask kernel
// agree whatever their launch geometry.
// PADDING.  dense2_bwd.hpp's rules: x4 / g4 return zeros for a row >= n, what is parked for it (ln, xh and go too) is a selected
// 0.0f, and gln and go of such a row are never read by the column sums.
#include "mixer_channel.hpp"
#include "dense2_bwd.hpp"
#include "rows_contract.hpp"

namespace tpnet {

// ---- the activations (dense2.hpp: split16 of slice w; register q of lane half h = hidden unit 32 w + acc_row(q, h) = 4 consecutive
// units per q >> 2 = ONE block 8 w + 2 (q >> 2) + h of draws)
struct mxc_drop {
    int64_t row;
    int h;
    float s;
    uint32_t thr, k0, k1;
    __device__ __forceinline__ float scale(uint32_t keep, int j) const { return ((keep >> j) & 1u) ? s : 0.0f; }
};

// the forward's: gelu, then m1 s
struct act_gelu_drop : mxc_drop {
    __device__ __forceinline__ void split16(const f32x16& a, const float (&bias)[16], int w, bf16x8 (&bh)[2], bf16x8 (&bl)[2]) const {
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
            float x[8];
#pragma unroll
            for (int q4 = 2 * s2; q4 < 2 * s2 + 2; ++q4) {
                const uint32_t keep = mxc_keep4(row, (uint32_t)(8 * w + 2 * q4 + h), thr, k0, k1);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float g = gelu_erf(a[4 * q4 + j] + bias[4 * q4 + j]);
                    x[4 * (q4 - 2 * s2) + j] = thr ? g * scale(keep, j) : g;
                }
            }
            split8(x, bh[s2], bl[s2]);
        }
    }
};

// HG hidden slices per pass, OSM output tiles, MULTI: dense2_rows'.  thr = floor(p 2^32): 0 = no dropout; s = 1 / (1 - p)
template <int HG, int OSM, bool MULTI>
__global__ __launch_bounds__(D2_T) void k_mixer_channel_train(const float* __restrict__ x, int64_t n, const float* __restrict__ gamma,
                                                              const float* __restrict__ beta, float eps, const d2_dims d,
                                                              const uint4* __restrict__ img, float s, uint32_t thr, uint32_t k0,
                                                              uint32_t k1, float* __restrict__ out) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int64_t row = ((int64_t)blockIdx.x * 4 + wave) * 32 + r;
    const bool valid = row < n;
    const int C = d.Din;
    const float* xr = x + (valid ? row : 0) * C;
    mx_ln_row x4{xr, gamma, beta, C, valid};
    x4.stats(h, eps);
    act_gelu_drop act;
    act.row = row; act.h = h; act.s = s; act.thr = thr; act.k0 = k0; act.k1 = k1;
    const uint32_t b2 = (uint32_t)((d.H + 3) / 4);                              // m2's first block
    float* yo = out + row * C;
    dense2_rows<HG, OSM, MULTI, act_gelu_drop>(d, img, valid, x4, [&](int o, const float4 v) {
        const float4 a = *reinterpret_cast<const float4*>(xr + o);
        if (thr) {
            const uint32_t keep = mxc_keep4(row, b2 + (uint32_t)(o >> 2), thr, k0, k1);
            *reinterpret_cast<float4*>(yo + o) = make_float4(v.x * act.scale(keep, 0) + a.x, v.y * act.scale(keep, 1) + a.y,
                                                             v.z * act.scale(keep, 2) + a.z, v.w * act.scale(keep, 3) + a.w);
        } else {
            *reinterpret_cast<float4*>(yo + o) = make_float4(v.x + a.x, v.y + a.y, v.z + a.z, v.w + a.w);
        }
    }, act);
}

// one thread per (row, block of four draws)
__global__ __launch_bounds__(256) void k_mixer_channel_masks(int64_t n, int C, int Ch, uint32_t thr, uint32_t k0, uint32_t k1,
                                                             uint8_t* __restrict__ m1, uint8_t* __restrict__ m2) {
    const int nb1 = (Ch + 3) / 4, nb = nb1 + C / 4;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n * nb) return;
    const int64_t row = i / nb;
    const int b = (int)(i - row * nb);
    const uint32_t keep = mxc_keep4(row, (uint32_t)b, thr, k0, k1);
    for (int j = 0; j < 4; ++j) {
        if (b < nb1) {
            if (4 * b + j < Ch) m1[row * Ch + 4 * b + j] = (uint8_t)((keep >> j) & 1u);
        } else {
            m2[row * C + 4 * (b - nb1) + j] = (uint8_t)((keep >> j) & 1u);
        }
    }
}

// ---- the backward's workspace: dense2_bwd.hpp's head (hT, gaT) and four transposed column arrays, tile by tile
struct mxc_ws : d2b_ws {
    int CS;                                      // parked columns per tile (a multiple of 32)
    float *lnT, *xhT, *goT, *glnT;               // [T][CS][32]
};

static __host__ __device__ inline int64_t mxc_ws_floats(int64_t n, int C, int Ch) {
    return d2b_tiles(n) * 32 * (2 * (int64_t)d2b_pad32(Ch) + 4 * (int64_t)d2b_pad32(C));
}

static mxc_ws mxc_make_ws(float* base, int64_t n, int C, int Ch) {
    mxc_ws w;
    w.lnT = d2b_make_ws(w, base, n, Ch);
    w.CS = d2b_pad32(C);
    const int64_t col = w.T * w.CS * 32;
    w.xhT = w.lnT + col;
    w.goT = w.xhT + col;
    w.glnT = w.goT + col;
    return w;
}

// the backward's sizes: dense2_bwd.hpp's with Din = Dout = C and every column of W1^T, in place
static void mxc_bwd_dims(int C, int Ch, d2b_dims& o) { d2b_make_dims(C, Ch, C, C, 0, 0, 0, o); }

// ---- the backward's rule (dense2_bwd.hpp): h = gelu(a) m1 s and ga = gh m1 s gelu'(a).  The four units of a block are ONE block of
// draws (the activations' comment above)
struct rule_gelu_drop : mxc_drop {
    __device__ __forceinline__ uint32_t block(int slice, int q4) const {
        return mxc_keep4(row, (uint32_t)(8 * slice + 2 * q4 + h), thr, k0, k1);
    }
    __device__ __forceinline__ void unit(uint32_t keep, int j, bool real, float a, float gh, float& hv, float& gav) const {
        const float ms = thr ? scale(keep, j) : 1.0f;
        const float g = gelu_erf(a), gd = gelu_erf_grad(a);
        hv = real ? (thr ? g * ms : g) : 0.0f;
        gav = real ? gh * (ms * gd) : 0.0f;
    }
};

// ---- the backward's row-tile kernel: dense2_bwd_rows on ln (the LayerNorm of the lane's row) and go = gy m2 s, the LayerNorm
// backward behind it
template <int OSM>
__global__ __launch_bounds__(D2_T) void k_mxc_bwd_rows(const float* __restrict__ x, const float* __restrict__ gy, int64_t n,
                                                       const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                       const d2b_dims d, const uint4* __restrict__ img, float s, uint32_t thr,
                                                       uint32_t k0, uint32_t k1, const mxc_ws ws, float* __restrict__ gx) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int64_t tile = (int64_t)blockIdx.x * 4 + wave;
    const int64_t row = tile * 32 + r;
    const bool valid = row < n, park = tile < ws.T;
    const int C = d.Din;
    const float* xr = x + (valid ? row : 0) * C;
    const float* gr = gy + (valid ? row : 0) * C;
    mx_ln_row x4{xr, gamma, beta, C, valid};
    x4.stats(h, eps);
    rule_gelu_drop drop;
    drop.row = row; drop.h = h; drop.s = s; drop.thr = thr; drop.k0 = k0; drop.k1 = k1;
    const uint32_t b2 = (uint32_t)((d.H + 3) / 4);                              // m2's first block
    // columns c .. c + 3 of go = gy m2 s
    auto g4 = [&](int c) -> float4 {
        if (!valid || c >= C) return make_float4(0.f, 0.f, 0.f, 0.f);
        const float4 a = *reinterpret_cast<const float4*>(gr + c);
        if (!thr) return a;
        const uint32_t keep = mxc_keep4(row, b2 + (uint32_t)(c >> 2), thr, k0, k1);
        return make_float4(a.x * drop.scale(keep, 0), a.y * drop.scale(keep, 1), a.z * drop.scale(keep, 2), a.w * drop.scale(keep, 3));
    };
    float* glnT = ws.glnT + (park ? tile : 0) * ws.CS * 32 + r;
    // ---- ln, xh and go of the tile, parked for k_mxc_bwd_weights (a selected 0.0f for a row or a column of the padding)
    if (park) {
        float* lnT = ws.lnT + tile * ws.CS * 32 + r;
        float* xhT = ws.xhT + tile * ws.CS * 32 + r;
        float* goT = ws.goT + tile * ws.CS * 32 + r;
        for (int c = 4 * h; c < ws.CS; c += 8) {
            float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
            const bool real = valid && c < C;
            if (real) a = *reinterpret_cast<const float4*>(xr + c);
            const float4 ln = x4(c), g = g4(c);
            const float xv[4] = {a.x, a.y, a.z, a.w}, lv[4] = {ln.x, ln.y, ln.z, ln.w}, gv[4] = {g.x, g.y, g.z, g.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                lnT[(c + k) * 32] = lv[k];
                xhT[(c + k) * 32] = real ? x4.xh(xv[k]) : 0.0f;
                goT[(c + k) * 32] = gv[k];
            }
        }
    }
    dense2_bwd_rows<OSM, false>(d, img, ws, valid, x4, g4, drop, [&](const f32x16 (&y)[OSM]) {
        // ---- the LayerNorm backward on the lane pair's row: y = gln
        float s1 = 0.0f, s2 = 0.0f;                                             // the row sums of gt = gln gamma and of gt xh
        if (valid) {
#pragma unroll
            for (int t = 0; t < OSM; ++t) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int o = 32 * t + 8 * i + 4 * h;
                    if (o < C) {
                        const float4 a = *reinterpret_cast<const float4*>(xr + o), g = *reinterpret_cast<const float4*>(gamma + o);
                        const float xv[4] = {a.x, a.y, a.z, a.w}, gm[4] = {g.x, g.y, g.z, g.w};
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            glnT[(o + k) * 32] = y[t][4 * i + k];
                            const float gt = y[t][4 * i + k] * gm[k];
                            s1 += gt;
                            s2 += gt * x4.xh(xv[k]);
                        }
                    }
                }
            }
        }
        s1 += __shfl_xor(s1, 32);
        s2 += __shfl_xor(s2, 32);
        if (!valid || !gx) return;
        s1 /= (float)C;
        s2 /= (float)C;
        float* go = gx + row * C;
#pragma unroll
        for (int t = 0; t < OSM; ++t) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int o = 32 * t + 8 * i + 4 * h;
                if (o < C) {
                    const float4 a = *reinterpret_cast<const float4*>(xr + o), g = *reinterpret_cast<const float4*>(gamma + o),
                                 yy = *reinterpret_cast<const float4*>(gr + o);
                    const float xv[4] = {a.x, a.y, a.z, a.w}, gm[4] = {g.x, g.y, g.z, g.w}, yv[4] = {yy.x, yy.y, yy.z, yy.w};
                    float o4[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) o4[k] = x4.rstd * ((y[t][4 * i + k] * gm[k] - s1) - x4.xh(xv[k]) * s2) + yv[k];
                    *reinterpret_cast<float4*>(go + o) = make_float4(o4[0], o4[1], o4[2], o4[3]);
                }
            }
        }
    });
}

static constexpr int MXC_WT = 8;                 // accumulator tiles of a weight wave: C <= 256

// grid (ceil(NS / 2) + 1, row parts).  tpp: tiles per row part (every part holds one)
__global__ __launch_bounds__(256) void k_mxc_bwd_weights(const mxc_ws ws, int64_t n, int C, int Ch, int64_t tpp,
                                                         float* __restrict__ partial) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int64_t t0 = (int64_t)blockIdx.y * tpp, t1 = t0 + tpp < ws.T ? t0 + tpp : ws.T;
    const int64_t P = 2 * (int64_t)C + 2 * (int64_t)C * Ch + Ch + C;
    float* out = partial + (int64_t)blockIdx.y * P;
    float* gw1 = out + 2 * C;
    float* gb1 = gw1 + (int64_t)Ch * C;
    float* gw2 = gb1 + Ch;
    float* gb2 = gw2 + (int64_t)C * Ch;
    if (blockIdx.x == gridDim.x - 1) {
        // ---- the three sums over rows that are no matrix product: thread = column, rows in order, rows >= n never added
        if (tid >= C) return;
        float sg = 0.0f, sb = 0.0f, so = 0.0f;
        for (int64_t t = t0; t < t1; ++t) {
            const int nr = d2b_tile_rows(n, t);
            const float4* gl = reinterpret_cast<const float4*>(ws.glnT + (t * ws.CS + tid) * 32);
            const float4* xh = reinterpret_cast<const float4*>(ws.xhT + (t * ws.CS + tid) * 32);
            const float4* go = reinterpret_cast<const float4*>(ws.goT + (t * ws.CS + tid) * 32);
            for (int i = 0; 4 * i < nr; ++i) {                  // (a column's 32 rows are 128 consecutive bytes: whole lines per thread)
                const float4 a = gl[i], b = xh[i], c = go[i];
                const float av[4] = {a.x, a.y, a.z, a.w}, bv[4] = {b.x, b.y, b.z, b.w}, cv[4] = {c.x, c.y, c.z, c.w};
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if (4 * i + k < nr) {
                        sg += av[k] * bv[k];
                        sb += av[k];
                        so += cv[k];
                    }
                }
            }
        }
        out[tid] = sg;
        out[C + tid] = sb;
        gb2[tid] = so;
        return;
    }
    const int slice = 2 * blockIdx.x + (wave & 1), which = wave >> 1;           // which: 0 = gw1 (ga, ln), 1 = gw2 (h, go)
    if (slice >= ws.NS) return;                                                 // (no barrier in this kernel)
    const float* A = which ? ws.hT : ws.gaT;
    const float* B = which ? ws.goT : ws.lnT;
    const int nt = ws.CS / 32;
    f32x16 acc[MXC_WT];
#pragma unroll
    for (int t = 0; t < MXC_WT; ++t)
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[t][q] = 0.0f;
    // (rows_contract.hpp) acc[t][q] = sum over rows of A[unit 32 slice + acc_row(q, h)] B[column 32 t + r]
    float asum = rc_walk(A, ws.CHS, slice, B, ws.CS, 0, nt, t0, t1, r, h, acc);
#pragma unroll
    for (int tt = 0; tt < MXC_WT; ++tt) {
        const int c = 32 * tt + r;
        if (tt < nt && c < C) {
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int j = 32 * slice + acc_row(q, h);
                if (j < Ch) {
                    if (which) gw2[(int64_t)c * Ch + j] = acc[tt][q];
                    else gw1[(int64_t)j * C + c] = acc[tt][q];
                }
            }
        }
    }
    asum += __shfl_xor(asum, 32);
    if (which == 0 && h == 0 && 32 * slice + r < Ch) gb1[32 * slice + r] = asum;
}

static bool mxc_served(int64_t n_rows, int32_t C, int32_t Ch, d2_dims& d) {
    return n_rows >= 0 && n_rows <= (1ll << 31) && mx_channel_dims(C, Ch, d);
}

}  // namespace tpnet

using namespace tpnet;

// the variant of d: k_mixer_channel's choice
#define MXC_LAUNCH(KERNEL, d, grid, stream, ...)                                                                              \
    do {                                                                                                                       \
        if ((d).HG == D2_HG)                                                                                                   \
            hipLaunchKernelGGL((KERNEL<D2_HG, D2_OS, false>), grid, dim3(D2_T), 0, stream, __VA_ARGS__);                       \
        else if ((d).OS == D2_OS)                                                                                              \
            hipLaunchKernelGGL((KERNEL<D2_HG_WIDE, D2_OS, true>), grid, dim3(D2_T), 0, stream, __VA_ARGS__);                   \
        else                                                                                                                   \
            hipLaunchKernelGGL((KERNEL<D2_HG_WIDE, D2_OS_WIDE, true>), grid, dim3(D2_T), 0, stream, __VA_ARGS__);              \
    } while (0)

extern "C" int tpnet_mixer_channel_train(const float* x, int64_t n_rows, int32_t C, int32_t Ch, const float* gamma, const float* beta,
                                         float eps, const void* img, float p, uint64_t key, float* out, void* stream) {
    d2_dims d;
    if (!x || !gamma || !beta || !img || !out || out == x) return TPNET_ERR_BAD_ARG;
    if (!mxc_served(n_rows, C, Ch, d) || !drop_rate(p)) return TPNET_ERR_BAD_ARG;
    if (!aligned16({x, gamma, beta, img, out})) return TPNET_ERR_BAD_ARG;
    if (n_rows == 0) return TPNET_OK;
    const dim3 grid((unsigned)((n_rows + D2_ROWS - 1) / D2_ROWS));
    MXC_LAUNCH(k_mixer_channel_train, d, grid, (hipStream_t)stream, x, n_rows, gamma, beta, eps, d, reinterpret_cast<const uint4*>(img),
               1.0f / (1.0f - p), drop_threshold(p), (uint32_t)key, (uint32_t)(key >> 32), out);
    TPNET_HIP_TRY(hipGetLastError());
    return TPNET_OK;
}

extern "C" int64_t tpnet_mixer_channel_bwd_partial_floats(int32_t C, int32_t Ch) {
    d2_dims d;
    return mx_channel_dims(C, Ch, d) ? 2 * (int64_t)C + 2 * (int64_t)C * Ch + Ch + C : 0;
}

extern "C" size_t tpnet_mixer_channel_bwd_image_bytes(int32_t C, int32_t Ch) {
    d2_dims d;
    d2b_dims b;
    if (!mx_channel_dims(C, Ch, d)) return 0;
    mxc_bwd_dims(C, Ch, b);
    return d2b_image_bytes(b);
}

extern "C" int tpnet_mixer_channel_bwd_prepare(const float* w1, const float* b1, const float* w2, int32_t C, int32_t Ch, void* bimg,
                                               void* stream) {
    d2_dims d;
    d2b_dims b;
    if (!w1 || !b1 || !w2 || !bimg || (reinterpret_cast<uintptr_t>(bimg) & 15) || !mx_channel_dims(C, Ch, d)) return TPNET_ERR_BAD_ARG;
    mxc_bwd_dims(C, Ch, b);
    TPNET_HIP_TRY(d2b_prepare(w1, b1, w2, b, bimg, (hipStream_t)stream));
    return TPNET_OK;
}

extern "C" size_t tpnet_mixer_channel_bwd_workspace_bytes(int64_t n_rows, int32_t C, int32_t Ch) {
    d2_dims d;
    return mxc_served(n_rows, C, Ch, d) ? (size_t)mxc_ws_floats(n_rows, C, Ch) * sizeof(float) : 0;
}

extern "C" int tpnet_mixer_channel_bwd(const float* x, const float* gy, int64_t n_rows, int32_t C, int32_t Ch, const float* gamma,
                                       const float* beta, float eps, const void* bimg, float p, uint64_t key, void* workspace, float* gx,
                                       float* partial, int32_t n_partial, void* stream) {
    d2_dims d;
    if (!x || !gy || !gamma || !beta || !bimg || !workspace || !partial || gx == x || gx == gy) return TPNET_ERR_BAD_ARG;
    if (!mxc_served(n_rows, C, Ch, d) || !drop_rate(p) || n_partial < 1) return TPNET_ERR_BAD_ARG;
    if (!aligned16({x, gy, gx, gamma, beta, bimg, workspace}) || (reinterpret_cast<uintptr_t>(partial) & 3)) return TPNET_ERR_BAD_ARG;
    if (n_rows == 0) return 0;
    const hipStream_t st = (hipStream_t)stream;
    const mxc_ws ws = mxc_make_ws(static_cast<float*>(workspace), n_rows, C, Ch);
    d2b_dims b;
    mxc_bwd_dims(C, Ch, b);
    D2B_LAUNCH_ROWS(k_mxc_bwd_rows, b, n_rows, st, x, gy, n_rows, gamma, beta, eps, b, reinterpret_cast<const uint4*>(bimg),
                    1.0f / (1.0f - p), drop_threshold(p), (uint32_t)key, (uint32_t)(key >> 32), ws, gx);
    int64_t tpp;
    const int parts = d2b_row_parts(ws.T, n_partial, tpp);
    hipLaunchKernelGGL(k_mxc_bwd_weights, dim3((unsigned)((ws.NS + 1) / 2 + 1), (unsigned)parts), dim3(256), 0, st, ws, n_rows, (int)C,
                       (int)Ch, tpp, partial);
    TPNET_HIP_TRY(hipGetLastError());
    return parts;
}

extern "C" int tpnet_mixer_channel_masks(int64_t n_rows, int32_t C, int32_t Ch, float p, uint64_t key, uint8_t* m1, uint8_t* m2,
                                         void* stream) {
    d2_dims d;
    if (!m1 || !m2 || !mxc_served(n_rows, C, Ch, d) || !drop_rate(p)) return TPNET_ERR_BAD_ARG;
    if (n_rows == 0) return TPNET_OK;
    const int64_t total = n_rows * ((Ch + 3) / 4 + C / 4);
    if (total > 0xffffff00ll) return TPNET_ERR_BAD_ARG;                         // (one thread per block of draws; a launch has < 2^32)
    hipLaunchKernelGGL(k_mixer_channel_masks, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n_rows, (int)C,
                       (int)Ch, drop_threshold(p), (uint32_t)key, (uint32_t)(key >> 32), m1, m2);
    TPNET_HIP_TRY(hipGetLastError());
    return TPNET_OK;
}
