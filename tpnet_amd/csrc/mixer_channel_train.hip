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
// THE BACKWARD'S TWO LAUNCHES share a workspace of the call (tpnet_mixer_channel_bwd_workspace_bytes; the caller allocates it for
// the call and frees it behind it), cut into tiles of 32 rows and held TRANSPOSED -- element [tile][unit or column][row of the
// tile] -- so that a lane of the row-tile kernel (lane = row) stores 32 consecutive floats per wave store, and a lane of the
// contraction over rows loads its 8 consecutive rows of one unit as two float4, already in operand order:
//   k_mxc_bwd_rows     row-tile parallel like the forward, on an image of its own (W1, W2^T, W1^T; k_mxc_bwd_image).  Per pass of 4
//                      hidden slices it holds TWO layer-1 accumulators per slice, a = W1 . ln + b1 and gh = W2^T . go (go = gy m2 s
//                      is the second row source), forms h and ga = gh m1 s gelu'(a) in registers, parks both, and feeds ga as the B
//                      operand of gln += W1^T . ga.  The epilogue parks gln and does the LayerNorm backward on the lane pair's row
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
// PADDING.  Rows >= n contribute nothing because the LOADS of x and gy are masked (x4 / g4 return zeros) and what is parked for them
// is a selected 0.0f, never a product with zero: NaN . 0 is NaN, and the contraction runs over rows.  gln and go of such a row are
// never read by the column sums (they stop at row n).  Columns >= C and hidden units >= Ch are zero in both images, so a padded
// hidden unit has a = 0 and gh = 0; what is parked for it, and for columns >= C, is again a selected 0.0f.  An accumulator row or column of the
// padding is never written to a partial.
#include "mixer_channel.hpp"
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

// ---- the backward's workspace: six transposed arrays, tile by tile
struct mxc_ws {
    int NS, CS, CHS;                             // hidden slices with a unit; parked columns and units per tile (multiples of 32)
    int64_t T;                                   // tiles of 32 rows
    float *hT, *gaT, *lnT, *xhT, *goT, *glnT;    // hT, gaT: [T][CHS][32]; the others [T][CS][32]
};

static __host__ __device__ inline int64_t mxc_ws_floats(int64_t n, int C, int Ch) {
    const int64_t T = (n + 31) / 32;
    return T * 32 * (2 * (int64_t)((Ch + 31) / 32 * 32) + 4 * (int64_t)((C + 31) / 32 * 32));
}

static mxc_ws mxc_make_ws(float* base, int64_t n, int C, int Ch) {
    mxc_ws w;
    w.NS = (Ch + 31) / 32;
    w.CHS = 32 * w.NS;
    w.CS = (C + 31) / 32 * 32;
    w.T = (n + 31) / 32;
    const int64_t hid = w.T * w.CHS * 32, col = w.T * w.CS * 32;
    w.hT = base;
    w.gaT = base + hid;
    w.lnT = base + 2 * hid;
    w.xhT = w.lnT + col;
    w.goT = w.xhT + col;
    w.glnT = w.goT + col;
    return w;
}

// ---- the backward's row-tile kernel and its image
static constexpr int MXB_HG = 4;                 // hidden slices per pass: each holds TWO layer-1 accumulators (a and gh)
// 16-byte elements of a chunk: the larger of a k-step of W1 and of W2^T for MXB_HG slices each and a slice of W1^T for OS output tiles
__host__ __device__ constexpr int mxb_chunk(int OS) { return OS * 256 > 2 * MXB_HG * 128 ? OS * 256 : 2 * MXB_HG * 128; }

struct mxb_dims {
    int C, Ch, KS, NP, OS, CH;                   // k-steps of 16 columns, passes, output tiles (6: C <= 192, else 8), elements per chunk
};
static void mxb_make_dims(int C, int Ch, mxb_dims& o) {
    o.C = C; o.Ch = Ch;
    o.KS = (C + 15) / 16;
    o.NP = ((Ch + 31) / 32 + MXB_HG - 1) / MXB_HG;
    o.OS = C <= 32 * D2_OS ? D2_OS : D2_OS_WIDE;
    o.CH = mxb_chunk(o.OS);
}
static __host__ __device__ inline uint32_t mxb_chunk_elems(const mxb_dims& d) { return (uint32_t)(d.NP * (d.KS + MXB_HG) * d.CH); }
static size_t mxb_image_bytes(const mxb_dims& d) { return (size_t)mxb_chunk_elems(d) * 16 + (size_t)d.NP * MXB_HG * 32 * sizeof(float); }

// The image, chunks of CH elements in the order k_mxc_bwd_rows consumes them, per pass p (slices w0 = 4 p .. w0 + 3), in dense2.hip's
// per-lane operand order (lane = 32 h + r, j = 0..7 the element's eight bf16, piece 0 = hi, 1 = lo):
//   k-step s = 0..KS-1:  element (v * 2 + piece) * 64 + lane, v = 0..3: W1[32 (w0 + v) + r][16 s + 8 h + j]
//                                                             v = 4..7: W2^T[32 (w0 + v - 4) + r][16 s + 8 h + j] = W2[16 s + 8 h + j][..]
//   slice wl = 0..3:     element ((s2 * OS + t) * 2 + piece) * 64 + lane = W1^T[32 t + r][32 (w0 + wl) + acc_row(8 s2 + j, h)]
// zero beyond C and Ch and in the rest of a chunk; then b1 padded to 128 NP floats.
__global__ __launch_bounds__(256) void k_mxc_bwd_image(const float* __restrict__ w1, const float* __restrict__ b1,
                                                       const float* __restrict__ w2, const mxb_dims d, uint4* __restrict__ img) {
    const uint32_t e = blockIdx.x * 256u + threadIdx.x;
    const uint32_t total = mxb_chunk_elems(d);
    const int C = d.C, Ch = d.Ch;
    if (e >= total) {
        const uint32_t f = (e - total) * 4u;                                   // first of four bias floats
        if (f >= (uint32_t)(d.NP * MXB_HG * 32)) return;
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = f + j < (uint32_t)Ch ? b1[f + j] : 0.0f;
        reinterpret_cast<float4*>(img + total)[f / 4u] = make_float4(v[0], v[1], v[2], v[3]);
        return;
    }
    const int chunk = e / (uint32_t)d.CH, el = e % (uint32_t)d.CH;
    const int w0 = chunk / (d.KS + MXB_HG) * MXB_HG, cj = chunk % (d.KS + MXB_HG);
    const int lane = el & 63, piece = (el >> 6) & 1, r = lane & 31, h = lane >> 5;
    float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (cj < d.KS) {
        const int vs = el >> 7;
        const int unit = 32 * (w0 + (vs & 3)) + r;
        if (vs < 2 * MXB_HG && unit < Ch) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int col = 16 * cj + 8 * h + j;
                if (col < C) v[j] = vs < MXB_HG ? w1[(size_t)unit * C + col] : w2[(size_t)col * Ch + unit];
            }
        }
    } else {
        const int wl = cj - d.KS;
        const int s2 = el / (d.OS * 128), t = (el >> 7) % d.OS;
        const int col = 32 * t + r;
        if (s2 < 2 && col < C) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int unit = 32 * (w0 + wl) + acc_row(8 * s2 + j, h);
                if (unit < Ch) v[j] = w1[(size_t)unit * C + col];
            }
        }
    }
    bf16x8 hi, lo;
    split8(v, hi, lo);
    *reinterpret_cast<bf16x8*>(img + e) = piece ? lo : hi;
}

// dense2_rows' mapping and chunk pipeline (a workgroup of 4 waves, one 32-row tile per wave, the image's chunks shared through two LDS
// buffers, one barrier per chunk) with two row sources and two layer-1 accumulators per hidden slice
template <int OSM>
__global__ __launch_bounds__(D2_T) void k_mxc_bwd_rows(const float* __restrict__ x, const float* __restrict__ gy, int64_t n,
                                                       const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                       const mxb_dims d, const uint4* __restrict__ img, float s, uint32_t thr,
                                                       uint32_t k0, uint32_t k1, const mxc_ws ws, float* __restrict__ gx) {
    constexpr int CH = mxb_chunk(OSM), PF = CH / D2_T;
    static_assert(PF == 6 || PF == 8, "the prefetch registers below");
    __shared__ uint4 buf[2][CH];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int64_t tile = (int64_t)blockIdx.x * 4 + wave;
    const int64_t row = tile * 32 + r;
    const bool valid = row < n, park = tile < ws.T;
    const int C = d.C, Ch = d.Ch;
    const float* xr = x + (valid ? row : 0) * C;
    const float* gr = gy + (valid ? row : 0) * C;
    mx_ln_row x4{xr, gamma, beta, C, valid};
    x4.stats(h, eps);
    mxc_drop drop;
    drop.row = row; drop.h = h; drop.s = s; drop.thr = thr; drop.k0 = k0; drop.k1 = k1;
    const uint32_t b2 = (uint32_t)((Ch + 3) / 4);                               // m2's first block
    // columns c .. c + 3 of go = gy m2 s
    auto g4 = [&](int c) -> float4 {
        if (!valid || c >= C) return make_float4(0.f, 0.f, 0.f, 0.f);
        const float4 a = *reinterpret_cast<const float4*>(gr + c);
        if (!thr) return a;
        const uint32_t keep = mxc_keep4(row, b2 + (uint32_t)(c >> 2), thr, k0, k1);
        return make_float4(a.x * drop.scale(keep, 0), a.y * drop.scale(keep, 1), a.z * drop.scale(keep, 2), a.w * drop.scale(keep, 3));
    };
    const int64_t tb = park ? tile : 0;
    float* glnT = ws.glnT + tb * ws.CS * 32 + r;
    float* hT = ws.hT + tb * ws.CHS * 32 + r;
    float* gaT = ws.gaT + tb * ws.CHS * 32 + r;
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
    // ---- the chunk pipeline (dense2_rows'): fetch(c) reads chunk c into registers, commit(b) writes it to buffer b
    const uint32_t nchunks = (uint32_t)(d.NP * (d.KS + MXB_HG));
    uint4 p0, p1, p2, p3, p4, p5, p6, p7;
    auto fetch = [&](uint32_t c) {
        const uint4* src = img + (c < nchunks ? c : 0u) * (uint32_t)CH + tid;
        p0 = src[0]; p1 = src[D2_T]; p2 = src[2 * D2_T]; p3 = src[3 * D2_T]; p4 = src[4 * D2_T]; p5 = src[5 * D2_T];
        if constexpr (PF == 8) { p6 = src[6 * D2_T]; p7 = src[7 * D2_T]; }
    };
    auto commit = [&](int b) {
        uint4* dst = buf[b] + tid;
        dst[0] = p0; dst[D2_T] = p1; dst[2 * D2_T] = p2; dst[3 * D2_T] = p3; dst[4 * D2_T] = p4; dst[5 * D2_T] = p5;
        if constexpr (PF == 8) { dst[6 * D2_T] = p6; dst[7 * D2_T] = p7; }
        __syncthreads();
    };
    const float* bias = reinterpret_cast<const float*>(img + mxb_chunk_elems(d));
    f32x16 y[OSM];                                                              // gln
#pragma unroll
    for (int t = 0; t < OSM; ++t)
#pragma unroll
        for (int q = 0; q < 16; ++q) y[t][q] = 0.0f;
    uint32_t chunk = 0;
    int cur = 0;
    fetch(0);
    commit(0);
    for (int p = 0; p < d.NP; ++p) {
        const int w0 = p * MXB_HG;
        f32x16 aa[MXB_HG], ag[MXB_HG];                                          // a - b1 = W1 . ln and gh = W2^T . go of the pass's slices
#pragma unroll
        for (int wl = 0; wl < MXB_HG; ++wl)
#pragma unroll
            for (int q = 0; q < 16; ++q) aa[wl][q] = ag[wl][q] = 0.0f;
        float4 xa = x4(8 * h), xb = x4(8 * h + 4), ga = g4(8 * h), gb = g4(8 * h + 4);
        for (int ks = 0; ks < d.KS; ++ks) {
            fetch(chunk + 1);
            bf16x8 bxh, bxl, bgh, bgl;
            split8(xa, xb, bxh, bxl);
            split8(ga, gb, bgh, bgl);
            xa = x4(16 * (ks + 1) + 8 * h);                                     // (beyond C: zeros)
            xb = x4(16 * (ks + 1) + 8 * h + 4);
            ga = g4(16 * (ks + 1) + 8 * h);
            gb = g4(16 * (ks + 1) + 8 * h + 4);
            const bf16x8* W = reinterpret_cast<const bf16x8*>(buf[cur]) + lane;
            bf16x8 ah[MXB_HG], al[MXB_HG];
#pragma unroll
            for (int wl = 0; wl < MXB_HG; ++wl) {
                ah[wl] = W[(wl * 2) * 64];
                al[wl] = W[(wl * 2 + 1) * 64];
            }
            mm3(ah, al, bxh, bxl, aa);
#pragma unroll
            for (int wl = 0; wl < MXB_HG; ++wl) {
                ah[wl] = W[((MXB_HG + wl) * 2) * 64];
                al[wl] = W[((MXB_HG + wl) * 2 + 1) * 64];
            }
            mm3(ah, al, bgh, bgl, ag);
            commit(cur ^ 1);
            cur ^= 1;
            ++chunk;
        }
        // ---- slice by slice: h and ga = gh m1 s gelu'(a) of the lane's 16 units (parked for k_mxc_bwd_weights; a selected 0.0f for
        // a row or a unit of the padding), ga the B operand of gln += W1^T . ga
#pragma unroll
        for (int wl = 0; wl < MXB_HG; ++wl) {
            fetch(chunk + 1);
            const int slice = w0 + wl;
            const bool live = park && slice < ws.NS;
            bf16x8 bhh[2], bhl[2];
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                float xg[8];
#pragma unroll
                for (int q4 = 2 * s2; q4 < 2 * s2 + 2; ++q4) {
                    const float4 bb = *reinterpret_cast<const float4*>(bias + 32 * slice + 8 * q4 + 4 * h);
                    const float bv[4] = {bb.x, bb.y, bb.z, bb.w};
                    const uint32_t keep = mxc_keep4(row, (uint32_t)(8 * slice + 2 * q4 + h), thr, k0, k1);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int q = 4 * q4 + j, u = 32 * slice + acc_row(q, h);
                        const float av = aa[wl][q] + bv[j];
                        const float ms = thr ? drop.scale(keep, j) : 1.0f;
                        const float g = gelu_erf(av), gd = gelu_erf_grad(av);
                        const bool real = valid && u < Ch;
                        const float hv = real ? (thr ? g * ms : g) : 0.0f, gav = real ? ag[wl][q] * (ms * gd) : 0.0f;
                        if (live) {
                            hT[u * 32] = hv;
                            gaT[u * 32] = gav;
                        }
                        xg[q - 8 * s2] = gav;
                    }
                }
                split8(xg, bhh[s2], bhl[s2]);
            }
            const bf16x8* W = reinterpret_cast<const bf16x8*>(buf[cur]) + lane;
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                bf16x8 ah[OSM], al[OSM];
#pragma unroll
                for (int t = 0; t < OSM; ++t) {
                    ah[t] = W[((s2 * OSM + t) * 2) * 64];
                    al[t] = W[((s2 * OSM + t) * 2 + 1) * 64];
                }
                mm3(ah, al, bhh[s2], bhl[s2], y);
            }
            commit(cur ^ 1);
            cur ^= 1;
            ++chunk;
        }
    }
    // ---- the LayerNorm backward on the lane pair's row: y[t][4 i .. 4 i + 3] = gln of columns 32 t + 8 i + 4 h + (0..3)
    float s1 = 0.0f, s2 = 0.0f;                                                 // the row sums of gt = gln gamma and of gt xh
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
            const int64_t left = n - t * 32;
            const int nr = left < 32 ? (int)left : 32;
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

static bool mxc_rate(float p) { return p >= 0.0f && p < 1.0f; }                 // (a NaN fails both)
static uint32_t mxc_threshold(float p) { return (uint32_t)((double)p * 4294967296.0); }
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
    if (!mxc_served(n_rows, C, Ch, d) || !mxc_rate(p)) return TPNET_ERR_BAD_ARG;
    if (!mx_aligned16({x, gamma, beta, img, out})) return TPNET_ERR_BAD_ARG;
    if (n_rows == 0) return TPNET_OK;
    const dim3 grid((unsigned)((n_rows + D2_ROWS - 1) / D2_ROWS));
    MXC_LAUNCH(k_mixer_channel_train, d, grid, (hipStream_t)stream, x, n_rows, gamma, beta, eps, d, reinterpret_cast<const uint4*>(img),
               1.0f / (1.0f - p), mxc_threshold(p), (uint32_t)key, (uint32_t)(key >> 32), out);
    TPNET_HIP_TRY(hipGetLastError());
    return TPNET_OK;
}

extern "C" int64_t tpnet_mixer_channel_bwd_partial_floats(int32_t C, int32_t Ch) {
    d2_dims d;
    return mx_channel_dims(C, Ch, d) ? 2 * (int64_t)C + 2 * (int64_t)C * Ch + Ch + C : 0;
}

extern "C" size_t tpnet_mixer_channel_bwd_image_bytes(int32_t C, int32_t Ch) {
    d2_dims d;
    mxb_dims b;
    if (!mx_channel_dims(C, Ch, d)) return 0;
    mxb_make_dims(C, Ch, b);
    return mxb_image_bytes(b);
}

extern "C" int tpnet_mixer_channel_bwd_prepare(const float* w1, const float* b1, const float* w2, int32_t C, int32_t Ch, void* bimg,
                                               void* stream) {
    d2_dims d;
    mxb_dims b;
    if (!w1 || !b1 || !w2 || !bimg || (reinterpret_cast<uintptr_t>(bimg) & 15) || !mx_channel_dims(C, Ch, d)) return TPNET_ERR_BAD_ARG;
    mxb_make_dims(C, Ch, b);
    const uint32_t elems = mxb_chunk_elems(b) + (uint32_t)(b.NP * MXB_HG) * 8u;
    hipLaunchKernelGGL(k_mxc_bwd_image, dim3((elems + 255) / 256), dim3(256), 0, (hipStream_t)stream, w1, b1, w2, b,
                       reinterpret_cast<uint4*>(bimg));
    TPNET_HIP_TRY(hipGetLastError());
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
    if (!mxc_served(n_rows, C, Ch, d) || !mxc_rate(p) || n_partial < 1) return TPNET_ERR_BAD_ARG;
    if (!mx_aligned16({x, gy, gx, gamma, beta, bimg, workspace}) || (reinterpret_cast<uintptr_t>(partial) & 3)) return TPNET_ERR_BAD_ARG;
    if (n_rows == 0) return 0;
    const hipStream_t st = (hipStream_t)stream;
    const mxc_ws ws = mxc_make_ws(static_cast<float*>(workspace), n_rows, C, Ch);
    mxb_dims b;
    mxb_make_dims(C, Ch, b);
    const float s = 1.0f / (1.0f - p);
    const uint32_t thr = mxc_threshold(p), k0 = (uint32_t)key, k1 = (uint32_t)(key >> 32);
    const dim3 grid((unsigned)((n_rows + D2_ROWS - 1) / D2_ROWS));
    const auto rows = b.OS == D2_OS ? k_mxc_bwd_rows<D2_OS> : k_mxc_bwd_rows<D2_OS_WIDE>;
    hipLaunchKernelGGL(rows, grid, dim3(D2_T), 0, st, x, gy, n_rows, gamma, beta, eps, b, reinterpret_cast<const uint4*>(bimg), s, thr, k0,
                       k1, ws, gx);
    TPNET_HIP_TRY(hipGetLastError());
    // row parts of equal tile counts, none empty
    const int64_t tpp = (ws.T + n_partial - 1) / n_partial;
    const int parts = (int)((ws.T + tpp - 1) / tpp);
    hipLaunchKernelGGL(k_mxc_bwd_weights, dim3((unsigned)((ws.NS + 1) / 2 + 1), (unsigned)parts), dim3(256), 0, st, ws, n_rows, (int)C,
                       (int)Ch, tpp, partial);
    TPNET_HIP_TRY(hipGetLastError());
    return parts;
}

extern "C" int tpnet_mixer_channel_masks(int64_t n_rows, int32_t C, int32_t Ch, float p, uint64_t key, uint8_t* m1, uint8_t* m2,
                                         void* stream) {
    d2_dims d;
    if (!m1 || !m2 || !mxc_served(n_rows, C, Ch, d) || !mxc_rate(p)) return TPNET_ERR_BAD_ARG;
    if (n_rows == 0) return TPNET_OK;
    const int64_t total = n_rows * ((Ch + 3) / 4 + C / 4);
    if (total > 0xffffff00ll) return TPNET_ERR_BAD_ARG;                         // (one thread per block of draws; a launch has < 2^32)
    hipLaunchKernelGGL(k_mixer_channel_masks, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n_rows, (int)C,
                       (int)Ch, mxc_threshold(p), (uint32_t)key, (uint32_t)(key >> 32), m1, m2);
    TPNET_HIP_TRY(hipGetLastError());
    return TPNET_OK;
}
