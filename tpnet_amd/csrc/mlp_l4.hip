// self.mlp = Linear(100, 400) -> ReLU -> Linear(400, 100) of num_layer 4 (models/TPNet.py:63-65) on the matrix cores in the fp32
// class: one launch forward, two backward.  The split weights are 320 KB against 160 KB of LDS (tpnet_mlp_rows_supported), so they
// are STREAMED: the kernels are dense2.hpp's two layers and dense2_bwd.hpp's backward with a row source of their own -- x[n][100],
// one masked float4 per four columns -- and nothing else new.
//   k_mlp_l4<false>   y = W2 . relu(W1 . x + b1) + b2: dense2_rows with act_relu, two passes of 7 hidden slices, 4 output tiles
//                     (l4_dims below: the variant).
//   k_mlp_l4<true>    the same body with act_relu_bits: relu_bits [n][13] uint32, bit u % 32 of word u / 32 = (W1 . x + b1)[u] > 0
//                     exactly as this launch decided it; the bits of the padded units 400..415 are 0.  y has the bits of <false>'s.
//   the backward from gy   a = W1 . x + b1      h = m ? a : 0       gh = W2^T . gy      ga = m ? gh : 0      (m the saved bits)
//                          gw1 = sum ga (x) x   gb1 = sum ga        gw2 = sum gy (x) h  gb2 = sum gy         (every sum over the rows)
//                     No gradient by x is formed (G = 0: the features come from the readout, which has none).
//   k_l4b_rows        parks x and gy of its tiles transposed, then dense2_bwd_rows with x and gy as the row sources and the rule
//                     of the saved bits, which parks h and ga.  Its y (W1[:, G columns]^T . ga, G = 0) is not stored.
//   k_l4b_weights     the contraction over rows (rows_contract.hpp).  A wave owns a 32-unit hidden slice of ONE product -- gw1[slice,
//                     :] = sum_rows ga^T x or gw2[:, slice]^T = sum_rows h^T gy, 4 column tiles each -- and a workgroup one part of
//                     the row tiles; gb1 is the sum of the ga operands gw1's wave loads.  The last workgroup of a row part adds gb2 in
//                     plain fp32, thread = column, rows in order.  Every row part writes ONE partial (gw1 | gb1 | gw2 | gb2,
//                     unpadded); the caller adds the partials in a fixed order.  No atomics: two calls give equal bits.
// ARITHMETIC.  All products are the fp32 class of mfma_split.hpp; the masks and the column sums are plain fp32.
// PADDING.  dense2.hpp's and dense2_bwd.hpp's rules: the row sources return zeros for a row >= n and a column >= 100 (never a load),
// rows >= n and the padded output columns are never stored, a hidden unit of the padding has bit 0.
#include "dense2_bwd.hpp"
#include "rows_contract.hpp"

namespace tpnet {

static constexpr int L4_F = 100, L4_H = 400;
static constexpr int L4_NW = (L4_H + 31) / 32;  // words of relu_bits per row
static constexpr int L4_WT = 4;                  // accumulator tiles of a weight wave: pad32(100) = 128 columns

// columns c .. c + 3 of the lane's row of a [n][100] matrix (c % 4 == 0; 400-byte rows keep a float4 aligned); zeros beyond 100
// columns and for a row >= n
struct l4_row {
    const float* p;                              // the row; NULL for a row >= n
    __device__ __forceinline__ float4 operator()(int c) const {
        if (!p || c >= L4_F) return make_float4(0.f, 0.f, 0.f, 0.f);
        return *reinterpret_cast<const float4*>(p + c);
    }
};

// The forward's variant.  d2_make_dims(100, 400, 100, mid) gives passes of 8 hidden slices with 6 output tiles: 16 slices and 6 tiles
// are computed where 13 and 4 hold data, 912 matrix instructions per 32-row tile.  TWO passes of 7 slices with 4 output tiles hold
// everything in 630, in chunks of 1 024 elements (4 prefetch registers); the sums run in the same order, so the outputs have the
// same bits.  -DTPNET_L4_FIRST_VARIANT builds the first one (profiles/mlp_l4.md: the comparison).
#ifdef TPNET_L4_FIRST_VARIANT
static constexpr int L4_HG = D2_HG_WIDE, L4_OS = D2_OS;
static void l4_dims(d2_dims& d) { d2_make_dims(L4_F, L4_H, L4_F, true, d); }
#else
static constexpr int L4_HG = 7, L4_OS = 4;
static void l4_dims(d2_dims& d) {
    d.Din = L4_F; d.H = L4_H; d.Dout = L4_F;
    d.KS = (L4_F + 15) / 16;
    d.HG = L4_HG; d.NP = 2; d.OS = L4_OS;
    d.CH = d2_chunk(L4_HG, L4_OS);
}
static_assert(2 * L4_HG * 32 >= L4_H && L4_OS * 32 >= L4_F, "two passes hold every hidden unit, the tiles every output");
#endif

template <bool BITS>
__global__ __launch_bounds__(D2_T) void k_mlp_l4(const float* __restrict__ x, int64_t n, const d2_dims d, const uint4* __restrict__ img,
                                                 float* __restrict__ y, uint32_t* __restrict__ relu_bits) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t row = ((int64_t)blockIdx.x * 4 + wave) * 32 + (lane & 31);
    const bool valid = row < n;
    const l4_row x4{valid ? x + row * L4_F : nullptr};
    float* yo = y + (valid ? row : 0) * L4_F;
    auto put = [&](int o, const float4 v) { *reinterpret_cast<float4*>(yo + o) = v; };
    if constexpr (BITS) {
        act_relu_bits act;
        act.NW = valid ? L4_NW : 0;
        act.words = relu_bits + (valid ? row : 0) * L4_NW;
        dense2_rows<L4_HG, L4_OS, true, act_relu_bits>(d, img, valid, x4, put, act);
    } else {
        dense2_rows<L4_HG, L4_OS, true, act_relu>(d, img, valid, x4, put);
    }
}

static void l4b_dims(d2b_dims& d) { d2b_make_dims(L4_F, L4_H, L4_F, 0, 0, 0, 0, d); }
static constexpr int64_t L4B_PARTIAL = 2 * (int64_t)L4_H * L4_F + L4_H + L4_F;

// ---- the backward's workspace: dense2_bwd.hpp's head (hT, gaT) and x and gy transposed, tile by tile
struct l4b_ws : d2b_ws {
    int CS;                                      // parked columns of x and of gy per tile: pad32(100)
    float *xT, *gyT;                             // [T][CS][32] each
};
static int64_t l4b_ws_floats(int64_t n) { return d2b_tiles(n) * 32 * (2 * (int64_t)d2b_pad32(L4_H) + 2 * d2b_pad32(L4_F)); }
static l4b_ws l4b_make_ws(float* base, int64_t n) {
    l4b_ws w;
    w.xT = d2b_make_ws(w, base, n, L4_H);
    w.CS = d2b_pad32(L4_F);
    w.gyT = w.xT + w.T * w.CS * 32;
    return w;
}

__global__ __launch_bounds__(D2_T) void k_l4b_rows(const float* __restrict__ x, const uint32_t* __restrict__ relu_bits,
                                                   const float* __restrict__ gy, int64_t n, const d2b_dims d,
                                                   const uint4* __restrict__ img, const l4b_ws ws) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int64_t tile = (int64_t)blockIdx.x * 4 + wave;
    const int64_t row = tile * 32 + r;
    const bool valid = row < n;
    const l4_row x4{valid ? x + row * L4_F : nullptr}, g4{valid ? gy + row * L4_F : nullptr};
    rule_relu_bits rule;
    rule.NW = valid ? L4_NW : 0;
    rule.words = relu_bits + (valid ? row : 0) * L4_NW;
    // ---- x and gy of the tile, parked for the weight kernel before the accumulators are live (a row >= n, a column >= 100:
    // selected zeros); the two lanes of a row take alternate groups of four columns
    if (tile < ws.T) {
        float* xT = ws.xT + tile * ws.CS * 32 + r;
        float* gyT = ws.gyT + tile * ws.CS * 32 + r;
        for (int c = 4 * h; c < ws.CS; c += 8) {
            const float4 a = x4(c), b = g4(c);
            xT[c * 32] = a.x; xT[(c + 1) * 32] = a.y; xT[(c + 2) * 32] = a.z; xT[(c + 3) * 32] = a.w;
            gyT[c * 32] = b.x; gyT[(c + 1) * 32] = b.y; gyT[(c + 2) * 32] = b.z; gyT[(c + 3) * 32] = b.w;
        }
    }
    dense2_bwd_rows<D2_OS, false>(d, img, ws, valid, x4, g4, rule, [](const f32x16 (&)[D2_OS]) {});
}

// grid (ceil(2 NS / 4) + 1, row parts).  tpp: tiles per row part (every part holds one)
__global__ __launch_bounds__(256) void k_l4b_weights(const l4b_ws ws, int64_t n, int64_t tpp, float* __restrict__ partial) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int64_t t0 = (int64_t)blockIdx.y * tpp, t1 = t0 + tpp < ws.T ? t0 + tpp : ws.T;
    float* gw1 = partial + (int64_t)blockIdx.y * L4B_PARTIAL;
    float* gb1 = gw1 + L4_H * L4_F;
    float* gw2 = gb1 + L4_H;
    float* gb2 = gw2 + L4_F * L4_H;
    if (blockIdx.x == gridDim.x - 1) {
        // ---- gb2, no matrix product: thread = column, rows in order, rows >= n never added
        for (int c = tid; c < L4_F; c += 256) {
            float so = 0.0f;
            for (int64_t t = t0; t < t1; ++t) {
                const int nr = d2b_tile_rows(n, t);
                const float* go = ws.gyT + (t * ws.CS + c) * 32;
                for (int i = 0; i < nr; ++i) so += go[i];
            }
            gb2[c] = so;
        }
        return;
    }
    const int item = 4 * blockIdx.x + wave;                                     // (no barrier in this kernel)
    if (item >= 2 * ws.NS) return;
    const bool first = item < ws.NS;                                            // gw1[slice, :] = sum_rows ga^T x, else
    const int slice = first ? item : item - ws.NS;                              // gw2[:, slice]^T = sum_rows h^T gy
    f32x16 acc[L4_WT];
#pragma unroll
    for (int t = 0; t < L4_WT; ++t)
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[t][q] = 0.0f;
    float asum = rc_walk(first ? ws.gaT : ws.hT, ws.CHS, slice, first ? ws.xT : ws.gyT, ws.CS, 0, L4_WT, t0, t1, r, h, acc);
#pragma unroll
    for (int tt = 0; tt < L4_WT; ++tt) {
        const int c = 32 * tt + r;
        if (c < L4_F) {
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int j = 32 * slice + acc_row(q, h);
                if (j < L4_H) (first ? gw1 + j * L4_F + c : gw2 + c * L4_H + j)[0] = acc[tt][q];
            }
        }
    }
    asum += __shfl_xor(asum, 32);
    if (first && h == 0 && 32 * slice + r < L4_H) gb1[32 * slice + r] = asum;
}

}  // namespace tpnet

using namespace tpnet;

extern "C" int tpnet_mlp_l4_supported(int32_t F, int32_t H) { return F == L4_F && H == L4_H; }

extern "C" size_t tpnet_mlp_l4_image_bytes(void) {
    d2_dims d;
    l4_dims(d);
    return d2_image_bytes(d);
}

extern "C" int tpnet_mlp_l4_prepare(const float* w1, const float* b1, const float* w2, const float* b2, void* img, void* stream) {
    if (!w1 || !b1 || !w2 || !b2 || !img || (reinterpret_cast<uintptr_t>(img) & 15)) return TPNET_ERR_BAD_ARG;
    d2_dims d;
    l4_dims(d);
    return d2_prepare(w1, b1, w2, b2, d, img, (hipStream_t)stream);
}

extern "C" int tpnet_mlp_l4_f32(const float* x, int64_t n, const void* img, float* y, uint32_t* relu_bits, void* stream) {
    if (!x || !y || !img || n < 0 || n > (1ll << 31) || !aligned16({x, y, img}) || (reinterpret_cast<uintptr_t>(relu_bits) & 3))
        return TPNET_ERR_BAD_ARG;
    if (n == 0) return TPNET_OK;
    d2_dims d;
    l4_dims(d);
    const dim3 grid((unsigned)((n + D2_ROWS - 1) / D2_ROWS));
    const uint4* im = reinterpret_cast<const uint4*>(img);
    if (relu_bits) hipLaunchKernelGGL(k_mlp_l4<true>, grid, dim3(D2_T), 0, (hipStream_t)stream, x, n, d, im, y, relu_bits);
    else hipLaunchKernelGGL(k_mlp_l4<false>, grid, dim3(D2_T), 0, (hipStream_t)stream, x, n, d, im, y, relu_bits);
    TPNET_HIP_TRY(hipGetLastError());
    return TPNET_OK;
}

extern "C" size_t tpnet_mlp_l4_bwd_image_bytes(void) {
    d2b_dims d;
    l4b_dims(d);
    return d2b_image_bytes(d);
}

extern "C" int tpnet_mlp_l4_bwd_prepare(const float* w1, const float* b1, const float* w2, void* bimg, void* stream) {
    if (!w1 || !b1 || !w2 || !bimg || (reinterpret_cast<uintptr_t>(bimg) & 15)) return TPNET_ERR_BAD_ARG;
    d2b_dims d;
    l4b_dims(d);
    TPNET_HIP_TRY(d2b_prepare(w1, b1, w2, d, bimg, (hipStream_t)stream));
    return TPNET_OK;
}

extern "C" int64_t tpnet_mlp_l4_bwd_partial_floats(void) { return L4B_PARTIAL; }

extern "C" size_t tpnet_mlp_l4_bwd_workspace_bytes(int64_t n) {
    if (n < 0 || n > (1ll << 31)) return 0;
    return (size_t)l4b_ws_floats(n) * sizeof(float);
}

extern "C" int tpnet_mlp_l4_bwd_f32(const float* x, const uint32_t* relu_bits, const float* gy, int64_t n, const void* bimg, void* ws,
                                    float* partial, int32_t n_partial, void* stream) {
    if (!x || !relu_bits || !gy || !bimg || !ws || !partial || n < 0 || n > (1ll << 31) || n_partial < 1) return TPNET_ERR_BAD_ARG;
    if (!aligned16({x, gy, bimg, ws}) || ((reinterpret_cast<uintptr_t>(relu_bits) | reinterpret_cast<uintptr_t>(partial)) & 3))
        return TPNET_ERR_BAD_ARG;
    if (n == 0) return 0;
    const hipStream_t st = (hipStream_t)stream;
    d2b_dims d;
    l4b_dims(d);
    const l4b_ws w = l4b_make_ws(static_cast<float*>(ws), n);
    hipLaunchKernelGGL(k_l4b_rows, dim3((unsigned)((n + D2_ROWS - 1) / D2_ROWS)), dim3(D2_T), 0, st, x, relu_bits, gy, n, d,
                       reinterpret_cast<const uint4*>(bimg), w);
    TPNET_HIP_TRY(hipGetLastError());
    int64_t tpp;
    const int parts = d2b_row_parts(w.T, n_partial, tpp);
    hipLaunchKernelGGL(k_l4b_weights, dim3((unsigned)((2 * w.NS + 3) / 4 + 1), (unsigned)parts), dim3(256), 0, st, w, n, tpp, partial);
    TPNET_HIP_TRY(hipGetLastError());
    return parts;
}
