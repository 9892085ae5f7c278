// The backward of dense2.hpp's two layers in a TRAINING step on the matrix cores, once (mixer_channel_train.hip: the channel FFN
// behind a LayerNorm, GELU with dropout; encoder_input_train.hip: projection_layer on the gathered concat, the saved ReLU bits).
// With x the layers' input rows, g the gradient of their output, a = W1 . x + b1 and (h, ga) = rule(a, gh):
//   gh = W2^T . g        ga -> gb1 = sum ga, gw1 = sum ga (x) x        h -> gw2 = sum g (x) h        y = W1[:, G columns]^T . ga
// in TWO launches that share a workspace of the call, cut into tiles of 32 rows and held TRANSPOSED -- element [tile][unit or
// column][row of the tile] (rows_contract.hpp) -- so that a lane of the row-tile kernel (lane = row) stores 32 consecutive floats per
// wave store, and a lane of the contraction over rows loads its 8 consecutive rows of one unit as two float4, already in operand order.
// A row-tile kernel gives dense2_bwd_rows the two row sources -- columns c .. c + 3 of x and of g of its lane's row -- the rule
// and what is done with y; it parks what else its weight kernel contracts.  Everything between is here: the sizes, the image and its
// kernel, the workspace's head, the row-tile body and the host's launch geometry.
// ARITHMETIC.  All products are the fp32 class of mfma_split.hpp (two bf16 pieces per operand, mm3's three products, fp32
// accumulators); a rule, the masks and the column sums are plain fp32.
// PADDING.  Rows >= n contribute nothing because the LOADS of x and g are masked (the row sources return zeros) and what is parked for
// them is a selected 0.0f, never a product with zero: NaN . 0 is NaN, and the contraction runs over rows.  What a kernel parks per
// column for such a row is never read by the column sums (they stop at row n: d2b_tile_rows).  Columns >= Din / Dout / G and hidden
// units >= H are zero in the image, so a padded hidden unit has a = 0 and gh = 0; what is parked for it, and for a column of the
// padding, is again a selected 0.0f.  An accumulator row or column of the padding is never written to a partial or to a gradient.
#pragma once
#include "dense2.hpp"

namespace tpnet {

// ---- the sizes
static constexpr int D2B_HG = 4;                 // hidden slices per pass: each holds TWO layer-1 accumulators (a and gh)
// 16-byte elements of a chunk: the larger of a k-step of W1 and of W2^T for D2B_HG slices each and a slice of W1^T for OS output tiles
__host__ __device__ constexpr int d2b_chunk(int OS) { return OS * 256 > 2 * D2B_HG * 128 ? OS * 256 : 2 * D2B_HG * 128; }

struct d2b_dims {
    int Din, H, Dout;                            // W1 [H][Din], W2 [Dout][H]
    int G, Gt, ct, cf;                           // G columns of x take a gradient: W1's columns ct + g for g < Gt, else cf + g - Gt
    int KS, NS, NP, OS, CH;                      // k-steps of 16 (of the longer of Din and Dout), hidden slices with a unit, passes,
};                                               // output tiles (6: G <= 192, else 8), elements per chunk

// the caller's check: G <= 256 (8 output tiles of the row-tile kernel).  mixer_channel_train.hip is Din = Dout = G = Gt = C, ct = 0
static inline void d2b_make_dims(int Din, int H, int Dout, int Gt, int ct, int Gf, int cf, d2b_dims& o) {
    o.Din = Din; o.H = H; o.Dout = Dout;
    o.G = Gt + Gf; o.Gt = Gt; o.ct = ct; o.cf = cf;
    o.KS = ((Din > Dout ? Din : Dout) + 15) / 16;
    o.NS = (H + 31) / 32;
    o.NP = (o.NS + D2B_HG - 1) / D2B_HG;
    o.OS = o.G <= 32 * D2_OS ? D2_OS : D2_OS_WIDE;
    o.CH = d2b_chunk(o.OS);
}
static __host__ __device__ inline uint32_t d2b_chunk_elems(const d2b_dims& d) { return (uint32_t)(d.NP * (d.KS + D2B_HG) * d.CH); }
static inline size_t d2b_image_bytes(const d2b_dims& d) {
    return (size_t)d2b_chunk_elems(d) * 16 + (size_t)d.NP * D2B_HG * 32 * sizeof(float);
}

// The image, chunks of CH elements in the order dense2_bwd_rows consumes them, per pass p (slices w0 = 4 p .. w0 + 3), in dense2.hip's
// per-lane operand order (lane = 32 h + r, j = 0..7 the element's eight bf16, piece 0 = hi, 1 = lo):
//   k-step s = 0..KS-1:  element (v * 2 + piece) * 64 + lane, v = 0..3: W1[32 (w0 + v) + r][16 s + 8 h + j]
//                                                             v = 4..7: W2^T[32 (w0 + v - 4) + r][16 s + 8 h + j] = W2[16 s + 8 h + j][..]
//   slice wl = 0..3:     element ((s2 * OS + t) * 2 + piece) * 64 + lane = W1[32 (w0 + wl) + acc_row(8 s2 + j, h)][column of g = 32 t + r]
//                        = W1^T of the G columns (d2b_dims: ct + g, or cf + g - Gt)
// zero beyond Din, Dout, G and H and in the rest of a chunk; then b1 padded to 128 NP floats.  (static: a header's kernel, one copy per
// file that includes it, like scan_common.hpp's)
static __global__ __launch_bounds__(256) void k_dense2_bwd_image(const float* __restrict__ w1, const float* __restrict__ b1,
                                                          const float* __restrict__ w2, const d2b_dims d, uint4* __restrict__ img) {
    const uint32_t e = blockIdx.x * 256u + threadIdx.x;
    const uint32_t total = d2b_chunk_elems(d);
    if (e >= total) {
        const uint32_t f = (e - total) * 4u;                                   // first of four bias floats
        if (f >= (uint32_t)(d.NP * D2B_HG * 32)) return;
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = f + j < (uint32_t)d.H ? b1[f + j] : 0.0f;
        reinterpret_cast<float4*>(img + total)[f / 4u] = make_float4(v[0], v[1], v[2], v[3]);
        return;
    }
    const int chunk = e / (uint32_t)d.CH, el = e % (uint32_t)d.CH;
    const int w0 = chunk / (d.KS + D2B_HG) * D2B_HG, cj = chunk % (d.KS + D2B_HG);
    const int lane = el & 63, piece = (el >> 6) & 1, r = lane & 31, h = lane >> 5;
    float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (cj < d.KS) {
        const int vs = el >> 7;
        const int unit = 32 * (w0 + (vs & 3)) + r;
        if (vs < 2 * D2B_HG && unit < d.H) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int col = 16 * cj + 8 * h + j;
                if (vs < D2B_HG) {
                    if (col < d.Din) v[j] = w1[(size_t)unit * d.Din + col];
                } else if (col < d.Dout) {
                    v[j] = w2[(size_t)col * d.H + unit];
                }
            }
        }
    } else {
        const int wl = cj - d.KS;
        const int s2 = el / (d.OS * 128), t = (el >> 7) % d.OS;
        const int g = 32 * t + r;
        if (s2 < 2 && g < d.G) {
            const int col = g < d.Gt ? d.ct + g : d.cf + (g - d.Gt);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int unit = 32 * (w0 + wl) + acc_row(8 * s2 + j, h);
                if (unit < d.H) v[j] = w1[(size_t)unit * d.Din + col];
            }
        }
    }
    bf16x8 hi, lo;
    split8(v, hi, lo);
    *reinterpret_cast<bf16x8*>(img + e) = piece ? lo : hi;
}

// ONE launch that writes the image from the three Parameters it holds
static inline hipError_t d2b_prepare(const float* w1, const float* b1, const float* w2, const d2b_dims& d, void* bimg, hipStream_t st) {
    const uint32_t elems = d2b_chunk_elems(d) + (uint32_t)(d.NP * D2B_HG) * 8u;
    hipLaunchKernelGGL(k_dense2_bwd_image, dim3((elems + 255) / 256), dim3(256), 0, st, w1, b1, w2, d, reinterpret_cast<uint4*>(bimg));
    return hipGetLastError();
}

// ---- the workspace's head: h and ga of every row, transposed, tile by tile.  A kernel file's workspace derives from it and adds its
// tail of padded column arrays
struct d2b_ws {
    int NS, CHS;                                 // hidden slices with a unit; parked units per tile (a multiple of 32)
    int64_t T;                                   // tiles of 32 rows
    float *hT, *gaT;                             // [T][CHS][32]
};
static __host__ __device__ inline int d2b_pad32(int v) { return (v + 31) / 32 * 32; }
static __host__ __device__ inline int64_t d2b_tiles(int64_t n) { return (n + 31) / 32; }
// fills the head from `base`; returns the first float behind it
static inline float* d2b_make_ws(d2b_ws& w, float* base, int64_t n, int H) {
    w.NS = (H + 31) / 32;
    w.CHS = 32 * w.NS;
    w.T = d2b_tiles(n);
    w.hT = base;
    w.gaT = base + w.T * w.CHS * 32;
    return w.gaT + w.T * w.CHS * 32;
}
// rows < n of tile t: where the column sums of a weight kernel stop
__device__ __forceinline__ int d2b_tile_rows(int64_t n, int64_t t) {
    const int64_t left = n - t * 32;
    return left < 32 ? (int)left : 32;
}

// The body of a row-tile kernel of D2_T threads: dense2_rows' mapping and chunk pipeline (a workgroup of 4 waves, one 32-row tile per
// wave, the image's chunks shared through two LDS buffers, one barrier per chunk) with two row sources and two layer-1 accumulators
// per hidden slice.  OSM output tiles; SHORTG: Dout may be shorter than Din, and the k-steps beyond it skip gh's products (a kernel
// with Din == Dout has no such step and no test in its loop).  Lane (r = lane & 31, h = lane >> 5) of wave w works on row
// 32 tile + r, tile = 4 blockIdx.x + w: x4(c), g4(c) = columns c .. c + 3 of that row's x and g (c % 4 == 0; zeros beyond Din / Dout
// and for a row that is not `valid`).
// A rule is an object, like dense2_rows' activations.  Registers 4 q4 .. 4 q4 + 3 of a lane are four consecutive hidden units,
// 32 slice + acc_row(4 q4 + j, h): block(slice, q4) gives the rule's four decisions about them (bit j; a mask, a saved bit), and
// unit(bits, j, real, a, gh, hv, gav) turns a = W1 . x + b1 and gh of unit j into h and ga -- a selected 0.0f for both unless
// `real` (a row of the call and a unit of the layer).  What it needs of the row it carries as members.  epi(y) takes
// y[t][4 i .. 4 i + 3] = columns 32 t + 8 i + 4 h + (0..3) of W1[:, G columns]^T . ga, by every lane of the wave.
template <int OSM, bool SHORTG, class SRCX, class SRCG, class RULE, class EPI>
__device__ __forceinline__ void dense2_bwd_rows(const d2b_dims& d, const uint4* __restrict__ img, const d2b_ws& ws, const bool valid,
                                                const SRCX& x4, const SRCG& g4, const RULE& rule, const EPI& epi) {
    constexpr int CH = d2b_chunk(OSM), PF = CH / D2_T;
    static_assert(PF == 6 || PF == 8, "the prefetch registers below");
    __shared__ uint4 buf[2][CH];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int64_t tile = (int64_t)blockIdx.x * 4 + wave;
    const bool park = tile < ws.T;
    const int64_t tb = park ? tile : 0;
    float* hT = ws.hT + tb * ws.CHS * 32 + r;
    float* gaT = ws.gaT + tb * ws.CHS * 32 + r;
    // ---- the chunk pipeline (dense2_rows'): fetch(c) reads chunk c into registers, commit(b) writes it to buffer b
    const uint32_t nchunks = (uint32_t)(d.NP * (d.KS + D2B_HG));
    uint4 p0, p1, p2, p3, p4, p5, p6, p7;      // (named, not an array: dense2_rows' reason)
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
    const float* bias = reinterpret_cast<const float*>(img + d2b_chunk_elems(d));
    f32x16 y[OSM];
#pragma unroll
    for (int t = 0; t < OSM; ++t)
#pragma unroll
        for (int q = 0; q < 16; ++q) y[t][q] = 0.0f;
    uint32_t chunk = 0;
    int cur = 0;
    fetch(0);
    commit(0);
    for (int p = 0; p < d.NP; ++p) {
        const int w0 = p * D2B_HG;
        f32x16 aa[D2B_HG], ag[D2B_HG];                                          // a - b1 = W1 . x and gh = W2^T . g of the pass's slices
#pragma unroll
        for (int wl = 0; wl < D2B_HG; ++wl)
#pragma unroll
            for (int q = 0; q < 16; ++q) aa[wl][q] = ag[wl][q] = 0.0f;
        float4 xa = x4(8 * h), xb = x4(8 * h + 4), ga = g4(8 * h), gb = g4(8 * h + 4);
        for (int ks = 0; ks < d.KS; ++ks) {
            fetch(chunk + 1);
            bf16x8 bxh, bxl, bgh, bgl;
            split8(xa, xb, bxh, bxl);
            split8(ga, gb, bgh, bgl);
            xa = x4(16 * (ks + 1) + 8 * h);                                     // (beyond Din / Dout: zeros)
            xb = x4(16 * (ks + 1) + 8 * h + 4);
            ga = g4(16 * (ks + 1) + 8 * h);
            gb = g4(16 * (ks + 1) + 8 * h + 4);
            const bf16x8* W = reinterpret_cast<const bf16x8*>(buf[cur]) + lane;
            bf16x8 ah[D2B_HG], al[D2B_HG];
#pragma unroll
            for (int wl = 0; wl < D2B_HG; ++wl) {
                ah[wl] = W[(wl * 2) * 64];
                al[wl] = W[(wl * 2 + 1) * 64];
            }
            mm3(ah, al, bxh, bxl, aa);
            if (!SHORTG || 16 * ks < d.Dout) {                                  // (uniform; beyond Dout both operands are zeros)
#pragma unroll
                for (int wl = 0; wl < D2B_HG; ++wl) {
                    ah[wl] = W[((D2B_HG + wl) * 2) * 64];
                    al[wl] = W[((D2B_HG + wl) * 2 + 1) * 64];
                }
                mm3(ah, al, bgh, bgl, ag);
            }
            commit(cur ^ 1);
            cur ^= 1;
            ++chunk;
        }
        // ---- slice by slice: h and ga of the lane's 16 units (parked for the weight kernel; a selected 0.0f for a row or a unit of
        // the padding), ga the B operand of y += W1[:, G columns]^T . ga
#pragma unroll
        for (int wl = 0; wl < D2B_HG; ++wl) {
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
                    const uint32_t bits = rule.block(slice, q4);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int q = 4 * q4 + j, u = 32 * slice + acc_row(q, h);
                        float hv, gav;
                        rule.unit(bits, j, valid && u < d.H, aa[wl][q] + bv[j], ag[wl][q], hv, gav);
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
    epi(y);
}

// ---- the saved ReLU bits (encoder_input_train.hip, mlp_l4.hip): relu_bits [n][ceil(H / 32)] uint32, bit u % 32 of word u / 32 of a
// row = the forward's decision about hidden unit u.
// The forward's activation (dense2.hpp: split16 of slice w; register q of lane half h = hidden unit 32 w + acc_row(q, h)): ReLU,
// and bit acc_row(q, h) of word w of the lane's row = the decision.  The two lanes of a row hold 16 units each.
struct act_relu_bits {
    uint32_t* words;                             // relu_bits of the lane's row
    int NW;                                      // ceil(H / 32) words per row; 0 for a row >= n: nothing is stored
    __device__ __forceinline__ void split16(const f32x16& a, const float (&bias)[16], int w, bf16x8 (&bh)[2], bf16x8 (&bl)[2]) const {
        const int h = (threadIdx.x >> 5) & 1;
        uint32_t m = 0u;
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
            float x[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int q = 8 * s2 + j;
                x[j] = a[q] + bias[q];
                const bool on = x[j] > 0.0f;
                m |= on ? 1u << acc_row(q, 0) : 0u;
                x[j] = on ? x[j] : 0.0f;
            }
            split8(x, bh[s2], bl[s2]);
        }
        m <<= 4 * h;                                                            // acc_row(q, h) = acc_row(q, 0) + 4 h
        m |= (uint32_t)__shfl_xor((int)m, 32);
        if (h == 0 && w < NW) words[w] = m;
    }
};
// The backward's rule: h = m ? a : 0 and ga = m ? gh : 0, m the saved bit of the unit -- the four of a block are bits
// acc_row(4 q4, h) .. + 3 of the slice's word of the lane's row (act_relu_bits wrote it; 0 for a slice of the padding)
struct rule_relu_bits {
    const uint32_t* __restrict__ words;          // relu_bits of the lane's row
    int NW;                                      // ceil(H / 32) words per row; 0 for a row >= n: nothing is read
    __device__ __forceinline__ uint32_t block(int slice, int q4) const {
        return (slice < NW ? words[slice] : 0u) >> acc_row(4 * q4, (threadIdx.x >> 5) & 1);
    }
    __device__ __forceinline__ void unit(uint32_t m, int j, bool real, float a, float gh, float& hv, float& gav) const {
        const bool on = ((m >> j) & 1u) != 0u && real;
        hv = on ? a : 0.0f;
        gav = on ? gh : 0.0f;
    }
};

// ---- the host's side of the two launches
// row parts of equal tile counts, none empty: tiles per part, and the parts (= the partials the weight kernel writes)
static inline int d2b_row_parts(int64_t T, int32_t n_partial, int64_t& tpp) {
    tpp = (T + n_partial - 1) / n_partial;
    return (int)((T + tpp - 1) / tpp);
}
// the row-tile kernel of d (6 or 8 output tiles) on the grid of n rows
#define D2B_LAUNCH_ROWS(KERNEL, d, n, stream, ...)                                                                         \
    do {                                                                                                                   \
        hipLaunchKernelGGL((d).OS == D2_OS ? KERNEL<D2_OS> : KERNEL<D2_OS_WIDE>, dim3((unsigned)(((n) + D2_ROWS - 1) / D2_ROWS)), \
                           dim3(D2_T), 0, stream, __VA_ARGS__);                                                            \
        TPNET_HIP_TRY(hipGetLastError());                                                                                  \
    } while (0)

}  // namespace tpnet
