// Two dense layers on the matrix cores over rows that are never written as a matrix: out[row] = W2 . act(W1 . x[row] + b1) + b2,
// once (encoder_input.hip: the gathered concat, ReLU; mixer.hip: the LayerNorm of a row, GELU, + residual; mixer_channel_train.hip:
// the same with dropout).  A kernel gives the
// row source -- columns c .. c + 3 of its lane's row -- the activation and what is done with four outputs; everything between is here.
// Arithmetic: the project's fp32 class (mfma_split.hpp: two-piece operands, three products per term on v_mfma_f32_32x32x16_bf16,
// fp32 accumulators).  Layer 1 is computed as H^T = W1 . X^T, so a hidden slice's accumulator registers
// (row r of the tile, 16 hidden units per lane) are layer 2's B operand without a transpose.
// Mapping: a workgroup of 4 waves takes 128 rows, one 32-row tile per wave.  The split weights (dense2_prepare: 1.16 MB
// at 572 -> 344 -> 172, in exactly the per-lane operand order) do not fit LDS; they are cut into equal chunks -- one k-step
// of W1 for all hidden slices of a pass, later one hidden slice of W2 for all output tiles -- that the four waves share through
// two LDS buffers: the next chunk is fetched into registers ahead of the current one's products and written to the other buffer
// behind them, one barrier per chunk.  Up to 11 hidden slices (352 units) stay in accumulators at once; a wider hidden layer or
// more than 192 outputs take passes of 8 slices over the row's operands.
#pragma once
#include "tpnet_common.h"
#include "mfma_split.hpp"

namespace tpnet {

static constexpr int D2_T = 256;                 // threads per workgroup: 4 waves, one per SIMD (the accumulators want the registers)
static constexpr int D2_ROWS = 128;              // rows per workgroup
static constexpr int D2_HG = 11;                 // hidden slices of 32 units in one pass of the narrow variant (H <= 352, Dout <= 192)
static constexpr int D2_HG_WIDE = 8;             // ... per pass of the others (any served H): fewer, to leave room for the later passes
static constexpr int D2_OS = 6, D2_OS_WIDE = 8;  // output tiles of 32 columns a variant computes
// 16-byte elements of a chunk of the weight image: the larger of a k-step of W1 for HG slices (HG * 128) and a slice of W2 for OS
// output tiles (OS * 256), a multiple of the workgroup size -- every thread moves the same number of elements of every chunk
__host__ __device__ constexpr int d2_chunk(int HG, int OS) { return ((HG * 128 > OS * 256 ? HG * 128 : OS * 256) + D2_T - 1) / D2_T * D2_T; }

struct d2_dims {
    int Din, H, Dout;                            // W1 [H][Din], W2 [Dout][H]
    int KS;                                      // k-steps of 16 columns
    int HG, NP, OS, CH;                          // the variant: hidden slices per pass, passes, output tiles (all computed; the
};                                               // image holds zeros beyond H and Dout), elements per chunk

// The variant of (Din, H, Dout): 11 slices in one pass with 6 output tiles where that holds everything; else passes of 8 slices
// with 8 output tiles -- or, with `mid`, with 6 where Dout <= 192 (a quarter fewer layer-2 products).  The widths are the caller's check.
void d2_make_dims(int Din, int H, int Dout, bool mid, d2_dims& o);
// 16-byte elements of the chunks (everything in front of the biases)
static __host__ __device__ inline uint32_t d2_chunk_elems(const d2_dims& d) {
    return (uint32_t)(d.NP * (d.KS + d.HG)) * (uint32_t)d.CH;
}
size_t d2_image_bytes(const d2_dims& d);
// ONE launch that writes the image (dense2.hip: the layout) from the four Parameters
int d2_prepare(const float* w1, const float* b1, const float* w2, const float* b2, const d2_dims& d, void* img, hipStream_t s);

// An activation is an object: split16(a, bias, w, bh, bl) turns the accumulators of hidden slice w (units 32 w + acc_row(q, h) of the
// lane's row) into layer 2's B operand.  The two stateless ones ignore w; one that needs the row and the units it holds
// (mixer_channel_train.hip: the dropout mask) carries them as members.
struct act_relu {
    static __device__ __forceinline__ void split16(const f32x16& a, const float (&bias)[16], int, bf16x8 (&bh)[2], bf16x8 (&bl)[2]) {
        relu_split16(a, bias, bh, bl);
    }
};
struct act_gelu {
    static __device__ __forceinline__ void split16(const f32x16& a, const float (&bias)[16], int, bf16x8 (&bh)[2], bf16x8 (&bl)[2]) {
        gelu_split16(a, bias, bh, bl);
    }
};

// The body of a kernel of D2_T threads.  HG hidden slices per pass, OSM output tiles; MULTI: more than one pass may be needed
// (layer 2's accumulators then live through the later passes' layer 1).  Lane (r = lane & 31, h = lane >> 5) of wave w works on row
// 32 (4 blockIdx.x + w) + r: x4(c) = columns c .. c + 3 of that row (c % 4 == 0; zeros beyond Din and for a row that is not `valid`),
// put(o, v) takes outputs o .. o + 3 of a valid row, bias added.
template <int HG, int OSM, bool MULTI, class ACT, class SRC, class PUT>
__device__ __forceinline__ void dense2_rows(const d2_dims& d, const uint4* __restrict__ img, const bool valid, const SRC& x4,
                                            const PUT& put, const ACT& act = ACT()) {
    constexpr int CH = d2_chunk(HG, OSM), D2_PF = CH / D2_T;
    static_assert(CH >= HG * 128 && CH >= OSM * 256 && CH % D2_T == 0, "a chunk holds a k-step of W1 and a slice of W2");
    __shared__ uint4 buf[2][CH];
    const int tid = threadIdx.x, lane = tid & 63;
    const int h = lane >> 5;
    // ---- the chunk pipeline: fetch(c) reads chunk c into registers, commit(b) writes it to buffer b behind the current products
    // (every chunk has CH elements and every thread moves D2_PF of them, unconditionally: the registers in between stay registers;
    // behind the last chunk the first one is fetched again and never used)
    const uint32_t nchunks = (uint32_t)(d.NP * (d.KS + HG));
    static_assert(D2_PF == 4 || D2_PF == 6 || D2_PF == 8, "the prefetch registers below");
    uint4 p0, p1, p2, p3, p4, p5, p6, p7;      // (named, not an array: an array indexed inside the lambdas ends up in scratch memory)
    auto fetch = [&](uint32_t c) {
        const uint4* src = img + (c < nchunks ? c : 0u) * (uint32_t)CH + tid;
        p0 = src[0]; p1 = src[D2_T]; p2 = src[2 * D2_T]; p3 = src[3 * D2_T];
        if constexpr (D2_PF >= 6) { p4 = src[4 * D2_T]; p5 = src[5 * D2_T]; }
        if constexpr (D2_PF == 8) { p6 = src[6 * D2_T]; p7 = src[7 * D2_T]; }
    };
    auto commit = [&](int b) {
        uint4* dst = buf[b] + tid;
        dst[0] = p0; dst[D2_T] = p1; dst[2 * D2_T] = p2; dst[3 * D2_T] = p3;
        if constexpr (D2_PF >= 6) { dst[4 * D2_T] = p4; dst[5 * D2_T] = p5; }
        if constexpr (D2_PF == 8) { dst[6 * D2_T] = p6; dst[7 * D2_T] = p7; }
        __syncthreads();
    };
    const float* bias = reinterpret_cast<const float*>(img + d2_chunk_elems(d));
    f32x16 y[OSM];
#pragma unroll
    for (int t = 0; t < OSM; ++t)
#pragma unroll
        for (int q = 0; q < 16; ++q) y[t][q] = 0.0f;
    uint32_t chunk = 0;
    int cur = 0;
    fetch(0);
    commit(0);
    for (int p = 0; p < (MULTI ? d.NP : 1); ++p) {
        const int w0 = p * HG;
        f32x16 acc[HG];
#pragma unroll
        for (int wl = 0; wl < HG; ++wl)
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[wl][q] = 0.0f;
        // ---- layer 1: H^T[32 w ..][rows] += W1[32 w .., 16 s ..] . X^T, k-step by k-step, all slices of the pass
        float4 xa = x4(8 * h), xb = x4(8 * h + 4);
        for (int s = 0; s < d.KS; ++s) {
            fetch(chunk + 1);
            bf16x8 bxh, bxl;
            split8(xa, xb, bxh, bxl);
            xa = x4(16 * (s + 1) + 8 * h);                                      // (beyond Din: zeros)
            xb = x4(16 * (s + 1) + 8 * h + 4);
            const bf16x8* W = reinterpret_cast<const bf16x8*>(buf[cur]) + lane;
            // all operands of the k-step first (one LDS round trip, not one per product), then the products term-major: the
            // three products of one accumulator lie HG instructions apart
            bf16x8 ah[HG], al[HG];
#pragma unroll
            for (int wl = 0; wl < HG; ++wl) {
                ah[wl] = W[(wl * 2) * 64];
                al[wl] = W[(wl * 2 + 1) * 64];
            }
            __builtin_amdgcn_sched_group_barrier(0x100, 2 * HG, 0);             // (the scheduler otherwise waits on every read in turn)
            __builtin_amdgcn_sched_group_barrier(0x008, 3 * HG, 0);
            mm3(ah, al, bxh, bxl, acc);
            commit(cur ^ 1);
            cur ^= 1;
            ++chunk;
        }
        // ---- layer 2, slice by slice: bias, activation and split of the slice's accumulators (ACT::split16) are the B operand;
        // every output tile takes its share
#pragma unroll
        for (int wl = 0; wl < HG; ++wl) {
            {
                fetch(chunk + 1);
                float bv[16];                                                   // b1 in accumulator order: acc_row(4 q4 + j, h) = 8 q4 + 4 h + j
#pragma unroll
                for (int q4 = 0; q4 < 4; ++q4) {
                    const float4 bb = *reinterpret_cast<const float4*>(bias + 32 * (w0 + wl) + 8 * q4 + 4 * h);
                    bv[4 * q4] = bb.x; bv[4 * q4 + 1] = bb.y; bv[4 * q4 + 2] = bb.z; bv[4 * q4 + 3] = bb.w;
                }
                bf16x8 bhh[2], bhl[2];
                act.split16(acc[wl], bv, w0 + wl, bhh, bhl);
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
    }
    // ---- y[t][4 i .. 4 i + 3] = outputs 32 t + 8 i + 4 h + (0..3) of row r
    if (valid) {
        const float* b2 = bias + 32 * d.NP * HG;
#pragma unroll
        for (int t = 0; t < OSM; ++t) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int o = 32 * t + 8 * i + 4 * h;
                if (o < d.Dout) {
                    const float4 c = *reinterpret_cast<const float4*>(b2 + o);
                    put(o, make_float4(y[t][4 * i] + c.x, y[t][4 * i + 1] + c.y, y[t][4 * i + 2] + c.z, y[t][4 * i + 3] + c.w));
                }
            }
        }
    }
}

}  // namespace tpnet
