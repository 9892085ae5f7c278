// The fp32-class arithmetic of the matrix-core kernels, once (mlp.hip, decoder.hip, feature_mfma.hip, encoder_mfma.hip;
// through mlp_wave_tile.hpp mlp_x3.hip and mlp_rows.hip; through mlp_wgrad.hpp mlp_bwd.hip and mlp_rows_bwd.hip; through dense2.hpp
// encoder_input.hip and mixer.hip).  Only the arithmetic atoms live here: every kernel
// keeps its own mapping, staging, pipelining and scheduling barriers.
//
// SPLIT OPERANDS.  Every f32 operand is a sum of bf16 pieces, leading piece first: x = p[0] + p[1] (+ p[2]), p[0] = bf16(x),
// p[1] = bf16(x - p[0]), p[2] = bf16(x - p[0] - p[1]).  Two pieces carry 16 bits of significand, three carry 24.
// TERM ORDER.  A product of two-piece operands (hi = p[0], lo = p[1]) is issued as lo*hi + hi*lo + hi*hi, the small terms
// first, into an fp32 accumulator (lo*lo, 2^-16 of the result, is dropped: the fp32 class, <= 2e-5 of the output scale against
// the torch layers, exact on small integers).  Three-piece operands take six products (mm6 below; 2^-24 is dropped).  The order
// is part of the results' bits; in the term-major forms so is the order in which the accumulators take turns (and it is a
// measured speed property: the products of one accumulation chain lie N instructions apart, a chain's next product waits for
// its previous one).
// ACCUMULATOR LAYOUT of v_mfma_f32_32x32x16_bf16: register q of lane (r = lane & 31, h = lane >> 5) holds row acc_row(q, h) of
// column r.  With layer 1 computed transposed (H^T = W1 . X^T) a lane's 16 registers are 16 hidden units of ITS row, which is
// the B operand shape of layer 2: k-position 8 s2 + j of lane half h <-> register q = 8 s2 + j <-> hidden unit acc_row(q, h).
#pragma once
#include <hip/hip_runtime.h>

namespace tpnet {

typedef __attribute__((__vector_size__(8 * sizeof(__bf16)))) __bf16 bf16x8;
typedef __attribute__((__vector_size__(4 * sizeof(__bf16)))) __bf16 bf16x4;
typedef __attribute__((__vector_size__(16 * sizeof(float)))) float f32x16;
typedef __attribute__((__vector_size__(4 * sizeof(float)))) float f32x4;

// row of a 32x32 accumulator tile that register q of lane half h holds (the kernels, the bias staging and the image builders)
__host__ __device__ constexpr int acc_row(int q, int h) { return (q & 3) + 8 * (q >> 2) + 4 * h; }

// The weight image of self.mlp = Linear(64, 256) -> ReLU -> Linear(256, 64) in split pieces, byte offsets: hi / lo planes of W1
// and W2 (2 048 16-byte elements each, every element the operand of one lane of one matrix instruction), then b1 and b2.  Two
// element orders use these offsets, each documented where the image is built: k_mlp64_x3's LDS image (32x32x16 operands,
// MlpRowsGeo<3> of mlp_wave_tile.hpp, which asserts the equality) and tpnet_mlp::wimg (16x16x32 operands, k_mlp_image in encoder_mfma.hip).
static constexpr int IMG_W1H = 0, IMG_W1L = 32768, IMG_W2H = 65536, IMG_W2L = 98304, IMG_B1 = 131072, IMG_B2 = IMG_B1 + 1024;
static constexpr int IMG_BYTES = IMG_B2 + 256;                              // 132 352

template <int N>
struct SplitOp {
    bf16x8 p[N];                          // p[0] = the leading bf16 piece of 8 values, p[1], p[2] = the pieces below
};

// one float -> N bf16 pieces (SPLIT OPERANDS above)
template <int N>
__device__ __forceinline__ void split1(float x, __bf16 (&p)[N]) {
#pragma unroll
    for (int t = 0; t < N; ++t) {
        p[t] = (__bf16)x;
        if (t + 1 < N) x = x - (float)p[t];
    }
}
// E floats -> N bf16 pieces each (V = bf16x8 or bf16x4)
template <int N, class V, int E>
__device__ __forceinline__ void split(const float (&v)[E], V (&p)[N]) {
    static_assert(sizeof(V) == E * sizeof(__bf16), "split: one vector element per float");
#pragma unroll
    for (int j = 0; j < E; ++j) {
        __bf16 b[N];
        split1(v[j], b);
#pragma unroll
        for (int t = 0; t < N; ++t) p[t][j] = b[t];
    }
}
template <int N>
__device__ __forceinline__ void split8(const float (&v)[8], SplitOp<N>& o) { split(v, o.p); }
// the two-piece forms: an array, two float4, 8 consecutive floats in memory (16-byte aligned)
__device__ __forceinline__ void split8(const float (&v)[8], bf16x8& hi, bf16x8& lo) {
    bf16x8 p[2];
    split(v, p);
    hi = p[0];
    lo = p[1];
}
__device__ __forceinline__ void split8(const float4 a, const float4 b, bf16x8& hi, bf16x8& lo) {
    const float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    split8(v, hi, lo);
}
__device__ __forceinline__ void load_split8(const float* __restrict__ x, bf16x8& hi, bf16x8& lo) {
    split8(*reinterpret_cast<const float4*>(x), *reinterpret_cast<const float4*>(x + 4), hi, lo);
}

// 8 floats -> bf16, one piece (the opt-in bf16 class)
__device__ __forceinline__ bf16x8 cvt8(const float (&v)[8]) {
    bf16x8 b;
#pragma unroll
    for (int j = 0; j < 8; ++j) b[j] = (__bf16)v[j];
    return b;
}
__device__ __forceinline__ bf16x8 load_cvt8(const float* __restrict__ x) {
    const float4 a = *reinterpret_cast<const float4*>(x), b = *reinterpret_cast<const float4*>(x + 4);
    const float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    return cvt8(v);
}

// one matrix instruction, chosen by the accumulator: f32x16 = 32x32x16 (16-deep step), f32x4 = 16x16x32 (32-deep step)
__device__ __forceinline__ f32x16 mfma(const bf16x8 a, const bf16x8 b, const f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ f32x4 mfma(const bf16x8 a, const bf16x8 b, const f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

// c += A B over one step of two-piece operands (TERM ORDER above)
template <class ACC>
__device__ __forceinline__ ACC mm3(const bf16x8 ah, const bf16x8 al, const bf16x8 bh, const bf16x8 bl, ACC c) {
    c = mfma(al, bh, c);
    c = mfma(ah, bl, c);
    return mfma(ah, bh, c);
}
// ... term-major over N independent accumulators that share the B operand: c[t] += A[t] B
template <class ACC, int N>
__device__ __forceinline__ void mm3(const bf16x8 (&ah)[N], const bf16x8 (&al)[N], const bf16x8 bh, const bf16x8 bl, ACC (&c)[N]) {
#pragma unroll
    for (int t = 0; t < N; ++t) c[t] = mfma(al[t], bh, c[t]);
#pragma unroll
    for (int t = 0; t < N; ++t) c[t] = mfma(ah[t], bl, c[t]);
#pragma unroll
    for (int t = 0; t < N; ++t) c[t] = mfma(ah[t], bh, c[t]);
}

// c += A B^T over one 32-deep step of three-piece operands, the small terms first
__device__ __forceinline__ f32x4 mm6(const SplitOp<3>& a, const SplitOp<3>& b, f32x4 c) {
    c = mfma(a.p[2], b.p[0], c);
    c = mfma(a.p[0], b.p[2], c);
    c = mfma(a.p[1], b.p[1], c);
    c = mfma(a.p[1], b.p[0], c);
    c = mfma(a.p[0], b.p[1], c);
    return mfma(a.p[0], b.p[0], c);
}
// ... cw += A A^T, ca += A B^T: the two accumulation chains take turns in the matrix pipe
__device__ __forceinline__ void mm6x2(const SplitOp<3>& a, const SplitOp<3>& b, f32x4& cw, f32x4& ca) {
    constexpr int TA[6] = {2, 0, 1, 1, 0, 0}, TB[6] = {0, 2, 1, 0, 1, 0};      // mm6's terms
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        cw = mfma(a.p[TA[i]], a.p[TB[i]], cw);
        ca = mfma(a.p[TA[i]], b.p[TB[i]], ca);
    }
}

// layer 1's accumulator tile -> layer 2's B operand: + bias (in accumulator order), ReLU, two-piece split; piece [s2] is the B
// operand of layer 2's k-step s2 (ACCUMULATOR LAYOUT above)
__device__ __forceinline__ void relu_split16(const f32x16& a, const float (&bias)[16], bf16x8 (&bh)[2], bf16x8 (&bl)[2]) {
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
        float x[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            x[j] = a[8 * s2 + j] + bias[8 * s2 + j];
            x[j] = x[j] > 0.0f ? x[j] : 0.0f;
        }
        split8(x, bh[s2], bl[s2]);
    }
}
// ... with the exact GELU x Phi(x) = 0.5 x (1 + erf(x / sqrt 2)) in place of the ReLU (torch.nn.GELU(approximate='none'))
__device__ __forceinline__ void gelu_split16(const f32x16& a, const float (&bias)[16], bf16x8 (&bh)[2], bf16x8 (&bl)[2]) {
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
        float x[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            x[j] = a[8 * s2 + j] + bias[8 * s2 + j];
            x[j] = 0.5f * x[j] * (1.0f + erff(x[j] * 0.70710678118654752440f));
        }
        split8(x, bh[s2], bl[s2]);
    }
}

}  // namespace tpnet
