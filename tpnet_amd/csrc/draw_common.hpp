// What the two device samplers share (sampler.hip: neighbours, negsampler.hip: negative edges): the order-preserving time key, the
// 256-thread workgroup scan and the counter-based generator (also the dropout draws of mixer_token_train.hip).  One copy of each.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tpnet {

// order-preserving map of an IEEE double onto uint64
__device__ __forceinline__ uint64_t time_key(double t) {
    const uint64_t b = (uint64_t)__double_as_longlong(t);
    return (b & 0x8000000000000000ull) ? ~b : (b | 0x8000000000000000ull);
}

// inclusive scan of one value per thread over a 256-thread workgroup; sh = 4 values of LDS; total = the workgroup's sum
template <class T>
__device__ __forceinline__ T wg_scan256(T v, T* sh, T& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int off = 1; off < 64; off <<= 1) {
        const T u = __shfl_up(v, off, 64);
        if (lane >= off) v += u;
    }
    if (lane == 63) sh[wave] = v;
    __syncthreads();
    T base = 0;
    for (int w = 0; w < wave; ++w) base += sh[w];
    total = (sh[0] + sh[1]) + (sh[2] + sh[3]);
    __syncthreads();
    return base + v;
}

// Philox4x32-10 (Salmon et al., SC'11): counter-based, so a draw depends on (key, counter) alone, never on the launch geometry
__device__ __forceinline__ uint32_t philox_word(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                                int word) {
    for (int r = 0; r < 10; ++r) {
        const uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
        const uint32_t h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
        c0 = h1 ^ c1 ^ k0;
        c1 = l1;
        c2 = h0 ^ c3 ^ k1;
        c3 = l0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return word == 0 ? c0 : word == 1 ? c1 : word == 2 ? c2 : c3;
}

// all four words of the block: .x .. .w = philox_word(..., 0 .. 3)
__device__ __forceinline__ uint4 philox_block(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
    for (int r = 0; r < 10; ++r) {
        const uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
        const uint32_t h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
        c0 = h1 ^ c1 ^ k0;
        c1 = l1;
        c2 = h0 ^ c3 ^ k1;
        c3 = l0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return make_uint4(c0, c1, c2, c3);
}

// a dropout rate the training kernels serve, and its threshold floor(p 2^32): a draw (one 32-bit word) keeps where word >= threshold;
// 0 = no dropout, nothing is drawn
static inline bool drop_rate(float p) { return p >= 0.0f && p < 1.0f; }         // (a NaN fails both)
static inline uint32_t drop_threshold(float p) { return (uint32_t)((double)p * 4294967296.0); }

}  // namespace tpnet
