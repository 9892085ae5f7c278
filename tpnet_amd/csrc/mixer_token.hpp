// What the token-mixing kernels share (mixer.hip: k_mixer_token; mixer_token_train.hip: forward with dropout and backward): the size
// limit, the exact GELU and the dropout draws of a (node, channel) column.  One copy of each.
#pragma once
#include "draw_common.hpp"

namespace tpnet {

static constexpr int MX_KMAX = 32;               // tokens and token-hidden units the token kernels serve

__device__ __forceinline__ float gelu_erf(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678118654752440f)); }

// d gelu_erf / dx = Phi(x) + x exp(-x^2 / 2) / sqrt(2 pi)
__device__ __forceinline__ float gelu_erf_grad(float x) {
    return 0.5f * (1.0f + erff(x * 0.70710678118654752440f)) + x * expf(-0.5f * x * x) * 0.39894228040143267794f;
}

static constexpr uint32_t MX_DROP_TAG = 0x4D58544Bu;   // c3 of every dropout draw of the token kernels ("MXTK")

// The keep bits of column `col` (= node * C + channel): bit i = draw i >= thr, i < ndraws <= 64.  Draw 4 b + w is word w of the
// Philox4x32-10 block with counter (col low, col high, b, MX_DROP_TAG) and key (k0, k1): draws 0 .. Kh - 1 are the dropout behind
// the GELU, draws Kh .. Kh + K - 1 the one behind the second Linear (include/tpnet_hip.h).  Bits >= ndraws are unspecified.
__device__ __forceinline__ uint64_t mx_keep_bits(int64_t col, int ndraws, uint32_t thr, uint32_t k0, uint32_t k1) {
    uint64_t keep = 0;
    for (int b = 0; 4 * b < ndraws; ++b) {
        const uint4 w = philox_block((uint32_t)col, (uint32_t)((uint64_t)col >> 32), (uint32_t)b, MX_DROP_TAG, k0, k1);
        const uint32_t four = (w.x >= thr ? 1u : 0u) | (w.y >= thr ? 2u : 0u) | (w.z >= thr ? 4u : 0u) | (w.w >= thr ? 8u : 0u);
        keep |= (uint64_t)four << (4 * b);
    }
    return keep;
}

}  // namespace tpnet
