// What the channel-mixing kernels share (mixer.hip: k_mixer_channel; mixer_channel_train.hip: forward with dropout and backward): the
// served sizes, the LayerNorm statistics of a lane pair's row and the dropout draws of a row.  One copy of each.
#pragma once
#include "dense2.hpp"
#include "mixer_token.hpp"                       // gelu_erf, gelu_erf_grad, philox_block

namespace tpnet {

static inline bool mx_channel_dims(int32_t C, int32_t Ch, d2_dims& d) {
    if (C < 4 || C > 256 || (C & 3) || Ch < 1 || Ch > 1024) return false;
    d2_make_dims(C, Ch, C, true, d);
    return true;
}

// The first-pass mean m0, the deviations' own mean dl and 1 / sqrt(var + eps) of row xr [C] (mixer.hip's rule): the two lanes of a row
// (h = 0, 1) take every other float4 and add their sums (a + b = b + a: both hold the same bits).  Every lane of the wave calls it;
// a row that is not `valid` is not read and gets the statistics of a zero row.
__device__ __forceinline__ void mx_row_stats(const float* __restrict__ xr, int C, bool valid, int h, float eps, float& m0, float& dl,
                                             float& rstd) {
    float s = 0.0f;
    if (valid) {
        for (int c = 4 * h; c < C; c += 8) {
            const float4 a = *reinterpret_cast<const float4*>(xr + c);
            s += (a.x + a.y) + (a.z + a.w);
        }
    }
    s += __shfl_xor(s, 32);
    m0 = s / (float)C;
    float sd = 0.0f, sq = 0.0f;
    if (valid) {
        for (int c = 4 * h; c < C; c += 8) {
            const float4 a = *reinterpret_cast<const float4*>(xr + c);
            const float d0 = a.x - m0, d1 = a.y - m0, d2 = a.z - m0, d3 = a.w - m0;
            sd += (d0 + d1) + (d2 + d3);
            sq += (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
        }
    }
    sd += __shfl_xor(sd, 32);
    sq += __shfl_xor(sq, 32);
    dl = sd / (float)C;
    rstd = 1.0f / sqrtf(fmaxf(sq / (float)C - dl * dl, 0.0f) + eps);
}

// The LayerNorm of a lane's row as dense2_rows' row source: columns c .. c + 3 of xh gamma + beta (zeros beyond C and for a row that
// is not valid).  stats() first, by every lane of the wave.
struct mx_ln_row {
    const float *xr, *gamma, *beta;
    int C;
    bool valid;
    float m0, dl, rstd;
    __device__ __forceinline__ void stats(int h, float eps) { mx_row_stats(xr, C, valid, h, eps, m0, dl, rstd); }
    __device__ __forceinline__ float xh(float v) const { return ((v - m0) - dl) * rstd; }
    __device__ __forceinline__ float4 operator()(int c) const {
        if (!valid || c >= C) return make_float4(0.f, 0.f, 0.f, 0.f);
        const float4 a = *reinterpret_cast<const float4*>(xr + c), g = *reinterpret_cast<const float4*>(gamma + c),
                     b = *reinterpret_cast<const float4*>(beta + c);
        return make_float4(xh(a.x) * g.x + b.x, xh(a.y) * g.y + b.y, xh(a.z) * g.z + b.z, xh(a.w) * g.w + b.w);
    }
};

static constexpr uint32_t MXC_DROP_TAG = 0x4D584348u;  // c3 of every dropout draw of the channel kernels ("MXCH")

// The keep bits of block b of row `row`: bit w = word w of the Philox4x32-10 block with counter (row low, row high, b, MXC_DROP_TAG)
// and key (k0, k1) >= thr.  Blocks 0 .. ceil(Ch / 4) - 1 are the dropout behind the GELU (hidden units 4 b .. 4 b + 3), the next C / 4
// the one behind the second Linear (include/tpnet_hip.h).  thr = 0: nothing is drawn, everything is kept.
__device__ __forceinline__ uint32_t mxc_keep4(int64_t row, uint32_t b, uint32_t thr, uint32_t k0, uint32_t k1) {
    if (thr == 0) return 15u;
    const uint4 w = philox_block((uint32_t)row, (uint32_t)((uint64_t)row >> 32), b, MXC_DROP_TAG, k0, k1);
    return (w.x >= thr ? 1u : 0u) | (w.y >= thr ? 2u : 0u) | (w.z >= thr ? 4u : 0u) | (w.w >= thr ? 8u : 0u);
}

}  // namespace tpnet
