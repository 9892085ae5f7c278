// One MLP-Mixer layer (models/TPNet.py:371-416, dropout as identity) in two launches, forward only:
//   k_mixer_token    x [n_nodes][K][C] -> t = x + W2 . gelu(W1 . LN_K(x[node, :, c]) + b1) + b2 for every (node, channel) column of K
//                    tokens.  0.3 % of the layer's products, memory-bound: plain fp32 on the vector ALU, one thread per column,
//                    consecutive threads on consecutive channels (every one of the K loads and stores coalesced), the K x Kh weights
//                    uniform across the wave (scalar loads).
//   k_mixer_channel  t [n_rows][C] -> out = t + W2 . gelu(W1 . LN_C(t[row]) + b1) + b2 on the matrix cores: dense2.hpp's two layers
//                    (fp32 class of mfma_split.hpp) with the LayerNorm of the lane's row as the row source -- the normalised row is
//                    never written -- GELU as the activation and the residual in the epilogue.  C <= 256, hidden width <= 1024:
//                    up to 352 hidden units in one pass of 11 slices; beyond, passes of 8 slices with 6 output tiles (C <= 192: the
//                    reference's 172 -> 688 -> 172 is 3 passes) or 8.
// Both LayerNorms: biased variance from the deviations of a first-pass mean m0, corrected by the deviations' own mean
// (mean = m0 + dl, x - mean = (x - m0) - dl, var = sum (x - m0)^2 / n - dl^2): a row of mean >> spread loses nothing, a constant row
// normalises to beta exactly as torch's does.
#include "mixer_channel.hpp"                     // the row statistics and size checks: shared with mixer_channel_train.hip
#include "mixer_token.hpp"                       // MX_KMAX, gelu_erf: shared with mixer_token_train.hip

namespace tpnet {

// KC, KHC: compile-time K and Kh (20 and 10: the reference's num_neighbors), or 0: the caller's, up to MX_KMAX -- the loops over
// the tokens are then unrolled to MX_KMAX and guarded by a wave-uniform test, so that the per-thread arrays stay registers, and the
// loop over the hidden units is a loop
template <int KC, int KHC>
__global__ __launch_bounds__(256) void k_mixer_token(const float* __restrict__ x, int64_t total, int Kr, int Khr, int C,
                                                     const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                     const float* __restrict__ w1, const float* __restrict__ b1,
                                                     const float* __restrict__ w2, const float* __restrict__ b2,
                                                     float* __restrict__ out) {
    constexpr int KM = KC ? KC : MX_KMAX;
    const int K = KC ? KC : Kr, Kh = KHC ? KHC : Khr;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;                  // (node, channel)
    if (i >= total) return;
    const int64_t node = i / C;
    const int64_t base = node * K * C + (i - node * C);
    float v[KM], ln[KM], o[KM];
    float s = 0.0f;
#pragma unroll
    for (int k = 0; k < KM; ++k) {
        v[k] = 0.0f;
        if (k < K) {
            v[k] = x[base + (int64_t)k * C];
            s += v[k];
        }
    }
    const float m0 = s / (float)K;
    float sd = 0.0f, sq = 0.0f;
#pragma unroll
    for (int k = 0; k < KM; ++k) {
        if (k < K) {
            const float dv = v[k] - m0;
            sd += dv;
            sq += dv * dv;
        }
    }
    const float dl = sd / (float)K;
    const float rstd = 1.0f / sqrtf(fmaxf(sq / (float)K - dl * dl, 0.0f) + eps);
#pragma unroll
    for (int k = 0; k < KM; ++k) {
        ln[k] = 0.0f;
        o[k] = 0.0f;
        if (k < K) ln[k] = ((v[k] - m0) - dl) * rstd * gamma[k] + beta[k];
    }
    // hidden unit by hidden unit: its value, then its share of every output token
    for (int j = 0; j < Kh; ++j) {
        float a = 0.0f;
#pragma unroll
        for (int k = 0; k < KM; ++k)
            if (k < K) a += w1[j * K + k] * ln[k];
        const float hj = gelu_erf(a + b1[j]);
#pragma unroll
        for (int k = 0; k < KM; ++k)
            if (k < K) o[k] += w2[k * Kh + j] * hj;
    }
#pragma unroll
    for (int k = 0; k < KM; ++k)
        if (k < K) out[base + (int64_t)k * C] = (o[k] + b2[k]) + v[k];
}

// HG hidden slices per pass, OSM output tiles, MULTI: dense2_rows'
template <int HG, int OSM, bool MULTI>
__global__ __launch_bounds__(D2_T) void k_mixer_channel(const float* __restrict__ x, int64_t n, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, float eps, const d2_dims d,
                                                        const uint4* __restrict__ img, float* __restrict__ out) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int64_t row = ((int64_t)blockIdx.x * 4 + wave) * 32 + r;
    const bool valid = row < n;
    const int C = d.Din;
    const float* xr = x + (valid ? row : 0) * C;
    mx_ln_row x4{xr, gamma, beta, C, valid};
    x4.stats(h, eps);
    float* yo = out + row * C;
    dense2_rows<HG, OSM, MULTI, act_gelu>(d, img, valid, x4, [&](int o, const float4 v) {
        const float4 a = *reinterpret_cast<const float4*>(xr + o);
        *reinterpret_cast<float4*>(yo + o) = make_float4(v.x + a.x, v.y + a.y, v.z + a.z, v.w + a.w);
    });
}

}  // namespace tpnet

extern "C" int tpnet_mixer_supported(int32_t K, int32_t Kh, int32_t C, int32_t Ch) {
    tpnet::d2_dims d;
    return K >= 2 && K <= tpnet::MX_KMAX && Kh >= 1 && Kh <= tpnet::MX_KMAX && tpnet::mx_channel_dims(C, Ch, d) ? 1 : 0;
}

extern "C" size_t tpnet_mixer_channel_image_bytes(int32_t C, int32_t Ch) {
    tpnet::d2_dims d;
    return tpnet::mx_channel_dims(C, Ch, d) ? tpnet::d2_image_bytes(d) : 0;
}

extern "C" int tpnet_mixer_channel_prepare(const float* w1, const float* b1, const float* w2, const float* b2, int32_t C, int32_t Ch,
                                           void* img, void* stream) {
    tpnet::d2_dims d;
    if (!w1 || !b1 || !w2 || !b2 || !img || (reinterpret_cast<uintptr_t>(img) & 15) || !tpnet::mx_channel_dims(C, Ch, d))
        return TPNET_ERR_BAD_ARG;
    return tpnet::d2_prepare(w1, b1, w2, b2, d, img, (hipStream_t)stream);
}

extern "C" int tpnet_mixer_token(const float* x, int64_t n_nodes, int32_t K, int32_t C, const float* gamma, const float* beta, float eps,
                                 const float* w1, const float* b1, int32_t Kh, const float* w2, const float* b2, float* out,
                                 void* stream) {
    if (!x || !gamma || !beta || !w1 || !b1 || !w2 || !b2 || !out || out == x) return TPNET_ERR_BAD_ARG;
    if (n_nodes < 0 || K < 2 || K > tpnet::MX_KMAX || Kh < 1 || Kh > tpnet::MX_KMAX || C < 4 || (C & 3)) return TPNET_ERR_BAD_ARG;
    if (n_nodes > (1ll << 31) / K || n_nodes * C > (1ll << 38)) return TPNET_ERR_BAD_ARG;
    if (!tpnet::aligned16({x, out}) || ((reinterpret_cast<uintptr_t>(gamma) | reinterpret_cast<uintptr_t>(beta) |
                                            reinterpret_cast<uintptr_t>(w1) | reinterpret_cast<uintptr_t>(b1) |
                                            reinterpret_cast<uintptr_t>(w2) | reinterpret_cast<uintptr_t>(b2)) & 3))
        return TPNET_ERR_BAD_ARG;
    const int64_t total = n_nodes * C;
    if (total == 0) return TPNET_OK;
    const auto kernel = K == 20 && Kh == 10 ? tpnet::k_mixer_token<20, 10> : tpnet::k_mixer_token<0, 0>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, total, (int)K, (int)Kh,
                       (int)C, gamma, beta, eps, w1, b1, w2, b2, out);
    TPNET_HIP_TRY(hipGetLastError());
    return TPNET_OK;
}

extern "C" int tpnet_mixer_channel(const float* x, int64_t n_rows, int32_t C, int32_t Ch, const float* gamma, const float* beta,
                                   float eps, const void* img, float* out, void* stream) {
    tpnet::d2_dims d;
    if (!x || !gamma || !beta || !img || !out || out == x) return TPNET_ERR_BAD_ARG;
    if (n_rows < 0 || n_rows > (1ll << 31) || !tpnet::mx_channel_dims(C, Ch, d)) return TPNET_ERR_BAD_ARG;
    if (!tpnet::aligned16({x, gamma, beta, img, out})) return TPNET_ERR_BAD_ARG;
    if (n_rows == 0) return TPNET_OK;
    const auto kernel = d.HG == tpnet::D2_HG   ? tpnet::k_mixer_channel<tpnet::D2_HG, tpnet::D2_OS, false>
                        : d.OS == tpnet::D2_OS ? tpnet::k_mixer_channel<tpnet::D2_HG_WIDE, tpnet::D2_OS, true>
                                               : tpnet::k_mixer_channel<tpnet::D2_HG_WIDE, tpnet::D2_OS_WIDE, true>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)((n_rows + tpnet::D2_ROWS - 1) / tpnet::D2_ROWS)), dim3(tpnet::D2_T), 0,
                       (hipStream_t)stream, x, n_rows, gamma, beta, eps, d, reinterpret_cast<const uint4*>(img), out);
    TPNET_HIP_TRY(hipGetLastError());
    return TPNET_OK;
}
