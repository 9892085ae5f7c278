// The token-mixing half of an MLP-Mixer layer (models/TPNet.py:371-416) in a TRAINING step: one launch forward, one backward.
// Per (node, channel) column v[0 .. K) of x [n_nodes][K][C], with s = 1 / (1 - p) and the keep masks m1 [Kh], m2 [K] of the two
// dropouts of FeedForwardNet (behind the GELU, behind the second Linear):
//   xh[k] = ((v[k] - m0) - dl) rstd        ln[k] = xh[k] gamma[k] + beta[k]            (the LayerNorm rule of mixer.hip)
//   a[j]  = sum_k w1[j][k] ln[k] + b1[j]   h[j]  = gelu(a[j]) m1[j] s
//   o[k]  = sum_j w2[k][j] h[j] + b2[k]    y[k]  = o[k] m2[k] s + v[k]
//   k_mixer_token_train  the forward: k_mixer_token's geometry (one thread per column, consecutive threads on consecutive channels,
//                        the weights uniform across the wave) and its arithmetic -- at p = 0 nothing is drawn and the output has
//                        the bits of k_mixer_token's.
//   k_mixer_token_bwd    from gy: gx (optional) and the six parameter gradients.  Nothing but x is saved by the caller: the column's
//                        forward is recomputed from x and the key.
//     go[k] = gy[k] m2[k] s                  gb2[k] += go[k]    gw2[k][j] += go[k] h[j]
//     gh[j] = sum_k w2[k][j] go[k]           ga[j] = gh[j] m1[j] s gelu'(a[j])
//     gb1[j] += ga[j]                        gw1[j][k] += ga[j] ln[k]
//     gln[k] = sum_j w1[j][k] ga[j]          gbeta[k] += gln[k]  ggamma[k] += gln[k] xh[k]
//     gxh[k] = gln[k] gamma[k]               gx[k] = rstd (gxh[k] - mean(gxh) - xh[k] mean(gxh xh)) + gy[k]
//   k_mixer_token_masks  m1 / m2 as bytes, for whoever wants to evaluate the same dropout elsewhere (the tests).
// DRAWS.  mixer_token.hpp's mx_keep_bits: Philox4x32-10 keyed by the call's key, counter = (column index, block, tag); a draw depends on
// (key, column, slot) alone, so the forward, the backward and the mask kernel agree whatever their launch geometry.
// PARAMETER SUMS (k_mixer_token_bwd).  A workgroup walks batches of `cols` columns (256; 128 where a batch's staging would not fit
// the LDS: 4 K + 2 Kh > 159) in a grid-stride loop.  Per batch, phase 1: thread = column as in the forward; it leaves
// go | h | ga | ln | gln | xh | 1.0 of its column in an LDS row of RS = 4 K + 2 Kh + 1 floats (odd: the 32 lanes of a store hit 32
// banks).  Phase 2: thread = output; every one of the P = 3 K + 2 K Kh + Kh sums is sum_columns row[ia] row[ib] for two slots of
// the row (the three bias-like sums take the 1.0), added in column order into a register that lives over all batches of the
// workgroup: lanes with consecutive outputs read consecutive slots of ONE row -- distinct banks or a broadcast.  470 outputs at
// K = 20, Kh = 10: two per thread; the generic instantiation carries up to 9 (2 176 at K = Kh = 32).  About as many multiply-adds
// per column as the forward's two dot products (2 P / 256 per thread and column), no atomics, no shuffles; the matrix cores were
// not used because the sums must be exact fp32 in a fixed order and P x 256 products per batch are few.
// Every workgroup writes ONE partial (ggamma | gbeta | gw1 | gb1 | gw2 | gb2, unpadded); the caller adds the partials in a fixed
// order: run-to-run identical bits.
#include "tpnet_common.h"
#include "mixer_token.hpp"

namespace tpnet {

// the column's LayerNorm statistics from its values (k_mixer_token's two passes)
template <int KM>
__device__ __forceinline__ void mx_column_stats(const float (&v)[KM], int K, float eps, float& m0, float& dl, float& rstd) {
    float s = 0.0f;
#pragma unroll
    for (int k = 0; k < KM; ++k)
        if (k < K) s += v[k];
    m0 = s / (float)K;
    float sd = 0.0f, sq = 0.0f;
#pragma unroll
    for (int k = 0; k < KM; ++k) {
        if (k < K) {
            const float dv = v[k] - m0;
            sd += dv;
            sq += dv * dv;
        }
    }
    dl = sd / (float)K;
    rstd = 1.0f / sqrtf(fmaxf(sq / (float)K - dl * dl, 0.0f) + eps);
}

// KC, KHC: k_mixer_token's.  thr = floor(p 2^32): 0 = no dropout, nothing drawn; s = 1 / (1 - p)
template <int KC, int KHC>
__global__ __launch_bounds__(256) void k_mixer_token_train(const float* __restrict__ x, int64_t total, int Kr, int Khr, int C,
                                                           const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                           const float* __restrict__ w1, const float* __restrict__ b1,
                                                           const float* __restrict__ w2, const float* __restrict__ b2, float s,
                                                           uint32_t thr, uint32_t k0, uint32_t k1, float* __restrict__ out) {
    constexpr int KM = KC ? KC : MX_KMAX;
    const int K = KC ? KC : Kr, Kh = KHC ? KHC : Khr;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;                  // (node, channel)
    if (i >= total) return;
    const int64_t node = i / C;
    const int64_t base = node * K * C + (i - node * C);
    const uint64_t keep = thr ? mx_keep_bits(i, Kh + K, thr, k0, k1) : ~0ull;
    float v[KM], ln[KM], o[KM];
#pragma unroll
    for (int k = 0; k < KM; ++k) {
        v[k] = 0.0f;
        if (k < K) v[k] = x[base + (int64_t)k * C];
    }
    float m0, dl, rstd;
    mx_column_stats<KM>(v, K, eps, m0, dl, rstd);
#pragma unroll
    for (int k = 0; k < KM; ++k) {
        ln[k] = 0.0f;
        o[k] = 0.0f;
        if (k < K) ln[k] = ((v[k] - m0) - dl) * rstd * gamma[k] + beta[k];
    }
    for (int j = 0; j < Kh; ++j) {
        float a = 0.0f;
#pragma unroll
        for (int k = 0; k < KM; ++k)
            if (k < K) a += w1[j * K + k] * ln[k];
        const float hj = gelu_erf(a + b1[j]) * (((keep >> j) & 1) ? s : 0.0f);
#pragma unroll
        for (int k = 0; k < KM; ++k)
            if (k < K) o[k] += w2[k * Kh + j] * hj;
    }
#pragma unroll
    for (int k = 0; k < KM; ++k)
        if (k < K) out[base + (int64_t)k * C] = (o[k] + b2[k]) * (((keep >> (Kh + k)) & 1) ? s : 0.0f) + v[k];
}

__global__ __launch_bounds__(256) void k_mixer_token_masks(int64_t total, int K, int Kh, int C, uint32_t thr, uint32_t k0, uint32_t k1,
                                                           uint8_t* __restrict__ m1, uint8_t* __restrict__ m2) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int64_t node = i / C;
    const int64_t base = node * K * C + (i - node * C);
    const uint64_t keep = thr ? mx_keep_bits(i, Kh + K, thr, k0, k1) : ~0ull;
    for (int j = 0; j < Kh; ++j) m1[i * Kh + j] = (uint8_t)((keep >> j) & 1);
    for (int k = 0; k < K; ++k) m2[base + (int64_t)k * C] = (uint8_t)((keep >> (Kh + k)) & 1);
}

// floats of a column's LDS row, and the columns of a batch (PARAMETER SUMS)
static constexpr int MXB_LDS_MAX = 160 * 1024;
__host__ __device__ constexpr int mxb_row_floats(int K, int Kh) { return 4 * K + 2 * Kh + 1; }
__host__ __device__ constexpr int mxb_cols(int K, int Kh) { return 256 * mxb_row_floats(K, Kh) * 4 <= MXB_LDS_MAX ? 256 : 128; }
__host__ __device__ constexpr int mxb_partial_floats(int K, int Kh) { return 3 * K + 2 * K * Kh + Kh; }

template <int KC, int KHC>
__global__ __launch_bounds__(256) void k_mixer_token_bwd(const float* __restrict__ x, const float* __restrict__ gy, int64_t total, int Kr,
                                                         int Khr, int C, const float* __restrict__ gamma,
                                                         const float* __restrict__ beta, float eps, const float* __restrict__ w1,
                                                         const float* __restrict__ b1, const float* __restrict__ w2, float s,
                                                         uint32_t thr, uint32_t k0, uint32_t k1, float* __restrict__ gx,
                                                         float* __restrict__ partial) {
    constexpr int KM = KC ? KC : MX_KMAX, KHM = KHC ? KHC : MX_KMAX;
    constexpr int NO = (mxb_partial_floats(KM, KHM) + 255) / 256;               // outputs per thread
    constexpr int UN = NO <= 2 ? 8 : 2;                                         // columns of phase 2 in flight
    const int K = KC ? KC : Kr, Kh = KHC ? KHC : Khr;
    const int GO = 0, H = K, GA = K + Kh, LN = K + 2 * Kh, GLN = 2 * K + 2 * Kh, XH = 3 * K + 2 * Kh, ONE = 4 * K + 2 * Kh;
    const int RS = mxb_row_floats(K, Kh), cols = mxb_cols(K, Kh), P = mxb_partial_floats(K, Kh);
    extern __shared__ float stage[];
    const int tid = threadIdx.x;
    // this thread's outputs tid, tid + 256 ...: the two slots of a row whose product it sums (beyond P: 1.0 * 1.0, never written)
    int ia[NO], ib[NO];
    float acc[NO];
#pragma unroll
    for (int q = 0; q < NO; ++q) {
        int o = tid + 256 * q;
        acc[q] = 0.0f;
        ia[q] = ONE;
        ib[q] = ONE;
        if (o < K) {                                            // ggamma[k]
            ia[q] = GLN + o;
            ib[q] = XH + o;
        } else if ((o -= K) < K) {                              // gbeta[k]
            ia[q] = GLN + o;
        } else if ((o -= K) < Kh * K) {                         // gw1[j][k]
            ia[q] = GA + o / K;
            ib[q] = LN + o % K;
        } else if ((o -= Kh * K) < Kh) {                        // gb1[j]
            ia[q] = GA + o;
        } else if ((o -= Kh) < K * Kh) {                        // gw2[k][j]
            ia[q] = GO + o / Kh;
            ib[q] = H + o % Kh;
        } else if ((o -= K * Kh) < K) {                         // gb2[k]
            ia[q] = GO + o;
        }
    }
    const int64_t nbatch = (total + cols - 1) / cols;
    for (int64_t b = blockIdx.x; b < nbatch; b += gridDim.x) {
        const int64_t i = b * cols + tid;                       // (node, channel)
        if (tid < cols && i < total) {
            // ---- phase 1: the column's forward again, then its gradients
            float* row = stage + tid * RS;
            const int64_t node = i / C;
            const int64_t base = node * K * C + (i - node * C);
            const uint64_t keep = thr ? mx_keep_bits(i, Kh + K, thr, k0, k1) : ~0ull;
            float v[KM], ln[KM], go[KM], gln[KM];
#pragma unroll
            for (int k = 0; k < KM; ++k) {
                v[k] = 0.0f;
                if (k < K) v[k] = x[base + (int64_t)k * C];
            }
            float m0, dl, rstd;
            mx_column_stats<KM>(v, K, eps, m0, dl, rstd);
#pragma unroll
            for (int k = 0; k < KM; ++k) {
                ln[k] = 0.0f;
                go[k] = 0.0f;
                gln[k] = 0.0f;
                if (k < K) {
                    const float xh = ((v[k] - m0) - dl) * rstd;
                    ln[k] = xh * gamma[k] + beta[k];
                    go[k] = gy[base + (int64_t)k * C] * (((keep >> (Kh + k)) & 1) ? s : 0.0f);
                    row[XH + k] = xh;
                    row[LN + k] = ln[k];
                    row[GO + k] = go[k];
                }
            }
            row[ONE] = 1.0f;
            for (int j = 0; j < Kh; ++j) {
                float a = 0.0f, gh = 0.0f;
#pragma unroll
                for (int k = 0; k < KM; ++k) {
                    if (k < K) {
                        a += w1[j * K + k] * ln[k];
                        gh += w2[k * Kh + j] * go[k];
                    }
                }
                a += b1[j];
                const float ms = ((keep >> j) & 1) ? s : 0.0f;
                const float ga = gh * ms * gelu_erf_grad(a);
                row[H + j] = gelu_erf(a) * ms;
                row[GA + j] = ga;
#pragma unroll
                for (int k = 0; k < KM; ++k)
                    if (k < K) gln[k] += w1[j * K + k] * ga;
            }
            float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
            for (int k = 0; k < KM; ++k) {
                if (k < K) {
                    row[GLN + k] = gln[k];
                    gln[k] *= gamma[k];                         // gxh
                    s1 += gln[k];
                    s2 += gln[k] * (((v[k] - m0) - dl) * rstd);
                }
            }
            if (gx) {
                s1 /= (float)K;
                s2 /= (float)K;
#pragma unroll
                for (int k = 0; k < KM; ++k)
                    if (k < K)
                        gx[base + (int64_t)k * C] =
                            rstd * ((gln[k] - s1) - (((v[k] - m0) - dl) * rstd) * s2) + gy[base + (int64_t)k * C];
            }
        }
        __syncthreads();
        // ---- phase 2: every output's sum over the batch's columns, in column order
        const int64_t left = total - b * cols;
        const int nc = left < cols ? (int)left : cols;
        // (one wave per SIMD: the rows of UN columns are read ahead of the dependent adds; the order of the adds stays the columns')
#pragma unroll UN
        for (int c = 0; c < nc; ++c) {
            const float* row = stage + c * RS;
#pragma unroll
            for (int q = 0; q < NO; ++q) acc[q] += row[ia[q]] * row[ib[q]];
        }
        __syncthreads();                                        // (the next batch rewrites the rows)
    }
    float* out = partial + (int64_t)blockIdx.x * P;
#pragma unroll
    for (int q = 0; q < NO; ++q)
        if (tid + 256 * q < P) out[tid + 256 * q] = acc[q];
}

static bool mxt_served(int64_t n_nodes, int32_t K, int32_t Kh, int32_t C) {
    if (n_nodes < 0 || K < 2 || K > MX_KMAX || Kh < 1 || Kh > MX_KMAX || C < 4 || (C & 3)) return false;
    return n_nodes <= (1ll << 31) / K && n_nodes * C <= (1ll << 38);
}

static bool mxt_aligned(std::initializer_list<const void*> ps, uintptr_t mask) {
    uintptr_t a = 0;
    for (const void* p : ps) a |= reinterpret_cast<uintptr_t>(p);
    return (a & mask) == 0;
}

template <int KC, int KHC>
static int launch_mixer_token_bwd(const float* x, const float* gy, int64_t total, int32_t K, int32_t Kh, int32_t C, const float* gamma,
                                  const float* beta, float eps, const float* w1, const float* b1, const float* w2, float p, uint64_t key,
                                  float* gx, float* partial, int32_t n_partial, hipStream_t s) {
    // the largest staging of the instantiation: <20, 10> 103 424 bytes; the generic one up to 256 rows of 159 floats
    constexpr int MAXB = KC ? mxb_cols(KC, KHC) * mxb_row_floats(KC, KHC) * 4 : 256 * 159 * 4;
    static LdsOptIn lds;
    const void* kernel = reinterpret_cast<const void*>(k_mixer_token_bwd<KC, KHC>);
    if (!lds.granted({kernel}, MAXB)) return TPNET_ERR_BAD_ARG;
    const int cols = mxb_cols(K, Kh);
    const int64_t nbatch = (total + cols - 1) / cols;
    const int grid = (int)(nbatch < n_partial ? nbatch : n_partial);
    hipLaunchKernelGGL((k_mixer_token_bwd<KC, KHC>), dim3((unsigned)grid), dim3(256), (size_t)cols * mxb_row_floats(K, Kh) * 4, s, x, gy,
                       total, (int)K, (int)Kh, (int)C, gamma, beta, eps, w1, b1, w2, 1.0f / (1.0f - p), drop_threshold(p), (uint32_t)key,
                       (uint32_t)(key >> 32), gx, partial);
    TPNET_HIP_TRY(hipGetLastError());
    return grid;
}

}  // namespace tpnet

using namespace tpnet;

extern "C" int tpnet_mixer_token_train(const float* x, int64_t n_nodes, int32_t K, int32_t C, const float* gamma, const float* beta,
                                       float eps, const float* w1, const float* b1, int32_t Kh, const float* w2, const float* b2, float p,
                                       uint64_t key, float* out, void* stream) {
    if (!x || !gamma || !beta || !w1 || !b1 || !w2 || !b2 || !out || out == x) return TPNET_ERR_BAD_ARG;
    if (!mxt_served(n_nodes, K, Kh, C) || !drop_rate(p)) return TPNET_ERR_BAD_ARG;
    if (!mxt_aligned({x, out}, 15) || !mxt_aligned({gamma, beta, w1, b1, w2, b2}, 3)) return TPNET_ERR_BAD_ARG;
    const int64_t total = n_nodes * C;
    if (total == 0) return TPNET_OK;
    const auto kernel = K == 20 && Kh == 10 ? k_mixer_token_train<20, 10> : k_mixer_token_train<0, 0>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, total, (int)K, (int)Kh, (int)C,
                       gamma, beta, eps, w1, b1, w2, b2, 1.0f / (1.0f - p), drop_threshold(p), (uint32_t)key, (uint32_t)(key >> 32), out);
    TPNET_HIP_TRY(hipGetLastError());
    return TPNET_OK;
}

extern "C" int64_t tpnet_mixer_token_bwd_partial_floats(int32_t K, int32_t Kh) {
    return mxt_served(0, K, Kh, 4) ? mxb_partial_floats(K, Kh) : 0;
}

extern "C" int tpnet_mixer_token_bwd(const float* x, const float* gy, int64_t n_nodes, int32_t K, int32_t C, const float* gamma,
                                     const float* beta, float eps, const float* w1, const float* b1, int32_t Kh, const float* w2,
                                     const float* b2, float p, uint64_t key, float* gx, float* partial, int32_t n_partial, void* stream) {
    if (!x || !gy || !gamma || !beta || !w1 || !b1 || !w2 || !b2 || !partial || gx == x || gx == gy) return TPNET_ERR_BAD_ARG;
    if (!mxt_served(n_nodes, K, Kh, C) || !drop_rate(p) || n_partial < 1) return TPNET_ERR_BAD_ARG;
    if (!mxt_aligned({x, gy, gx}, 15) || !mxt_aligned({gamma, beta, w1, b1, w2, b2, partial}, 3)) return TPNET_ERR_BAD_ARG;
    const int64_t total = n_nodes * C;
    if (total == 0) return 0;
    // (b2 itself is not read: its gradient is a sum of go)
    return K == 20 && Kh == 10 ? launch_mixer_token_bwd<20, 10>(x, gy, total, K, Kh, C, gamma, beta, eps, w1, b1, w2, p, key, gx, partial,
                                                                n_partial, (hipStream_t)stream)
                               : launch_mixer_token_bwd<0, 0>(x, gy, total, K, Kh, C, gamma, beta, eps, w1, b1, w2, p, key, gx, partial,
                                                              n_partial, (hipStream_t)stream);
}

extern "C" int tpnet_mixer_token_masks(int64_t n_nodes, int32_t K, int32_t Kh, int32_t C, float p, uint64_t key, uint8_t* m1, uint8_t* m2,
                                       void* stream) {
    if (!m1 || !m2 || !mxt_served(n_nodes, K, Kh, C) || !drop_rate(p)) return TPNET_ERR_BAD_ARG;
    const int64_t total = n_nodes * C;
    if (total == 0) return TPNET_OK;
    hipLaunchKernelGGL(k_mixer_token_masks, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, total, (int)K,
                       (int)Kh, (int)C, drop_threshold(p), (uint32_t)key, (uint32_t)(key >> 32), m1, m2);
    TPNET_HIP_TRY(hipGetLastError());
    return TPNET_OK;
}
