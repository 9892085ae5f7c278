// Link-prediction metrics of one batch on the device: BCE loss, average precision and ROC-AUC (the reference's per-batch
// `loss.item()`, `predicts.sigmoid().cpu()` and the two sklearn calls: evaluate_models_utils.py:187-193, utils/metrics.py:8-22).
// No sort: every positive counts the scores at or above its own -- a_i among the positives, b_i among the negatives -- and the
// negatives equal to it, c_i; AP = mean a_i / (a_i + b_i), AUC = sum(2 (N - b_i) + c_i) / (2 P N).  The rule is spelled out in
// include/tpnet_hip.h.  Everything that crosses threads out of order is an integer, and the float64 sums are reduced in a fixed
// order, so a call's record does not depend on scheduling.
// A training batch (tpnet_lp_train_loss: train_link_prediction.py:375-386) is the same three launches: the workgroups that evaluate
// a logit's loss term also write d(mean loss) / d(logit), and the finish workgroup the loss as one fp32.
#include "tpnet_common.h"
#include "arena.hpp"

#include <math.h>

namespace tpnet {

static constexpr int LPM_TILE = 256;                 // positives per workgroup of the counting kernel, one per thread
static constexpr int LPM_CHUNK = 256;                // scores of the (positives, negatives) axis a workgroup stages in LDS
static constexpr int LPM_FIN = 1024;                 // threads of the finish kernel's one workgroup
static constexpr int64_t LPM_MAX_SCORES = 1 << 18;   // P + N of a call

// Sum over the workgroup in a fixed order: a halving tree over the threads' values (sh: NT entries).  Every thread gets the sum.
template <int NT, class T>
__device__ T lpm_tree_sum(T v, T* sh) {
    __syncthreads();                                           // (the previous sum's readers are done with sh)
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int s = NT / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
        __syncthreads();
    }
    return sh[0];
}

__device__ inline double lpm_bce_term(float logit, double y) {
    const double x = (double)logit;
    return fmax(x, 0.0) - x * y + log1p(exp(-fabs(x)));
}

// d/dx of the mean of the P + N terms, (sigmoid(x) - y) / n, formed from the LOGIT in the branch that does not cancel -- a positive:
// sigmoid(x) - 1 = -1 / (1 + exp(x)), a negative: sigmoid(x) = 1 / (1 + exp(-x)) -- in float64 and rounded once: where an fp32
// sigmoid has saturated to 1 or 0 the gradient keeps its relative accuracy.  exp overflows to inf -> 0; NaN -> NaN.
__device__ inline float lpm_bce_grad(float logit, bool positive, double n) {
    const double x = (double)logit;
    return (float)(positive ? -1.0 / (1.0 + exp(x)) / n : 1.0 / (1.0 + exp(-x)) / n);
}

// the scratch buffer (8-byte aligned by the caller, laid out from where it starts): cnt [3][P] uint32 = a | b | c, the NaN word in a
// 256-byte slot of its own, then part double[chunks].  zero_bytes: cnt and the NaN word are zeroed by one fill before the counting
// kernel; part is written whole
struct LpmScratch { uint32_t* cnt; uint32_t* nan; double* part; size_t zero_bytes; };
static void lpm_layout(Arena& a, LpmScratch& w, int64_t n_pos, int64_t n_neg) {
    w.cnt = a.take<uint32_t>(3 * (size_t)n_pos);
    w.nan = a.take<uint32_t>(64);
    w.zero_bytes = a.off;
    w.part = a.take<double>((size_t)(n_pos + n_neg + LPM_CHUNK - 1) / LPM_CHUNK);
}

// Workgroup (x, y): positives [256 x, 256 x + 256) against scores [256 y, 256 y + 256) of the concatenated axis (the P
// positives, then the N negatives).  The chunk's positives and its negatives are staged as two runs, each padded with NaN -- which
// compares false both ways -- to whole float4s: the loops read no labels and no bounds, and every lane reads the same 16 bytes (a
// broadcast).  The workgroups x = 0 see every score once while staging: they raise the NaN word and sum their chunk's loss terms
// (thread k: entries k, k + 256, ... of the staged order, then a tree) into part[y].  GRAD (a training batch; has_loss holds): they
// also write each logit's gradient, pos_grad[P] / neg_grad[N], one plain store per element.
template <bool GRAD>
__global__ __launch_bounds__(LPM_TILE) void k_lpm_count(const float* __restrict__ pos, uint32_t P, const float* __restrict__ neg,
                                                        uint32_t N, const float* __restrict__ pos_logit,
                                                        const float* __restrict__ neg_logit, int has_loss,
                                                        uint32_t* __restrict__ cnt, uint32_t* __restrict__ nan_word,
                                                        double* __restrict__ part, float* __restrict__ pos_grad,
                                                        float* __restrict__ neg_grad) {
    __shared__ __attribute__((aligned(16))) float sh[LPM_CHUNK + 8];
    __shared__ double shd[LPM_TILE];
    const uint32_t i = blockIdx.x * LPM_TILE + threadIdx.x;
    const uint32_t c0 = blockIdx.y * LPM_CHUNK;
    const uint32_t c1 = min(c0 + (uint32_t)LPM_CHUNK, P + N);
    const uint32_t np = c0 < P ? min(c1, P) - c0 : 0u;        // positives / negatives of the chunk
    const uint32_t nn = (c1 - c0) - np;
    const uint32_t np4 = (np + 3u) & ~3u, nn4 = (nn + 3u) & ~3u;   // np4 + nn4 <= LPM_CHUNK + 6
    const uint32_t n0 = c0 + np - P;                          // first negative of the chunk (nn > 0: c0 + np >= P)
    const bool first = blockIdx.x == 0;
    const double n = (double)((long long)P + (long long)N);
    double loss = 0.0;
    bool bad = false;
    for (uint32_t k = threadIdx.x; k < np4 + nn4; k += LPM_TILE) {
        float v = NAN;
        if (k < np) {
            v = pos[c0 + k];
            bad |= isnan(v);
            if (first && has_loss) {
                const float x = pos_logit[c0 + k];
                loss += lpm_bce_term(x, 1.0);
                if constexpr (GRAD) pos_grad[c0 + k] = lpm_bce_grad(x, true, n);
            }
        } else if (k >= np4 && k - np4 < nn) {
            v = neg[n0 + (k - np4)];
            bad |= isnan(v);
            if (first && has_loss) {
                const float x = neg_logit[n0 + (k - np4)];
                loss += lpm_bce_term(x, 0.0);
                if constexpr (GRAD) neg_grad[n0 + (k - np4)] = lpm_bce_grad(x, false, n);
            }
        }
        sh[k] = v;
    }
    if (first) {                                              // (uniform over the workgroup: the tree's barriers are met by all)
        if (bad) atomicOr(nan_word, 1u);
        if (has_loss) {
            loss = lpm_tree_sum<LPM_TILE>(loss, shd);
            if (threadIdx.x == 0) part[blockIdx.y] = loss;
        }
    }
    __syncthreads();
    if (i >= P) return;
    const float p = pos[i];
    const float4* s4 = reinterpret_cast<const float4*>(sh);
    uint32_t a = 0, b = 0, c = 0;
#pragma unroll 4
    for (uint32_t k = 0; k < np4 / 4u; ++k) {
        const float4 v = s4[k];
        a += (uint32_t)(v.x >= p) + (uint32_t)(v.y >= p) + (uint32_t)(v.z >= p) + (uint32_t)(v.w >= p);
    }
#pragma unroll 4
    for (uint32_t k = np4 / 4u; k < (np4 + nn4) / 4u; ++k) {
        const float4 v = s4[k];
        b += (uint32_t)(v.x >= p) + (uint32_t)(v.y >= p) + (uint32_t)(v.z >= p) + (uint32_t)(v.w >= p);
        c += (uint32_t)(v.x == p) + (uint32_t)(v.y == p) + (uint32_t)(v.z == p) + (uint32_t)(v.w == p);
    }
    if (a) atomicAdd(&cnt[i], a);
    if (b) atomicAdd(&cnt[P + i], b);
    if (c) atomicAdd(&cnt[2u * P + i], c);
}

// ONE workgroup: thread k takes entries k, k + 1024, ... of every list in ascending order, the 1024 partial sums meet in the tree.
// n_part: the counting kernel's chunks (0: no loss).  loss_out (a training batch; else null): the record's loss word once more, as fp32.
__global__ __launch_bounds__(LPM_FIN) void k_lpm_finish(uint32_t P, uint32_t N, const uint32_t* __restrict__ cnt,
                                                        const uint32_t* __restrict__ nan_word, const double* __restrict__ part,
                                                        uint32_t n_part, int has_loss, void* __restrict__ record,
                                                        float* __restrict__ loss_out) {
    __shared__ double shd[LPM_FIN];
    __shared__ long long shi[LPM_FIN];
    double ap = 0.0, loss = 0.0;
    long long u2 = 0;
    for (uint32_t i = threadIdx.x; i < P; i += LPM_FIN) {
        const uint32_t a = cnt[i], b = cnt[P + i], c = cnt[2u * P + i];
        ap += (double)a / (double)(a + b);                     // (a NaN positive: 0 / 0, and the flag below)
        u2 += 2ll * (long long)(N - b) + (long long)c;
    }
    if (has_loss)
        for (uint32_t j = threadIdx.x; j < n_part; j += LPM_FIN) loss += part[j];
    ap = lpm_tree_sum<LPM_FIN>(ap, shd);
    loss = lpm_tree_sum<LPM_FIN>(loss, shd);
    u2 = lpm_tree_sum<LPM_FIN>(u2, shi);
    if (threadIdx.x == 0) {
        const long long flags = ((P == 0 || N == 0) ? 1ll : 0ll) | ((P + N > 0 && *nan_word) ? 2ll : 0ll);
        const double nan = __builtin_nan("");
        double* rd = reinterpret_cast<double*>(record);
        long long* ri = reinterpret_cast<long long*>(record);
        const double mean = has_loss ? loss / (double)((long long)P + (long long)N) : nan;
        rd[0] = mean;
        if (loss_out) *loss_out = (float)mean;
        rd[1] = flags ? nan : ap / (double)P;
        rd[2] = flags ? nan : (double)u2 / (double)(2ll * (long long)P * (long long)N);
        ri[3] = u2;
        ri[4] = (long long)P;
        ri[5] = (long long)N;
        ri[6] = flags;
        ri[7] = 0;
    }
}

static bool lpm_sizes_ok(int64_t n_pos, int64_t n_neg) {
    return n_pos >= 0 && n_neg >= 0 && n_pos <= LPM_MAX_SCORES && n_neg <= LPM_MAX_SCORES && n_pos + n_neg <= LPM_MAX_SCORES;
}

static size_t lpm_scratch_bytes(int64_t n_pos, int64_t n_neg) {
    if (!lpm_sizes_ok(n_pos, n_neg)) return 0;
    return measured([&](Arena& a) { LpmScratch w; lpm_layout(a, w, n_pos, n_neg); });
}

// What tpnet_lp_metrics and tpnet_lp_train_loss share: the checks of the common arguments and the three launches.  train: the
// counting kernel's first row writes the gradients, the finish workgroup loss_out (the caller has checked those three pointers).
static int lpm_enqueue(const float* pos_score, int64_t n_pos, const float* neg_score, int64_t n_neg, const float* pos_logit,
                       const float* neg_logit, void* scratch, size_t scratch_bytes, void* record, bool train, float* pos_grad,
                       float* neg_grad, float* loss_out, void* stream) {
    if (!lpm_sizes_ok(n_pos, n_neg) || !record || ((size_t)record & 7) || (n_pos > 0 && !pos_score) || (n_neg > 0 && !neg_score))
        return TPNET_ERR_BAD_ARG;
    const bool any = n_pos + n_neg > 0;
    if (any && (!scratch || ((size_t)scratch & 7))) return TPNET_ERR_BAD_ARG;
    if (any && scratch_bytes < lpm_scratch_bytes(n_pos, n_neg)) return TPNET_ERR_WORKSPACE;
    // the loss needs the logits of every side that is not empty
    const bool has_loss = (pos_logit || neg_logit) && (n_pos == 0 || pos_logit) && (n_neg == 0 || neg_logit);
    hipStream_t s = (hipStream_t)stream;
    const uint32_t P = (uint32_t)n_pos, N = (uint32_t)n_neg;
    Arena wa(any ? scratch : nullptr, scratch_bytes);
    LpmScratch w;
    lpm_layout(wa, w, n_pos, n_neg);
    uint32_t chunks = 0;
    if (any) {
        const uint32_t gx = P ? (P + LPM_TILE - 1) / LPM_TILE : 1u;          // (no positives: one row of workgroups for the loss)
        chunks = (P + N + LPM_CHUNK - 1) / LPM_CHUNK;
        TPNET_HIP_TRY(hipMemsetAsync(scratch, 0, w.zero_bytes, s));
        hipLaunchKernelGGL(train ? k_lpm_count<true> : k_lpm_count<false>, dim3(gx, chunks), dim3(LPM_TILE), 0, s, pos_score, P,
                           neg_score, N, pos_logit, neg_logit, (int)has_loss, w.cnt, w.nan, w.part, pos_grad, neg_grad);
    }
    hipLaunchKernelGGL(k_lpm_finish, dim3(1), dim3(LPM_FIN), 0, s, P, N, (const uint32_t*)w.cnt, (const uint32_t*)w.nan,
                       (const double*)w.part, chunks, (int)has_loss, record, loss_out);
    TPNET_HIP_TRY(hipGetLastError());
    return TPNET_OK;
}

// ---- one-vs-many ranking (tpnet_lp_ranking; the rule: include/tpnet_hip.h) ------------------------------------------------------------
static constexpr int LPR_BLOCK = 256;                // four waves, one query each
static constexpr int32_t LPR_MAX_C1 = 1 << 20;
enum { LPR_FLAG_NO_QUERY = 1, LPR_FLAG_NAN_SCORE = 2, LPR_FLAG_EMPTY_QUERY = 4, LPR_FLAG_FILTER_OVERFLOW = 8 };

// scratch: three words per query -- m_i (0: not counted), its valid candidates, its flags
struct LprScratch { uint32_t* m; uint32_t* nv; uint32_t* fl; };
static void lpr_layout(Arena& a, LprScratch& w, int64_t B) {
    const size_t n = (size_t)(B < 1 ? 1 : B);
    w.m = a.take<uint32_t>(n);
    w.nv = a.take<uint32_t>(n);
    w.fl = a.take<uint32_t>(n);
}
static bool lpr_sizes_ok(int64_t B, int32_t C1) { return B >= 0 && B < (1ll << 31) && C1 >= 1 && C1 <= LPR_MAX_C1; }

// one wave per query, strided over its C1 columns: integer counts only, combined by shuffles
// SKIP (tpnet_lp_ranking_skip): `cand` is not read; candidate column skip[i] of query i (-1: none) is absent instead
template <bool SKIP>
__global__ __launch_bounds__(LPR_BLOCK) void k_lpr_rows(const float* __restrict__ logits, int64_t B, int C1,
                                                        const int64_t* __restrict__ cand, const int64_t* __restrict__ skip,
                                                        uint32_t* __restrict__ m_out, uint32_t* __restrict__ nv_out,
                                                        uint32_t* __restrict__ fl_out) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * (LPR_BLOCK / 64) + (threadIdx.x >> 6);
    if (i >= B) return;
    const float* row = logits + i * (int64_t)C1;
    const int64_t* crow = (!SKIP && cand) ? cand + i * (int64_t)(C1 - 1) : nullptr;
    const int64_t sk = SKIP ? skip[i] : -1;
    const float p = row[0];
    uint32_t g = 0, e = 0, nv = 0, bad = isnan(p) ? 1u : 0u;
    for (int c = lane; c < C1 - 1; c += 64) {
        if (SKIP ? c == sk : (crow && crow[c] < 0)) continue;
        const float q = row[1 + c];
        nv += 1u;
        g += (uint32_t)(q > p);
        e += (uint32_t)(q == p);
        bad |= isnan(q) ? 1u : 0u;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        g += (uint32_t)__shfl_xor((int)g, o, 64);
        e += (uint32_t)__shfl_xor((int)e, o, 64);
        nv += (uint32_t)__shfl_xor((int)nv, o, 64);
        bad |= (uint32_t)__shfl_xor((int)bad, o, 64);
    }
    if (lane == 0) {
        const uint32_t fl = (bad ? (uint32_t)LPR_FLAG_NAN_SCORE : 0u) | (nv == 0 ? (uint32_t)LPR_FLAG_EMPTY_QUERY : 0u);
        m_out[i] = fl ? 0u : 2u + 2u * g + e;
        nv_out[i] = nv;
        fl_out[i] = fl;
    }
}

// the three words per query from COUNTS (tpnet_lp_ranking_counts): counts[i] = {g, e, nv, flags} as the scoring kernel left them
// (tpnet_score_rank_range), less what the query's filter list holds -- over its slots j < min(n_fil, F) with an id >= 0,
// g_f = #{fil_logit > p}, e_f = #{fil_logit == p}.  One thread per query: the lists are short (a source's known destinations)
__global__ __launch_bounds__(LPR_BLOCK) void k_lpr_counts(const int4* __restrict__ counts, const float* __restrict__ pos_logit, int64_t B,
                                                          const float* __restrict__ fil_logits, const int64_t* __restrict__ fil_ids,
                                                          const int32_t* __restrict__ n_fil, int F, uint32_t* __restrict__ m_out,
                                                          uint32_t* __restrict__ nv_out, uint32_t* __restrict__ fl_out) {
    const int64_t i = (int64_t)blockIdx.x * LPR_BLOCK + threadIdx.x;
    if (i >= B) return;
    const int4 c = counts[i];
    const float p = pos_logit[i];
    int64_t g = c.x, e = c.y, nv = c.z;
    uint32_t fl = ((c.w & LPR_FLAG_NAN_SCORE) || isnan(p)) ? (uint32_t)LPR_FLAG_NAN_SCORE : 0u;
    if (fil_logits) {
        const int nf = n_fil[i];
        const int n = nf < F ? (nf < 0 ? 0 : nf) : F;
        if (nf > F) fl |= (uint32_t)LPR_FLAG_FILTER_OVERFLOW;
        for (int j = 0; j < n; ++j) {
            if (fil_ids[i * F + j] < 0) continue;
            const float q = fil_logits[i * F + j];
            g -= (int64_t)(q > p);
            e -= (int64_t)(q == p);
            if (isnan(q)) fl |= (uint32_t)LPR_FLAG_NAN_SCORE;
        }
        nv -= nf < 0 ? 0 : nf;
    }
    if (nv <= 0) { nv = 0; fl |= (uint32_t)LPR_FLAG_EMPTY_QUERY; }
    m_out[i] = fl ? 0u : (uint32_t)(2 + 2 * g + e);
    nv_out[i] = (uint32_t)nv;
    fl_out[i] = fl;
}

// ONE workgroup: thread k takes queries k, k + 1024, ... in ascending order, the 1024 partial sums meet in the tree
__global__ __launch_bounds__(LPM_FIN) void k_lpr_finish(int64_t B, const uint32_t* __restrict__ m, const uint32_t* __restrict__ nv,
                                                        const uint32_t* __restrict__ fl, int k1, int k2, int k3,
                                                        int64_t* __restrict__ record) {
    __shared__ double shd[LPM_FIN];
    __shared__ long long shi[LPM_FIN];
    double rr = 0.0;
    long long msum = 0, n = 0, nvalid = 0, h1 = 0, h2 = 0, h3 = 0, flags = 0;
    for (int64_t i = threadIdx.x; i < B; i += LPM_FIN) {
        const long long mi = (long long)m[i];
        nvalid += (long long)nv[i];
        flags |= (long long)fl[i];
        if (mi) {
            rr += 2.0 / (double)mi;
            msum += mi;
            n += 1;
            h1 += mi <= 2ll * k1;
            h2 += mi <= 2ll * k2;
            h3 += mi <= 2ll * k3;
        }
    }
    rr = lpm_tree_sum<LPM_FIN>(rr, shd);
    msum = lpm_tree_sum<LPM_FIN>(msum, shi);
    n = lpm_tree_sum<LPM_FIN>(n, shi);
    nvalid = lpm_tree_sum<LPM_FIN>(nvalid, shi);
    h1 = lpm_tree_sum<LPM_FIN>(h1, shi);
    h2 = lpm_tree_sum<LPM_FIN>(h2, shi);
    h3 = lpm_tree_sum<LPM_FIN>(h3, shi);
    // (flags: one bit at a time through the sum tree -- a count, then a test)
    long long f2 = lpm_tree_sum<LPM_FIN>((long long)((flags & LPR_FLAG_NAN_SCORE) != 0), shi);
    long long f4 = lpm_tree_sum<LPM_FIN>((long long)((flags & LPR_FLAG_EMPTY_QUERY) != 0), shi);
    long long f8 = lpm_tree_sum<LPM_FIN>((long long)((flags & LPR_FLAG_FILTER_OVERFLOW) != 0), shi);      // (tpnet_lp_ranking_counts only)
    if (threadIdx.x == 0) {
        const double nan = __builtin_nan("");
        double* rd = reinterpret_cast<double*>(record);
        long long* ri = reinterpret_cast<long long*>(record);
        const double dn = (double)n;
        rd[0] = n ? rr / dn : nan;
        rd[1] = n ? (double)h1 / dn : nan;
        rd[2] = n ? (double)h2 / dn : nan;
        rd[3] = n ? (double)h3 / dn : nan;
        ri[4] = msum;
        ri[5] = n;
        ri[6] = nvalid;
        ri[7] = (n ? 0ll : (long long)LPR_FLAG_NO_QUERY) | (f2 ? (long long)LPR_FLAG_NAN_SCORE : 0ll) |
                (f4 ? (long long)LPR_FLAG_EMPTY_QUERY : 0ll) | (f8 ? (long long)LPR_FLAG_FILTER_OVERFLOW : 0ll);
    }
}

}  // namespace tpnet

using namespace tpnet;

extern "C" {

size_t tpnet_lp_metrics_scratch_bytes(int64_t n_pos, int64_t n_neg) { return lpm_scratch_bytes(n_pos, n_neg); }

int tpnet_lp_metrics(const float* pos_score, int64_t n_pos, const float* neg_score, int64_t n_neg, const float* pos_logit,
                     const float* neg_logit, void* scratch, size_t scratch_bytes, void* record, void* stream) {
    return lpm_enqueue(pos_score, n_pos, neg_score, n_neg, pos_logit, neg_logit, scratch, scratch_bytes, record, false, nullptr,
                       nullptr, nullptr, stream);
}

int tpnet_lp_train_loss(const float* pos_score, int64_t n_pos, const float* neg_score, int64_t n_neg, const float* pos_logit,
                        const float* neg_logit, void* scratch, size_t scratch_bytes, void* record, float* pos_grad, float* neg_grad,
                        float* loss_out, void* stream) {
    if (!lpm_sizes_ok(n_pos, n_neg) || n_pos + n_neg == 0 || !loss_out || ((size_t)loss_out & 3)) return TPNET_ERR_BAD_ARG;
    if ((n_pos > 0 && (!pos_logit || !pos_grad)) || (n_neg > 0 && (!neg_logit || !neg_grad))) return TPNET_ERR_BAD_ARG;
    return lpm_enqueue(pos_score, n_pos, neg_score, n_neg, pos_logit, neg_logit, scratch, scratch_bytes, record, true, pos_grad,
                       neg_grad, loss_out, stream);
}

size_t tpnet_lp_ranking_scratch_bytes(int64_t B, int32_t C1) {
    if (!lpr_sizes_ok(B, C1)) return 0;
    return measured([&](Arena& a) { LprScratch w; lpr_layout(a, w, B); });
}

// what tpnet_lp_ranking and tpnet_lp_ranking_skip share: the checks, the scratch, the two launches (skip: one absent column per query)
static int lpr_enqueue(const float* logits, int64_t B, int32_t C1, const int64_t* cand_or_null, const int64_t* skip, bool with_skip,
                       int32_t k1, int32_t k2, int32_t k3, void* scratch, size_t scratch_bytes, int64_t* record, void* stream) {
    if (!lpr_sizes_ok(B, C1) || k1 < 1 || k2 < 1 || k3 < 1 || !record || ((size_t)record & 7)) return TPNET_ERR_BAD_ARG;
    if (B > 0 && (!logits || !scratch || ((size_t)scratch & 7))) return TPNET_ERR_BAD_ARG;
    if (with_skip && B > 0 && (!skip || ((size_t)skip & 7))) return TPNET_ERR_BAD_ARG;
    if (B > 0 && scratch_bytes < tpnet_lp_ranking_scratch_bytes(B, C1)) return TPNET_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    Arena wa(B > 0 ? scratch : nullptr, scratch_bytes);
    LprScratch w;
    lpr_layout(wa, w, B);
    if (B > 0) {
        const int per = LPR_BLOCK / 64;
        hipLaunchKernelGGL(with_skip ? k_lpr_rows<true> : k_lpr_rows<false>, dim3((unsigned)((B + per - 1) / per)), dim3(LPR_BLOCK), 0, s,
                           logits, B, (int)C1, cand_or_null, skip, w.m, w.nv, w.fl);
    }
    hipLaunchKernelGGL(k_lpr_finish, dim3(1), dim3(LPM_FIN), 0, s, B, (const uint32_t*)w.m, (const uint32_t*)w.nv,
                       (const uint32_t*)w.fl, (int)k1, (int)k2, (int)k3, record);
    TPNET_HIP_TRY(hipGetLastError());
    return TPNET_OK;
}

int tpnet_lp_ranking(const float* logits, int64_t B, int32_t C1, const int64_t* cand_or_null, int32_t k1, int32_t k2, int32_t k3,
                     void* scratch, size_t scratch_bytes, int64_t* record, void* stream) {
    return lpr_enqueue(logits, B, C1, cand_or_null, nullptr, false, k1, k2, k3, scratch, scratch_bytes, record, stream);
}

int tpnet_lp_ranking_skip(const float* logits, int64_t B, int32_t C1, const int64_t* skip_col, int32_t k1, int32_t k2, int32_t k3,
                          void* scratch, size_t scratch_bytes, int64_t* record, void* stream) {
    return lpr_enqueue(logits, B, C1, nullptr, skip_col, true, k1, k2, k3, scratch, scratch_bytes, record, stream);
}

int tpnet_lp_ranking_counts(const int32_t* counts, const float* pos_logit, int64_t B, const float* fil_logits, const int64_t* fil_ids,
                            const int32_t* n_fil, int32_t F, int32_t k1, int32_t k2, int32_t k3, void* scratch, size_t scratch_bytes,
                            int64_t* record, void* stream) {
    if (!lpr_sizes_ok(B, 1) || k1 < 1 || k2 < 1 || k3 < 1 || !record || ((size_t)record & 7)) return TPNET_ERR_BAD_ARG;
    if (B > 0 && (!counts || ((size_t)counts & 15) || !pos_logit || ((size_t)pos_logit & 3) || !scratch || ((size_t)scratch & 7)))
        return TPNET_ERR_BAD_ARG;
    if (B > 0 && fil_logits &&
        (F < 1 || F >= (1 << 16) || !fil_ids || !n_fil || ((size_t)fil_logits & 3) || ((size_t)fil_ids & 7) || ((size_t)n_fil & 3)))
        return TPNET_ERR_BAD_ARG;
    if (B > 0 && scratch_bytes < tpnet_lp_ranking_scratch_bytes(B, 1)) return TPNET_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    Arena wa(B > 0 ? scratch : nullptr, scratch_bytes);
    LprScratch w;
    lpr_layout(wa, w, B);
    if (B > 0)
        hipLaunchKernelGGL(k_lpr_counts, dim3((unsigned)((B + LPR_BLOCK - 1) / LPR_BLOCK)), dim3(LPR_BLOCK), 0, s,
                           reinterpret_cast<const int4*>(counts), pos_logit, B, fil_logits, fil_ids, n_fil, (int)F, w.m, w.nv, w.fl);
    hipLaunchKernelGGL(k_lpr_finish, dim3(1), dim3(LPM_FIN), 0, s, B, (const uint32_t*)w.m, (const uint32_t*)w.nv,
                       (const uint32_t*)w.fl, (int)k1, (int)k2, (int)k3, record);
    TPNET_HIP_TRY(hipGetLastError());
    return TPNET_OK;
}

}  // extern "C"
