// Device-side EdgeBank, the memorisation baseline of the reference (models/EdgeBank.py, evaluate_models_utils.py:202-318) in its three
// memory modes.  The reference rebuilds a Python set (or a dict of lists) over train + val + test[:batch_start] for every batch.  Here
// the whole chronological stream is one table, built once: the U unique edges in ascending (src << 32 | dst) order, each with the
// ascending list of the stream POSITIONS at which it occurs, a copy of the stamps, and present[h] = the number of distinct edges among
// the first h positions.  A call names a history length h and answers from the prefix: one binary search for the pair, one for h in its
// position list.  The rule is spelled out in include/tpnet_hip.h.  No floating-point atomics: the one float64 sum (repeat_interval) runs
// in a fixed order, so a call gives the same bits every time.
#include "tpnet_common.h"
#include "scan_common.hpp"
#include "arena.hpp"
#include "sort_tmp.hpp"

namespace tpnet {

static constexpr int EB_STAT_WGS = 256;              // workgroups of k_eb_stats at most: one partial each, folded by 256 threads

// header words of the table
enum { EB_U = 0, EB_BAD = 1, EB_DEC = 2, EB_FIRSTS = 8 };   // EB_FIRSTS: the second scan's total (the first occurrences: U again)

// ---- build ---------------------------------------------------------------------------------------------------------------------
// key and position of every edge, the copy of the stamps; flags a bad id and a stamp below its predecessor's (a NaN included)
__global__ void k_eb_keys(const int64_t* __restrict__ src, const int64_t* __restrict__ dst, const double* __restrict__ t, int64_t E,
                          uint64_t* __restrict__ key, uint32_t* __restrict__ idx, double* __restrict__ tcopy,
                          uint32_t* __restrict__ hdr) {
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < E; j += (int64_t)gridDim.x * blockDim.x) {
        const int64_t s = src[j], d = dst[j];
        if ((uint64_t)s >= (1ull << 31) || (uint64_t)d >= (1ull << 31)) atomicAdd(&hdr[EB_BAD], 1u);
        const double tj = t[j];
        if (!(tj == tj) || (j > 0 && !(tj >= t[j - 1]))) atomicAdd(&hdr[EB_DEC], 1u);
        key[j] = ((uint64_t)((uint32_t)s & 0x7FFFFFFFu) << 32) | (uint64_t)((uint32_t)d & 0x7FFFFFFFu);
        idx[j] = (uint32_t)j;
        tcopy[j] = tj;
    }
}

struct EbHead {
    const uint64_t* k;
    __device__ uint32_t operator()(uint32_t j) const { return (j == 0 || k[j] != k[j - 1]) ? 1u : 0u; }
};
// a unique edge's key and the start of its position list; its first position (the list is ascending) is where the stream first shows it
struct EbEmit {
    const uint64_t* ek; const uint32_t* pos; uint64_t* ukey; uint32_t* ustart; uint8_t* first;
    __device__ void operator()(uint32_t j, uint32_t r) const {
        ukey[r] = ek[j];
        ustart[r] = j;
        first[pos[j]] = 1;
    }
};
struct EbFirst {
    const uint8_t* first;
    __device__ uint32_t operator()(uint32_t p) const { return first[p]; }
};

// present[p + 1] = first occurrences among positions 0..p (blk: the exclusive tile sums of the scan); closes ustart with E
__global__ __launch_bounds__(256) void k_eb_present(const uint8_t* __restrict__ first, uint32_t n, const uint32_t* __restrict__ blk,
                                                    const uint32_t* __restrict__ hdr, uint32_t* __restrict__ present,
                                                    uint32_t* __restrict__ ustart) {
    __shared__ uint32_t sh[4];
    const uint32_t nb = (n + 255u) / 256u;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        present[0] = 0u;
        ustart[hdr[EB_U]] = n;                                 // U <= n: ustart holds n + 1 entries
    }
    for (uint32_t tile = blockIdx.x; tile < nb; tile += gridDim.x) {
        const uint32_t j = tile * 256u + threadIdx.x;
        const uint32_t v = j < n ? first[j] : 0u;
        uint32_t tot;
        const uint32_t incl = wg_scan256(v, sh, tot);
        if (j < n) present[j + 1] = blk[tile] + incl;
    }
}

// ---- predict -------------------------------------------------------------------------------------------------------------------
struct EbTable {
    const uint32_t* hdr; const uint64_t* ukey; const uint32_t* ustart; const uint32_t* pos; const double* t; const uint32_t* present;
};

// occurrences of unique edge u among the first h positions: an upper bound of h - 1 in its ascending position list
__device__ __forceinline__ uint32_t eb_count(const EbTable& tb, uint32_t u, uint32_t h, uint32_t& lo0) {
    uint32_t lo = tb.ustart[u], hi = tb.ustart[u + 1];
    lo0 = lo;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (tb.pos[mid] < h) lo = mid + 1; else hi = mid;
    }
    return lo - lo0;
}

// Sum over the workgroup in a fixed order: a halving tree over the lanes of each wave, then the four waves' sums in wave order.
// Every thread gets the sum.  sh: 4 doubles.
__device__ __forceinline__ double eb_wg_sum(double v, double* sh) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    __syncthreads();                                           // (the previous sum's readers are done with sh)
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

// repeat_interval: per unique edge with c > 1 occurrences in the prefix its mean inter-occurrence interval, which telescopes to
// (t[last] - t[first]) / (c - 1).  Thread k of workgroup w takes edges w * 256 + k, + gridDim.x * 256, ... in ascending order.
__global__ __launch_bounds__(256) void k_eb_stats(EbTable tb, uint32_t h, double* __restrict__ part) {
    __shared__ double sh[4];
    const uint32_t U = tb.hdr[EB_U];
    double acc = 0.0;
    for (uint32_t u = blockIdx.x * 256u + threadIdx.x; u < U; u += gridDim.x * 256u) {
        uint32_t lo;
        const uint32_t c = eb_count(tb, u, h, lo);
        if (c > 1u) acc += (tb.t[tb.pos[lo + c - 1u]] - tb.t[tb.pos[lo]]) / (double)(c - 1u);
    }
    acc = eb_wg_sum(acc, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = acc;
}

// np.quantile(t[:h], q), method 'linear', on the sorted prefix: NumPy's _lerp, both branches, every operation rounded on its own
__device__ __forceinline__ double eb_quantile(const double* __restrict__ t, uint32_t h, double q) {
    const double v = __dmul_rn((double)(h - 1u), q);
    const double fl = floor(v);
    uint32_t i = (uint32_t)fl;
    if (i > h - 1u) i = h - 1u;
    const double g = __dsub_rn(v, fl);
    const double a = t[i], b = t[i + 1u < h ? i + 1u : h - 1u];
    const double d = __dsub_rn(b, a);
    return g >= 0.5 ? __dsub_rn(b, __dmul_rn(d, __dsub_rn(1.0, g))) : __dadd_rn(a, __dmul_rn(d, g));
}

// One thread per query of the two lists (list 0 first).  Prologue, the same in every workgroup: the window start or the threshold.
__global__ __launch_bounds__(256) void k_eb_predict(EbTable tb, uint32_t h, int memory_mode, int window_mode, double q,
                                                    const double* __restrict__ part, uint32_t n_part,
                                                    const int64_t* __restrict__ src0, const int64_t* __restrict__ dst0, int64_t Q0,
                                                    float* __restrict__ out0, const int64_t* __restrict__ src1,
                                                    const int64_t* __restrict__ dst1, int64_t Q1, float* __restrict__ out1,
                                                    double* __restrict__ out_window) {
    __shared__ double shp[EB_STAT_WGS];
    const uint32_t U = tb.hdr[EB_U];
    const double n_present = (double)tb.present[h];
    const double t_end = tb.t[h - 1u];
    double bound = -__builtin_inf();                           // unlimited: every seen edge is remembered
    if (memory_mode == TPNET_EB_TIME_WINDOW) {
        if (window_mode == TPNET_EB_FIXED_PROPORTION) {
            bound = eb_quantile(tb.t, h, q);
        } else {
            shp[threadIdx.x] = threadIdx.x < n_part ? part[threadIdx.x] : 0.0;                  // n_part <= 256
            __syncthreads();
            if (threadIdx.x == 0) {                            // the workgroups' partials in index order
                double acc = 0.0;
                for (uint32_t w = 0; w < n_part; ++w) acc += shp[w];
                shp[0] = acc;
            }
            __syncthreads();
            const double S = shp[0];
            bound = __dsub_rn(t_end, __ddiv_rn(S, n_present));
        }
    } else if (memory_mode == TPNET_EB_REPEAT_THRESHOLD) {
        bound = __ddiv_rn((double)h, n_present);
    }
    if (out_window && blockIdx.x == 0 && threadIdx.x == 0) {
        out_window[0] = bound;
        out_window[1] = memory_mode == TPNET_EB_REPEAT_THRESHOLD ? n_present : t_end;
    }
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= Q0 + Q1) return;
    const bool second = i >= Q0;
    const int64_t k = second ? i - Q0 : i;
    const int64_t s = second ? src1[k] : src0[k], d = second ? dst1[k] : dst0[k];
    float p = 0.0f;
    if ((uint64_t)s < (1ull << 31) && (uint64_t)d < (1ull << 31)) {      // no edge of the table has another id
        const uint64_t key = ((uint64_t)s << 32) | (uint64_t)d;
        uint32_t lo = 0, hi = U;
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (tb.ukey[mid] < key) lo = mid + 1; else hi = mid;
        }
        if (lo < U && tb.ukey[lo] == key) {
            uint32_t l0;
            const uint32_t c = eb_count(tb, lo, h, l0);
            if (c > 0u) {
                if (memory_mode == TPNET_EB_TIME_WINDOW) p = tb.t[tb.pos[l0 + c - 1u]] >= bound ? 1.0f : 0.0f;
                else if (memory_mode == TPNET_EB_REPEAT_THRESHOLD) p = (double)c >= bound ? 1.0f : 0.0f;
                else p = 1.0f;
            }
        }
    }
    (second ? out1 : out0)[k] = p;
}

// ---- layout ----------------------------------------------------------------------------------------------------------------------
struct EbView {
    uint32_t* hdr; uint64_t* ukey; uint32_t* ustart; uint32_t* pos; double* t; uint32_t* present;
    uint64_t* k_a; uint64_t* k_b; uint32_t* ix_a; uint8_t* first; uint32_t* blk; Arena::Span tmp;       // build only
};
static void eb_layout(Arena& a, EbView& v, int64_t E) {
    const size_t n = (size_t)(E < 1 ? 1 : E);
    a.head();
    v.hdr = a.take<uint32_t>(64);
    v.ukey = a.take<uint64_t>(n);
    v.ustart = a.take<uint32_t>(n + 1);
    v.pos = a.take<uint32_t>(n);
    v.t = a.take<double>(n);
    v.present = a.take<uint32_t>(n + 1);
    v.k_a = a.take<uint64_t>(n);
    v.k_b = a.take<uint64_t>(n);
    v.ix_a = a.take<uint32_t>(n);
    v.first = a.take<uint8_t>(n);
    v.blk = a.take<uint32_t>(n / 256 + 2);
    v.tmp = a.rest();
    a.skip(sort_pairs_tmp<uint64_t, uint32_t>(n));
    a.skip(256);                                     // tail slack
}
static EbView eb_view(const void* eb, size_t bytes, int64_t E) {
    Arena a(const_cast<void*>(eb), bytes);
    EbView v;
    eb_layout(a, v, E);
    return v;
}
static EbTable eb_table(const EbView& v) { return {v.hdr, v.ukey, v.ustart, v.pos, v.t, v.present}; }
// the scratch of the repeat-interval statistics: one partial sum per workgroup of k_eb_stats
static double* eb_scratch_layout(Arena& a) {
    a.head();
    return a.take<double>(EB_STAT_WGS);
}

}  // namespace tpnet

using namespace tpnet;

extern "C" {

size_t tpnet_edgebank_bytes(int64_t E) {
    if (E < 1 || E >= (1ll << 30)) return 0;
    return measured([&](Arena& a) { EbView v; eb_layout(a, v, E); });
}

int tpnet_edgebank_build(void* eb, size_t bytes, const int64_t* src, const int64_t* dst, const double* t, int64_t E, int64_t* counts,
                         void* stream) {
    if (!eb || !src || !dst || !t || !counts || E < 1 || E >= (1ll << 30)) return TPNET_ERR_BAD_ARG;
    if (bytes < tpnet_edgebank_bytes(E)) return TPNET_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    EbView v = eb_view(eb, bytes, E);
    const size_t n = (size_t)E;
    const uint32_t n32 = (uint32_t)E;
    const int grid = grid_1d(E, 4096);
    TPNET_HIP_TRY(hipMemsetAsync(v.hdr, 0, 256, s));
    TPNET_HIP_TRY(hipMemsetAsync(v.first, 0, n, s));
    hipLaunchKernelGGL(k_eb_keys, dim3(grid), dim3(256), 0, s, src, dst, t, E, v.k_a, v.ix_a, v.t, v.hdr);
    // ONE stable sort by (src, dst) with the position as payload: positions come out ascending inside each key
    TPNET_HIP_TRY(rocprim::radix_sort_pairs(v.tmp.ptr, v.tmp.bytes, v.k_a, v.k_b, v.ix_a, v.pos, n, 0u, 64u, s, false));
    // the unique edges (head flags in key order), then the distinct edges per prefix (first occurrences in position order)
    scan_compact(EbHead{v.k_b}, EbEmit{v.k_b, v.pos, v.ukey, v.ustart, v.first}, nullptr, n32, v.blk, v.hdr + EB_U, grid, s);
    scan_count(EbFirst{v.first}, nullptr, n32, v.blk, v.hdr + EB_FIRSTS, grid, s);
    hipLaunchKernelGGL(k_eb_present, dim3(grid), dim3(256), 0, s, (const uint8_t*)v.first, n32, (const uint32_t*)v.blk,
                       (const uint32_t*)v.hdr, v.present, v.ustart);
    TPNET_HIP_TRY(hipGetLastError());
    uint32_t h[4] = {0};
    TPNET_HIP_TRY(hipMemcpyAsync(h, v.hdr, sizeof(h), hipMemcpyDeviceToHost, s));
    TPNET_HIP_TRY(hipStreamSynchronize(s));
    if (h[EB_BAD]) return TPNET_ERR_INDEX;
    if (h[EB_DEC]) return TPNET_ERR_BAD_ARG;
    counts[0] = h[EB_U];
    return TPNET_OK;
}

size_t tpnet_edgebank_scratch_bytes(int64_t E) {
    if (E < 1 || E >= (1ll << 30)) return 0;
    return measured([](Arena& a) { (void)eb_scratch_layout(a); });
}

int tpnet_edgebank_predict(const void* eb, int64_t E, int32_t memory_mode, int32_t window_mode, double proportion, int64_t h,
                           const int64_t* src0, const int64_t* dst0, int64_t Q0, float* out0, const int64_t* src1, const int64_t* dst1,
                           int64_t Q1, float* out1, void* scratch, size_t scratch_bytes, double* out_window, void* stream) {
    if (!eb || E < 1 || E >= (1ll << 30) || h < 1 || h > E || !(proportion >= 0.0 && proportion <= 1.0) ||
        memory_mode < TPNET_EB_UNLIMITED || memory_mode > TPNET_EB_REPEAT_THRESHOLD || window_mode < TPNET_EB_FIXED_PROPORTION ||
        window_mode > TPNET_EB_REPEAT_INTERVAL || Q0 < 0 || Q1 < 0 || Q0 >= (1ll << 31) || Q1 >= (1ll << 31) ||
        (Q0 > 0 && (!src0 || !dst0 || !out0)) || (Q1 > 0 && (!src1 || !dst1 || !out1)))
        return TPNET_ERR_BAD_ARG;
    const bool stats = memory_mode == TPNET_EB_TIME_WINDOW && window_mode == TPNET_EB_REPEAT_INTERVAL;
    if (stats && !scratch) return TPNET_ERR_BAD_ARG;
    if (stats && scratch_bytes < tpnet_edgebank_scratch_bytes(E)) return TPNET_ERR_WORKSPACE;
    if (Q0 + Q1 == 0) return TPNET_OK;
    hipStream_t s = (hipStream_t)stream;
    const EbTable tb = eb_table(eb_view(eb, 0, E));
    double* part = nullptr;
    uint32_t n_part = 0;
    if (stats) {
        Arena a(scratch, scratch_bytes);
        part = eb_scratch_layout(a);
        n_part = (uint32_t)grid_1d(E, EB_STAT_WGS);
        hipLaunchKernelGGL(k_eb_stats, dim3(n_part), dim3(256), 0, s, tb, (uint32_t)h, part);
    }
    hipLaunchKernelGGL(k_eb_predict, dim3((unsigned)((Q0 + Q1 + 255) / 256)), dim3(256), 0, s, tb, (uint32_t)h, (int)memory_mode,
                       (int)window_mode, 1.0 - proportion, (const double*)part, n_part, src0, dst0, Q0, out0, src1, dst1, Q1, out1,
                       out_window);
    TPNET_HIP_TRY(hipGetLastError());
    return TPNET_OK;
}

}  // extern "C"
