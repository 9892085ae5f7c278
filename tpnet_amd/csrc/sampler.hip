// Device-side 'recent' neighbour sampler: the step in front of the hot path.  The reference builds
// per-node time-sorted adjacency lists on the host and, per query, runs np.searchsorted + a last-K slice in a Python
// loop over the batch (utils/utils.py:140-152, 160-224, 293-312).  Here: one CSR of the undirected interaction graph
// (stable sort by (node, time), ties in the reference's append order) and one thread per (query, slot).  The two random strategies
// ('uniform', 'time_interval_aware') draw from the same CSR with a counter-based generator: k_sampler_weights / k_sample_random.
#include "tpnet_common.h"
#include "draw_common.hpp"
#include "arena.hpp"
#include "sort_tmp.hpp"

#include <cstring>

namespace tpnet {

// entry 2e = (node src[e] -> neighbour dst[e]), entry 2e+1 = (node dst[e] -> neighbour src[e]): the reference's
// append order (utils/utils.py:307-309)
__global__ void k_adj_keys(const int64_t* __restrict__ src, const int64_t* __restrict__ dst,
                           const double* __restrict__ t, int64_t E, uint64_t* __restrict__ tkey,
                           uint32_t* __restrict__ idx) {
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < 2 * E; j += (int64_t)gridDim.x * blockDim.x) {
        tkey[j] = time_key(t[j >> 1]);
        idx[j] = (uint32_t)j;
    }
}

__global__ void k_adj_nodekeys(const int64_t* __restrict__ src, const int64_t* __restrict__ dst, int64_t E,
                               const uint32_t* __restrict__ idx, uint32_t* __restrict__ nkey) {
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < 2 * E; j += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t o = idx[j];
        nkey[j] = (uint32_t)((o & 1u) ? dst[o >> 1] : src[o >> 1]);
    }
}

// sorted order -> CSR payload (neighbour, edge id, time) and row starts
__global__ void k_adj_fill(const int64_t* __restrict__ src, const int64_t* __restrict__ dst,
                           const double* __restrict__ t, const int64_t* __restrict__ eid, int64_t E,
                           const uint32_t* __restrict__ nkey_sorted, const uint32_t* __restrict__ idx_sorted,
                           int64_t num_nodes, int64_t* __restrict__ row_start, int32_t* __restrict__ nbr,
                           int64_t* __restrict__ nbr_eid, double* __restrict__ nbr_t) {
    const int64_t n2 = 2 * E;
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n2; j += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t o = idx_sorted[j];
        const int64_t e = o >> 1;
        nbr[j] = (int32_t)((o & 1u) ? src[e] : dst[e]);
        nbr_eid[j] = eid ? eid[e] : e + 1;
        nbr_t[j] = t[e];
        const uint32_t k = nkey_sorted[j];
        const uint32_t kp = j ? nkey_sorted[j - 1] : 0xFFFFFFFFu;
        if (j == 0 || k != kp) {
            // nodes (kp, k] start here (empty lists in between)
            const int64_t first = (j == 0) ? 0 : (int64_t)kp + 1;
            for (int64_t q = first; q <= (int64_t)k && q <= num_nodes; ++q) row_start[q] = j;
        }
        if (j == n2 - 1)
            for (int64_t q = (int64_t)k + 1; q <= num_nodes; ++q) row_start[q] = n2;
    }
}

__global__ void k_adj_empty(int64_t num_nodes, int64_t* __restrict__ row_start) {
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q <= num_nodes; q += (int64_t)gridDim.x * blockDim.x)
        row_start[q] = 0;
}

// one thread per (query, slot): cut = first interaction of the node with time >= query time (searchsorted left,
// utils/utils.py:152); the K most recent before it go to the BACK of the row, the front is padded with 0 (:211-219)
__global__ void k_sample_recent(const int64_t* __restrict__ row_start, const int32_t* __restrict__ nbr,
                                const int64_t* __restrict__ nbr_eid, const double* __restrict__ nbr_t,
                                int64_t num_nodes, const int64_t* __restrict__ node_ids,
                                const double* __restrict__ times, int64_t n, int K, int64_t* __restrict__ out_ids,
                                int64_t* __restrict__ out_eids, double* __restrict__ out_t) {
    const int64_t tot = n * K;
    for (int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; x < tot; x += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = x / K;
        const int k = (int)(x - i * K);
        const int64_t nid = node_ids[i];
        int64_t id = 0, ee = 0;
        double tt = 0.0;
        if ((uint64_t)nid < (uint64_t)num_nodes) {
            const int64_t lo0 = row_start[nid], hi0 = row_start[nid + 1];
            const double q = times[i];
            int64_t lo = lo0, hi = hi0;
            while (lo < hi) {
                const int64_t mid = (lo + hi) >> 1;
                if (nbr_t[mid] < q) lo = mid + 1; else hi = mid;
            }
            const int64_t cut = lo;
            const int64_t pos = cut - K + k;          // slot k of the K-wide window ending at cut
            if (pos >= lo0) {
                id = nbr[pos];
                ee = nbr_eid[pos];
                tt = nbr_t[pos];
            }
        }
        out_ids[x] = id;
        if (out_eids) out_eids[x] = ee;
        if (out_t) out_t[x] = tt;
    }
}

// ---- the reference's random strategies, 'uniform' and 'time_interval_aware' (utils/utils.py:123-224) ----

// The weights table of 'time_interval_aware', once per sampler: one workgroup per node walks the node's time-sorted list in
// chunks of 256 with two running carries.  E_j = exp(s (t_j - t_last)) and p_j = E_j / cumsum(E)_j in float64 over the WHOLE
// list (compute_sampled_probabilities, utils/utils.py:123-139); the reference then takes softmax(float32(p[:n])) with NaN -> -1e10
// (:194), i.e. P(j) ~ w_j = exp((double)(float)p_j) and 0 for a NaN p_j; W = the node's inclusive prefix sum of w.
__global__ __launch_bounds__(256) void k_sampler_weights(const int64_t* __restrict__ row_start, const double* __restrict__ nbr_t,
                                                         int64_t num_nodes, double s, double* __restrict__ W) {
    __shared__ double sh[4];
    for (int64_t node = blockIdx.x; node < num_nodes; node += gridDim.x) {
        const int64_t lo = row_start[node], hi = row_start[node + 1];
        if (hi <= lo) continue;                                   // (block-uniform)
        const double t_last = nbr_t[hi - 1];
        double carry_e = 0.0, carry_w = 0.0;
        for (int64_t base = lo; base < hi; base += 256) {
            const int64_t j = base + threadIdx.x;
            const double e = j < hi ? exp(s * (nbr_t[j] - t_last)) : 0.0;
            double tot_e, tot_w;
            const double ce = carry_e + wg_scan256(e, sh, tot_e);
            const double p = e / ce;
            const double w = (j < hi && p == p) ? exp((double)(float)p) : 0.0;
            const double cw = carry_w + wg_scan256(w, sh, tot_w);
            if (j < hi) W[j] = cw;
            carry_e += tot_e;
            carry_w += tot_w;
        }
    }
}

// One workgroup holds 256 / K whole rows (one row when K > 128); thread = (row, slot).  The row's first lane does the cut search
// and shares (row start, prefix length, total weight) through LDS; every thread draws its position, and after a barrier finds its
// rank among the row's K positions (smaller positions, plus equal ones in lower slots) and writes its triple to output slot `rank`:
// the row comes out in ascending CSR position, which is a time sort.  W == nullptr: uniform.
__global__ __launch_bounds__(256) void k_sample_random(const int64_t* __restrict__ row_start, const int32_t* __restrict__ nbr,
                                                       const int64_t* __restrict__ nbr_eid, const double* __restrict__ nbr_t,
                                                       const double* __restrict__ W, int64_t num_nodes,
                                                       const int64_t* __restrict__ node_ids, const double* __restrict__ times,
                                                       int64_t n, int K, int rows_per_wg, uint32_t k0, uint32_t k1,
                                                       uint32_t call_index, int64_t* __restrict__ out_ids,
                                                       int64_t* __restrict__ out_eids, double* __restrict__ out_t) {
    __shared__ int64_t s_lo[256];
    __shared__ uint32_t s_len[256];
    __shared__ double s_wtot[256];
    __shared__ uint32_t s_pos[256];
    const int tid = threadIdx.x;
    const int r = tid / K, slot = tid - r * K;
    const int64_t row = (int64_t)blockIdx.x * rows_per_wg + r;
    const bool live = r < rows_per_wg && row < n;
    if (live && slot == 0) {
        const int64_t nid = node_ids[row];
        int64_t lo0 = 0, cut = 0;
        if ((uint64_t)nid < (uint64_t)num_nodes) {
            lo0 = row_start[nid];
            const double q = times[row];
            int64_t lo = lo0, hi = row_start[nid + 1];
            while (lo < hi) {
                const int64_t mid = (lo + hi) >> 1;
                if (nbr_t[mid] < q) lo = mid + 1; else hi = mid;
            }
            cut = lo;
        }
        s_lo[r] = lo0;
        s_len[r] = (uint32_t)(cut - lo0);                       // (2E < 2^31: tpnet_sampler_build)
        s_wtot[r] = (W && cut > lo0) ? W[cut - 1] : 0.0;
    }
    __syncthreads();
    const int64_t lo0 = live ? s_lo[r] : 0;
    const uint32_t len = live ? s_len[r] : 0u;
    uint32_t pos = 0;
    if (len) {
        const uint32_t rnd = philox_word((uint32_t)row, (uint32_t)((uint64_t)row >> 32), (uint32_t)slot >> 2, call_index, k0, k1,
                                         slot & 3);
        const double wtot = s_wtot[r];
        if (wtot > 0.0) {
            const double x = ((double)rnd + 0.5) * 0x1p-32 * wtot;
            uint32_t a = 0, b = len - 1;                          // first j with W[j] >= x, clamped to the prefix's last entry
            while (a < b) {
                const uint32_t mid = (a + b) >> 1;
                if (W[lo0 + mid] < x) a = mid + 1; else b = mid;
            }
            pos = a;
        } else {
            pos = (uint32_t)(((uint64_t)rnd * (uint64_t)len) >> 32);
        }
    }
    s_pos[tid] = pos;
    __syncthreads();
    if (!live) return;
    const int64_t o = row * K;
    if (!len) {
        out_ids[o + slot] = 0;
        if (out_eids) out_eids[o + slot] = 0;
        if (out_t) out_t[o + slot] = 0.0;
        return;
    }
    int rank = 0;
    const uint32_t* rp = s_pos + r * K;
    for (int k = 0; k < K; ++k) {
        const uint32_t pk = rp[k];
        rank += (pk < pos || (pk == pos && k < slot)) ? 1 : 0;
    }
    const int64_t j = lo0 + pos;
    out_ids[o + rank] = nbr[j];
    if (out_eids) out_eids[o + rank] = nbr_eid[j];
    if (out_t) out_t[o + rank] = nbr_t[j];
}

// the encoder's rows for one (src, other) batch (models/TPNet.py:280-316): nodes = [src; other], times = tile(t, 2), and the
// two anchors of row i = the edge's endpoints (src[i % B], other[i % B])
__global__ void k_encoder_rows(const int64_t* __restrict__ src, const int64_t* __restrict__ other, const double* __restrict__ t,
                               int64_t B, int64_t* __restrict__ nodes, double* __restrict__ t2, int64_t* __restrict__ a1,
                               int64_t* __restrict__ a2) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < 2 * B; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t e = i < B ? i : i - B;
        const int64_t s = src[e], o = other[e];
        nodes[i] = i < B ? s : o;
        t2[i] = t[e];
        a1[i] = s;
        a2[i] = o;
    }
}

// the two kernels above in ONE launch for the encoder's call (round 3): thread (row i, slot k) derives the row's node and time
// from the batch itself (three loads that a wave shares: its 64 threads span 3-4 rows), slot 0 also writes the row's record
// (node, time, anchors); then the sampler's cut and window as in k_sample_recent.  One launch less per encoder call (~5 us each).
__global__ void k_encoder_sample(const int64_t* __restrict__ row_start, const int32_t* __restrict__ nbr,
                                 const double* __restrict__ nbr_t, int64_t num_nodes, const int64_t* __restrict__ src,
                                 const int64_t* __restrict__ other, const double* __restrict__ t, int64_t B, int K,
                                 int64_t* __restrict__ nodes, double* __restrict__ t2, int64_t* __restrict__ a1,
                                 int64_t* __restrict__ a2, int64_t* __restrict__ out_ids, int64_t* __restrict__ pu,
                                 int64_t* __restrict__ pv) {
    const int64_t tot = 2 * B * K;
    for (int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; x < tot; x += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = x / K;
        const int k = (int)(x - i * K);
        const int64_t e = i < B ? i : i - B;
        const int64_t sn = src[e], on = other[e];
        const double q = t[e];
        const int64_t nid = i < B ? sn : on;
        if (k == 0) {
            nodes[i] = nid;
            t2[i] = q;
            a1[i] = sn;
            a2[i] = on;
        }
        int64_t id = 0;
        if ((uint64_t)nid < (uint64_t)num_nodes) {
            const int64_t lo0 = row_start[nid], hi0 = row_start[nid + 1];
            int64_t lo = lo0, hi = hi0;
            while (lo < hi) {
                const int64_t mid = (lo + hi) >> 1;
                if (nbr_t[mid] < q) lo = mid + 1; else hi = mid;
            }
            const int64_t pos = lo - K + k;           // slot k of the K-wide window ending at the cut
            if (pos >= lo0) id = nbr[pos];
        }
        out_ids[x] = id;
        if (pu) {
            // narrow rows: the call's pairs spelled out, (neighbour, src) then (neighbour, other) -- get_pair_wise_feature's own
            // order (models/TPNet.py:311-316) -- for the generic readout, which beats the anchored walk on rows of <= 128 floats
            pu[x] = id;
            pu[tot + x] = id;
            pv[x] = sn;
            pv[tot + x] = on;
        }
    }
}

}  // namespace tpnet

using namespace tpnet;

extern "C" {

// Layout of the sampler buffer (caller-owned device memory of tpnet_sampler_bytes): the CSR, which is all a sampling call reads,
// and the scratch of the build behind it.
struct SamplerView {
    int64_t* row_start; int32_t* nbr; int64_t* nbr_eid; double* nbr_t;
    uint64_t* tk_a; uint64_t* tk_b; uint32_t* ix_a; uint32_t* ix_b; uint32_t* nk_a; uint32_t* nk_b; Arena::Span tmp;
};
static void csr_layout(Arena& a, SamplerView& v, int64_t E, int64_t num_nodes) {
    const size_t n2 = 2 * (size_t)(E < 1 ? 1 : E);
    a.head();
    v.row_start = a.take<int64_t>((size_t)(num_nodes + 1));
    v.nbr = a.take<int32_t>(n2);
    v.nbr_eid = a.take<int64_t>(n2);
    v.nbr_t = a.take<double>(n2);
}
static void sampler_layout(Arena& a, SamplerView& v, int64_t E, int64_t num_nodes) {
    const size_t n2 = 2 * (size_t)(E < 1 ? 1 : E);
    csr_layout(a, v, E, num_nodes);
    v.tk_a = a.take<uint64_t>(n2);
    v.tk_b = a.take<uint64_t>(n2);
    v.ix_a = a.take<uint32_t>(n2);
    v.ix_b = a.take<uint32_t>(n2);
    v.nk_a = a.take<uint32_t>(n2);
    v.nk_b = a.take<uint32_t>(n2);
    v.tmp = a.rest();
    const size_t t1 = sort_pairs_tmp<uint64_t, uint32_t>(n2), t2 = sort_pairs_tmp<uint32_t, uint32_t>(n2);
    a.skip(t1 > t2 ? t1 : t2);
}
static SamplerView csr_view(const void* sampler, int64_t E, int64_t num_nodes) {
    Arena a(const_cast<void*>(sampler), 0);
    SamplerView v{};
    csr_layout(a, v, E, num_nodes);
    return v;
}
// W[2E] doubles (the scan keeps its carries in registers)
static double* weights_layout(Arena& a, int64_t E) {
    a.head();
    return a.take<double>(2 * (size_t)(E < 1 ? 1 : E));
}

size_t tpnet_sampler_bytes(int64_t E, int64_t num_nodes) {
    return measured([&](Arena& a) { SamplerView v; sampler_layout(a, v, E, num_nodes); });
}

int tpnet_sampler_build(void* sampler, size_t sampler_bytes, const int64_t* src, const int64_t* dst, const double* t,
                        const int64_t* edge_ids, int64_t E, int64_t num_nodes, void* stream) {
    if (!sampler || E < 0 || num_nodes < 1 || num_nodes >= (1ll << 31) || (E > 0 && (!src || !dst || !t)))
        return TPNET_ERR_BAD_ARG;
    if (E >= (1ll << 30)) return TPNET_ERR_BAD_ARG;
    if (sampler_bytes < tpnet_sampler_bytes(E, num_nodes)) return TPNET_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    Arena a(sampler, sampler_bytes);
    SamplerView v;
    sampler_layout(a, v, E, num_nodes);
    if (E == 0) {
        hipLaunchKernelGGL(k_adj_empty, dim3(64), dim3(256), 0, s, num_nodes, v.row_start);
        TPNET_HIP_TRY(hipGetLastError());
        return TPNET_OK;
    }
    const size_t n2 = 2 * (size_t)E;
    const int grid = grid_1d((int64_t)n2, 4096);
    // stable sort by time, then stable sort by node  ==  sort by (node, time) with ties in append order
    hipLaunchKernelGGL(k_adj_keys, dim3(grid), dim3(256), 0, s, src, dst, t, E, v.tk_a, v.ix_a);
    TPNET_HIP_TRY(rocprim::radix_sort_pairs(v.tmp.ptr, v.tmp.bytes, v.tk_a, v.tk_b, v.ix_a, v.ix_b, n2, 0u, 64u, s, false));
    hipLaunchKernelGGL(k_adj_nodekeys, dim3(grid), dim3(256), 0, s, src, dst, E, v.ix_b, v.nk_a);
    int bits = 1;
    while ((1ll << bits) < num_nodes && bits < 32) ++bits;
    TPNET_HIP_TRY(rocprim::radix_sort_pairs(v.tmp.ptr, v.tmp.bytes, v.nk_a, v.nk_b, v.ix_b, v.ix_a, n2, 0u, (unsigned)bits, s, false));
    hipLaunchKernelGGL(k_adj_fill, dim3(grid), dim3(256), 0, s, src, dst, t, edge_ids, E, v.nk_b, v.ix_a, num_nodes,
                       v.row_start, v.nbr, v.nbr_eid, v.nbr_t);
    TPNET_HIP_TRY(hipGetLastError());
    return TPNET_OK;
}

int tpnet_sample_recent(const void* sampler, int64_t E, int64_t num_nodes, const int64_t* node_ids, const double* times,
                        int64_t n, int32_t K, int64_t* out_ids, int64_t* out_eids, double* out_times, void* stream) {
    if (!sampler || n < 0 || K < 1 || num_nodes < 1 || (n > 0 && (!node_ids || !times || !out_ids)))
        return TPNET_ERR_BAD_ARG;
    if (n == 0) return TPNET_OK;
    SamplerView v = csr_view(sampler, E, num_nodes);
    const int grid = grid_1d(n * (int64_t)K, 8192);
    hipLaunchKernelGGL(k_sample_recent, dim3(grid), dim3(256), 0, (hipStream_t)stream, v.row_start, v.nbr, v.nbr_eid,
                       v.nbr_t, num_nodes, node_ids, times, n, (int)K, out_ids, out_eids, out_times);
    TPNET_HIP_TRY(hipGetLastError());
    return TPNET_OK;
}

size_t tpnet_sampler_weights_bytes(int64_t E) {
    return measured([&](Arena& a) { (void)weights_layout(a, E); });
}

int tpnet_sampler_build_weights(const void* sampler, int64_t E, int64_t num_nodes, double time_scaling_factor, void* weights,
                                size_t weights_bytes, void* stream) {
    if (!sampler || !weights || E < 0 || E >= (1ll << 30) || num_nodes < 1 || num_nodes >= (1ll << 31)) return TPNET_ERR_BAD_ARG;
    if (weights_bytes < tpnet_sampler_weights_bytes(E)) return TPNET_ERR_WORKSPACE;
    if (E == 0) return TPNET_OK;
    SamplerView v = csr_view(sampler, E, num_nodes);
    Arena wa(weights, weights_bytes);
    double* W = weights_layout(wa, E);
    const int grid = (int)(num_nodes < 8192 ? num_nodes : 8192);
    hipLaunchKernelGGL(k_sampler_weights, dim3(grid), dim3(256), 0, (hipStream_t)stream, v.row_start, v.nbr_t, num_nodes,
                       time_scaling_factor, W);
    TPNET_HIP_TRY(hipGetLastError());
    return TPNET_OK;
}

int tpnet_sample_random(const void* sampler, const void* weights, int64_t E, int64_t num_nodes, const int64_t* node_ids,
                        const double* times, int64_t n, int32_t K, uint64_t seed, uint32_t call_index, int64_t* out_ids,
                        int64_t* out_eids, double* out_times, void* stream) {
    if (!sampler || n < 0 || K < 1 || K > 256 || E < 0 || num_nodes < 1 || (n > 0 && (!node_ids || !times || !out_ids)))
        return TPNET_ERR_BAD_ARG;
    if (n == 0) return TPNET_OK;
    const int rows_per_wg = 256 / K;                             // whole rows per workgroup (K > 128: one)
    const int64_t grid = (n + rows_per_wg - 1) / rows_per_wg;
    if (grid > 0x7fffffffll) return TPNET_ERR_BAD_ARG;
    SamplerView v = csr_view(sampler, E, num_nodes);
    Arena wa(const_cast<void*>(weights), 0);
    const double* W = (weights && E > 0) ? weights_layout(wa, E) : nullptr;
    hipLaunchKernelGGL(k_sample_random, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, v.row_start, v.nbr, v.nbr_eid,
                       v.nbr_t, W, num_nodes, node_ids, times, n, (int)K, rows_per_wg, (uint32_t)seed, (uint32_t)(seed >> 32),
                       call_index, out_ids, out_eids, out_times);
    TPNET_HIP_TRY(hipGetLastError());
    return TPNET_OK;
}

size_t tpnet_encoder_scratch_bytes(int64_t B, int32_t K) {
    if (B < 0) B = 0;
    if (K < 1) K = 1;
    return (size_t)(8 * B + 10 * B * (int64_t)K) * 8 + 256;       // (+ the spelled-out pair lists of narrow rows: 2 x 4 B K ids)
}

int tpnet_encoder_rows(const tpnet_state* st, const void* sampler, int64_t E, int64_t num_nodes, const int64_t* src,
                       const int64_t* other, const double* t, int64_t B, int32_t K, void* scratch, size_t scratch_bytes,
                       void* stream) {
    return encoder_rows(st, sampler, E, num_nodes, src, other, t, B, K, 0, scratch, scratch_bytes, stream);
}

}  // extern "C"

int tpnet::encoder_rows(const tpnet_state* st, const void* sampler, int64_t E, int64_t num_nodes, const int64_t* src,
                        const int64_t* other, const double* t, int64_t B, int32_t K, uint32_t flags, void* scratch,
                        size_t scratch_bytes, void* stream) {
    if (!st || !sampler || B < 0 || K < 1 || num_nodes < 1 || (B > 0 && (!src || !other || !t || !scratch))) return TPNET_ERR_BAD_ARG;
    if (B == 0) return TPNET_OK;
    if (scratch_bytes < tpnet_encoder_scratch_bytes(B, K)) return TPNET_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    int64_t* nodes = (int64_t*)align256((size_t)scratch);
    double* t2 = (double*)(nodes + 2 * B);
    int64_t* a1 = (int64_t*)(t2 + 2 * B);
    int64_t* a2 = a1 + 2 * B;
    int64_t* neigh = a2 + 2 * B;
    static const int two = TPNET_DEV_INT(ENCODER_TWO_LAUNCHES, 0);     // developer override: row set-up and sampler apart
    if (two) {
        hipLaunchKernelGGL(k_encoder_rows, dim3(grid_1d(2 * B, 1024)), dim3(256), 0, s, src, other, t, B, nodes, t2, a1, a2);
        return tpnet_sample_recent(sampler, E, num_nodes, nodes, t2, 2 * B, K, neigh, nullptr, nullptr, stream);
    }
    SamplerView v = csr_view(sampler, E, num_nodes);
    const int grid = grid_1d(2 * B * (int64_t)K, 8192);
    // (the call's pairs spelled out behind the neighbour ids: only where the generic pair kernel will read them)
    int64_t* pu = anchored_route(*st, 2 * B, K, flags, nullptr, true, true).gram == AK_GENERIC ? neigh + 2 * B * (int64_t)K : nullptr;
    hipLaunchKernelGGL(k_encoder_sample, dim3(grid), dim3(256), 0, s, v.row_start, v.nbr, v.nbr_t, num_nodes, src, other, t, B, (int)K,
                       nodes, t2, a1, a2, neigh, pu, pu ? pu + 4 * B * (int64_t)K : nullptr);
    TPNET_HIP_TRY(hipGetLastError());
    return TPNET_OK;
}

extern "C" {

int tpnet_encoder_gram(const tpnet_state* st, const void* sampler, int64_t E, int64_t num_nodes, const int64_t* src,
                       const int64_t* other, const double* t, int64_t B, int32_t K, double now_time, double lambda,
                       uint32_t flags, void* scratch, size_t scratch_bytes, float* out, void* stream) {
    if (!st || !out) return TPNET_ERR_BAD_ARG;
    if (flags & TPNET_FLAG_PACKED) return TPNET_ERR_BAD_ARG;
    if (B == 0) return TPNET_OK;
    if (check_state(st)) return TPNET_ERR_BAD_ARG;
    // (TPNET_FLAG_LAYERS_MFMA needs 16-byte aligned outputs; without them the call is the one without the flag, pair lists included)
    if (!aligned16({out})) flags &= ~TPNET_FLAG_LAYERS_MFMA;
    // needs what tpnet_pair_gram_anchored serves -- also on narrow rows, which the generic kernel then takes from the pair lists
    if (anchored_route(*st, 2 * B, K, flags, nullptr, true, false).gram == AK_REFUSED) return TPNET_ERR_BAD_ARG;
    int rc = encoder_rows(st, sampler, E, num_nodes, src, other, t, B, K, flags, scratch, scratch_bytes, stream);
    if (rc) return rc;
    int64_t* nodes = (int64_t*)align256((size_t)scratch);
    int64_t* a1 = nodes + 4 * B;
    int64_t* a2 = a1 + 2 * B;
    int64_t* neigh = a2 + 2 * B;
    const int NN = 2 * st->L + 2;
    if (anchored_route(*st, 2 * B, K, flags, nullptr, true, true).gram == AK_GENERIC) {
        const int64_t half = 2 * B * (int64_t)K;
        return tpnet_pair_gram(st, neigh + half, neigh + 3 * half, 2 * half, now_time, lambda, flags, out, stream);
    }
    return tpnet_pair_gram_anchored(st, neigh, a1, a2, 2 * B, K, now_time, lambda, flags, out,
                                    out + (size_t)(2 * B) * (size_t)K * (size_t)(NN * NN), stream);
}

}  // extern "C"
