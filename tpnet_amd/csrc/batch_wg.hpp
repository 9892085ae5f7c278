// The phases shared by the kernels that plan ONE batch per workgroup -- k_plan_one, k_plan_one_h (plan.hip), wsort_batch
// (wplan_common.hpp: k_wsort, k_dense_sort), k_dense_group, k_dense_sort_shard (wplan_dense.hip) -- written once.  Each piece
// encodes a rule of the reference (summation order, the f32 casts of the time weight, a bad edge counted once, the clock left by
// the previous batch): a fix is made here.  The kernels keep their own LDS layout, barriers between the pieces and phase stamps.
#pragma once
#include "tpnet_common.h"
#include "device_common.hpp"

namespace tpnet {

// ---- the batch of workgroup bb: edges [e0, e0 + B) of the chunk, sorted positions [2 e0, 2 e0 + 2 B) (as plan_build lays a chunk
// out); a single-batch call is the chunk of one batch
struct BatchSpan {
    int64_t e0;
    int32_t B;
    const int64_t* src;
    const int64_t* dst;
    const double* t;
};
__device__ __forceinline__ BatchSpan batch_span(int64_t bb, const int64_t* __restrict__ src_c, const int64_t* __restrict__ dst_c,
                                                const double* __restrict__ t_c, int64_t Ec, int64_t Bfull) {
    const int64_t e0 = bb * Bfull;
    return {e0, (int32_t)((Ec - e0 < Bfull) ? (Ec - e0) : Bfull), src_c + e0, dst_c + e0, t_c + e0};
}

// ---- edge staging, in two steps: a caller clears its tables while the loads are in flight
template <int EPT>
struct EdgeBurst {
    int64_t s[EPT], d[EPT];
    double t[EPT];
    double t_last;
};
// every thread's edges in ONE burst of independent loads (src / dst / t may sit in host memory: a load is microseconds)
template <int BS, int EPT>
__device__ __forceinline__ EdgeBurst<EPT> edges_load(const BatchSpan& sp) {
    EdgeBurst<EPT> r;
    const int tid = threadIdx.x;
#pragma unroll
    for (int k = 0; k < EPT; ++k) {
        const int e = k * BS + tid;
        const int ec = e < sp.B ? e : sp.B - 1;
        r.s[k] = sp.src[ec];
        r.d[k] = sp.dst[ec];
        r.t[k] = sp.t[ec];
    }
    r.t_last = sp.t[sp.B - 1];                           // next_time = node_interact_times[-1]   (TPNet.py:76)
    return r;
}
// per edge in LDS: endpoints (0 if out of range) | bit 31: the EDGE has a bad endpoint; time weight (0 for a bad edge)
template <int BS, int EPT>
__device__ __forceinline__ void edges_stage(const EdgeBurst<EPT>& r, int32_t B, int64_t N, double lambda, uint32_t* err,
                                            uint32_t* e_src, uint32_t* e_dst, float* e_w) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int k = 0; k < EPT; ++k) {
        const int e = k * BS + tid;
        if (e < B) {
            const int64_t s = r.s[k], dd = r.d[k];
            const bool oks = (uint64_t)s < (uint64_t)N, okd = (uint64_t)dd < (uint64_t)N;
            const uint32_t bad = (oks && okd) ? 0u : 0x80000000u;
            if (bad) atomicAdd(err, 1u);                 // once per bad edge
            e_src[e] = (oks ? (uint32_t)s : 0u) | bad;
            e_dst[e] = (okd ? (uint32_t)dd : 0u) | bad;
            // time weight with the reference's casts: absolute times rounded to f32 BEFORE the subtraction, f32 lambda
            // (models/TPNet.py:77-78), as contribution() of the chunk planner
            const float x = (float)r.t_last - (float)r.t[k];
            e_w[e] = bad ? 0.0f : expf((float)(-lambda) * x);
        }
    }
}

// ---- contribution j of the batch: first the src-side scatter-adds (target src[e] <- partner dst[e]), then the dst-side ones
// (TPNet.py:93-96)
__device__ __forceinline__ uint32_t contrib_target(int j, int B, const uint32_t* e_src, const uint32_t* e_dst) {
    return ((j >= B) ? e_dst[j - B] : e_src[j]) & 0x7FFFFFFFu;
}
__device__ __forceinline__ void contrib_partner_weight(int j, int B, const uint32_t* e_src, const uint32_t* e_dst, const float* e_w,
                                                       int32_t& partner, float& w) {
    const bool side = j >= B;
    const int e = side ? j - B : j;
    const uint32_t es = e_src[e], ed = e_dst[e];
    const bool ok = !(es & 0x80000000u);
    partner = ok ? (int32_t)((side ? es : ed) & 0x7FFFFFFFu) : 0;
    w = ok ? e_w[e] : 0.0f;
}
// keys / payload of the block sort: thread `tid` holds contributions [tid * IPT, tid * IPT + IPT)
template <int IPT>
__device__ __forceinline__ void sort_keys(uint32_t (&keys)[IPT], uint32_t (&vals)[IPT], int nc, int B, int node_bits,
                                          const uint32_t* e_src, const uint32_t* e_dst) {
    const uint32_t pad_key = 1u << node_bits;            // above every node id: padding sorts last
#pragma unroll
    for (int k = 0; k < IPT; ++k) {
        const int j = (int)threadIdx.x * IPT + k;
        vals[k] = (uint32_t)j;
        keys[k] = j < nc ? contrib_target(j, B, e_src, e_dst) : pad_key;
    }
}

// ---- ranks of a group's members by contribution number (the grouping planners).  cb[idx[k]] = span base << 16 | count of the
// group of contribution k * BS + tid; mem[] = the members span by span in arrival order.  A group of up to SMALL is ranked by
// counting its smaller members, a larger one (a hub, listed in big[]) by one wave with a bitmap over j and prefix pop-counts.
// emit(j, span base, rank, count) once per contribution.
template <int BS, int IPT, uint32_t SMALL, typename BigT, typename Emit>
__device__ __forceinline__ void rank_groups(const uint32_t* cb, const uint32_t (&idx)[IPT], int nc, const uint16_t* mem,
                                            const BigT* big, uint32_t nbig, uint32_t (*bm)[BS * IPT / 32], Emit emit) {
    constexpr int NC = BS * IPT, NW = BS / 64, BMW = NC / 32;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int q = 0; q < IPT; ++q) {
        const int j = q * BS + tid;
        if (j < nc) {
            const uint32_t w = cb[idx[q]];
            const uint32_t gb = w >> 16, cnt = w & 0xFFFFu;
            if (cnt <= SMALL) {
                uint32_t rank = 0;
                if (cnt > 1) {
                    for (uint32_t m = 0; m < cnt; m += 4) {          // (four independent LDS reads per round; the span of the
#pragma unroll                                                       //  last group ends inside mem[], a read past a span is masked)
                        for (uint32_t k = 0; k < 4; ++k) {
                            const uint32_t mm = m + k;
                            const uint32_t o = mem[(gb + mm) < (uint32_t)NC ? gb + mm : 0u];
                            rank += (mm < cnt && o < (uint32_t)j) ? 1u : 0u;
                        }
                    }
                }
                emit((uint32_t)j, gb, rank, cnt);
            }
        }
    }
    for (uint32_t k = wave; k < nbig; k += NW) {         // a hub: one wave, a bitmap over j, prefix pop-counts
        const uint32_t w = cb[big[k]];
        const uint32_t gb = w >> 16, cnt = w & 0xFFFFu;
        if (lane < BMW) bm[wave][lane] = 0;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        for (uint32_t m = lane; m < cnt; m += 64) {
            const uint32_t j = mem[gb + m];
            atomicOr(&bm[wave][j >> 5], 1u << (j & 31u));
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        const uint32_t word = lane < BMW ? bm[wave][lane] : 0u;
        const uint32_t own = (uint32_t)__popc(word);
        const uint32_t pre = wave_incl_scan(own) - own;
        for (uint32_t m0 = 0; m0 < cnt; m0 += 64) {      // (uniform trip count: the shuffles are wave-wide)
            const uint32_t m = m0 + lane;
            const bool on = m < cnt;
            const uint32_t j = on ? mem[gb + m] : 0u;
            const uint32_t pw = (uint32_t)__shfl((int)pre, (int)(j >> 5), 64);
            const uint32_t ww = (uint32_t)__shfl((int)word, (int)(j >> 5), 64);
            const uint32_t rank = pw + (uint32_t)__popc(ww & ((1u << (j & 31u)) - 1u));
            if (on) emit(j, gb, rank, cnt);
        }
        __builtin_amdgcn_wave_barrier();
    }
}

// ---- structure bits of the contribution of rank ri in its (node, batch) run (k_wchains / k_dense_place add the chain's bits)
__device__ __forceinline__ uint32_t wref_run_flags(uint32_t ri, bool tail) {
    uint32_t fl = 0;
    if (ri == 0) fl |= WREF_RUN_HEAD;
    if (tail) fl |= WREF_RUN_TAIL;
    if (ri % WIN_BLOCK == 0) fl |= WREF_BLK_HEAD;
    if (ri % WIN_BLOCK == WIN_BLOCK - 1 || tail) fl |= WREF_BLK_TAIL;
    return fl;
}

// ---- run structure after the block sort (thread `tid` holds sorted positions [tid * IPT, tid * IPT + IPT); hd[k]: the position
// is the head of a run; rank: the run heads before this thread's, from a block-wide exclusive scan of the threads' head counts).
// In three pieces: the sorting kernels stamp their phases between them.
// heads -> ustart[run] = its first position, myrun[k] = the run every item of this thread belongs to
template <int IPT>
__device__ __forceinline__ void run_starts(const bool (&hd)[IPT], uint32_t rank, uint32_t* ustart, uint32_t (&myrun)[IPT]) {
#pragma unroll
    for (int k = 0; k < IPT; ++k) {
        if (hd[k]) {
            ustart[rank] = (uint32_t)(threadIdx.x * IPT + k);
            ++rank;
        }
        myrun[k] = rank - 1u;                            // (item 0 is a head: never underflows for j < nc)
    }
}
// (behind a barrier) every contribution's rank inside its run and the structure bits that follow from it
template <int IPT>
__device__ __forceinline__ void run_ranks_store(const uint32_t (&myrun)[IPT], const uint32_t* ustart, uint32_t total, int nc,
                                                uint32_t* __restrict__ bri, uint32_t* __restrict__ bflags) {
#pragma unroll
    for (int k = 0; k < IPT; ++k) {
        const int j = (int)threadIdx.x * IPT + k;
        if (j < nc) {
            const uint32_t st = ustart[myrun[k]];
            const uint32_t en = (myrun[k] + 1 < total) ? ustart[myrun[k] + 1] : (uint32_t)nc;
            const uint32_t ri = (uint32_t)j - st;
            bri[j] = ri;
            bflags[j] = wref_run_flags(ri, (uint32_t)j + 1u == en);
        }
    }
}
// the runs' lengths into the batch's row of the dense planner's run-length matrix (zeroed by the workgroup beforehand)
template <int BS>
__device__ __forceinline__ void run_lengths_store(const uint32_t* key, const uint32_t* ustart, uint32_t total, int nc,
                                                  uint16_t* __restrict__ lenrow) {
    for (uint32_t r = threadIdx.x; r < total; r += BS) {
        const uint32_t st = ustart[r];
        const uint32_t en = (r + 1 < total) ? ustart[r + 1] : (uint32_t)nc;
        lenrow[key[st]] = (uint16_t)(en - st);
    }
}

// ---- wave-aggregated append to an item list: one LDS atomic per wave and list (a typical batch has ~1500 leaders: as many
// same-address atomics otherwise).  Wave-wide: every lane of the wave calls it.
__device__ __forceinline__ void append_item(bool pred, const Item& it, uint32_t* n, Item* __restrict__ list) {
    const int lane = threadIdx.x & 63;
    const unsigned long long m = __ballot(pred);
    if (m) {
        const int first = __ffsll((long long)m) - 1;
        uint32_t base = 0;
        if (lane == first) base = atomicAdd(n, (uint32_t)__popcll(m));
        base = __shfl(base, first);
        if (pred) list[base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = it;
    }
}
__device__ __forceinline__ void append_items(bool lt, bool hv, const Item& it, uint32_t* n_light, uint32_t* n_heavy,
                                             Item* __restrict__ light, Item* __restrict__ heavy) {
    append_item(lt, it, n_light, light);
    append_item(hv, it, n_heavy, heavy);
}

// ---- the batch's descriptor (one thread)
// clock left by the previous batch (TPNet.py:99)
__device__ __forceinline__ double batch_clock(int64_t bb, int64_t e0, const double* __restrict__ t_c, const double* __restrict__ t_prev,
                                              double now_time) {
    return (bb == 0) ? (t_prev ? *t_prev : now_time) : t_c[e0 - 1];
}
// the dense decay's factors only where a dense decay will read them (k_decay_desc, eager mode, which never takes the windowed
// schedule): exp + pow in f64 are ~2 us of this one thread's time behind the kernel's last barrier
__device__ __forceinline__ void batch_desc_store(BatchDesc* __restrict__ desc, int64_t bb, const BatchSpan& sp, double now,
                                                 double t_last, uint32_t n_light, uint32_t n_heavy, bool eager, double lambda, int L) {
    BatchDesc D;
    D.e0 = sp.e0;
    D.ne = sp.B;
    D.pad = 0;
    D.t_last = t_last;
    D.now = now;
    D.n_light = n_light;
    D.n_heavy = n_heavy;
    const double g = eager ? exp(-lambda * (t_last - now)) : 1.0;      // TPNet.py:84-85, f64 then rounded to f32 once
    for (int i = 0; i < TPNET_MAX_LAYERS; ++i)
        D.decay[i] = (eager && i < L) ? (float)pow(g, (double)(i + 1)) : 1.0f;
    desc[bb] = D;
}

// ---- host side: the <threads, contributions per thread> of a workgroup that holds a batch's n2 = 2 B contributions
#define TPNET_FOR_BATCH_TILE(n2, LAUNCH)            \
    do {                                            \
        if ((n2) <= 512) LAUNCH(256, 2);            \
        else if ((n2) <= 1024) LAUNCH(512, 2);      \
        else if ((n2) <= 2048) LAUNCH(1024, 2);     \
        else LAUNCH(1024, 4);                       \
    } while (0)

}  // namespace tpnet
