// Shared by the planners of a windowed chunk that sort every batch in LDS (wplan3.hip: the hashed planner, wplan_dense.hip:
// the dense planner): scratch views of the workspace, the runs' / chains' hash tables of the hashed planner, and the per-batch
// sort itself (one workgroup per batch).
#pragma once
#include "tpnet_common.h"
#include "device_common.hpp"
#include "batch_wg.hpp"

#include <rocprim/block/block_radix_sort.hpp>

namespace tpnet {

// ---- WPlan::rec (tpnet_common.h: WRec): THE writer and THE reader of a contribution's record ----------------------------------
// A planner forms the whole record in registers and stores it once at its sorted position: two 16-byte stores to the same 32
// aligned bytes (every byte written, the spare word as 0; nothing is read back or patched afterwards).
__device__ __forceinline__ void wrec_store(WRec* __restrict__ rec, size_t f, int32_t partner, float coef, uint32_t ref, float g,
                                           float dec, int32_t target, uint32_t bc) {
    uint4* r = reinterpret_cast<uint4*>(rec + f);
    r[0] = make_uint4((uint32_t)partner, __float_as_uint(coef), ref, __float_as_uint(g));
    r[1] = make_uint4(__float_as_uint(dec), (uint32_t)target, bc, 0u);
}
struct WRecWalk {         // first half: {partner, coef, ref, g}
    int32_t partner;
    float coef;
    uint32_t ref;
    float g;
};
struct WRecEnds {         // second half: {dec, target, bc}
    float dec;
    int32_t target;
    uint32_t bc;
};
__device__ __forceinline__ WRecWalk wrec_load_walk(const WRec* __restrict__ rec, size_t f) {
    const uint4 v = reinterpret_cast<const uint4*>(rec + f)[0];
    return {(int32_t)v.x, __uint_as_float(v.y), v.z, __uint_as_float(v.w)};
}
__device__ __forceinline__ WRecEnds wrec_load_ends(const WRec* __restrict__ rec, size_t f) {
    const uint4 v = reinterpret_cast<const uint4*>(rec + f)[1];
    return {__uint_as_float(v.x), (int32_t)v.y, v.z};
}

static constexpr uint32_t WT_CHAIN_HEAD = 1u;       // bflags: first contribution of its node in the window
static constexpr uint32_t WT_WIN_LAST = 2u;         // bflags: tail of its node's last run in the window
static constexpr uint32_t WT_STRUCT_MASK = WREF_RUN_HEAD | WREF_RUN_TAIL | WREF_BLK_HEAD | WREF_BLK_TAIL;
static constexpr int WCLS = 8;                      // length classes of a window's chain list (class 0: workgroup-walked)

// H1, runs: one open-addressing SEGMENT per batch (linear probing inside the segment, at most a third full), built by the
// batch's workgroup in LDS and written out whole with plain stores -- no global atomics, nothing to zero.  (One chunk-wide
// table claimed with atomicCAS cost k_wsort 25 of its 37 us: ~240 000 scattered returning atomics per epoch of C2.)
// H2, chains: indexed [window][node] where that fits the table's bytes (one non-returning atomic OR per run marks the batch);
// else open addressing over the whole table (key 0 = empty; zeroed before every plan).
struct HEnt {
    unsigned long long key;
    uint32_t a, b;
};
static_assert(sizeof(HEnt) == 16, "HEnt must be 16 bytes");
struct CEnt {                  // chain table: one entry per (node, window)
    unsigned long long key;
    unsigned long long mask;   // bit k: the node is a target in batch (first batch of the window) + k      (A: atomic or)
    uint32_t xh;               // batch-sorted position of the chain's head                                 (B: the chain head)
    uint32_t cnt;              // contributions of the chain                                                (B)
    uint32_t pad0, pad1;
};
static_assert(sizeof(CEnt) == 32, "CEnt must be 32 bytes");

#ifdef TPNET_STAMPS
#define WSTAMP(slot)                                                                          \
    do {                                                                                      \
        if (q.dbg && blockIdx.x == gridDim.x / 2 && threadIdx.x == 0) {                       \
            q.dbg[(slot) * 2 + 0] = __builtin_amdgcn_s_memtime();                             \
            q.dbg[(slot) * 2 + 1] = __builtin_amdgcn_s_memrealtime();                         \
        }                                                                                     \
    } while (0)
#else
#define WSTAMP(slot) do { } while (0)
#endif

struct WTmp {              // scratch of the stages, aliased onto arrays of the base plan that this planner does not use
    uint32_t* bkey;        // [nc] target node of the contribution at this batch-sorted position (batch b owns [2 e0(b), ...))
    int32_t* bpart;        // [nc] its partner
    float* bcoef;          // [nc] its time weight
    uint32_t* bval;        // [nc] its pre-sort index inside the batch (side * ne + edge)
    uint32_t* binv;        // [nc] chunk-relative pre-sort index -> chunk-relative batch-sorted position
    uint32_t* bsb;         // [nc] at a run's HEAD: contributions of the node in EARLIER batches of the window
    uint32_t* bri;         // [nc] rank inside its (node, batch) run (k_wsort)
    uint32_t* rprevb;      // [nc] at a run's HEAD: batch of the node's previous run inside the window (bsb > 0); chain heads: their place in the window's list of their length class
    uint32_t* bflags;      // [nc] WREF_* structure bits (k_wsort) | WT_* (k_wchains)
    HEnt* h1;              // (node, batch) -> a = chunk-relative batch-sorted position of the run's head, b = its length
    CEnt* h2;              // (node, window) -> the batches the node is a target in, its chain
    uint32_t hcap;         // entries of H2
    uint32_t seg;          // entries of a batch's segment of H1
    uint32_t direct2;      // H2 is indexed [window][node] (n2 nodes per window)
    uint32_t n2;
    uint32_t* blkcnt;      // [nblk][9] per workgroup of k_wchains: chain heads per length class, positions their chains need
    uint32_t* blkbase;     // [nblk][9] k_wscan: the same, summed over the earlier workgroups of the window
    uint32_t* boff;        // [nc] chain heads: what the chain heads before it in its workgroup claimed (positions)
    uint32_t* wtot;        // [WIN_MAX_WINDOWS][9] k_wscan: the window's totals of the same counters
    uint32_t bpb;          // workgroups of k_wchains per batch
    unsigned long long* dbg;   // diagnostic builds (-DTPNET_STAMPS): phase stamps of workgroup `stamp block`
};

static inline uint32_t wplan3_table_entries(size_t nc) { return (uint32_t)(2 * nc + 1021); }   // H2: at most half full
// contributions a workgroup of k_wsort sorts (its BS * IPT), and the segment of H1 it builds: the LDS of its three per-edge arrays
static inline uint32_t wplan3_nc_block(int64_t batch) {
    const int64_t n2 = 2 * batch;
    return n2 <= 512 ? 512u : n2 <= 1024 ? 1024u : n2 <= 2048 ? 2048u : 4096u;
}
static inline uint32_t wplan3_seg(int64_t batch) { return wplan3_nc_block(batch) * 3; }   // (16-bit slots in 3 * NC / 2 words)
static inline size_t wplan3_h2_bytes(int64_t Ec) { return (size_t)wplan3_table_entries(2 * (size_t)Ec) * sizeof(CEnt); }
static inline uint32_t wplan3_bpb(int64_t batch) { return (uint32_t)((2 * batch + 255) / 256); }

static WTmp wtmp_of(const WPlan& p, size_t nc) {
    WTmp q;
    q.dbg = p.base.dbg;
    uint32_t* ki = reinterpret_cast<uint32_t*>(p.base.keys_in);     // 8 nc bytes
    uint32_t* ko = reinterpret_cast<uint32_t*>(p.base.keys_out);    // 8 nc bytes
    q.bkey = ki;
    q.bpart = reinterpret_cast<int32_t*>(ki + nc);
    q.bcoef = reinterpret_cast<float*>(ko);
    q.bval = p.base.vals_out;
    q.binv = p.inv;
    // (base.heavy holds the contributions' records, WPlan::rec; vals_in is the sorted planner's)
    q.bsb = p.wscr;
    q.bri = p.wscr + nc;
    q.rprevb = p.wscr + 2 * nc;
    q.bflags = p.base.vals_in;
    const uint32_t cap = wplan3_table_entries(nc);
    q.h2 = reinterpret_cast<CEnt*>(p.wtab);                          // (first: the fill of a plan ends behind what H2 uses)
    q.h1 = reinterpret_cast<HEnt*>(reinterpret_cast<char*>(p.wtab) + (wplan3_h2_bytes((int64_t)(nc / 2)) + 255) / 256 * 256);
    q.hcap = cap;
    q.seg = 0;
    q.direct2 = 0;
    q.n2 = 0;
    q.boff = p.rhead;
    q.wtot = p.wcls;
    return q;
}

__device__ __forceinline__ float decay3_f32(double lambda, double dt) {   // as plan.hip decay_f32 / device_common.hpp meta_view
    const float x = (float)(-lambda * dt);
    return (x == 0.0f) ? 1.0f : expf(x);
}

__device__ __forceinline__ uint32_t hmix(unsigned long long k) {
    k ^= k >> 33;
    k *= 0xff51afd7ed558ccdULL;
    k ^= k >> 33;
    k *= 0xc4ceb9fe1a85ec53ULL;
    k ^= k >> 33;
    return (uint32_t)k;
}
__device__ __forceinline__ unsigned long long hkey(uint32_t node, uint32_t minor) {      // minor: batch (H1) / window (H2), < 2^16
    return ((unsigned long long)(node + 1u) << 16) | (unsigned long long)minor;
}
// the run of (node, batch): a = chunk-relative batch-sorted position of its head, b = its length (false: the node is no target there)
__device__ __forceinline__ bool hfind(const HEnt* __restrict__ T, uint32_t seg, unsigned long long key, uint32_t& a, uint32_t& b) {
    const HEnt* __restrict__ S = T + (size_t)(key & 0xFFFFull) * seg;
    uint32_t i = hmix(key) % seg;
    for (;;) {
        const uint4 e = *reinterpret_cast<const uint4*>(S + i);
        const unsigned long long k = ((unsigned long long)e.y << 32) | e.x;
        if (k == key) { a = e.z; b = e.w; return true; }
        if (k == 0ull) { a = 0; b = 0; return false; }
        i = (i + 1 == seg) ? 0u : i + 1;
    }
}

// G probes at once: all first loads are issued before any is looked at (a loop per probe would be G dependent round
// trips); a probe that lands on another key's slot walks on alone (rare: a segment is at most a third full)
template <int G>
__device__ __forceinline__ void hfind_multi(const HEnt* __restrict__ T, uint32_t seg, const unsigned long long* key,
                                            const bool* valid, uint32_t* a, uint32_t* b) {
    uint32_t idx[G];
    uint4 e[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        idx[g] = hmix(key[g]) % seg;
        e[g] = *reinterpret_cast<const uint4*>(T + (valid[g] ? (size_t)(key[g] & 0xFFFFull) * seg + idx[g] : (size_t)0));
    }
#pragma unroll
    for (int g = 0; g < G; ++g) {
        a[g] = 0;
        b[g] = 0;
        if (!valid[g]) continue;
        const HEnt* __restrict__ S = T + (size_t)(key[g] & 0xFFFFull) * seg;
        uint32_t i = idx[g];
        uint4 x = e[g];
        for (;;) {
            const unsigned long long k = ((unsigned long long)x.y << 32) | x.x;
            if (k == key[g]) { a[g] = x.z; b[g] = x.w; break; }
            if (k == 0ull) break;
            i = (i + 1 == seg) ? 0u : i + 1;
            x = *reinterpret_cast<const uint4*>(S + i);
        }
    }
}

// chain table: A marks batch `bit` of window w in the node's entry (hashed: created by whoever comes first)
__device__ __forceinline__ void cmark(const WTmp& q, uint32_t node, uint32_t w, unsigned bit) {
    if (q.direct2) {
        (void)__hip_atomic_fetch_or(&q.h2[(size_t)w * q.n2 + node].mask, 1ull << bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return;
    }
    const unsigned long long key = hkey(node, w);
    uint32_t i = hmix(key ^ 0x5bd1e995ull) % q.hcap;
    for (;;) {
        const unsigned long long old = atomicCAS(&q.h2[i].key, 0ull, key);
        if (old == 0ull || old == key) {
            (void)__hip_atomic_fetch_or(&q.h2[i].mask, 1ull << bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return;
        }
        i = (i + 1 == q.hcap) ? 0u : i + 1;
    }
}
// the entry of (node, window) (nullptr: the node is no target in the window)
__device__ __forceinline__ CEnt* cfind(const WTmp& q, uint32_t node, uint32_t w) {
    if (q.direct2) {
        CEnt* e = q.h2 + ((size_t)w * q.n2 + node);
        return e->mask ? e : nullptr;
    }
    const unsigned long long key = hkey(node, w);
    uint32_t i = hmix(key ^ 0x5bd1e995ull) % q.hcap;
    for (;;) {
        const unsigned long long k = q.h2[i].key;
        if (k == key) return q.h2 + i;
        if (k == 0ull) return nullptr;
        i = (i + 1 == q.hcap) ? 0u : i + 1;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// A: per-batch sort.  One workgroup per batch.
// ---------------------------------------------------------------------------------------------------------------
template <int BS, int IPT>
struct WSortShared {
    using Sort = rocprim::block_radix_sort<uint32_t, BS, IPT, uint32_t>;
    static constexpr int NC = BS * IPT;
    union U {
        typename Sort::storage_type sort;
        struct { uint32_t key[NC]; uint32_t ustart[NC]; } s;     // sorted keys; then the heads of the distinct targets' runs
    } u;
    // per edge: endpoints (0 if out of range) | bit 31: the EDGE has a bad endpoint; time weight.  Dead once the sorted arrays are
    // stored: the batch's segment of H1 is then built in the same 3 * NC / 2 words
    uint32_t e_all[3 * (NC / 2)];
    uint32_t wsum[BS / 64];
};

// DENSE = the dense planner's variant: instead of the batch's segment of H1 and the marks in the chain table, the batch's ROW of
// the run-length matrix (lenrow[n] = contributions to node n in this batch; every entry written: nothing to zero beforehand)
template <int BS, int IPT, bool DENSE>
__device__ __forceinline__ void wsort_batch(WSortShared<BS, IPT>& sh, const WTmp& q, BatchDesc* __restrict__ desc,
                                            const int64_t* __restrict__ src_c, const int64_t* __restrict__ dst_c,
                                            const double* __restrict__ t_c, int64_t Ec, int32_t Bfull, int64_t N, int node_bits,
                                            double now_time, const double* __restrict__ t_prev, double lambda, int L, uint32_t* err,
                                            int KW, int64_t bb, uint16_t* __restrict__ lenrow) {
    const BatchSpan sp = batch_span(bb, src_c, dst_c, t_c, Ec, Bfull);
    const int64_t e0 = sp.e0;
    const int32_t B = sp.B;
    const int64_t g0 = 2 * e0;
    using Sort = typename WSortShared<BS, IPT>::Sort;
    constexpr int NC = BS * IPT;
    auto& u = sh.u;
    uint32_t* const e_all = sh.e_all;
    uint32_t* const wsum = sh.wsum;
    uint32_t* const e_src = e_all;
    uint32_t* const e_dst = e_all + NC / 2;
    float* const e_w = reinterpret_cast<float*>(e_all + NC);
    constexpr uint32_t SEG = 3 * NC;                  // slots of 16 bits: at most a third full (a probe that walks is a dependent
                                                      // round trip for every reader of the table: short clusters matter more than bytes)
    static_assert(sizeof(WSortShared<BS, IPT>) <= 64 * 1024, "k_wsort: LDS budget");
    static_assert(NC <= 65535 / 2 * 2, "k_wsort: run indices");
    const int tid = threadIdx.x;
    const int nc = 2 * B;
    WSTAMP(0);
    if constexpr (DENSE) {
        // (16-bit stores, coalesced; the barriers between here and the scatter of the runs' lengths order the two)
        for (int64_t n = tid; n < N; n += BS) lenrow[n] = 0;
    }
    const auto burst = edges_load<BS, IPT / 2>(sp);
    const double t_last = burst.t_last;
    edges_stage<BS>(burst, B, N, lambda, err, e_src, e_dst, e_w);
    __syncthreads();
    WSTAMP(1);
    uint32_t keys[IPT], vals[IPT];
    sort_keys(keys, vals, nc, B, node_bits, e_src, e_dst);
    Sort().sort(keys, vals, u.sort, 0u, (unsigned)(node_bits + 1));
    __syncthreads();
    WSTAMP(2);
#pragma unroll
    for (int k = 0; k < IPT; ++k) u.s.key[tid * IPT + k] = keys[k];
    __syncthreads();
    // the sorted contributions; the heads of the runs are ranked by a block-wide exclusive scan (thread `tid` holds
    // positions [tid * IPT, tid * IPT + IPT))
    uint32_t hcount = 0;
    bool hd[IPT];
#pragma unroll
    for (int k = 0; k < IPT; ++k) {
        const int j = tid * IPT + k;
        hd[k] = j < nc && (j == 0 || u.s.key[j - 1] != keys[k]);
        hcount += hd[k] ? 1u : 0u;
        if (j < nc) {
            const uint32_t val = vals[k];
            int32_t partner;
            float w;
            contrib_partner_weight((int)val, B, e_src, e_dst, e_w, partner, w);
            q.bkey[g0 + j] = keys[k];
            q.bpart[g0 + j] = partner;
            q.bcoef[g0 + j] = w;
            q.bval[g0 + j] = val;
            q.binv[g0 + val] = (uint32_t)(g0 + j);
        }
    }
    uint32_t total;
    const uint32_t rank = block_excl_scan<BS, false>(hcount, wsum, total);
    WSTAMP(3);
    if constexpr (!DENSE)
        for (uint32_t i = tid; i < SEG / 2; i += BS) e_all[i] = 0u;  // (every thread has read its edges' entries: the scan's barrier)
    uint32_t myrun[IPT];
    run_starts(hd, rank, u.s.ustart, myrun);
    __syncthreads();
    WSTAMP(4);
    run_ranks_store(myrun, u.s.ustart, total, nc, q.bri + g0, q.bflags + g0);
    if constexpr (DENSE) {
        // ---- the runs: this batch's row of the run-length matrix (zeroed by this workgroup before its first barrier)
        run_lengths_store<BS>(u.s.key, u.s.ustart, total, nc, lenrow);
    } else {
    // ---- the runs: the batch's segment of H1 in LDS (slot = run + 1; the runs' nodes are distinct: a claim needs no key
    // compare), the node's entry of the chain table marked with this batch
    for (uint32_t r = tid; r < total; r += BS) {
        const uint32_t st = u.s.ustart[r];
        const uint32_t node = u.s.key[st];
        uint32_t i = hmix(hkey(node, (uint32_t)bb)) % SEG;
        for (;;) {                                       // claim the first empty 16-bit slot from i on (two slots per LDS word)
            const uint32_t sh = (i & 1u) * 16u;
            uint32_t old = e_all[i >> 1];
            bool done = false;
            while (((old >> sh) & 0xFFFFu) == 0u) {
                const uint32_t seen = atomicCAS(&e_all[i >> 1], old, old | ((r + 1u) << sh));
                if (seen == old) { done = true; break; }
                old = seen;                              // (the word's other slot was claimed meanwhile, or this one)
            }
            if (done) break;
            i = (i + 1 == SEG) ? 0u : i + 1;
        }
        cmark(q, node, (uint32_t)(bb / KW), (unsigned)(bb % KW));
    }
    __syncthreads();
    {
        HEnt* __restrict__ S = q.h1 + (size_t)bb * SEG;
        for (uint32_t i = tid; i < SEG; i += BS) {
            const uint32_t v = (e_all[i >> 1] >> ((i & 1u) * 16u)) & 0xFFFFu;
            uint4 e = make_uint4(0u, 0u, 0u, 0u);
            if (v) {
                const uint32_t r = v - 1u;
                const uint32_t st = u.s.ustart[r];
                const uint32_t en = (r + 1 < total) ? u.s.ustart[r + 1] : (uint32_t)nc;
                const unsigned long long k1 = hkey(u.s.key[st], (uint32_t)bb);
                e = make_uint4((uint32_t)k1, (uint32_t)(k1 >> 32), (uint32_t)(g0 + st), en - st);
            }
            *reinterpret_cast<uint4*>(S + i) = e;
        }
    }
    }
    WSTAMP(5);
    // (eager = false: the dense decay's factors are read by the eager mode only, which never takes the windowed schedule)
    if (tid == 0) batch_desc_store(desc, bb, sp, batch_clock(bb, e0, t_c, t_prev, now_time), t_last, 0u, 0u, false, lambda, L);
    WSTAMP(6);
}

}  // namespace tpnet
