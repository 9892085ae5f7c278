// Device-side negative edge sampler: the 'historical' and 'inductive' strategies of the reference's NegativeEdgeSampler
// (utils/utils.py:315-505), and its 'random' one.  The reference rebuilds Python sets of (src, dst) tuples over every edge seen so far
// for each batch, and keeps |unique src| x |unique dst| tuples from construction on.  Here: one table of the U unique edges in
// ascending (src << 32 | dst) order, each with its ascending list of occurrence times (built once, two device-wide sorts); per call a
// candidate flag per unique edge (one lower-bound search), a scan + compaction, and one pick kernel that draws by a keyed permutation,
// so the |Us| x |Ud| domain of the fill is never materialised.  The draw rule is spelled out in include/tpnet_hip.h.
#include "tpnet_common.h"
#include "draw_common.hpp"
#include "scan_common.hpp"
#include "arena.hpp"
#include "sort_tmp.hpp"

namespace tpnet {

static constexpr int NEG_HASH_SLOTS = 2048;          // LDS table of the batch's pairs: batches of up to NEG_HASH_MAX_B
static constexpr int64_t NEG_HASH_MAX_B = 1024;      // (load <= 1/2); larger batches are sorted and searched
static constexpr int NEG_ROUNDS = 6;                 // Feistel rounds of the permutation (even: the halves alternate)
static constexpr uint64_t NEG_EMPTY = ~0ull;         // no pair of ids < 2^31 has this key

// header words of the sampler buffer
enum { NEG_U = 0, NEG_NUS = 1, NEG_NUD = 2, NEG_ERR = 3, NEG_BAD = 4 };

// ---- build ---------------------------------------------------------------------------------------------------------------------
__global__ void k_neg_keys(const int64_t* __restrict__ src, const int64_t* __restrict__ dst, const double* __restrict__ t, int64_t E,
                           uint64_t* __restrict__ tkey, uint32_t* __restrict__ idx, uint32_t* __restrict__ hdr) {
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < E; j += (int64_t)gridDim.x * blockDim.x) {
        if ((uint64_t)src[j] >= (1ull << 31) || (uint64_t)dst[j] >= (1ull << 31)) atomicAdd(&hdr[NEG_BAD], 1u);
        tkey[j] = time_key(t ? t[j] : 0.0);
        idx[j] = (uint32_t)j;
    }
}

__global__ void k_neg_edgekeys(const int64_t* __restrict__ src, const int64_t* __restrict__ dst, int64_t E,
                               const uint32_t* __restrict__ idx, uint64_t* __restrict__ ekey) {
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < E; j += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t o = idx[j];
        ekey[j] = ((uint64_t)((uint32_t)src[o] & 0x7FFFFFFFu) << 32) | (uint64_t)((uint32_t)dst[o] & 0x7FFFFFFFu);
    }
}

// sorted order -> the occurrence times (ascending inside an edge) and the dst ids as keys of their own sort
__global__ void k_neg_times(const double* __restrict__ t, int64_t E, const uint32_t* __restrict__ idx,
                            const uint64_t* __restrict__ ekey, double* __restrict__ times, uint32_t* __restrict__ dkey) {
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < E; j += (int64_t)gridDim.x * blockDim.x) {
        times[j] = t ? t[idx[j]] : 0.0;
        dkey[j] = (uint32_t)ekey[j];
    }
}

struct HeadEdge {
    const uint64_t* k;
    __device__ uint32_t operator()(uint32_t j) const { return (j == 0 || k[j] != k[j - 1]) ? 1u : 0u; }
};
struct HeadSrc {
    const uint64_t* k;
    __device__ uint32_t operator()(uint32_t j) const { return (j == 0 || (k[j] >> 32) != (k[j - 1] >> 32)) ? 1u : 0u; }
};
struct HeadDst {
    const uint32_t* k;
    __device__ uint32_t operator()(uint32_t j) const { return (j == 0 || k[j] != k[j - 1]) ? 1u : 0u; }
};
struct EmitEdge {
    const uint64_t* ek; const double* times; uint64_t* ukey; uint32_t* ustart; double* ufirst; uint8_t* uobs;
    double last_observed; int has_observed;
    __device__ void operator()(uint32_t j, uint32_t pos) const {
        ukey[pos] = ek[j];
        ustart[pos] = j;
        ufirst[pos] = times[j];
        uobs[pos] = (has_observed && times[j] <= last_observed) ? 1 : 0;
    }
};
struct EmitSrc {
    const uint64_t* ek; int64_t* us;
    __device__ void operator()(uint32_t j, uint32_t pos) const { us[pos] = (int64_t)(ek[j] >> 32); }
};
struct EmitDst {
    const uint32_t* dk; int64_t* ud;
    __device__ void operator()(uint32_t j, uint32_t pos) const { ud[pos] = (int64_t)dk[j]; }
};

// ---- sample --------------------------------------------------------------------------------------------------------------------
// candidate iff first_time <= t0, no occurrence in [t0, t1] (the first occurrence >= t0, if any, lies behind t1), and for
// 'inductive' first_time > last_observed_time; the flag is kept for the compaction pass
struct CandFlag {
    const double* ufirst; const uint32_t* ustart; const uint8_t* uobs; const double* times; const uint32_t* hdr; uint32_t E;
    double t0, t1; int inductive; uint8_t* flag;
    __device__ uint32_t operator()(uint32_t u) const {
        uint32_t c = 0;
        if (ufirst[u] <= t0 && !(inductive && uobs[u])) {
            const uint32_t end = (u + 1 < hdr[NEG_U]) ? ustart[u + 1] : E;
            uint32_t lo = ustart[u], hi = end;
            while (lo < hi) {
                const uint32_t mid = (lo + hi) >> 1;
                if (times[mid] < t0) lo = mid + 1; else hi = mid;
            }
            c = (lo < end && times[lo] <= t1) ? 0u : 1u;
        }
        flag[u] = (uint8_t)c;
        return c;
    }
};
struct ByteFlag {
    const uint8_t* flag;
    __device__ uint32_t operator()(uint32_t u) const { return flag[u]; }
};
struct EmitCand {
    uint32_t* cand;
    __device__ void operator()(uint32_t u, uint32_t pos) const { cand[pos] = u; }
};

struct NegKey {
    uint32_t k0, k1, call;
    __device__ __forceinline__ uint32_t word(uint32_t tag, uint32_t a, uint32_t b) const { return philox_word(a, b, tag, call, k0, k1, 0); }
};

// slot i of the keyed permutation of [0, n): an alternating Feistel network over the bitlength(n - 1) bits of a slot (the high a
// bits and the low b bits take turns being xored with a keyed word of the other half), walked until it lands below n: the
// network's domain is smaller than 2 n, so a slot takes fewer than two passes on average
__device__ __forceinline__ uint64_t neg_perm(uint64_t n, uint32_t tag, uint64_t i, const NegKey& k) {
    if (n <= 1) return 0;
    const int bits = 64 - __builtin_clzll(n - 1);             // 1 <= bits <= 62 (n < 2^62)
    const int a = bits >> 1, b = bits - a;                    // a <= b <= 31
    const uint32_t mask_l = (1u << a) - 1u, mask_r = (1u << b) - 1u;
    uint64_t x = i;
    do {
        uint32_t L = (uint32_t)(x >> b), R = (uint32_t)x & mask_r;
        for (int r = 0; r < NEG_ROUNDS; r += 2) {
            L ^= k.word(tag, R, (uint32_t)r) & mask_l;
            R ^= k.word(tag, L, (uint32_t)r + 1u) & mask_r;
        }
        x = ((uint64_t)L << b) | R;
    } while (x >= n);
    return x;
}

__device__ __forceinline__ uint64_t batch_key(int64_t s, int64_t d) {
    if ((uint64_t)s >= (1ull << 31) || (uint64_t)d >= (1ull << 31)) return NEG_EMPTY;     // no edge of the table has such an id
    return ((uint64_t)s << 32) | (uint64_t)d;
}
__device__ __forceinline__ uint32_t hash_slot(uint64_t key) { return (uint32_t)((key * 0x9E3779B97F4A7C15ull) >> 53); }   // 11 bits

__global__ void k_neg_bkeys(const int64_t* __restrict__ bs, const int64_t* __restrict__ bd, int64_t B, uint64_t* __restrict__ keys) {
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < B; j += (int64_t)gridDim.x * blockDim.x)
        keys[j] = batch_key(bs[j], bd[j]);
}

__global__ __launch_bounds__(256) void k_neg_random(const int64_t* __restrict__ us, const int64_t* __restrict__ ud,
                                                    const uint32_t* __restrict__ hdr, int64_t size, NegKey k,
                                                    int64_t* __restrict__ out_src, int64_t* __restrict__ out_dst) {
    const uint64_t ns = hdr[NEG_NUS], nd = hdr[NEG_NUD];
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < size; i += (int64_t)gridDim.x * blockDim.x) {
        out_src[i] = us[((uint64_t)k.word(3, (uint32_t)i, 0) * ns) >> 32];
        out_dst[i] = ud[((uint64_t)k.word(4, (uint32_t)i, 0) * nd) >> 32];
    }
}

// The outputs of one call.  M = the candidate count the scan left on the device.  size <= M: slot i takes candidate perm_M(i).
// Otherwise the M candidates go to the back, every workgroup a share, and workgroup 0 fills the F = size - M slots in front: trial
// slots in chunks of 256, a workgroup scan over the valid ones (not a pair of the batch), until F are placed or the trials end.
// bsorted: the batch's keys sorted (B > NEG_HASH_MAX_B), else they go through an LDS hash table.
__global__ __launch_bounds__(256) void k_neg_pick(uint32_t* __restrict__ hdr, const int64_t* __restrict__ us,
                                                  const int64_t* __restrict__ ud, const uint64_t* __restrict__ ukey,
                                                  const uint32_t* __restrict__ cand, const uint32_t* __restrict__ words,
                                                  int64_t size, const int64_t* __restrict__ bs, const int64_t* __restrict__ bd,
                                                  int64_t B, const uint64_t* __restrict__ bsorted, uint64_t* valid, NegKey k,
                                                  int64_t* __restrict__ out_src, int64_t* __restrict__ out_dst) {
    __shared__ unsigned long long tab[NEG_HASH_SLOTS];
    __shared__ uint32_t sh[4];
    const uint64_t M = words[0];
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    if ((uint64_t)size <= M) {
        for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < size; i += stride) {
            const uint64_t key = ukey[cand[neg_perm(M, 0, (uint64_t)i, k)]];
            out_src[i] = (int64_t)(key >> 32);
            out_dst[i] = (int64_t)(key & 0xFFFFFFFFull);
        }
        return;
    }
    const uint64_t F = (uint64_t)size - M;
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < (int64_t)M; j += stride) {
        const uint64_t key = ukey[cand[j]];
        out_src[F + j] = (int64_t)(key >> 32);
        out_dst[F + j] = (int64_t)(key & 0xFFFFFFFFull);
    }
    if (blockIdx.x != 0) return;
    const int tid = threadIdx.x;
    if (!bsorted) {
        for (int s = tid; s < NEG_HASH_SLOTS; s += 256) tab[s] = NEG_EMPTY;
        __syncthreads();
        for (int64_t b = tid; b < B; b += 256) {
            const uint64_t key = batch_key(bs[b], bd[b]);
            if (key == NEG_EMPTY) continue;
            uint32_t s = hash_slot(key);
            for (;;) {
                const unsigned long long old = atomicCAS(&tab[s], (unsigned long long)NEG_EMPTY, (unsigned long long)key);
                if (old == NEG_EMPTY || old == key) break;
                s = (s + 1) & (NEG_HASH_SLOTS - 1);
            }
        }
        __syncthreads();
    }
    const uint64_t nd = hdr[NEG_NUD];
    const uint64_t D = (uint64_t)hdr[NEG_NUS] * nd;
    const uint64_t T = D < F + (uint64_t)B ? D : F + (uint64_t)B;
    uint64_t count = 0;                                                        // valid trials so far (the same in every thread)
    for (uint64_t base = 0; base < T && count < F; base += 256) {
        const uint64_t j = base + tid;
        uint32_t v = 0;
        uint64_t key = 0;
        if (j < T) {
            const uint64_t x = neg_perm(D, 1, j, k);
            key = ((uint64_t)us[x / nd] << 32) | (uint64_t)ud[x % nd];
            bool hit = false;
            if (bsorted) {
                int64_t lo = 0, hi = B;
                while (lo < hi) {
                    const int64_t mid = (lo + hi) >> 1;
                    if (bsorted[mid] < key) lo = mid + 1; else hi = mid;
                }
                hit = lo < B && bsorted[lo] == key;
            } else {
                uint32_t s = hash_slot(key);
                for (;;) {
                    const uint64_t q = tab[s];
                    if (q == NEG_EMPTY) break;
                    if (q == key) { hit = true; break; }
                    s = (s + 1) & (NEG_HASH_SLOTS - 1);
                }
            }
            v = hit ? 0u : 1u;
        }
        uint32_t tot;
        const uint32_t incl = wg_scan256(v, sh, tot);
        const uint64_t pos = count + incl - v;
        if (v && pos < F) {
            out_src[pos] = (int64_t)(key >> 32);
            out_dst[pos] = (int64_t)(key & 0xFFFFFFFFull);
            valid[pos] = key;
        }
        count += tot;
    }
    if (count >= F) return;
    // the whole domain was enumerated and only P = count < F pairs are valid: F draws with replacement from them
    __syncthreads();
    const uint64_t P = count;
    for (uint64_t i = tid; i < F; i += 256) {
        int64_t s = -1, d = -1;
        if (P) {
            const uint64_t key = valid[((uint64_t)k.word(2, (uint32_t)i, 0) * P) >> 32];
            s = (int64_t)(key >> 32);
            d = (int64_t)(key & 0xFFFFFFFFull);
        }
        out_src[i] = s;
        out_dst[i] = d;
    }
    if (!P && tid == 0) hdr[NEG_ERR] = 1u;
}

// ---- per-query candidates (tpnet_neg_sample_many; the rule: include/tpnet_hip.h) ---------------------------------------------------
static constexpr int NEGM_BLOCK = 256;                // four waves, one query each

// first index in [lo, hi) of the ascending keys whose key is >= `key`
__device__ __forceinline__ uint32_t key_lower_bound(const uint64_t* __restrict__ k, uint32_t lo, uint32_t hi, uint64_t key) {
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (k[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// does unique edge e occur at time exactly t?  (its occurrence times are ascending in times[ustart[e] .. ustart[e + 1]))
__device__ __forceinline__ bool occurs_at(const uint32_t* __restrict__ ustart, const double* __restrict__ times, uint32_t U,
                                          uint32_t E, uint32_t e, double t) {
    const uint32_t end = (e + 1 < U) ? ustart[e + 1] : E;
    uint32_t lo = ustart[e], hi = end;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (times[mid] < t) lo = mid + 1; else hi = mid;
    }
    return lo < end && times[lo] == t;
}

// One wave per query i = (s, d, t).  Historical part: the source's run [e0, e0 + R) of the table, visited in the order of perm_i(R, 5, .),
// 64 slots per step; the eligible ones are compacted by a ballot into cand[i, 0 .. h).  Random part: Ud in the order of perm_i(|Ud|, 6, .),
// 64 slots per step; a slot's destination is looked up in the source's run (excluded when that edge occurs at t) and among the row's h
// historical picks -- read back from the row itself, every lane the same word at a time (a broadcast), behind a workgroup fence.
__global__ __launch_bounds__(NEGM_BLOCK) void k_neg_many(const uint32_t* __restrict__ hdr, const uint64_t* __restrict__ ukey,
                                                         const uint32_t* __restrict__ ustart, const double* __restrict__ ufirst,
                                                         const double* __restrict__ times, const int64_t* __restrict__ ud, uint32_t E,
                                                         const int64_t* __restrict__ bs, const int64_t* __restrict__ bd,
                                                         const double* __restrict__ bt, int64_t B, int Q, int Qh, NegKey key,
                                                         int64_t* cand, int32_t* __restrict__ n_hist) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * (NEGM_BLOCK / 64) + (threadIdx.x >> 6);
    if (i >= B) return;                                          // (a whole wave leaves: no workgroup barrier below)
    const uint32_t U = hdr[NEG_U];
    const uint64_t nud = hdr[NEG_NUD];
    const int64_t s = bs[i], d = bd[i];
    const double t = bt[i];
    int64_t* row = cand + i * (int64_t)Q;
    const NegKey k{key.k0, key.k1 ^ (uint32_t)i, key.call};
    const unsigned long long below = (1ull << lane) - 1ull;
    uint32_t e0 = 0, R = 0;
    if ((uint64_t)s < (1ull << 31)) {                            // (no edge of the table has another source)
        e0 = key_lower_bound(ukey, 0, U, (uint64_t)s << 32);
        R = key_lower_bound(ukey, e0, U, ((uint64_t)s + 1) << 32) - e0;
    }
    int h = 0;
    for (uint32_t base = 0; base < R && h < Qh; base += 64) {
        const uint32_t j = base + (uint32_t)lane;
        bool ok = false;
        int64_t dd = 0;
        if (j < R) {
            const uint32_t e = e0 + (uint32_t)neg_perm(R, 5, j, k);
            dd = (int64_t)(ukey[e] & 0xFFFFFFFFull);
            ok = dd != d && ufirst[e] < t && !occurs_at(ustart, times, U, E, e, t);
        }
        const unsigned long long m = __ballot(ok);
        const int pos = h + __popcll(m & below);
        if (ok && pos < Qh) row[pos] = dd;
        h += __popcll(m);
    }
    h = h < Qh ? h : Qh;
    if (lane == 0) n_hist[i] = h;
    __threadfence_block();                                       // the picks are read back below by the other lanes of this wave
    int fill = h;
    for (uint64_t base = 0; base < nud && fill < Q; base += 64) {
        const uint64_t j = base + (uint64_t)lane;
        bool ok = false;
        int64_t dd = 0;
        if (j < nud) {
            dd = ud[neg_perm(nud, 6, j, k)];
            ok = dd != d;
            if (ok && R) {
                const uint64_t ek = ((uint64_t)s << 32) | (uint64_t)dd;
                const uint32_t e = key_lower_bound(ukey, e0, e0 + R, ek);
                if (e < e0 + R && ukey[e] == ek) ok = !occurs_at(ustart, times, U, E, e, t);
            }
        }
        for (int q = 0; q < h; ++q) {
            const int64_t picked = row[q];
            ok = ok && picked != dd;
        }
        const unsigned long long m = __ballot(ok);
        const int pos = fill + __popcll(m & below);
        if (ok && pos < Q) row[pos] = dd;
        fill += __popcll(m);
    }
    fill = fill < Q ? fill : Q;
    for (int q = fill + lane; q < Q; q += 64) row[q] = -1;
}

// ---- per-query filter lists (tpnet_neg_filter_lists; the rule: include/tpnet_hip.h) -------------------------------------------------
// One wave per query i = (s, d, t): the source's run [e0, e0 + R) of the table IS its distinct destinations in ascending order; 64 per
// step, the excluded ones inside [lo, hi) (known: all of them; same_time: those that occur at exactly t) compacted by a ballot into
// fil[i, 0 .. F) in that order.  The count goes on past F: n_fil[i] is the true number.
__global__ __launch_bounds__(NEGM_BLOCK) void k_neg_filter(const uint32_t* __restrict__ hdr, const uint64_t* __restrict__ ukey,
                                                           const uint32_t* __restrict__ ustart, const double* __restrict__ times,
                                                           uint32_t E, const int64_t* __restrict__ bs, const int64_t* __restrict__ bd,
                                                           const double* __restrict__ bt, int64_t B, int mode, int64_t lo, int64_t hi,
                                                           int F, int64_t* __restrict__ fil, int32_t* __restrict__ n_fil) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * (NEGM_BLOCK / 64) + (threadIdx.x >> 6);
    if (i >= B) return;                                          // (a whole wave leaves: no workgroup barrier below)
    const uint32_t U = hdr[NEG_U];
    const int64_t s = bs[i], d = bd[i];
    const double t = bt[i];
    int64_t* row = fil + i * (int64_t)F;
    const unsigned long long below = (1ull << lane) - 1ull;
    uint32_t e0 = 0, R = 0;
    if ((uint64_t)s < (1ull << 31)) {                            // (no edge of the table has another source)
        e0 = key_lower_bound(ukey, 0, U, (uint64_t)s << 32);
        R = key_lower_bound(ukey, e0, U, ((uint64_t)s + 1) << 32) - e0;
    }
    int64_t n = 0;
    for (uint32_t base = 0; base < R; base += 64) {
        const uint32_t j = base + (uint32_t)lane;
        bool ok = false;
        int64_t dd = 0;
        if (j < R) {
            const uint32_t e = e0 + j;
            dd = (int64_t)(ukey[e] & 0xFFFFFFFFull);
            ok = dd != d && dd >= lo && dd < hi && (mode == TPNET_FILTER_KNOWN || occurs_at(ustart, times, U, E, e, t));
        }
        const unsigned long long m = __ballot(ok);
        const int64_t pos = n + __popcll(m & below);
        if (ok && pos < F) row[pos] = dd;
        n += __popcll(m);
    }
    if (lane == 0) n_fil[i] = (int32_t)n;                        // (R < 2^30)
    for (int64_t q = n + lane; q < F; q += 64) row[q] = -1;
}

// ---- layouts ---------------------------------------------------------------------------------------------------------------------
struct NegView {
    uint32_t* hdr; uint64_t* ukey; double* ufirst; uint32_t* ustart; uint8_t* uobs; double* times; int64_t* us; int64_t* ud;
    uint64_t* k_a; uint64_t* k_b; uint32_t* ix_a; uint32_t* ix_b; uint32_t* d_a; uint32_t* d_b; uint32_t* blk; Arena::Span tmp;
};
static void neg_layout(Arena& a, NegView& v, int64_t E) {
    const size_t n = (size_t)(E < 1 ? 1 : E);
    a.head();
    v.hdr = a.take<uint32_t>(64);
    v.ukey = a.take<uint64_t>(n);
    v.ufirst = a.take<double>(n);
    v.ustart = a.take<uint32_t>(n);
    v.uobs = a.take<uint8_t>(n);
    v.times = a.take<double>(n);
    v.us = a.take<int64_t>(n);
    v.ud = a.take<int64_t>(n);
    v.k_a = a.take<uint64_t>(n);
    v.k_b = a.take<uint64_t>(n);
    v.ix_a = a.take<uint32_t>(n);
    v.ix_b = a.take<uint32_t>(n);
    v.d_a = a.take<uint32_t>(n);
    v.d_b = a.take<uint32_t>(n);
    v.blk = a.take<uint32_t>(n / 256 + 2);
    v.tmp = a.rest();
    const size_t t1 = sort_pairs_tmp<uint64_t, uint32_t>(n), t2 = sort_keys_tmp<uint32_t>(n);
    a.skip(t1 > t2 ? t1 : t2);
    a.skip(256);                                     // tail slack
}
static NegView neg_view(const void* neg, size_t bytes, int64_t E) {
    Arena a(const_cast<void*>(neg), bytes);
    NegView v;
    neg_layout(a, v, E);
    return v;
}

struct NegScratch {
    uint32_t* words; uint8_t* flag; uint32_t* blk; uint32_t* cand; uint64_t* valid; uint64_t* b_a; uint64_t* b_b; Arena::Span tmp;
};
static void scratch_layout(Arena& a, NegScratch& v, int64_t E, int64_t size, int64_t B) {
    const size_t n = (size_t)(E < 1 ? 1 : E);
    const size_t nb = B > NEG_HASH_MAX_B ? (size_t)B : 1;         // the batch's keys are sorted only beyond the LDS hash table
    a.head();
    v.words = a.take<uint32_t>(64);
    v.flag = a.take<uint8_t>(n);
    v.blk = a.take<uint32_t>(n / 256 + 2);
    v.cand = a.take<uint32_t>(n);
    v.valid = a.take<uint64_t>((size_t)(size < 1 ? 1 : size));
    v.b_a = a.take<uint64_t>(nb);
    v.b_b = a.take<uint64_t>(nb);
    v.tmp = a.rest();
    a.skip(B > NEG_HASH_MAX_B ? sort_keys_tmp<uint64_t>((size_t)B) : 0);
    a.skip(256);                                     // tail slack
}

}  // namespace tpnet

using namespace tpnet;

extern "C" {

size_t tpnet_neg_bytes(int64_t E) {
    if (E < 1 || E >= (1ll << 30)) return 0;
    return measured([&](Arena& a) { NegView v; neg_layout(a, v, E); });
}

int tpnet_neg_build(void* neg, size_t neg_bytes, const int64_t* src, const int64_t* dst, const double* t, int64_t E,
                    double last_observed_time, int32_t has_observed, int64_t* counts, void* stream) {
    if (!neg || !src || !dst || !counts || E < 1 || E >= (1ll << 30)) return TPNET_ERR_BAD_ARG;
    if (neg_bytes < tpnet_neg_bytes(E)) return TPNET_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    NegView v = neg_view(neg, neg_bytes, E);
    const size_t n = (size_t)E;
    const uint32_t n32 = (uint32_t)E;
    const int grid = grid_1d(E, 4096);
    TPNET_HIP_TRY(hipMemsetAsync(v.hdr, 0, 256, s));
    // stable sort by time, then stable sort by (src, dst)  ==  sort by (edge, time)
    hipLaunchKernelGGL(k_neg_keys, dim3(grid), dim3(256), 0, s, src, dst, t, E, v.k_a, v.ix_a, v.hdr);
    TPNET_HIP_TRY(rocprim::radix_sort_pairs(v.tmp.ptr, v.tmp.bytes, v.k_a, v.k_b, v.ix_a, v.ix_b, n, 0u, 64u, s, false));
    hipLaunchKernelGGL(k_neg_edgekeys, dim3(grid), dim3(256), 0, s, src, dst, E, v.ix_b, v.k_a);
    TPNET_HIP_TRY(rocprim::radix_sort_pairs(v.tmp.ptr, v.tmp.bytes, v.k_a, v.k_b, v.ix_b, v.ix_a, n, 0u, 64u, s, false));
    hipLaunchKernelGGL(k_neg_times, dim3(grid), dim3(256), 0, s, t, E, v.ix_a, v.k_b, v.times, v.d_a);
    TPNET_HIP_TRY(rocprim::radix_sort_keys(v.tmp.ptr, v.tmp.bytes, v.d_a, v.d_b, n, 0u, 32u, s, false));
    // the table of unique edges, then the sorted unique src and dst ids: three scans over the same tile sums
    scan_compact(HeadEdge{v.k_b}, EmitEdge{v.k_b, v.times, v.ukey, v.ustart, v.ufirst, v.uobs, last_observed_time, (int)has_observed},
                 nullptr, n32, v.blk, v.hdr + NEG_U, grid, s);
    scan_compact(HeadSrc{v.k_b}, EmitSrc{v.k_b, v.us}, nullptr, n32, v.blk, v.hdr + NEG_NUS, grid, s);
    scan_compact(HeadDst{v.d_b}, EmitDst{v.d_b, v.ud}, nullptr, n32, v.blk, v.hdr + NEG_NUD, grid, s);
    TPNET_HIP_TRY(hipGetLastError());
    uint32_t h[8] = {0};
    TPNET_HIP_TRY(hipMemcpyAsync(h, v.hdr, sizeof(h), hipMemcpyDeviceToHost, s));
    TPNET_HIP_TRY(hipStreamSynchronize(s));
    if (h[NEG_BAD]) return TPNET_ERR_INDEX;
    counts[0] = h[NEG_U];
    counts[1] = h[NEG_NUS];
    counts[2] = h[NEG_NUD];
    return TPNET_OK;
}

int tpnet_neg_uniques(const void* neg, int64_t E, int64_t n_src, int64_t n_dst, int64_t* unique_src, int64_t* unique_dst,
                      void* stream) {
    if (!neg || E < 1 || E >= (1ll << 30) || n_src < 0 || n_dst < 0 || n_src > E || n_dst > E || (n_src > 0 && !unique_src) ||
        (n_dst > 0 && !unique_dst))
        return TPNET_ERR_BAD_ARG;
    NegView v = neg_view(neg, 0, E);
    if (n_src) TPNET_HIP_TRY(hipMemcpyAsync(unique_src, v.us, (size_t)n_src * 8, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    if (n_dst) TPNET_HIP_TRY(hipMemcpyAsync(unique_dst, v.ud, (size_t)n_dst * 8, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return TPNET_OK;
}

size_t tpnet_neg_scratch_bytes(int64_t E, int64_t size, int64_t B) {
    if (E < 1 || E >= (1ll << 30) || size < 0 || size >= (1ll << 31) || B < 0 || B >= (1ll << 31)) return 0;
    return measured([&](Arena& a) { NegScratch w; scratch_layout(a, w, E, size, B); });
}

int tpnet_neg_sample(void* neg, int64_t E, int32_t strategy, int64_t size, const int64_t* batch_src, const int64_t* batch_dst,
                     int64_t B, double t0, double t1, uint64_t seed, uint32_t call_index, void* scratch, size_t scratch_bytes,
                     int64_t* out_src, int64_t* out_dst, void* stream) {
    if (!neg || E < 1 || E >= (1ll << 30) || strategy < TPNET_NEG_RANDOM || strategy > TPNET_NEG_INDUCTIVE || size < 0 ||
        size >= (1ll << 31) || B < 0 || B >= (1ll << 31) || (size > 0 && (!out_src || !out_dst)))
        return TPNET_ERR_BAD_ARG;
    if (strategy != TPNET_NEG_RANDOM && (!scratch || (B > 0 && (!batch_src || !batch_dst)))) return TPNET_ERR_BAD_ARG;
    if (size == 0) return TPNET_OK;
    hipStream_t s = (hipStream_t)stream;
    NegView v = neg_view(neg, 0, E);
    const NegKey key{(uint32_t)seed, (uint32_t)(seed >> 32), call_index};
    if (strategy == TPNET_NEG_RANDOM) {
        hipLaunchKernelGGL(k_neg_random, dim3(grid_1d(size, 1024)), dim3(256), 0, s, v.us, v.ud, v.hdr, size, key, out_src, out_dst);
        TPNET_HIP_TRY(hipGetLastError());
        return TPNET_OK;
    }
    if (scratch_bytes < tpnet_neg_scratch_bytes(E, size, B)) return TPNET_ERR_WORKSPACE;
    Arena wa(scratch, scratch_bytes);
    NegScratch w;
    scratch_layout(wa, w, E, size, B);
    const int grid = grid_1d(E, 1024);
    const uint32_t* U = v.hdr + NEG_U;
    const CandFlag cf{v.ufirst, v.ustart, v.uobs, v.times, v.hdr, (uint32_t)E, t0, t1, strategy == TPNET_NEG_INDUCTIVE, w.flag};
    scan_count(cf, U, 0u, w.blk, w.words, grid, s);
    hipLaunchKernelGGL((k_scan_emit<ByteFlag, EmitCand>), dim3(grid), dim3(256), 0, s, ByteFlag{w.flag}, EmitCand{w.cand}, U, 0u,
                       (const uint32_t*)w.blk);                 // (the flags the count pass left, not the search again)
    const uint64_t* bsorted = nullptr;
    if (B > NEG_HASH_MAX_B) {
        hipLaunchKernelGGL(k_neg_bkeys, dim3(grid_1d(B, 1024)), dim3(256), 0, s, batch_src, batch_dst, B, w.b_a);
        TPNET_HIP_TRY(rocprim::radix_sort_keys(w.tmp.ptr, w.tmp.bytes, w.b_a, w.b_b, (size_t)B, 0u, 64u, s, false));
        bsorted = w.b_b;
    }
    hipLaunchKernelGGL(k_neg_pick, dim3(grid_1d(size, 1024)), dim3(256), 0, s, v.hdr, v.us, v.ud, v.ukey, w.cand, w.words, size,
                       batch_src, batch_dst, B, bsorted, w.valid, key, out_src, out_dst);
    TPNET_HIP_TRY(hipGetLastError());
    return TPNET_OK;
}

int tpnet_neg_check(void* neg, void* stream) {
    if (!neg) return TPNET_ERR_BAD_ARG;
    uint32_t* err = (uint32_t*)align256((size_t)neg) + NEG_ERR;      // (the header leads the layout)
    uint32_t h = 0;
    TPNET_HIP_TRY(hipMemcpyAsync(&h, err, sizeof(h), hipMemcpyDeviceToHost, (hipStream_t)stream));
    TPNET_HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    if (h != 0) {
        TPNET_HIP_TRY(hipMemsetAsync(err, 0, sizeof(h), (hipStream_t)stream));
        return TPNET_ERR_BAD_ARG;
    }
    return TPNET_OK;
}

int tpnet_neg_sample_many(const void* neg, int64_t E, const int64_t* batch_src, const int64_t* batch_dst, const double* batch_t,
                          int64_t B, int32_t Q, int32_t Qh, uint64_t seed, uint32_t call_index, int64_t* cand, int32_t* n_hist,
                          void* stream) {
    if (!neg || E < 1 || E >= (1ll << 30) || B < 0 || B >= (1ll << 31) || Q < 1 || Q >= (1 << 16) || Qh < 0 || Qh > Q)
        return TPNET_ERR_BAD_ARG;
    if (B > 0 && (!batch_src || !batch_dst || !batch_t || !cand || !n_hist)) return TPNET_ERR_BAD_ARG;
    if (B == 0) return TPNET_OK;
    NegView v = neg_view(neg, 0, E);
    const NegKey key{(uint32_t)seed, (uint32_t)(seed >> 32), call_index};
    const int per = NEGM_BLOCK / 64;
    hipLaunchKernelGGL(k_neg_many, dim3((unsigned)((B + per - 1) / per)), dim3(NEGM_BLOCK), 0, (hipStream_t)stream,
                       (const uint32_t*)v.hdr, (const uint64_t*)v.ukey, (const uint32_t*)v.ustart, (const double*)v.ufirst,
                       (const double*)v.times, (const int64_t*)v.ud, (uint32_t)E, batch_src, batch_dst, batch_t, B, (int)Q, (int)Qh,
                       key, cand, n_hist);
    TPNET_HIP_TRY(hipGetLastError());
    return TPNET_OK;
}

int tpnet_neg_filter_lists(const void* neg, int64_t E, const int64_t* batch_src, const int64_t* batch_dst, const double* batch_t,
                           int64_t B, int32_t mode, int64_t lo, int64_t hi, int32_t F, int64_t* fil, int32_t* n_fil, void* stream) {
    if (!neg || E < 1 || E >= (1ll << 30) || B < 0 || B >= (1ll << 31) || F < 1 || F >= (1 << 16) || lo > hi ||
        (mode != TPNET_FILTER_SAME_TIME && mode != TPNET_FILTER_KNOWN))
        return TPNET_ERR_BAD_ARG;
    if (B > 0 && (!batch_src || !batch_dst || !batch_t || !fil || !n_fil)) return TPNET_ERR_BAD_ARG;
    if (B == 0) return TPNET_OK;
    NegView v = neg_view(neg, 0, E);
    const int per = NEGM_BLOCK / 64;
    hipLaunchKernelGGL(k_neg_filter, dim3((unsigned)((B + per - 1) / per)), dim3(NEGM_BLOCK), 0, (hipStream_t)stream,
                       (const uint32_t*)v.hdr, (const uint64_t*)v.ukey, (const uint32_t*)v.ustart, (const double*)v.times, (uint32_t)E,
                       batch_src, batch_dst, batch_t, B, (int)mode, lo, hi, (int)F, fil, n_fil);
    TPNET_HIP_TRY(hipGetLastError());
    return TPNET_OK;
}

}  // extern "C"
