// One source against many candidates, scored in ONE launch: tpnet_score_one_to_many.  For row i with source src[i] and every
// candidate c of that row
//   f     = G(src[i], c)                      the fan-out readout's finished features, source's layers first (readout.hpp::FanWalk)
//   y     = W2m . relu(W1m . f + b1m) + b2m   self.mlp, 64 -> 256 -> 64 (dense_tile.hpp: split-bf16 operands, the fp32 class)
//   a     = Wd[:, off : off + 64] . y + bd    the decoder's fc1 restricted to its feature columns (not_encode: the rest meets zeros)
//   logit = wd2 . relu(a) + bd2
// and only out[i, c] is written: the 256 bytes of features per pair, their copy behind self.mlp and the decoder's hidden layer of
// the composition (fan-out readout, dense layers, decoder: three launches and more) never exist unless the caller asks for `gram`.
// The structure is k_anchored_feature's (anchored_feature.hip): a workgroup of 512 threads holds 512 / LPP lane groups; every group
// takes one unit = (row, chunk of KC columns; cut by anchored_chunk) and the groups step through their columns TOGETHER, each step
// leaving one finished feature row per group in a 32-column LDS tile.  On a full tile the eight waves run self.mlp on it (W1's split
// operands in a wave's registers, W2's in LDS), the 32 x 64 y tile goes back to LDS and a second matrix-core block forms `a`: wave w
// owns the hidden units [32 w, 32 w + 32) of the decoder, its split operands read once per workgroup from fc1.weight AS IT IS (row
// stride ldw, column offset off: no image, no prepare call), three products per term.  Bias, ReLU and the product with wd2 happen in
// the accumulators; the 16 partial sums of a column (8 waves x 2 lane halves) meet in LDS and are added in a FIXED order.
// Workgroup barriers only; every loop around a barrier has a workgroup-uniform trip count.  Groups whose unit is short, absent or
// past the end run the same steps on masked columns: computed, never stored -- a pair is one column of every matrix product, so its
// logit depends on its two nodes and the weights alone (the promises: include/tpnet_hip.h).  No floating-point atomics.
// The EPILOGUE of a finished column is a policy: ScoreStore writes the logit (tpnet_score_one_to_many); ScoreRank compares it with the
// row's positive logit and counts (tpnet_score_rank_range: ranking against a whole id range without the logit matrix) -- the walk,
// the two matrix-core blocks and the fixed-order sum exist once, so the logit that is compared is the logit that would be stored.
// ScoreTopK keeps each unit's K best candidates as 64-bit keys in LDS (tpnet_score_topk_range: the K best ids of a whole range per
// source, again without the logit matrix); a second kernel, k_score_topk_rows, selects a row's K best among its units' lists.
#include "readout.hpp"
#include "dense_tile.hpp"

namespace tpnet {

// dynamic LDS of a workgroup: feature / y tile | four partial-output slabs | the columns' output slots | W2 split | b1 |
// the decoder's bias and second layer (padded to 256 units) | the columns' NaN marks | the 16 partial sums of each column
static constexpr int SF_SLAB = 32 * TS * 4, SF_DEST = 5 * SF_SLAB, SF_W2 = SF_DEST + 32 * 8, SF_B1 = SF_W2 + DENSE_W2_LDS_BYTES;
static constexpr int SF_BD = SF_B1 + DENSE_B1_LDS_BYTES, SF_WD2 = SF_BD + 256 * 4, SF_NAN = SF_WD2 + 256 * 4, SF_PART = SF_NAN + 32 * 4;
static constexpr int SF_LDS = SF_PART + 16 * 32 * 4;                        // 114 560 bytes
// ScoreRank only, behind them: the units' counters {g, e, nv, flags} | the units' positive logits
static constexpr int SF_CNT = SF_LDS, SF_POSL = SF_CNT + 32 * 16, SF_LDS_RANK = SF_POSL + 32 * 4;      // 115 200 bytes
// ScoreTopK only, behind SF_LDS: the units' thresholds (their smallest kept key) | their counts | the threshold's slot | the groups'
// exclusion cursors {entry, entries, the step that meets it} | the units' lists of K keys each -- sized by the call's K, 148 352
// bytes at K = 128
static constexpr int SF_TK_MIN = SF_LDS, SF_TK_CNT = SF_TK_MIN + 32 * 8, SF_TK_SLOT = SF_TK_CNT + 32 * 4, SF_TK_CUR = SF_TK_SLOT + 32 * 4;
static constexpr int SF_TK_KEYS = SF_TK_CUR + 32 * 16;
static constexpr int sf_lds_topk(int K) { return SF_TK_KEYS + 32 * K * 8; }

struct score_dec {
    const float *wd, *bd, *wd2, *bd2;         // fc1.weight [H][ldw], fc1.bias [H], fc2.weight [1][H], fc2.bias [1]
    int ldw, off, H;
};

// the epilogue policies.  ScoreStore: out[slot] = logit (gram: optional copy of the features).  ScoreRank: row i's columns are the ids
// cand_lo + k (range mode, no lead); a column whose id is not pos[i] is COUNTED against p = pos_logit[i]: g += q > p, e += q == p,
// nv += 1, flags |= 2 where q or p is NaN.  A unit's four integers live in LDS (thread u < GPB of the workgroup owns unit u's: plain
// adds, no atomics) and leave the workgroup once, as the 16-byte record rec[unit].
// ScoreTopK: range mode without a lead, as ScoreRank; a column whose id is skip[i] (optional) or on row i's exclusion list (optional:
// excl [n_rows][F] ascending, distinct, -1 padded, n_excl its true length) is left out; every other column's logit and column
// index form a 64-bit key (score_topk_key: larger = better, unique inside a row) and thread u < GPB keeps unit u's K best in LDS.
// At the units' end their lists leave the workgroup once, best first: decoded into ids / logits / info where a row is one unit,
// else as the record keys[unit][min(K, KC)] for k_score_topk_rows.
// The body is ONE inlined function; the three kernels below hand it their own (restrict-qualified) arguments.
__device__ __forceinline__ unsigned long long score_topk_key(float q, uint32_t col) {
    uint32_t b = __float_as_uint(q), hi = 0xFFFFFFFFu;                       // NaN: above everything, as in torch.topk
    if (q == q) {
        if (b == 0x80000000u) b = 0u;                                         // -0.0 ties with +0.0
        hi = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    }
    return ((unsigned long long)hi << 32) | (unsigned long long)(0xFFFFFFFFu - col);
}
__device__ __forceinline__ float score_topk_logit(unsigned long long key) {
    const uint32_t hi = (uint32_t)(key >> 32);
    if (key == 0ull) return -__builtin_inff();                                // an empty slot
    if (hi == 0xFFFFFFFFu) return __builtin_nanf("");
    return __uint_as_float((hi & 0x80000000u) ? (hi ^ 0x80000000u) : ~hi);
}
__device__ __forceinline__ int64_t score_topk_id(unsigned long long key, int64_t cand_lo) {
    return key == 0ull ? -1 : cand_lo + (int64_t)(0xFFFFFFFFu - (uint32_t)key);
}

struct ScoreStore {
    static constexpr bool RANK = false, TOPK = false;
    float* __restrict__ gram;
    float* __restrict__ out;
};
struct ScoreRank {
    static constexpr bool RANK = true, TOPK = false;
    const int64_t* __restrict__ pos;
    const float* __restrict__ pos_logit;
    int4* __restrict__ rec;
};
struct ScoreTopK {
    static constexpr bool RANK = false, TOPK = true;
    const int64_t* __restrict__ skip;          // (may be null)
    const int64_t* __restrict__ excl;          // (may be null)
    const int32_t* __restrict__ n_excl;
    int F, K;
    unsigned long long* __restrict__ keys;     // several units per row: their records
    int64_t* __restrict__ ids;                 // one unit per row: the outputs
    float* __restrict__ logits;
    int32_t* __restrict__ info;
};

template <int LPP, int VPL, bool FULL, class Epi>
__device__ __forceinline__ void score_fanout_body(const tpnet_state& S, const int64_t* __restrict__ src, const int64_t* __restrict__ cand,
                                                  const int64_t* __restrict__ lead, int64_t cand_lo, int64_t n_rows, int C, int KC,
                                                  int spt, double now, double lambda, uint32_t flags, const float* __restrict__ w1f,
                                                  const float* __restrict__ b1, const float* __restrict__ w2f,
                                                  const float* __restrict__ b2, const score_dec& dec, const Epi& ep) {
    constexpr int W = 4, L = 3;
    constexpr int GPB = MB / LPP;             // units in flight per workgroup = tile columns filled per step
    using Walk = FanWalk<LPP, VPL, W, L, FULL>;
    static_assert(LPP * Walk::PER == MF && GPB <= 32 && 32 % GPB == 0, "k_score_fanout: 16, 32 or 64 lanes per unit");
    constexpr bool STORE = !Epi::RANK && !Epi::TOPK;
    extern __shared__ __attribute__((aligned(16))) char smem[];               // SF_LDS bytes (ScoreRank: SF_LDS_RANK; ScoreTopK: sf_lds_topk(K))
    float* feat = reinterpret_cast<float*>(smem);                             // the feature tile, then the y tile
    float (*slab)[32 * TS] = reinterpret_cast<float (*)[32 * TS]>(smem + SF_SLAB);
    int64_t* dest = reinterpret_cast<int64_t*>(smem + SF_DEST);               // output slot of each tile column (row * C1 + column), -1: masked
                                                                              // (ScoreRank: 0 = counted, -1: masked or the row's own positive;
                                                                              //  ScoreTopK: the column of the range, -1: masked or left out)
    float* bds = reinterpret_cast<float*>(smem + SF_BD);
    float* wd2s = reinterpret_cast<float*>(smem + SF_WD2);
    int* nans = reinterpret_cast<int*>(smem + SF_NAN);
    float* part = reinterpret_cast<float*>(smem + SF_PART);
    int4* cnt = reinterpret_cast<int4*>(smem + SF_CNT);                       // (ScoreRank) unit u of the workgroup: thread u's own
    float* posl = reinterpret_cast<float*>(smem + SF_POSL);
    unsigned long long* tmin = reinterpret_cast<unsigned long long*>(smem + SF_TK_MIN);      // (ScoreTopK) unit u: thread u's own
    int* tcnt = reinterpret_cast<int*>(smem + SF_TK_CNT);
    int* tslot = reinterpret_cast<int*>(smem + SF_TK_SLOT);
    int4* tcur = reinterpret_cast<int4*>(smem + SF_TK_CUR);                   // (ScoreTopK) group g: its lane 0's own
    unsigned long long* tkeys = reinterpret_cast<unsigned long long*>(smem + SF_TK_KEYS);
    const int tid = threadIdx.x;
    const int gl = tid % LPP, g = tid / LPP;
    const int lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const bool do_scale = !(flags & TPNET_FLAG_NOT_SCALE);
    const int hl = lead ? 1 : 0;
    const int C1 = C + hl;                    // columns of a row: [lead |] candidates
    const int nch = (C1 + KC - 1) / KC;
    const int64_t units = n_rows * nch;
    const int64_t base0 = (int64_t)blockIdx.x * GPB;

    DenseTileW<true, true> wt;                // (W1 in registers, W2 and b1 in LDS)
    dense_tile_weights_lds(wt, w1f, b1, w2f, wave, lane, reinterpret_cast<bf16x8*>(smem + SF_W2), reinterpret_cast<float*>(smem + SF_B1));
    // the decoder's A operands: unit 32 wave + r, columns off + 16 s + 8 h .. + 7 of fc1.weight; a unit of the padding reads unit 0's
    // row and takes a selected zero
    bf16x8 dh[4], dl[4];
    {
        const int u = wave * 32 + r;
        const bool real = u < dec.H;
        const float* wrow = dec.wd + (int64_t)(real ? u : 0) * dec.ldw + dec.off + 8 * h;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const float4 a = *reinterpret_cast<const float4*>(wrow + 16 * s), b = *reinterpret_cast<const float4*>(wrow + 16 * s + 4);
            const float z = 0.0f;
            split8(make_float4(real ? a.x : z, real ? a.y : z, real ? a.z : z, real ? a.w : z),
                   make_float4(real ? b.x : z, real ? b.y : z, real ? b.z : z, real ? b.w : z), dh[s], dl[s]);
        }
        if (tid < 256) {
            bds[tid] = tid < dec.H ? dec.bd[tid] : 0.0f;
            wd2s[tid] = tid < dec.H ? dec.wd2[tid] : 0.0f;
        }
    }
    const float bd2 = dec.bd2[0];
    const bool wave_has_units = wave * 32 < dec.H;
    if constexpr (Epi::RANK) {
        if (tid < GPB) cnt[tid] = make_int4(0, 0, 0, 0);
    }
    if constexpr (Epi::TOPK) {
        if (tid < GPB) tcnt[tid] = 0;
    }

    for (int64_t base = base0; base < units; base += (int64_t)gridDim.x * GPB) {
        const int64_t un = base + g;
        const bool valid = un < units;
        const int64_t rr = valid ? un / nch : 0;
        const int ch = valid ? (int)(un - rr * nch) : 0;
        const int kb = ch * KC, ke = (kb + KC < C1) ? kb + KC : C1;
        const int nk_u = valid ? ke - kb : 0;              // columns of this group's unit
        const int64_t slot0 = rr * C1 + kb;
        int own = -1;                                      // (ScoreRank) the step of this unit that meets the row's positive: not counted
        if constexpr (Epi::RANK) {
            const int64_t o = valid ? ep.pos[rr] - cand_lo - kb : -1;
            own = (o >= 0 && o < KC) ? (int)o : -1;
            if (gl == 0) posl[g] = valid ? ep.pos_logit[rr] : 0.0f;      // (read behind the tile's barriers)
        }
        // (ScoreTopK) lane 0 of the group walks the row's exclusion list beside the unit's ascending ids: `cur` = the first entry not
        // below the unit's ids met so far, nxo = the step of this unit that meets it (-1: none left in the unit).  The three integers
        // live in LDS (the lane's own words: no barrier), not in registers held across the walk
        if constexpr (Epi::TOPK) {
            const int64_t o = (valid && ep.skip) ? ep.skip[rr] - cand_lo - kb : -1;
            own = (o >= 0 && o < KC) ? (int)o : -1;
            if (gl == 0) {
                int cur = 0, ne = 0, nxo = -1;
                if (valid && ep.excl) {
                    const int64_t* __restrict__ lst = ep.excl + rr * ep.F;
                    ne = ep.n_excl[rr];
                    ne = ne < 0 ? 0 : (ne > ep.F ? ep.F : ne);
                    const int64_t first = cand_lo + kb;
                    int a = 0, b = ne;
                    while (a < b) {                        // the first entry >= the unit's first id
                        const int m = (a + b) >> 1;
                        if (lst[m] < first) a = m + 1; else b = m;
                    }
                    cur = a;
                    if (cur < ne) {
                        const int64_t o2 = lst[cur] - first;
                        nxo = (o2 >= 0 && o2 < KC) ? (int)o2 : -1;
                    }
                }
                tcur[g] = make_int4(cur, ne, nxo, 0);
            }
        }
        Walk wk;
        wk.begin(S, valid ? src[rr] : 0, valid, now, lambda, do_scale, gl);
        for (int j = 0; j < KC; ++j) {                     // (uniform: every group of the workgroup takes KC steps)
            const int jf = j % LPP;                        // position inside the current fetch of up to LPP ids
            if (jf == 0) {
                int nk = nk_u - j;
                nk = nk < 0 ? 0 : (nk > LPP ? LPP : nk);
                if (nk > 0 || j == 0) {
                    const bool has = gl < nk;
                    const int k = kb + j + gl;             // this lane's column of the row
                    int64_t id = 0;
                    if (has) id = (k < hl) ? lead[rr] : (cand ? cand[rr * C + (k - hl)] : cand_lo + (k - hl));
                    wk.fetch(S, id, has, valid, now, lambda);
                    wk.issue(S, 0, gl);
                }
            }
            const bool live = j < nk_u;
            const int sub = j % spt;
            const int c1 = sub * GPB + g;                  // this group's column of the tile
            wk.step(S, jf, jf + 1 < LPP && j + 1 < nk_u, do_scale, gl, [&](int idx, float x) { feat[c1 * TS + idx] = x; });
            if constexpr (Epi::RANK) {
                if (gl == 0) dest[c1] = (live && j != own) ? 0 : -1;
            } else if constexpr (Epi::TOPK) {
                if (gl == 0) {
                    bool adm = live && j != own;
                    if (j == tcur[g].z) {                  // on the list: left out, and the cursor moves on (entries ascend)
                        adm = false;
                        int4 c = tcur[g];
                        ++c.x;
                        c.z = -1;
                        if (c.x < c.y) {
                            const int64_t o2 = ep.excl[rr * ep.F + c.x] - cand_lo - kb;
                            c.z = (o2 > j && o2 < KC) ? (int)o2 : -1;
                        }
                        tcur[g] = c;
                    }
                    dest[c1] = adm ? kb + j : -1;
                }
            } else {
                if (gl == 0) dest[c1] = live ? slot0 + j : -1;
            }
            if (sub == spt - 1 || j == KC - 1) {           // (uniform) the tile is full, or the units end
                __syncthreads();
                const int ncol = (sub + 1) * GPB;          // columns beyond: stale rows, computed and never stored
                const int pair = tid >> 4, o = (tid & 15) * 4;      // 512 threads x 4 floats = 32 columns x 64
                int64_t dd = -1;
                if constexpr (STORE) dd = pair < ncol ? dest[pair] : -1;
                const float4 f4 = *reinterpret_cast<const float4*>(feat + pair * TS + o);
                if constexpr (STORE) {
                    if (ep.gram && dd >= 0) *reinterpret_cast<float4*>(ep.gram + dd * MF + o) = f4;      // the features as the kernel formed them
                }
                // a feature row that holds a NaN (an id out of range: all of it) answers a NaN logit, as the torch layers do -- the
                // ReLUs of the matrix-core blocks would turn it into a finite number.  A row is 16 neighbouring lanes of a wave.
                const unsigned long long nanl = __ballot(f4.x != f4.x || f4.y != f4.y || f4.z != f4.z || f4.w != f4.w);
                if ((tid & 15) == 0) nans[pair] = ((nanl >> (lane & 48)) & 0xFFFFull) != 0 ? 1 : 0;
                dense_tile_partials<true>(wt, feat, slab, wave, lane);     // (every wave is past its reads of the feature tile)
                *reinterpret_cast<float4*>(feat + pair * TS + o) = dense_tile_out4(slab, b2, pair, o);      // y, one column per pair
                __syncthreads();
                // ---- the decoder: A^T = Wd . Y^T for the wave's 32 hidden units; lane (r, h) holds Y[pair r][16 s + 8 h + j] as B operand
                float p = 0.0f;
                if (wave_has_units) {
                    f32x16 acc;
#pragma unroll
                    for (int q = 0; q < 16; ++q) acc[q] = 0.0f;
#pragma unroll
                    for (int s = 0; s < 4; ++s) {
                        bf16x8 bxh, bxl;
                        load_split8(feat + r * TS + 16 * s + 8 * h, bxh, bxl);
                        acc = mm3(dh[s], dl[s], bxh, bxl, acc);
                    }
                    // register q = hidden unit 32 wave + acc_row(q, h) of pair r: bias, ReLU, the product with wd2, in register order
#pragma unroll
                    for (int q = 0; q < 16; ++q) {
                        const int u = wave * 32 + acc_row(q, h);
                        float a = acc[q] + bds[u];
                        a = a > 0.0f ? a : 0.0f;
                        p = p + a * wd2s[u];
                    }
                }
                part[(wave * 2 + h) * 32 + r] = p;
                __syncthreads();
                if (tid < 32) {
                    float sum = 0.0f;
#pragma unroll
                    for (int i = 0; i < 16; ++i) sum = sum + part[i * 32 + tid];
                    const int64_t d1 = tid < ncol ? dest[tid] : -1;
                    if constexpr (Epi::RANK) {
                        const float q = nans[tid] ? __builtin_nanf("") : sum + bd2;        // the logit the other policy stores
                        // column tid belongs to unit tid % GPB; the columns of one unit are GPB lanes apart: folded, then thread u adds
                        const float p = posl[tid % GPB];
                        const bool on = d1 >= 0;
                        int cg = (on && q > p) ? 1 : 0, ce = (on && q == p) ? 1 : 0, cn = on ? 1 : 0;
                        int cf = (on && (q != q || p != p)) ? 2 : 0;
#pragma unroll
                        for (int o2 = GPB; o2 < 32; o2 <<= 1) {
                            cg += __shfl_xor(cg, o2, 64);
                            ce += __shfl_xor(ce, o2, 64);
                            cn += __shfl_xor(cn, o2, 64);
                            cf |= __shfl_xor(cf, o2, 64);
                        }
                        if (tid < GPB) {
                            int4 c = cnt[tid];
                            c.x += cg; c.y += ce; c.z += cn; c.w |= cf;
                            cnt[tid] = c;
                        }
                    } else if constexpr (Epi::TOPK) {
                        const float q = nans[tid] ? __builtin_nanf("") : sum + bd2;        // the logit the first policy stores
                        const unsigned long long key = d1 >= 0 ? score_topk_key(q, (uint32_t)d1) : 0ull;
                        const unsigned klo = (unsigned)key, khi = (unsigned)(key >> 32);
                        // thread u < GPB takes unit u's columns u, u + GPB, ... of the tile in column order: plain LDS, no atomics
                        const int u = tid % GPB;
                        const int K = ep.K;
                        unsigned long long* lst = tkeys + u * K;
                        int n = tcnt[u], slot = tslot[u];
                        unsigned long long mn = tmin[u];
#pragma unroll
                        for (int s2 = 0; s2 < 32 / GPB; ++s2) {
                            const int from = s2 * GPB + u;
                            const unsigned long long k2 = ((unsigned long long)__shfl(khi, from, 64) << 32) | __shfl(klo, from, 64);
                            if (tid < GPB && k2 != 0ull) {
                                if (n < K) {                   // not full: append, track the minimum
                                    lst[n] = k2;
                                    if (n == 0 || k2 < mn) { mn = k2; slot = n; }
                                    ++n;
                                } else if (k2 > mn) {          // full: almost every column ends at this compare
                                    lst[slot] = k2;
                                    mn = lst[0];
                                    slot = 0;
#pragma unroll 8
                                    for (int t = 1; t < K; ++t) {
                                        const unsigned long long x = lst[t];
                                        if (x < mn) { mn = x; slot = t; }
                                    }
                                }
                            }
                        }
                        if (tid < GPB) { tcnt[u] = n; tslot[u] = slot; tmin[u] = mn; }
                    } else {
                        if (d1 >= 0) ep.out[d1] = nans[tid] ? __builtin_nanf("") : sum + bd2;
                    }
                }
                __syncthreads();                           // the tiles are reused by the next steps of this workgroup
            }
        }
        if constexpr (Epi::RANK) {                         // the units end: their records leave, the counters start over
            if (tid < GPB) {
                int4 c = cnt[tid];
                const float p = posl[tid];
                if (p != p) c.w |= 2;                      // (a NaN positive marks the row even where nothing is counted)
                if (base + tid < units) ep.rec[base + tid] = c;
                cnt[tid] = make_int4(0, 0, 0, 0);
            }
            // (posl[g] is rewritten by the next unit's group only behind the barrier that ended the last tile; thread tid read it
            // above -- a workgroup barrier keeps that read in front of the rewrite)
            __syncthreads();
        }
        if constexpr (Epi::TOPK) {
            // the units end (behind the barrier that ended their last tile): every thread ranks entries of the lists -- entry i of
            // unit u goes to the place #{entries of u above it}; keys are distinct, so the places are -- and writes it out
            const int K = ep.K, Kc = K < KC ? K : KC;
            for (int idx = tid; idx < GPB * K; idx += MB) {
                const int u = idx / K, i = idx - u * K;
                const int64_t un2 = base + u;
                if (un2 >= units) continue;                // (no barrier inside this loop)
                const int n = tcnt[u];
                const unsigned long long* lst = tkeys + u * K;
                unsigned long long key = 0ull;
                int place = i;                             // slots n .. K - 1 stay empty
                if (i < n) {
                    key = lst[i];
                    place = 0;
                    for (int t = 0; t < n; ++t) place += lst[t] > key ? 1 : 0;
                }
                if (nch == 1) {                            // a row of one unit: un2 is the row
                    ep.ids[un2 * K + place] = score_topk_id(key, cand_lo);
                    ep.logits[un2 * K + place] = score_topk_logit(key);
                    if (place == 0) {                      // the best key (or an empty row's slot 0): a NaN sorts first
                        ep.info[2 * un2] = n;
                        ep.info[2 * un2 + 1] = ((uint32_t)(key >> 32) == 0xFFFFFFFFu ? 2 : 0) | ((ep.excl && ep.n_excl[un2] > ep.F) ? 8 : 0);
                    }
                } else if (place < Kc) {                   // (n <= Kc: a unit has at most KC columns)
                    ep.keys[un2 * Kc + place] = key;
                }
            }
            __syncthreads();
            if (tid < GPB) tcnt[tid] = 0;                  // (thread u's own word: next touched in a tile epilogue, behind barriers)
        }
    }
}

template <int LPP, int VPL, bool FULL>
__global__ __launch_bounds__(MB) void k_score_fanout(tpnet_state S, const int64_t* __restrict__ src, const int64_t* __restrict__ cand,
                                                     const int64_t* __restrict__ lead, int64_t cand_lo, int64_t n_rows, int C, int KC,
                                                     int spt, double now, double lambda, uint32_t flags,
                                                     const float* __restrict__ w1f, const float* __restrict__ b1,
                                                     const float* __restrict__ w2f, const float* __restrict__ b2, score_dec dec,
                                                     float* __restrict__ gram, float* __restrict__ out) {
    score_fanout_body<LPP, VPL, FULL>(S, src, cand, lead, cand_lo, n_rows, C, KC, spt, now, lambda, flags, w1f, b1, w2f, b2, dec,
                                      ScoreStore{gram, out});
}

// range mode without a lead: row i's columns are the ids cand_lo .. cand_lo + C - 1, counted against pos_logit[i] unless pos[i]
template <int LPP, int VPL, bool FULL>
__global__ __launch_bounds__(MB) void k_score_rank(tpnet_state S, const int64_t* __restrict__ src, const int64_t* __restrict__ pos,
                                                   const float* __restrict__ pos_logit, int64_t cand_lo, int64_t n_rows, int C, int KC,
                                                   int spt, double now, double lambda, uint32_t flags,
                                                   const float* __restrict__ w1f, const float* __restrict__ b1,
                                                   const float* __restrict__ w2f, const float* __restrict__ b2, score_dec dec,
                                                   int4* __restrict__ rec) {
    score_fanout_body<LPP, VPL, FULL>(S, src, nullptr, nullptr, cand_lo, n_rows, C, KC, spt, now, lambda, flags, w1f, b1, w2f, b2, dec,
                                      ScoreRank{pos, pos_logit, rec});
}

// a row's records summed (integers: any order gives the same words): one wave per row
__global__ __launch_bounds__(256) void k_score_rank_rows(const int4* __restrict__ rec, int64_t n_rows, int nch, int4* __restrict__ counts) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n_rows) return;                               // (a whole wave leaves: no workgroup barrier below)
    int g = 0, e = 0, nv = 0, fl = 0;
    for (int c = lane; c < nch; c += 64) {
        const int4 r = rec[i * nch + c];
        g += r.x; e += r.y; nv += r.z; fl |= r.w;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        g += __shfl_xor(g, o, 64);
        e += __shfl_xor(e, o, 64);
        nv += __shfl_xor(nv, o, 64);
        fl |= __shfl_xor(fl, o, 64);
    }
    if (lane == 0) counts[i] = make_int4(g, e, nv, fl);
}

// range mode without a lead: row i's K best ids of cand_lo .. cand_lo + C - 1 other than skip[i] and the row's exclusion list
template <int LPP, int VPL, bool FULL>
__global__ __launch_bounds__(MB) void k_score_topk(tpnet_state S, const int64_t* __restrict__ src, const int64_t* __restrict__ skip,
                                                   const int64_t* __restrict__ excl, const int32_t* __restrict__ n_excl, int F,
                                                   int64_t cand_lo, int64_t n_rows, int C, int KC, int spt, double now, double lambda,
                                                   uint32_t flags, const float* __restrict__ w1f, const float* __restrict__ b1,
                                                   const float* __restrict__ w2f, const float* __restrict__ b2, score_dec dec, int K,
                                                   unsigned long long* __restrict__ keys, int64_t* __restrict__ ids,
                                                   float* __restrict__ logits, int32_t* __restrict__ info) {
    score_fanout_body<LPP, VPL, FULL>(S, src, nullptr, nullptr, cand_lo, n_rows, C, KC, spt, now, lambda, flags, w1f, b1, w2f, b2, dec,
                                      ScoreTopK{skip, excl, n_excl, F, K, keys, ids, logits, info});
}

// a row's K best among its units' records keys[row][M] (M = nch * Kc; 0 = an empty slot): one workgroup per row.  Keys are distinct,
// so the K-th largest is found by a radix select from the top byte down -- a 256-bin histogram of the keys that share the prefix
// found so far, eight passes at most, each linear in M, ended early once a bin is taken whole -- the keys at or above it are
// gathered (in any order) and placed by their rank among themselves: the same words whatever order the lanes ran in.
__global__ __launch_bounds__(256) void k_score_topk_rows(const unsigned long long* __restrict__ keys, int64_t M, int K, int64_t cand_lo,
                                                         const int32_t* __restrict__ n_excl, int F, int64_t* __restrict__ ids,
                                                         float* __restrict__ logits, int32_t* __restrict__ info) {
    __shared__ int hist[256];
    __shared__ unsigned long long sel[SCORE_TOPK_MAX];
    __shared__ int s_bin, s_rem, s_whole, s_n;
    const int tid = threadIdx.x;
    const int64_t row = blockIdx.x;
    const unsigned long long* __restrict__ kr = keys + row * M;
    unsigned long long prefix = 0ull, mask = 0ull;
    int rem = K;
    if (tid == 0) s_n = 0;
    for (int pass = 7; pass >= 0; --pass) {                // (uniform: every thread reads the same s_bin / s_whole)
        hist[tid] = 0;
        __syncthreads();
        for (int64_t t = tid; t < M; t += 256) {
            const unsigned long long k = kr[t];
            if (k != 0ull && (k & mask) == prefix) atomicAdd(&hist[(int)(k >> (8 * pass)) & 255], 1);
        }
        __syncthreads();
        if (tid == 0) {
            int cum = 0, b = 255;
            for (; b >= 0; --b) {
                const int c = hist[b];
                if (cum + c >= rem) break;
                cum += c;
            }
            s_bin = b;                                     // -1: fewer than K keys in the row -- all of them are taken
            s_rem = rem - cum;
            s_whole = (b >= 0 && hist[b] == rem - cum) ? 1 : 0;
        }
        __syncthreads();
        const int b = s_bin;
        if (b < 0) { prefix = 1ull; break; }               // (first pass only: later passes count >= rem keys by construction)
        prefix |= (unsigned long long)b << (8 * pass);
        mask |= 0xFFull << (8 * pass);
        rem = s_rem;
        if (s_whole) break;                                // every key of this bin is wanted: the threshold is the prefix
    }
    // the keys at or above the threshold: min(K, the row's keys) of them
    for (int64_t t = tid; t < M; t += 256) {
        const unsigned long long k = kr[t];
        if (k != 0ull && k >= prefix) {
            const int p = atomicAdd(&s_n, 1);
            if (p < K) sel[p] = k;
        }
    }
    __syncthreads();
    const int n = s_n < K ? s_n : K;
    if (tid < K) {
        unsigned long long key = 0ull;
        int place = tid;
        if (tid < n) {
            key = sel[tid];
            place = 0;
            for (int t = 0; t < n; ++t) place += sel[t] > key ? 1 : 0;
        }
        ids[row * K + place] = score_topk_id(key, cand_lo);
        logits[row * K + place] = score_topk_logit(key);
        if (place == 0) {
            info[2 * row] = n;
            info[2 * row + 1] = ((uint32_t)(key >> 32) == 0xFFFFFFFFu ? 2 : 0) | ((n_excl && n_excl[row] > F) ? 8 : 0);
        }
    }
}

#define TPNET_SF_KERNELS(K_)                                                                                                       \
    {reinterpret_cast<const void*>(K_<16, 1, true>), reinterpret_cast<const void*>(K_<16, 1, false>),                                  \
     reinterpret_cast<const void*>(K_<32, 1, true>), reinterpret_cast<const void*>(K_<32, 1, false>),                                  \
     reinterpret_cast<const void*>(K_<32, 2, true>), reinterpret_cast<const void*>(K_<32, 2, false>),                                  \
     reinterpret_cast<const void*>(K_<64, 2, true>), reinterpret_cast<const void*>(K_<64, 2, false>)}
static LdsOptIn score_fanout_lds, score_rank_lds, score_topk_lds;
static bool score_fanout_available() { return score_fanout_lds.granted(TPNET_SF_KERNELS(k_score_fanout), SF_LDS); }
static bool score_rank_available() { return score_rank_lds.granted(TPNET_SF_KERNELS(k_score_rank), SF_LDS_RANK); }
static bool score_topk_available() { return score_topk_lds.granted(TPNET_SF_KERNELS(k_score_topk), sf_lds_topk(SCORE_TOPK_MAX)); }
#undef TPNET_SF_KERNELS

// host arithmetic only: the four geometries of rows of 36..512 floats in ONE chunk (16 x 1, 32 x 1, 32 x 2, 64 x 2)
static bool score_geom(const tpnet_state& st, Geom& gm) {
    gm = pick_geom(st.d);
    return gm.w == 4 && ((gm.lpp == 16 && gm.vpl == 1) || (gm.lpp == 32 && (gm.vpl == 1 || gm.vpl == 2)) || (gm.lpp == 64 && gm.vpl == 2)) &&
           st.d <= gm.lpp * gm.vpl * 4;
}

bool score_fanout_supported(const tpnet_state& st, const tpnet_mlp* mlp, int H, int off, int ldw) {
    Geom gm;
    return mlp && mlp->F == 64 && mlp->H == 256 && mlp->w1 && mlp->w2f && mlp->b1 && mlp->b2 && st.L == 3 && st.d % 4 == 0 &&
           st.d >= 36 && st.d <= 512 && score_geom(st, gm) && H >= 1 && H <= 256 && off >= 0 && off % 4 == 0 && ldw >= off + 64 &&
           ldw % 4 == 0;
}

// what both launches share: the geometry, one workgroup per CU (its LDS) that loads its weights once, 32 / gpb steps per tile
struct ScoreGrid { Geom gm; int grid, spt; bool full; };
static ScoreGrid score_grid(const tpnet_state& st, int64_t n_rows, int C1, int kc) {
    ScoreGrid g;
    score_geom(st, g.gm);
    const int gpb = MB / g.gm.lpp;
    const int64_t units = n_rows * (((int64_t)C1 + kc - 1) / kc);
    g.grid = grid_for(units, gpb, 256);
    g.spt = 32 / gpb;                                            // steps that fill the 32 columns of the matrix products
    g.full = st.d == g.gm.lpp * g.gm.vpl * 4;
    return g;
}
// K_<lanes, vectors, exact fit> for the geometry g
#define TPNET_SF_DISPATCH(g, LAUNCH)                                                                       \
    do {                                                                                                   \
        if (g.gm.lpp == 16) { if (g.full) LAUNCH(16, 1, true); else LAUNCH(16, 1, false); }                \
        else if (g.gm.vpl == 1) { if (g.full) LAUNCH(32, 1, true); else LAUNCH(32, 1, false); }            \
        else if (g.gm.lpp == 32) { if (g.full) LAUNCH(32, 2, true); else LAUNCH(32, 2, false); }           \
        else { if (g.full) LAUNCH(64, 2, true); else LAUNCH(64, 2, false); }                               \
    } while (0)

int launch_score_fanout(const tpnet_state& st, const int64_t* src, const int64_t* cand, int64_t cand_lo, const int64_t* lead,
                        int64_t n_rows, int C, double now, double lambda, uint32_t flags, const tpnet_mlp* mlp, const float* wd, int ldw,
                        int off, const float* bd, const float* wd2, const float* bd2, int H, float* gram, float* out, hipStream_t s) {
    if (!score_fanout_supported(st, mlp, H, off, ldw)) return TPNET_ERR_BAD_ARG;
    if (!score_fanout_available()) return TPNET_ERR_HIP;         // (a device that does not give a workgroup 112 KB of LDS)
    const int C1 = C + (lead ? 1 : 0);
    const int kc = anchored_chunk(n_rows, C1);
    const ScoreGrid g = score_grid(st, n_rows, C1, kc);
    const score_dec dec = {wd, bd, wd2, bd2, ldw, off, H};
#define TPNET_SF(LPP_, VPL_, FULL_)                                                                                            \
    hipLaunchKernelGGL((k_score_fanout<LPP_, VPL_, FULL_>), dim3(g.grid), dim3(MB), SF_LDS, s, st, src, cand, lead, cand_lo, n_rows, C, \
                       kc, g.spt, now, lambda, flags, reinterpret_cast<const float*>(mlp->w1), mlp->b1,                        \
                       reinterpret_cast<const float*>(mlp->w2f), mlp->b2, dec, gram, out)
    TPNET_SF_DISPATCH(g, TPNET_SF);
#undef TPNET_SF
    TPNET_HIP_TRY(hipGetLastError());
    return TPNET_OK;
}

// one 16-byte record per unit; a row of ONE unit writes its counts itself (no records, no third launch)
static int64_t score_rank_chunks(int64_t n_rows, int C, int* kc) {
    *kc = anchored_chunk(n_rows, C);
    return ((int64_t)C + *kc - 1) / *kc;
}

size_t score_rank_scratch_bytes(int64_t n_rows, int C) {
    if (n_rows < 0 || n_rows >= (1ll << 31) || C < 1) return 0;
    int kc;
    const int64_t nch = score_rank_chunks(n_rows, C, &kc);
    return 16 + (nch > 1 ? (size_t)n_rows * (size_t)nch * sizeof(int4) : 0);
}

int launch_score_rank(const tpnet_state& st, const int64_t* src, const int64_t* pos, int64_t cand_lo, int64_t n_rows, int C, double now,
                      double lambda, uint32_t flags, const tpnet_mlp* mlp, const float* wd, int ldw, int off, const float* bd,
                      const float* wd2, const float* bd2, int H, void* scratch, size_t scratch_bytes, float* pos_logit, int32_t* counts,
                      hipStream_t s) {
    if (!score_fanout_supported(st, mlp, H, off, ldw)) return TPNET_ERR_BAD_ARG;
    if (scratch_bytes < score_rank_scratch_bytes(n_rows, C)) return TPNET_ERR_WORKSPACE;
    if (!score_rank_available()) return TPNET_ERR_HIP;
    // (1) the positives' logits: the storing kernel as it is, list mode, one candidate per row
    const int rc = launch_score_fanout(st, src, pos, 0, nullptr, n_rows, 1, now, lambda, flags, mlp, wd, ldw, off, bd, wd2, bd2, H,
                                       nullptr, pos_logit, s);
    if (rc) return rc;
    // (2) the range, counted against them
    int kc;
    const int64_t nch = score_rank_chunks(n_rows, C, &kc);
    const ScoreGrid g = score_grid(st, n_rows, C, kc);
    const score_dec dec = {wd, bd, wd2, bd2, ldw, off, H};
    int4* rec = nch > 1 ? reinterpret_cast<int4*>(scratch) : reinterpret_cast<int4*>(counts);
#define TPNET_SR(LPP_, VPL_, FULL_)                                                                                              \
    hipLaunchKernelGGL((k_score_rank<LPP_, VPL_, FULL_>), dim3(g.grid), dim3(MB), SF_LDS_RANK, s, st, src, pos, (const float*)pos_logit, \
                       cand_lo, n_rows, C, kc, g.spt, now, lambda, flags, reinterpret_cast<const float*>(mlp->w1), mlp->b1,      \
                       reinterpret_cast<const float*>(mlp->w2f), mlp->b2, dec, rec)
    TPNET_SF_DISPATCH(g, TPNET_SR);
#undef TPNET_SR
    TPNET_HIP_TRY(hipGetLastError());
    // (3) several units per row: their records, added
    if (nch > 1) {
        hipLaunchKernelGGL(k_score_rank_rows, dim3((unsigned)((n_rows + 3) / 4)), dim3(256), 0, s, (const int4*)rec, n_rows, (int)nch,
                           reinterpret_cast<int4*>(counts));
        TPNET_HIP_TRY(hipGetLastError());
    }
    return TPNET_OK;
}

// one record of Kc = min(K, KC) keys per unit; a row of ONE unit writes its outputs itself (no records, no second launch)
size_t score_topk_scratch_bytes(int64_t n_rows, int C, int K) {
    if (n_rows < 0 || n_rows >= (1ll << 31) || C < 1 || K < 1 || K > SCORE_TOPK_MAX) return 0;
    int kc;
    const int64_t nch = score_rank_chunks(n_rows, C, &kc);
    const int Kc = K < kc ? K : kc;
    return 16 + (nch > 1 ? (size_t)n_rows * (size_t)nch * (size_t)Kc * 8 : 0);
}

int launch_score_topk(const tpnet_state& st, const int64_t* src, const int64_t* skip, const int64_t* excl, const int32_t* n_excl, int F,
                      int64_t cand_lo, int64_t n_rows, int C, int K, double now, double lambda, uint32_t flags, const tpnet_mlp* mlp,
                      const float* wd, int ldw, int off, const float* bd, const float* wd2, const float* bd2, int H, void* scratch,
                      size_t scratch_bytes, int64_t* ids, float* logits, int32_t* info, hipStream_t s) {
    if (!score_fanout_supported(st, mlp, H, off, ldw) || K < 1 || K > SCORE_TOPK_MAX) return TPNET_ERR_BAD_ARG;
    const size_t need = score_topk_scratch_bytes(n_rows, C, K);
    if (need == 0) return TPNET_ERR_BAD_ARG;
    if (scratch_bytes < need) return TPNET_ERR_WORKSPACE;
    if (!score_topk_available()) return TPNET_ERR_HIP;
    int kc;
    const int64_t nch = score_rank_chunks(n_rows, C, &kc);
    const int Kc = K < kc ? K : kc;
    const ScoreGrid g = score_grid(st, n_rows, C, kc);
    const score_dec dec = {wd, bd, wd2, bd2, ldw, off, H};
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(scratch);
#define TPNET_ST(LPP_, VPL_, FULL_)                                                                                              \
    hipLaunchKernelGGL((k_score_topk<LPP_, VPL_, FULL_>), dim3(g.grid), dim3(MB), sf_lds_topk(K), s, st, src, skip, excl, n_excl, F,   \
                       cand_lo, n_rows, C, kc, g.spt, now, lambda, flags, reinterpret_cast<const float*>(mlp->w1), mlp->b1,      \
                       reinterpret_cast<const float*>(mlp->w2f), mlp->b2, dec, K, keys, ids, logits, info)
    TPNET_SF_DISPATCH(g, TPNET_ST);
#undef TPNET_ST
    TPNET_HIP_TRY(hipGetLastError());
    if (nch > 1) {                                             // several units per row: the K best of their records
        hipLaunchKernelGGL(k_score_topk_rows, dim3((unsigned)n_rows), dim3(256), 0, s, (const unsigned long long*)keys, nch * (int64_t)Kc,
                           K, cand_lo, n_excl, F, ids, logits, info);
        TPNET_HIP_TRY(hipGetLastError());
    }
    return TPNET_OK;
}
#undef TPNET_SF_DISPATCH

}  // namespace tpnet
