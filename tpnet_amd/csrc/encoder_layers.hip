// The encoder's readout (models/TPNet.py:311-324) on the matrix cores for num_layer L = 1, 2, 4, behind TPNET_FLAG_LAYERS_MFMA: the
// Gram walk of encoder_mfma.hip (L = 3) with the tile geometry and the block scatter as functions of the layer count.  Arithmetic,
// operand layout, row fetch and masked last step are that file's (encoder_rows.hpp, mfma_split.hpp: v_mfma_f32_16x16x32_bf16 on
// three-piece operands, mm6, fp32 class).  With LT = L + 1 rows per node:
//
//   L   neighbours per tile   live rows    anchor operand: nodes x 2 sides x LT   feature row
//       NB = 16 / LT          NB LT        NA = 16 / (2 LT), live rows            F = (2 LT)^2 floats
//   1   8                     16           4 nodes, 16 rows                        16  (64 bytes)
//   2   5                     15           2 nodes, 12 rows                        36  (144 bytes)
//   4   3                     15           1 node,  10 rows                        100 (400 bytes)
//
// Operand row r is neighbour r / LT, layer r % LT (anchor operand: anchor r / LT = node (r / LT) >> 1, side (r / LT) & 1); the rows
// past the live ones (and a short tile's missing neighbours) enter the products as exact zeros.
// L = 1, 2: a tile is NB consecutive slots of the flat [n_rows * K] list; with K >= 4 it spans at most 3 resp. 2 nodes, which the
// anchor operand holds.  L = 4: only ONE node's anchors fit an operand, so tiles do not straddle a node boundary -- a node's K
// slots are cut into ceil(K / 3) tiles, the last one short.  Chosen over a second anchor operand for the straddling tiles: that
// costs 12 KS more registers (the L = 3 kernel already runs at two waves per SIMD) and a third accumulation chain in EVERY tile,
// the short tile costs at most one tile in ceil(K / 3) (K = 20: 7 tiles instead of 6.67).  layer_tile below is the enumeration,
// on the host too (tpnet_encoder_layers_tile: tests/test_encoder_layers.py walks it exhaustively).
// The anchor operand is rebuilt (rows fetched, decay applied, split, own blocks formed) only when a tile leaves the node range
// [n0, n0 + NA) it stands for.  The blocks leave the accumulators through an LDS tile of 2 NB feature rows, [side][neighbour][F]
// without padding: a side's rows are contiguous there and in the output, so the store loop reads consecutive 16-byte vectors
// (conflict-free) and writes whole rows.
#include "device_common.hpp"
#include "mfma_split.hpp"
#include "encoder_rows.hpp"

namespace tpnet {

static constexpr int ELB = 256;            // threads per workgroup: 4 waves, every wave on its own tiles

template <int L>
struct LayerGeo {
    static constexpr int LT = L + 1;
    static constexpr int NB = 16 / LT;                 // neighbours per tile
    static constexpr int WR = NB * LT;                 // live rows of the neighbour operand
    static constexpr int NA = 16 / (2 * LT);           // nodes whose anchors one operand holds
    static constexpr int AR = NA * 2 * LT;             // live rows of the anchor operand
    static constexpr int FW = 2 * LT;                  // the Gram is FW x FW
    static constexpr int F = FW * FW;
    static constexpr int GT = 64 / NB;                 // tiles per group: their slots are fetched lane-parallel
    static constexpr int TILE = 2 * NB * F;            // floats of a wave's staged tile
    static constexpr bool NODE_TILES = NA == 1;        // tiles end at node boundaries
};

// tile t of the call -> its first slot and its slots (<= NB); t < layer_tiles
template <int L>
__host__ __device__ inline void layer_tile(int t, int K, int T, int& s0, int& cnt) {
    using G = LayerGeo<L>;
    if constexpr (G::NODE_TILES) {
        const int tpn = (K + G::NB - 1) / G::NB;
        const int node = t / tpn, o = (t - node * tpn) * G::NB;
        s0 = node * K + o;
        cnt = K - o < G::NB ? K - o : G::NB;
    } else {
        s0 = t * G::NB;
        cnt = T - s0 < G::NB ? T - s0 : G::NB;
    }
}
template <int L>
static inline int layer_tiles(int64_t n_rows, int K) {
    using G = LayerGeo<L>;
    if (G::NODE_TILES) return (int)(n_rows * ((K + G::NB - 1) / G::NB));
    return (int)((n_rows * K + G::NB - 1) / G::NB);
}

// g, g*g, (g*g)*g, ((g*g)*g)*g: the association of readout.hpp::decay_rows
__device__ __forceinline__ float layer_decay(float gd, int layer) {
    const float p2 = gd * gd, p3 = p2 * gd, p4 = p3 * gd;
    return layer == 0 ? 1.0f : layer == 1 ? gd : layer == 2 ? p2 : layer == 3 ? p3 : p4;
}

// load layout -> operand layout as to_lanes, a row that is not live as exact zeros; SCALE: times rs on the way
template <int KS, bool SCALE>
__device__ __forceinline__ void live_to_lanes(const float (&raw)[KS][8], bool live, float rs, int pull, float (&v)[KS][8]) {
#pragma unroll
    for (int s = 0; s < KS; ++s)
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const float x = SCALE ? raw[s][k] * rs : raw[s][k];
            v[s][k] = __int_as_float(__builtin_amdgcn_ds_bpermute(pull, __float_as_int(live ? x : 0.0f)));
        }
}

// out1 / out2: the pre-mlp features of the two anchor sides, rows [slot][F]; a wave walks tiles [wid * tpw, + tpw)
template <int L, int KS, bool FULL>
__global__ __launch_bounds__(ELB) void k_encoder_gram_mfma_layers(tpnet_state S, const int64_t* __restrict__ neigh,
                                                                  const int64_t* __restrict__ a1, const int64_t* __restrict__ a2,
                                                                  int n_rows, int K, int T, int ntiles, int tpw, double now,
                                                                  double lambda, uint32_t flags, float* __restrict__ out1,
                                                                  float* __restrict__ out2) {
    using G = LayerGeo<L>;
    constexpr int LT = G::LT, NB = G::NB, WR = G::WR, NA = G::NA, AR = G::AR, FW = G::FW, F = G::F, GT = G::GT;
    static_assert(F % 4 == 0 && GT * NB <= 64 && WR <= 16 && AR <= 16, "k_encoder_gram_mfma_layers: geometry");
    __shared__ __attribute__((aligned(16))) float stg_all[(ELB / 64) * G::TILE];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    float* const tb = stg_all + wave * G::TILE;
    const int t_begin = (blockIdx.x * (ELB / 64) + wave) * tpw;
    const int t_end = t_begin + tpw < ntiles ? t_begin + tpw : ntiles;
    if (t_begin >= t_end) return;                  // (no workgroup barrier in this kernel)

    const int c = lane & 15, g = lane >> 4;        // operand layout: row c, k-group g; accumulator q of the lane = D[4 g + q][c]
    const int lr = lane >> 2, lp = lane & 3;       // load layout: row lr, 16-byte piece lp of a 64-byte segment
    const int pull = (4 * c + g) * 4;              // ds_bpermute address: operand lane (c, g) <- load lane 4 c + g
    const int l_idx = lr / LT, l_layer = lr - l_idx * LT;      // load layout: the row's neighbour (or anchor) index and layer
    const bool l_wlive = lr < WR, l_alive = lr < AR;
    const int c_idx = c / LT, c_layer = c - c_idx * LT;        // the same for operand row c (a column of the accumulators)
    const bool c_wlive = c < WR, c_alive = c < AR;
    const int s_tile = lane / NB, s_nb = lane - s_tile * NB;   // slot layout of a group: tile of the group, neighbour of the tile
    const int d = FULL ? 32 * KS : S.d;            // row stride; KS = ceil(d / 32) steps, the last one masked when !FULL
    const int left = d - 4 * lp;
    const NodeMeta* meta = reinterpret_cast<const NodeMeta*>(S.meta);
    const bool do_scale = !(flags & TPNET_FLAG_NOT_SCALE);

    const float* const tab_p0 = S.p0;
    const float* const tab_q = S.q;
    const int64_t tab_n = S.N;
    auto row_ptr = [&](int id, int copy, int layer) -> const float* {
        const int64_t off0 = (int64_t)id * d;
        const int64_t off1 = (((int64_t)copy * tab_n + id) * L + (layer - 1)) * (int64_t)d;
        const float* b = layer == 0 ? tab_p0 : tab_q;
        return b + (layer == 0 ? off0 : off1) + 4 * lp;
    };

    int cur_n0 = -(1 << 20), pre_n0 = -(1 << 20);  // first node the anchor operands stand for; ... whose anchor rows are in flight
    SplitOp<3> anch[KS];
    f32x4 daa = {0.0f, 0.0f, 0.0f, 0.0f};
    float pre_g = 1.0f;
    float raw[KS][8], ra[KS][8];

    for (int tb0 = t_begin; tb0 < t_end; tb0 += GT) {
        const int ngt = t_end - tb0 < GT ? t_end - tb0 : GT;
        // ---- the group's slots: lane l for neighbour l % NB of tile tb0 + l / NB -- id, node (row of the call), meta record
        int gs0, gcnt, ts0, tcnt;
        layer_tile<L>(tb0, K, T, gs0, gcnt);
        layer_tile<L>(tb0 + (s_tile < ngt ? s_tile : 0), K, T, ts0, tcnt);
        const bool in = s_tile < ngt && s_nb < tcnt;
        const int j = in ? ts0 + s_nb : gs0;
        const int64_t w64 = in ? neigh[j] : 0;
        const int node = j / K;
        const bool wok = in && (uint64_t)w64 < (uint64_t)S.N;
        if (in && !wok) atomicAdd(S.err, 1u);
        const int w = wok ? (int)w64 : 0;
        // ---- the group's anchors: lane l for anchor (row nfirst + (l >> 1), side l & 1); <= 64 slots, K >= 4: <= 17 rows
        const int nfirst = gs0 / K;
        int ls0, lcnt;
        layer_tile<L>(tb0 + ngt - 1, K, T, ls0, lcnt);
        const int nlast = (ls0 + lcnt - 1) / K;
        const int an = (nfirst + (lane >> 1) < n_rows) ? nfirst + (lane >> 1) : n_rows - 1;
        const int64_t aid64 = (lane & 1) ? a2[an] : a1[an];
        const bool abad = (uint64_t)aid64 >= (uint64_t)S.N;
        if (abad && nfirst + (lane >> 1) <= nlast) atomicAdd(S.err, 1u);
        const int aid = abad ? 0 : (int)aid64;
        const unsigned long long abadmask = __ballot(abad);
        const MetaView mv = read_meta(meta, w, READER_BID, now, lambda);
        const MetaView am = read_meta(meta, aid, READER_BID, now, lambda);
        // a pair answers NaN if its neighbour or one of its row's two anchors is no valid id
        const bool pok = wok && ((abadmask >> (2 * (node - nfirst))) & 3ull) == 0;
        const unsigned long long pokmask = __ballot(pok);

        auto issue_tile = [&](int t) {             // rows of tile t of the group (load layout)
            const int sl = t * NB + (l_wlive ? l_idx : 0);
            const int wv = __shfl(w, sl), cp = __shfl(mv.copy, sl);
            load_rows<KS, FULL>(row_ptr(wv, cp, l_layer), left, raw);
        };
        auto issue_anchors = [&](int n0) {         // the anchor rows of nodes n0 .. n0 + NA - 1 (load layout)
            int al = 2 * (n0 - nfirst) + (l_alive ? l_idx : 0);   // lane that holds anchor (n0 + (l_idx >> 1), side l_idx & 1)
            al = al > 63 ? 63 : al;
            const int id = __shfl(aid, al), cp = __shfl(am.copy, al);
            pre_g = __shfl(am.g, al);
            load_rows<KS, FULL>(row_ptr(id, cp, l_layer), left, ra);
            pre_n0 = n0;
        };
        issue_tile(0);
        for (int t = 0; t < ngt; ++t) {
            int s0, cnt;
            layer_tile<L>(tb0 + t, K, T, s0, cnt);
            const int nf = s0 / K, nl = (s0 + cnt - 1) / K;
            // ---- the anchor operand and the anchors' own blocks, when the tile leaves the nodes they stand for
            if (nf < cur_n0 || nl >= cur_n0 + NA) {
                if (pre_n0 != nf) issue_anchors(nf);
                cur_n0 = nf;
                float v[KS][8];
                live_to_lanes<KS, true>(ra, l_alive, layer_decay(pre_g, l_layer), pull, v);
#pragma unroll
                for (int s = 0; s < KS; ++s) split8(v[s], anch[s]);
                daa = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                for (int s = 0; s < KS; ++s) daa = mm6(anch[s], anch[s], daa);
            }
            // ---- this tile's rows -> operand lanes; the next tile's rows (and anchors) ride under the matrix work
            float av[KS][8];
            live_to_lanes<KS, false>(raw, l_wlive && l_idx < cnt, 1.0f, pull, av);
            if (t + 1 < ngt) {
                issue_tile(t + 1);
                int s0n, cntn;
                layer_tile<L>(tb0 + t + 1, K, T, s0n, cntn);
                const int nfn = s0n / K, nln = (s0n + cntn - 1) / K;
                if (nfn < cur_n0 || nln >= cur_n0 + NA) issue_anchors(nfn);
            }
            f32x4 dww = {0.0f, 0.0f, 0.0f, 0.0f}, dwa = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                SplitOp<3> aop;
                split8(av[s], aop);
                mm6x2(aop, anch[s], dww, dwa);
            }
            // ---- pending decay as powers of g on the blocks: row r of the neighbour operand carries g(neighbour r / LT)^(r % LT)
            // (the anchors' operand is scaled when it is formed, once per anchor set)
            // (the shuffle outside the select: a lane that sits out a ds_bpermute is read as 0 by the others)
            const float gcol = __shfl(mv.g, t * NB + (c_wlive ? c_idx : 0));
            const float scol = c_wlive ? layer_decay(gcol, c_layer) : 0.0f;
            float srow[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) srow[q] = __shfl(scol, 4 * g + q);
            // (wave-uniform) two bits per neighbour of the tile: its node - cur_n0, < NA
            uint32_t nimask = 0;
            if constexpr (NA > 1) {
#pragma unroll
                for (int nb = 0; nb < NB; ++nb) {
                    const int nd = __builtin_amdgcn_readlane(node, t * NB + (nb < cnt ? nb : 0));
                    nimask |= ((uint32_t)(nd - cur_n0) & 3u) << (2 * nb);
                }
            }
            // ---- accumulators -> the LDS tile: feature row side * NB + neighbour, element FW a + b of the [w rows | anchor rows]^2 Gram
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int i = 4 * g + q;                          // accumulator row: operand row i of the first factor
                const int i_idx = i / LT, i_layer = i - i_idx * LT;
                if (i < WR && c_wlive && i_idx == c_idx) {        // w.w block of neighbour i_idx: (a, b) = (i_layer, c_layer), both sides
                    const float x = dww[q] * (srow[q] * scol);
                    tb[i_idx * F + i_layer * FW + c_layer] = x;
                    tb[(NB + i_idx) * F + i_layer * FW + c_layer] = x;
                }
                // w.anchor block: column c = anchor c_idx (node cur_n0 + (c_idx >> 1), side c_idx & 1), where that is the neighbour's node
                if (i < WR && c_alive && (uint32_t)(c_idx >> 1) == ((nimask >> (2 * i_idx)) & 3u)) {
                    const float x = dwa[q] * srow[q];
                    float* row = tb + ((c_idx & 1) * NB + i_idx) * F;
                    row[i_layer * FW + LT + c_layer] = x;
                    row[(LT + c_layer) * FW + i_layer] = x;       // mirrored
                }
                if (i < AR && c_alive && i_idx == c_idx) {        // anchor c_idx's own block -> every neighbour of its node
#pragma unroll
                    for (int nb = 0; nb < NB; ++nb)
                        if (((nimask >> (2 * nb)) & 3u) == (uint32_t)(c_idx >> 1))
                            tb[((c_idx & 1) * NB + nb) * F + (LT + i_layer) * FW + LT + c_layer] = daa[q];
                }
            }
            __builtin_amdgcn_wave_barrier();       // one wave: LDS executes in issue order
            // ---- feature rows out: clamp, log(x + 1) (models/TPNet.py:127-128); a side's cnt rows are contiguous here and there
            const uint32_t okm = (uint32_t)(pokmask >> (t * NB));
#pragma unroll
            for (int side = 0; side < 2; ++side) {
                float* o = (side ? out2 : out1) + (int64_t)s0 * F;
                const float* src = tb + side * NB * F;
#pragma unroll
                for (int it = 0; it < (NB * F / 4 + 63) / 64; ++it) {
                    const int i4 = it * 64 + lane;
                    if (i4 < cnt * (F / 4)) {
                        f32x4 v = *reinterpret_cast<const f32x4*>(src + 4 * i4);
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            float x = v[k];
                            if (do_scale) {
                                x = (x < 0.0f) ? 0.0f : x;     // NaN < 0 is false: NaN passes through, as in the reference (:127)
                                x = __builtin_amdgcn_logf(x + 1.0f) * 0.693147180559945309f;   // as in encoder_mfma.hip
                            }
                            v[k] = x;
                        }
                        if (!((okm >> ((4 * i4) / F)) & 1u))
                            v = f32x4{__builtin_nanf(""), __builtin_nanf(""), __builtin_nanf(""), __builtin_nanf("")};
                        __builtin_nontemporal_store(v, reinterpret_cast<f32x4*>(o + 4 * i4));
                    }
                }
            }
            __builtin_amdgcn_wave_barrier();       // the tile is rewritten by the next one
        }
    }
}

bool encoder_layers_supported(const tpnet_state& st, int64_t n_rows, int K) {
    static const int off = TPNET_DEV_INT(NO_ENCODER_LAYERS, 0);
    // rows of whole 16-byte vectors in 2..5 steps of 32, as the L = 3 kernels take them; K >= 4 bounds the nodes a tile spans
    return !off && (st.L == 1 || st.L == 2 || st.L == 4) && st.d % 4 == 0 && encoder_row_width(st.d) && K >= 4 &&
           st.N < (int64_t)1 << 31 && n_rows > 0 && n_rows * (int64_t)K < ((int64_t)1 << 31) / 64;
}

template <int L>
static int launch_layers(const tpnet_state& st, const int64_t* neigh, const int64_t* a1, const int64_t* a2, int64_t n_rows, int K,
                         double now, double lambda, uint32_t flags, float* out1, float* out2, hipStream_t s) {
    const int T = (int)(n_rows * K);
    const int ntiles = layer_tiles<L>(n_rows, K);
    // tiles per wave: ONE round of the waves the chip holds (encoder_mfma.hip)
    static const int waves_dev = TPNET_DEV_INT(ENCODER_WAVES, 256 * 8);
    const TileRound g = tile_round(ntiles, waves_dev, ELB / 64);
#define TPNET_EL_LAUNCH(KS_, FULL_, R8_) /* (R8_: never -- encoder_layers_supported takes d % 4 == 0 only) */                          \
    hipLaunchKernelGGL((k_encoder_gram_mfma_layers<L, KS_, FULL_>), dim3(g.grid), dim3(ELB), 0, s, st, neigh, a1, a2, (int)n_rows, K, T, \
                       ntiles, g.tpw, now, lambda, flags, out1, out2)
    TPNET_ENCODER_WIDTH_SWITCH(st.d, TPNET_EL_LAUNCH);
#undef TPNET_EL_LAUNCH
    TPNET_HIP_TRY(hipGetLastError());
    return TPNET_OK;
}

int launch_encoder_gram_layers(const tpnet_state& st, const int64_t* neigh, const int64_t* a1, const int64_t* a2, int64_t n_rows,
                               int K, double now, double lambda, uint32_t flags, float* out1, float* out2, hipStream_t s) {
    if (n_rows == 0 || K == 0) return TPNET_OK;
    if (!encoder_layers_supported(st, n_rows, K) || (flags & TPNET_FLAG_PACKED)) return TPNET_ERR_BAD_ARG;
    if ((reinterpret_cast<uintptr_t>(out1) | reinterpret_cast<uintptr_t>(out2)) & 15) return TPNET_ERR_BAD_ARG;
    switch (st.L) {
        case 1: return launch_layers<1>(st, neigh, a1, a2, n_rows, K, now, lambda, flags, out1, out2, s);
        case 2: return launch_layers<2>(st, neigh, a1, a2, n_rows, K, now, lambda, flags, out1, out2, s);
        default: return launch_layers<4>(st, neigh, a1, a2, n_rows, K, now, lambda, flags, out1, out2, s);
    }
}

}  // namespace tpnet

using namespace tpnet;

extern "C" {

int64_t tpnet_encoder_layers_tiles(int32_t L, int64_t n_rows, int32_t K) {
    if ((L != 1 && L != 2 && L != 4) || n_rows < 1 || K < 4 || n_rows * (int64_t)K >= ((int64_t)1 << 31) / 64) return 0;
    return L == 1 ? layer_tiles<1>(n_rows, K) : L == 2 ? layer_tiles<2>(n_rows, K) : layer_tiles<4>(n_rows, K);
}

int tpnet_encoder_layers_tile(int32_t L, int64_t n_rows, int32_t K, int64_t t, int64_t* first_slot, int32_t* count) {
    if (!first_slot || !count || t < 0 || t >= tpnet_encoder_layers_tiles(L, n_rows, K)) return TPNET_ERR_BAD_ARG;
    int s0 = 0, cnt = 0;
    const int T = (int)(n_rows * K);
    if (L == 1) layer_tile<1>((int)t, K, T, s0, cnt);
    else if (L == 2) layer_tile<2>((int)t, K, T, s0, cnt);
    else layer_tile<4>((int)t, K, T, s0, cnt);
    *first_slot = s0;
    *count = cnt;
    return TPNET_OK;
}

}  // extern "C"
