// The encoder's call (models/TPNet.py:311-324, then self.mlp, :129) for rows of 164..512 floats in ONE launch: the vector-ALU
// anchored walk (readout.hpp::AnchorWalk -- at these widths the readout is bound by row traffic, not arithmetic) with the dense
// layers of feature_mfma.hip's MODE 2 (dense_tile.hpp: split-bf16 operands, the fp32 class) behind it inside the kernel.  A
// workgroup of 512 threads holds 16 (32 lanes x 2 vectors: d <= 256) or 8 (64 lanes x 2 vectors) lane groups; every group takes
// one unit = (row, chunk of KC neighbours), cut exactly as k_pair_gram_anchored cuts them, and the groups step through the
// neighbour index j = 0 .. KC-1 TOGETHER: per step every group leaves its two finished feature rows (anchor side 1, side 2) in an
// LDS tile instead of in global memory, and when the tile is full (one step of 16 groups, `spt` steps of 8) the eight waves run
// self.mlp on it (W1's split operands in a wave's registers, W2's in LDS: the walk leaves no room for both) and store the output rows.  The [2 n K, 64] feature matrix of the
// two-launch path (written, then read back by the dense-layer kernel) never exists unless the caller asks for it (`gram`).
// Workgroup barriers only; every loop around a barrier has a workgroup-uniform trip count.  Groups whose unit is short, absent or
// past the end run the same steps on masked columns: computed, never stored -- a pair is one column of every matrix product.
#include "readout.hpp"
#include "dense_tile.hpp"

namespace tpnet {

// dynamic LDS of a workgroup: feature tile | four partial-output slabs | the columns' output rows | W2 split | b1
static constexpr int AF_SLAB = 32 * TS * 4, AF_DEST = 5 * AF_SLAB, AF_W2 = AF_DEST + 32 * 8, AF_B1 = AF_W2 + DENSE_W2_LDS_BYTES;
static constexpr int AF_LDS = AF_B1 + DENSE_B1_LDS_BYTES;                   // 110 336 bytes

template <int LPP, int VPL, bool FULL>
__global__ __launch_bounds__(MB) void k_anchored_feature(tpnet_state S, const int64_t* __restrict__ neigh,
                                                         const int64_t* __restrict__ a1, const int64_t* __restrict__ a2,
                                                         int64_t n_rows, int K, int KC, int spt, double now, double lambda,
                                                         uint32_t flags, const float* __restrict__ w1f, const float* __restrict__ b1,
                                                         const float* __restrict__ w2f, const float* __restrict__ b2,
                                                         float* __restrict__ gram, float* __restrict__ out) {
    constexpr int W = 4, L = 3;
    constexpr int GPB = MB / LPP;             // units in flight per workgroup
    constexpr int CPS = 2 * GPB;              // tile columns filled per step: two anchor sides per group
    using Walk = AnchorWalk<LPP, VPL, W, L, FULL>;
    static_assert(LPP * Walk::PER == MF && CPS <= 32 && 32 % CPS == 0, "k_anchored_feature: 32 or 64 lanes per unit");
    extern __shared__ __attribute__((aligned(16))) char smem[];               // AF_LDS bytes
    float* feat = reinterpret_cast<float*>(smem);
    float (*slab)[32 * TS] = reinterpret_cast<float (*)[32 * TS]>(smem + AF_SLAB);
    int64_t* dest = reinterpret_cast<int64_t*>(smem + AF_DEST);               // output row of each tile column (side * T + row * K + k), -1: masked
    const int tid = threadIdx.x;
    const int gl = tid % LPP, g = tid / LPP;
    const int lane = tid & 63, wave = tid >> 6;
    const bool do_scale = !(flags & TPNET_FLAG_NOT_SCALE);
    const int nch = (K + KC - 1) / KC;
    const int64_t units = n_rows * nch;
    const int64_t T = n_rows * (int64_t)K;    // pairs per anchor side
    // the first unit's anchor ids BEFORE the weights: vector loads return in order, and the ids head the walk's dependent chain
    const int64_t base0 = (int64_t)blockIdx.x * GPB;
    int64_t a1_0 = 0, a2_0 = 0;
    if (base0 + g < units) {
        const int64_t rr = (base0 + g) / nch;
        a1_0 = a1[rr];
        a2_0 = a2[rr];
    }
    DenseTileW<true, true> wt;                // (W1 in registers, W2 and b1 in LDS: the walk needs the rest of the 256 registers)
    dense_tile_weights_lds(wt, w1f, b1, w2f, wave, lane, reinterpret_cast<bf16x8*>(smem + AF_W2), reinterpret_cast<float*>(smem + AF_B1));

    for (int64_t base = base0; base < units; base += (int64_t)gridDim.x * GPB) {
        const int64_t un = base + g;
        const bool valid = un < units;
        const int64_t rr = valid ? un / nch : 0;
        const int ch = valid ? (int)(un - rr * nch) : 0;
        const int kb = ch * KC, ke = (kb + KC < K) ? kb + KC : K;
        const int nk_u = valid ? ke - kb : 0;              // neighbours of this group's unit
        const int64_t slot0 = rr * K + kb;
        const bool first = base == base0;
        Walk wk;
        wk.begin(S, first ? a1_0 : (valid ? a1[rr] : 0), first ? a2_0 : (valid ? a2[rr] : 0), valid, now, lambda, do_scale, gl);
        for (int j = 0; j < KC; ++j) {                     // (uniform: every group of the workgroup takes KC steps)
            const int jf = j % LPP;                        // position inside the current fetch of up to LPP ids
            if (jf == 0) {
                int nk = nk_u - j;
                nk = nk < 0 ? 0 : (nk > LPP ? LPP : nk);
                if (nk > 0 || j == 0) {
                    wk.fetch(S, neigh + (nk > 0 ? slot0 + j : 0), nk, valid, now, lambda, gl);
                    wk.issue(S, 0, gl);
                }
            }
            const bool live = j < nk_u;
            const int sub = j % spt;
            const int c1 = sub * CPS + g, c2 = c1 + GPB;   // this group's two columns of the tile: anchor side 1, side 2
            wk.step(S, jf, jf + 1 < LPP && j + 1 < nk_u, do_scale, gl, [&](int idx, float x1, float x2) {
                feat[c1 * TS + idx] = x1;
                feat[c2 * TS + idx] = x2;
            });
            if (gl == 0) {
                dest[c1] = live ? slot0 + j : -1;
                dest[c2] = live ? T + slot0 + j : -1;
            }
            if (sub == spt - 1 || j == KC - 1) {           // (uniform) the tile is full, or the units end
                __syncthreads();
                const int ncol = (sub + 1) * CPS;          // columns beyond: stale rows, computed and never stored
                const int pair = tid >> 4, o = (tid & 15) * 4;      // 512 threads x 4 floats = 32 columns x 64
                const int64_t dd = pair < ncol ? dest[pair] : -1;
                const float4 f4 = *reinterpret_cast<const float4*>(feat + pair * TS + o);
                if (gram && dd >= 0) *reinterpret_cast<float4*>(gram + dd * MF + o) = f4;      // the pre-mlp features, for a backward pass
                // a feature row that holds a NaN (an id out of range: all of it) answers a NaN row, as the torch layers do -- the
                // ReLU of the matrix-core block would turn it into b2.  A row is 16 neighbouring lanes of a wave.
                const unsigned long long nanl = __ballot(f4.x != f4.x || f4.y != f4.y || f4.z != f4.z || f4.w != f4.w);
                const bool nanrow = ((nanl >> (lane & 48)) & 0xFFFFull) != 0;
                dense_tile_partials<true>(wt, feat, slab, wave, lane);
                if (dd >= 0) {
                    const float qn = __builtin_nanf("");
                    *reinterpret_cast<float4*>(out + dd * MF + o) = nanrow ? make_float4(qn, qn, qn, qn) : dense_tile_out4(slab, b2, pair, o);
                }
                __syncthreads();                           // the tiles are reused by the next steps of this workgroup
            }
        }
    }
}

static LdsOptIn anchored_feature_lds;
static bool anchored_feature_available() {
    return anchored_feature_lds.granted({reinterpret_cast<const void*>(k_anchored_feature<32, 2, true>),
                                         reinterpret_cast<const void*>(k_anchored_feature<32, 2, false>),
                                         reinterpret_cast<const void*>(k_anchored_feature<64, 2, true>),
                                         reinterpret_cast<const void*>(k_anchored_feature<64, 2, false>)}, AF_LDS);
}

static bool wide_geom(const tpnet_state& st, Geom& gm) {
    gm = pick_geom(st.d);
    return gm.w == 4 && gm.vpl == 2 && (gm.lpp == 32 || gm.lpp == 64) && st.d <= gm.lpp * gm.vpl * 4;
}

bool encoder_wide_supported(const tpnet_state& st, int64_t n_rows, int K, const tpnet_mlp* mlp) {
    Geom gm;
    return mlp && mlp->F == 64 && mlp->H == 256 && mlp->w1 && mlp->w2f && mlp->b1 && mlp->b2 && st.L == 3 && st.d % 4 == 0 &&
           st.d >= 164 && st.d <= 512 && K >= 4 && n_rows > 0 && wide_geom(st, gm) && anchored_feature_available();
}

int encoder_wide_class(const tpnet_state& st) {
    Geom gm;
    return wide_geom(st, gm) ? gm.lpp : 0;
}

int launch_anchored_feature(const tpnet_state& st, const int64_t* neigh, const int64_t* a1, const int64_t* a2, int64_t n_rows, int K,
                            double now, double lambda, uint32_t flags, const tpnet_mlp* mlp, float* gram, float* out,
                            hipStream_t s) {
    if (!encoder_wide_supported(st, n_rows, K, mlp) || (flags & TPNET_FLAG_PACKED)) return TPNET_ERR_BAD_ARG;
    if ((reinterpret_cast<uintptr_t>(gram) | reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(mlp->b2) |
         reinterpret_cast<uintptr_t>(mlp->w1) | reinterpret_cast<uintptr_t>(mlp->w2f)) & 15)
        return TPNET_ERR_BAD_ARG;
    Geom gm;
    wide_geom(st, gm);
    const int gpb = MB / gm.lpp;
    const int kc = anchored_chunk(n_rows, K);
    const int64_t units = n_rows * ((K + kc - 1) / kc);
    // ONE workgroup per CU (the walk's registers and a wave's 96 of weights: two waves per SIMD), each loading its weights once
    static const int grid_cap = TPNET_DEV_INT(ENCODER_WIDE_GRID, 256);
    const int grid = grid_for(units, gpb, grid_cap);
    // steps per tile at 8 groups per workgroup: 2 fill the 32 columns of the matrix products, 1 leaves half of them idle
    static const int spt_dev = TPNET_DEV_INT(ENCODER_WIDE_SPT, 0);
    const int spt = gm.lpp == 32 ? 1 : (spt_dev == 1 ? 1 : 2);
#define TPNET_AF(LPP_, FULL_)                                                                                                   \
    hipLaunchKernelGGL((k_anchored_feature<LPP_, 2, FULL_>), dim3(grid), dim3(MB), AF_LDS, s, st, neigh, a1, a2, n_rows, K, kc, spt, now, \
                       lambda, flags, reinterpret_cast<const float*>(mlp->w1), mlp->b1, reinterpret_cast<const float*>(mlp->w2f),  \
                       mlp->b2, gram, out)
    const bool full = st.d == gm.lpp * gm.vpl * 4;
    if (gm.lpp == 32) { if (full) TPNET_AF(32, true); else TPNET_AF(32, false); }
    else { if (full) TPNET_AF(64, true); else TPNET_AF(64, false); }
#undef TPNET_AF
    TPNET_HIP_TRY(hipGetLastError());
    return TPNET_OK;
}

}  // namespace tpnet
