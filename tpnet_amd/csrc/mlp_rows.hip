// self.mlp = Linear(F, 4F) -> ReLU -> Linear(4F, F) (models/TPNet.py:63-65, 129) for rp_num_layer L = 1 and L = 2 (F = (2L+2)^2 = 16
// and 36, H = 64 and 144) on rows of features that already exist ([n][F] f32), fp32 class, for LONG lists.  The tile walk is
// mlp_wave_tile.hpp's, the one k_mlp64_x3 (mlp_x3.hip) runs for L = 3: same arithmetic, same mapping, the padded geometry
// MlpRowsGeo<L> and its PADDING RULES stated there.  This file holds the staging of the split weights from w1t / w2t, the
// occupancy of two workgroups per CU and the launch rule.
#include "tpnet_common.h"
#include "mlp_wave_tile.hpp"

namespace tpnet {

static constexpr int R_GRID = 512;                    // workgroups per launch at most: two per CU (two LDS images of L = 2 fit a CU's 160 KB)

// w1t = f32 [F][H] (mlp[0].weight transposed), w2t = f32 [H][F] (mlp[2].weight transposed): tpnet_mlp's fields for every F
template <int L>
__global__ __launch_bounds__(WT_BLOCK) __attribute__((amdgpu_waves_per_eu(4, 4)))      // two workgroups per CU: 128 registers per lane
void k_mlp_rows_x3(const float* __restrict__ X, int64_t n, const float* __restrict__ w1t, const float* __restrict__ b1,
                   const float* __restrict__ w2t, const float* __restrict__ b2, float* __restrict__ Y, int nact) {
    using G = MlpRowsGeo<L>;
    constexpr int F = G::F, H = G::H, KS = G::KS, NT = G::NT;
    // ---- the split weights -> LDS, walked in the order of the image (consecutive lanes write consecutive 16-byte slots and read
    // consecutive floats of a row of w1t / w2t); padded k positions, hidden units and outputs are zeros
    auto stage = [&](char* smem, int tid) {
        for (int i = tid; i < G::W1_SLOTS; i += WT_BLOCK) {                  // W1: slot ((w * KS + s) * 64 + lane (h, r))
            const int ws = i >> 6, w = ws / KS, s = ws - w * KS, hh = (i >> 5) & 1, rr = i & 31;
            const int hid = 32 * w + rr, k0 = 16 * s + 8 * hh;
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = (hid < H && k0 + j < F) ? w1t[(k0 + j) * H + hid] : 0.0f;
            bf16x8 hi, lo;
            split8(v, hi, lo);
            *reinterpret_cast<bf16x8*>(smem + G::W1H + i * 16) = hi;
            *reinterpret_cast<bf16x8*>(smem + G::W1L + i * 16) = lo;
        }
        for (int i = tid; i < G::W2_SLOTS; i += WT_BLOCK) {                  // W2: slot (((w * 2 + s2) * NT + t) * 64 + lane)
            const int g = i >> 6, t2 = g % NT, s2 = (g / NT) & 1, w = g / (2 * NT), hh = (i >> 5) & 1, rr = i & 31;
            const int o = 32 * t2 + rr;
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int hid = 32 * w + acc_row(8 * s2 + j, hh);          // (ACCUMULATOR LAYOUT, mfma_split.hpp)
                v[j] = (hid < H && o < F) ? w2t[hid * F + o] : 0.0f;
            }
            bf16x8 hi, lo;
            split8(v, hi, lo);
            *reinterpret_cast<bf16x8*>(smem + G::W2H + i * 16) = hi;
            *reinterpret_cast<bf16x8*>(smem + G::W2L + i * 16) = lo;
        }
    };
    mlp_wave_tiles<G>(X, n, b1, b2, Y, nact, stage);
}

template <int L>
static int launch_mlp_rows_l(const float* x, int64_t n, const tpnet_mlp* mlp, float* y, hipStream_t s) {
    static LdsOptIn lds;                               // L = 2: 72 576 bytes of dynamic LDS need the opt-in
    const void* k = reinterpret_cast<const void*>(k_mlp_rows_x3<L>);
    if (!lds.granted({k}, MlpRowsGeo<L>::BYTES)) return TPNET_ERR_BAD_ARG;
    // grid rule: as many waves per workgroup take tiles as one round over R_GRID workgroups needs (mlp_x3.hip's rule, two
    // workgroups per CU); from R_GRID * WT_WAVES * 32 = 131 072 rows on, a wave walks more than one tile
    const int64_t tiles = (n + 31) / 32;
    int64_t nact = (tiles + R_GRID - 1) / R_GRID;
    nact = nact > WT_WAVES ? WT_WAVES : nact;
    int64_t grid = (tiles + nact - 1) / nact;
    grid = grid > R_GRID ? R_GRID : grid;
    hipLaunchKernelGGL(k_mlp_rows_x3<L>, dim3((unsigned)grid), dim3(WT_BLOCK), MlpRowsGeo<L>::BYTES, s, x, n, mlp->w1t, mlp->b1,
                       mlp->w2t, mlp->b2, y, (int)nact);
    if (hipGetLastError() != hipSuccess) {             // (a runtime that refuses the launch: the callers fall back for good)
        lds.refused();
        return TPNET_ERR_BAD_ARG;
    }
    return TPNET_OK;
}

}  // namespace tpnet

using namespace tpnet;

extern "C" int tpnet_mlp_rows_supported(int32_t F, int32_t H) {
    return (F == MlpRowsGeo<1>::F && H == MlpRowsGeo<1>::H) || (F == MlpRowsGeo<2>::F && H == MlpRowsGeo<2>::H);
}

extern "C" int tpnet_mlp_rows_f32(const float* x, int64_t n, const tpnet_mlp* mlp, float* y, void* stream) {
    if (n < 0 || !mlp || (n > 0 && (!x || !y))) return TPNET_ERR_BAD_ARG;
    if (n == 0) return TPNET_OK;
    if (!tpnet_mlp_rows_supported(mlp->F, mlp->H) || !mlp->w1t || !mlp->b1 || !mlp->w2t || !mlp->b2) return TPNET_ERR_BAD_ARG;
    if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 15) return TPNET_ERR_BAD_ARG;
    return mlp->F == MlpRowsGeo<1>::F ? launch_mlp_rows_l<1>(x, n, mlp, y, (hipStream_t)stream)
                                      : launch_mlp_rows_l<2>(x, n, mlp, y, (hipStream_t)stream);
}
