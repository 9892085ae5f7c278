// gfx950 kernel of the one-vs-many readout: tpnet_pair_gram_fanout.  Row i of the call has ONE source and C candidate
// destinations; out[i * C + c] = G(src[i], cand[i * C + c]) with the source's layers first -- tpnet_pair_gram(repeat(src, C), cand)
// (models/modules.py:112, models/TPNet.py:112-128 before self.mlp) with the source's rows fetched, decayed and reduced once per unit.
#include "readout.hpp"

namespace tpnet {

static constexpr int FB = BLOCK_SMALL;   // threads per workgroup

// unit = (row, chunk of KC candidates), cut as the anchored walk cuts its rows (anchored_chunk): a long list of rows takes KC = C
// (the source fetched once per row); few rows are cut into chunks so that the launch still fills the chip
template <int LPP, int VPL, int W, int L, bool FULL>
__global__ __launch_bounds__(FB) void k_pair_gram_fanout(tpnet_state S, const int64_t* __restrict__ src,
                                                         const int64_t* __restrict__ cand, int64_t n_rows, int C, int KC,
                                                         double now, double lambda, uint32_t flags, float* __restrict__ out) {
    constexpr int GPB = FB / LPP;
    constexpr int NG = GramCfg<LPP, L>::NG;
    const int gl = threadIdx.x % LPP;
    const int g = threadIdx.x / LPP;
    const bool do_scale = !(flags & TPNET_FLAG_NOT_SCALE);
    const int nch = (C + KC - 1) / KC;
    const int64_t units = n_rows * nch;
    if constexpr (W == 4 && LPP >= 16) {       // one chunk of 16-byte vectors per row; !FULL: the chunk's tail lanes hold zeros
        for (int64_t base = (int64_t)blockIdx.x * GPB; base < units; base += (int64_t)gridDim.x * GPB) {
            const int64_t un = base + g;
            const bool valid = un < units;
            const int64_t rr = valid ? un / nch : 0;
            const int ch = valid ? (int)(un - rr * nch) : 0;
            const int kb = ch * KC, ke = (kb + KC < C) ? kb + KC : C;
            gram_fanout<LPP, VPL, W, L, FULL>(S, cand + rr * C, valid ? src[rr] : 0, kb, ke, valid, now, lambda, do_scale,
                                              out + rr * C * NG, gl);
        }
    }
}

// the anchored walk's geometry class: rows of whole 16-byte vectors inside ONE chunk of a geometry of >= 16 lanes
bool pair_gram_fanout_supported(const tpnet_state& st) { return pair_gram_anchored_supported(st); }

int launch_pair_gram_fanout(const tpnet_state& st, const int64_t* src, const int64_t* cand, int64_t n_rows, int C, double now,
                            double lambda, uint32_t flags, float* out, hipStream_t s) {
    if (n_rows == 0) return TPNET_OK;
    if (!pair_gram_fanout_supported(st)) return TPNET_ERR_BAD_ARG;
    TPNET_DISPATCH(({
        if constexpr (W == 4 && LPP >= 16) {
            const int kc = anchored_chunk(n_rows, C);
            const int64_t units = n_rows * ((C + kc - 1) / kc);
            const int grid = grid_for(units, FB / LPP, 256 * 16);
            hipLaunchKernelGGL((k_pair_gram_fanout<LPP, VPL, W, L, FULL>), dim3(grid), dim3(FB), 0, s, st, src, cand, n_rows, C,
                               kc, now, lambda, flags, out);
        } else {
            return TPNET_ERR_BAD_ARG;
        }
    }));
    TPNET_HIP_TRY(hipGetLastError());
    return TPNET_OK;
}

}  // namespace tpnet
