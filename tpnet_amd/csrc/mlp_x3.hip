// self.mlp = Linear(64,256) -> ReLU -> Linear(256,64) (models/TPNet.py:63-65,129) on rows of features that already exist ([n][64]
// f32: the encoder's call, models/TPNet.py:311-324 -- 4*B*K rows per call), fp32 class, for LONG lists.
// Same arithmetic as MODE 2 of feature_mfma.hip (two-piece operands, three products per term on v_mfma_f32_32x32x16_bf16, fp32
// accumulators: mfma_split.hpp), other mapping: there a 32-row tile is spread over the 8
// waves of a workgroup (one hidden slice each, weights in registers) and costs three workgroup barriers and an 8-way partial-sum
// exchange through LDS per tile -- ~3 us per tile of which 0.3 us is matrix work.  Here every WAVE owns whole 32-row tiles: it
// walks the 8 hidden slices itself, layer 2's accumulators never leave its registers, and the split weights (128 KB: W1 and W2,
// hi and lo, in exactly the per-lane operand order) live in the CU's LDS (160 KB on gfx950), staged once per workgroup.  No
// barrier after the staging; 192 matrix instructions per tile and wave against 128 ds_read_b128 (lanes consecutive: conflict-free).
// The hidden slices are summed inside the accumulator (slice 0..7 in order) instead of the other kernel's fixed tree: the two
// kernels differ in the last bits, both within the fp32-class bound (<= 2e-5 of the output scale against the torch layers).
// Measured: 80 000 rows 32.5 -> 23 us, 800 000 rows 224 -> 150 us (load + split + store alone: 12 / 97 us; matrix pipe busy 4.8 M x
// 32 cycles per launch = 42 % of a 2.4 GHz clock).  Not kept: twelve waves per workgroup (157 us); slice w + 1's layer-1 products
// issued ahead of slice w's vector work, with and without sched_group_barrier interleaving (162 us: more registers, no overlap won).
// Nor: the weights of a step read from LDS one step ahead of their products behind scheduling barriers (164 us); one LDS block per
// slice (every read base + 16-bit offset), the accumulators started from the bias and a one-instruction ReLU -- 130 vector instructions
// per two slices instead of 225 -- at 153 us: neither the LDS round trips nor the vector work is what the launch waits for.
// The tile walk, the geometry (MlpRowsGeo<3>: its LDS image is IMG_* of mfma_split.hpp) and the padding rules: mlp_wave_tile.hpp,
// shared with mlp_rows.hip's kernel for F = 16 and 36.
#include "tpnet_common.h"
#include "mlp_wave_tile.hpp"

namespace tpnet {

using X3 = MlpRowsGeo<3>;

// w1f = f32 [256][64] (mlp[0].weight as is); w2f = f32 [8 slices][2 output tiles][64 lanes][16] (tpnet_mlp::w2f, include/tpnet_hip.h)
__global__ __launch_bounds__(WT_BLOCK) void k_mlp64_x3(const float* __restrict__ X, int64_t n, const float* __restrict__ w1f,
                                                       const float* __restrict__ b1, const float* __restrict__ w2f,
                                                       const float* __restrict__ b2, float* __restrict__ Y, int nact) {
    // ---- the split weights -> LDS, every thread 4 + 4 pieces of 8 floats
    // (walked in the order of the LDS image: consecutive lanes write consecutive 16-byte slots -- in the sources' own order eight
    // consecutive lanes hit one bank, 4 096 conflict cycles per workgroup -- and read 32-byte pieces 256 / 64 bytes apart)
    auto stage = [&](char* smem, int tid) {
        for (int i = tid; i < X3::W1_SLOTS; i += WT_BLOCK) {                // W1: slot ((w * 4 + s) * 64 + lane (h, r))
            const int w = i >> 8, sx = (i >> 6) & 3, hh = (i >> 5) & 1, rr = i & 31;
            const float* p = w1f + ((w * 32 + rr) * X3::F + 16 * sx + 8 * hh);
            bf16x8 hi, lo;
            load_split8(p, hi, lo);
            *reinterpret_cast<bf16x8*>(smem + X3::W1H + i * 16) = hi;
            *reinterpret_cast<bf16x8*>(smem + X3::W1L + i * 16) = lo;
        }
        for (int i = tid; i < X3::W2_SLOTS; i += WT_BLOCK) {                // W2: slot (((w * 2 + s2) * 2 + t2) * 64 + lane)
            const int w = i >> 8, s2 = (i >> 7) & 1, t2 = (i >> 6) & 1, ln = i & 63;
            const float* p = w2f + ((((w * 2 + t2) * 64 + ln) * 16) + 8 * s2);
            bf16x8 hi, lo;
            load_split8(p, hi, lo);
            *reinterpret_cast<bf16x8*>(smem + X3::W2H + i * 16) = hi;
            *reinterpret_cast<bf16x8*>(smem + X3::W2L + i * 16) = lo;
        }
    };
    mlp_wave_tiles<X3>(X, n, b1, b2, Y, nact, stage);
}

static LdsOptIn mlp_x3_lds;                           // a workgroup's 132 KB of LDS

bool mlp_x3_available() {
    static const int off = TPNET_DEV_INT(NO_MLP_X3, 0);
    return mlp_x3_lds.granted({reinterpret_cast<const void*>(k_mlp64_x3)}, X3::BYTES, off != 0);
}

// rows from which the per-wave-tile kernel takes a list (below: feature_mfma.hip's kernel spreads the few tiles over more CUs)
int64_t mlp_x3_from() {
    static const int64_t from = (int64_t)TPNET_DEV_INT(MLP_X3_FROM, 8192);
    return from;
}

int launch_mlp_rows_x3(const float* x, int64_t n, const float* w1f, const float* b1, const float* w2f, const float* b2, float* y,
                       hipStream_t s) {
    if (n == 0) return TPNET_OK;
    if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(w1f) |
         reinterpret_cast<uintptr_t>(w2f)) & 15)
        return TPNET_ERR_BAD_ARG;
    if (!mlp_x3_available()) return TPNET_ERR_BAD_ARG;
    const int64_t tiles = (n + 31) / 32;
    int64_t nact = (tiles + 255) / 256;                // waves per workgroup that take tiles: a CU's share of one round
    nact = nact > WT_WAVES ? WT_WAVES : nact;
    static const int nact_dev = TPNET_DEV_INT(X3_WAVES, 0);
    if (nact_dev > 0 && nact_dev < nact) nact = nact_dev;
    int64_t grid = (tiles + nact - 1) / nact;
    grid = grid > 256 ? 256 : grid;
    hipLaunchKernelGGL(k_mlp64_x3, dim3((unsigned)grid), dim3(WT_BLOCK), X3::BYTES, s, x, n, w1f, b1, w2f, b2, y, (int)nact);
    if (hipGetLastError() != hipSuccess) {             // (a runtime that refuses the launch: the callers fall back for good)
        mlp_x3_lds.refused();
        return TPNET_ERR_BAD_ARG;
    }
    return TPNET_OK;
}

}  // namespace tpnet
