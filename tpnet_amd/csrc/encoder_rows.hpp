// The row fetch of the encoder's matrix-core readouts, once (encoder_mfma.hip: L = 3; encoder_layers.hip: L = 1, 2, 4): 16 rows in
// the LOAD layout (lane 4 r + p reads the 16-byte piece p of a 64-byte segment of row r, so every quad of lanes reads 64
// contiguous bytes) and their move to the OPERAND layout of v_mfma_f32_16x16x32_bf16 (lane (c = lane & 15, g = lane >> 4) holds
// row c, floats {32 s + 4 g .. + 3} and {32 s + 16 + 4 g .. + 3} of step s) through ds_bpermute_b32 (the LDS crossbar, no LDS
// memory).  Which node and layer a row is, the tiles and the scatter of the blocks stay with each kernel.
#pragma once
#include "mfma_split.hpp"

namespace tpnet {

// 16 rows of KS 32-deep steps, one row pointer per load-layout lane (already offset by the lane's 16-byte piece):
// raw[s][0..3] = floats 32 s + 4 p .., raw[s][4..7] = floats 32 s + 16 + 4 p ..
// FULL: a row is exactly 32 KS floats.  !FULL: a row is d floats, 32 (KS - 1) < d <= 32 KS, d % 4 == 0: a piece is loaded only if
// it lies inside the row (`left` = d - 4 p, the floats from the lane's first piece to the row's end) and is zero otherwise -- a
// zero k-position adds exactly 0 to every product, and what follows a row in memory (the next node's row) is never read.
// R8 (with !FULL): d % 4 == 2 -- a row starts at 0 or 8 mod 16 bytes, by the parity of its index, so a piece is only 8-byte
// aligned and is fetched as two 8-byte halves; d - 4 p is even, not a multiple of 4: a row ends with a HALF piece, and each half is
// loaded only if it lies inside the row (`left` compared in steps of 2 floats), zero otherwise -- the same guarantee as above.
template <int KS, bool FULL, bool R8 = false>
__device__ __forceinline__ void load_rows(const float* __restrict__ rp, int left, float (&raw)[KS][8]) {
    static_assert(!(FULL && R8), "load_rows: a full row is a row of whole 16-byte pieces");
    // R8: the second halves through a pointer the compiler cannot relate to `rp` -- where both halves of a piece are loaded
    // unconditionally it would otherwise fuse them into ONE 16-byte load of an address that is only 8-byte aligned
    // (the OFFSET is what is hidden: the pointer keeps its provenance, the loads stay global loads)
    int two = 2;
    if constexpr (R8) asm volatile("" : "+v"(two));
    const float* rp2 = rp + two;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
        if constexpr (R8) {
            float2 h[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {          // halves at floats 32 s + {0, 2, 16, 18} of the lane's pointer
                const int o = 32 * s + 16 * (k >> 1) + 2 * (k & 1);
                h[k] = make_float2(0.f, 0.f);
                // (d > 32 (KS - 1): every step but the last lies inside the row for every lane -- 4 lane masks to keep, not 4 KS)
                if (s + 1 < KS || o + 2 <= left) h[k] = *reinterpret_cast<const float2*>((k & 1) ? rp2 + (o - 2) : rp + o);
            }
            raw[s][0] = h[0].x; raw[s][1] = h[0].y; raw[s][2] = h[1].x; raw[s][3] = h[1].y;
            raw[s][4] = h[2].x; raw[s][5] = h[2].y; raw[s][6] = h[3].x; raw[s][7] = h[3].y;
        } else {
            float4 x = make_float4(0.f, 0.f, 0.f, 0.f), y = x;
            if (FULL || 32 * s + 4 <= left) x = *reinterpret_cast<const float4*>(rp + 32 * s);
            if (FULL || 32 * s + 20 <= left) y = *reinterpret_cast<const float4*>(rp + 32 * s + 16);
            raw[s][0] = x.x; raw[s][1] = x.y; raw[s][2] = x.z; raw[s][3] = x.w;
            raw[s][4] = y.x; raw[s][5] = y.y; raw[s][6] = y.z; raw[s][7] = y.w;
        }
    }
}

// load layout -> operand layout (lane (c, g) takes what lane 4 c + g loaded); SCALE: the row's pending decay applied on the way
template <int KS, bool SCALE = true>
__device__ __forceinline__ void to_lanes(const float (&raw)[KS][8], float rs, int pull, float (&v)[KS][8]) {
#pragma unroll
    for (int s = 0; s < KS; ++s)
#pragma unroll
        for (int k = 0; k < 8; ++k)
            v[s][k] = __int_as_float(__builtin_amdgcn_ds_bpermute(pull, __float_as_int(SCALE ? raw[s][k] * rs : raw[s][k])));
}
// ... and the split on top
template <int KS, int SPLIT>
__device__ __forceinline__ void to_operands(const float (&raw)[KS][8], float rs, int pull, SplitOp<SPLIT> (&op)[KS]) {
    float v[KS][8];
    to_lanes<KS>(raw, rs, pull, v);
#pragma unroll
    for (int s = 0; s < KS; ++s) split8(v[s], op[s]);
}

// ---- host side: what the launchers of both files ask of a row width and a tile count ---------------------------------------
// rows of 2..5 steps of 32 floats (d % 4 == 0: 36..160; d % 4 == 2, 8-byte rows: 38..158)
inline bool encoder_row_width(int d) { return d >= 36 && d <= 160; }
inline int encoder_steps(int d) { return (d + 31) / 32; }      // KS: 32-deep steps of a row of d floats

// LAUNCH(KS, FULL, R8) for the instantiation that serves such a row: d = 64 / 128 in whole steps, every other d % 4 == 0 with the
// last step masked, d % 4 == 2 the same in 8-byte halves
#define TPNET_ENCODER_STEP_SWITCH(D_, LAUNCH, R8_) \
    switch (tpnet::encoder_steps(D_)) {            \
        case 2: LAUNCH(2, false, R8_); break;      \
        case 3: LAUNCH(3, false, R8_); break;      \
        case 4: LAUNCH(4, false, R8_); break;      \
        default: LAUNCH(5, false, R8_); break;     \
    }
#define TPNET_ENCODER_WIDTH_SWITCH(D_, LAUNCH)                              \
    do {                                                                    \
        if ((D_) == 128) LAUNCH(4, true, false);                            \
        else if ((D_) == 64) LAUNCH(2, true, false);                        \
        else if ((D_) % 4 == 0) TPNET_ENCODER_STEP_SWITCH(D_, LAUNCH, false) \
        else TPNET_ENCODER_STEP_SWITCH(D_, LAUNCH, true)                    \
    } while (0)

// tiles per wave for ONE round of the `waves` waves the chip holds, at least two tiles each; the grid of blocks of `per_block` of them
struct TileRound { int tpw, grid; };
inline TileRound tile_round(int ntiles, int waves, int per_block) {
    int tpw = (ntiles + waves - 1) / waves;
    if (tpw < 2) tpw = 2;
    const int nwaves = (ntiles + tpw - 1) / tpw;
    return {tpw, (nwaves + per_block - 1) / per_block};
}

}  // namespace tpnet
