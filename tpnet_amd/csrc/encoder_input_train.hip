// The encoder's input stage (models/TPNet.py:297-330) in a TRAINING step on the matrix cores: one launch forward, two backward.  Per
// row, with x the row's concat [node | time | edge | f1 | f2] built from the sources (encoder_input.hpp) and never written:
//   k_encoder_input_train  the forward: k_encoder_input (dense2.hpp's two layers) with an activation that, besides the ReLU, stores
//                          one bit per (row, hidden unit) -- a + b1 > 0 exactly as this launch decided it -- into relu_bits
//                          [n][ceil(H / 32)] uint32.  out has the bits of k_encoder_input's.
//   the backward from gy   a  = W1 . x + b1        h  = m ? a : 0          (m the saved bits)
//                          gb2 = sum gy            gw2 = sum gy (x) h
//                          gh = W2^T . gy          ga = m ? gh : 0         gb1 = sum ga       gw1 = sum ga (x) x
//                          gxt = W1[:, time]^T . ga                        gxf = W1[:, f1 | f2]^T . ga
//                          arg = tw lt + tb        gtw = sum gxt (-sin arg) lt                gtb = sum gxt (-sin arg)
//                          gfeat[row] = gxf[:F]    gfeat[n + row] = gxf[F:]                   (every sum over the rows)
//                          The backward is the gradient of the forward that ran: the ReLU's decisions are read, not recomputed
//                          (mlp_rows_bwd.hip recomputes the pre-activations in exact f32 for that; at Din = 572 that pass would be
//                          ~8 G vector FMAs per call).  Only G = Dt + 2 F columns of W1^T are multiplied: the raw tables take no gradient.
// THE BACKWARD'S TWO LAUNCHES are dense2_bwd.hpp's (the transposed workspace of the call, the image of W1, W2^T and the G columns
// of W1^T, the row-tile body, the padding rules):
//   k_eib_rows     first parks x, gy and the row's lt -- every lane the columns of x it is layer 1's B operand for, so that the passes
//                  read x back and hold no gather and no cosf.  Then dense2_bwd_rows with the parked x and gy as the two row
//                  sources and the rule of the saved bits; y is gx of the G columns.  The epilogue stores gxf into gfeat (may be
//                  NULL) and parks gxt, which a loop behind the accumulators turns into d = gxt (-sin arg) in place.
//   k_eib_weights  the contraction over rows.  A wave owns a 32-unit hidden slice of ONE product and up to 8 column tiles of it --
//                  gw1[slice, 256 columns of Din] = sum_rows ga^T x, or gw2[:, slice]^T = sum_rows h^T gy -- and a workgroup one part
//                  of the row tiles; gb1 is the sum of the ga operands a wave of gw1's first column group loads.  The last workgroup of
//                  a row part adds gb2, gtw and gtb in plain fp32, thread = column, rows in order.  Every row part writes ONE partial
//                  (gw1 | gb1 | gw2 | gb2 | gtw | gtb, unpadded); the caller adds the partials in a fixed order.  No atomics but the
//                  error word's: two calls give equal bits.
// x IS PARKED, not gathered again by the contraction: its B operand wants 8 consecutive ROWS of one column per lane, which from the
// sources is 8 gathers of one float (and a cosf each in the time columns).  The workspace is 128 (2 ceil(H / 32) + ceil(Din / 32) +
// ceil(Dout / 32) + ceil(Dt / 32)) + 4 bytes per row for the time of the backward (profiles/encoder_input_training.md).
// ARITHMETIC.  All products are the fp32 class of mfma_split.hpp; sinf, the masks and the column sums are plain fp32.
// PADDING.  dense2_bwd.hpp's rules: the row sources return zeros for a row >= n, d and lt of such a row are never read by the column
// sums, a hidden unit of the padding has bit 0, and an accumulator column of the padding is never written to gfeat.
#include "encoder_input.hpp"
#include "dense2_bwd.hpp"
#include "rows_contract.hpp"

namespace tpnet {

// (the forward's activation, act_relu_bits, and the backward's rule, rule_relu_bits: dense2_bwd.hpp -- mlp_l4.hip shares them)

// HG hidden slices per pass, OSM output tiles, MULTI: dense2_rows'
template <int HG, int OSM, bool MULTI>
__global__ __launch_bounds__(D2_T) void k_encoder_input_train(const ei_src src, const ei_dims d, const uint4* __restrict__ img,
                                                              float* __restrict__ out, uint32_t* __restrict__ relu_bits,
                                                              uint32_t* __restrict__ err) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31;
    const int64_t row = ((int64_t)blockIdx.x * 4 + wave) * 32 + r;
    ei_row x4;
    x4.init(src, d, row, err);
    const int NW = (d.l.H + 31) / 32;
    act_relu_bits act;
    act.NW = x4.valid ? NW : 0;
    act.words = relu_bits + (x4.valid ? row : 0) * NW;
    float* yo = out + row * d.l.Dout;
    dense2_rows<HG, OSM, MULTI, act_relu_bits>(d.l, img, x4.valid, x4,
                                               [&](int o, const float4 v) { *reinterpret_cast<float4*>(yo + o) = v; }, act);
}

// ---- the backward's sizes: dense2_bwd.hpp's with the G = Dt + 2 F columns of x that take a gradient (the time columns from Dn, the
// relative encodings from Dn + Dt + De).  It serves the forward's sizes with G <= 256 (8 output tiles of the row-tile kernel)
static constexpr int EIB_WT = 8;                 // accumulator tiles of a weight wave: 256 columns
static bool eib_make_dims(const int32_t* v, ei_dims& e, d2b_dims& o) {
    if (!ei_make_dims(v, e) || e.Dt + 2 * e.F > 32 * D2_OS_WIDE) return false;
    d2b_make_dims(e.l.Din, e.l.H, e.l.Dout, e.Dt, e.Dn, 2 * e.F, e.Dn + e.Dt + e.De, o);
    return true;
}
static int64_t eib_partial_floats(const d2b_dims& d) {
    return (int64_t)d.H * d.Din + d.H + (int64_t)d.Dout * d.H + d.Dout + 2 * (int64_t)d.Gt;
}

// ---- the backward's workspace: dense2_bwd.hpp's head (hT, gaT), three transposed column arrays, tile by tile, and the rows' lt
struct eib_ws : d2b_ws {
    int CSI, CSO, CST;                           // parked columns of x, of gy and time columns per tile (multiples of 32)
    float *xT, *gyT, *dT, *lt;                   // xT [T][CSI][32]; gyT [T][CSO][32]; dT [T][CST][32]; lt [T][32]
};
static int64_t eib_ws_floats(int64_t n, const d2b_dims& d) {
    return d2b_tiles(n) * 32 * (2 * (int64_t)d2b_pad32(d.H) + d2b_pad32(d.Din) + d2b_pad32(d.Dout) + d2b_pad32(d.Gt) + 1);
}
static eib_ws eib_make_ws(float* base, int64_t n, const d2b_dims& d) {
    eib_ws w;
    w.xT = d2b_make_ws(w, base, n, d.H);
    w.CSI = d2b_pad32(d.Din);
    w.CSO = d2b_pad32(d.Dout);
    w.CST = d2b_pad32(d.Gt);
    w.gyT = w.xT + w.T * w.CSI * 32;
    w.dT = w.gyT + w.T * w.CSO * 32;
    w.lt = w.dT + w.T * w.CST * 32;
    return w;
}

// ---- the backward's row-tile kernel: dense2_bwd_rows on the parked x and gy, gfeat and the time encoder's d behind it
template <int OSM>
__global__ __launch_bounds__(D2_T) void k_eib_rows(const ei_src src, const ei_dims ed, const d2b_dims d, const float* __restrict__ gy,
                                                   const uint32_t* __restrict__ relu_bits, const uint4* __restrict__ img, const eib_ws ws,
                                                   float* __restrict__ gfeat, int time_grads, uint32_t* __restrict__ err) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int64_t tile = (int64_t)blockIdx.x * 4 + wave;
    const int64_t row = tile * 32 + r;
    ei_row x4;
    x4.init(src, ed, row, err);
    const bool valid = x4.valid, park = tile < ws.T;
    const int Dout = d.Dout;
    const float* gr = gy + (valid ? row : 0) * Dout;
    rule_relu_bits rule;
    rule.NW = valid ? ws.NS : 0;
    rule.words = relu_bits + (valid ? row : 0) * ws.NS;
    // columns c .. c + 3 of gy
    auto g4 = [&](int c) -> float4 {
        if (!valid || c >= Dout) return make_float4(0.f, 0.f, 0.f, 0.f);
        return *reinterpret_cast<const float4*>(gr + c);
    };
    // ---- x and gy of the tile, parked before the accumulators are live.  A lane parks the columns 16 s + 8 h + (0..7) of its row: the
    // ones it is layer 1's B operand for, so the k-steps read x back (the lane's own stores) and hold no gather and no cosf
    float* xT = ws.xT + (park ? tile : 0) * ws.CSI * 32 + r;
    if (park) {
        float* gyT = ws.gyT + tile * ws.CSO * 32 + r;
        for (int c = 8 * h; c < ws.CSI; c += 16) {
            const float4 a = x4(c), b = x4(c + 4);                              // (a row >= n, a column >= Din: selected zeros)
            xT[c * 32] = a.x; xT[(c + 1) * 32] = a.y; xT[(c + 2) * 32] = a.z; xT[(c + 3) * 32] = a.w;
            xT[(c + 4) * 32] = b.x; xT[(c + 5) * 32] = b.y; xT[(c + 6) * 32] = b.z; xT[(c + 7) * 32] = b.w;
        }
        for (int c = 4 * h; c < ws.CSO; c += 8) {
            const float4 a = g4(c);
            gyT[c * 32] = a.x; gyT[(c + 1) * 32] = a.y; gyT[(c + 2) * 32] = a.z; gyT[(c + 3) * 32] = a.w;
        }
        if (h == 0) ws.lt[tile * 32 + r] = x4.lt;                               // (0 for a row >= n)
    }
    // columns c .. c + 3 of the row's parked x
    auto xp4 = [&](int c) -> float4 {
        if (!valid || c >= ws.CSI) return make_float4(0.f, 0.f, 0.f, 0.f);
        return make_float4(xT[c * 32], xT[(c + 1) * 32], xT[(c + 2) * 32], xT[(c + 3) * 32]);
    };
    dense2_bwd_rows<OSM, true>(d, img, ws, valid, xp4, g4, rule, [&](const f32x16 (&y)[OSM]) {
        // ---- y = gx of the G columns of row r: time columns first, then f1, then f2
        if (!valid) return;
        float* dT = ws.dT + tile * ws.CST * 32 + r;
        const int Dt = d.Gt, F = ed.F;
#pragma unroll
        for (int t = 0; t < OSM; ++t) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int o = 32 * t + 8 * i + 4 * h;
                if (o < Dt) {
                    if (time_grads) {
                        dT[o * 32] = y[t][4 * i];
                        dT[(o + 1) * 32] = y[t][4 * i + 1];
                        dT[(o + 2) * 32] = y[t][4 * i + 2];
                        dT[(o + 3) * 32] = y[t][4 * i + 3];
                    }
                } else if (o < d.G && gfeat) {
                    float* gf = o < Dt + F ? gfeat + row * F + (o - Dt) : gfeat + (src.n + row) * F + (o - Dt - F);
                    *reinterpret_cast<float4*>(gf) = make_float4(y[t][4 * i], y[t][4 * i + 1], y[t][4 * i + 2], y[t][4 * i + 3]);
                }
            }
        }
        // ---- d = gxt (-sin arg) in place, behind the accumulators (128 inlined sinf among them spilt): the lane's own stores, the
        // time columns 8 j + 4 h + (0..3)
        if (!time_grads) return;
#pragma unroll 1
        for (int o = 4 * h; o < Dt; o += 8) {
            const float4 a = x4.arg4(o);
            dT[o * 32] *= -sinf(a.x);
            dT[(o + 1) * 32] *= -sinf(a.y);
            dT[(o + 2) * 32] *= -sinf(a.z);
            dT[(o + 3) * 32] *= -sinf(a.w);
        }
    });
}

// grid (ceil(NS (NG + 1) / 4) + 1, row parts), NG = column groups of gw1.  tpp: tiles per row part (every part holds one)
__global__ __launch_bounds__(256) void k_eib_weights(const eib_ws ws, int64_t n, const d2b_dims d, int64_t tpp, int time_grads,
                                                     float* __restrict__ partial) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int64_t t0 = (int64_t)blockIdx.y * tpp, t1 = t0 + tpp < ws.T ? t0 + tpp : ws.T;
    const int Din = d.Din, H = d.H, Dout = d.Dout, Dt = d.Gt;
    float* gw1 = partial + (int64_t)blockIdx.y * ((int64_t)H * Din + H + (int64_t)Dout * H + Dout + 2 * (int64_t)Dt);
    float* gb1 = gw1 + (int64_t)H * Din;
    float* gw2 = gb1 + H;
    float* gb2 = gw2 + (int64_t)Dout * H;
    float* gtw = gb2 + Dout;
    float* gtb = gtw + Dt;
    if (blockIdx.x == gridDim.x - 1) {
        // ---- the three sums over rows that are no matrix product: thread = column, rows in order, rows >= n never added
        for (int c = tid; c < Dout; c += 256) {
            float so = 0.0f;
            for (int64_t t = t0; t < t1; ++t) {
                const int nr = d2b_tile_rows(n, t);
                const float* go = ws.gyT + (t * ws.CSO + c) * 32;
                for (int i = 0; i < nr; ++i) so += go[i];
            }
            gb2[c] = so;
        }
        for (int c = tid; c < Dt; c += 256) {
            float sw = 0.0f, sb = 0.0f;
            if (time_grads) {
                for (int64_t t = t0; t < t1; ++t) {
                    const int nr = d2b_tile_rows(n, t);
                    const float* dd = ws.dT + (t * ws.CST + c) * 32;
                    const float* lt = ws.lt + t * 32;
                    for (int i = 0; i < nr; ++i) {
                        sw += dd[i] * lt[i];
                        sb += dd[i];
                    }
                }
            }
            gtw[c] = sw;                                                        // (a frozen time encoder: zeros)
            gtb[c] = sb;
        }
        return;
    }
    const int nti = ws.CSI / 32, NG = (nti + EIB_WT - 1) / EIB_WT;
    const int item = 4 * blockIdx.x + wave;                                     // (no barrier in this kernel)
    f32x16 acc[EIB_WT];
#pragma unroll
    for (int t = 0; t < EIB_WT; ++t)
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[t][q] = 0.0f;
    if (item < ws.NS * NG) {
        // gw1[slice, columns 256 grp ..] = sum_rows ga^T x
        const int slice = item / NG, grp = item % NG;
        const int ct0 = EIB_WT * grp, nt = nti - ct0 < EIB_WT ? nti - ct0 : EIB_WT;
        float asum = rc_walk(ws.gaT, ws.CHS, slice, ws.xT, ws.CSI, ct0, nt, t0, t1, r, h, acc);
#pragma unroll
        for (int tt = 0; tt < EIB_WT; ++tt) {
            const int c = 32 * (ct0 + tt) + r;
            if (tt < nt && c < Din) {
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    const int j = 32 * slice + acc_row(q, h);
                    if (j < H) gw1[(int64_t)j * Din + c] = acc[tt][q];
                }
            }
        }
        asum += __shfl_xor(asum, 32);
        if (grp == 0 && h == 0 && 32 * slice + r < H) gb1[32 * slice + r] = asum;
    } else if (item < ws.NS * (NG + 1)) {
        // gw2[:, slice]^T = sum_rows h^T gy
        const int slice = item - ws.NS * NG;
        rc_walk(ws.hT, ws.CHS, slice, ws.gyT, ws.CSO, 0, ws.CSO / 32, t0, t1, r, h, acc);
#pragma unroll
        for (int tt = 0; tt < EIB_WT; ++tt) {
            const int c = 32 * tt + r;
            if (tt < ws.CSO / 32 && c < Dout) {
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    const int j = 32 * slice + acc_row(q, h);
                    if (j < H) gw2[(int64_t)c * H + j] = acc[tt][q];
                }
            }
        }
    }
}

template <int HG, int OSM, bool MULTI>
static void ei_launch_train(const ei_src& s, const ei_dims& d, const void* img, float* out, uint32_t* bits, uint32_t* err, hipStream_t st) {
    hipLaunchKernelGGL((k_encoder_input_train<HG, OSM, MULTI>), dim3((unsigned)((s.n + D2_ROWS - 1) / D2_ROWS)), dim3(D2_T), 0, st, s, d,
                       reinterpret_cast<const uint4*>(img), out, bits, err);
}

}  // namespace tpnet

using namespace tpnet;

extern "C" int tpnet_encoder_input_train(const float* node_raw, int64_t n_node_rows, const float* edge_raw, int64_t n_edge_rows,
                                         const int64_t* neigh, const int64_t* eid, const double* tn, const double* tq, const float* tw,
                                         const float* tb, const float* feat, int64_t n_nodes, int32_t K, const int32_t* dims,
                                         const void* img, float* out, uint32_t* relu_bits, uint32_t* err, void* stream) {
    ei_dims d;
    ei_src s{node_raw, edge_raw, tw, tb, feat, neigh, eid, tn, tq, n_node_rows, n_edge_rows, 0, K};
    if (!ei_src_ok(s, n_nodes) || !img || !out || !relu_bits || !err || !ei_make_dims(dims, d)) return TPNET_ERR_BAD_ARG;
    if (!aligned16({img, out}) || (reinterpret_cast<uintptr_t>(relu_bits) & 3)) return TPNET_ERR_BAD_ARG;
    s.n = n_nodes * K;
    if (s.n == 0) return TPNET_OK;
    if (d.l.HG == D2_HG) ei_launch_train<D2_HG, D2_OS, false>(s, d, img, out, relu_bits, err, (hipStream_t)stream);
    else ei_launch_train<D2_HG_WIDE, D2_OS_WIDE, true>(s, d, img, out, relu_bits, err, (hipStream_t)stream);
    TPNET_HIP_TRY(hipGetLastError());
    return TPNET_OK;
}

extern "C" size_t tpnet_encoder_input_bwd_image_bytes(int32_t Dn, int32_t Dt, int32_t De, int32_t F, int32_t H, int32_t Dout) {
    const int32_t v[6] = {Dn, Dt, De, F, H, Dout};
    ei_dims e;
    d2b_dims b;
    return eib_make_dims(v, e, b) ? d2b_image_bytes(b) : 0;
}

extern "C" int64_t tpnet_encoder_input_bwd_partial_floats(int32_t Dn, int32_t Dt, int32_t De, int32_t F, int32_t H, int32_t Dout) {
    const int32_t v[6] = {Dn, Dt, De, F, H, Dout};
    ei_dims e;
    d2b_dims b;
    return eib_make_dims(v, e, b) ? eib_partial_floats(b) : 0;
}

extern "C" size_t tpnet_encoder_input_bwd_workspace_bytes(int64_t n_rows, int32_t Dn, int32_t Dt, int32_t De, int32_t F, int32_t H,
                                                          int32_t Dout) {
    const int32_t v[6] = {Dn, Dt, De, F, H, Dout};
    ei_dims e;
    d2b_dims b;
    if (n_rows < 0 || n_rows > (1ll << 31) || !eib_make_dims(v, e, b)) return 0;
    return (size_t)eib_ws_floats(n_rows, b) * sizeof(float);
}

extern "C" int tpnet_encoder_input_bwd_prepare(const float* w1, const float* b1, const float* w2, const int32_t* dims, void* bimg,
                                               void* stream) {
    ei_dims e;
    d2b_dims b;
    if (!w1 || !b1 || !w2 || !bimg || (reinterpret_cast<uintptr_t>(bimg) & 15) || !eib_make_dims(dims, e, b)) return TPNET_ERR_BAD_ARG;
    TPNET_HIP_TRY(d2b_prepare(w1, b1, w2, b, bimg, (hipStream_t)stream));
    return TPNET_OK;
}

extern "C" int tpnet_encoder_input_bwd(const float* node_raw, int64_t n_node_rows, const float* edge_raw, int64_t n_edge_rows,
                                       const int64_t* neigh, const int64_t* eid, const double* tn, const double* tq, const float* tw,
                                       const float* tb, const float* feat, const uint32_t* relu_bits, const float* gy, int64_t n_nodes,
                                       int32_t K, const int32_t* dims, const void* bimg, void* workspace, float* gfeat,
                                       int32_t time_grads, float* partial, int32_t n_partial, uint32_t* err, void* stream) {
    ei_dims e;
    d2b_dims b;
    ei_src s{node_raw, edge_raw, tw, tb, feat, neigh, eid, tn, tq, n_node_rows, n_edge_rows, 0, K};
    if (!ei_src_ok(s, n_nodes) || !relu_bits || !gy || !bimg || !workspace || !partial || !err) return TPNET_ERR_BAD_ARG;
    if (!eib_make_dims(dims, e, b) || n_partial < 1 || gfeat == feat || gfeat == gy) return TPNET_ERR_BAD_ARG;
    if (!aligned16({gy, bimg, workspace, gfeat}) || ((reinterpret_cast<uintptr_t>(relu_bits) | reinterpret_cast<uintptr_t>(partial)) & 3))
        return TPNET_ERR_BAD_ARG;
    s.n = n_nodes * K;
    if (s.n == 0) return 0;
    const hipStream_t st = (hipStream_t)stream;
    const eib_ws ws = eib_make_ws(static_cast<float*>(workspace), s.n, b);
    D2B_LAUNCH_ROWS(k_eib_rows, b, s.n, st, s, e, b, gy, relu_bits, reinterpret_cast<const uint4*>(bimg), ws, gfeat, (int)(time_grads != 0),
                    err);
    int64_t tpp;
    const int parts = d2b_row_parts(ws.T, n_partial, tpp);
    const int items = ws.NS * ((ws.CSI / 32 + EIB_WT - 1) / EIB_WT + 1);
    hipLaunchKernelGGL(k_eib_weights, dim3((unsigned)((items + 3) / 4 + 1), (unsigned)parts), dim3(256), 0, st, ws, s.n, b, tpp,
                       (int)(time_grads != 0), partial);
    TPNET_HIP_TRY(hipGetLastError());
    return parts;
}
