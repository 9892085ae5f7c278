// What the input-stage kernels share (encoder_input.hip: the forward; encoder_input_train.hip: the forward that records the ReLU
// decisions and the backward): the served sizes and the row source -- the gathered concat of a lane's row, never written.  One copy.
#pragma once
#include "dense2.hpp"

namespace tpnet {

struct ei_dims {
    int Dn, Dt, De, F;                           // the segments of a row: node | time | edge | two halves of F relative encodings
    d2_dims l;                                   // the layers: Din = Dn + Dt + De + 2 F, H, Dout and the variant
};

static inline bool ei_make_dims(const int32_t* d, ei_dims& o) {
    if (!d) return false;
    o.Dn = d[0]; o.Dt = d[1]; o.De = d[2]; o.F = d[3];
    const int H = d[4], Dout = d[5];
    if (o.Dn < 4 || o.Dt < 4 || o.De < 4 || o.F < 4 || H < 1 || Dout < 4) return false;
    if ((o.Dn | o.Dt | o.De | o.F | Dout) & 3) return false;
    if (o.Dn > 1024 || o.Dt > 1024 || o.De > 1024 || o.F > 512 || H > 512 || Dout > 256) return false;
    const int Din = o.Dn + o.Dt + o.De + 2 * o.F;
    if (Din > 1024) return false;
    d2_make_dims(Din, H, Dout, false, o.l);
    return true;
}

// the arrays a row is built from (tpnet_encoder_input's arguments)
struct ei_src {
    const float *node_raw, *edge_raw, *tw, *tb, *feat;
    const int64_t *neigh, *eid;
    const double *tn, *tq;
    int64_t n_node_rows, n_edge_rows, n;         // n = n_nodes * K rows
    int K;
};

// This lane's row: the four sources and the scaled time delta (f64 difference -> f32 -> log(x + 1), TPNet.py:299-301).  An id
// outside its table reads row 0 and sets err[0]; a row >= n reads nothing.
struct ei_row {
    const float *nrow, *erow, *f1, *f2, *tw, *tb;
    float lt;
    int e0, e1, e2, e3, e4;
    bool valid;
    __device__ __forceinline__ void init(const ei_src& s, const ei_dims& d, int64_t row, uint32_t* __restrict__ err) {
        valid = row < s.n;
        nrow = s.node_raw; erow = s.edge_raw; f1 = f2 = s.feat; tw = s.tw; tb = s.tb;
        lt = 0.0f;
        if (valid) {
            int64_t ni = s.neigh[row], ei = s.eid[row];
            bool bad = false;
            if (ni < 0 || ni >= s.n_node_rows) { ni = 0; bad = true; }
            if (ei < 0 || ei >= s.n_edge_rows) { ei = 0; bad = true; }
            if (bad) atomicOr(err, 1u);
            nrow = s.node_raw + ni * d.Dn;
            erow = s.edge_raw + ei * d.De;
            f1 = s.feat + row * d.F;
            f2 = s.feat + (s.n + row) * d.F;
            lt = logf((float)(s.tq[row / s.K] - s.tn[row]) + 1.0f);
        }
        e0 = d.Dn; e1 = e0 + d.Dt; e2 = e1 + d.De; e3 = e2 + d.F; e4 = e3 + d.F;
    }
    // tw * lt + tb of time columns t .. t + 3
    __device__ __forceinline__ float4 arg4(int t) const {
        const float4 a = *reinterpret_cast<const float4*>(tw + t), b = *reinterpret_cast<const float4*>(tb + t);
        return make_float4(a.x * lt + b.x, a.y * lt + b.y, a.z * lt + b.z, a.w * lt + b.w);
    }
    // columns c .. c + 3 of the row's concat (c % 4 == 0: one segment)
    __device__ __forceinline__ float4 operator()(int c) const {
        if (!valid || c >= e4) return make_float4(0.f, 0.f, 0.f, 0.f);
        if (c < e0) return *reinterpret_cast<const float4*>(nrow + c);
        if (c < e1) {
            const float4 a = arg4(c - e0);
            return make_float4(cosf(a.x), cosf(a.y), cosf(a.z), cosf(a.w));
        }
        if (c < e2) return *reinterpret_cast<const float4*>(erow + (c - e1));
        if (c < e3) return *reinterpret_cast<const float4*>(f1 + (c - e2));
        return *reinterpret_cast<const float4*>(f2 + (c - e3));
    }
};

// the host's checks of the arrays every input-stage entry takes
static inline bool ei_src_ok(const ei_src& s, int64_t n_nodes) {
    if (!s.node_raw || !s.edge_raw || !s.neigh || !s.eid || !s.tn || !s.tq || !s.tw || !s.tb || !s.feat) return false;
    if (s.n_node_rows < 1 || s.n_edge_rows < 1 || n_nodes < 0 || s.K < 1 || n_nodes > (1ll << 31) / s.K) return false;
    return aligned16({s.node_raw, s.edge_raw, s.tw, s.tb, s.feat});
}

}  // namespace tpnet
