// The encoder's input stage (models/TPNet.py:297-330) in one launch: gather node_raw[neigh] and edge_raw[eid], the time encoding
// cos(tw * log(f32(tq - tn) + 1) + tb), the two halves of the relative encodings, and projection_layer = Linear(Din, H) -> ReLU ->
// Linear(H, Dout) on the matrix cores.  The [n, Din] concat (91 MB per call at B = 1000, K = 20, Din = 572) is never written: every
// lane builds the 8-float operand pieces of its row straight from the sources.
// The two layers, their weight image, the chunk pipeline and the mapping (128 rows per workgroup, one 32-row tile per wave) are
// dense2.hpp's, in the fp32 class of mfma_split.hpp; this file is the row source.  H <= 352 and Dout <= 192 keep all 11 hidden slices
// in accumulators; a wider hidden layer or more outputs take passes of 8 slices with 8 output tiles.  313 workgroups at 40 000 rows.
// Ids outside node_raw / edge_raw read row 0 and set err[0] (tpnet_encoder_input_check reports it); no hand-off between workgroups.
#include "dense2.hpp"

namespace tpnet {

struct ei_dims {
    int Dn, Dt, De, F;                           // the segments of a row: node | time | edge | two halves of F relative encodings
    d2_dims l;                                   // the layers: Din = Dn + Dt + De + 2 F, H, Dout and the variant
};

static bool ei_make_dims(const int32_t* d, ei_dims& o) {
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

// HG hidden slices per pass, OSM output tiles, MULTI: dense2_rows'
template <int HG, int OSM, bool MULTI>
__global__ __launch_bounds__(D2_T) void k_encoder_input(const float* __restrict__ node_raw, int64_t n_node_rows,
                                                        const float* __restrict__ edge_raw, int64_t n_edge_rows,
                                                        const int64_t* __restrict__ neigh, const int64_t* __restrict__ eid,
                                                        const double* __restrict__ tn, const double* __restrict__ tq,
                                                        const float* __restrict__ tw, const float* __restrict__ tb,
                                                        const float* __restrict__ feat, int64_t n, int K, const ei_dims d,
                                                        const uint4* __restrict__ img, float* __restrict__ out,
                                                        uint32_t* __restrict__ err) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31;
    const int64_t row = ((int64_t)blockIdx.x * 4 + wave) * 32 + r;
    const bool valid = row < n;
    // ---- this lane's row: the four sources and the scaled time delta (f64 difference -> f32 -> log(x + 1), TPNet.py:299-301)
    const float *nrow = node_raw, *erow = edge_raw, *f1 = feat, *f2 = feat;
    float lt = 0.0f;
    if (valid) {
        int64_t ni = neigh[row], ei = eid[row];
        bool bad = false;
        if (ni < 0 || ni >= n_node_rows) { ni = 0; bad = true; }
        if (ei < 0 || ei >= n_edge_rows) { ei = 0; bad = true; }
        if (bad) atomicOr(err, 1u);
        nrow = node_raw + ni * d.Dn;
        erow = edge_raw + ei * d.De;
        f1 = feat + row * d.F;
        f2 = feat + (n + row) * d.F;
        lt = logf((float)(tq[row / K] - tn[row]) + 1.0f);
    }
    const int e0 = d.Dn, e1 = e0 + d.Dt, e2 = e1 + d.De, e3 = e2 + d.F, e4 = e3 + d.F;
    // columns c .. c + 3 of the row's concat (c % 4 == 0: one segment)
    auto x4 = [&](int c) -> float4 {
        if (!valid || c >= e4) return make_float4(0.f, 0.f, 0.f, 0.f);
        if (c < e0) return *reinterpret_cast<const float4*>(nrow + c);
        if (c < e1) {
            const float4 a = *reinterpret_cast<const float4*>(tw + (c - e0)), b = *reinterpret_cast<const float4*>(tb + (c - e0));
            return make_float4(cosf(a.x * lt + b.x), cosf(a.y * lt + b.y), cosf(a.z * lt + b.z), cosf(a.w * lt + b.w));
        }
        if (c < e2) return *reinterpret_cast<const float4*>(erow + (c - e1));
        if (c < e3) return *reinterpret_cast<const float4*>(f1 + (c - e2));
        return *reinterpret_cast<const float4*>(f2 + (c - e3));
    };
    float* yo = out + row * d.l.Dout;
    dense2_rows<HG, OSM, MULTI, act_relu>(d.l, img, valid, x4, [&](int o, const float4 v) { *reinterpret_cast<float4*>(yo + o) = v; });
}

}  // namespace tpnet

extern "C" int tpnet_encoder_input_supported(int32_t Dn, int32_t Dt, int32_t De, int32_t F, int32_t H, int32_t Dout) {
    const int32_t v[6] = {Dn, Dt, De, F, H, Dout};
    tpnet::ei_dims d;
    return tpnet::ei_make_dims(v, d) ? 1 : 0;
}

extern "C" size_t tpnet_encoder_input_image_bytes(int32_t Dn, int32_t Dt, int32_t De, int32_t F, int32_t H, int32_t Dout) {
    const int32_t v[6] = {Dn, Dt, De, F, H, Dout};
    tpnet::ei_dims d;
    if (!tpnet::ei_make_dims(v, d)) return 0;
    return tpnet::d2_image_bytes(d.l);
}

extern "C" int tpnet_encoder_input_prepare(const float* w1, const float* b1, const float* w2, const float* b2, const int32_t* dims,
                                           void* img, void* stream) {
    tpnet::ei_dims d;
    if (!w1 || !b1 || !w2 || !b2 || !img || (reinterpret_cast<uintptr_t>(img) & 15) || !tpnet::ei_make_dims(dims, d))
        return TPNET_ERR_BAD_ARG;
    return tpnet::d2_prepare(w1, b1, w2, b2, d.l, img, (hipStream_t)stream);
}

extern "C" int tpnet_encoder_input(const float* node_raw, int64_t n_node_rows, const float* edge_raw, int64_t n_edge_rows,
                                   const int64_t* neigh, const int64_t* eid, const double* tn, const double* tq, const float* tw,
                                   const float* tb, const float* feat, int64_t n_nodes, int32_t K, const int32_t* dims,
                                   const void* img, float* out, uint32_t* err, void* stream) {
    tpnet::ei_dims d;
    if (!node_raw || !edge_raw || !neigh || !eid || !tn || !tq || !tw || !tb || !feat || !img || !out || !err) return TPNET_ERR_BAD_ARG;
    if (n_node_rows < 1 || n_edge_rows < 1 || n_nodes < 0 || K < 1 || !tpnet::ei_make_dims(dims, d)) return TPNET_ERR_BAD_ARG;
    if (n_nodes > (1ll << 31) / K) return TPNET_ERR_BAD_ARG;
    if ((reinterpret_cast<uintptr_t>(node_raw) | reinterpret_cast<uintptr_t>(edge_raw) | reinterpret_cast<uintptr_t>(tw) |
         reinterpret_cast<uintptr_t>(tb) | reinterpret_cast<uintptr_t>(feat) | reinterpret_cast<uintptr_t>(img) |
         reinterpret_cast<uintptr_t>(out)) & 15)
        return TPNET_ERR_BAD_ARG;
    const int64_t n = n_nodes * K;
    if (n == 0) return TPNET_OK;
    const auto kernel = d.l.HG == tpnet::D2_HG ? tpnet::k_encoder_input<tpnet::D2_HG, tpnet::D2_OS, false>
                                             : tpnet::k_encoder_input<tpnet::D2_HG_WIDE, tpnet::D2_OS_WIDE, true>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)((n + tpnet::D2_ROWS - 1) / tpnet::D2_ROWS)), dim3(tpnet::D2_T), 0, (hipStream_t)stream,
                       node_raw, n_node_rows, edge_raw, n_edge_rows, neigh, eid, tn, tq, tw, tb, feat, n, (int)K, d,
                       reinterpret_cast<const uint4*>(img), out, err);
    TPNET_HIP_TRY(hipGetLastError());
    return TPNET_OK;
}

extern "C" int tpnet_encoder_input_check(uint32_t* err, void* stream) {
    if (!err) return TPNET_ERR_BAD_ARG;
    uint32_t h = 0;
    TPNET_HIP_TRY(hipMemcpyAsync(&h, err, sizeof(h), hipMemcpyDeviceToHost, (hipStream_t)stream));
    TPNET_HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    if (h != 0) {
        TPNET_HIP_TRY(hipMemsetAsync(err, 0, sizeof(h), (hipStream_t)stream));
        return TPNET_ERR_INDEX;
    }
    return TPNET_OK;
}
