// The encoder's input stage (models/TPNet.py:297-330) in one launch: gather node_raw[neigh] and edge_raw[eid], the time encoding
// cos(tw * log(f32(tq - tn) + 1) + tb), the two halves of the relative encodings, and projection_layer = Linear(Din, H) -> ReLU ->
// Linear(H, Dout) on the matrix cores.  The [n, Din] concat (91 MB per call at B = 1000, K = 20, Din = 572) is never written: every
// lane builds the 8-float operand pieces of its row straight from the sources.
// The two layers, their weight image, the chunk pipeline and the mapping (128 rows per workgroup, one 32-row tile per wave) are
// dense2.hpp's, in the fp32 class of mfma_split.hpp; this file is the row source.  H <= 352 and Dout <= 192 keep all 11 hidden slices
// in accumulators; a wider hidden layer or more outputs take passes of 8 slices with 8 output tiles.  313 workgroups at 40 000 rows.
// Ids outside node_raw / edge_raw read row 0 and set err[0] (tpnet_encoder_input_check reports it); no hand-off between workgroups.
#include "encoder_input.hpp"

namespace tpnet {

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
    const ei_src src{node_raw, edge_raw, tw, tb, feat, neigh, eid, tn, tq, n_node_rows, n_edge_rows, n, K};
    ei_row x4;
    x4.init(src, d, row, err);
    const bool valid = x4.valid;
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
