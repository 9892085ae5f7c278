// The encoder's input stage (models/TPNet.py:297-330) in one launch: gather node_raw[neigh] and edge_raw[eid], the time encoding
// cos(tw * log(f32(tq - tn) + 1) + tb), the two halves of the relative encodings, and projection_layer = Linear(Din, H) -> ReLU ->
// Linear(H, Dout) on the matrix cores.  The [n, Din] concat (91 MB per call at B = 1000, K = 20, Din = 572) is never written: every
// lane builds the 8-float operand pieces of its row straight from the sources.
// Arithmetic: the project's fp32 class (mfma_split.hpp: two-piece operands, three products per term on v_mfma_f32_32x32x16_bf16,
// fp32 accumulators).  Layer 1 is computed as H^T = W1 . X^T, so a hidden slice's accumulator registers
// (row r of the tile, 16 hidden units per lane) are layer 2's B operand without a transpose.
// Mapping: a workgroup of 4 waves takes 128 rows, one 32-row tile per wave.  The split weights (tpnet_encoder_input_prepare: 1.16 MB
// at 572 -> 344 -> 172, in exactly the per-lane operand order) do not fit LDS; they are cut into equal chunks of 24 KB -- one k-step
// of W1 for all hidden slices of a pass, later one hidden slice of W2 for all output tiles -- that the four waves share through
// two LDS buffers: the next chunk is fetched into registers ahead of the current one's products and written to the other buffer
// behind them, one barrier per chunk.  Up to 11 hidden slices (352 units) stay in accumulators at once; a wider hidden layer or
// more than 192 outputs take the second variant: passes of 8 slices over the row's operands.  313 workgroups at 40 000 rows.
// Ids outside node_raw / edge_raw read row 0 and set err[0] (tpnet_encoder_input_check reports it); no hand-off between workgroups.
#include "tpnet_common.h"
#include "mfma_split.hpp"

namespace tpnet {

static constexpr int EI_T = 256;                 // threads per workgroup: 4 waves, one per SIMD (the accumulators want the registers)
static constexpr int EI_ROWS = 128;              // rows per workgroup
static constexpr int EI_HG = 11;                 // hidden slices of 32 units in one pass of the narrow variant (H <= 352, Dout <= 192)
static constexpr int EI_HG_WIDE = 8;             // ... per pass of the wide one (any served H and Dout): fewer, to leave room for 8 output tiles
static constexpr int EI_OS = 6, EI_OS_WIDE = 8;  // output tiles of 32 columns the two variants compute
// 16-byte elements of a chunk of the weight image: the larger of a k-step of W1 for HG slices (HG * 128) and a slice of W2 for OS
// output tiles (OS * 256), a multiple of the workgroup size -- every thread moves the same number of elements of every chunk
static constexpr int EI_CH = 1536, EI_CH_WIDE = 2048;

struct ei_dims {
    int Dn, Dt, De, F, H, Dout;                  // the caller's six
    int Din, KS;                                 // Dn + Dt + De + 2 F; k-steps of 16 columns
    int HG, NP, OS, CH;                          // the variant: hidden slices per pass, passes, output tiles (all computed; the
};                                               // image holds zeros beyond H and Dout), elements per chunk

static bool ei_make_dims(const int32_t* d, ei_dims& o) {
    if (!d) return false;
    o.Dn = d[0]; o.Dt = d[1]; o.De = d[2]; o.F = d[3]; o.H = d[4]; o.Dout = d[5];
    if (o.Dn < 4 || o.Dt < 4 || o.De < 4 || o.F < 4 || o.H < 1 || o.Dout < 4) return false;
    if ((o.Dn | o.Dt | o.De | o.F | o.Dout) & 3) return false;
    if (o.Dn > 1024 || o.Dt > 1024 || o.De > 1024 || o.F > 512 || o.H > 512 || o.Dout > 256) return false;
    o.Din = o.Dn + o.Dt + o.De + 2 * o.F;
    if (o.Din > 1024) return false;
    o.KS = (o.Din + 15) / 16;
    const int HS = (o.H + 31) / 32, OS = (o.Dout + 31) / 32;
    const bool narrow = HS <= EI_HG && OS <= EI_OS;
    o.HG = narrow ? EI_HG : EI_HG_WIDE;
    o.NP = (HS + o.HG - 1) / o.HG;
    o.OS = narrow ? EI_OS : EI_OS_WIDE;
    o.CH = narrow ? EI_CH : EI_CH_WIDE;
    return true;
}

// 16-byte elements of the chunks (everything in front of the biases)
static __host__ __device__ inline uint32_t ei_chunk_elems(const ei_dims& d) {
    return (uint32_t)(d.NP * (d.KS + d.HG)) * (uint32_t)d.CH;
}

// ---- the weight image.  Chunks of CH elements in the order the kernel consumes them, per pass p (slices w0 = HG p .. w0 + HG - 1;
// HG = 11, one pass and OS = 6 output tiles where H <= 352 and Dout <= 192, else HG = 8 and OS = 8: the kernel computes ALL of
// them, so that every loop over slices and tiles has a compile-time count)
//   k-step s = 0..KS-1:  element (wl * 2 + piece) * 64 + lane  = W1[32 (w0 + wl) + r][16 s + 8 h + j], piece 0 = hi, 1 = lo
//   slice wl = 0..HG-1:  element ((s2 * OS + t) * 2 + piece) * 64 + lane = W2[32 t + r][32 (w0 + wl) + acc_row(q, h)], q = 8 s2 + j
// (lane = 32 h + r, j = 0..7 the element's eight bf16), zero beyond H / Din / Dout; then b1 padded to 32 NP HG and b2 to 32 OS floats.
__global__ __launch_bounds__(256) void k_encoder_input_image(const float* __restrict__ w1, const float* __restrict__ b1,
                                                             const float* __restrict__ w2, const float* __restrict__ b2,
                                                             const ei_dims d, uint4* __restrict__ img) {
    const uint32_t e = blockIdx.x * 256u + threadIdx.x;
    const uint32_t total = ei_chunk_elems(d);
    if (e >= total) {
        const uint32_t f = (e - total) * 4u;                                   // first of four bias floats
        const uint32_t nb1 = (uint32_t)(d.NP * d.HG) * 32u, nb2 = (uint32_t)d.OS * 32u;
        if (f >= nb1 + nb2) return;
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t i = f + j;
            v[j] = i < nb1 ? (i < (uint32_t)d.H ? b1[i] : 0.0f) : (i - nb1 < (uint32_t)d.Dout ? b2[i - nb1] : 0.0f);
        }
        reinterpret_cast<float4*>(img + total)[f / 4u] = make_float4(v[0], v[1], v[2], v[3]);
        return;
    }
    const int chunk = e / (uint32_t)d.CH, el = e % (uint32_t)d.CH;             // el: element of the chunk
    const int w0 = chunk / (d.KS + d.HG) * d.HG, cj = chunk % (d.KS + d.HG);   // the pass's first slice; chunk of the pass
    const int lane = el & 63, piece = (el >> 6) & 1, r = lane & 31, h = lane >> 5;
    float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (cj < d.KS) {
        const int s = cj, wl = el >> 7;
        const int row = 32 * (w0 + wl) + r;
        if (wl < d.HG) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int col = 16 * s + 8 * h + j;
                v[j] = (row < d.H && col < d.Din) ? w1[(size_t)row * d.Din + col] : 0.0f;
            }
        }
    } else {
        const int wl = cj - d.KS;
        const int s2 = el / (d.OS * 128), t = (el >> 7) % d.OS;
        const int row = 32 * t + r;
        if (s2 < 2) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int q = 8 * s2 + j;
                const int col = 32 * (w0 + wl) + acc_row(q, h);
                v[j] = (row < d.Dout && col < d.H) ? w2[(size_t)row * d.H + col] : 0.0f;
            }
        }
    }
    bf16x8 hi, lo;
    split8(v, hi, lo);
    *reinterpret_cast<bf16x8*>(img + e) = piece ? lo : hi;
}

// HG hidden slices per pass, OSM output tiles; MULTI: more than one pass may be needed (layer 2's accumulators then live through
// the later passes' layer 1)
template <int HG, int OSM, bool MULTI>
__global__ __launch_bounds__(EI_T) void k_encoder_input(const float* __restrict__ node_raw, int64_t n_node_rows,
                                                        const float* __restrict__ edge_raw, int64_t n_edge_rows,
                                                        const int64_t* __restrict__ neigh, const int64_t* __restrict__ eid,
                                                        const double* __restrict__ tn, const double* __restrict__ tq,
                                                        const float* __restrict__ tw, const float* __restrict__ tb,
                                                        const float* __restrict__ feat, int64_t n, int K, const ei_dims d,
                                                        const uint4* __restrict__ img, float* __restrict__ out,
                                                        uint32_t* __restrict__ err) {
    constexpr int CH = MULTI ? EI_CH_WIDE : EI_CH, EI_PF = CH / EI_T;
    static_assert(CH >= HG * 128 && CH >= OSM * 256 && CH % EI_T == 0, "a chunk holds a k-step of W1 and a slice of W2");
    __shared__ uint4 buf[2][CH];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
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
    // ---- the chunk pipeline: fetch(c) reads chunk c into registers, commit(b) writes it to buffer b behind the current products
    // (every chunk has CH elements and every thread moves EI_PF of them, unconditionally: the registers in between stay registers;
    // behind the last chunk the first one is fetched again and never used)
    const uint32_t nchunks = (uint32_t)(d.NP * (d.KS + HG));
    static_assert(EI_PF == 6 || EI_PF == 8, "the prefetch registers below");
    uint4 p0, p1, p2, p3, p4, p5, p6, p7;      // (named, not an array: an array indexed inside the lambdas ends up in scratch memory)
    auto fetch = [&](uint32_t c) {
        const uint4* src = img + (c < nchunks ? c : 0u) * (uint32_t)CH + tid;
        p0 = src[0]; p1 = src[EI_T]; p2 = src[2 * EI_T]; p3 = src[3 * EI_T]; p4 = src[4 * EI_T]; p5 = src[5 * EI_T];
        if constexpr (EI_PF == 8) { p6 = src[6 * EI_T]; p7 = src[7 * EI_T]; }
    };
    auto commit = [&](int b) {
        uint4* dst = buf[b] + tid;
        dst[0] = p0; dst[EI_T] = p1; dst[2 * EI_T] = p2; dst[3 * EI_T] = p3; dst[4 * EI_T] = p4; dst[5 * EI_T] = p5;
        if constexpr (EI_PF == 8) { dst[6 * EI_T] = p6; dst[7 * EI_T] = p7; }
        __syncthreads();
    };
    const float* bias = reinterpret_cast<const float*>(img + ei_chunk_elems(d));
    f32x16 y[OSM];
#pragma unroll
    for (int t = 0; t < OSM; ++t)
#pragma unroll
        for (int q = 0; q < 16; ++q) y[t][q] = 0.0f;
    uint32_t chunk = 0;
    int cur = 0;
    fetch(0);
    commit(0);
    for (int p = 0; p < (MULTI ? d.NP : 1); ++p) {
        const int w0 = p * HG;
        f32x16 acc[HG];
#pragma unroll
        for (int wl = 0; wl < HG; ++wl)
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[wl][q] = 0.0f;
        // ---- layer 1: H^T[32 w ..][rows] += W1[32 w .., 16 s ..] . X^T, k-step by k-step, all slices of the pass
        float4 xa = x4(8 * h), xb = x4(8 * h + 4);
        for (int s = 0; s < d.KS; ++s) {
            fetch(chunk + 1);
            bf16x8 bxh, bxl;
            split8(xa, xb, bxh, bxl);
            xa = x4(16 * (s + 1) + 8 * h);                                      // (beyond Din: zeros)
            xb = x4(16 * (s + 1) + 8 * h + 4);
            const bf16x8* W = reinterpret_cast<const bf16x8*>(buf[cur]) + lane;
            // all operands of the k-step first (one LDS round trip, not one per product), then the products term-major: the
            // three products of one accumulator lie HG instructions apart
            bf16x8 ah[HG], al[HG];
#pragma unroll
            for (int wl = 0; wl < HG; ++wl) {
                ah[wl] = W[(wl * 2) * 64];
                al[wl] = W[(wl * 2 + 1) * 64];
            }
            __builtin_amdgcn_sched_group_barrier(0x100, 2 * HG, 0);             // (the scheduler otherwise waits on every read in turn)
            __builtin_amdgcn_sched_group_barrier(0x008, 3 * HG, 0);
            mm3(ah, al, bxh, bxl, acc);
            commit(cur ^ 1);
            cur ^= 1;
            ++chunk;
        }
        // ---- layer 2, slice by slice: bias, ReLU and split of the slice's accumulators (relu_split16) are the B operand; every
        // output tile takes its share
#pragma unroll
        for (int wl = 0; wl < HG; ++wl) {
            {
                fetch(chunk + 1);
                float bv[16];                                                   // b1 in accumulator order: acc_row(4 q4 + j, h) = 8 q4 + 4 h + j
#pragma unroll
                for (int q4 = 0; q4 < 4; ++q4) {
                    const float4 bb = *reinterpret_cast<const float4*>(bias + 32 * (w0 + wl) + 8 * q4 + 4 * h);
                    bv[4 * q4] = bb.x; bv[4 * q4 + 1] = bb.y; bv[4 * q4 + 2] = bb.z; bv[4 * q4 + 3] = bb.w;
                }
                bf16x8 bhh[2], bhl[2];
                relu_split16(acc[wl], bv, bhh, bhl);
                const bf16x8* W = reinterpret_cast<const bf16x8*>(buf[cur]) + lane;
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2) {
                    bf16x8 ah[OSM], al[OSM];
#pragma unroll
                    for (int t = 0; t < OSM; ++t) {
                        ah[t] = W[((s2 * OSM + t) * 2) * 64];
                        al[t] = W[((s2 * OSM + t) * 2 + 1) * 64];
                    }
                    mm3(ah, al, bhh[s2], bhl[s2], y);
                }
                commit(cur ^ 1);
                cur ^= 1;
                ++chunk;
            }
        }
    }
    // ---- y[t][4 i .. 4 i + 3] = outputs 32 t + 8 i + 4 h + (0..3) of row r
    if (valid) {
        const float* b2 = bias + 32 * d.NP * HG;
        float* yo = out + row * d.Dout;
#pragma unroll
        for (int t = 0; t < OSM; ++t) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int o = 32 * t + 8 * i + 4 * h;
                if (o < d.Dout) {
                    const float4 c = *reinterpret_cast<const float4*>(b2 + o);
                    *reinterpret_cast<float4*>(yo + o) =
                        make_float4(y[t][4 * i] + c.x, y[t][4 * i + 1] + c.y, y[t][4 * i + 2] + c.z, y[t][4 * i + 3] + c.w);
                }
            }
        }
    }
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
    return (size_t)tpnet::ei_chunk_elems(d) * 16 + (size_t)(d.NP * d.HG + d.OS) * 32 * sizeof(float);
}

extern "C" int tpnet_encoder_input_prepare(const float* w1, const float* b1, const float* w2, const float* b2, const int32_t* dims,
                                           void* img, void* stream) {
    tpnet::ei_dims d;
    if (!w1 || !b1 || !w2 || !b2 || !img || (reinterpret_cast<uintptr_t>(img) & 15) || !tpnet::ei_make_dims(dims, d))
        return TPNET_ERR_BAD_ARG;
    const uint32_t elems = tpnet::ei_chunk_elems(d) + (uint32_t)(d.NP * d.HG + d.OS) * 8u;
    hipLaunchKernelGGL(tpnet::k_encoder_input_image, dim3((elems + 255) / 256), dim3(256), 0, (hipStream_t)stream, w1, b1, w2, b2, d,
                       reinterpret_cast<uint4*>(img));
    TPNET_HIP_TRY(hipGetLastError());
    return TPNET_OK;
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
    const auto kernel = d.HG == tpnet::EI_HG ? tpnet::k_encoder_input<tpnet::EI_HG, tpnet::EI_OS, false>
                                             : tpnet::k_encoder_input<tpnet::EI_HG_WIDE, tpnet::EI_OS_WIDE, true>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)((n + tpnet::EI_ROWS - 1) / tpnet::EI_ROWS)), dim3(tpnet::EI_T), 0, (hipStream_t)stream,
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
