// The weight image of dense2.hpp's two layers and its host arithmetic (the kernels that consume it: encoder_input.hip, mixer.hip,
// mixer_channel_train.hip).
#include "dense2.hpp"

namespace tpnet {

void d2_make_dims(int Din, int H, int Dout, bool mid, d2_dims& o) {
    o.Din = Din; o.H = H; o.Dout = Dout;
    o.KS = (Din + 15) / 16;
    const int HS = (H + 31) / 32, OS = (Dout + 31) / 32;
    const bool narrow = HS <= D2_HG && OS <= D2_OS;
    o.HG = narrow ? D2_HG : D2_HG_WIDE;
    o.NP = (HS + o.HG - 1) / o.HG;
    o.OS = narrow || (mid && OS <= D2_OS) ? D2_OS : D2_OS_WIDE;
    o.CH = d2_chunk(o.HG, o.OS);
}

size_t d2_image_bytes(const d2_dims& d) {
    return (size_t)d2_chunk_elems(d) * 16 + (size_t)(d.NP * d.HG + d.OS) * 32 * sizeof(float);
}

// ---- the weight image.  Chunks of CH elements in the order the kernel consumes them, per pass p (slices w0 = HG p .. w0 + HG - 1;
// the kernel computes ALL HG slices and OS tiles of its variant, so that every loop over slices and tiles has a compile-time count)
//   k-step s = 0..KS-1:  element (wl * 2 + piece) * 64 + lane  = W1[32 (w0 + wl) + r][16 s + 8 h + j], piece 0 = hi, 1 = lo
//   slice wl = 0..HG-1:  element ((s2 * OS + t) * 2 + piece) * 64 + lane = W2[32 t + r][32 (w0 + wl) + acc_row(q, h)], q = 8 s2 + j
// (lane = 32 h + r, j = 0..7 the element's eight bf16), zero beyond H / Din / Dout; then b1 padded to 32 NP HG and b2 to 32 OS floats.
__global__ __launch_bounds__(256) void k_dense2_image(const float* __restrict__ w1, const float* __restrict__ b1,
                                                      const float* __restrict__ w2, const float* __restrict__ b2,
                                                      const d2_dims d, uint4* __restrict__ img) {
    const uint32_t e = blockIdx.x * 256u + threadIdx.x;
    const uint32_t total = d2_chunk_elems(d);
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

int d2_prepare(const float* w1, const float* b1, const float* w2, const float* b2, const d2_dims& d, void* img, hipStream_t s) {
    const uint32_t elems = d2_chunk_elems(d) + (uint32_t)(d.NP * d.HG + d.OS) * 8u;
    hipLaunchKernelGGL(k_dense2_image, dim3((elems + 255) / 256), dim3(256), 0, s, w1, b1, w2, b2, d, reinterpret_cast<uint4*>(img));
    TPNET_HIP_TRY(hipGetLastError());
    return TPNET_OK;
}

}  // namespace tpnet
