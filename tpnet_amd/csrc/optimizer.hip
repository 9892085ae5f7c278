// The optimizer step on the device: Adam, SGD and RMSprop as utils.create_optimizer builds them (utils/utils.py:61-79 -- L2
// weight_decay, no amsgrad, momentum 0, not centered), for MANY tensors in one launch (train_link_prediction.py:386 steps the 38
// trainable tensors of a TPNet + LinkPredictor_v1 once per batch).
//
// The rules, per element, fp32, ONE rounding per written operation (-ffp-contract=off: no fused multiply-add; hipcc's IEEE division
// and square root).  c[] are the entry's scalars, formed by the caller in double and rounded once to fp32 (include/tpnet_hip.h):
//   every rule    g1 = c[1] != 0 ? g + c[1] * p : g                                          c[1] = weight_decay
//   Adam          m' = c[2] * m + c[3] * g1                                                  c[2] = beta1, c[3] = 1 - beta1
//                 v' = c[4] * v + (c[5] * g1) * g1                                           c[4] = beta2, c[5] = 1 - beta2
//                 p' = p - c[0] * (m' / (sqrt(v') / c[6] + c[7]))                            c[0] = lr / (1 - beta1^t), c[6] = sqrt(1 - beta2^t),
//                                                                                            c[7] = eps
//   SGD           p' = p - c[0] * g1                                                         c[0] = lr
//   RMSprop       s' = c[2] * s + (c[3] * g1) * g1                                           c[2] = alpha, c[3] = 1 - alpha
//                 p' = p - c[0] * (g1 / (sqrt(s') + c[4]))                                   c[0] = lr, c[4] = eps
// Every product, sum, quotient and root above is one operation, evaluated in the order the parentheses and the usual left-to-right
// reading give; tpnet_amd/optimizer.py: optimizer_step_host restates exactly this in numpy and the tests compare bits.
//
// The table of tensors travels BY VALUE in the kernel arguments: gradients get new addresses every step (zero_grad sets them to None),
// so the table is rebuilt every step, and a by-value table needs no copy to the device, no staging buffer that has to outlive the
// launch and no synchronisation.  OPT_CAP entries keep the argument block under 4 KB; more tensors are more launches.
// A workgroup takes ONE chunk of OPT_CHUNK elements of ONE tensor; it finds the tensor by counting the entries whose first chunk is
// at or below its own index (the table's chunk prefix, a compact array: a few wide scalar loads and scalar compares).
// Elements are independent: no fences, no atomics, no hand-off between workgroups.
#include "tpnet_common.h"

#include <math.h>

namespace tpnet {

static constexpr int OPT_CAP = 44;            // entries per launch: 44 * 80 + 44 * 4 + 16 = 3 712 bytes of kernel arguments
static constexpr int OPT_CHUNK = 2048;        // elements per workgroup: 256 threads x 2 x float4
static constexpr int OPT_THREADS = 256;
static constexpr uint32_t OPT_VEC = 1u;       // OptimTable::e[].flags: p, g and the state arrays the rule reads are 16-byte aligned
static constexpr int64_t OPT_MAX_CHUNKS = (int64_t)1 << 30;   // chunks per launch (a grid's x extent stays below 2^31)

struct OptimTable {
    tpnet_optim_tensor e[OPT_CAP];            // flags: OPT_VEC or 0, set here (the caller's word is not looked at)
    uint32_t chunk0[OPT_CAP];                 // first chunk of entry k; 0xffffffff behind the last entry
    int32_t count;
    int32_t pad[3];
};
static_assert(sizeof(tpnet_optim_tensor) == 80, "tpnet_optim_tensor must be 80 bytes");
static_assert(sizeof(OptimTable) + 256 <= 4096, "the table and the hidden arguments must fit the 4 KB argument block");

template <int RULE>
__device__ inline void optim_elem(const float* c, float p, float g, float& s1, float& s2, float& p_out) {
    if (c[1] != 0.f) {
        const float t = c[1] * p;
        g = g + t;
    }
    if constexpr (RULE == TPNET_OPTIM_ADAM) {
        const float a = c[2] * s1;
        const float b = c[3] * g;
        s1 = a + b;
        const float d = c[4] * s2;
        float e = c[5] * g;
        e = e * g;
        s2 = d + e;
        float den = sqrtf(s2);
        den = den / c[6];
        den = den + c[7];
        const float q = s1 / den;
        const float u = c[0] * q;
        p_out = p - u;
    } else if constexpr (RULE == TPNET_OPTIM_SGD) {
        const float u = c[0] * g;
        p_out = p - u;
    } else {
        const float a = c[2] * s1;
        float e = c[3] * g;
        e = e * g;
        s1 = a + e;
        float den = sqrtf(s1);
        den = den + c[4];
        const float q = g / den;
        const float u = c[0] * q;
        p_out = p - u;
    }
}

template <int RULE>
__global__ __launch_bounds__(OPT_THREADS) void k_optim_step(const OptimTable tab) {
    constexpr bool HAS1 = RULE != TPNET_OPTIM_SGD, HAS2 = RULE == TPNET_OPTIM_ADAM;
    const uint32_t b = blockIdx.x;
    int k = 0;                                                 // chunk0 ascends: the entry is the last one that starts at or below b
#pragma unroll
    for (int j = 1; j < OPT_CAP; ++j) k += tab.chunk0[j] <= b ? 1 : 0;
    const tpnet_optim_tensor& e = tab.e[k];                    // (k is uniform: loads from the argument block)
    const int64_t base = (int64_t)(b - tab.chunk0[k]) * OPT_CHUNK;
    const int64_t left = e.n - base;
    const int m = left < OPT_CHUNK ? (int)left : OPT_CHUNK;    // elements of this chunk, >= 1
    float c[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) c[j] = e.c[j];
    float* __restrict__ p = e.p + base;
    const float* __restrict__ g = e.g + base;
    float* __restrict__ s1 = HAS1 ? e.s1 + base : nullptr;
    float* __restrict__ s2 = HAS2 ? e.s2 + base : nullptr;
    if (e.flags & OPT_VEC) {                                   // (base is a multiple of 4 elements: the alignment holds in every chunk)
        const int m4 = m & ~3;
        for (int i = (int)threadIdx.x * 4; i < m4; i += OPT_THREADS * 4) {
            float4 pv = *reinterpret_cast<const float4*>(p + i);
            const float4 gv = *reinterpret_cast<const float4*>(g + i);
            float4 av = make_float4(0.f, 0.f, 0.f, 0.f), bv = av;
            if constexpr (HAS1) av = *reinterpret_cast<const float4*>(s1 + i);
            if constexpr (HAS2) bv = *reinterpret_cast<const float4*>(s2 + i);
            optim_elem<RULE>(c, pv.x, gv.x, av.x, bv.x, pv.x);
            optim_elem<RULE>(c, pv.y, gv.y, av.y, bv.y, pv.y);
            optim_elem<RULE>(c, pv.z, gv.z, av.z, bv.z, pv.z);
            optim_elem<RULE>(c, pv.w, gv.w, av.w, bv.w, pv.w);
            if constexpr (HAS1) *reinterpret_cast<float4*>(s1 + i) = av;
            if constexpr (HAS2) *reinterpret_cast<float4*>(s2 + i) = bv;
            *reinterpret_cast<float4*>(p + i) = pv;
        }
        const int i = m4 + (int)threadIdx.x;                   // the tail: at most 3 elements
        if (i < m) {
            float a = 0.f, v = 0.f, pn;
            if constexpr (HAS1) a = s1[i];
            if constexpr (HAS2) v = s2[i];
            optim_elem<RULE>(c, p[i], g[i], a, v, pn);
            if constexpr (HAS1) s1[i] = a;
            if constexpr (HAS2) s2[i] = v;
            p[i] = pn;
        }
    } else {
        for (int i = (int)threadIdx.x; i < m; i += OPT_THREADS) {
            float a = 0.f, v = 0.f, pn;
            if constexpr (HAS1) a = s1[i];
            if constexpr (HAS2) v = s2[i];
            optim_elem<RULE>(c, p[i], g[i], a, v, pn);
            if constexpr (HAS1) s1[i] = a;
            if constexpr (HAS2) s2[i] = v;
            p[i] = pn;
        }
    }
}

static int optim_launch(int rule, OptimTable& tab, uint32_t chunks, hipStream_t s) {
    for (int k = tab.count; k < OPT_CAP; ++k) tab.chunk0[k] = 0xffffffffu;
    const dim3 grid(chunks), block(OPT_THREADS);
    if (rule == TPNET_OPTIM_ADAM) hipLaunchKernelGGL(k_optim_step<TPNET_OPTIM_ADAM>, grid, block, 0, s, tab);
    else if (rule == TPNET_OPTIM_SGD) hipLaunchKernelGGL(k_optim_step<TPNET_OPTIM_SGD>, grid, block, 0, s, tab);
    else hipLaunchKernelGGL(k_optim_step<TPNET_OPTIM_RMSPROP>, grid, block, 0, s, tab);
    TPNET_HIP_TRY(hipGetLastError());
    return TPNET_OK;
}

}  // namespace tpnet

using namespace tpnet;

extern "C" {

int tpnet_optim_max_tensors(void) { return OPT_CAP; }
int tpnet_optim_chunk(void) { return OPT_CHUNK; }

int tpnet_optim_step(int rule, const tpnet_optim_tensor* tensors, int32_t count, void* stream) {
    if (rule != TPNET_OPTIM_ADAM && rule != TPNET_OPTIM_SGD && rule != TPNET_OPTIM_RMSPROP) return TPNET_ERR_BAD_ARG;
    if (count < 0 || (count > 0 && !tensors)) return TPNET_ERR_BAD_ARG;
    const bool has1 = rule != TPNET_OPTIM_SGD, has2 = rule == TPNET_OPTIM_ADAM;
    for (int32_t i = 0; i < count; ++i) {                      // every refusal comes before the first launch
        const tpnet_optim_tensor& t = tensors[i];
        if (!t.p || !t.g || (has1 && !t.s1) || (has2 && !t.s2)) return TPNET_ERR_BAD_ARG;
        if (t.n < 0 || t.n > OPT_MAX_CHUNKS * OPT_CHUNK) return TPNET_ERR_BAD_ARG;
        if (((uintptr_t)t.p | (uintptr_t)t.g | (has1 ? (uintptr_t)t.s1 : 0) | (has2 ? (uintptr_t)t.s2 : 0)) & 3) return TPNET_ERR_BAD_ARG;
    }
    hipStream_t s = (hipStream_t)stream;
    OptimTable tab;
    tab.count = 0;
    tab.pad[0] = tab.pad[1] = tab.pad[2] = 0;
    int64_t chunks = 0;
    for (int32_t i = 0; i < count; ++i) {
        const tpnet_optim_tensor& t = tensors[i];
        if (t.n == 0) continue;
        const int64_t nc = (t.n + OPT_CHUNK - 1) / OPT_CHUNK;
        if (tab.count == OPT_CAP || chunks + nc > OPT_MAX_CHUNKS) {
            const int rc = optim_launch(rule, tab, (uint32_t)chunks, s);
            if (rc != TPNET_OK) return rc;
            tab.count = 0;
            chunks = 0;
        }
        tpnet_optim_tensor& e = tab.e[tab.count];
        e = t;
        if (!has1) e.s1 = nullptr;
        if (!has2) e.s2 = nullptr;
        e.flags = aligned16({e.p, e.g, e.s1, e.s2}) ? OPT_VEC : 0u;
        e.reserved = 0;
        tab.chunk0[tab.count++] = (uint32_t)chunks;
        chunks += nc;
    }
    return tab.count ? optim_launch(rule, tab, (uint32_t)chunks, s) : TPNET_OK;
}

}  // extern "C"
