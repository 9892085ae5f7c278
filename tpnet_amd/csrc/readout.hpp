// Pairwise readout (models/TPNet.py:112-128 before self.mlp) as device functions: one pair per group of LPP lanes
// (gram_pair, gram_rows), two pairs that share their first node (gram_shared) and the encoder's anchored walk (gram_anchored,
// AnchorWalk).  Used by readout.hip, the fused step, the windowed pipeline and the feature kernels.  The phases they share
// (row set-up, Gram accumulation, reduce-and-store tail, output slots, finish rule) are free functions over arrays the
// caller owns, each written once.
#pragma once
#include "device_common.hpp"

namespace tpnet {

// ---------------------------------------------------------------------------------------------------------------
// shared pieces
// ---------------------------------------------------------------------------------------------------------------
// the finish rule of a feature (models/TPNet.py:127-128), every readout's last two operations, in its two steps ...
__device__ __forceinline__ float clamp_feature(float x) { return (x < 0.0f) ? 0.0f : x; }   // NaN < 0 is false: NaN passes through, as in the reference (TPNet.py:127)
__device__ __forceinline__ float log_feature(float x) { return logf(x + 1.0f); }            // log(x + 1), not log1p (TPNet.py:128)
// ... for one value ...
__device__ __forceinline__ float finish_feature(float x, bool do_scale) {
    return do_scale ? log_feature(clamp_feature(x)) : x;
}
// ... and for the two values of a two-output kernel, step by step as those kernels were tuned (the two logs overlap)
__device__ __forceinline__ void finish_features(float& x1, float& x2, bool do_scale) {
    if (do_scale) {
        x1 = clamp_feature(x1);
        x2 = clamp_feature(x2);
        x1 = log_feature(x1);
        x2 = log_feature(x2);
    }
}

// entry (i, j), i <= j, of a symmetric n x n matrix in its row-major upper triangle
constexpr __host__ __device__ int tri_slot(int n, int i, int j) { return i * n - (i * (i - 1)) / 2 + (j - i); }

// a node's table bundle (layers 1..L, L rows of d floats) in copy `copy`
__device__ __forceinline__ float* bundle_base(const tpnet_state& S, int copy, int64_t id, int L) {
    return S.q + ((int64_t)copy * S.N + id) * ((int64_t)L * S.d);
}

// the 1 + L rows of a node and the powers g^i of its pending decay: layer 0 (`row0`, never decays) and layers 1..L at `qb`
template <int L>
__device__ __forceinline__ void decay_rows(const float* row0, const float* qb, int d, float g, const float** rowp, float* rs) {
    rowp[0] = row0;
    rs[0] = 1.0f;
    float gi = 1.0f;
#pragma unroll
    for (int i = 1; i <= L; ++i) {
        gi *= g;
        rowp[i] = qb + (int64_t)(i - 1) * d;
        rs[i] = gi;
    }
}

// ... from the node's table bundle (k_wpipe's readout block, wstep.hip, calls decay_rows itself: its base is a windowed reference)
template <int L>
__device__ __forceinline__ void bundle_rows(const tpnet_state& S, int64_t id, int copy, float g, const float** rowp, float* rs) {
    decay_rows<L>(S.p0 + id * (int64_t)S.d, bundle_base(S, copy, id, L), S.d, g, rowp, rs);
}

// one chunk of the Gram of NN rows, already scaled by their decay: the upper-triangle sums.  (The scaling, `f[a][k] *= rs[a]` for
// rows a % NR != 0, stays in the two callers' chunk loops: written through a function -- tried with rs as pointer, array
// reference, __restrict__ and a local copy -- the !FULL kernels of readout.hip lose a wave, e.g. k_pair_gram<64,1,4,3,false>
// 152 -> 178 VGPRs, 3 -> 2 waves per SIMD, and <16,1,4,3,false>, <32,1,4,3,false>, <64,1,1,3,false> likewise.)
template <int NN, int F>
__device__ __forceinline__ void gram_accumulate(const float (&f)[NN][F], float* acc) {
#pragma unroll
    for (int a = 0; a < NN; ++a) {
#pragma unroll
        for (int b = a; b < NN; ++b) acc[a * NN + b] = acc[a * NN + b] + dot_chunk<F>(f[a], f[b]);
    }
}

// the tail of a one-pair readout: the lanes' partial sums acc[a * NN + b], a <= b, reduced over the group, finished and stored.
// PACKED (TPNET_FLAG_PACKED): only the NT distinct entries a <= b are written, raw, row-major upper triangle.
// `stage`: LDS, GramCfg::stage_floats per workgroup.  Three forms:
//   LDSRED           reduction through LDS (GramCfg::lds_reduce): park the NT distinct partials, sum row v, mirror into the output tile
//   Halve, LPP < 16  the narrow geometries: a lane ends up with 8 or 16 consecutive outputs, so a direct store touches one 64-byte
//                    line per lane and instruction; the values go through LDS instead and leave as whole lines (measured at d=16,
//                    B=8000: the store phase of a readout wave 5.6 -> 0.7 us)
//   Halve, direct    every lane streams its PER outputs out
// `dbg` is passed through for STAMP(3) (before the reduction) and STAMP(4) (behind it) of the -DTPNET_STAMPS build.
template <int LPP, int L, bool PACKED, bool LDSRED>
__device__ __forceinline__ void gram_finish(float* acc, bool valid, bool idok, bool do_scale, float* out, int gl, float* stage,
                                            unsigned long long* dbg = nullptr) {
    using C = GramCfg<LPP, L>;
    constexpr int NN = C::NN, NOUT = PACKED ? C::NT : C::NG;
    (void)dbg;
    if constexpr (LDSRED) {
        STAMP(3);
        constexpr int RS = C::RSTRIDE;
        float* red = stage + (threadIdx.x / LPP) * C::RED;
        float* so = red + C::NT * RS;
        {
            int tix = 0;
#pragma unroll
            for (int a = 0; a < NN; ++a) {
#pragma unroll
                for (int b = a; b < NN; ++b) {
                    red[tix * RS + gl] = acc[a * NN + b];
                    ++tix;
                }
            }
        }
        __builtin_amdgcn_wave_barrier();            // a group's lanes are in one wave: LDS executes in issue order
#pragma unroll
        for (int it = 0; it * LPP < C::NT; ++it) {
            const int v = it * LPP + gl;
            if (v < C::NT) {
                typedef float v4f __attribute__((ext_vector_type(4)));
                const v4f* row = reinterpret_cast<const v4f*>(red + v * RS);
                float sum = 0.0f;
#pragma unroll
                for (int l = 0; l < LPP / 4; ++l) {
                    const v4f q = row[l];
                    sum = (((sum + q.x) + q.y) + q.z) + q.w;
                }
                if constexpr (PACKED) {
                    so[v] = sum;
                } else {
                    int a = 0, off = 0;                          // v -> (a, b): row a of the upper triangle starts at off
#pragma unroll
                    for (int r = 1; r < NN; ++r) {
                        const int o = tri_slot(NN, r, r);
                        if (v >= o) { a = r; off = o; }
                    }
                    const int b = a + (v - off);
                    so[a * NN + b] = sum;
                    so[b * NN + a] = sum;
                }
            }
        }
        __builtin_amdgcn_wave_barrier();
        STAMP(4);
#pragma unroll
        for (int j = 0; j * LPP < NOUT; ++j) {                    // lane gl takes outputs gl, gl+LPP, ...: whole lines
            const int c = j * LPP + gl;
            if (valid && c < NOUT) {
                float x = finish_feature(so[c], do_scale && !PACKED);
                if (!idok) x = __builtin_nanf("");
                __builtin_nontemporal_store(x, out + c);
            }
        }
        __builtin_amdgcn_wave_barrier();            // the tiles are reused by the next pair of this group
    } else {
#pragma unroll
        for (int a = 1; a < NN; ++a) {
#pragma unroll
            for (int b = 0; b < a; ++b) acc[a * NN + b] = acc[b * NN + a];
        }
        STAMP(3);
        Halve<C::MP, LPP / 2>::run(acc, gl);
        STAMP(4);
        // lane gl holds elements idx = gl * PER + k of the full tile, finished -> this group's LDS row (STAGED; full or packed
        // layout) or straight out (features are consumed by another kernel: stream them out)
        constexpr bool STAGED = LPP < 16;
        float* sg = STAGED ? stage + (threadIdx.x / LPP) * C::NG : nullptr;
        if (STAGED || valid) {
#pragma unroll
            for (int k = 0; k < C::PER; ++k) {
                const int idx = gl * C::PER + k;
                if (idx < C::NG) {
                    float x = finish_feature(acc[k], do_scale && !PACKED);
                    if (!idok) x = __builtin_nanf("");
                    const int a = idx / NN, b = idx - a * NN;
                    const int slot = PACKED ? tri_slot(NN, a, b) : idx;
                    if (!PACKED || a <= b) {
                        if constexpr (STAGED) sg[slot] = x;
                        else __builtin_nontemporal_store(x, out + slot);
                    }
                }
            }
        }
        if constexpr (STAGED) {
            __builtin_amdgcn_wave_barrier();            // the group's lanes are in one wave: LDS executes in issue order
            if constexpr (NOUT % 4 == 0) {
#pragma unroll
                for (int j = 0; j * LPP < NOUT / 4; ++j) {
                    const int c = j * LPP + gl;
                    if (valid && c < NOUT / 4) {
                        typedef float v4f __attribute__((ext_vector_type(4)));   // rows are 16-byte aligned (checked by the launchers)
                        const v4f q = reinterpret_cast<const v4f*>(sg)[c];
                        __builtin_nontemporal_store(q, reinterpret_cast<v4f*>(out) + c);
                    }
                }
            } else {
#pragma unroll
                for (int j = 0; j * LPP < NOUT; ++j) {
                    const int c = j * LPP + gl;
                    if (valid && c < NOUT) __builtin_nontemporal_store(sg[c], out + c);
                }
            }
            __builtin_amdgcn_wave_barrier();            // the row is reused by the next pair of this group
        }
    }
}

// gram_finish's middle form (Halve, staged store) as text, for the instantiations that do not take it as a function: called through
// gram_finish, k_step<4,1,4,3,false,false,BS,FUSE> (step.hip, step256.hip, step256f.hip) goes from 140 to 152 bytes of scratch (320 ->
// 328 with FUSE) and k_wpipe<8,1,3,false,false,*> (wstep.hip) from 144 to 148, in every form of the call that was tried (acc as pointer
// or array reference, the group's row passed in, __restrict__, the two store loops merged or apart).  L = 3 only: rows of 64 or 36
// floats, always whole 16-byte vectors.  The triangle slot is written out: with tri_slot() the k_wpipe pair stays at 148.
#define TPNET_GRAM_FINISH_STAGED_L3()                                                                                          \
    do {                                                                                                                       \
        _Pragma("unroll") for (int a = 1; a < NN; ++a) {                                                                       \
            _Pragma("unroll") for (int b = 0; b < a; ++b) acc[a * NN + b] = acc[b * NN + a];                                   \
        }                                                                                                                      \
        STAMP(3);                                                                                                              \
        Halve<C::MP, LPP / 2>::run(acc, gl);                                                                                   \
        STAMP(4);                                                                                                              \
        constexpr int NOUT = PACKED ? C::NT : C::NG;                                                                           \
        static_assert(L == 3 && LPP < 16 && !LDSRED && NOUT % 4 == 0, "the staged tail of whole vectors");                     \
        float* sg = stage + (threadIdx.x / LPP) * C::NG;                                                                       \
        _Pragma("unroll") for (int k = 0; k < C::PER; ++k) {                                                                   \
            const int idx = gl * C::PER + k;                                                                                   \
            if (idx < C::NG) {                                                                                                 \
                float x = finish_feature(acc[k], do_scale && !PACKED);                                                         \
                if (!idok) x = __builtin_nanf("");                                                                             \
                if constexpr (PACKED) {                                                                                        \
                    const int a = idx / NN, b = idx - a * NN;                                                                  \
                    if (a <= b) sg[a * NN - (a * (a - 1)) / 2 + (b - a)] = x;                                                  \
                } else {                                                                                                       \
                    sg[idx] = x;                                                                                               \
                }                                                                                                              \
            }                                                                                                                  \
        }                                                                                                                      \
        __builtin_amdgcn_wave_barrier();                                                                                       \
        _Pragma("unroll") for (int j = 0; j * LPP < NOUT / 4; ++j) {                                                           \
            const int c = j * LPP + gl;                                                                                        \
            if (valid && c < NOUT / 4) {                                                                                       \
                typedef float v4f __attribute__((ext_vector_type(4)));                                                         \
                const v4f q = reinterpret_cast<const v4f*>(sg)[c];                                                             \
                __builtin_nontemporal_store(q, reinterpret_cast<v4f*>(out) + c);                                               \
            }                                                                                                                  \
        }                                                                                                                      \
        __builtin_amdgcn_wave_barrier();                                                                                       \
    } while (0)

// ---------------------------------------------------------------------------------------------------------------
// pairwise readout of ONE pair by one group of LPP lanes (models/TPNet.py:119-128); PACKED, `stage`: gram_finish
// ---------------------------------------------------------------------------------------------------------------
template <int LPP, int VPL, int W, int L, bool FULL, bool PACKED = false, bool FUSE = false, bool LDSRED = false>
__device__ __forceinline__ void gram_pair(const tpnet_state& S, int64_t u, int64_t v, bool valid, uint32_t bid,
                                          double now, double lambda, bool do_scale, float* __restrict__ out, int gl,
                                          unsigned long long* dbg = nullptr, float* __restrict__ stage = nullptr,
                                          uint32_t fuse = 0, float fuse_w = 0.0f, double t_last = 0.0) {
    // FUSE / fuse (bit 0: u, bit 1: v; only the fused step sets it, and only for an edge's (src,dst) pair): this group also
    // writes the new bundle of that endpoint -- it is the target's ONLY contribution in the batch (Plan::fuse_*), and
    // both operands, old[i][target] and P[i-1][partner], are among the rows loaded for the Gram:
    //   new[i][target] = old[i][target] * g_t^i + (P[i-1][partner] * g_p^(i-1)) * w,   g = decay to the batch's LAST time
    // (the same operations in the same order as update_item, so the result does not depend on which path ran)
    using C = GramCfg<LPP, L>;
    constexpr int NR = C::NR, NN = C::NN, F = VPL * W;
    const int d = S.d;
    const int nvec = d / W;
    const NodeMeta* meta = reinterpret_cast<const NodeMeta*>(S.meta);

    bool idok = valid && (uint64_t)u < (uint64_t)S.N && (uint64_t)v < (uint64_t)S.N;
    if (valid && !idok && gl == 0) atomicAdd(S.err, 1u);
    if (!idok) { u = 0; v = 0; }

    STAMP(1);
    const float* rowp[NN];
    float rs[NN];
    float gl_last[2] = {1.0f, 1.0f};     // decay of layer 1 to t_last (fused update only)
    int cur[2] = {0, 0};
    const int64_t ids[2] = {u, v};
    if (!FUSE || !idok) fuse = 0;
    // (the fused step's variant -- batches of thousands of edges, bound by memory: its layer-0 rows do not depend on the nodes' records,
    // so their loads go out WITH the records' instead of behind them: a quarter of a pair's bytes one round trip earlier)
    constexpr bool EARLY0 = FUSE && FULL;
    float f[NN][F];
    if constexpr (EARLY0) {
#pragma unroll
        for (int s = 0; s < 2; ++s) {
#pragma unroll
            for (int j = 0; j < VPL; ++j) ldv_maybe<W, true>(S.p0 + ids[s] * (int64_t)d, j * LPP + gl, true, &f[s * NR][j * W]);
        }
    }
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const uint4* mp = reinterpret_cast<const uint4*>(meta + ids[s]);
        const uint4 ma = mp[0], mb = mp[1];
        const MetaView m = meta_view(ma, mb, bid, now, lambda);
        if constexpr (FUSE) {
            if (fuse) gl_last[s] = meta_view(ma, mb, bid, t_last, lambda).g;
        }
        cur[s] = m.copy;
        bundle_rows<L>(S, ids[s], m.copy, m.g, rowp + s * NR, rs + s * NR);
    }

    float acc[C::MP];
#pragma unroll
    for (int i = 0; i < C::MP; ++i) acc[i] = 0.0f;
    STAMP(2);

    for (int c0 = 0; c0 < (FULL ? 1 : nvec); c0 += LPP * VPL) {
#pragma unroll
        for (int a = 0; a < NN; ++a) {
            if (EARLY0 && a % NR == 0) continue;
#pragma unroll
            for (int j = 0; j < VPL; ++j) {
                const int vi = c0 + j * LPP + gl;
                ldv_maybe<W, FULL>(rowp[a], vi, vi < nvec, &f[a][j * W]);
            }
        }
        if constexpr (FUSE) if (fuse) {
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                if (fuse & (1u << s)) {
                    // (not bundle_base: through it four FUSE kernels of step256f.hip gain scratch, k_step<16,1,4,4,false,false,256,true> 28 -> 44 bytes)
                    float* qnew = S.q + ((int64_t)(cur[s] ^ 1) * S.N + ids[s]) * ((int64_t)L * d);
                    float gt = 1.0f, gp = 1.0f;
#pragma unroll
                    for (int i = 1; i <= L; ++i) {
                        gt *= gl_last[s];                            // g_t^i
                        float nw[F];
#pragma unroll
                        for (int k = 0; k < F; ++k) {
                            const float m = (f[(1 - s) * NR + i - 1][k] * gp) * fuse_w;
                            nw[k] = f[s * NR + i][k] * gt + m;
                        }
                        gp *= gl_last[1 - s];                        // g_p^(i-1) for the next layer
#pragma unroll
                        for (int j = 0; j < VPL; ++j) {
                            const int vi = c0 + j * LPP + gl;
                            if (FULL || vi < nvec) stv<W>(qnew + (int64_t)(i - 1) * d, vi, &nw[j * W]);
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int a = 0; a < NN; ++a) {
            if (a % NR != 0) {
#pragma unroll
                for (int k = 0; k < F; ++k) f[a][k] *= rs[a];
            }
        }
        gram_accumulate<NN, F>(f, acc);
    }
    if constexpr (FUSE) if (fuse && gl == 0) {
        NodeMeta* wm = reinterpret_cast<NodeMeta*>(S.meta);
#pragma unroll
        for (int s = 0; s < 2; ++s)
            if (fuse & (1u << s)) publish_meta(wm + ids[s], cur[s] ^ 1, t_last, bid);
    }
    // (the macro is gram_finish's middle form as text and must track it; which geometry needs it: see the macro's comment)
    if constexpr (LPP == 4 && L == 3 && !FULL) TPNET_GRAM_FINISH_STAGED_L3();
    else gram_finish<LPP, L, PACKED, LDSRED>(acc, valid, idok, do_scale, out, gl, stage, dbg);
}


// ---------------------------------------------------------------------------------------------------------------
// pairwise readout of ONE pair whose 2(L+1) rows have already been located (windowed stream path, wstep.hip: a row
// version is either a table bundle or a slot of the window's version log): the Gram, its reduction over the group and
// the store, exactly as in gram_pair (same sums in the same order).
// ---------------------------------------------------------------------------------------------------------------
template <int LPP, int VPL, int W, int L, bool FULL, bool PACKED, bool LDSRED>
__device__ __forceinline__ void gram_rows(const float* const (&rowp)[2 * (L + 1)], const float (&rs)[2 * (L + 1)], int d,
                                          bool valid, bool idok, bool do_scale, float* __restrict__ out, int gl,
                                          float* __restrict__ stage) {
    using C = GramCfg<LPP, L>;
    constexpr int NR = C::NR, NN = C::NN, F = VPL * W;
    const int nvec = d / W;
    float acc[C::MP];
#pragma unroll
    for (int i = 0; i < C::MP; ++i) acc[i] = 0.0f;
    for (int c0 = 0; c0 < (FULL ? 1 : nvec); c0 += LPP * VPL) {
        float f[NN][F];
#pragma unroll
        for (int a = 0; a < NN; ++a) {
#pragma unroll
            for (int j = 0; j < VPL; ++j) {
                const int vi = c0 + j * LPP + gl;
                ldv_maybe<W, FULL>(rowp[a], vi, vi < nvec, &f[a][j * W]);
            }
        }
#pragma unroll
        for (int a = 0; a < NN; ++a) {
            if (a % NR != 0) {
#pragma unroll
                for (int k = 0; k < F; ++k) f[a][k] *= rs[a];
            }
        }
        gram_accumulate<NN, F>(f, acc);
    }
    // (the macro is gram_finish's middle form as text and must track it; here it is k_wpipe's 8-lane kernels that need it)
    if constexpr (LPP == 8 && L == 3 && !FULL) {
        unsigned long long* dbg = nullptr;          // (STAMP's name: the windowed readout carries no stamps)
        (void)dbg;
        TPNET_GRAM_FINISH_STAGED_L3();
    } else {
        gram_finish<LPP, L, PACKED, LDSRED>(acc, valid, idok, do_scale, out, gl, stage);
    }
}
#undef TPNET_GRAM_FINISH_STAGED_L3


// ---------------------------------------------------------------------------------------------------------------
// Two outputs per unit: G(first, second1) and G(first, second2) with the first node's rows loaded once.  Only the distinct
// inner products are formed and reduced, in ONE recursive-halving pass for both outputs:
//   slots = [ f.f (tri) | f.s1 (R*R) | f.s2 (R*R) | s1.s1 (tri) | s2.s2 (tri) ],  R = L+1, tri = R(R+1)/2
// OWN2 = false leaves out the second nodes' own blocks (the anchored walk forms them once per row, not per unit).
// Afterwards every lane picks the (at most two per output) slots its output elements mirror from by shuffles.
// ---------------------------------------------------------------------------------------------------------------
template <int LPP, int L, bool OWN2>
struct TwoOutCfg {
    static constexpr int R = L + 1;
    static constexpr int TRI = R * (R + 1) / 2;
    static constexpr bool OWN = OWN2;
    static constexpr int O_FF = 0, O_FS1 = TRI, O_FS2 = TRI + R * R, O_S1 = TRI + 2 * R * R, O_S2 = 2 * TRI + 2 * R * R;
    static constexpr int NS = (OWN2 ? 3 : 1) * TRI + 2 * R * R;
    static constexpr int MPS = ((NS + LPP - 1) / LPP) * LPP;
    static constexpr int PERS = MPS / LPP;
    static constexpr __host__ __device__ int tri(int i, int j) { return tri_slot(R, i, j); }   // i <= j
};
template <int LPP, int L> using SharedCfg = TwoOutCfg<LPP, L, true>;     // 62 slots at L = 3
template <int LPP, int L> using AnchorCfg = TwoOutCfg<LPP, L, false>;    // 42 slots at L = 3

// output element idx = a*NN + b of the two Gram matrices [first rows | second rows]^2 -> the slots s1, s2 it comes from.
// Returns true for an element of the second nodes' own blocks, entry `ta` of their triangles (OWN: s = O_S1/O_S2 + ta)
template <class TC>
__device__ __forceinline__ bool out_slots(int idx, int& s1, int& s2, int& ta) {
    constexpr int NR = TC::R, NN = 2 * NR;
    const int a = idx / NN, b = idx - a * NN;
    ta = 0;
    if (a < NR && b < NR) {
        const int i = a < b ? a : b, j = a < b ? b : a;
        s1 = s2 = TC::O_FF + TC::tri(i, j);
    } else if (a < NR) {                       // (first row a, second row b-NR)
        s1 = TC::O_FS1 + a * NR + (b - NR);
        s2 = TC::O_FS2 + a * NR + (b - NR);
    } else if (b < NR) {                       // mirrored
        s1 = TC::O_FS1 + b * NR + (a - NR);
        s2 = TC::O_FS2 + b * NR + (a - NR);
    } else {
        const int x = a - NR, y = b - NR;
        ta = TC::tri(x < y ? x : y, x < y ? y : x);
        s1 = TC::OWN ? TC::O_S1 + ta : 0;
        s2 = TC::OWN ? TC::O_S2 + ta : 0;
        return true;
    }
    return false;
}

// slots s1 and s2 of the reduced sums (lane l holds slots [l * PERS, (l + 1) * PERS) in acc) by shuffles, the two picks in one loop
template <int PERS, int LPP>
__device__ __forceinline__ void pick_slots(const float* acc, int s1, int s2, float& x1, float& x2) {
    x1 = 0.0f;
    x2 = 0.0f;
#pragma unroll
    for (int j = 0; j < PERS; ++j) {
        const float t1 = __shfl(acc[j], s1 / PERS, LPP);
        const float t2 = __shfl(acc[j], s2 / PERS, LPP);
        x1 = (s1 % PERS == j) ? t1 : x1;
        x2 = (s2 % PERS == j) ? t2 : x2;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// pairwise readout of TWO pairs that share their first node: out1 = G(u, v1), out2 = G(u, v2).  u's rows are loaded
// once.  This is the shape of both callers of the readout: the decoder's (src,dst) / (src,neg) pairs
// (models/modules.py:112, train_link_prediction.py:359-368) and the encoder's relative encodings, where every
// neighbour w is paired with the edge's src AND dst (models/TPNet.py:311-316: first half of the pair list =
// G(w, src), second half = G(w, dst)).  SharedCfg: 62 slots at L = 3 (one 64-value reduction instead of two, 62 dot
// products instead of 72, 12 row loads instead of 16)
// ---------------------------------------------------------------------------------------------------------------
template <int LPP, int VPL, int W, int L, bool FULL>
__device__ __forceinline__ void gram_shared(const tpnet_state& S, int64_t u, int64_t v1, int64_t v2, bool valid,
                                            uint32_t bid, double now, double lambda, bool do_scale,
                                            float* __restrict__ out1, float* __restrict__ out2, int gl) {
    using C = GramCfg<LPP, L>;
    using SC = SharedCfg<LPP, L>;
    constexpr int NR = C::NR, F = VPL * W;
    const int d = S.d;
    const int nvec = d / W;
    const NodeMeta* meta = reinterpret_cast<const NodeMeta*>(S.meta);

    bool idok = valid && (uint64_t)u < (uint64_t)S.N && (uint64_t)v1 < (uint64_t)S.N && (uint64_t)v2 < (uint64_t)S.N;
    if (valid && !idok && gl == 0) atomicAdd(S.err, 1u);
    if (!idok) { u = 0; v1 = 0; v2 = 0; }

    const float* rowp[3][NR];
    float rs[3][NR];
    {
        const int64_t ids[3] = {u, v1, v2};
#pragma unroll
        for (int s = 0; s < 3; ++s) {
            const MetaView m = read_meta(meta, ids[s], bid, now, lambda);
            bundle_rows<L>(S, ids[s], m.copy, m.g, rowp[s], rs[s]);
        }
    }
    float acc[SC::MPS];
#pragma unroll
    for (int i = 0; i < SC::MPS; ++i) acc[i] = 0.0f;

    for (int c0 = 0; c0 < (FULL ? 1 : nvec); c0 += LPP * VPL) {
        float f[3][NR][F];
#pragma unroll
        for (int s = 0; s < 3; ++s) {
#pragma unroll
            for (int a = 0; a < NR; ++a) {
#pragma unroll
                for (int j = 0; j < VPL; ++j) {
                    const int vi = c0 + j * LPP + gl;
                    ldv_maybe<W, FULL>(rowp[s][a], vi, vi < nvec, &f[s][a][j * W]);
                }
            }
        }
#pragma unroll
        for (int s = 0; s < 3; ++s) {
#pragma unroll
            for (int a = 1; a < NR; ++a) {
#pragma unroll
                for (int k = 0; k < F; ++k) f[s][a][k] *= rs[s][a];
            }
        }
#pragma unroll
        for (int a = 0; a < NR; ++a) {
#pragma unroll
            for (int b = a; b < NR; ++b) {
                acc[SC::O_FF + SC::tri(a, b)] = acc[SC::O_FF + SC::tri(a, b)] + dot_chunk<F, false>(f[0][a], f[0][b]);
                acc[SC::O_S1 + SC::tri(a, b)] = acc[SC::O_S1 + SC::tri(a, b)] + dot_chunk<F, false>(f[1][a], f[1][b]);
                acc[SC::O_S2 + SC::tri(a, b)] = acc[SC::O_S2 + SC::tri(a, b)] + dot_chunk<F, false>(f[2][a], f[2][b]);
            }
#pragma unroll
            for (int b = 0; b < NR; ++b) {
                acc[SC::O_FS1 + a * NR + b] = acc[SC::O_FS1 + a * NR + b] + dot_chunk<F, false>(f[0][a], f[1][b]);
                acc[SC::O_FS2 + a * NR + b] = acc[SC::O_FS2 + a * NR + b] + dot_chunk<F, false>(f[0][a], f[2][b]);
            }
        }
    }
    // (a reduction through LDS like gram_pair's was measured here: 62 slots x (LPP+4) floats per unit cost the kernel its
    // occupancy -- 800 000 units at d=256: 348 -> 414 us)
    Halve<SC::MPS, LPP / 2>::run(acc, gl);        // lane gl now holds the complete sums of slots [gl*PERS, ...)

#pragma unroll
    for (int k = 0; k < C::PER; ++k) {
        int idx = gl * C::PER + k;
        const bool in = idx < C::NG;
        idx = in ? idx : 0;
        // (out_slots' map as text: through the function the slot arithmetic of every element compiles to other code, and the readout of
        // 80 000 pairs at d = 128 takes 30.6 us instead of 29.1 on the MI355X; must track out_slots)
        constexpr int NN = C::NN;
        const int a = idx / NN, b = idx - a * NN;
        int s1, s2;
        if (a < NR && b < NR) {
            const int i = a < b ? a : b, j = a < b ? b : a;
            s1 = s2 = SC::O_FF + SC::tri(i, j);
        } else if (a < NR) {                       // (u row a, v row b-NR)
            s1 = SC::O_FS1 + a * NR + (b - NR);
            s2 = SC::O_FS2 + a * NR + (b - NR);
        } else if (b < NR) {                       // mirrored
            s1 = SC::O_FS1 + b * NR + (a - NR);
            s2 = SC::O_FS2 + b * NR + (a - NR);
        } else {
            const int x = a - NR, y = b - NR;
            const int i = x < y ? x : y, j = x < y ? y : x;
            s1 = SC::O_S1 + SC::tri(i, j);
            s2 = SC::O_S2 + SC::tri(i, j);
        }
        float x1, x2;
        pick_slots<SC::PERS, LPP>(acc, s1, s2, x1, x2);
        finish_features(x1, x2, do_scale);
        if (!idok) { x1 = __builtin_nanf(""); x2 = x1; }
        if (valid && in) {
            out1[idx] = x1;
            out2[idx] = x2;
        }
    }
}


// ---------------------------------------------------------------------------------------------------------------
// The encoder's readout (models/TPNet.py:311-324): row i of the call has TWO anchors (the edge's src and dst) and K
// sampled neighbours w_0..w_{K-1}; the pair list is [G(w_k, src_i) for all i, k] followed by [G(w_k, dst_i)].  ONE lane
// group walks a row: the anchors' 2(L+1) rows are loaded once and stay in registers for all K neighbours, their own
// blocks <a,a> are reduced once per row, and per neighbour only its L+1 rows are fetched (instead of 3(L+1) per
// (w, src, dst) unit) and only the neighbour's blocks are formed and reduced (AnchorCfg: first = w, second = the anchors;
// 42 slots at L = 3 against 62).
// The walk in pieces: anchor_rows + anchor_output_plan = the anchors of a unit, neighbour_fetch + neighbour_issue(0) = ids
// and meta records of up to LPP neighbours and the first one's rows, neighbour_step(j) = neighbour j's 42 inner products,
// reduced and finished (clamp, log).  One chunk per row (d <= LPP * VPL * W); !FULL: lanes whose vector lies past the row's
// end hold zeros.
// ---------------------------------------------------------------------------------------------------------------
// all-reduce of one value over the LPP lanes of a group (butterfly; used once per row for the anchors' own blocks)
template <int LPP>
__device__ __forceinline__ float group_allreduce(float v) {
#pragma unroll
    for (int o = LPP / 2; o >= 1; o >>= 1) v += __shfl_xor(v, o, LPP);
    return v;
}

// the L + 1 rows of node w (bundle copy cp), raw, one chunk
template <int LPP, int VPL, int W, int L, bool FULL>
__device__ __forceinline__ void load_node_rows(const tpnet_state& S, int64_t w, int cp, int gl, float (&fr)[L + 1][VPL * W]) {
    const int d = S.d;
    const int nvec = d / W;
    const float* qb = bundle_base(S, cp, w, L);
#pragma unroll
    for (int jj = 0; jj < VPL; ++jj)
        ldv_maybe<W, FULL>(S.p0 + w * (int64_t)d, jj * LPP + gl, jj * LPP + gl < nvec, &fr[0][jj * W]);
#pragma unroll
    for (int i = 1; i <= L; ++i) {
#pragma unroll
        for (int jj = 0; jj < VPL; ++jj)
            ldv_maybe<W, FULL>(qb + (int64_t)(i - 1) * d, jj * LPP + gl, jj * LPP + gl < nvec, &fr[i][jj * W]);
    }
}

// the anchors of a unit: their rows fa (decay applied) and their own blocks aa, once per row.  Returns whether both ids are in range
template <int LPP, int VPL, int W, int L, bool FULL>
__device__ __forceinline__ bool anchor_rows(const tpnet_state& S, int64_t a1, int64_t a2, bool valid, double now, double lambda,
                                            int gl, float (&fa)[2][L + 1][VPL * W], float (&aa)[2][(L + 1) * (L + 2) / 2]) {
    constexpr int NR = L + 1, F = VPL * W;
    const NodeMeta* meta = reinterpret_cast<const NodeMeta*>(S.meta);
    const bool aok = valid && (uint64_t)a1 < (uint64_t)S.N && (uint64_t)a2 < (uint64_t)S.N;
    if (valid && !aok && gl == 0) atomicAdd(S.err, 1u);
    if (!aok) { a1 = 0; a2 = 0; }
    const int64_t ids[2] = {a1, a2};
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const MetaView m = read_meta(meta, ids[s], READER_BID, now, lambda);
        load_node_rows<LPP, VPL, W, L, FULL>(S, ids[s], m.copy, gl, fa[s]);
        float g = 1.0f;
#pragma unroll
        for (int i = 1; i <= L; ++i) {
            g *= m.g;
#pragma unroll
            for (int k = 0; k < F; ++k) fa[s][i][k] *= g;
        }
    }
#pragma unroll
    for (int s = 0; s < 2; ++s) {
#pragma unroll
        for (int a = 0; a < NR; ++a) {
#pragma unroll
            for (int b = a; b < NR; ++b) aa[s][tri_slot(NR, a, b)] = group_allreduce<LPP>(dot_chunk<F, false>(fa[s][a], fa[s][b]));
        }
    }
    return aok;
}

// per-lane output plan (invariant over the unit): where each of this lane's PER output elements comes from -- a slot of the
// neighbour's sums, or the anchors' own block, finished (clamp, log) once per unit
template <int PER>
struct AnchorPlan {
    int s1[PER], s2[PER];
    bool own[PER], in[PER];
    float y1[PER], y2[PER];
};

template <int LPP, int L>
__device__ __forceinline__ void anchor_output_plan(const float (&aa)[2][(L + 1) * (L + 2) / 2], bool do_scale, int gl,
                                                   AnchorPlan<GramCfg<LPP, L>::PER>& p) {
    using C = GramCfg<LPP, L>;
    using AC = AnchorCfg<LPP, L>;
#pragma unroll
    for (int kk = 0; kk < C::PER; ++kk) {
        int idx = gl * C::PER + kk;
        p.in[kk] = idx < C::NG;
        idx = p.in[kk] ? idx : 0;
        int ta;
        p.own[kk] = out_slots<AC>(idx, p.s1[kk], p.s2[kk], ta);
        p.y1[kk] = 0.0f;
        p.y2[kk] = 0.0f;
        if (p.own[kk]) {
            float y1 = 0.0f, y2 = 0.0f;
#pragma unroll
            for (int q = 0; q < AC::TRI; ++q) {     // (register arrays: a select chain, no dynamic indexing)
                y1 = (ta == q) ? aa[0][q] : y1;
                y2 = (ta == q) ? aa[1][q] : y2;
            }
            finish_features(y1, y2, do_scale);
            p.y1[kk] = y1;
            p.y2[kk] = y2;
        }
    }
}

// ids and meta records of the neighbours w[0 .. nk) (nk <= LPP), fetched lane-parallel: two round trips for all of them
template <int LPP>
__device__ __forceinline__ void neighbour_fetch(const tpnet_state& S, const int64_t* __restrict__ w, int nk, bool valid, bool aok,
                                                double now, double lambda, int gl, int64_t& my_w, bool& my_ok, MetaView& my_m) {
    const NodeMeta* meta = reinterpret_cast<const NodeMeta*>(S.meta);
    my_w = (valid && gl < nk) ? w[gl] : 0;
    my_ok = aok && (uint64_t)my_w < (uint64_t)S.N;
    if (valid && aok && gl < nk && !my_ok) atomicAdd(S.err, 1u);
    if (!my_ok) my_w = 0;
    my_m = read_meta(meta, my_w, READER_BID, now, lambda);
}

// the rows of neighbour j of the fetch -> fn (in flight while the neighbour before it is worked on)
template <int LPP, int VPL, int W, int L, bool FULL>
__device__ __forceinline__ void neighbour_issue(const tpnet_state& S, int64_t my_w, const MetaView& my_m, int j, int gl,
                                                float (&fn)[L + 1][VPL * W]) {
    const int64_t w = __shfl(my_w, j, LPP);
    const int cp = __shfl(my_m.copy, j, LPP);
    load_node_rows<LPP, VPL, W, L, FULL>(S, w, cp, gl, fn);
}

// a neighbour's 42 inner products (its rows fw against themselves and against the anchors' fa), reduced over the group
template <int LPP, int L, int F>
__device__ __forceinline__ void neighbour_sums(const float (&fw)[L + 1][F], const float (&fa)[2][L + 1][F], int gl,
                                               float (&acc)[AnchorCfg<LPP, L>::MPS]) {
    using AC = AnchorCfg<LPP, L>;
    constexpr int NR = L + 1;
#pragma unroll
    for (int i = 0; i < AC::MPS; ++i) acc[i] = 0.0f;
#pragma unroll
    for (int a = 0; a < NR; ++a) {
#pragma unroll
        for (int b = a; b < NR; ++b) acc[AC::O_FF + AC::tri(a, b)] = dot_chunk<F, false>(fw[a], fw[b]);
#pragma unroll
        for (int b = 0; b < NR; ++b) {
            acc[AC::O_FS1 + a * NR + b] = dot_chunk<F, false>(fw[a], fa[0][b]);
            acc[AC::O_FS2 + a * NR + b] = dot_chunk<F, false>(fw[a], fa[1][b]);
        }
    }
    Halve<AC::MPS, LPP / 2>::run(acc, gl);        // lane gl now holds the complete sums of slots [gl*PERS, ...)
}

// neighbour j of the fetch (its rows in fn; `more`: issue neighbour j + 1 behind it), reduced and finished (clamp, log):
// emit(idx, x1, x2) for each of this lane's elements idx = gl * PER + kk (< NG) of the two feature rows G(w, a1), G(w, a2)
template <int LPP, int VPL, int W, int L, bool FULL, class Emit>
__device__ __forceinline__ void neighbour_step(const tpnet_state& S, int j, bool more, bool do_scale, int gl,
                                               const float (&fa)[2][L + 1][VPL * W], float (&fn)[L + 1][VPL * W], int64_t my_w,
                                               bool my_ok, const MetaView& my_m, const AnchorPlan<GramCfg<LPP, L>::PER>& p,
                                               Emit&& emit) {
    using C = GramCfg<LPP, L>;
    using AC = AnchorCfg<LPP, L>;
    constexpr int F = VPL * W;
    const bool wok = __shfl((int)my_ok, j, LPP) != 0;
    const float mg = __shfl(my_m.g, j, LPP);
    float fw[L + 1][F];                                // the neighbour's rows, decay applied
#pragma unroll
    for (int x = 0; x < F; ++x) fw[0][x] = fn[0][x];
    float g = 1.0f;
#pragma unroll
    for (int i = 1; i <= L; ++i) {
        g *= mg;
#pragma unroll
        for (int x = 0; x < F; ++x) fw[i][x] = fn[i][x] * g;
    }
    if (more) neighbour_issue<LPP, VPL, W, L, FULL>(S, my_w, my_m, j + 1, gl, fn);
    float acc[AC::MPS];
    neighbour_sums<LPP, L, F>(fw, fa, gl, acc);
    // output elements of the two Gram matrices [w rows | anchor rows]^2 from their slots (or the anchors' block)
#pragma unroll
    for (int kk = 0; kk < C::PER; ++kk) {
        const int idx = p.in[kk] ? gl * C::PER + kk : 0;
        float x1, x2;
        pick_slots<AC::PERS, LPP>(acc, p.s1[kk], p.s2[kk], x1, x2);
        finish_features(x1, x2, do_scale);
        if (p.own[kk]) { x1 = p.y1[kk]; x2 = p.y2[kk]; }
        if (!wok) { x1 = __builtin_nanf(""); x2 = x1; }
        if (p.in[kk]) emit(idx, x1, x2);
    }
}

// one lane group walks the neighbours [k_begin, k_end) of a row.  Software pipeline: ids and meta records of up to LPP
// neighbours are fetched lane-parallel (two round trips for the whole chunk), and the rows of neighbour k+1 are in flight
// while neighbour k's 42 inner products are formed and reduced.  The loop body is neighbour_step's text with the stores in
// place of emit: called through neighbour_step, k_pair_gram_anchored at 16 lanes x 1 vector, L = 3 goes from 166 to 174 VGPRs
// (three waves per SIMD -> two; the limit is 168) and at 32 lanes x 2 vectors, L = 2 from 167 to 172.  It is the decay of the
// neighbour's rows (166 -> 169) and the output loop (166 -> 174) that do it when they are called as functions;
// neighbour_sums, neighbour_issue, pick_slots and finish_features are shared (166 -> 168), and that kernel is not to lose its wave.
template <int LPP, int VPL, int W, int L, bool FULL>
__device__ __forceinline__ void gram_anchored(const tpnet_state& S, const int64_t* __restrict__ neigh, int64_t a1, int64_t a2,
                                              int k_begin, int k_end, bool valid, double now, double lambda, bool do_scale,
                                              float* __restrict__ out1, float* __restrict__ out2, int gl) {
    using C = GramCfg<LPP, L>;
    using AC = AnchorCfg<LPP, L>;
    constexpr int NR = C::NR, F = VPL * W;
    float fa[2][NR][F];
    float aa[2][AC::TRI];
    const bool aok = anchor_rows<LPP, VPL, W, L, FULL>(S, a1, a2, valid, now, lambda, gl, fa, aa);
    AnchorPlan<C::PER> plan;
    anchor_output_plan<LPP, L>(aa, do_scale, gl, plan);
    for (int kc = k_begin; kc < k_end; kc += LPP) {
        const int nk = (k_end - kc < LPP) ? k_end - kc : LPP;
        int64_t my_w;
        bool my_ok;
        MetaView my_m;
        neighbour_fetch<LPP>(S, neigh + kc, nk, valid, aok, now, lambda, gl, my_w, my_ok, my_m);
        float fn[NR][F];                                   // rows of the NEXT neighbour (raw)
        neighbour_issue<LPP, VPL, W, L, FULL>(S, my_w, my_m, 0, gl, fn);
        for (int j = 0; j < nk; ++j) {
            const int k = kc + j;
            const bool wok = __shfl((int)my_ok, j, LPP) != 0;
            const float mg = __shfl(my_m.g, j, LPP);
            float fw[NR][F];
#pragma unroll
            for (int x = 0; x < F; ++x) fw[0][x] = fn[0][x];
            float g = 1.0f;
#pragma unroll
            for (int i = 1; i <= L; ++i) {
                g *= mg;
#pragma unroll
                for (int x = 0; x < F; ++x) fw[i][x] = fn[i][x] * g;
            }
            if (j + 1 < nk) neighbour_issue<LPP, VPL, W, L, FULL>(S, my_w, my_m, j + 1, gl, fn);
            float acc[AC::MPS];
            neighbour_sums<LPP, L, F>(fw, fa, gl, acc);
#pragma unroll
            for (int kk = 0; kk < C::PER; ++kk) {
                const int idx = plan.in[kk] ? gl * C::PER + kk : 0;
                float x1, x2;
                pick_slots<AC::PERS, LPP>(acc, plan.s1[kk], plan.s2[kk], x1, x2);
                finish_features(x1, x2, do_scale);
                if (plan.own[kk]) { x1 = plan.y1[kk]; x2 = plan.y2[kk]; }
                if (!wok) { x1 = __builtin_nanf(""); x2 = x1; }
                if (valid && plan.in[kk]) {
                    __builtin_nontemporal_store(x1, out1 + (int64_t)k * C::NG + idx);
                    __builtin_nontemporal_store(x2, out2 + (int64_t)k * C::NG + idx);
                }
            }
        }
    }
}


// ---------------------------------------------------------------------------------------------------------------
// One source against a list of candidates (the ranking protocol: a positive edge's source scored against C destinations):
// out[k] = G(src, cand[k]) with the SOURCE's rows first -- rows stacked [src 0..L ; cand 0..L], the decoder's order
// (models/modules.py:112), i.e. tpnet_pair_gram(repeat(src, C), cand).  The mirror image of the anchored walk with ONE anchor:
// the source's L+1 rows are fetched and decayed once per unit and stay in registers, its own block is reduced once per unit,
// and per candidate only the candidate's L+1 rows are loaded and only its (L+1)^2 cross products and (L+1)(L+2)/2 self products
// are formed and reduced (FanCfg: 26 slots at L = 3 against the anchored walk's 42).  The candidate side is the anchored walk's:
// neighbour_fetch (ids and meta records lane-parallel), neighbour_issue (candidate k+1's rows in flight while k is reduced).
// A pair's sums depend on its two nodes' rows alone -- never on the unit, the chunk or the position in the list.
// ---------------------------------------------------------------------------------------------------------------
template <int LPP, int L>
struct FanCfg {
    static constexpr int R = L + 1;
    static constexpr int TRI = R * (R + 1) / 2;
    static constexpr int O_CC = 0, O_SC = TRI;               // slots = [ c.c (tri) | s.c (R*R, source row major) ]
    static constexpr int NS = TRI + R * R;
    static constexpr int MPS = ((NS + LPP - 1) / LPP) * LPP;
    static constexpr int PERS = MPS / LPP;
    static constexpr __host__ __device__ int tri(int i, int j) { return tri_slot(R, i, j); }   // i <= j
};

// slot s of the reduced sums (lane l holds slots [l * PERS, (l + 1) * PERS) in acc) by shuffles
template <int PERS, int LPP>
__device__ __forceinline__ float pick_slot(const float* acc, int s) {
    float x = 0.0f;
#pragma unroll
    for (int j = 0; j < PERS; ++j) {
        const float t = __shfl(acc[j], s / PERS, LPP);
        x = (s % PERS == j) ? t : x;
    }
    return x;
}

template <int LPP, int VPL, int W, int L, bool FULL>
__device__ __forceinline__ void gram_fanout(const tpnet_state& S, const int64_t* __restrict__ cand, int64_t u, int k_begin,
                                            int k_end, bool valid, double now, double lambda, bool do_scale,
                                            float* __restrict__ out, int gl) {
    using C = GramCfg<LPP, L>;
    using FC = FanCfg<LPP, L>;
    constexpr int NR = C::NR, NN = C::NN, F = VPL * W;
    const NodeMeta* meta = reinterpret_cast<const NodeMeta*>(S.meta);
    const bool sok = valid && (uint64_t)u < (uint64_t)S.N;
    if (valid && !sok && gl == 0) atomicAdd(S.err, 1u);
    if (!sok) u = 0;
    // the source: rows (decay applied) and own block, once per unit
    float fs[NR][F];
    {
        const MetaView m = read_meta(meta, u, READER_BID, now, lambda);
        load_node_rows<LPP, VPL, W, L, FULL>(S, u, m.copy, gl, fs);
        float g = 1.0f;
#pragma unroll
        for (int i = 1; i <= L; ++i) {
            g *= m.g;
#pragma unroll
            for (int k = 0; k < F; ++k) fs[i][k] *= g;
        }
    }
    // per-lane output plan (invariant over the unit): element idx = a * NN + b of [src rows | cand rows]^2 comes from the
    // source's own block (finished once, here) or from slot sl of the candidate's sums
    int sl[C::PER];
    bool own[C::PER], in[C::PER];
    float ys[C::PER];
    {
        float ss[FC::TRI];
#pragma unroll
        for (int a = 0; a < NR; ++a) {
#pragma unroll
            for (int b = a; b < NR; ++b) ss[FC::tri(a, b)] = group_allreduce<LPP>(dot_chunk<F, false>(fs[a], fs[b]));
        }
#pragma unroll
        for (int kk = 0; kk < C::PER; ++kk) {
            int idx = gl * C::PER + kk;
            in[kk] = idx < C::NG;
            idx = in[kk] ? idx : 0;
            const int a = idx / NN, b = idx - a * NN;
            own[kk] = a < NR && b < NR;
            ys[kk] = 0.0f;
            if (own[kk]) {
                const int ta = FC::tri(a < b ? a : b, a < b ? b : a);
                float y = 0.0f;
#pragma unroll
                for (int q = 0; q < FC::TRI; ++q) y = (ta == q) ? ss[q] : y;     // (register array: a select chain)
                ys[kk] = finish_feature(y, do_scale);
                sl[kk] = 0;
            } else if (a < NR) {                       // (source row a, candidate row b - NR)
                sl[kk] = FC::O_SC + a * NR + (b - NR);
            } else if (b < NR) {                       // mirrored
                sl[kk] = FC::O_SC + b * NR + (a - NR);
            } else {
                const int x = a - NR, y = b - NR;
                sl[kk] = FC::O_CC + FC::tri(x < y ? x : y, x < y ? y : x);
            }
        }
    }
    for (int kc = k_begin; kc < k_end; kc += LPP) {
        const int nk = (k_end - kc < LPP) ? k_end - kc : LPP;
        int64_t my_w;
        bool my_ok;
        MetaView my_m;
        neighbour_fetch<LPP>(S, cand + kc, nk, valid, sok, now, lambda, gl, my_w, my_ok, my_m);
        float fn[NR][F];                                   // rows of the NEXT candidate (raw)
        neighbour_issue<LPP, VPL, W, L, FULL>(S, my_w, my_m, 0, gl, fn);
        for (int j = 0; j < nk; ++j) {
            const int k = kc + j;
            const bool wok = __shfl((int)my_ok, j, LPP) != 0;
            const float mg = __shfl(my_m.g, j, LPP);
            float fw[NR][F];                               // the candidate's rows, decay applied
#pragma unroll
            for (int x = 0; x < F; ++x) fw[0][x] = fn[0][x];
            float g = 1.0f;
#pragma unroll
            for (int i = 1; i <= L; ++i) {
                g *= mg;
#pragma unroll
                for (int x = 0; x < F; ++x) fw[i][x] = fn[i][x] * g;
            }
            if (j + 1 < nk) neighbour_issue<LPP, VPL, W, L, FULL>(S, my_w, my_m, j + 1, gl, fn);
            float acc[FC::MPS];
#pragma unroll
            for (int i = 0; i < FC::MPS; ++i) acc[i] = 0.0f;
#pragma unroll
            for (int a = 0; a < NR; ++a) {
#pragma unroll
                for (int b = a; b < NR; ++b) acc[FC::O_CC + FC::tri(a, b)] = dot_chunk<F, false>(fw[a], fw[b]);
#pragma unroll
                for (int b = 0; b < NR; ++b) acc[FC::O_SC + a * NR + b] = dot_chunk<F, false>(fs[a], fw[b]);
            }
            Halve<FC::MPS, LPP / 2>::run(acc, gl);         // lane gl now holds the complete sums of slots [gl*PERS, ...)
#pragma unroll
            for (int kk = 0; kk < C::PER; ++kk) {
                const int idx = in[kk] ? gl * C::PER + kk : 0;
                float x = finish_feature(pick_slot<FC::PERS, LPP>(acc, sl[kk]), do_scale);
                if (own[kk]) x = ys[kk];
                if (!wok) x = __builtin_nanf("");
                if (valid && in[kk]) __builtin_nontemporal_store(x, out + (int64_t)k * C::NG + idx);
            }
        }
    }
}


// the walk's arrays for a kernel that steps all the lane groups of a workgroup through their units TOGETHER
// (k_anchored_feature, anchored_feature.hip): begin() = anchor_rows + anchor_output_plan, fetch() + issue(0), step(j) = neighbour_step.
// The same operations in the same order as gram_anchored (whose loop body is neighbour_step's text): the features of the two are
// the same bits (tests/test_encoder_wide.py compares them with torch.equal).
template <int LPP, int VPL, int W, int L, bool FULL>
struct AnchorWalk {
    using C = GramCfg<LPP, L>;
    static constexpr int NR = C::NR, F = VPL * W, PER = C::PER;
    float fa[2][NR][F];                      // the anchors' rows, decay applied
    AnchorPlan<PER> plan;
    bool aok;
    int64_t my_w;                            // lane gl: neighbour kc + gl of the current fetch
    bool my_ok;
    MetaView my_m;
    float fn[NR][F];                         // rows of the NEXT neighbour (raw)

    __device__ __forceinline__ void begin(const tpnet_state& S, int64_t a1, int64_t a2, bool valid, double now, double lambda,
                                          bool do_scale, int gl) {
        float aa[2][AnchorCfg<LPP, L>::TRI];
        aok = anchor_rows<LPP, VPL, W, L, FULL>(S, a1, a2, valid, now, lambda, gl, fa, aa);
        anchor_output_plan<LPP, L>(aa, do_scale, gl, plan);
    }
    __device__ __forceinline__ void fetch(const tpnet_state& S, const int64_t* __restrict__ w, int nk, bool valid, double now,
                                          double lambda, int gl) {
        neighbour_fetch<LPP>(S, w, nk, valid, aok, now, lambda, gl, my_w, my_ok, my_m);
    }
    __device__ __forceinline__ void issue(const tpnet_state& S, int j, int gl) {
        neighbour_issue<LPP, VPL, W, L, FULL>(S, my_w, my_m, j, gl, fn);
    }
    template <class Emit>
    __device__ __forceinline__ void step(const tpnet_state& S, int j, bool more, bool do_scale, int gl, Emit&& emit) {
        neighbour_step<LPP, VPL, W, L, FULL>(S, j, more, do_scale, gl, fa, fn, my_w, my_ok, my_m, plan, emit);
    }
};

// the fan-out walk's arrays for a kernel that steps all the lane groups of a workgroup through their candidates TOGETHER
// (k_score_fanout, score_fanout.hip): begin() = the source's rows, own block and output plan, fetch() + issue(0) = ids and meta
// records of up to LPP candidates and the first one's rows, step(j) = candidate j's 26 inner products, reduced and finished.  The same
// operations in the same order as gram_fanout (whose text this is, with emit in place of the stores): the features of the two are
// the same bits (tests/test_score_fanout.py compares them with torch.equal).  fetch() takes the lane's candidate id itself, not a
// list: the caller forms it (a list entry, an id of a contiguous range, a row's lead id).
template <int LPP, int VPL, int W, int L, bool FULL>
struct FanWalk {
    using C = GramCfg<LPP, L>;
    using FC = FanCfg<LPP, L>;
    static constexpr int NR = C::NR, NN = C::NN, F = VPL * W, PER = C::PER;
    float fs[NR][F];                         // the source's rows, decay applied
    int sl[PER];                             // per-lane output plan (invariant over the unit): gram_fanout's
    bool own[PER], in[PER];
    float ys[PER];
    bool sok;
    int64_t my_w;                            // lane gl: candidate gl of the current fetch
    bool my_ok;
    MetaView my_m;
    float fn[NR][F];                         // rows of the NEXT candidate (raw)

    __device__ __forceinline__ void begin(const tpnet_state& S, int64_t u, bool valid, double now, double lambda, bool do_scale,
                                          int gl) {
        const NodeMeta* meta = reinterpret_cast<const NodeMeta*>(S.meta);
        sok = valid && (uint64_t)u < (uint64_t)S.N;
        if (valid && !sok && gl == 0) atomicAdd(S.err, 1u);
        if (!sok) u = 0;
        {
            const MetaView m = read_meta(meta, u, READER_BID, now, lambda);
            load_node_rows<LPP, VPL, W, L, FULL>(S, u, m.copy, gl, fs);
            float g = 1.0f;
#pragma unroll
            for (int i = 1; i <= L; ++i) {
                g *= m.g;
#pragma unroll
                for (int k = 0; k < F; ++k) fs[i][k] *= g;
            }
        }
        float ss[FC::TRI];
#pragma unroll
        for (int a = 0; a < NR; ++a) {
#pragma unroll
            for (int b = a; b < NR; ++b) ss[FC::tri(a, b)] = group_allreduce<LPP>(dot_chunk<F, false>(fs[a], fs[b]));
        }
#pragma unroll
        for (int kk = 0; kk < PER; ++kk) {
            int idx = gl * PER + kk;
            in[kk] = idx < C::NG;
            idx = in[kk] ? idx : 0;
            const int a = idx / NN, b = idx - a * NN;
            own[kk] = a < NR && b < NR;
            ys[kk] = 0.0f;
            if (own[kk]) {
                const int ta = FC::tri(a < b ? a : b, a < b ? b : a);
                float y = 0.0f;
#pragma unroll
                for (int q = 0; q < FC::TRI; ++q) y = (ta == q) ? ss[q] : y;     // (register array: a select chain)
                ys[kk] = finish_feature(y, do_scale);
                sl[kk] = 0;
            } else if (a < NR) {                       // (source row a, candidate row b - NR)
                sl[kk] = FC::O_SC + a * NR + (b - NR);
            } else if (b < NR) {                       // mirrored
                sl[kk] = FC::O_SC + b * NR + (a - NR);
            } else {
                const int x = a - NR, y = b - NR;
                sl[kk] = FC::O_CC + FC::tri(x < y ? x : y, x < y ? y : x);
            }
        }
    }
    // id: this lane's candidate (has: the lane has one), neighbour_fetch's checks and meta record
    __device__ __forceinline__ void fetch(const tpnet_state& S, int64_t id, bool has, bool valid, double now, double lambda) {
        const NodeMeta* meta = reinterpret_cast<const NodeMeta*>(S.meta);
        my_w = (valid && has) ? id : 0;
        my_ok = sok && (uint64_t)my_w < (uint64_t)S.N;
        if (valid && sok && has && !my_ok) atomicAdd(S.err, 1u);
        if (!my_ok) my_w = 0;
        my_m = read_meta(meta, my_w, READER_BID, now, lambda);
    }
    __device__ __forceinline__ void issue(const tpnet_state& S, int j, int gl) {
        neighbour_issue<LPP, VPL, W, L, FULL>(S, my_w, my_m, j, gl, fn);
    }
    // candidate j of the fetch (its rows in fn; `more`: issue candidate j + 1 behind it): emit(idx, x) for each of this lane's
    // elements idx = gl * PER + kk (< NG) of the feature row G(source, candidate)
    template <class Emit>
    __device__ __forceinline__ void step(const tpnet_state& S, int j, bool more, bool do_scale, int gl, Emit&& emit) {
        const bool wok = __shfl((int)my_ok, j, LPP) != 0;
        const float mg = __shfl(my_m.g, j, LPP);
        float fw[NR][F];                               // the candidate's rows, decay applied
#pragma unroll
        for (int x = 0; x < F; ++x) fw[0][x] = fn[0][x];
        float g = 1.0f;
#pragma unroll
        for (int i = 1; i <= L; ++i) {
            g *= mg;
#pragma unroll
            for (int x = 0; x < F; ++x) fw[i][x] = fn[i][x] * g;
        }
        if (more) issue(S, j + 1, gl);
        float acc[FC::MPS];
#pragma unroll
        for (int i = 0; i < FC::MPS; ++i) acc[i] = 0.0f;
#pragma unroll
        for (int a = 0; a < NR; ++a) {
#pragma unroll
            for (int b = a; b < NR; ++b) acc[FC::O_CC + FC::tri(a, b)] = dot_chunk<F, false>(fw[a], fw[b]);
#pragma unroll
            for (int b = 0; b < NR; ++b) acc[FC::O_SC + a * NR + b] = dot_chunk<F, false>(fs[a], fw[b]);
        }
        Halve<FC::MPS, LPP / 2>::run(acc, gl);         // lane gl now holds the complete sums of slots [gl*PERS, ...)
#pragma unroll
        for (int kk = 0; kk < PER; ++kk) {
            const int idx = in[kk] ? gl * PER + kk : 0;
            float x = finish_feature(pick_slot<FC::PERS, LPP>(acc, sl[kk]), do_scale);
            if (own[kk]) x = ys[kk];
            if (!wok) x = __builtin_nanf("");
            if (in[kk]) emit(idx, x);
        }
    }
};


}  // namespace tpnet
