// The encoder's call (models/TPNet.py:311-324, 129) end to end in ONE C call: anchored readout, then self.mlp in the fp32 class
// (the dense-layer kernel of feature_mfma.hip) on the same stream -- and THE route of every anchored readout (anchored_route).
// Measured and not kept (round 3): the dense layers of a chunk of rows on a helper stream BESIDE the readout of the next chunk.
// Side by side the two kernels slow each other more than the overlap wins -- 800 000 pairs at d=256: readout 355 us + dense
// layers 237 us = 592 us one after the other; 608 us in 2 chunks, 707 in 4, 752 in 8, 1 194 in 16 (tools/encoder_call_rate.py) --
// both live on the memory system (gathers there, a 410 MB tile stream here).  What removes the dense layers' traffic is their
// fusion INTO the anchored kernel: encoder_mfma.hip for rows of 36..160 floats, anchored_feature.hip for rows of 164..512
// (the latter is the route of a geometry class only where it was measured faster than the two launches).
#include "tpnet_common.h"

using namespace tpnet;

// ---- the predicates that only the route reads: TPNET_FLAG_ROWS8 on a row of d % 4 == 2 (the matrix cores, or the call is refused)
static bool rows8_asked(const tpnet_state& st, uint32_t flags) { return (flags & TPNET_FLAG_ROWS8) && st.d % 4 == 2; }
// TPNET_FLAG_LAYERS_MFMA on a shape it serves, not taken back by TPNET_FLAG_NO_MFMA_READOUT: every other call keeps its route
static bool layers_asked(const tpnet_state& st, int64_t n_rows, int K, uint32_t flags) {
    return (flags & TPNET_FLAG_LAYERS_MFMA) && !(flags & (TPNET_FLAG_NO_MFMA_READOUT | TPNET_FLAG_PACKED)) &&
           encoder_layers_supported(st, n_rows, K);
}
// rows of <= 128 floats: the generic pair kernel's 16-lane geometry reads an encoder-style list faster than the anchored walk
// (tools/encoder_readout.py, 80 000 pairs at d=128: 27.1 against 31.3 us; 16 000 at d=64: 7.1 against 13.2) -- the encoder's calls
// take it there, from pair lists the sampler kernel writes beside the neighbour ids
static bool encoder_generic_readout(const tpnet_state& st) {
    static const int off = TPNET_DEV_INT(ENCODER_ANCHORED_ONLY, 0);
    return !off && st.d <= 128;
}
// rows of 164..512 floats: is k_anchored_feature the ROUTE of this shape (tpnet_anchored_features_wide reaches it regardless)?
// Per geometry class, by measurement (profiles/encoder_wide.md): 32 lanes x 2 vectors (d <= 256), 64 lanes x 2 vectors (d >= 260).
static constexpr bool WIDE_ROUTE_32x2 = false, WIDE_ROUTE_64x2 = false;
static bool encoder_wide_routed(const tpnet_state& st, int64_t n_rows, int K, const tpnet_mlp* mlp) {
    static const int off = TPNET_DEV_INT(NO_ENCODER_WIDE, 0);
    if (off || !encoder_wide_supported(st, n_rows, K, mlp)) return false;
    return encoder_wide_class(st) == 32 ? WIDE_ROUTE_32x2 : WIDE_ROUTE_64x2;
}

AnchoredRoute tpnet::anchored_route(const tpnet_state& st, int64_t n_rows, int K, uint32_t flags, const tpnet_mlp* mlp, bool aligned,
                                    bool pair_lists) {
    AnchoredRoute r{AK_REFUSED, 0, false};
    if (flags & TPNET_FLAG_PACKED) return r;           // packed rows exist for the one-pair readout only
    // who forms the Gram: the first match wins
    if ((r.rows8 = rows8_asked(st, flags)))            // (alignment: the launch's own check -- there is no walk to fall back to)
        r.gram = encoder_mfma_supported(st, n_rows, K, flags) ? AK_MFMA : AK_REFUSED;
    else if (pair_lists && encoder_generic_readout(st) && !encoder_mfma_supported(st, n_rows, K, flags) &&
             !layers_asked(st, n_rows, K, flags))
        r.gram = AK_GENERIC;      // (never d = 64, L = 3 with TPNET_FLAG_NO_MFMA_READOUT: on 16-byte rows the query ignores that flag)
    else if (!pair_gram_anchored_supported(st))
        r.gram = AK_REFUSED;
    else if (!(flags & TPNET_FLAG_NO_MFMA_READOUT) && encoder_mfma_supported(st, n_rows, K) && aligned)
        r.gram = AK_MFMA;
    else if (layers_asked(st, n_rows, K, flags) && aligned)
        r.gram = AK_LAYERS;
    else
        r.gram = AK_WALK;
    // ONE launch with self.mlp: k_encoder_fused where it serves, else the wide kernel where its class is routed
    if (mlp && !(flags & TPNET_FLAG_NO_MFMA_READOUT))
        r.one_launch = encoder_fused_supported(st, n_rows, K, mlp, flags) ? 1 : encoder_wide_routed(st, n_rows, K, mlp) ? 2 : 0;
    return r;
}

static bool state_set(const tpnet_state* st) { return st && st->p0 && st->q && st->meta && st->N >= 1 && st->d >= 1; }

extern "C" {

int tpnet_anchored_route(const tpnet_state* st, int64_t n_rows, int32_t K, uint32_t flags, const tpnet_mlp* mlp) {
    if (check_state(st)) return 0;
    const AnchoredRoute r = anchored_route(*st, n_rows, K, flags, mlp, true, false);
    return r.gram == AK_REFUSED ? 0 : (int)r.gram | r.one_launch << 4;
}

int tpnet_pair_gram_anchored_supported(const tpnet_state* st) { return !check_state(st) && pair_gram_anchored_supported(*st); }

int tpnet_encoder_fused_supported(const tpnet_state* st, int64_t n_rows, int32_t K, const tpnet_mlp* mlp) {
    return state_set(st) && anchored_route(*st, n_rows, K, 0, mlp, true, false).one_launch != 0;
}

int tpnet_encoder_rows8_supported(const tpnet_state* st, int64_t n_rows, int32_t K, const tpnet_mlp* mlp) {
    if (!state_set(st)) return 0;
    const AnchoredRoute r = anchored_route(*st, n_rows, K, TPNET_FLAG_ROWS8, mlp, true, false);
    return r.rows8 && (mlp ? r.one_launch == 1 : r.gram == AK_MFMA);
}

int tpnet_encoder_layers_supported(const tpnet_state* st, int64_t n_rows, int32_t K) {
    return state_set(st) && encoder_layers_supported(*st, n_rows, K);
}

int tpnet_encoder_wide_supported(const tpnet_state* st, int64_t n_rows, int32_t K, const tpnet_mlp* mlp) {
    return state_set(st) && encoder_wide_supported(*st, n_rows, K, mlp);
}

int tpnet_anchored_features_wide(const tpnet_state* st, const int64_t* neigh, const int64_t* a1, const int64_t* a2, int64_t n_rows,
                                 int32_t K, double now_time, double lambda, uint32_t flags, const tpnet_mlp* mlp, float* gram,
                                 float* out, void* stream) {
    if (check_state(st) || n_rows < 0 || K < 0 || !mlp) return TPNET_ERR_BAD_ARG;
    if (n_rows == 0 || K == 0) return TPNET_OK;
    if (!neigh || !a1 || !a2 || !out) return TPNET_ERR_BAD_ARG;
    return launch_anchored_feature(*st, neigh, a1, a2, n_rows, K, now_time, lambda, flags, mlp, gram, out, (hipStream_t)stream);
}

int tpnet_anchored_features(const tpnet_state* st, const int64_t* neigh, const int64_t* a1, const int64_t* a2, int64_t n_rows,
                            int32_t K, double now_time, double lambda, uint32_t flags, const tpnet_mlp* mlp, float* gram,
                            float* out, void* stream) {
    if (check_state(st) || st->L != 3) return TPNET_ERR_BAD_ARG;
    if (n_rows < 0 || K < 0 || (n_rows > 0 && K > 0 && (!neigh || !a1 || !a2 || !out || !mlp))) return TPNET_ERR_BAD_ARG;
    if (n_rows == 0 || K == 0) return TPNET_OK;
    if (flags & TPNET_FLAG_PACKED) return TPNET_ERR_BAD_ARG;
    if (mlp->F != 64 || mlp->H != 256 || !mlp->w1 || !mlp->w2f || !mlp->b1 || !mlp->b2) return TPNET_ERR_BAD_ARG;
    if (!aligned16({gram, out})) return TPNET_ERR_BAD_ARG;
    const AnchoredRoute r = anchored_route(*st, n_rows, K, flags, mlp, true, false);
    if (r.rows8 && r.gram == AK_REFUSED) return TPNET_ERR_BAD_ARG;
    // readout + dense layers in ONE launch on the matrix cores (encoder_mfma.hip); a runtime that refuses it: two launches below
    if (r.one_launch == 1 &&
        launch_encoder_fused(*st, neigh, a1, a2, n_rows, K, now_time, lambda, flags, mlp, gram, out, (hipStream_t)stream) == TPNET_OK)
        return TPNET_OK;
    // wide rows: the vector-ALU walk with the dense layers inside (anchored_feature.hip), where that is the class's route
    if (r.one_launch == 2)
        return launch_anchored_feature(*st, neigh, a1, a2, n_rows, K, now_time, lambda, flags, mlp, gram, out, (hipStream_t)stream);
    if (!gram) return TPNET_ERR_NEED_GRAM;             // (the fused launch was refused after the caller had been told it may pass NULL)
    if (r.gram == AK_REFUSED) return TPNET_ERR_BAD_ARG;
    const int64_t half = n_rows * (int64_t)K;                // pairs per anchor side
    int rc = tpnet_pair_gram_anchored(st, neigh, a1, a2, n_rows, K, now_time, lambda, flags, gram, gram + half * 64, stream);
    if (rc) return rc;
    return launch_mlp_rows(mlp, gram, 2 * half, out, (hipStream_t)stream);
}

int tpnet_encoder_features(const tpnet_state* st, const void* sampler, int64_t E, int64_t num_nodes, const int64_t* src,
                           const int64_t* other, const double* t, int64_t B, int32_t K, double now_time, double lambda,
                           uint32_t flags, const tpnet_mlp* mlp, void* scratch, size_t scratch_bytes, float* gram, float* out,
                           void* stream) {
    if (!st || !sampler || B < 0 || K < 1 || (B > 0 && (!src || !other || !t || !scratch || !out || !mlp)))
        return TPNET_ERR_BAD_ARG;
    if (B == 0) return TPNET_OK;
    const AnchoredRoute r = anchored_route(*st, 2 * B, K, flags, nullptr, true, true);      // (the Gram kernel alone: as encoder_rows asks)
    if (r.rows8 && r.gram == AK_REFUSED) return TPNET_ERR_BAD_ARG;
    // rows + neighbours exactly as tpnet_encoder_gram lays them out in `scratch`
    int rc = encoder_rows(st, sampler, E, num_nodes, src, other, t, B, K, flags, scratch, scratch_bytes, stream);
    if (rc) return rc;
    int64_t* nodes = (int64_t*)(((size_t)scratch + 255) / 256 * 256);
    int64_t* a1 = nodes + 4 * B;
    int64_t* a2 = a1 + 2 * B;
    int64_t* neigh = a2 + 2 * B;
    if (gram && r.gram == AK_GENERIC && st->L == 3 && mlp->F == 64 && mlp->H == 256 && mlp->w1 && mlp->w2f && mlp->b1 && mlp->b2 &&
        aligned16({gram, out})) {
        // narrow rows: the generic readout on the pair lists the sampler kernel wrote behind the neighbour ids, then the dense layers
        const int64_t half = 2 * B * (int64_t)K;
        rc = tpnet_pair_gram(st, neigh + half, neigh + 3 * half, 2 * half, now_time, lambda, flags, gram, stream);
        if (rc) return rc;
        return launch_mlp_rows(mlp, gram, 2 * half, out, (hipStream_t)stream);
    }
    return tpnet_anchored_features(st, neigh, a1, a2, 2 * B, K, now_time, lambda, flags, mlp, gram, out, stream);
}

}  // extern "C"
