/*
 * tpnet_hip.h -- C ABI of the MI355X (gfx950) implementation of TPNet's temporal-walk-matrix hot path.
 *
 * Drop-in boundary: the functions below are what a binding for the reference's
 * `RandomProjectionModule` (reference: models/TPNet.py:9-157) calls instead of the stock ATen ops.
 * Plain C: device pointers, sizes, a hipStream_t passed as void*; no torch types.  All device buffers
 * are owned by the caller (e.g. the PyTorch caching allocator); nothing is allocated or freed inside;
 * kernels are enqueued on the given stream and the functions do not synchronise unless stated.
 *
 * Every function returns 0 on success or a negative tpnet_status code; tpnet_strerror() names it.
 *
 * ---------------------------------------------------------------------------------------------------
 * State layout in HBM (one instance per RandomProjectionModule):
 *   p0   float [N][d]            layer 0 (the random projection matrix P[0]; never written by update)
 *   q    float [2][N][L][d]      layers 1..L as per-node "bundles" (L*d contiguous floats), two copies
 *                                (ping-pong): a batch reads the pre-batch copy and writes the other one,
 *                                which removes the read/write hazard between layers inside ONE launch
 *   meta tpnet_node_meta [N]     per node: which copy is current + the time its bundle was last decayed to
 * Mathematical state (what the reference keeps eagerly, models/TPNet.py:83-85):
 *   P[i][n] = q[c][n][i-1] * exp(-lambda * i * (now_time - meta[n].tref[c])),  c = cur(n), i = 1..L
 * i.e. the dense per-batch decay of the reference is carried lazily per row and applied on read.
 * ---------------------------------------------------------------------------------------------------
 */
#ifndef TPNET_HIP_H
#define TPNET_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TPNET_ABI_VERSION 7 /* 2: + tpnet_gather_elems, tpnet_gram_finish, tpnet_gram_unpack, tpnet_decoder_bf16, TPNET_FLAG_PACKED;
                               3: + tpnet_stream_workspace_bytes (windowed schedule of tpnet_run_stream);
                               4: + tpnet_pair_feature (readout + self.mlp in one launch), host-array entry points
                                    (tpnet_stage_*, tpnet_host_pair_feature, tpnet_host_update), tpnet_pair_gram_anchored;
                               5: + tpnet_run_stream_tagged / tpnet_plan_tag (a stream's plan replayed across epochs), the encoder's call as one
                                    crossing (tpnet_anchored_features, tpnet_encoder_features, tpnet_host_encoder_features), the targeted
                                    exchange's plan on the device (tpnet_xplan_targeted);
                               6: + tpnet_mlp::wimg / tpnet_mlp_prepare_image (the encoder's readout and self.mlp in ONE launch on the matrix
                                    cores), TPNET_FLAG_NO_MFMA_READOUT, tpnet_rows_stream_targeted, tpnet_mlp64_bwd_f32, tpnet_host_anchored_features;
                                    tpnet_run_stream_tagged replays streams of up to 64 chunks;
                               7: + tpnet_stream_schedule (which schedule tpnet_run_stream would take); tpnet_xplan_targeted serves G = 1;
                                    tpnet_xplan_targeted_large (batches beyond one workgroup's lists); tpnet_wshard_* (a row shard on the windowed pipeline);
                                    the side-by-side plans of a multi-chunk stream are bounded (TPNET_ARENA_MAX_RATIO);
                                    added since without a new number: tpnet_neg_* (the negative edge sampler's three strategies);
                                    tpnet_lp_metrics* (a batch's BCE loss, average precision and ROC-AUC as one device record);
                                    tpnet_lp_train_loss (the same record for a training batch, with the loss's gradient by the logits);
                                    tpnet_edgebank_* (the EdgeBank baseline's three memory modes on a prefix of one static stream);
                                    tpnet_mlp_rows_* (self.mlp on the matrix cores for num_layer 1 and 2);
                                    tpnet_mlp_rows_bwd_* (its weight gradients on the matrix cores, same widths);
                                    tpnet_decoder_f32* (LinkPredictor_v1 in the fp32 class, forward and backward);
                                    tpnet_mlp_l4_* (self.mlp on the matrix cores for num_layer 4, forward and backward);
                                    TPNET_FLAG_ROWS8 / tpnet_encoder_rows8_supported (the encoder's matrix-core calls on rows of d % 4 == 2);
                                    tpnet_import_layers_ld / tpnet_export_layers_ld / tpnet_pad_rows / tpnet_gather_rows_ld (a table whose rows
                                    are kept wider than the caller's, pad columns zero);
                                    TPNET_FLAG_LAYERS_MFMA / tpnet_encoder_layers_* (the encoder's matrix-core readout for num_layer 1, 2, 4);
                                    tpnet_pair_gram_fanout* (one source against C candidates), tpnet_neg_sample_many (per-query candidates),
                                    tpnet_lp_ranking* (a batch's MRR and Hits@k as one device record);
                                    tpnet_anchored_route (which kernel serves an anchored readout: the one table);
                                    tpnet_score_one_to_many* (one source against many candidates, one logit per pair, in one launch),
                                    tpnet_lp_ranking_skip (the ranking record with one absent candidate column per query);
                                    tpnet_score_topk_range (the K best ids of a whole id range per source, formed in the scoring kernel) */
#define TPNET_MAX_LAYERS 4 /* num_layer L in 1..4 (reference default 3, utils/load_configs.py:70) */

typedef enum tpnet_status {
    TPNET_OK = 0,
    TPNET_ERR_BAD_ARG = -1,     /* null pointer, negative size, L out of range, d < 1 */
    TPNET_ERR_WORKSPACE = -2,   /* workspace too small (see tpnet_workspace_bytes) */
    TPNET_ERR_HIP = -3,         /* a HIP runtime call failed; tpnet_last_hip_error() has the hipError_t */
    TPNET_ERR_INDEX = -4,       /* a node id outside [0, N) was found (checked on device; such ids are skipped,
                                   never dereferenced) -- reported by tpnet_check_errors() */
    TPNET_ERR_NO_DEVICE = -5,
    TPNET_ERR_NEED_GRAM = -6    /* tpnet_anchored_features / tpnet_encoder_features / tpnet_host_*: called with gram == NULL (allowed
                                   where tpnet_encoder_fused_supported), but the one-launch kernel could not be launched on this
                                   runtime: call again with a gram buffer (readout and dense layers then run as two launches) */
} tpnet_status;

/* 32-byte per-node record.  tref is kept per copy so that a launch rewriting a node never disturbs what a
 * concurrent reader of the same launch needs (the pre-batch copy and its reference time). */
typedef struct tpnet_node_meta {
    uint32_t ver;   /* (launch_id << 1) | current_copy */
    uint32_t pad0;
    double tref[2]; /* time each copy's bundle is expressed at (f64, like now_time: models/TPNet.py:36-37,99) */
    uint64_t pad1;
} tpnet_node_meta;

typedef struct tpnet_state {
    float* p0;             /* [N][d] */
    float* q;              /* [2][N][L][d] */
    tpnet_node_meta* meta; /* [N] */
    int64_t N;             /* rows, including padding row 0 (reference node_num) */
    int32_t d;             /* projection dimension (any d >= 1; d % 4 == 0 takes the vector path) */
    int32_t L;             /* num_layer */
    uint32_t* err;         /* [4] device error words, zeroed by tpnet_state_init; err[0] = bad-id count */
} tpnet_state;

/* flags */
#define TPNET_FLAG_NOT_SCALE 1u     /* readout: return the raw Gram (reference not_scale=True, TPNet.py:124-125) */
#define TPNET_FLAG_EAGER_DECAY 2u   /* update: dense decay of every row first, exactly models/TPNet.py:83-85 */
#define TPNET_FLAG_SEQUENTIAL 4u    /* update: never split a target's contributions over several wave groups:
                                       the sum is then accumulated in the reference's index order (src side,
                                       then dst side, models/TPNet.py:93-96) */
#define TPNET_FLAG_PACKED 8u        /* readout (tpnet_pair_gram, tpnet_run_stream, tpnet_step_batch): write only the
                                       (2L+2)(2L+3)/2 distinct entries a <= b of the symmetric Gram, raw (no x<0 -> 0 /
                                       log), row-major upper triangle, row stride (2L+2)(2L+3)/2 floats -- the wire
                                       format of the column-sharded table, whose partial inner products are summed
                                       across GPUs before tpnet_gram_unpack finishes them */

#define TPNET_FLAG_SCHED_WINDOWED 16u /* tpnet_run_stream: take the windowed schedule whenever it applies (>= 4 batches), not
                                       only for streams long enough for it to pay (>= 28 batches of <= 2048 edges, >= 56 larger
                                       ones) */
#define TPNET_FLAG_SCHED_BATCH 32u    /* tpnet_run_stream: one launch per batch, always */
#define TPNET_FLAG_PLAN_SORTED 64u    /* tpnet_run_stream, windowed schedule: plan every chunk with the chunk planner (two device-wide
                                       radix sorts) even where the three-launch planner applies (batches of <= 2048 edges, <= 64
                                       windows per chunk).  Both give the same bits; this one is the slower start-up */
#define TPNET_FLAG_PLAN_HASHED 128u   /* tpnet_run_stream, windowed schedule: plan with the hashed planner (a fill + four kernels, <= 64
                                       windows per chunk) even where the one-launch dense planner applies (table small against the
                                       stream: N * 12 bytes <= batch * L * d * 4).  Same bits again */

#define TPNET_FLAG_NO_MFMA_READOUT 256u /* tpnet_pair_gram_anchored and the encoder calls built on it: keep the vector-ALU readout where
                                       the matrix-core one applies (rows of 36..160 floats, d % 4 == 0, L = 3, K >= 4: split-bf16 operands,
                                       three pieces per value, fp32 accumulation -- fp32 class, other summation order) */
#define TPNET_FLAG_ROWS8 512u         /* tpnet_pair_gram_anchored, tpnet_anchored_features, tpnet_encoder_gram, tpnet_encoder_features,
                                       tpnet_host_encoder_features, tpnet_host_anchored_features: serve rows that are only 8-byte
                                       aligned (d % 4 == 2, 38 <= d <= 158 -- the reference's default widths 110 / 130 / 150 --, L = 3,
                                       K >= 4) on the matrix cores, every 16-byte piece of a row fetched as two 8-byte halves
                                       (tpnet_encoder_rows8_supported).  No effect where d % 4 == 0.  With d % 4 == 2 only the
                                       matrix-core kernels serve the call: TPNET_ERR_BAD_ARG for K < 4, L != 3, d outside 38..158,
                                       outputs that are not 16-byte aligned, or TPNET_FLAG_NO_MFMA_READOUT beside it */
#define TPNET_FLAG_LAYERS_MFMA 1024u  /* tpnet_pair_gram_anchored, tpnet_encoder_gram: a state with L = 1, 2 or 4 takes the anchored
                                       readout on the matrix cores (csrc/encoder_layers.hip, fp32 class as at L = 3) where
                                       tpnet_encoder_layers_supported answers 1 and the outputs are 16-byte aligned.  Every other call
                                       with the flag -- L = 3, a shape the query declines, TPNET_FLAG_NO_MFMA_READOUT beside it --
                                       is the call without it, bit for bit: never an error */

const char* tpnet_strerror(int status);
int tpnet_abi_version(void);
int tpnet_last_hip_error(void);
/* number of HIP devices visible (0 without a GPU; never initialises a context) */
int tpnet_device_count(void);

/* First-use costs of the HIP runtime, paid when the caller chooses (e.g. once per process and device, when the module's engine
 * is created) instead of inside the first long call: measured, the first 20-launch call of a fresh process takes 60-70 us
 * longer than every later one unless a burst of launches FOLLOWED BY A SYNCHRONISE came before it.  Enqueues one kernel that
 * keeps the stream busy for spin_us microseconds and `launches` kernels with 512 bytes of arguments behind it; does not
 * synchronise itself (the caller does, once).  Touches no caller memory. */
int tpnet_runtime_warmup(int32_t launches, int32_t spin_us, void* stream);

/* Bytes the caller must allocate for q and meta. */
size_t tpnet_q_bytes(int64_t N, int32_t d, int32_t L);
size_t tpnet_meta_bytes(int64_t N);

/* Zero q, set meta[n] = {ver 0, tref = t0}, zero err.  (reset_random_projections, models/TPNet.py:131-139,
 * minus the P[0] redraw which stays with the caller's RNG.) */
int tpnet_state_init(const tpnet_state* st, double t0, void* stream);

/* layers[i-1] (device, row-major [N][d], i = 1..L)  ->  q (copy 0), meta = {0, now_time}.
 * (reload_random_projections / load_state_dict / .to(): models/TPNet.py:149-157) */
int tpnet_import_layers(const tpnet_state* st, const float* const* layers, double now_time, void* stream);

/* q -> layers[i-1][N][d] with the pending decay applied: the eager matrices the reference would hold at
 * now_time.  (backup_random_projections / state_dict: models/TPNet.py:141-147) */
int tpnet_export_layers(const tpnet_state* st, float* const* layers, double now_time, double lambda, void* stream);

/* Eager dense decay, P[i] <- P[i] * factors[i-1] (host array, L floats), tref <- t_new for all rows.
 * (models/TPNet.py:83-85; factors = f32(exp(-lambda*(t_new-now))^i) computed by the caller in f64) */
int tpnet_decay(const tpnet_state* st, const float* factors, double t_new, void* stream);

/* get_random_projections (models/TPNet.py:101-110): out[(i*n + k)*d + :] = P[i][ids[k]] at now_time, i = 0..L. */
int tpnet_gather_rows(const tpnet_state* st, const int64_t* ids, int64_t n, double now_time, double lambda,
                      float* out, void* stream);

/* A table kept wider than the caller's tensors (RandomProjectionModule.padded_rows): the engine's rows are st->d floats, the
 * caller's rows `ld` floats, 1 <= ld <= st->d; columns ld..st->d-1 of the engine's rows ("pad columns") hold +0.0 -- a zero column adds
 * exactly 0 to every inner product and stays 0 under every update.  The wide side (st->q, st->p0, the mirror) is read and written
 * in 16-byte vectors: it must be 16-byte aligned, with st->d % 4 == 0 (ld == st->d is allowed: the plain entry points' result); the
 * narrow side in 8-byte vectors when ld is even (rows then 8-byte aligned: the base must be), else float by float.
 * TPNET_ERR_BAD_ARG, before anything is launched, for a null pointer, ld outside its range, or a wide side that is not aligned.
 *
 * tpnet_import_layers_ld: tpnet_import_layers from layers of [N][ld]; the pad columns of copy 0 AND copy 1 of every bundle are
 * written as +0.0 (copy 1's other columns are left as they are: nothing reads them before a launch has written them). */
int tpnet_import_layers_ld(const tpnet_state* st, const float* const* layers, int32_t ld, double now_time, void* stream);
/* tpnet_export_layers_ld: tpnet_export_layers into layers of [N][ld]: the first ld columns of every row, never a float past them. */
int tpnet_export_layers_ld(const tpnet_state* st, float* const* layers, int32_t ld, double now_time, double lambda, void* stream);
/* dst[n][0..ld_src-1] = src[n][0..ld_src-1], dst[n][ld_src..ld_dst-1] = +0.0 for n < N: the wide copy of P[0] that st->p0 points at.
 * 1 <= ld_src <= ld_dst; dst is the wide side (16-byte aligned, ld_dst % 4 == 0). */
int tpnet_pad_rows(const float* src, int32_t ld_src, float* dst, int32_t ld_dst, int64_t N, void* stream);
/* tpnet_gather_rows with output rows of ld_out floats: out[(i*n + k)*ld_out + c] = P[i][ids[k]][c], c < ld_out <= st->d. */
int tpnet_gather_rows_ld(const tpnet_state* st, const int64_t* ids, int64_t n, double now_time, double lambda, int32_t ld_out,
                         float* out, void* stream);

/* Single elements of every layer: out[k][i] = P[i][rows[k]][cols[k]] at now_time, i = 0..L (out: device float[n][L+1]).
 * With a square table (d = N) this is the readout of the reference's sibling walk-matrix state, PINT's
 * MatrixMemory.get_memory before its normalisation (models/MemoryModel.py:396-405: `matrix[src, dst]`). */
int tpnet_gather_elems(const tpnet_state* st, const int64_t* rows, const int64_t* cols, int64_t n, double now_time,
                       double lambda, float* out, void* stream);

/* get_pair_wise_feature up to (not including) self.mlp (models/TPNet.py:112-128):
 * out[p][(2L+2)*a + b] = <R_a, R_b>, R = [P0[u_p]..PL[u_p], P0[v_p]..PL[v_p]] at now_time; then, unless
 * TPNET_FLAG_NOT_SCALE, x<0 -> 0 and log(x+1).  u, v: device int64[n]; out: device float[n][(2L+2)^2]. */
int tpnet_pair_gram(const tpnet_state* st, const int64_t* u, const int64_t* v, int64_t n, double now_time,
                    double lambda, uint32_t flags, float* out, void* stream);

/* Two pairwise readouts that share their first node, u's rows loaded once: out1[p] = G(u_p, v1_p), out2[p] =
 * G(u_p, v2_p) (same layout and scaling as tpnet_pair_gram).  This is the shape of the reference's callers: the
 * decoder's (src,dst)/(src,neg) pairs (models/modules.py:112) and the encoder's relative encodings, where every
 * neighbour is paired with the edge's src AND dst (models/TPNet.py:311-316). */
int tpnet_pair_gram_shared(const tpnet_state* st, const int64_t* u, const int64_t* v1, const int64_t* v2, int64_t n,
                           double now_time, double lambda, uint32_t flags, float* out1, float* out2, void* stream);

/* self.mlp = Linear(F, 4F) -> ReLU -> Linear(4F, F), F = (2L+2)^2 (models/TPNet.py:63-65), as device arrays in the layout
 * the fused kernel reads coalesced: w1t[k][j] = mlp[0].weight[j][k] ([F][H]), w2t[k][o] = mlp[2].weight[o][k] ([H][F]). */
typedef struct tpnet_mlp {
    const float* w1t; /* [F][H] */
    const float* b1;  /* [H] */
    const float* w2t; /* [H][F] */
    const float* b2;  /* [F] */
    int32_t F;        /* (2L+2)^2 */
    int32_t H;        /* 4 F */
    /* optional (NULL: never the matrix-core kernel), L = 3 only: the layouts the fp32 matrix-core kernel reads --
     * w1 = mlp[0].weight as is ([256][64]); w2f[((w * 2 + t) * 64 + lane) * 16 + s] = mlp[2].weight[32 t + (lane & 31)]
     * [32 w + (s & 3) + 8 (s >> 2) + 4 (lane >> 5)]  (w = 0..7 hidden tile, t = 0..1 output tile, s = 0..15 k-step) */
    const float* w1;
    const float* w2f;
    /* optional (NULL: the encoder's calls run readout and dense layers as two launches), F = 64 / H = 256 only: the image
     * tpnet_mlp_prepare_image writes -- both weight matrices split into two bf16 pieces per value, every 16-byte element the
     * operand of one lane of one v_mfma_f32_16x16x32_bf16, then b1 and b2 (tpnet_mlp_image_bytes() bytes, 16-byte aligned) */
    const void* wimg;
} tpnet_mlp;

/* get_pair_wise_feature INCLUDING self.mlp (models/TPNet.py:112-129) in one launch: the features of tpnet_pair_gram stay
 * in LDS and go through both dense layers in fp32 (differs from the torch layers in summation order only): on the fp32
 * matrix cores (v_mfma_f32_32x32x2_f32; L = 3, rows of >= 36 floats in 16-byte vectors, mlp->w1 / w2f given) for lists of any
 * length, else on the vector ALUs (any L; meant for short lists).
 * out: device float[n][F]; out_gram (optional, may be NULL): the pre-mlp features [n][F], what a backward pass needs.
 * Meant for the decoder's short pair lists (models/modules.py:112: n = batch size); any L in 1..4. */
int tpnet_pair_feature(const tpnet_state* st, const int64_t* u, const int64_t* v, int64_t n, double now_time,
                       double lambda, uint32_t flags, const tpnet_mlp* mlp, float* out_gram, float* out, void* stream);

/* self.mlp alone on the fp32 matrix cores (L = 3: 64 -> 256 -> 64; mlp->w1 / w2f required): y[n][64] = mlp(x[n][64]), for
 * features that a separate readout produced (the anchored / shared-first-node kernels of the encoder's call). */
int tpnet_mlp64_f32(const float* x, int64_t n, const tpnet_mlp* mlp, float* y, void* stream);

/* Which (F, H) tpnet_mlp_rows_f32 serves: 1 for (16, 64) and (36, 144) -- num_layer 1 and 2 -- else 0.  (64, 256) is
 * tpnet_mlp64_f32's; (100, 400), num_layer 4, is not served: its split weights (320 KB) do not fit a CU's LDS.  Pure host arithmetic.
 * (100, 400) has entries of its own that stream the weights: tpnet_mlp_l4_* below. */
int tpnet_mlp_rows_supported(int32_t F, int32_t H);
/* self.mlp alone for num_layer 1 and 2 in the fp32 class on the matrix cores: y[n][F] = mlp(x[n][F]) in ONE launch on the caller's
 * stream, no synchronisation (csrc/mlp_rows.hip: two-piece bf16 operands, three products per term, fp32 accumulators; <= 2e-5 of
 * the output scale against the torch layers, exact on small integers).  Weights from mlp->w1t, b1, w2t, b2 (mlp->w1 / w2f / wimg
 * are not read and stay NULL for these widths).  x and y: device, 16-byte aligned, x read only inside its n * F floats, y written
 * only inside its n * F floats.  n == 0: TPNET_OK.  TPNET_ERR_BAD_ARG, before any HIP call: a null pointer, an (F, H) that
 * tpnet_mlp_rows_supported refuses, a misaligned x or y; also when the runtime refuses the kernel's LDS (71 KB at F = 36) or
 * the launch -- the caller then runs the layers its other way.  A row of x that holds a NaN gives unspecified values in THAT row
 * of y (a NaN hidden unit passes the ReLU as 0); every other row is unaffected. */
int tpnet_mlp_rows_f32(const float* x, int64_t n, const tpnet_mlp* mlp, float* y, void* stream);

/* The derived layouts of a tpnet_mlp from the Parameters of self.mlp = Linear(F, H) -> ReLU -> Linear(H, F) (models/TPNet.py:63-65)
 * in ONE launch: w1 = mlp[0].weight [H][F], w2 = mlp[2].weight [F][H] (device, contiguous) -> w1t [F][H], w2t [H][F] and, for
 * F = 64 / H = 256 (else NULL), w2f in the gathered order tpnet_mlp documents.  b1, b2 and tpnet_mlp::w1 are the Parameters'
 * own storage.  A training loop calls this after every optimizer step (train_link_prediction.py:384-386). */
int tpnet_mlp_prepare(const float* w1, const float* w2, int32_t F, int32_t H, float* w1t, float* w2t, float* w2f, void* stream);
/* tpnet_mlp::wimg from the Parameters of self.mlp = Linear(64, 256) -> ReLU -> Linear(256, 64): w1 [256][64], b1 [256], w2 [64][256],
 * b2 [64] (device, contiguous) -> img (device, tpnet_mlp_image_bytes() bytes), one launch; to be called again whenever a
 * Parameter changed (the biases are copied into the image too). */
size_t tpnet_mlp_image_bytes(void);
int tpnet_mlp_prepare_image(const float* w1, const float* b1, const float* w2, const float* b2, void* img, void* stream);

/* ---- host-array entry points: what the reference's per-batch calls hand over are HOST numpy arrays (models/TPNet.py:
 * 74-77, 107, 117; train_link_prediction.py:359-373).  These variants take host pointers, check the ids on the host
 * (TPNET_ERR_INDEX for an id outside [-N, N); negative ids wrap like ATen indexing), copy them into a slot of a pinned,
 * device-mapped staging ring and launch kernels that read the slot directly -- no separate host->device copy is enqueued,
 * and a call costs one FFI crossing.  A tpnet_stage is the ONLY object this library allocates (pinned host memory + one
 * event per slot); a slot is reused only after the launch that read it has finished (the call waits if the ring wrapped).
 * A stage serves ONE calling thread and one device (the reference's loop is single-threaded under the GIL). */
typedef struct tpnet_stage tpnet_stage;
int tpnet_stage_create(int32_t slots, size_t slot_bytes, tpnet_stage** out);
/* (ABI 7) where the ring lives: mode 0 = pinned, device-mapped HOST memory (tpnet_stage_create: the kernels read the ids over PCIe,
 * one more ~2-us round trip at the head of every kernel's chain of dependent loads); 1 = DEVICE memory that the host writes through
 * the large BAR (fine-grained; +~1.6 us of host stores per 16 KB call, a local read at the head of the kernels; TPNET_ERR_NO_DEVICE
 * without a large BAR); -1 = 1 where the device has a large BAR, else 0.  Meant for the small per-batch ring: host stores through
 * the BAR run at ~7 GB/s. */
int tpnet_stage_create_ex(int32_t slots, size_t slot_bytes, int32_t mode, tpnet_stage** out);
int tpnet_stage_in_device_memory(const tpnet_stage* stage);
int tpnet_stage_destroy(tpnet_stage* stage);
/* largest n / B the host entry points accept for a stage (slot_bytes / 16, slot_bytes / 24 capped at 2048) */
int64_t tpnet_stage_max_pairs(const tpnet_stage* stage);
int64_t tpnet_stage_max_batch(const tpnet_stage* stage);

/* get_pair_wise_feature from host ids: mlp == NULL -> out = the pre-mlp features (tpnet_pair_gram); else out = mlp(features)
 * and out_gram (optional) the pre-mlp features (tpnet_pair_feature). */
int tpnet_host_pair_feature(const tpnet_state* st, tpnet_stage* stage, const int64_t* h_u, const int64_t* h_v, int64_t n,
                            double now_time, double lambda, uint32_t flags, const tpnet_mlp* mlp, float* out_gram,
                            float* out, void* stream);

/* update (models/TPNet.py:67-99) from host arrays, B <= tpnet_stage_max_batch: ONE plan kernel (a single workgroup sorts
 * the batch's 2B contributions in LDS and writes the item lists) + the step kernel.  workspace: tpnet_workspace_bytes(B, B).
 * Larger batches (up to slot_bytes / 24 edges): the staged arrays are copied to the tail of the workspace (which must then hold
 * tpnet_workspace_bytes(B, B) rounded up to 256 + 24 B bytes) and tpnet_update plans and steps from there. */
int tpnet_host_update(const tpnet_state* st, tpnet_stage* stage, const int64_t* h_src, const int64_t* h_dst,
                      const double* h_t, int64_t B, double now_time, double lambda, uint32_t launch_id, uint32_t flags,
                      void* workspace, size_t ws_bytes, void* stream);

/* The encoder's readout (models/TPNet.py:311-324): row i has two anchors a1[i], a2[i] (the edge's src and dst) and K sampled
 * neighbours neigh[i*K .. i*K+K); out1[(i*K + k)] = G(neigh[i*K+k], a1[i]), out2[(i*K + k)] = G(neigh[i*K+k], a2[i]), rows of
 * (2L+2)^2 floats laid out and scaled like tpnet_pair_gram's -- with out2 = out1 + n_rows*K*(2L+2)^2 this IS the reference's
 * get_pair_wise_feature(tile(neigh, 2), concat(repeat(a1, K), repeat(a2, K))) before self.mlp.  One lane group walks a row:
 * the anchors' rows are fetched once per row (not once per pair) and stay in registers, their own Gram blocks are reduced
 * once per row.  Needs rows of whole 16-byte vectors inside one chunk (d % 4 == 0 and 36 <= d <= 512, the reference's default
 * widths 120 / 140 / 160 included: tpnet_pair_gram_anchored_supported returns 1; a row that does not fill the chunk reads as
 * zeros past its end); other shapes take tpnet_pair_gram_shared / tpnet_pair_gram.  Rows of 36..160 floats with L = 3 and
 * K >= 4 are served by the matrix cores (csrc/encoder_mfma.hip: 16 x 16 x 32 bf16 products on operands split into three bf16
 * pieces, fp32 accumulation over d inside the pipe -- no cross-lane reduction; d = 64 / 128 in whole 32-deep steps, every other
 * width with the last step masked; TPNET_FLAG_NO_MFMA_READOUT keeps the vector-ALU walk).  Rows of d % 4 == 2 floats are
 * refused unless TPNET_FLAG_ROWS8 is set and tpnet_encoder_rows8_supported(st, n_rows, K, NULL): then the matrix cores serve
 * them too (no vector-ALU walk exists at those widths). */
int tpnet_pair_gram_anchored(const tpnet_state* st, const int64_t* neigh, const int64_t* a1, const int64_t* a2,
                             int64_t n_rows, int32_t K, double now_time, double lambda, uint32_t flags, float* out1,
                             float* out2, void* stream);
int tpnet_pair_gram_anchored_supported(const tpnet_state* st);

/* The one-vs-many readout of the ranking protocol: row i has ONE source src[i] and C candidate destinations cand[i*C .. i*C+C);
 * out[(i*C + c)] = G(src[i], cand[i*C + c]), rows of (2L+2)^2 floats laid out and scaled like tpnet_pair_gram's, with the SOURCE's
 * layers first -- rows stacked [src 0..L ; cand 0..L], the decoder's order (models/modules.py:112; NOT the anchored readout's, where
 * the neighbour comes first): this IS tpnet_pair_gram(repeat(src, C), cand) before self.mlp.  One lane group walks a unit = (row,
 * chunk of candidates; chunks as tpnet_pair_gram_anchored cuts them): the source's L+1 rows are fetched and decayed once per unit
 * and stay in registers, its own Gram block is reduced once per unit; per candidate only its L+1 rows are loaded and (L+1)^2 cross
 * products + (L+1)(L+2)/2 self products are formed (26 at L = 3; the anchored walk forms 42), candidate k+1's rows in flight while
 * candidate k is reduced.  Every row goes through the same lazy per-row decay as every other readout, and a pair's row depends on
 * its two nodes alone: the same (src, cand) gives the same bits whatever n_rows, C and its position.
 * Geometry: the anchored walk's class, d % 4 == 0, 36 <= d <= 512, L = 1..4 (tpnet_pair_gram_fanout_supported returns 1); other
 * states: TPNET_ERR_BAD_ARG -- the caller expands the ids and takes tpnet_pair_gram.  TPNET_FLAG_NOT_SCALE is honoured,
 * TPNET_FLAG_PACKED is refused.  Null pointers, C <= 0, n_rows < 0, n_rows * C >= 2^31 or an `out` that is not 16-byte aligned:
 * TPNET_ERR_BAD_ARG, nothing launched; n_rows == 0: TPNET_OK.  An id outside [0, N), source or candidate: the pairs it touches are
 * NaN rows (a source: its C rows; a candidate: its one row), every other row is untouched, the state's error word is raised. */
int tpnet_pair_gram_fanout(const tpnet_state* st, const int64_t* src, const int64_t* cand, int64_t n_rows, int32_t C,
                           double now_time, double lambda, uint32_t flags, float* out, void* stream);
int tpnet_pair_gram_fanout_supported(const tpnet_state* st);

/* ---- one source against many candidates, ONE logit per pair, in one launch (additive to ABI 7; csrc/score_fanout.hip, DESIGN.md
 * section 3.3 / 3.8).  For row i with source src[i] and every candidate c of that row
 *   f     = G(src[i], c)                      tpnet_pair_gram_fanout's finished row (64 floats, L = 3), bit for bit
 *   y     = W2m . relu(W1m . f + b1m) + b2m   self.mlp (tpnet_mlp: F = 64, H = 256, w1 and w2f present), the fp32 class
 *   a     = Wd[:, off : off + 64] . y + bd    LinkPredictor_v1's fc1 restricted to its feature columns (not_encode: the embedding
 *                                             columns meet zeros), read from fc1.weight AS IT IS: wd = [H][ldw] row-major
 *   logit = wd2 . relu(a) + bd2               fc2.weight [1][H], fc2.bias [1]
 * and only out[i, c] is written: features, mlp output and hidden layer never reach memory.
 * Candidates: cand != NULL: the list cand[i*C .. i*C+C), laid out as for tpnet_pair_gram_fanout; cand == NULL: the ids
 * [cand_lo, cand_lo + C), the same for every row, formed in the kernel (no id array).
 * lead (optional, [n_rows]): one more id per row, scored into column 0 -- out is then [n_rows, 1 + C], the layout tpnet_lp_ranking
 * reads; without it out is [n_rows, C].  gram (optional, NULL in production): [n_rows * C_1, 64] with C_1 = the row's column count
 * (C or 1 + C), the features f as the kernel formed them, 16-byte aligned.
 * PROMISES.  (1) A pair's logit depends on its two nodes, the state and the weights alone: the same (u, v) gives the same bits
 * whatever n_rows, C, its tile column, its chunk, list or range mode, lead or candidate column -- a pair is one column of every
 * matrix product, and the sums across waves are taken in a fixed order.  (2) Two calls on the same inputs give the same bits: no
 * floating-point atomics.
 * Served (tpnet_score_one_to_many_supported returns 1; host arithmetic, no GPU call): L = 3 with the reference mlp; d % 4 == 0,
 * 36 <= d <= 512 (lane geometries 16x1, 32x1, 32x2 and 64x2, exact-fit and masked; every instantiation builds without scratch);
 * 1 <= H <= 256; off % 4 == 0, ldw % 4 == 0,
 * off + 64 <= ldw; n_rows (1 + C) < 2^31.  TPNET_FLAG_NOT_SCALE is honoured, TPNET_FLAG_PACKED is refused.
 * Null pointers (cand, lead and gram may be NULL), C <= 0, n_rows < 0, a range that leaves [0, N), wd / gram / mlp->w1 / w2f / b2 not
 * 16-byte aligned, an unserved size: TPNET_ERR_BAD_ARG, nothing launched; n_rows == 0: TPNET_OK.  An id outside [0, N): its pairs
 * are NaN logits (a source: its whole row; a candidate or lead: its one entry), every other entry is untouched, the state's error
 * word is raised -- tpnet_pair_gram_fanout's rules.  A feature row that holds a NaN answers a NaN logit, as the torch layers do.
 * Needs 114 560 bytes of dynamic LDS per workgroup; a device that refuses them: TPNET_ERR_HIP. */
int tpnet_score_one_to_many(const tpnet_state* st, const int64_t* src, const int64_t* cand, int64_t cand_lo, const int64_t* lead,
                            int64_t n_rows, int32_t C, double now_time, double lambda, uint32_t flags, const tpnet_mlp* mlp,
                            const float* wd, int32_t ldw, int32_t off, const float* bd, const float* wd2, const float* bd2, int32_t H,
                            float* gram, float* out, void* stream);
int tpnet_score_one_to_many_supported(const tpnet_state* st, const tpnet_mlp* mlp, int32_t H, int32_t off, int32_t ldw);

/* ---- one source ranked against a whole id range, the counts formed in the scoring kernel (additive to ABI 7; csrc/score_fanout.hip,
 * DESIGN.md section 3.7 / 3.8).  For row i:  p = logit(src[i], pos[i])  (the four lines above), and over every id c of
 * [cand_lo, cand_lo + C) with c != pos[i], q = logit(src[i], c):
 *   counts[4 i + 0] = g  = #{q > p}        counts[4 i + 1] = e = #{q == p}        counts[4 i + 2] = nv = the ids counted
 *   counts[4 i + 3] = flags: value 2 when p or a counted q is NaN (tpnet_lp_ranking's rule and flag value), else 0
 * pos_logit[i] = p.  No other logit reaches memory: this is tpnet_score_one_to_many(range mode, lead = pos) followed by
 * tpnet_lp_ranking_skip's integer rule without the [n_rows, 1 + C] matrix between them, so neither n_rows (1 + C) < 2^31 nor the
 * 2^20 columns of one ranking record bound it:  1 <= C < 2^31,  0 <= n_rows < 2^31.
 * PROMISES.  (1) counts and pos_logit equal EXACTLY what tpnet_score_one_to_many(cand = NULL, cand_lo, lead = pos) followed by the
 * integer rule on its logits (column pos[i] - cand_lo skipped where it exists) gives -- promise (1) of that call: a pair's logit has
 * the same bits wherever it is computed, and everything behind the compare is an integer.  (2) Two calls give the same bits.
 * Launches, two or three, all on `stream`, no synchronisation, no atomics, no memset: (a) tpnet_score_one_to_many's kernel as it is,
 * list mode with C = 1 and cand = pos, into pos_logit; (b) the same kernel body with a counting epilogue -- a unit = (row, chunk of
 * KC ids), cut as for tpnet_score_one_to_many; the unit's four integers are summed in LDS and leave the workgroup ONCE, as one
 * 16-byte record (into `scratch`, or straight into counts when every row is one unit); (c) where a row has several units, one wave
 * per row adds its records.  At most about 8192 + n_rows units.
 * scratch: tpnet_score_rank_scratch_bytes(n_rows, C) device bytes, 16-byte aligned (0 for sizes out of range).  pos_logit: device
 * float[n_rows]; counts: device int32[4 n_rows], 16-byte aligned.
 * Served exactly where tpnet_score_one_to_many_supported returns 1; checks and error returns as for tpnet_score_one_to_many (null
 * pointers, C <= 0, n_rows < 0, a range that leaves [0, N), misaligned weights, TPNET_FLAG_PACKED, an unserved state:
 * TPNET_ERR_BAD_ARG, nothing launched; a short scratch: TPNET_ERR_WORKSPACE; n_rows == 0: TPNET_OK).  A src[i] or pos[i] outside
 * [0, N): row i's NaN flag is set (pos_logit[i] is NaN), every other row is untouched, the state's error word is raised. */
size_t tpnet_score_rank_scratch_bytes(int64_t n_rows, int32_t C);
int tpnet_score_rank_range(const tpnet_state* st, const int64_t* src, const int64_t* pos, int64_t cand_lo, int64_t n_rows, int32_t C,
                           double now_time, double lambda, uint32_t flags, const tpnet_mlp* mlp, const float* wd, int32_t ldw,
                           int32_t off, const float* bd, const float* wd2, const float* bd2, int32_t H, void* scratch,
                           size_t scratch_bytes, float* pos_logit, int32_t* counts, void* stream);

/* ---- the K best ids of a whole id range per source, the lists formed in the scoring kernel (additive to ABI 7;
 * csrc/score_fanout.hip).  For row i, over every ADMITTED id c of [cand_lo, cand_lo + C) with
 * q = logit(src[i], c) (the four lines above): ids[i][0 .. K) = the K best candidates, best first, logits[i][..] their logits.
 * Admission: c is left out when c == skip[i] (skip: optional, one id per row; a recommender passes the source itself) or when c is
 * on the row's exclusion list -- excl: optional, [n_rows][F] int64, each row ascending, distinct, -1 padded; n_excl: [n_rows] int32,
 * the true length of the row's list (only its first min(n_excl, F) slots are read): exactly tpnet_neg_filter_lists' output.
 * THE ORDER is one rule on a 64-bit key, larger = better:
 *   hi32 = 0xFFFFFFFF for a NaN logit (NaN sorts FIRST, as in torch.topk: a poisoned state shows up), else the monotone map of the
 *          fp32 bits of q + 0.0f (-0.0 and +0.0 tie): all bits flipped where the sign is set, else the sign bit set;
 *   lo32 = 0xFFFFFFFF - (c - cand_lo);      key = hi32 << 32 | lo32;      key 0 = an empty slot, below every real key
 * -- logit descending, id ascending at equal logits; no two candidates of a row share a key, so the K best and their order are
 * unique.  The returned logit is decoded from the key (-0.0 comes back as +0.0).  Empty slots (fewer than K admitted ids; K > C is
 * allowed): id -1, logit -inf.  info[2 i] = n_valid = min(K, admitted ids); info[2 i + 1] = flags: value 2 when a NaN logit was
 * among the row's admitted candidates, value 8 when the row's exclusion list overflowed (n_excl[i] > F: the ids beyond the first F
 * were NOT left out) -- the ranking records' flag values.
 * Limits: 1 <= C < 2^31, 0 <= n_rows < 2^31, 1 <= K <= 128 (the lists of a workgroup's 32 units are 32 K 8 bytes of LDS: 148 352
 * bytes of dynamic LDS at K = 128, sized by the call's K; every instantiation builds without scratch).  No logit matrix exists: n_rows (1 + C) is not bounded.
 * PROMISES.  (1) ids, logits and info equal EXACTLY what tpnet_score_one_to_many(cand = NULL, cand_lo) on the same range followed
 * by the rule above gives -- promise (1) of that call, and everything behind the logit is an integer.  (2) Two calls agree bit for
 * bit: the K best of distinct keys do not depend on the order they are met in.
 * Launches, one or two, all on `stream`, no synchronisation, no memset, no floating-point atomics: (a) the scoring kernel body with
 * a list epilogue -- a unit = (row, chunk of KC ids), cut as for tpnet_score_one_to_many; one lane per unit walks the row's
 * exclusion list beside the ascending ids (one binary search per unit, one compare per id); the unit's K best keys live in LDS
 * (append, then replace-the-minimum behind a cached threshold) and min(K, KC) of them leave the workgroup ONCE, sorted -- decoded
 * into ids / logits / info when every row is one unit, else as one record in `scratch`; (b) where a row has several units, one
 * workgroup per row selects the K best of its records' keys by a radix select (eight passes at most, linear in the keys) and sorts
 * them.
 * scratch: tpnet_score_topk_scratch_bytes(n_rows, C, K) device bytes = 16 + n_rows nch min(K, KC) 8 where a row has nch > 1 units,
 * else 16 -- at most about (8192 + n_rows) K 8; 0 for sizes out of range.  16-byte aligned.  ids: device int64[n_rows K];
 * logits: device float[n_rows K]; info: device int32[2 n_rows].
 * Served exactly where tpnet_score_one_to_many_supported returns 1; checks and error returns as for tpnet_score_rank_range, and:
 * excl without n_excl or with F < 1, K out of range: TPNET_ERR_BAD_ARG; a short scratch: TPNET_ERR_WORKSPACE; n_rows == 0: TPNET_OK.
 * A src[i] outside [0, N): row i's logits are NaN and its flag 2 is set, its ids are the K smallest admitted ids (every key ties
 * at NaN), every other row is untouched, the state's error word is raised.  A device that refuses the LDS: TPNET_ERR_HIP.
 * NOT measured (profiles/topk_streaming.md): tables beyond the caches, rows wider than 256 floats, K between 10 and 100. */
size_t tpnet_score_topk_scratch_bytes(int64_t n_rows, int32_t C, int32_t K);
int tpnet_score_topk_range(const tpnet_state* st, const int64_t* src, const int64_t* skip, const int64_t* excl, const int32_t* n_excl,
                           int32_t F, int64_t cand_lo, int64_t n_rows, int32_t C, int32_t K, double now_time, double lambda,
                           uint32_t flags, const tpnet_mlp* mlp, const float* wd, int32_t ldw, int32_t off, const float* bd,
                           const float* wd2, const float* bd2, int32_t H, void* scratch, size_t scratch_bytes, int64_t* ids,
                           float* logits, int32_t* info, void* stream);

/* Workspace for tpnet_update / tpnet_run_stream with at most max_edges edges per call. */
size_t tpnet_workspace_bytes(int64_t max_edges, int64_t batch);

/* Workspace for tpnet_run_stream on a table of N rows x d columns x L layers and a stream of up to max_edges edges: the
 * larger of the per-batch plan (capped at a chunk of ~2 M edges; longer streams are walked chunk by chunk) and what the
 * WINDOWED schedule needs: its plan + a version log of 2*L*d*4 bytes per edge of a chunk (at most 16 GiB).  With at
 * least this much, tpnet_run_stream runs a stream of small batches (<= 4096 edges, d % 4 == 0) as a software pipeline
 * over windows of batches -- one launch per window carrying one layer of the update for each of L consecutive windows
 * plus the readouts of the window behind them -- instead of one launch per batch; with less it falls back to per-batch
 * launches.  The two schedules differ in f32 summation order only (both within 1e-4 of the reference). */
size_t tpnet_stream_workspace_bytes(int64_t N, int32_t d, int32_t L, int64_t max_edges, int64_t batch);
/* The same with the version log of a chunk capped at log_cap_bytes (0 = the library's 16 GiB): the windowed schedule costs
 * 2*L*d*4 bytes of log per edge of a chunk (C2: 3 KB per edge, 484 MB for one Wikipedia epoch) plus ~0.5 KB per edge of plan; a
 * caller short of memory trades chunk length (more pipeline fills and drains) for workspace.  tpnet_run_stream takes whatever
 * chunk the workspace it is given holds.  Both functions add, for a stream of 2 .. 64 chunks, the room that keeps every chunk's
 * plan (everything but the log) resident: what tpnet_run_stream_tagged needs to replay such a stream. */
size_t tpnet_stream_workspace_bytes_capped(int64_t N, int32_t d, int32_t L, int64_t max_edges, int64_t batch,
                                           size_t log_cap_bytes);

/* The room tpnet_stream_workspace_bytes(_capped) adds so that a stream of several chunks can be replayed (every chunk's plan kept
 * side by side in front of one version log) is bounded: it is granted only while the whole workspace stays within
 * TPNET_ARENA_MAX_RATIO times the workspace of ONE chunk; beyond that the functions return the one-chunk size (the stream then
 * runs chunk by chunk and is planned again every time).  A 100 M-edge C2 stream asks for 21 GB, not 108. */
#define TPNET_ARENA_MAX_RATIO 3

/* Which schedule tpnet_run_stream / tpnet_run_stream_tagged would take for a stream of E edges in batches of `batch` on a table of
 * N x d x L with these flags and a workspace of ws_bytes: 1 = the windowed pipeline (k_wpipe: one launch per window of batches),
 * 0 = one launch per batch (k_step).  Host-side arithmetic only; lets a caller warm up the kernels the real call will run. */
int tpnet_stream_schedule(int64_t N, int32_t d, int32_t L, int64_t E, int64_t batch, uint32_t flags, size_t ws_bytes);

/* update (models/TPNet.py:67-99) for one batch: src, dst device int64[B], t device double[B] (absolute times,
 * chronological; t[B-1] is the new now_time).  now_time = the module's clock before the call; launch_id = a
 * caller-kept counter, strictly increasing over calls that write the state (start at 1).  The new clock t[B-1] is
 * read on the device; the caller keeps its own host copy of it. */
int tpnet_update(const tpnet_state* st, const int64_t* src, const int64_t* dst, const double* t, int64_t B,
                 double now_time, double lambda, uint32_t launch_id, uint32_t flags, void* workspace,
                 size_t ws_bytes, void* stream);

/* The caller loop of train_link_prediction.py:253-373 / evaluate_models_utils.py:56-184 for a device-resident
 * edge stream: for each chronological batch of `batch` edges (last one partial): readout (src,dst) and
 * (src,neg) on the pre-batch state, then update.  out_pos/out_neg: device float[E][(2L+2)^2] (pre-mlp
 * features); either may be NULL to skip that readout.  neg may be NULL (then out_neg must be NULL).
 * now_time: in = clock before the stream; the new clock is t[E-1] (returned through *t_end_out if non-NULL,
 * which costs one 8-byte device->host copy + stream sync at the end; pass NULL to stay asynchronous).
 * launch_id_base: first launch id; the call uses ids launch_id_base .. launch_id_base + ceil(E/batch) - 1. */
int tpnet_run_stream(const tpnet_state* st, const int64_t* src, const int64_t* dst, const int64_t* neg,
                     const double* t, int64_t E, int64_t batch, double now_time, double lambda,
                     uint32_t launch_id_base, uint32_t flags, float* out_pos, float* out_neg,
                     void* workspace, size_t ws_bytes, double* t_end_out, void* stream);

/* The same loop for a stream that is run AGAIN: train_link_prediction.py:234-253 replays the same chronological stream every
 * epoch (reset_random_projections at the epoch's start, then the same batches), so the plan of the update -- sorted
 * contributions, chains, version references of src / dst -- is the same every epoch; only the negatives are drawn anew.  A call
 * that runs the windowed schedule on the whole stream leaves its plan in the workspace and describes it in tag->built -- the stream
 * is ONE chunk, or (since ABI 6) up to 64 chunks whose plans find room side by side in front of the one version log they share
 * (tpnet_stream_workspace_bytes sizes the workspace for that) --; a later call with equal arguments, the same workspace and the same two signatures skips the planning and only
 * resolves the negatives' readout references again (tag->replayed = 1).  The CALLER vouches with the signatures:
 *   stream_sig: identifies the CONTENTS of src / dst / t (equal value = unchanged arrays; 0 = never replay).  Equal pointers are
 *               not equal arrays: memory that was freed and handed to another array comes back at the same address, so the
 *               value must name the arrays themselves (tpnet_amd keys it on the live tensor objects, their addresses and version
 *               counters) and change whenever one of them was written or replaced;
 *   table_sig:  identifies the table's per-node (current copy, reference time) state before the call -- e.g. one constant
 *               for "just after tpnet_state_init(t0)" per t0, a fresh value after anything else wrote the state (0 = never).
 * A stream on the per-batch schedule that is ONE chunk (up to ~2 M edges) replays its plan too: that plan is a function of src / dst / t,
 * now_time and the flags alone, so stream_sig decides and table_sig is not looked at.
 * A caller that lets anything else use the workspace in between clears the tag (memset 0).  tag == NULL: tpnet_run_stream. */
typedef struct tpnet_plan_tag {
    uint64_t table_sig;   /* in */
    uint64_t stream_sig;  /* in */
    uint64_t replayed;    /* out: 1 = this call reused the plan in the workspace */
    uint64_t built[20];   /* library-owned description of the plan the workspace holds (zero = none) */
} tpnet_plan_tag;
int tpnet_run_stream_tagged(const tpnet_state* st, const int64_t* src, const int64_t* dst, const int64_t* neg,
                            const double* t, int64_t E, int64_t batch, double now_time, double lambda,
                            uint32_t launch_id_base, uint32_t flags, float* out_pos, float* out_neg,
                            void* workspace, size_t ws_bytes, double* t_end_out, void* stream, tpnet_plan_tag* tag);

/* ---- row-sharded multi-GPU building blocks (one process per GPU; the exchange itself is the caller's RCCL call) ----
 * Rows are owned cyclically: owner(n) = n % G.  Every rank holds the full stream; per batch it (1) packs the
 * touched rows it owns, (2) all-gathers them over RCCL, (3) unpacks the other ranks' rows into its local table,
 * (4) runs the fused step restricted to the targets / pairs it owns.  See tpnet_amd/sharded.py. */

/* Plan the update of a whole device-resident stream once (the per-batch item lists tpnet_step_batch consumes).
 * The workspace must hold the whole stream: tpnet_workspace_bytes(E, batch). */
int tpnet_plan_stream(const tpnet_state* st, const int64_t* src, const int64_t* dst, const double* t, int64_t E,
                      int64_t batch, double now_time, double lambda, uint32_t flags, void* workspace, size_t ws_bytes,
                      void* stream);

/* One fused launch for batch b of a planned stream: readout of the pairs whose src node this rank owns (other
 * output rows are left untouched) + update of the targets it owns (id % own_mod == own_rem; own_mod = 1: all;
 * own_mod = 0: ids < own_rem, the owned rows of a compact local table). */
int tpnet_step_batch(const tpnet_state* st, const int64_t* src, const int64_t* dst, const int64_t* neg,
                     const double* t, int64_t E, int64_t batch, int64_t b, double lambda, uint32_t launch_id,
                     uint32_t flags, int32_t own_mod, int32_t own_rem, float* out_pos, float* out_neg,
                     void* workspace, size_t ws_bytes, void* stream);

/* out[k][i][:] = P[i+1][ids[k]] at now_time (i = 0..L-1; layer 0 is static and replicated, never exchanged). */
int tpnet_pack_rows(const tpnet_state* st, const int64_t* ids, int64_t n, double now_time, double lambda, float* out,
                    void* stream);
/* Local copy of row ids[k] <- in[k] (expressed at now_time).  Only for rows owned by another rank. */
int tpnet_unpack_rows(const tpnet_state* st, const int64_t* ids, int64_t n, double now_time, const float* in,
                      void* stream);

/* All peers' rows in one launch after the all-gather: ids = the batch's touched nodes ordered by (owner, node)
 * (device int64[n]), recv = device float [G][maxc][L*d] as gathered, offs = device int64[G] start of each owner's
 * run inside ids.  Rows owned by `me` are skipped. */
int tpnet_unpack_gathered(const tpnet_state* st, const int64_t* ids, int64_t n, double now_time, const float* recv,
                          int64_t maxc, const int64_t* offs, int32_t G, int32_t me, void* stream);

/* Compact row shards: a rank's table holds ONLY the rows it owns (local row = global id / G) followed by halo rows, which
 * per batch receive copies of the other ranks' rows that the batch reads.  Layer 0 is sharded like the others, so whole
 * bundles travel:
 *   tpnet_pack_bundles:   out[k][i][:] = P[i][ids[k]] at now_time, i = 0..L          (ids: LOCAL rows of this rank's table)
 *   tpnet_unpack_bundles: list entry k of the batch's touched nodes (ordered by (owner, node); offs[r] = start of owner r's run)
 *                         sits at recv[r][k - offs[r]] ([G][maxc][L+1][d] as all-gathered) and is written to local row
 *                         local_ids[k] (< 0: skip): layer 0 into p0, layers 1..L into the row's current copy, as of now_time.
 * tpnet_step_batch with own_mod = 0 then restricts the step to the targets / pair sources with local id < own_rem. */
int tpnet_pack_bundles(const tpnet_state* st, const int64_t* ids, int64_t n, double now_time, double lambda, float* out,
                       void* stream);
int tpnet_unpack_bundles(const tpnet_state* st, const int64_t* local_ids, int64_t n, double now_time, const float* recv,
                         int64_t maxc, const int64_t* offs, int32_t G, void* stream);

/* One batch of the compact row-sharded stream in ONE call, the exchange included: tpnet_pack_bundles(pack_ids, n_pack) into
 * `send` ([maxc][(L+1)*d], padded), ONE RCCL all-gather into `recv` ([G][maxc][(L+1)*d]) on `stream`, tpnet_unpack_bundles
 * (unpack_ids, n_unpack, offs), then tpnet_step_batch(b) with own_mod = 0, own_rem = n_owned.  comm: a communicator from
 * tpnet_rccl_comm_create (NULL, or maxc = 0: no exchange, just the step).  RCCL is resolved at run time (dlopen of lib_path,
 * else "librccl.so" -- the library PyTorch already loaded): tpnet_rccl_unique_id on one rank, the 128 bytes broadcast by the
 * caller, tpnet_rccl_comm_create on every rank (collective: ncclCommInitRank). */
int tpnet_rccl_unique_id(const char* lib_path, void* id128);
int tpnet_rccl_comm_create(const char* lib_path, const void* id128, int32_t nranks, int32_t rank, void** comm);
int tpnet_rccl_comm_destroy(void* comm);
int tpnet_rows_step(const tpnet_state* st, void* comm, const int64_t* pack_ids, int64_t n_pack, float* send, float* recv,
                    int64_t maxc, const int64_t* unpack_ids, int64_t n_unpack, const int64_t* offs, int32_t G,
                    double now_time, const int64_t* src, const int64_t* dst, const int64_t* neg, const double* t, int64_t E,
                    int64_t batch, int64_t b, double lambda, uint32_t launch_id, uint32_t flags, int32_t n_owned,
                    float* out_pos, float* out_neg, void* workspace, size_t ws_bytes, void* stream);

/* The same batch with the TARGETED exchange: every owned row travels only to the ranks that read it, as two
 * messages (layer 0; layers 1..L decayed to now_time) that the reader receives STRAIGHT INTO the halo rows of its p0 and q
 * arrays -- so a sharded batch is two launches (pack, step) around one grouped ncclSend / ncclRecv, with no unpack.
 *   pack_ids:  device int64, the LOCAL rows to send, ordered by (reader rank, node): send_cnt[r] of them for rank r;
 *   send_cnt / recv_cnt: HOST int64[G] (entry `me` = 0); the rows from rank r land in halo rows
 *              [n_owned + sum(recv_cnt[:r]), ...) in the sender's order -- the local ids the caller relabelled the batch with;
 *   send_p0 [sum(send_cnt)][d], send_q [sum(send_cnt)][L*d]: device scratch.
 * tpnet_pack_split is the pack launch alone (a caller that moves the rows with another transport, e.g. the gloo tests): it
 * also stamps halo rows [halo0, halo0 + n_halo) as "as of now_time". */
int tpnet_pack_split(const tpnet_state* st, const int64_t* ids, int64_t n, double now_time, double lambda, float* out_p0,
                     float* out_q, int64_t halo0, int64_t n_halo, void* stream);
int tpnet_rows_step_targeted(const tpnet_state* st, void* comm, const int64_t* pack_ids, float* send_p0, float* send_q,
                             const int64_t* send_cnt, const int64_t* recv_cnt, int32_t G, int32_t me, double now_time,
                             const int64_t* src, const int64_t* dst, const int64_t* neg, const double* t, int64_t E,
                             int64_t batch, int64_t b, double lambda, uint32_t launch_id, uint32_t flags, int32_t n_owned,
                             float* out_pos, float* out_neg, void* workspace, size_t ws_bytes, void* stream);
/* Batches [b0, b1) of a stream through tpnet_rows_step_targeted in ONE call (the per-batch loop of tpnet_amd/sharded.py was one
 * FFI crossing, ~10 us of host time, per batch): pack_start[b] = offset of batch b's rows in pack_ids, send_cnt / recv_cnt
 * HOST int64[nb][G], t_last HOST double[nb] (the clock batch b leaves: its rows of batch b + 1 are packed at it), launch ids
 * launch_id_base + b. */
int tpnet_rows_stream_targeted(const tpnet_state* st, void* comm, const int64_t* pack_ids, const int64_t* pack_start,
                               float* send_p0, float* send_q, const int64_t* send_cnt, const int64_t* recv_cnt, int32_t G,
                               int32_t me, double now_time, const double* t_last, const int64_t* src, const int64_t* dst,
                               const int64_t* neg, const double* t, int64_t E, int64_t batch, int64_t b0, int64_t b1,
                               double lambda, uint32_t launch_id_base, uint32_t flags, int32_t n_owned, float* out_pos,
                               float* out_neg, void* workspace, size_t ws_bytes, void* stream);

/* The targeted exchange's plan on the device (what tpnet_rows_step_targeted's callers need per batch): for rank `me` of G (owner(n)
 * = n % G), from the stream's device arrays, two launches and no synchronisation:
 *   recv_keys [nb][cap] uint32 (cap = tpnet_xplan_capacity()): the distinct remote nodes the rank reads in batch b, as (owner <<
 *       bits(N) | node), ascending = the order the peers' messages land in the halo rows;
 *   pack_ids  [nb][cap] int64: the local rows (node / G) the rank sends in batch b, ordered (reader, node), a row once per reader;
 *   cnt       [nb][2][G] int64: rows received from each owner / rows sent to each reader (the host reads these back);
 *   status    [2] uint32: ids outside [0, N) seen; batches whose lists exceeded cap (then the caller plans another way);
 *   local_src / local_dst / local_neg [E] int64: every endpoint relabelled (owned: n / G; received in its batch: n_owned + its
 *       place in the batch's receive list; else n_owned).
 * TPNET_ERR_BAD_ARG when bits(N) + bits(G) > 31 or G > 64 (the caller plans another way). */
int64_t tpnet_xplan_capacity(void);
int tpnet_xplan_targeted(const int64_t* src, const int64_t* dst, const int64_t* neg, int64_t E, int64_t batch, int64_t N, int32_t G,
                         int32_t me, int32_t n_owned, uint32_t* recv_keys, int64_t* pack_ids, int64_t* cnt, uint32_t* status,
                         int64_t* local_src, int64_t* local_dst, int64_t* local_neg, void* stream);

/* The same plan for batches whose lists exceed tpnet_xplan_capacity() (C4's law over 8 ranks: ~25 000 rows received per batch of
 * 80 000 edges): one device-wide radix sort of the call's (list, batch, peer, node) keys instead of a workgroup per batch.  The
 * lists are COMPACT: pack_ids holds the local rows to send, all batches back to back in (batch, reader, node) order (at most 3 E;
 * batch b starts at the sum of the earlier batches' send counts), and a remote node's halo row is n_owned + its place in its
 * batch's receive list ((owner, node) order) -- both as tpnet_rows_stream_targeted consumes them.  cnt / status / local_* as
 * above.  scratch: tpnet_xplan_large_bytes(E, batch, G) device bytes.  Synchronises `stream` ONCE in the middle (the number of
 * keys sizes the sort); the caller reads cnt / status back afterwards as for tpnet_xplan_targeted. */
size_t tpnet_xplan_large_bytes(int64_t E, int64_t batch, int32_t G);
int tpnet_xplan_targeted_large(const int64_t* src, const int64_t* dst, const int64_t* neg, int64_t E, int64_t batch, int64_t N,
                               int32_t G, int32_t me, int32_t n_owned, void* scratch, size_t scratch_bytes, int64_t* pack_ids,
                               int64_t* cnt, uint32_t* status, int64_t* local_src, int64_t* local_dst, int64_t* local_neg,
                               void* stream);

/* ---- a row shard on the WINDOWED pipeline (ABI 7; csrc/wshard.hip) -------------------------------------------
 * The per-batch shard above exchanges rows and launches a kernel per batch.  Here one chunk of the stream (the whole call) runs as
 * the software pipeline of tpnet_run_stream's windowed schedule -- one launch per window of batches -- and the ranks meet once per
 * launch: every node the chunk touches gets ONE halo row for the whole chunk (filled at its start with the owner's pre-chunk row),
 * every rank plans from the whole stream and derives, without a request round, which of its runs' results another rank reads; after
 * each launch those rows are packed, exchanged with ONE grouped ncclSend / ncclRecv, and unpacked into the version log.  A log slot
 * travels bit for bit: G shards compute what one GPU computes on the windowed schedule.
 *   st: the rank's LOCAL table (n_owned rows + halo rows: tpnet_state::N = n_owned + halo capacity); src / dst / neg: GLOBAL ids.
 *   tpnet_wshard_plan returns TPNET_OK and *out, or 1 = this call is not served (batches beyond 8 192 edges, fewer than 4 batches,
 *   more remote nodes in the chunk than halo rows, a table too large for the dense planner, exact / packed modes ...): the caller
 *   takes tpnet_rows_stream_targeted.  It synchronises `stream` twice (halo counts, message counts).  A tpnet_wshard is a HOST object
 *   (counts and views into the caller's workspace; the second thing besides tpnet_stage this library allocates); device memory is
 *   the caller's: workspace (tpnet_wshard_workspace_bytes) and the exchange buffers (tpnet_wshard_info -> tpnet_wshard_set_buffers).
 *   phases of begin / step (bit mask): 1 = launch the pipeline step, 2 = pack, 4 = exchange over `comm` (tpnet_rccl_comm_create),
 *   8 = unpack; a caller with another transport runs 2, moves the rows itself (sendbuf rows [sum of send_cnt[j][:r], +send_cnt[j][r])
 *   go to peer r's recvbuf rows [sum of ITS recv_cnt[j][:me], ...); the chunk's halo rows: send_p0 / send_q of owner o to halo rows
 *   [n_owned + hstart(o), ...) of p0 and of copy 0 of q, hstart(o) = sum of chunk_cnt[o'] over o' < o, o' != me), then 8. */
typedef struct tpnet_wshard tpnet_wshard;
size_t tpnet_wshard_workspace_bytes(int64_t n_local, int32_t d, int32_t L, int64_t E, int64_t batch, int32_t G, int32_t n_owned);
int tpnet_wshard_plan(const tpnet_state* st, const int64_t* src, const int64_t* dst, const int64_t* neg, const double* t, int64_t E,
                      int64_t batch, int64_t N_global, int32_t G, int32_t me, int32_t n_owned, double now_time, double lambda,
                      uint32_t flags, int32_t want_pos, int32_t want_neg, void* workspace, size_t ws_bytes, void* stream,
                      tpnet_wshard** out);
int tpnet_wshard_info(const tpnet_wshard* w, int64_t* n_steps, int64_t* halo_rows, int64_t* max_send_rows, int64_t* max_recv_rows,
                      const int64_t** chunk_cnt, const int64_t** send_cnt, const int64_t** recv_cnt);
int tpnet_wshard_set_buffers(tpnet_wshard* w, float* send_p0, float* send_q, float* sendbuf, float* recvbuf);
int tpnet_wshard_begin(tpnet_wshard* w, void* comm, uint32_t phases, void* stream);
int tpnet_wshard_step(tpnet_wshard* w, void* comm, int64_t j, uint32_t phases, float* out_pos, float* out_neg, void* stream);
int tpnet_wshard_finish(tpnet_wshard* w, uint32_t launch_id, void* stream);
/* begin + every step + finish in one call (comm may be NULL with one rank) */
int tpnet_wshard_run(tpnet_wshard* w, void* comm, float* out_pos, float* out_neg, uint32_t launch_id, void* stream);
void tpnet_wshard_destroy(tpnet_wshard* w);

/* ---- the step in front of the path: 'recent' historical-neighbour sampling on the device ----------
 * Replaces NeighborSampler('recent') + get_neighbor_sampler (utils/utils.py:82-224, 293-312): undirected adjacency,
 * per node sorted by time (stable: ties keep the reference's append order), neighbours strictly BEFORE the query
 * time, the K most recent at the back of the row, zeros in front. */
size_t tpnet_sampler_bytes(int64_t E, int64_t num_nodes);
/* sampler: caller-owned device buffer of tpnet_sampler_bytes(E, num_nodes); src/dst/t (and optional edge_ids, NULL =
 * 1..E) are device arrays of E interactions; num_nodes = largest node id + 1. */
int tpnet_sampler_build(void* sampler, size_t sampler_bytes, const int64_t* src, const int64_t* dst, const double* t,
                        const int64_t* edge_ids, int64_t E, int64_t num_nodes, void* stream);
/* out_ids [n][K] int64 (required), out_eids [n][K] int64 and out_times [n][K] double (optional, may be NULL). */
int tpnet_sample_recent(const void* sampler, int64_t E, int64_t num_nodes, const int64_t* node_ids, const double* times,
                        int64_t n, int32_t K, int64_t* out_ids, int64_t* out_eids, double* out_times, void* stream);

/* ---- the reference's two random strategies on the same CSR ('uniform', 'time_interval_aware': utils/utils.py:123-224) ----------
 * Per query: the n interactions of the node strictly before the query time (the cut of tpnet_sample_recent), K positions drawn
 * WITH replacement, the K triples written in ascending CSR position (a time sort; ties in the CSR's append order).  n == 0 or a
 * node id outside [0, num_nodes): a row of zeros.
 *   uniform:              every position with probability 1/n.
 *   time_interval_aware:  P(j) ~ w_j = exp((double)(float)p_j), p_j = E_j / cumsum(E)_j over the node's WHOLE list,
 *                         E_j = exp(time_scaling_factor * (t_j - t_last)) in float64; w_j = 0 where p_j is NaN; a prefix whose
 *                         weights are all 0 is drawn uniformly.  This is the reference's softmax(float32(p[:n])) with NaN -> -1e10.
 * Random numbers: Philox4x32-10, key = (seed & 0xffffffff, seed >> 32), counter = (row & 0xffffffff, row >> 32, slot >> 2,
 * call_index), word used = out[slot & 3]; row = the query's index within the call.  A draw depends on (seed, call_index, row,
 * slot) alone -- reproducible per seed, NOT numpy's RandomState.choice stream.  From the word r: uniform position =
 * (uint64(r) * n) >> 32; weighted: x = (r + 0.5) * 2^-32 * W[cut-1], position = first j of the prefix with W[j] >= x, W = the
 * per-node inclusive prefix sum of w (float64). */
size_t tpnet_sampler_weights_bytes(int64_t E);          /* W table + its build scratch */
/* weights: caller-owned device buffer of tpnet_sampler_weights_bytes(E); `sampler` was built by tpnet_sampler_build on the same
 * stream (or the build has finished).  Once per sampler and time_scaling_factor. */
int tpnet_sampler_build_weights(const void* sampler, int64_t E, int64_t num_nodes, double time_scaling_factor, void* weights,
                                size_t weights_bytes, void* stream);
/* weights NULL = uniform.  1 <= K <= 256.  out_eids / out_times may be NULL as in tpnet_sample_recent. */
int tpnet_sample_random(const void* sampler, const void* weights, int64_t E, int64_t num_nodes, const int64_t* node_ids,
                        const double* times, int64_t n, int32_t K, uint64_t seed, uint32_t call_index, int64_t* out_ids,
                        int64_t* out_eids, double* out_times, void* stream);

/* ---- the reference's negative edge sampler on the device (additive to ABI 7; csrc/negsampler.hip) ----------
 * NegativeEdgeSampler (utils/utils.py:315-505), strategies 'random', 'historical', 'inductive'.  With the sampler's own E edges
 * (src, dst, t), a batch window [t0, t1] and the batch's own B pairs:
 *   candidates C: the unique edges e with first_time(e) <= t0 and no occurrence in [t0, t1] (both ends inclusive); 'inductive': and
 *                 first_time(e) > last_observed_time.  M = |C|, cand[0..M) = C in ascending (src << 32 | dst) order.
 *   size <= M:    out[i] = cand[perm(M, tag 0, i)]: `size` distinct candidates, uniform.
 *   size >  M:    F = size - M, Us / Ud = the sorted unique src / dst ids, D = |Us| |Ud|, index x = the pair (Us[x / |Ud|], Ud[x % |Ud|]).
 *                 Trial slot j < min(D, F + B) holds x = perm(D, tag 1, j); it is valid when its pair is none of the batch's B pairs.
 *                 At least F valid trials (always so when P = |Us x Ud - batch pairs| >= F): the first F valid ones in slot order fill
 *                 out[0..F) -- distinct.  Otherwise the whole domain was enumerated and P < F: out[i] = valid[(word(2, i, 0) * P) >> 32],
 *                 valid = the P valid pairs in slot order (with replacement).  P = 0: out[0..F) = -1 and the sampler's error word is
 *                 set (tpnet_neg_check).  out[F + j] = cand[j], j < M: ALL candidates follow the fill.
 *   'random':     out_src[i] = Us[(word(3, i, 0) * |Us|) >> 32], out_dst[i] = Ud[(word(4, i, 0) * |Ud|) >> 32].
 * word(tag, a, b) = word 0 of Philox4x32-10 with counter (a, b, tag, call_index) and key (seed & 0xffffffff, seed >> 32).
 * perm(n, tag, i), a keyed permutation of [0, n) evaluated per slot in O(1) memory: n <= 1: 0.  Else bits = bitlength(n - 1), a = bits / 2
 * (rounded down), b = bits - a, x = i; repeat { (L, R) = (x >> b, x & (2^b - 1)); three times, r = 0, 2, 4: L ^= word(tag, R, r) & (2^a - 1),
 * then R ^= word(tag, L, r + 1) & (2^b - 1); x = L << b | R } until x < n.  (Six rounds of an alternating Feistel network: each xor is
 * undone by itself, so the network is a bijection of [0, 2^bits), and walking its cycle back into [0, n) keeps it one; 2^bits < 2 n, so
 * fewer than two passes on average.)
 * The draws follow the reference's probabilities and depend on (seed, call_index, slot) alone; they are NOT numpy's RandomState.choice
 * stream, and the order inside C (Python-set order in the reference) is the key order here.
 *
 * tpnet_neg_build, once per sampler: sorts the edges by (src, dst, time) and writes, into the caller-owned device buffer `neg` of
 *   tpnet_neg_bytes(E): the table of the U unique edges (key, first time, start of the ascending occurrence-time list, observed bit =
 *   first_time <= last_observed_time when has_observed) and Us / Ud.  src / dst / t: device arrays of E (t may be NULL: all times 0);
 *   1 <= E < 2^30; every id in [0, 2^31), else TPNET_ERR_INDEX.  counts: HOST int64[3] = {U, |Us|, |Ud|}; the call synchronises `stream`.
 * tpnet_neg_uniques copies Us / Ud (n_src / n_dst entries, as counts gave them) to device arrays of the caller.
 * tpnet_neg_sample: 3 launches (flag + tile sums, scan of the sums, compaction) + 1 (pick) on `stream` -- 'random': 1 -- and no
 *   synchronisation; a batch of more than 1024 pairs adds a key sort (smaller ones are looked up in an LDS table).  batch_src / batch_dst:
 *   device arrays of B (not read by 'random', and read only by the fill); scratch: tpnet_neg_scratch_bytes(E, size, B) device bytes (not
 *   needed by 'random'); out_src / out_dst: device int64[size].  size, B < 2^31.  size == 0: TPNET_OK, nothing launched.
 * tpnet_neg_check copies the error word to the host (synchronises), clears it if set and returns TPNET_ERR_BAD_ARG: a fill found every pair
 *   of Us x Ud in its batch (possible only when |Us| |Ud| <= B).
 * Null pointers and sizes out of range: TPNET_ERR_BAD_ARG (size helpers: 0), nothing launched. */
#define TPNET_NEG_RANDOM 0
#define TPNET_NEG_HISTORICAL 1
#define TPNET_NEG_INDUCTIVE 2
size_t tpnet_neg_bytes(int64_t E);
int tpnet_neg_build(void* neg, size_t neg_bytes, const int64_t* src, const int64_t* dst, const double* t, int64_t E,
                    double last_observed_time, int32_t has_observed, int64_t* counts, void* stream);
int tpnet_neg_uniques(const void* neg, int64_t E, int64_t n_src, int64_t n_dst, int64_t* unique_src, int64_t* unique_dst,
                      void* stream);
size_t tpnet_neg_scratch_bytes(int64_t E, int64_t size, int64_t B);
int tpnet_neg_sample(void* neg, int64_t E, int32_t strategy, int64_t size, const int64_t* batch_src, const int64_t* batch_dst,
                     int64_t B, double t0, double t1, uint64_t seed, uint32_t call_index, void* scratch, size_t scratch_bytes,
                     int64_t* out_src, int64_t* out_dst, void* stream);
int tpnet_neg_check(void* neg, void* stream);

/* ---- per-query candidates of the ranking protocol (additive to ABI 7; csrc/negsampler.hip) -------------------
 * tpnet_neg_sample_many: every query i = (s, d, t) of a batch of B positives gets its own row of Q candidate destinations,
 * cand[i*Q .. i*Q+Q), of which the first n_hist[i] <= Qh are destinations `s` was seen with earlier.  A rule of its own: no strategy,
 * no batch window; it reads the table tpnet_neg_build made.  word / perm: as defined above; perm_i = perm under the key
 * (seed & 0xffffffff, (seed >> 32) ^ i) -- the query's index within the call enters the second word of the Philox key, the counter
 * stays (a, b, tag, call_index) -- so a row depends on (seed, call_index, i) and its own (s, d, t) alone, not on B or on other rows.
 *   exclusion:   a destination d' is excluded when d' == d, or when the table holds an occurrence of (s, d') at time exactly t (another
 *                positive of the same instant).
 *   historical:  e_0 .. e_{R-1} = the unique edges with source s in ascending destination order.  Visit e_{perm_i(R, tag 5, j)},
 *                j = 0, 1, ...: entry j is eligible when its destination is not excluded and its first occurrence time is < t.  The
 *                first Qh eligible ones, in visiting order, fill cand[i, 0 .. h_i); n_hist[i] = h_i = min(Qh, #eligible).
 *   random:      visit Ud[perm_i(|Ud|, tag 6, j)], j = 0, 1, ...; accept a destination that is not excluded and not one of the row's
 *                historical picks, in visiting order, until the row is full or all of Ud has been visited.  Slots that cannot be filled
 *                hold -1: only when fewer than Q admissible distinct destinations exist.
 * So a row's entries (other than -1) are distinct, never the true destination and never a same-instant positive of the source.
 * One wave per query (64 visiting slots per step, ballot compaction, binary searches into the table and the occurrence lists), one
 * launch on `stream`, no scratch, no synchronisation.  batch_src / batch_dst: device int64[B], batch_t: device float64[B]; cand: device
 * int64[B*Q]; n_hist: device int32[B].  1 <= Q < 2^16, 0 <= Qh <= Q, 0 <= B < 2^31; B == 0: TPNET_OK, nothing launched.  Null pointers
 * and sizes out of range: TPNET_ERR_BAD_ARG, nothing launched. */
int tpnet_neg_sample_many(const void* neg, int64_t E, const int64_t* batch_src, const int64_t* batch_dst, const double* batch_t,
                          int64_t B, int32_t Q, int32_t Qh, uint64_t seed, uint32_t call_index, int64_t* cand, int32_t* n_hist,
                          void* stream);

/* ---- per-query filter lists of the all-node ranking protocol (additive to ABI 7; csrc/negsampler.hip) -------
 * tpnet_neg_filter_lists: query i = (s, d, t) gets the destinations d' != d with lo <= d' < hi that `mode` excludes from its
 * candidates, read from the table tpnet_neg_build made:
 *   TPNET_FILTER_SAME_TIME   d' is excluded when the table holds an occurrence of (s, d') at time exactly t: the exclusion rule of
 *                            tpnet_neg_sample_many, so the sampled and the all-node protocol agree about what a negative is
 *   TPNET_FILTER_KNOWN       d' is excluded when the table holds (s, d') at any time: the filtered protocol papers report
 * fil[i*F .. i*F+F): the excluded destinations, ascending and distinct, the rest of the row -1.  n_fil[i]: the TRUE number of
 * excluded destinations, which may exceed F -- then the row holds the F smallest, and a consumer treats n_fil[i] > F as overflow
 * (tpnet_lp_ranking_counts: flag value 8).  One wave per query walks the source's unique edges in destination order (64 per step,
 * ballot compaction; same_time: one binary search in the edge's occurrence list), one launch on `stream`, no scratch, no
 * synchronisation.  batch_src / batch_dst: device int64[B], batch_t: device float64[B]; fil: device int64[B*F]; n_fil: device int32[B].
 * 1 <= F < 2^16, 0 <= B < 2^31, lo <= hi; B == 0: TPNET_OK, nothing launched.  Null pointers, another mode and sizes out of range:
 * TPNET_ERR_BAD_ARG, nothing launched. */
#define TPNET_FILTER_SAME_TIME 1
#define TPNET_FILTER_KNOWN 2
int tpnet_neg_filter_lists(const void* neg, int64_t E, const int64_t* batch_src, const int64_t* batch_dst, const double* batch_t,
                           int64_t B, int32_t mode, int64_t lo, int64_t hi, int32_t F, int64_t* fil, int32_t* n_fil, void* stream);

/* ---- a batch's link-prediction metrics on the device (additive to ABI 7; csrc/metrics.hip) ------------------
 * What the reference's evaluation loop brings to the host per batch (evaluate_models_utils.py:187-193, utils/metrics.py:8-22):
 * BCEWithLogitsLoss(...).item() and sklearn's average_precision_score / roc_auc_score on predicts.sigmoid().cpu().
 * p[0..P) = the fp32 scores of the positives, q[0..N) = those of the negatives.  Per positive i, three integers:
 *   a_i = #{ j : p_j >= p_i } (i itself included),  b_i = #{ k : q_k >= p_i },  c_i = #{ k : q_k == p_i }
 * and then, in float64:
 *   AP  = (1 / P) sum_i a_i / (a_i + b_i)
 *   U2  = sum_i (2 (N - b_i) + c_i)          (int64, exact)
 *   AUC = U2 / (2 P N)
 * -- sklearn's definitions with ties: tied scores share one threshold (at the threshold p_i, a_i of the a_i + b_i scores at or above it
 * are positives; the recall step of a threshold, spread over the positives tied at it, is 1 / P each), and AUC counts a tied
 * (positive, negative) pair as half.  Comparisons are IEEE: -0.0 ties with +0.0.
 *   loss = (1 / (P + N)) sum over the P + N logits x with label y (1: positive, 0: negative) of max(x, 0) - x y + log1p(exp(-|x|)),
 *          every term evaluated in float64 from the fp32 logit, the terms summed in float64.
 * The a / b / c counts are combined across workgroups with integer atomics, the float64 sums run in a fixed order -- AP: entry k,
 * k + 1024, ... per thread, then a halving tree over 1024 threads; loss: per chunk of the counting kernel (256 consecutive logits, positives
 * before negatives) a halving tree over 256 threads, then the chunks' sums the same way over 1024 threads --: the same input gives the
 * same bits every time.
 * Degenerate batches are reported, not refused:  P == 0 or N == 0: AP = AUC = NaN, flag bit 0 (value 1), U2 = 0;  any NaN among the
 * scores: AP = AUC = NaN, flag bit 1 (value 2) -- a NaN compares false both ways, U2 is what the counts then give;  P + N == 0: the
 * loss is 0 / 0.
 * record: ONE 64-byte device record, 8-byte aligned:
 *   { double loss, double ap, double auc, int64 u2, int64 n_pos, int64 n_neg, int64 flags, int64 reserved (0) }
 * pos_logit / neg_logit may be NULL: no loss is computed, record.loss = NaN (the pointer of an EMPTY side is not looked at).
 * scratch: tpnet_lp_metrics_scratch_bytes(n_pos, n_neg) device bytes, 8-byte aligned (the 3 P counters, a NaN word, one partial loss
 * per chunk; not needed when P + N is 0).
 * Launches, all on `stream`: the counters' fill, the counting kernel on a (256 positives) x (256 scores) grid -- its first row
 * of workgroups also sums the loss terms and looks for NaN --, one finish workgroup; no host copy, no synchronisation.  The counting is O(P (P + N)) and meant for a batch: P + N > 2^18, a negative size or a missing
 * pointer: TPNET_ERR_BAD_ARG (the size helper: 0), nothing launched; a short scratch: TPNET_ERR_WORKSPACE. */
size_t tpnet_lp_metrics_scratch_bytes(int64_t n_pos, int64_t n_neg);
int tpnet_lp_metrics(const float* pos_score, int64_t n_pos, const float* neg_score, int64_t n_neg, const float* pos_logit,
                     const float* neg_logit, void* scratch, size_t scratch_bytes, void* record, void* stream);

/* ---- a TRAINING batch's loss on the device (additive to ABI 7; csrc/metrics.hip) ----------------------------
 * What the reference's training loop does behind the decoder (train_link_prediction.py:375-386): BCEWithLogitsLoss on
 * cat(positives, negatives) against labels 1 / 0, loss.item(), get_link_prediction_metrics(predicts.sigmoid(), labels), loss.backward().
 * tpnet_lp_train_loss is tpnet_lp_metrics -- the same arguments, the same three launches, the same scratch
 * (tpnet_lp_metrics_scratch_bytes), bit for bit the same record -- and two more outputs:
 *   pos_grad[n_pos], neg_grad[n_neg]: d(loss) / d(logit) = (sigmoid(x) - y) / (P + N), formed from the fp32 LOGIT in float64 in the
 *     branch that does not cancel -- a positive: -1 / (1 + exp(x)) / (P + N), a negative: 1 / (1 + exp(-x)) / (P + N) -- and rounded once
 *     to fp32.  Where an fp32 sigmoid has saturated to 1 or 0, sigmoid(x) - y in fp32 is 0; this gradient keeps its relative accuracy
 *     down to fp32's subnormals.  A NaN logit gives a NaN gradient for that element only.  They are written, one plain store per
 *     element, by the workgroups of the counting kernel's first row, which evaluate that logit's loss term anyway.
 *   loss_out: ONE float, 4-byte aligned: (float)record.loss, written by the finish workgroup.
 * The logits of every non-empty side are required here (they are optional for tpnet_lp_metrics).  TPNET_ERR_BAD_ARG, nothing
 * launched: what tpnet_lp_metrics refuses; n_pos + n_neg == 0; a null logit or gradient pointer of a non-empty side (an EMPTY side's
 * are not looked at); a null or misaligned loss_out. */
int tpnet_lp_train_loss(const float* pos_score, int64_t n_pos, const float* neg_score, int64_t n_neg, const float* pos_logit,
                        const float* neg_logit, void* scratch, size_t scratch_bytes, void* record, float* pos_grad, float* neg_grad,
                        float* loss_out, void* stream);

/* ---- a batch's one-vs-many ranking record on the device (additive to ABI 7; csrc/metrics.hip) ----------------
 * logits: [B, C1] fp32 row-major, one query per row; column 0 is the positive's logit p, column 1 + c a candidate's logit q_c, valid
 * when cand_or_null == NULL or cand_or_null[i*(C1-1) + c] >= 0 (the -1 slots of tpnet_neg_sample_many are absent candidates).
 * Per query i, over its valid candidates:  g_i = #{q > p},  e_i = #{q == p},  m_i = 2 + 2 g_i + e_i = twice the rank (ties get the
 * mean of the optimistic and the pessimistic rank).  Comparisons are IEEE on the fp32 logits as given -- no sigmoid, so a saturating
 * sigmoid adds no ties.  A query is NOT counted when p is NaN or a valid candidate's logit is NaN (flag bit 1, value 2; a NaN under
 * an absent slot is not looked at), or when it has no valid candidate (flag bit 2, value 4).  n = the counted queries.
 * record: ONE 64-byte device record, 8-byte aligned:
 *   { double mrr = (1/n) sum 2/m_i, double hits1 = #{m_i <= 2 k1} / n, double hits2 (k2), double hits3 (k3),
 *     int64 m_sum = sum m_i, int64 n, int64 n_valid_candidates (over all B queries, counted or not), int64 flags }
 * n == 0: the four doubles are NaN and flag bit 0 (value 1) is set.  Each hits word is ONE division of an integer count by n.
 * Two launches on `stream`: one wave per query strided over its C1 columns (integer counts) writes m_i (0: not counted), the
 * query's valid count and its flags into scratch; one finish workgroup sums 2/m_i in float64 in a fixed order (thread k: queries k,
 * k + 1024, ...; then a halving tree) -- no floating-point atomics: the same input gives the same record bits on every run.
 * scratch: tpnet_lp_ranking_scratch_bytes(B, C1) device bytes, 8-byte aligned (not needed when B == 0).  0 <= B < 2^31,
 * 1 <= C1 <= 2^20, k1, k2, k3 >= 1.  A size out of range, a null or misaligned pointer: TPNET_ERR_BAD_ARG (the size helper: 0),
 * nothing launched; a short scratch: TPNET_ERR_WORKSPACE. */
size_t tpnet_lp_ranking_scratch_bytes(int64_t B, int32_t C1);
int tpnet_lp_ranking(const float* logits, int64_t B, int32_t C1, const int64_t* cand_or_null, int32_t k1, int32_t k2, int32_t k3,
                     void* scratch, size_t scratch_bytes, int64_t* record, void* stream);
/* The same record with ONE absent candidate column per query (ranking against all nodes: the true destination sits among the
 * candidates, and a [B, C1 - 1] matrix of marks to drop one column per row would be larger than the logits).  skip_col: [B] int64 on
 * the device, 8-byte aligned; candidate column skip_col[i] (0-based among the C1 - 1 candidates; -1 or any value outside
 * [0, C1 - 1): none) of query i is treated as absent -- not ranked, not counted in n_valid_candidates, a NaN under it is not looked
 * at.  Same scratch size, same finish kernel, same checks as tpnet_lp_ranking; a null or misaligned skip_col with B > 0:
 * TPNET_ERR_BAD_ARG. */
int tpnet_lp_ranking_skip(const float* logits, int64_t B, int32_t C1, const int64_t* skip_col, int32_t k1, int32_t k2, int32_t k3,
                          void* scratch, size_t scratch_bytes, int64_t* record, void* stream);
/* The same record from COUNTS (tpnet_score_rank_range's output), with an optional per-query filter.  counts: [B][4] int32 =
 * {g, e, nv, flags} per query, 16-byte aligned; pos_logit: [B] fp32, the positive's logit p.  fil_logits == NULL: no filter
 * (fil_ids, n_fil and F are not looked at).  Else fil_logits [B][F] fp32, fil_ids [B][F] int64 and n_fil [B] int32 as
 * tpnet_neg_filter_lists lays them out, fil_logits[i][j] = the logit of (query i's source, fil_ids[i][j]) -- by promise (1) of
 * tpnet_score_one_to_many the bits the counting kernel compared -- and per query over the slots j < min(n_fil, F) with
 * fil_ids >= 0 (a logit under another slot is not looked at):
 *   g_f = #{fil_logit > p},  e_f = #{fil_logit == p},  m_i = 2 + 2 (g - g_f) + (e - e_f),  valid candidates = nv - n_fil
 * -- exact when every listed id is one of the query's counted candidates, which tpnet_neg_filter_lists on the same range promises.
 * A query is NOT counted when counts' flag value 2 is set or a looked-at filter logit is NaN (flag value 2), when n_fil > F (a NEW
 * flag, value 8: filter overflow -- the list is incomplete, so the filtered rank is unknown) or when no valid candidate is left
 * (value 4).  The call writes the three words per query the finish kernel reads (one launch, one thread per query), then launches
 * tpnet_lp_ranking's finish kernel: the record, its summation order and flags 1 / 2 / 4 are tpnet_lp_ranking's (the kernel carries
 * value 8 through as it carries 2 and 4; only this call ever sets it).  scratch: tpnet_lp_ranking_scratch_bytes(B, 1).  0 <= B < 2^31, 1 <= F < 2^16 with a
 * filter, k1, k2, k3 >= 1; null or misaligned pointers, sizes out of range: TPNET_ERR_BAD_ARG, nothing launched; a short scratch:
 * TPNET_ERR_WORKSPACE. */
int tpnet_lp_ranking_counts(const int32_t* counts, const float* pos_logit, int64_t B, const float* fil_logits, const int64_t* fil_ids,
                            const int32_t* n_fil, int32_t F, int32_t k1, int32_t k2, int32_t k3, void* scratch, size_t scratch_bytes,
                            int64_t* record, void* stream);

/* ---- the EdgeBank baseline on the device (additive to ABI 7; csrc/edgebank.hip) ------------------------------
 * models/EdgeBank.py as evaluate_models_utils.py:269-318 drives it: for every test batch the reference builds a memory over
 * train + val + test[:batch_start] and answers "is (u, v) in it" for the batch's positive and negative pairs.
 * One table holds the whole chronological stream, E edges (src[p], dst[p], t[p]), p = 0..E-1, t non-decreasing in p.  A call names a
 * history length h, 1 <= h <= E; the memory is what the reference builds from the first h edges -- the POSITION prefix, not a time cut: an
 * edge at a position >= h is no history even when its stamp equals t[h - 1].
 * For a query pair (u, v): p_0 < p_1 < ... the positions of its occurrences, c = #{ p_i < h }.  c == 0: the prediction is 0.  Else
 *   TPNET_EB_UNLIMITED:         1.
 *   TPNET_EB_TIME_WINDOW:       1 iff t[p_(c-1)] >= window_start  (the latest occurrence inside the prefix decides, because t is
 *                               non-decreasing; window_end = t[h - 1] never binds).
 *   TPNET_EB_REPEAT_THRESHOLD:  1 iff (double)c >= (double)h / (double)n_present(h), n_present(h) = the distinct edges among the first h
 *                               (np.mean of the reference's frequency dict).
 * window_start:
 *   TPNET_EB_FIXED_PROPORTION:  np.quantile(t[:h], 1 - proportion), method 'linear', in O(1) on the sorted prefix: q = 1 - proportion,
 *                               v = (h - 1) q, i = floor(v), g = v - i, a = t[i], b = t[min(i + 1, h - 1)];
 *                               g >= 0.5 ? b - (b - a) (1 - g) : a + (b - a) g  -- NumPy's _lerp, every operation rounded on its own
 *                               (no fused multiply-add), so the result equals NumPy's bit for bit.
 *   TPNET_EB_REPEAT_INTERVAL:   t[h - 1] - S / n_present(h), S = the sum over the distinct edges with c > 1 of their mean
 *                               inter-occurrence interval, which telescopes to (t[p_(c-1)] - t[p_0]) / (c - 1); the singletons count in
 *                               the denominator, as in the reference.  S is a float64 sum in a fixed order: thread k of workgroup w
 *                               of G = min(256, ceil(E / 256)) takes the unique edges (ascending src << 32 | dst order) 256 w + k,
 *                               + 256 G, ...; a halving tree over each wave's lanes, the four waves in order; then the G partials in
 *                               index order.  The same call gives the same bits; against the reference's dict-order sum the last
 *                               bits may differ.
 * Query ids outside [0, 2^31), negative ones included, and pairs that are not in the table predict 0.
 *
 * tpnet_edgebank_build, once per stream: checks ids and stamps on the device, sorts (src << 32 | dst, position) with one stable radix
 *   sort and writes, into the caller-owned device buffer `eb` of tpnet_edgebank_bytes(E): the U unique keys, the start of each one's
 *   ascending position list (U + 1 entries), the positions, a copy of t, and present[0..E], present[h] = n_present(h).  src / dst / t:
 *   device arrays of E; 1 <= E < 2^30.  An id outside [0, 2^31): TPNET_ERR_INDEX; a stamp below its predecessor's, or a NaN:
 *   TPNET_ERR_BAD_ARG (streams are refused, not sorted).  counts: HOST int64[1] = {U}; the call synchronises `stream` once.
 * tpnet_edgebank_predict: h by value, nothing read back, no synchronisation, at most two launches on `stream`: the partial sums of S
 *   (TIME_WINDOW with REPEAT_INTERVAL only), then one thread per query of BOTH lists -- list 0 (Q0 pairs -> out0) and list 1 (Q1 pairs
 *   -> out1, may be empty) -- so a batch's positives and negatives share one reduction.  out0 / out1: device fp32, 0.0 or 1.0.
 *   window_mode and proportion are checked always and used by TIME_WINDOW only.  scratch: tpnet_edgebank_scratch_bytes(E) device bytes,
 *   needed by REPEAT_INTERVAL only.  out_window: device double[2] or NULL: {window_start, window_end = t[h - 1]} (TIME_WINDOW),
 *   {threshold, n_present(h)} (REPEAT_THRESHOLD), {-inf, t[h - 1]} (UNLIMITED).
 * TPNET_ERR_BAD_ARG, nothing launched: a null table, a null array or output of a list that is not empty, h < 1 or h > E, proportion
 *   outside [0, 1], an unknown mode, Q < 0 (or >= 2^31), E outside [1, 2^30) (size helpers: 0), REPEAT_INTERVAL without scratch.  A short
 *   scratch: TPNET_ERR_WORKSPACE.  Q0 + Q1 == 0: TPNET_OK, nothing launched. */
#define TPNET_EB_UNLIMITED 0
#define TPNET_EB_TIME_WINDOW 1
#define TPNET_EB_REPEAT_THRESHOLD 2
#define TPNET_EB_FIXED_PROPORTION 0
#define TPNET_EB_REPEAT_INTERVAL 1
size_t tpnet_edgebank_bytes(int64_t E);
int tpnet_edgebank_build(void* eb, size_t bytes, const int64_t* src, const int64_t* dst, const double* t, int64_t E, int64_t* counts,
                         void* stream);
size_t tpnet_edgebank_scratch_bytes(int64_t E);
int tpnet_edgebank_predict(const void* eb, int64_t E, int32_t memory_mode, int32_t window_mode, double proportion, int64_t h,
                           const int64_t* src0, const int64_t* dst0, int64_t Q0, float* out0, const int64_t* src1, const int64_t* dst1,
                           int64_t Q1, float* out1, void* scratch, size_t scratch_bytes, double* out_window, void* stream);

/* The encoder's readout with the ids resident on the device end to end (models/TPNet.py:280-324, SURVEY §8 f-3 -> f-2): for one
 * (src, other) batch of B edges -- other = dst or the negatives -- the 2B nodes [src; other] at times tile(t, 2) draw their K most
 * recent neighbours from the device sampler, and every neighbour is paired with the edge's two endpoints: out[0][(i*K + k)] =
 * G(neigh[i][k], src[i % B]), out[1][...] = G(neigh[i][k], other[i % B]), i in [0, 2B) -- the reference's
 * get_pair_wise_feature(tile(neigh, 2), concat(repeat(tile(src,2),K), repeat(tile(other,2),K))) before self.mlp, without any index
 * array and without the neighbour ids visiting the host.  One call, two launches (rows + sampler, readout).  scratch: tpnet_encoder_scratch_bytes(B, K)
 * device bytes; the sampled neighbour ids [2B][K] (int64) are left at (scratch rounded up to 256) + 64 B bytes for the caller's
 * other neighbour features.  Needs tpnet_pair_gram_anchored_supported(st).  src / other / t: device arrays of B. */
size_t tpnet_encoder_scratch_bytes(int64_t B, int32_t K);
int tpnet_encoder_gram(const tpnet_state* st, const void* sampler, int64_t E, int64_t num_nodes, const int64_t* src,
                       const int64_t* other, const double* t, int64_t B, int32_t K, double now_time, double lambda,
                       uint32_t flags, void* scratch, size_t scratch_bytes, float* out, void* stream);

/* The first half of tpnet_encoder_gram alone: the rows [src; other] at tile(t, 2), their anchors and their K sampled neighbours,
 * laid out in `scratch` (rounded up to 256): nodes int64[2B] | times double[2B] | a1 int64[2B] | a2 int64[2B] | neigh int64[2B][K]
 * | (rows of <= 128 floats that the matrix-core readout does not serve: the call's pairs spelled out for the generic readout) u int64[4BK] | v int64[4BK].
 * (tpnet_encoder_gram / tpnet_encoder_features with TPNET_FLAG_ROWS8 on rows of d % 4 == 2 take the matrix cores and leave the pair lists out.) */
int tpnet_encoder_rows(const tpnet_state* st, const void* sampler, int64_t E, int64_t num_nodes, const int64_t* src,
                       const int64_t* other, const double* t, int64_t B, int32_t K, void* scratch, size_t scratch_bytes,
                       void* stream);

/* THE route of an anchored readout (additive to ABI 7; csrc/encoder.hip: anchored_route -- every entry point below and
 * tpnet_pair_gram_anchored ask that one function).  For n_rows x K neighbours read with `flags`, 16-byte aligned outputs, no pair
 * lists and `mlp` (may be NULL): 0 = refused (TPNET_ERR_BAD_ARG), else the kernel that forms the Gram in bits 0-3 and the
 * one-launch kind in bits 4-5.
 *   Gram kernel, first match wins
 *     TPNET_FLAG_PACKED                                                     -> refused
 *     TPNET_FLAG_ROWS8 on a row of d % 4 == 2                               -> 3 (matrix cores, 8-byte halves) where 38 <= d <= 158,
 *                                                                              L = 3, K >= 4 and no TPNET_FLAG_NO_MFMA_READOUT; else
 *                                                                              refused (no walk reads such rows; the launch refuses
 *                                                                              outputs that are not 16-byte aligned)
 *     [pair lists: tpnet_encoder_gram / tpnet_encoder_features only] d <= 128, not (L = 3, d % 4 == 0, 36 <= d <= 160, K >= 4),
 *       TPNET_FLAG_LAYERS_MFMA not served                                   -> 1 (generic pair kernel on the spelled-out lists;
 *                                                                              tpnet_encoder_gram: only where the next line passes,
 *                                                                              tpnet_encoder_features: only with a gram buffer)
 *     not (d % 4 == 0 and 36 <= d <= 512)                                   -> refused
 *     L = 3, 36 <= d <= 160, K >= 4, aligned, no TPNET_FLAG_NO_MFMA_READOUT  -> 3 (matrix cores, csrc/encoder_mfma.hip)
 *     TPNET_FLAG_LAYERS_MFMA, L = 1 / 2 / 4, 36 <= d <= 160, K >= 4, aligned,
 *       no TPNET_FLAG_NO_MFMA_READOUT                                       -> 4 (matrix cores, csrc/encoder_layers.hip)
 *     otherwise                                                             -> 2 (vector-ALU walk)
 *   One launch of readout + self.mlp (mlp of F = 64, H = 256, L = 3, no TPNET_FLAG_NO_MFMA_READOUT; gram may then be NULL)
 *     the Gram kernel is 3 and mlp->wimg is given                           -> 1 (k_encoder_fused)
 *     else 164 <= d <= 512, K >= 4, mlp->w1 / w2f given, the width's geometry class routed (at present none) -> 2 (k_anchored_feature)
 * (n_rows >= 1, n_rows * K < 2^25 and N < 2^31 wherever the matrix cores are named.)  The queries below are views of this table. */
int tpnet_anchored_route(const tpnet_state* st, int64_t n_rows, int32_t K, uint32_t flags, const tpnet_mlp* mlp);

/* The encoder's call INCLUDING self.mlp (models/TPNet.py:311-324, 129; L = 3, rows as tpnet_pair_gram_anchored needs them): gram =
 * tpnet_pair_gram_anchored's output [2][n_rows*K][64] (kept: what a backward pass needs), out = mlp(gram) in the fp32 class
 * (tpnet_mlp64_f32's kernel), both on `stream`: the encoder's call as ONE crossing.  Where tpnet_encoder_fused_supported
 * returns 1 (rows of 36..160 floats with d % 4 == 0, K >= 4, mlp->wimg given) readout and dense layers are ONE launch on the matrix cores
 * (csrc/encoder_mfma.hip) and gram may be NULL: the pre-mlp features are then never written.  It also returns 1 for rows of
 * 164..512 floats whose geometry class (32 lanes x 2 vectors up to d = 256, 64 x 2 from d = 260) is routed to the one-launch kernel
 * of csrc/anchored_feature.hip -- a class is routed only where that kernel was measured faster than the two launches
 * (profiles/encoder_wide.md: at present neither); TPNET_FLAG_NO_MFMA_READOUT selects the two launches at every width. */
int tpnet_encoder_fused_supported(const tpnet_state* st, int64_t n_rows, int32_t K, const tpnet_mlp* mlp);
/* Rows that are only 8-byte aligned (d % 4 == 2): does TPNET_FLAG_ROWS8 make the matrix-core kernels serve this shape
 * (38 <= d <= 158, L = 3, K >= 4)?  mlp == NULL: the readout alone (tpnet_pair_gram_anchored, tpnet_encoder_gram); mlp given:
 * readout and self.mlp as ONE launch (tpnet_anchored_features and the calls built on it; gram may then be NULL).  0 for every
 * d % 4 != 2: tpnet_pair_gram_anchored_supported / tpnet_encoder_fused_supported answer for those, and never count this flag. */
int tpnet_encoder_rows8_supported(const tpnet_state* st, int64_t n_rows, int32_t K, const tpnet_mlp* mlp);
/* Does TPNET_FLAG_LAYERS_MFMA send the anchored readout of this shape to the matrix cores?  1 for L = 1, 2, 4 on rows of 36..160
 * floats with d % 4 == 0 (a table padded to such a width included), K >= 4, N < 2^31; 0 otherwise -- L = 3 among them: that is
 * tpnet_pair_gram_anchored's own route and needs no flag. */
int tpnet_encoder_layers_supported(const tpnet_state* st, int64_t n_rows, int32_t K);
/* The tiles that kernel cuts the flat [n_rows * K] neighbour list into, on the host (tests): their number (0: not a served L /
 * K), and tile t's first slot and slot count.  L = 1, 2: 8 resp. 5 consecutive slots; L = 4: <= 3 slots, never across a row's end. */
int64_t tpnet_encoder_layers_tiles(int32_t L, int64_t n_rows, int32_t K);
int tpnet_encoder_layers_tile(int32_t L, int64_t n_rows, int32_t K, int64_t t, int64_t* first_slot, int32_t* count);
int tpnet_anchored_features(const tpnet_state* st, const int64_t* neigh, const int64_t* a1, const int64_t* a2, int64_t n_rows,
                            int32_t K, double now_time, double lambda, uint32_t flags, const tpnet_mlp* mlp, float* gram,
                            float* out, void* stream);
/* The same call on rows of 164..512 floats (d % 4 == 0, L = 3, K >= 4, mlp->w1 / w2f given: tpnet_encoder_wide_supported returns
 * 1) ALWAYS as one launch: the vector-ALU anchored walk with self.mlp on the matrix cores inside the kernel
 * (csrc/anchored_feature.hip).  Pre-mlp features with the bits of tpnet_pair_gram_anchored(..., TPNET_FLAG_NO_MFMA_READOUT),
 * outputs in the fp32 class; gram may be NULL.  TPNET_ERR_BAD_ARG on any other shape.  tpnet_anchored_features takes this kernel
 * on its own only for the classes it is routed for; this entry reaches it whatever the route is (tests, rate tools). */
int tpnet_encoder_wide_supported(const tpnet_state* st, int64_t n_rows, int32_t K, const tpnet_mlp* mlp);
int tpnet_anchored_features_wide(const tpnet_state* st, const int64_t* neigh, const int64_t* a1, const int64_t* a2, int64_t n_rows,
                                 int32_t K, double now_time, double lambda, uint32_t flags, const tpnet_mlp* mlp, float* gram,
                                 float* out, void* stream);
/* tpnet_encoder_rows + tpnet_anchored_features: the encoder's whole readout for one (src, other) batch, ids resident on the
 * device, self.mlp included, ONE call. */
int tpnet_encoder_features(const tpnet_state* st, const void* sampler, int64_t E, int64_t num_nodes, const int64_t* src,
                           const int64_t* other, const double* t, int64_t B, int32_t K, double now_time, double lambda,
                           uint32_t flags, const tpnet_mlp* mlp, void* scratch, size_t scratch_bytes, float* gram, float* out,
                           void* stream);

/* tpnet_encoder_features with the batch's src / other / times as HOST arrays (the reference's loop slices them from the edge
 * list on the host, train_link_prediction.py:325-340): staged through `stage` (B <= slot_bytes / 24), read in place by the row
 * set-up kernel; no copy is enqueued.  TPNET_ERR_INDEX for an id outside [0, N). */
int tpnet_host_encoder_features(const tpnet_state* st, tpnet_stage* stage, const void* sampler, int64_t E, int64_t num_nodes,
                                const int64_t* h_src, const int64_t* h_other, const double* h_t, int64_t B, int32_t K,
                                double now_time, double lambda, uint32_t flags, const tpnet_mlp* mlp, void* scratch,
                                size_t scratch_bytes, float* gram, float* out, void* stream);

/* Host-side check (no GPU work): is (src, dst) of a get_pair_wise_feature call of n pairs the encoder's pattern (models/TPNet.py:
 * 311-316: src = tile(neigh, 2), dst = concat(repeat(a1, K), repeat(a2, K)))?  Returns K >= 2, else 0 (N is unused: the ids' range
 * is the caller's to check). */
int64_t tpnet_host_encoder_pattern(const int64_t* src, const int64_t* dst, int64_t n, int64_t N);
/* The encoder's call from the reference's own HOST index arrays in one crossing (ABI 6): pattern check, range check, the n / 2
 * neighbour ids + the anchors staged through `stage` (slot_bytes >= (n / 2 + n / K) * 8; the kernel reads them there) and
 * tpnet_anchored_features launched on `stream`.  *K_out = the pattern's K (>= 4) if the call was served, 0 if not (not the
 * pattern, K < 4, an id outside [0, N), a shape the kernels do not serve): the caller then takes the general path.  gram: as for
 * tpnet_anchored_features (may be NULL where tpnet_encoder_fused_supported). */
int tpnet_host_anchored_features(const tpnet_state* st, tpnet_stage* stage, const int64_t* h_src, const int64_t* h_dst, int64_t n,
                                 double now_time, double lambda, uint32_t flags, const tpnet_mlp* mlp, float* gram, float* out,
                                 int32_t* K_out, void* stream);

/* ---- the step behind the path (BASELINE config 5): self.mlp = Linear(64,256)->ReLU->Linear(256,64)
 * (models/TPNet.py:64-65,129) fused in one kernel on the bf16 matrix cores, fp32 accumulate, L = 3 only.
 * x [n][64] f32 (the readout's features), y [n][64] f32.  w1_bf16: [256][64] bf16 = mlp[0].weight; w2p_bf16: [64][256]
 * bf16 = mlp[2].weight with its hidden axis permuted per 32-tile to the accumulator order
 * k' = 16 s + 8 h + j  <-  k = 16 s + 8 (j>>2) + 4 h + (j&3)   (s in 0..1, h in 0..1, j in 0..7). */
int tpnet_mlp64_bf16(const float* x, int64_t n, const void* w1_bf16, const float* b1, const void* w2p_bf16,
                     const float* b2, float* y, void* stream);

/* Backward of self.mlp with respect to its weights on the bf16 matrix cores (training; the projections carry no gradient,
 * models/TPNet.py:49-62).  x: the pre-mlp features [n][64] f32, gy: the gradient of the output [n][64] f32; w1_bf16 [256][64]
 * = mlp[0].weight, w2t_bf16 [256][64] = mlp[2].weight transposed.  Every workgroup writes ONE partial result of
 * tpnet_mlp64_bwd_partial_floats() floats, laid out gW1 [256][64] | gW2 [64][256] | gb1 [256] (gb2 = the column sums of gy is
 * the caller's); the call returns the
 * number of partials written (<= n_partial; negative = error) and the caller sums them (fixed order: deterministic). */
int64_t tpnet_mlp64_bwd_partial_floats(void);
int tpnet_mlp64_bwd_bf16(const float* x, const float* gy, int64_t n, const void* w1_bf16, const float* b1,
                         const void* w2t_bf16, float* partial, int32_t n_partial, void* stream);
/* The same backward in the fp32 class of the default forward paths (round 4): every operand in two bf16 pieces, every product as
 * lo*hi + hi*lo + hi*hi with fp32 accumulation; weights from the f32 layouts of `mlp` (mlp->w1 = mlp[0].weight [256][64], mlp->w2t =
 * mlp[2].weight transposed [256][64], mlp->b1).  Same partial layout and return value as tpnet_mlp64_bwd_bf16. */
int tpnet_mlp64_bwd_f32(const float* x, const float* gy, int64_t n, const tpnet_mlp* mlp, float* partial, int32_t n_partial,
                        void* stream);
/* The fp32-class backward for num_layer 1 and 2 (csrc/mlp_rows_bwd.hip): the weight gradients of self.mlp = Linear(F, 4F) -> ReLU ->
 * Linear(4F, F) for the (F, H) that tpnet_mlp_rows_supported accepts, (16, 64) and (36, 144), in ONE launch on the caller's stream,
 * no synchronisation.  x: the pre-mlp features [n][F] f32, gy: the gradient of the output [n][F] f32, both device, 16-byte aligned,
 * read only inside their n * F floats; weights from mlp->w1t, b1, w2t (what tpnet_mlp_rows_f32 reads).  fp32 class: two-piece bf16
 * operands with fp32 accumulation, the pre-activations that decide the ReLU in exact f32.  Every workgroup writes ONE
 * partial result of tpnet_mlp_rows_bwd_partial_floats(F, H) floats (0 for a width that is not served; 2 112 at F = 16, 10 512 at
 * F = 36), laid out gW1 [H][F] | gW2 [F][H] | gb1 [H], unpadded (gb2 = the column sums of gy is the caller's).  Returns the number of
 * partials written, min(n_partial, ceil(n / 32)); the caller sums them (fixed order: deterministic) and nothing beyond them is
 * written.  n == 0: nothing is written, returns 0.  TPNET_ERR_BAD_ARG, before any HIP call: a null pointer, a width that
 * tpnet_mlp_rows_supported refuses, a misaligned x or gy, n_partial < 1; a negative code also when the runtime refuses the kernel's
 * LDS (80 KB at F = 36) or the launch -- the caller then computes the gradients its other way.  A NaN in a row of x or gy reaches
 * the gradients, as it does in the torch expressions; memory outside the two lists never does. */
int64_t tpnet_mlp_rows_bwd_partial_floats(int32_t F, int32_t H);
int tpnet_mlp_rows_bwd_f32(const float* x, const float* gy, int64_t n, const tpnet_mlp* mlp, float* partial, int32_t n_partial,
                           void* stream);

/* get_pair_wise_feature with self.mlp on the bf16 matrix cores INSIDE the readout kernel (L = 3, d % 4 == 0 and d >= 64):
 * 8 waves form the features of 32 pairs into an LDS tile, which is the B operand of layer 1; wave w owns hidden units
 * [32w, 32w+32) of both layers, the 8 partial outputs are added in a fixed order.  The features never touch HBM (out_gram,
 * optional: a copy for a backward pass).  Weights as for tpnet_mlp64_bf16 (w1_bf16 [256][64], w2p_bf16 [64][256] permuted).
 * bf16 operands, fp32 accumulation: ~1e-2 relative, opt-in (RandomProjectionModule.fused_mlp). */
int tpnet_pair_feature_bf16(const tpnet_state* st, const int64_t* u, const int64_t* v, int64_t n, double now_time,
                            double lambda, uint32_t flags, const void* w1_bf16, const float* b1, const void* w2p_bf16,
                            const float* b2, float* out_gram, float* out, void* stream);

/* LinkPredictor_v1 (models/modules.py:73-117): out[p] = fc2(relu(fc1(concat[src_emb[p], dst_emb[p], feat[p]]))) with ONE
 * output unit, both layers in one bf16 matrix-core kernel (fp32 accumulate); neither the concatenation nor the hidden
 * layer touches memory.  src_emb, dst_emb: device f32 [n][D] (D % 4 == 0; both NULL = the reference's not_encode mode,
 * zeros); feat: device f32 [n][F] (F % 16 == 0; NULL if the decoder has no pairwise feature).  w1p: bf16
 * [32*hidden_tiles][2*DP + F], DP = 16*ceil(D/16): fc1.weight with its input axis laid out [src | pad | dst | pad | feat]
 * and zero rows beyond the hidden width; b1p, w2p: f32 [32*hidden_tiles] (fc1.bias, fc2.weight[0], zero-padded); b2 =
 * fc2.bias[0].  hidden_tiles in 1..8 (hidden width <= 256).  out: device f32 [n]. */
int tpnet_decoder_bf16(const float* src_emb, const float* dst_emb, int32_t D, const float* feat, int32_t F, int64_t n,
                       const void* w1p_bf16, const float* b1p, const float* w2p, float b2, int32_t hidden_tiles,
                       float* out, void* stream);

/* The readout's element-wise tail, in place on x[n]: x<0 -> 0, then log(x + 1) (models/TPNet.py:126-128).  For callers
 * that ran the readout with TPNET_FLAG_NOT_SCALE because the raw Gram entries still had to be summed across GPUs
 * (column-sharded table: every rank holds d/G columns of every row, the entries are partial inner products). */
int tpnet_gram_finish(float* x, int64_t n, void* stream);

/* packed[n][(2L+2)(2L+3)/2] (TPNET_FLAG_PACKED rows, summed over the ranks) -> out[n][(2L+2)^2]: mirrors the upper
 * triangle and, unless TPNET_FLAG_NOT_SCALE, applies x<0 -> 0, log(x + 1). */
int tpnet_gram_unpack(const float* packed, int64_t n, int32_t L, uint32_t flags, float* out, void* stream);

/* ---- the encoder's input stage in one launch (additive to ABI 7; csrc/encoder_input.hip) ------------------
 * TPNetEmbedding between the readout and the mixers (models/TPNet.py:297-330), n = n_nodes * K rows:
 *   out[row] = W2 . relu(W1 . x[row] + b1) + b2
 *   x[row]   = [ node_raw[neigh[row]] | cos(tw * log(f32(tq[row / K] - tn[row]) + 1) + tb) | edge_raw[eid[row]] | feat[row] | feat[n + row] ]
 * fp32 class on the matrix cores (two bf16 pieces per operand, three products per term, fp32 accumulators); the concat is never
 * written.  dims = HOST int32[6] {Dn, Dt, De, F, H, Dout}: W1 is [H][Dn + Dt + De + 2 F], W2 [Dout][H], both row-major f32.
 * Served (tpnet_encoder_input_supported = 1): Dn, Dt, De, F, Dout multiples of 4 and >= 4, Din <= 1024, 1 <= H <= 512, Dout <= 256.
 * tpnet_encoder_input_image_bytes: size of the split weights in the kernel's operand order (host arithmetic; 0 for unserved dims).
 * tpnet_encoder_input_prepare: ONE launch that writes the image from the four Parameters; again whenever one of them changed.
 * tpnet_encoder_input: one launch on `stream`, no synchronisation.  node_raw [n_node_rows][Dn], edge_raw [n_edge_rows][De], neigh /
 *   eid int64 [n], tn f64 [n], tq f64 [n_nodes], tw / tb f32 [Dt], feat f32 [2 n][F], out f32 [n][Dout]; the f32 arrays 16-byte
 *   aligned.  An id outside node_raw / edge_raw reads row 0 instead and sets err[0] (a device uint32 the caller zeroed once):
 * tpnet_encoder_input_check copies the word to the host (synchronises the stream), clears it if set and returns TPNET_ERR_INDEX.
 * Null pointers and sizes out of range: TPNET_ERR_BAD_ARG, nothing launched. */
int tpnet_encoder_input_supported(int32_t Dn, int32_t Dt, int32_t De, int32_t F, int32_t H, int32_t Dout);
size_t tpnet_encoder_input_image_bytes(int32_t Dn, int32_t Dt, int32_t De, int32_t F, int32_t H, int32_t Dout);
int tpnet_encoder_input_prepare(const float* w1, const float* b1, const float* w2, const float* b2, const int32_t* dims, void* img,
                                void* stream);
int tpnet_encoder_input(const float* node_raw, int64_t n_node_rows, const float* edge_raw, int64_t n_edge_rows, const int64_t* neigh,
                        const int64_t* eid, const double* tn, const double* tq, const float* tw, const float* tb, const float* feat,
                        int64_t n_nodes, int32_t K, const int32_t* dims, const void* img, float* out, uint32_t* err, void* stream);
int tpnet_encoder_input_check(uint32_t* err, void* stream);

/* ---- one MLP-Mixer layer in two launches, forward only (additive to ABI 7; csrc/mixer.hip) ------------------
 * MLPMixer.forward (models/TPNet.py:371-416) with dropout as identity, x [n_nodes][K][C] f32:
 *   tpnet_mixer_token:    out[node][:, c] = x[node][:, c] + W2 . gelu(W1 . LN_K(x[node][:, c]) + b1) + b2   for every channel c;
 *                         gamma, beta [K], w1 [Kh][K], b1 [Kh], w2 [K][Kh], b2 [K].  Plain fp32 on the vector ALU.
 *   tpnet_mixer_channel:  out[row] = x[row] + W2 . gelu(W1 . LN_C(x[row]) + b1) + b2   on n_rows = n_nodes * K rows of C floats;
 *                         gamma, beta [C]; W1 [Ch][C], b1 [Ch], W2 [C][Ch], b2 [C] come as the image tpnet_mixer_channel_prepare wrote
 *                         (ONE launch; again whenever one of the four changed).  fp32 class on the matrix cores (two bf16 pieces per
 *                         operand, three products per term, fp32 accumulators); the normalised rows are never written.
 * gelu is the exact one (erf); both LayerNorms use the biased variance and the call's eps.  Every launch goes to `stream`, nothing
 * synchronises.  Served (tpnet_mixer_supported = 1, host arithmetic): 2 <= K <= 32, 1 <= Kh <= 32, C % 4 == 0, 4 <= C <= 256,
 * 1 <= Ch <= 1024.  tpnet_mixer_channel_image_bytes: size of the image (a multiple of 16; 0 for unserved C, Ch).  x, out, the image and
 * the channel call's gamma / beta 16-byte aligned; out must not be x.  Null pointers, misaligned arrays, out == x and unserved
 * sizes: TPNET_ERR_BAD_ARG, nothing launched.  n_nodes / n_rows = 0: TPNET_OK, nothing launched. */
int tpnet_mixer_supported(int32_t K, int32_t Kh, int32_t C, int32_t Ch);
size_t tpnet_mixer_channel_image_bytes(int32_t C, int32_t Ch);
int tpnet_mixer_channel_prepare(const float* w1, const float* b1, const float* w2, const float* b2, int32_t C, int32_t Ch, void* img,
                                void* stream);
int tpnet_mixer_token(const float* x, int64_t n_nodes, int32_t K, int32_t C, const float* gamma, const float* beta, float eps,
                      const float* w1, const float* b1, int32_t Kh, const float* w2, const float* b2, float* out, void* stream);
int tpnet_mixer_channel(const float* x, int64_t n_rows, int32_t C, int32_t Ch, const float* gamma, const float* beta, float eps,
                        const void* img, float* out, void* stream);

/* ---- the token-mixing half in a training step: forward with dropout, backward (additive to ABI 7; csrc/mixer_token_train.hip,
 * DESIGN.md section 3.6) ---------------------------------------------------------------------------------------------------------
 * Per (node, channel) column v[0 .. K) of x [n_nodes][K][C] f32, with s = 1 / (1 - p) in float and the keep masks m1 [Kh], m2 [K] of
 * the two Dropout(p) of FeedForwardNet (behind the GELU, behind the second Linear); arguments as tpnet_mixer_token's:
 *   tpnet_mixer_token_train:  ln = LN_K(v); a[j] = sum_k w1[j][k] ln[k] + b1[j]; h[j] = gelu(a[j]) m1[j] s;
 *                             out[k] = (sum_j w2[k][j] h[j] + b2[k]) m2[k] s + v[k].  ONE launch.  p = 0: nothing is drawn and out has
 *                             the bits of tpnet_mixer_token's.
 *   tpnet_mixer_token_bwd:    from gy = dL/dout (as x: [n_nodes][K][C], 16-byte aligned), ONE launch that recomputes the column's
 *                             forward from x and the key (the caller saves x alone) and writes gx = dL/dx (gx may be NULL: not
 *                             computed; else as x, and neither x nor gy) and min(n_partial, batches) partial sums of the six parameter
 *                             gradients, batches = ceil(n_nodes C / 256) (/ 128 where 4 K + 2 Kh > 159).  A partial is
 *                             tpnet_mixer_token_bwd_partial_floats(K, Kh) = 3 K + 2 K Kh + Kh floats (0 for an unserved K / Kh), laid out
 *                             ggamma [K] | gbeta [K] | gw1 [Kh][K] | gb1 [Kh] | gw2 [K][Kh] | gb2 [K], unpadded, partial i at
 *                             partial + i * that many floats; `partial` holds n_partial >= 1 of them, those beyond the returned count
 *                             are not written.  Returns that count (>= 0; 0 for n_nodes = 0) or a negative error.  The caller adds
 *                             the partials in a fixed order; the kernel uses no atomics, so two calls give equal bits.
 *   tpnet_mixer_token_masks:  m1 as bytes [n_nodes][C][Kh] and m2 as bytes [n_nodes][K][C] (1 = kept; p = 0: all 1), for evaluating the
 *                             same dropout elsewhere.
 * THE DRAWS.  Column index i = node * C + channel.  Draw d of column i, 0 <= d < Kh + K, is word d % 4 of the Philox4x32-10 block with
 * counter (i & 0xffffffff, i >> 32, d / 4, 0x4D58544B) and key (key & 0xffffffff, key >> 32).  m1[j] = draw j, m2[k] = draw Kh + k;
 * a unit is kept when its word >= floor(p 2^32) (p the float argument, the product in double).  A draw depends on (key, column, slot)
 * alone, never on the launch geometry.  These are Dropout(p)'s probabilities, NOT torch's dropout stream.
 * 0 <= p < 1 (else, as for a null pointer, a misaligned array, out == x, an unserved size or n_partial < 1: TPNET_ERR_BAD_ARG,
 * nothing launched; all of these are checked before any GPU call).  The backward's LDS (up to 159 KB) needs the runtime's grant:
 * TPNET_ERR_BAD_ARG if refused.  n_nodes = 0: TPNET_OK / 0, nothing launched.  Exact fp32 on the vector ALU throughout. */
int tpnet_mixer_token_train(const float* x, int64_t n_nodes, int32_t K, int32_t C, const float* gamma, const float* beta, float eps,
                            const float* w1, const float* b1, int32_t Kh, const float* w2, const float* b2, float p, uint64_t key,
                            float* out, void* stream);
int64_t tpnet_mixer_token_bwd_partial_floats(int32_t K, int32_t Kh);
int tpnet_mixer_token_bwd(const float* x, const float* gy, int64_t n_nodes, int32_t K, int32_t C, const float* gamma, const float* beta,
                          float eps, const float* w1, const float* b1, int32_t Kh, const float* w2, const float* b2, float p,
                          uint64_t key, float* gx, float* partial, int32_t n_partial, void* stream);
int tpnet_mixer_token_masks(int64_t n_nodes, int32_t K, int32_t Kh, int32_t C, float p, uint64_t key, uint8_t* m1, uint8_t* m2,
                            void* stream);

/* ---- the channel-mixing half in a training step: forward with dropout, backward (additive to ABI 7; csrc/mixer_channel_train.hip,
 * DESIGN.md section 3.6) ---------------------------------------------------------------------------------------------------------
 * Per row v[0 .. C) of x [n_rows][C] f32, with s = 1 / (1 - p) in float and the keep masks m1 [Ch], m2 [C] of the two Dropout(p) of
 * FeedForwardNet (behind the GELU, behind the second Linear); arguments as tpnet_mixer_channel's, img the image
 * tpnet_mixer_channel_prepare wrote:
 *   tpnet_mixer_channel_train:  ln = LN_C(v); a = W1 . ln + b1; h = gelu(a) m1 s; out = (W2 . h + b2) m2 s + v.  ONE launch.  p = 0:
 *                               nothing is drawn and out has the bits of tpnet_mixer_channel's.
 *   tpnet_mixer_channel_bwd:    from gy = dL/dout (as x: [n_rows][C], 16-byte aligned), TWO launches that recompute the row's forward
 *                               from x and the key (the caller saves x alone) and write gx = dL/dx (gx may be NULL: not computed; else as
 *                               x, and neither x nor gy) and min(n_partial, ceil(n_rows / 32)) partial sums of the six parameter
 *                               gradients, one per part of the rows.  A partial is tpnet_mixer_channel_bwd_partial_floats(C, Ch) =
 *                               2 C + 2 C Ch + Ch + C floats (0 for an unserved C / Ch), laid out
 *                               ggamma [C] | gbeta [C] | gw1 [Ch][C] | gb1 [Ch] | gw2 [C][Ch] | gb2 [C], unpadded, partial i at
 *                               partial + i * that many floats; `partial` holds n_partial >= 1 of them, those beyond the returned
 *                               count are not written.  Returns that count (>= 0; 0 for n_rows = 0) or a negative error.  The caller
 *                               adds the partials in a fixed order; the kernels use no atomics, so two calls give equal bits.
 *                               bimg: the backward's image, in place of img (tpnet_mixer_channel_bwd_image_bytes;
 *                               tpnet_mixer_channel_bwd_prepare writes it from w1 [Ch][C], b1 [Ch] and w2 [C][Ch] in ONE launch; again
 *                               whenever one of the three changed).
 *                               workspace: tpnet_mixer_channel_bwd_workspace_bytes(n_rows, C, Ch) bytes (0 for an unserved size),
 *                               16-byte aligned, the call's own: its contents mean nothing before or after the two launches.
 *   tpnet_mixer_channel_masks:  m1 as bytes [n_rows][Ch] and m2 as bytes [n_rows][C] (1 = kept; p = 0: all 1), for evaluating the same
 *                               dropout elsewhere.  One thread per block of four draws in one launch: n_rows (ceil(Ch / 4) + C / 4)
 *                               <= 2^32 - 256, else TPNET_ERR_BAD_ARG.
 * THE DRAWS.  Row index i = the row's position in x.  Block b of row i is the four words of Philox4x32-10 with counter
 * (i & 0xffffffff, i >> 32, b, 0x4D584348) and key (key & 0xffffffff, key >> 32).  m1[j] = word j % 4 of block j / 4, m2[c] = word
 * c % 4 of block ceil(Ch / 4) + c / 4: both masks start on a block boundary.  A unit is kept when its word >= floor(p 2^32) (p the float
 * argument, the product in double).  A draw depends on (key, row, slot) alone, never on the launch geometry.  These are Dropout(p)'s
 * probabilities, NOT torch's dropout stream.
 * Served sizes: tpnet_mixer_supported's C and Ch, n_rows <= 2^31.  0 <= p < 1 (else, as for a null pointer, an array that is not
 * 16-byte aligned (partial: 4-byte), out == x, gx == x or gy, an unserved size or n_partial < 1: TPNET_ERR_BAD_ARG, nothing launched;
 * all of these are checked before any GPU call).  n_rows = 0: TPNET_OK / 0, nothing launched.  Every product is the fp32 class on
 * the matrix cores; LayerNorm, gelu, gelu', the masks and the LayerNorm backward are plain fp32. */
int tpnet_mixer_channel_train(const float* x, int64_t n_rows, int32_t C, int32_t Ch, const float* gamma, const float* beta, float eps,
                              const void* img, float p, uint64_t key, float* out, void* stream);
int64_t tpnet_mixer_channel_bwd_partial_floats(int32_t C, int32_t Ch);
size_t tpnet_mixer_channel_bwd_image_bytes(int32_t C, int32_t Ch);
int tpnet_mixer_channel_bwd_prepare(const float* w1, const float* b1, const float* w2, int32_t C, int32_t Ch, void* bimg, void* stream);
size_t tpnet_mixer_channel_bwd_workspace_bytes(int64_t n_rows, int32_t C, int32_t Ch);
int tpnet_mixer_channel_bwd(const float* x, const float* gy, int64_t n_rows, int32_t C, int32_t Ch, const float* gamma,
                            const float* beta, float eps, const void* bimg, float p, uint64_t key, void* workspace, float* gx,
                            float* partial, int32_t n_partial, void* stream);
int tpnet_mixer_channel_masks(int64_t n_rows, int32_t C, int32_t Ch, float p, uint64_t key, uint8_t* m1, uint8_t* m2, void* stream);

/* ---- the encoder's input stage in a training step: forward that records the ReLU decisions, backward (additive to ABI 7;
 * csrc/encoder_input_train.hip) ------------------------------------------------------------------------------
 * Arguments, sources, dims, weight image (img: tpnet_encoder_input_prepare's) and error word as tpnet_encoder_input's; n = n_nodes * K
 * rows, x[row] the row's concat, Din = Dn + Dt + De + 2 F, NW = ceil(H / 32):
 *   tpnet_encoder_input_train:  tpnet_encoder_input's launch -- out has its bits -- that also stores relu_bits [n][NW] uint32 (4-byte
 *                               aligned): bit u % 32 of word u / 32 of a row is (W1 . x + b1)[u] > 0 exactly as this launch decided it;
 *                               bits of units >= H are 0.  Serves everything tpnet_encoder_input serves.  ONE launch.
 *   tpnet_encoder_input_bwd:    from gy = dL/dout [n][Dout] (16-byte aligned) and relu_bits = m, TWO launches:
 *                                 a = W1 . x + b1, h = m ? a : 0, gh = W2^T . gy, ga = m ? gh : 0,
 *                                 gw1 = sum ga (x) x, gb1 = sum ga, gw2 = sum gy (x) h, gb2 = sum gy,
 *                                 gxt = W1[:, time columns]^T . ga, gtw = sum gxt (-sin(tw lt + tb)) lt, gtb = sum gxt (-sin(tw lt + tb)),
 *                                 gfeat[row] | gfeat[n + row] = W1[:, relative-encoding columns]^T . ga       (every sum over the rows)
 *                               with lt = log(f32(tq - tn) + 1).  The raw tables take no gradient.  gfeat [2 n][F] (16-byte aligned;
 *                               neither feat nor gy) may be NULL: not computed.  time_grads = 0: gtw and gtb are written as zeros.
 *                               min(n_partial, ceil(n / 32)) or fewer partial sums of the six parameter gradients are written, one per
 *                               part of the rows.  A partial is tpnet_encoder_input_bwd_partial_floats(dims) = H Din + H + Dout H +
 *                               Dout + 2 Dt floats, laid out gw1 [H][Din] | gb1 [H] | gw2 [Dout][H] | gb2 [Dout] | gtw [Dt] | gtb [Dt],
 *                               unpadded, partial i at partial + i * that many floats; `partial` (4-byte aligned) holds n_partial >= 1
 *                               of them, those beyond the returned count are not written.  Returns that count (>= 0; 0 for n = 0) or a
 *                               negative error.  The caller adds the partials in a fixed order; the kernels use no atomics but the
 *                               error word's, so two calls give equal bits.
 *                               bimg: the backward's image (tpnet_encoder_input_bwd_image_bytes; tpnet_encoder_input_bwd_prepare writes
 *                               it from w1 [H][Din], b1 [H] and w2 [Dout][H] in ONE launch; again whenever one of the three changed).
 *                               workspace: tpnet_encoder_input_bwd_workspace_bytes(n, dims) = ceil(n / 32) 32 (2 pad(H) + pad(Din) +
 *                               pad(Dout) + pad(Dt) + 1) 4 bytes, pad(v) = 32 ceil(v / 32); 16-byte aligned, the call's own: its contents
 *                               mean nothing before or after the two launches.
 * Served by the backward: tpnet_encoder_input_supported's sizes with Dt + 2 F <= 256 and n <= 2^31; the three size entries are host
 * arithmetic and return 0 for anything else.  An id outside node_raw / edge_raw reads row 0 and sets err[0] in the backward as in the
 * forward.  Null pointers, misaligned arrays, unserved sizes, n_partial < 1, gfeat == feat or gy: TPNET_ERR_BAD_ARG, nothing launched;
 * all of these are checked before any GPU call.  n = 0: TPNET_OK / 0, nothing launched.  Every product is the fp32 class on the matrix
 * cores; sin, the masks and the column sums are plain fp32. */
int tpnet_encoder_input_train(const float* node_raw, int64_t n_node_rows, const float* edge_raw, int64_t n_edge_rows,
                              const int64_t* neigh, const int64_t* eid, const double* tn, const double* tq, const float* tw,
                              const float* tb, const float* feat, int64_t n_nodes, int32_t K, const int32_t* dims, const void* img,
                              float* out, uint32_t* relu_bits, uint32_t* err, void* stream);
size_t tpnet_encoder_input_bwd_image_bytes(int32_t Dn, int32_t Dt, int32_t De, int32_t F, int32_t H, int32_t Dout);
int64_t tpnet_encoder_input_bwd_partial_floats(int32_t Dn, int32_t Dt, int32_t De, int32_t F, int32_t H, int32_t Dout);
size_t tpnet_encoder_input_bwd_workspace_bytes(int64_t n_rows, int32_t Dn, int32_t Dt, int32_t De, int32_t F, int32_t H, int32_t Dout);
int tpnet_encoder_input_bwd_prepare(const float* w1, const float* b1, const float* w2, const int32_t* dims, void* bimg, void* stream);
int tpnet_encoder_input_bwd(const float* node_raw, int64_t n_node_rows, const float* edge_raw, int64_t n_edge_rows, const int64_t* neigh,
                            const int64_t* eid, const double* tn, const double* tq, const float* tw, const float* tb, const float* feat,
                            const uint32_t* relu_bits, const float* gy, int64_t n_nodes, int32_t K, const int32_t* dims,
                            const void* bimg, void* workspace, float* gfeat, int32_t time_grads, float* partial, int32_t n_partial,
                            uint32_t* err, void* stream);

/* ---- self.mlp for num_layer 4, forward and backward (additive to ABI 7; csrc/mlp_l4.hip) --------------------
 * y[n][100] = W2 . relu(W1 . x[n][100] + b1) + b2 for Linear(100, 400) -> ReLU -> Linear(400, 100) in the fp32 class on the matrix
 * cores (two-piece bf16 operands, three products per term, fp32 accumulators), the split weights streamed through LDS from an image.
 * Everything runs on the caller's stream without synchronisation.
 *   tpnet_mlp_l4_supported:  1 only for (F, H) = (100, 400).  Pure host arithmetic.
 *   tpnet_mlp_l4_prepare:    ONE launch that writes the forward's image (tpnet_mlp_l4_image_bytes, 16-byte aligned) from w1 [400][100],
 *                            b1 [400], w2 [100][400], b2 [100]; again whenever one of the four changed.
 *   tpnet_mlp_l4_f32:        ONE launch.  x and y: device, 16-byte aligned, x read only inside its n * 100 floats, y written only inside
 *                            its n * 100 floats.  relu_bits (4-byte aligned; NULL: not recorded) [n][13] uint32: bit u % 32 of word
 *                            u / 32 of a row is (W1 . x + b1)[u] > 0 exactly as this launch decided it; the bits of units 400..415 are 0.
 *                            y has the same bits with and without relu_bits.
 *   tpnet_mlp_l4_bwd_f32:    from gy = dL/dy [n][100] (16-byte aligned) and relu_bits = m, TWO launches:
 *                              a = W1 . x + b1, h = m ? a : 0, gh = W2^T . gy, ga = m ? gh : 0,
 *                              gw1 = sum ga (x) x, gb1 = sum ga, gw2 = sum gy (x) h, gb2 = sum gy           (every sum over the rows)
 *                            No gradient by x is formed.  The decisions are the forward's: read, not recomputed.
 *                            min(n_partial, ceil(n / 32)) or fewer partial sums are written, one per part of the rows.  A partial is
 *                            tpnet_mlp_l4_bwd_partial_floats() = 80 500 floats, laid out gw1 [400][100] | gb1 [400] | gw2 [100][400] |
 *                            gb2 [100], partial i at partial + i * that many floats; `partial` (4-byte aligned) holds n_partial >= 1 of
 *                            them, those beyond the returned count are not written.  Returns that count (>= 0; 0 for n = 0) or a negative
 *                            error.  The caller adds the partials in a fixed order; the kernels use no atomics: two calls give equal bits.
 *                            bimg: the backward's image (tpnet_mlp_l4_bwd_image_bytes; tpnet_mlp_l4_bwd_prepare writes it from w1, b1
 *                            and w2 in ONE launch).  ws: tpnet_mlp_l4_bwd_workspace_bytes(n) = ceil(n / 32) 32 (2 * 416 + 2 * 128) 4 bytes
 *                            (0 for n < 0 or n > 2^31), 16-byte aligned, the call's own: its contents mean nothing before or after.
 * n == 0: TPNET_OK / 0, nothing launched.  TPNET_ERR_BAD_ARG, before any HIP call: a null or misaligned x, y, img (gy, bimg, ws,
 * relu_bits, partial), n < 0 or n > 2^31, n_partial < 1.  A negative code also when the runtime refuses a launch -- the caller then
 * runs the layers its other way.  A row of x that holds a NaN gives unspecified values in THAT row of y and of relu_bits (a NaN hidden
 * unit passes the ReLU as 0, bit 0); every other row is unaffected. */
int tpnet_mlp_l4_supported(int32_t F, int32_t H);
size_t tpnet_mlp_l4_image_bytes(void);
int tpnet_mlp_l4_prepare(const float* w1, const float* b1, const float* w2, const float* b2, void* img, void* stream);
int tpnet_mlp_l4_f32(const float* x, int64_t n, const void* img, float* y, uint32_t* relu_bits, void* stream);
size_t tpnet_mlp_l4_bwd_image_bytes(void);
int tpnet_mlp_l4_bwd_prepare(const float* w1, const float* b1, const float* w2, void* bimg, void* stream);
int64_t tpnet_mlp_l4_bwd_partial_floats(void);
size_t tpnet_mlp_l4_bwd_workspace_bytes(int64_t n);
int tpnet_mlp_l4_bwd_f32(const float* x, const uint32_t* relu_bits, const float* gy, int64_t n, const void* bimg, void* ws,
                         float* partial, int32_t n_partial, void* stream);

/* ---- LinkPredictor_v1 in the fp32 class, forward and backward (additive to ABI 7; csrc/decoder_train.hip) ----
 * out[p] = fc2(relu(fc1(x[p]))), x[p] = concat[src_emb[p], dst_emb[p], feat[p]] (never written), K = 2 D + F:
 *   a = W1 . x + b1 on the matrix cores in the fp32 class (two-piece split operands, three products per term, fp32 accumulators),
 *   logit = sum_u relu(a_u) w2_u + b2 in plain fp32.
 * src_emb, dst_emb: device f32 [n][D] (both NULL = the reference's not_encode mode: zeros, their k-steps skipped); feat: device f32
 * [n][F], NULL exactly where F = 0; w1 [H][K], b1 [H], w2 [H], b2 [1]: fc1 / fc2's Parameters as they are, read and split by the kernels
 * (no image, no prepare call).  src_emb, dst_emb, feat, w1, gsrc, gdst, gfeat and workspace are 16-byte aligned, everything else 4.
 * Served (tpnet_decoder_f32_supported): D % 4 == 0, 0 <= D <= 256, F % 4 == 0, 0 <= F <= 100, D + F > 0, 1 <= H <= 256; 0 <= n < 2^31.
 *   tpnet_decoder_f32:      ONE launch.  out [n].  hidden (may be NULL: not written): relu(a) [n][H] as this launch computed it.
 *   tpnet_decoder_f32_bwd:  from gout = dL/dout [n], TWO launches.  The ReLU's decisions are recomputed: the row-tile kernel runs the
 *                           forward's instruction sequence on the same operands, so its a has the forward's bits.
 *                             ga_u = a_u > 0 ? gout w2_u : 0, gw1 = sum ga (x) x, gb1 = sum ga, gw2_u = sum gout relu(a_u), gb2 = sum gout,
 *                             gsrc | gdst | gfeat = W1^T . ga                                                 (every sum over the rows)
 *                           gsrc, gdst [n][D], gfeat [n][F]: each may be NULL (not computed; all NULL: the product is skipped); gsrc
 *                           and gdst must be NULL where src_emb is.  With src_emb NULL the columns [0, 2 D) of gw1 are zeros.
 *                           min(n_partial, ceil(n / 32)) or fewer partial sums of the four parameter gradients are written, one per
 *                           part of the rows: tpnet_decoder_f32_partial_floats(D, F, H) = H K + 2 H + 1 floats each, laid out
 *                           gw1 [H][K] | gb1 [H] | gw2 [H] | gb2 [1], partial i at partial + i * that many floats; those beyond the
 *                           returned count are not written.  Returns that count (0 for n = 0) or a negative error.  The caller adds
 *                           the partials in a fixed order; no atomics, two calls give equal bits.
 *                           workspace: tpnet_decoder_f32_bwd_workspace_bytes(n, D, F, H) = ceil(n / 32) 32 (2 pad(H) + pad(K) + 1) 4
 *                           bytes, pad(v) = 32 ceil(v / 32); the call's own.  Between the launches it holds, tile by tile of 32 rows,
 *                           relu(a)^T [T][pad(H)][32] | ga^T [T][pad(H)][32] | x^T [T][pad(K)][32] | gout [T][32].
 * The three size entries are host arithmetic and return 0 for an unserved shape.  Null pointers, misaligned arrays, unserved sizes,
 * n < 0, n >= 2^31, n_partial < 1: TPNET_ERR_BAD_ARG, checked before any GPU call.  n = 0: TPNET_OK / 0, nothing launched. */
int tpnet_decoder_f32_supported(int32_t D, int32_t F, int32_t H);
int64_t tpnet_decoder_f32_partial_floats(int32_t D, int32_t F, int32_t H);
size_t tpnet_decoder_f32_bwd_workspace_bytes(int64_t n, int32_t D, int32_t F, int32_t H);
int tpnet_decoder_f32(const float* src_emb, const float* dst_emb, int32_t D, const float* feat, int32_t F, int64_t n, const float* w1,
                      const float* b1, const float* w2, const float* b2, int32_t H, float* out, float* hidden, void* stream);
int tpnet_decoder_f32_bwd(const float* src_emb, const float* dst_emb, int32_t D, const float* feat, int32_t F, int64_t n,
                          const float* w1, const float* b1, const float* w2, int32_t H, const float* gout, void* workspace, float* gsrc,
                          float* gdst, float* gfeat, float* partial, int32_t n_partial, void* stream);

/* ---- the optimizer step on the device (additive to ABI 7; csrc/optimizer.hip) --------------------------------
 * What utils.create_optimizer builds (utils/utils.py:61-79: Adam, SGD or RMSprop with an L2 weight_decay; no amsgrad, momentum 0, not
 * centered) and train_link_prediction.py:386 steps once per batch, for any number of tensors per call: every
 * tpnet_optim_max_tensors() non-empty tensors are ONE launch, a workgroup per tpnet_optim_chunk() elements of a tensor.
 * An entry: p [n] the parameter, g [n] its gradient, s1 / s2 [n] the rule's state, c[8] the rule's scalars, which the caller forms in
 * double and rounds once to fp32 -- so tensors of one call may be at different step counts and carry different hyperparameters:
 *   TPNET_OPTIM_ADAM     s1 = exp_avg, s2 = exp_avg_sq;  c = { lr / (1 - beta1^t), weight_decay, beta1, 1 - beta1, beta2, 1 - beta2,
 *                                                              sqrt(1 - beta2^t), eps }, t = the step being taken (1, 2, ...)
 *   TPNET_OPTIM_SGD      no state (s1, s2 not looked at); c = { lr, weight_decay }
 *   TPNET_OPTIM_RMSPROP  s1 = square_avg (s2 not looked at); c = { lr, weight_decay, alpha, 1 - alpha, eps }
 * Per element, fp32, one rounding per operation, in exactly this order (no fused multiply-add; IEEE division and square root):
 *   g1 = c[1] != 0 ? g + c[1] * p : g
 *   Adam:     s1 = c[2] * s1 + c[3] * g1;  s2 = c[4] * s2 + (c[5] * g1) * g1;  p = p - c[0] * (s1 / (sqrt(s2) / c[6] + c[7]))
 *   SGD:      p = p - c[0] * g1
 *   RMSprop:  s1 = c[2] * s1 + (c[3] * g1) * g1;  p = p - c[0] * (g1 / (sqrt(s1) + c[4]))
 * p, s1 and s2 are updated in place; nothing else is written.  Arrays need 4-byte alignment only: an entry whose arrays are all
 * 16-byte aligned moves 16 bytes per load and store, any other one 4, with the same bits.  The arrays of one call must not overlap.
 * flags and reserved are the library's (a caller's values are not looked at).  All launches go to `stream`; no copy, no
 * synchronisation.  TPNET_ERR_BAD_ARG, before any launch: an unknown rule, count < 0, a null table with count > 0, a null p or g, a
 * null state array that the rule reads, an array that is not 4-byte aligned, n < 0 or n > 2^41.  Entries with n == 0 are skipped. */
#define TPNET_OPTIM_ADAM 0
#define TPNET_OPTIM_SGD 1
#define TPNET_OPTIM_RMSPROP 2
typedef struct tpnet_optim_tensor {
    float* p;
    const float* g;
    float* s1;
    float* s2;
    int64_t n;
    float c[8];
    uint32_t flags;
    uint32_t reserved;
} tpnet_optim_tensor; /* 80 bytes */
int tpnet_optim_max_tensors(void);
int tpnet_optim_chunk(void);
int tpnet_optim_step(int rule, const tpnet_optim_tensor* tensors, int32_t count, void* stream);

/* Copies st->err to the host (synchronises the stream): returns TPNET_ERR_INDEX if any bad id was seen since
 * the last call (and clears the words), TPNET_OK otherwise. */
int tpnet_check_errors(const tpnet_state* st, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TPNET_HIP_H */
