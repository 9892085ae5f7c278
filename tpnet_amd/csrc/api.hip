// C ABI (include/tpnet_hip.h): argument checks, workspace carving, launch sequencing.  No allocation, no implicit
// synchronisation; everything is enqueued on the caller's stream.
#include "tpnet_common.h"

#include <cstring>

namespace tpnet {
thread_local int g_last_hip_error = 0;

int check_state(const tpnet_state* st) {
    if (!st || !st->p0 || !st->q || !st->meta || !st->err) return TPNET_ERR_BAD_ARG;
    if (st->N < 1 || st->d < 1 || st->L < 1 || st->L > TPNET_MAX_LAYERS) return TPNET_ERR_BAD_ARG;
    if (st->N >= (1ll << 31)) return TPNET_ERR_BAD_ARG;
    return TPNET_OK;
}

// the largest n < hi with fits(n), where fits(hi) is false and fits grows no truer with n; 0: none
template <class F> static int64_t most_that_fit(int64_t hi, F fits) {
    int64_t lo = 0;
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) / 2;
        if (fits(mid)) lo = mid; else hi = mid;
    }
    return lo;
}

// largest chunk (multiple of `batch`, at most E) whose plan fits the workspace.  Contribution indices are 32-bit inside a
// chunk (Item::j0, the sort's payload), so a chunk never exceeds 2^30 edges however large the workspace is.
static int64_t max_chunk(size_t ws_bytes, int64_t E, int64_t batch) {
    const int64_t hard = ((int64_t)1 << 30) / batch * batch;
    const int64_t lim = (E < hard || hard < batch) ? E : hard;
    if (plan_bytes(lim, batch) <= ws_bytes) return lim;
    return batch * most_that_fit((lim + batch - 1) / batch, [&](int64_t n) { return plan_bytes(n * batch, batch) <= ws_bytes; });
}

struct StepTimer {
    hipEvent_t* ev = nullptr;  // one pair per chunk, around its loop of step launches (plan kernels excluded)
    int64_t n = 0, cap = 0;    // pairs recorded / available
    int64_t launches = 0;      // step launches between the recorded pairs
    int64_t edges = 0;         // edges those launches covered
    bool begin(hipStream_t s) { return n < cap && ((void)hipEventRecord(ev[2 * n], s), true); }      // false: no pair left
    void end(hipStream_t s, int64_t nl, int64_t ne) { (void)hipEventRecord(ev[2 * n + 1], s); ++n; launches += nl; edges += ne; }
};

// The plans of a multi-chunk stream side by side -- one region per chunk, each with every array of a plan but the version log --
// in front of ONE version log: what lets a stream of several chunks be replayed (run_stream_windowed).  At most 64 chunks.
constexpr int64_t ARENA_MAX_CHUNKS = 64;
static size_t arena_region_bytes(int64_t N, int d, int L, int64_t chunk, int64_t batch) {
    return (wplan_bytes(chunk, batch, N, d, L) - wplan_log_bytes(chunk, d, L) + 511) / 256 * 256;
}
static size_t arena_bytes(int64_t N, int d, int L, int64_t E, int64_t chunk, int64_t batch) {
    const int64_t n = (E + chunk - 1) / chunk;
    return (size_t)n * arena_region_bytes(N, d, L, chunk, batch) + wplan_log_bytes(chunk, d, L) + 512;
}

// edges per window (*Ew_out) and the most a chunk may cover whatever the workspace (whole windows, or all of E); 0: not windowed
static int64_t window_chunk_limit(const tpnet_state& st, int64_t E, int64_t batch, uint32_t flags, int* K_out, int64_t* Ew_out) {
    const int K = wplan_window_batches(batch, st.d, st.L);
    if (K == 0) return 0;
    *K_out = K;
    int64_t Ew = (int64_t)K * batch;
    // packed rows of (2L+2)(2L+3)/2 floats: every chunk's output must start on a 16-byte boundary (launch_wstep)
    const int NN = 2 * st.L + 2;
    if ((flags & TPNET_FLAG_PACKED) && ((NN * (NN + 1) / 2) % 4) != 0 && Ew % 4 != 0) Ew *= (Ew % 2 == 0) ? 2 : 4;
    *Ew_out = Ew;
    int64_t cap = wplan_max_chunk_edges(batch, st.d, st.L);           // the version log of a chunk is bounded, and
    const int64_t maxw = choose_wplanner(st, nullptr, 0, batch, 0, flags).max_windows;      // so are the windows its planner serves
    if (maxw > 0 && cap > maxw * Ew) cap = maxw * Ew;
    const int64_t hard = cap / Ew * Ew;
    return (E <= cap) ? E : hard;
}

// The windowed path (wstep.hip) serves a stream when its arithmetic contract allows it (no eager decay / strictly
// sequential sums: those are the per-batch kernels' exact mode), the rows take 16-byte vectors, there are enough batches
// for a window to pay, and the caller's workspace holds the plan of at least one window.  Returns the chunk (edges per
// plan: whole windows of Kmax batches, or all of E) and Kmax; 0 = use the per-batch path.  `region_out` (may be null: the caller
// has no use for a replayable layout): set to the bytes per chunk region where the stream takes several chunks and the workspace
// holds them side by side (arena_bytes), else to 0.
static int64_t window_chunk(const tpnet_state& st, size_t ws_bytes, int64_t E, int64_t batch, uint32_t flags, int* K_out,
                            size_t* region_out = nullptr) {
    if (region_out) *region_out = 0;
    if (flags & (TPNET_FLAG_EAGER_DECAY | TPNET_FLAG_SEQUENTIAL | TPNET_FLAG_SCHED_BATCH)) return 0;
    const int64_t nb = (E + batch - 1) / batch;
    // short streams: the pipeline pays its plan (~31 us for 20 C2 batches with the dense planner, wplan_dense.hip) and L + 1 dependent
    // launches up front, the per-batch schedule ~20 us and ~6.6 us per batch (C2): the pipeline wins from 16 batches
    // (tools/short_sweep.py, round 4: 14 batches 138 against 134 us, 16: 135 against 145, 20: 143-158 against 173-179, 24: 157 against
    // 198; until round 4, with the hashed planner and lane-group walks of chains up to 52 contributions: from 24).  Larger batches keep
    // the chunk planner's crossover (two device-wide sorts).
    static const int min_nb3 = TPNET_DEV_INT(WIN_MIN_BATCHES, 16);
    const int64_t min_nb = (flags & TPNET_FLAG_SCHED_WINDOWED) ? 4 : (batch <= PLAN_ONE_MAX ? min_nb3 : 56);
    int64_t Ew = 0;
    const int64_t lim = window_chunk_limit(st, E, batch, flags, K_out, &Ew);
    if (lim == 0 || nb < min_nb) return 0;
    if ((lim + batch - 1) / batch < 4) return 0;
    // does a chunk of c edges fit -- as one region of an arena (every chunk's plan kept, side by side: several chunks, at most
    // ARENA_MAX_CHUNKS, and a planner that keeps something to replay), or as a plan on its own
    const bool arena_ok = region_out && choose_wplanner(st, nullptr, 0, batch, 0, flags).replayable;
    auto fits = [&](int64_t c, bool arena) {
        if (!arena) return wplan_bytes(c, batch, st.N, st.d, st.L) <= ws_bytes;
        return arena_ok && c < E && (E + c - 1) / c <= ARENA_MAX_CHUNKS && arena_bytes(st.N, st.d, st.L, E, c, batch) <= ws_bytes;
    };
    auto take = [&](int64_t c, bool arena) { if (arena) *region_out = arena_region_bytes(st.N, st.d, st.L, c, batch); return c; };
    // in order of preference.  The whole stream as one chunk:
    const bool lim_fits = fits(lim, false);
    if (lim_fits && lim >= E) return lim;
    // several chunks of whole windows, at least four batches each, in an arena: the largest chunk that fits (the log grows with the
    // chunk, the per-node arrays of the regions with the number of chunks: not monotone, and at most 256 candidates)
    for (int64_t w = arena_ok ? lim / Ew : 0; w * Ew >= 4 * batch; --w)
        if (fits(w * Ew, true)) return take(w * Ew, true);
    // the largest chunk its planner serves, else the most whole windows, planned anew every time
    if (lim_fits) return lim;
    const int64_t nw = most_that_fit((lim + Ew - 1) / Ew, [&](int64_t w) { return fits(w * Ew, false); });
    if (nw > 0) return nw * Ew;
    // not even one window of Kmax batches (a caller who capped the version log below that): chunks of fewer batches -- the window
    // length is chosen per chunk (window_batches_for) -- down to what the pipeline still wins at; a replayable layout first
    const int K = *K_out;
    const int64_t u = Ew / K;                                              // one batch (packed rows: whole 16 bytes of output)
    for (const bool arena : {true, false})
        for (int64_t n = K - 1; n >= 1 && n * u >= min_nb * batch; --n)
            if (n * u < E && fits(n * u, arena)) return take(n * u, arena);
    return 0;
}

// what a plan left in the workspace was built for (tpnet_plan_tag::built, opaque to the caller)
struct PlanBuilt {
    uint64_t valid;             // 1: a windowed plan, 2: a per-batch one
    const void *src, *dst, *t, *ws;
    int64_t E, batch, N;
    uint64_t ws_bytes;
    double now_time, lambda;
    int32_t d, L, K;
    uint32_t flags;
    uint64_t table_sig, stream_sig;
    uint64_t have_readout;
    int64_t chunk;              // edges per chunk, and
    uint64_t region;            // bytes per chunk region where the stream is several chunks (0: one chunk)
};
static_assert(sizeof(PlanBuilt) <= sizeof(((tpnet_plan_tag*)nullptr)->built), "tpnet_plan_tag::built too small");

// one tpnet_run_stream call
struct StreamCall {
    const tpnet_state& st;
    const int64_t *src, *dst, *neg;
    const double* t;
    int64_t E, batch;
    double now_time, lambda;
    uint32_t launch_id_base, flags;
    float *out_pos, *out_neg;
    void* ws;
    size_t ws_bytes;
    hipStream_t s;
    StepTimer* timer;
    tpnet_plan_tag* tag;
    StreamArgs args_at(int64_t c0) const {
        const int NN = 2 * st.L + 2;            // floats per feature row of the outputs: NN x NN, or its upper triangle
        return stream_args_at(src, dst, neg, t, out_pos, out_neg, c0, (flags & TPNET_FLAG_PACKED) ? NN * (NN + 1) / 2 : NN * NN);
    }
};

// The caller's tag for one call: may the plan in the workspace be replayed (`possible`: the schedule can do so at all, if the caller
// vouches for the stream and, with_table, for the table's per-node state), and the record -- a byte image -- of what this call leaves there
struct PlanReplay {
    tpnet_plan_tag* const tag;
    PlanBuilt now;
    bool replay = false;
    PlanReplay(const StreamCall& c, bool possible, uint64_t valid, bool with_table, int K, uint32_t flags, bool have_readout,
               int64_t chunk, size_t region) : tag(c.tag) {
        memset(&now, 0, sizeof(now));
        if (!tag) return;
        if (possible && tag->stream_sig && (!with_table || tag->table_sig)) {
            now.valid = valid; now.src = c.src; now.dst = c.dst; now.t = c.t; now.ws = c.ws; now.E = c.E; now.batch = c.batch;
            now.N = c.st.N; now.ws_bytes = c.ws_bytes; now.now_time = c.now_time; now.lambda = c.lambda; now.d = c.st.d; now.L = c.st.L;
            now.K = K; now.flags = flags; now.table_sig = with_table ? tag->table_sig : 0; now.stream_sig = tag->stream_sig;
            now.have_readout = have_readout ? 1 : 0; now.chunk = chunk; now.region = region;
            replay = memcmp(&now, tag->built, sizeof(PlanBuilt)) == 0;
        }
        memset(tag->built, 0, sizeof(tag->built));                   // (invalid unless this call completes: commit)
        tag->replayed = replay ? 1 : 0;
    }
    // the call completed; all_kept: every chunk's plan is still in the workspace (planned by a planner that keeps it)
    void commit(bool all_kept) { if (now.valid && all_kept) memcpy(tag->built, &now, sizeof(PlanBuilt)); }
};

static int run_stream_windowed(const StreamCall& c, int64_t chunk, int Kmax, size_t region) {
    const tpnet_state& st = c.st;
    const int64_t E = c.E, batch = c.batch;
    hipStream_t s = c.s;
    uint32_t lid = c.launch_id_base;
    const bool have_readout = c.out_pos || c.out_neg;
    // a plan may be replayed when the caller vouches (tag) that the stream arrays and the table's per-node state are what the
    // plan in this workspace was built for, and the workspace still holds the plan of EVERY chunk: the stream is one chunk, or
    // its chunks' plans lie side by side (`region` bytes each, window_chunk) in front of the one version log they share -- the
    // table state a later chunk's plan was built on follows from the first one's and the stream
    char* const arena = reinterpret_cast<char*>((reinterpret_cast<size_t>(c.ws) + 255) / 256 * 256);
    const int64_t n_chunks = (E + chunk - 1) / chunk;
    float* const shared_log = region ? reinterpret_cast<float*>(arena + (size_t)n_chunks * region) : nullptr;
    PlanReplay tag(c, n_chunks == 1 || region, 1, true, window_batches_for(((E < chunk ? E : chunk) + batch - 1) / batch, Kmax),
                   c.flags & ~(uint32_t)TPNET_FLAG_SCHED_WINDOWED, have_readout, chunk, region);
    bool all_kept = true;
    for (int64_t c0 = 0, ci = 0; c0 < E; c0 += chunk, ++lid, ++ci) {
        const int64_t Ec = (E - c0 < chunk) ? (E - c0) : chunk;
        const int64_t nb = (Ec + batch - 1) / batch;
        const int K = window_batches_for(nb, Kmax);
        WPlan p{};
        int rc = region ? wplan_carve(arena + (size_t)ci * region, region, Ec, batch, st.N, st.d, st.L, K, &p, shared_log)
                        : wplan_carve(c.ws, c.ws_bytes, Ec, batch, st.N, st.d, st.L, K, &p);
        if (rc) return rc;
        // (the sorted planner keeps nothing to replay: a stream with such a chunk is planned again every time; a recorded plan had
        // none, and the same sizes choose the same planners)
        const WPlanner planner = choose_wplanner(st, &p, Ec, batch, K, c.flags);
        all_kept &= planner.replayable;
        const StreamArgs a = c.args_at(c0);
        const WPlanArgs pa{a.src, a.dst, a.neg, a.t, Ec, batch, c.now_time, c0 > 0 ? c.t + c0 - 1 : nullptr, c.lambda, have_readout,
                           tag.replay};
        rc = planner.build(st, p, pa, s);
        if (rc) return rc;
        const int64_t nw = (Ec + p.Ew - 1) / p.Ew;
        const int64_t nsteps = nw + (have_readout ? st.L : st.L - 1);
        const bool timed = c.timer && c.timer->begin(s);
        for (int64_t j = 0; j < nsteps; ++j) {
            rc = launch_wstep(st, a, p, j, Ec, batch, c.lambda, c.flags, s);
            if (rc) return rc;
        }
        if (timed) c.timer->end(s, nsteps, Ec);
        // the write-back: node by node where the dense or the hashed planner planned the chunk (wplan3.hip: 9 us for the 158-batch
        // epoch), else the scan of the sorted positions for the last-run flag (wstep.hip: 25 us).  (Measured and not kept, round 3: the
        // write-back as extra blocks of the chunk's last pipeline step -- readouts only, nothing it reads is written -- grew that
        // step by what the write-back takes alone, leading the grid or not, and every other step by ~2 us: 634 against 635 us for
        // the epoch; a write-back driven by chain records that carry (last chain of the node, table copy, last clock): 30 us.)
        rc = planner.writeback(st, p, Ec, batch, lid, s, -1);
        if (rc) return rc;
    }
    tag.commit(all_kept);
    return TPNET_OK;
}

static int run_stream_impl(const StreamCall& c) {
    const tpnet_state& st = c.st;
    const int64_t E = c.E, batch = c.batch;
    const double lambda = c.lambda;
    const uint32_t flags = c.flags;
    hipStream_t s = c.s;
    if (E == 0) return TPNET_OK;
    int Kw = 0;
    size_t region = 0;
    const int64_t wchunk = window_chunk(st, c.ws_bytes, E, batch, flags, &Kw, c.tag ? &region : nullptr);
    if (wchunk > 0) return run_stream_windowed(c, wchunk, Kw, region);
    const int64_t chunk = max_chunk(c.ws_bytes, E, batch);
    // the per-batch plan of a stream (item lists, coefficients, batch descriptors: plan.hip) is a function of src / dst / t, the
    // clock at entry and the flags alone -- not of the table -- and the step kernels only read it: a stream that is ONE chunk (up
    // to ~2 M edges: every dataset of the reference at any batch size) replays it when the caller vouches for the arrays
    // (tag->stream_sig; table_sig is not looked at).  (have_readout: the edge-fused update's lists exist for a (src, dst) readout only)
    PlanReplay tag(c, chunk >= E, 2, false, 0, flags, c.out_pos != nullptr, chunk, 0);
    if (chunk < 1) return TPNET_ERR_WORKSPACE;
    uint32_t lid = c.launch_id_base;
    for (int64_t c0 = 0; c0 < E; c0 += chunk) {
        const int64_t Ec = (E - c0 < chunk) ? (E - c0) : chunk;
        Plan p{};
        int rc = plan_carve(c.ws, c.ws_bytes, Ec, batch, &p);
        if (rc) return rc;
        // edge-fused updates: every launch of this chunk must run BOTH roles with the (src,dst) readout on, and the sums
        // must not be order-sensitive by contract; worth it where the batch is bound by bytes, not by its longest chain
        static const int fuse_env = TPNET_DEV_INT(FUSE, -1);       // developer override: 0 / 1
        static const int role_mask = TPNET_DEV_INT(ROLE_MASK, 3);   // developer override: 1 / 2 / 3 = readout only / update only / both
        const bool fuse = c.out_pos && p.fuse_src && role_mask == 3 &&
                          !(flags & (TPNET_FLAG_EAGER_DECAY | TPNET_FLAG_SEQUENTIAL)) &&
                          (fuse_env >= 0 ? fuse_env == 1 : batch > 1024);
        const StreamArgs a = c.args_at(c0);
        // the clock before a later chunk is t[c0-1], read on device (no host copy of the timestamps is needed)
        if (!tag.replay) {
            rc = plan_build(st, p, a.src, a.dst, a.t, Ec, batch, c.now_time, c0 > 0 ? c.t + c0 - 1 : nullptr, lambda,
                            flags | (fuse ? PLAN_FUSE : 0u), s);
            if (rc) return rc;
        }
        const int64_t nb = (Ec + batch - 1) / batch;
        const bool have_readout = a.out_pos || a.out_neg;
        const bool timed = c.timer && !(flags & TPNET_FLAG_EAGER_DECAY) && c.timer->begin(s);
        for (int64_t b = 0; b < nb; ++b, ++lid) {
            const int32_t ne = (int32_t)((Ec - b * batch < batch) ? (Ec - b * batch) : batch);
            if (flags & TPNET_FLAG_EAGER_DECAY) {
                // reference order: readout on the pre-batch state, THEN decay + scatter-add (TPNet.py:83-96)
                if (have_readout) {
                    rc = launch_step(st, a, p, b, batch, ne, lambda, lid, flags | ROLE_READOUT, s);
                    if (rc) return rc;
                }
                rc = launch_decay_desc(st, p, b, s);
                if (rc) return rc;
                rc = launch_step(st, a, p, b, batch, ne, lambda, lid, flags | ROLE_UPDATE, s);
                if (rc) return rc;
            } else {
                const uint32_t roles = ((role_mask & 2) ? ROLE_UPDATE : 0u) |
                                       ((have_readout && (role_mask & 1)) ? ROLE_READOUT : 0u);
                rc = launch_step(st, a, p, b, batch, ne, lambda, lid, flags | roles | (fuse ? STEP_FUSE : 0u), s);
                if (rc) return rc;
            }
        }
        if (timed) c.timer->end(s, nb, Ec);
    }
    tag.commit(true);
    return TPNET_OK;
}

}  // namespace tpnet

using namespace tpnet;

extern "C" {

const char* tpnet_strerror(int status) {
    switch (status) {
        case TPNET_OK: return "ok";
        case TPNET_ERR_BAD_ARG: return "bad argument";
        case TPNET_ERR_WORKSPACE: return "workspace missing or too small";
        case TPNET_ERR_HIP: return "HIP runtime error";
        case TPNET_ERR_INDEX: return "node id out of range";
        case TPNET_ERR_NO_DEVICE: return "no HIP device";
        case TPNET_ERR_NEED_GRAM: return "the one-launch encoder kernel is not available: call again with a gram buffer";
        default: return "unknown status";
    }
}

int tpnet_abi_version(void) { return TPNET_ABI_VERSION; }
int tpnet_last_hip_error(void) { return g_last_hip_error; }

int tpnet_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

size_t tpnet_q_bytes(int64_t N, int32_t d, int32_t L) { return (size_t)2 * (size_t)N * (size_t)L * (size_t)d * sizeof(float); }
size_t tpnet_meta_bytes(int64_t N) { return (size_t)N * sizeof(tpnet_node_meta); }

int tpnet_state_init(const tpnet_state* st, double t0, void* stream) {
    int rc = check_state(st);
    if (rc) return rc;
    return launch_state_init(*st, t0, (hipStream_t)stream);
}

int tpnet_import_layers(const tpnet_state* st, const float* const* layers, double now_time, void* stream) {
    int rc = check_state(st);
    if (rc) return rc;
    if (!layers) return TPNET_ERR_BAD_ARG;
    for (int i = 0; i < st->L; ++i)
        if (!layers[i]) return TPNET_ERR_BAD_ARG;
    return launch_import(*st, layers, now_time, (hipStream_t)stream);
}

int tpnet_export_layers(const tpnet_state* st, float* const* layers, double now_time, double lambda, void* stream) {
    int rc = check_state(st);
    if (rc) return rc;
    if (!layers) return TPNET_ERR_BAD_ARG;
    for (int i = 0; i < st->L; ++i)
        if (!layers[i]) return TPNET_ERR_BAD_ARG;
    return launch_export(*st, layers, now_time, lambda, (hipStream_t)stream);
}

int tpnet_decay(const tpnet_state* st, const float* factors, double t_new, void* stream) {
    int rc = check_state(st);
    if (rc) return rc;
    if (!factors) return TPNET_ERR_BAD_ARG;
    return launch_decay(*st, factors, t_new, (hipStream_t)stream);
}

int tpnet_gather_rows(const tpnet_state* st, const int64_t* ids, int64_t n, double now_time, double lambda, float* out,
                      void* stream) {
    int rc = check_state(st);
    if (rc) return rc;
    if (n < 0 || (n > 0 && (!ids || !out))) return TPNET_ERR_BAD_ARG;
    return launch_gather_rows(*st, ids, n, now_time, lambda, out, (hipStream_t)stream);
}

// the wide side of the *_ld entry points: whole 16-byte vectors at 16-byte aligned addresses
static bool wide_ok(const void* p, int32_t d) { return p && d >= 4 && d % 4 == 0 && (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

int tpnet_import_layers_ld(const tpnet_state* st, const float* const* layers, int32_t ld, double now_time, void* stream) {
    int rc = check_state(st);
    if (rc) return rc;
    if (!layers || ld < 1 || ld > st->d || !wide_ok(st->q, st->d)) return TPNET_ERR_BAD_ARG;
    for (int i = 0; i < st->L; ++i)
        if (!layers[i]) return TPNET_ERR_BAD_ARG;
    return launch_import_ld(*st, layers, ld, now_time, (hipStream_t)stream);
}

int tpnet_export_layers_ld(const tpnet_state* st, float* const* layers, int32_t ld, double now_time, double lambda, void* stream) {
    int rc = check_state(st);
    if (rc) return rc;
    if (!layers || ld < 1 || ld > st->d || !wide_ok(st->q, st->d)) return TPNET_ERR_BAD_ARG;
    for (int i = 0; i < st->L; ++i)
        if (!layers[i]) return TPNET_ERR_BAD_ARG;
    return launch_export_ld(*st, layers, ld, now_time, lambda, (hipStream_t)stream);
}

int tpnet_pad_rows(const float* src, int32_t ld_src, float* dst, int32_t ld_dst, int64_t N, void* stream) {
    if (!src || ld_src < 1 || ld_src > ld_dst || !wide_ok(dst, ld_dst) || N < 0 || N >= (1ll << 31)) return TPNET_ERR_BAD_ARG;
    return launch_pad_rows(src, ld_src, dst, ld_dst, N, (hipStream_t)stream);
}

int tpnet_gather_rows_ld(const tpnet_state* st, const int64_t* ids, int64_t n, double now_time, double lambda, int32_t ld_out,
                         float* out, void* stream) {
    int rc = check_state(st);
    if (rc) return rc;
    if (n < 0 || !ids || !out || ld_out < 1 || ld_out > st->d || !wide_ok(st->q, st->d) || !wide_ok(st->p0, st->d))
        return TPNET_ERR_BAD_ARG;
    return launch_gather_rows_ld(*st, ids, n, now_time, lambda, ld_out, out, (hipStream_t)stream);
}

int tpnet_gather_elems(const tpnet_state* st, const int64_t* rows, const int64_t* cols, int64_t n, double now_time,
                       double lambda, float* out, void* stream) {
    int rc = check_state(st);
    if (rc) return rc;
    if (n < 0 || (n > 0 && (!rows || !cols || !out))) return TPNET_ERR_BAD_ARG;
    return launch_gather_elems(*st, rows, cols, n, now_time, lambda, out, (hipStream_t)stream);
}

int tpnet_pair_gram(const tpnet_state* st, const int64_t* u, const int64_t* v, int64_t n, double now_time,
                    double lambda, uint32_t flags, float* out, void* stream) {
    int rc = check_state(st);
    if (rc) return rc;
    if (n < 0 || (n > 0 && (!u || !v || !out))) return TPNET_ERR_BAD_ARG;
    return launch_pair_gram(*st, u, v, n, now_time, lambda, flags, out, (hipStream_t)stream);
}

int tpnet_pair_gram_shared(const tpnet_state* st, const int64_t* u, const int64_t* v1, const int64_t* v2, int64_t n,
                           double now_time, double lambda, uint32_t flags, float* out1, float* out2, void* stream) {
    int rc = check_state(st);
    if (rc) return rc;
    if (n < 0 || (n > 0 && (!u || !v1 || !v2 || !out1 || !out2))) return TPNET_ERR_BAD_ARG;
    if (flags & TPNET_FLAG_PACKED) return TPNET_ERR_BAD_ARG;   // packed rows exist for the one-pair readout only
    return launch_pair_gram_shared(*st, u, v1, v2, n, now_time, lambda, flags, out1, out2, (hipStream_t)stream);
}

int tpnet_pair_gram_anchored(const tpnet_state* st, const int64_t* neigh, const int64_t* a1, const int64_t* a2,
                             int64_t n_rows, int32_t K, double now_time, double lambda, uint32_t flags, float* out1,
                             float* out2, void* stream) {
    int rc = check_state(st);
    if (rc) return rc;
    if (n_rows < 0 || K < 0 || (n_rows > 0 && K > 0 && (!neigh || !a1 || !a2 || !out1 || !out2))) return TPNET_ERR_BAD_ARG;
    if (flags & TPNET_FLAG_PACKED) return TPNET_ERR_BAD_ARG;
    if (n_rows == 0 || K == 0) return TPNET_OK;
    hipStream_t s = (hipStream_t)stream;
    switch (anchored_route(*st, n_rows, K, flags, nullptr, aligned16({out1, out2}), false).gram) {
        // rows of 36..160 floats, L = 3, K >= 4 (8-byte rows with TPNET_FLAG_ROWS8 among them): the matrix cores (encoder_mfma.hip, fp32 class)
        case AK_MFMA: return launch_encoder_gram_mfma(*st, neigh, a1, a2, n_rows, K, now_time, lambda, flags, out1, out2, s);
        // L = 1, 2, 4 on the matrix cores (encoder_layers.hip): only with TPNET_FLAG_LAYERS_MFMA, same shapes otherwise
        case AK_LAYERS: return launch_encoder_gram_layers(*st, neigh, a1, a2, n_rows, K, now_time, lambda, flags, out1, out2, s);
        // everything else that is supported (K < 4, unaligned outputs, wider rows, TPNET_FLAG_NO_MFMA_READOUT): the vector-ALU walk
        case AK_WALK: return launch_pair_gram_anchored(*st, neigh, a1, a2, n_rows, K, now_time, lambda, flags, out1, out2, s);
        // rows that are not whole 16-byte vectors (d % 4 != 0: 110, 130, 150 ... without the flag), narrower than 36 or wider than 512
        // floats: the generic kernel, one launch per anchor side, on index arrays the caller would otherwise build -- not available
        // without them: report it
        default: return TPNET_ERR_BAD_ARG;
    }
}

int tpnet_pair_gram_fanout(const tpnet_state* st, const int64_t* src, const int64_t* cand, int64_t n_rows, int32_t C,
                           double now_time, double lambda, uint32_t flags, float* out, void* stream) {
    int rc = check_state(st);
    if (rc) return rc;
    if (n_rows < 0 || C <= 0 || !src || !cand || !out || (reinterpret_cast<uintptr_t>(out) & 15)) return TPNET_ERR_BAD_ARG;
    if (n_rows >= (1ll << 31) / C) return TPNET_ERR_BAD_ARG;
    if (flags & TPNET_FLAG_PACKED) return TPNET_ERR_BAD_ARG;   // packed rows exist for the one-pair readout only
    if (n_rows == 0) return TPNET_OK;
    if (!pair_gram_fanout_supported(*st)) return TPNET_ERR_BAD_ARG;   // (narrow or odd rows: the caller expands and takes tpnet_pair_gram)
    return launch_pair_gram_fanout(*st, src, cand, n_rows, C, now_time, lambda, flags, out, (hipStream_t)stream);
}

int tpnet_pair_gram_fanout_supported(const tpnet_state* st) {
    if (check_state(st)) return 0;
    return pair_gram_fanout_supported(*st) ? 1 : 0;
}

int tpnet_score_one_to_many_supported(const tpnet_state* st, const tpnet_mlp* mlp, int32_t H, int32_t off, int32_t ldw) {
    if (check_state(st)) return 0;
    return score_fanout_supported(*st, mlp, H, off, ldw) ? 1 : 0;
}

int tpnet_score_one_to_many(const tpnet_state* st, const int64_t* src, const int64_t* cand, int64_t cand_lo, const int64_t* lead,
                            int64_t n_rows, int32_t C, double now_time, double lambda, uint32_t flags, const tpnet_mlp* mlp,
                            const float* wd, int32_t ldw, int32_t off, const float* bd, const float* wd2, const float* bd2, int32_t H,
                            float* gram, float* out, void* stream) {
    int rc = check_state(st);
    if (rc) return rc;
    if (n_rows < 0 || C <= 0 || !src || !out || !mlp || !wd || !bd || !wd2 || !bd2) return TPNET_ERR_BAD_ARG;
    if (!aligned16({gram, wd, mlp->w1, mlp->w2f, mlp->b2}) ||
        ((reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(bd) | reinterpret_cast<uintptr_t>(wd2) |
          reinterpret_cast<uintptr_t>(bd2) | reinterpret_cast<uintptr_t>(mlp->b1)) & 3))
        return TPNET_ERR_BAD_ARG;
    if (n_rows > ((1ll << 31) - 1) / ((int64_t)C + 1)) return TPNET_ERR_BAD_ARG;        // n_rows (1 + C) < 2^31
    if (flags & TPNET_FLAG_PACKED) return TPNET_ERR_BAD_ARG;   // packed rows exist for the one-pair readout only
    if (!cand && (cand_lo < 0 || cand_lo > st->N - (int64_t)C)) return TPNET_ERR_BAD_ARG;   // the range lies inside [0, N)
    if (!score_fanout_supported(*st, mlp, H, off, ldw)) return TPNET_ERR_BAD_ARG;       // (the caller takes the composition)
    if (n_rows == 0) return TPNET_OK;
    return launch_score_fanout(*st, src, cand, cand_lo, lead, n_rows, C, now_time, lambda, flags, mlp, wd, ldw, off, bd, wd2, bd2, H,
                               gram, out, (hipStream_t)stream);
}

size_t tpnet_score_rank_scratch_bytes(int64_t n_rows, int32_t C) { return score_rank_scratch_bytes(n_rows, C); }

int tpnet_score_rank_range(const tpnet_state* st, const int64_t* src, const int64_t* pos, int64_t cand_lo, int64_t n_rows, int32_t C,
                           double now_time, double lambda, uint32_t flags, const tpnet_mlp* mlp, const float* wd, int32_t ldw,
                           int32_t off, const float* bd, const float* wd2, const float* bd2, int32_t H, void* scratch,
                           size_t scratch_bytes, float* pos_logit, int32_t* counts, void* stream) {
    int rc = check_state(st);
    if (rc) return rc;
    if (n_rows < 0 || n_rows >= (1ll << 31) || C <= 0 || !src || !pos || !pos_logit || !counts || !scratch || !mlp || !wd || !bd ||
        !wd2 || !bd2)
        return TPNET_ERR_BAD_ARG;
    if (!aligned16({wd, mlp->w1, mlp->w2f, mlp->b2, scratch, counts}) ||
        ((reinterpret_cast<uintptr_t>(pos_logit) | reinterpret_cast<uintptr_t>(bd) | reinterpret_cast<uintptr_t>(wd2) |
          reinterpret_cast<uintptr_t>(bd2) | reinterpret_cast<uintptr_t>(mlp->b1)) & 3))
        return TPNET_ERR_BAD_ARG;
    if (flags & TPNET_FLAG_PACKED) return TPNET_ERR_BAD_ARG;   // packed rows exist for the one-pair readout only
    if (cand_lo < 0 || cand_lo > st->N - (int64_t)C) return TPNET_ERR_BAD_ARG;             // the range lies inside [0, N)
    if (!score_fanout_supported(*st, mlp, H, off, ldw)) return TPNET_ERR_BAD_ARG;       // (the caller takes the composition)
    if (n_rows == 0) return TPNET_OK;
    return launch_score_rank(*st, src, pos, cand_lo, n_rows, C, now_time, lambda, flags, mlp, wd, ldw, off, bd, wd2, bd2, H, scratch,
                             scratch_bytes, pos_logit, counts, (hipStream_t)stream);
}

size_t tpnet_score_topk_scratch_bytes(int64_t n_rows, int32_t C, int32_t K) { return score_topk_scratch_bytes(n_rows, C, K); }

int tpnet_score_topk_range(const tpnet_state* st, const int64_t* src, const int64_t* skip, const int64_t* excl, const int32_t* n_excl,
                           int32_t F, int64_t cand_lo, int64_t n_rows, int32_t C, int32_t K, double now_time, double lambda,
                           uint32_t flags, const tpnet_mlp* mlp, const float* wd, int32_t ldw, int32_t off, const float* bd,
                           const float* wd2, const float* bd2, int32_t H, void* scratch, size_t scratch_bytes, int64_t* ids,
                           float* logits, int32_t* info, void* stream) {
    int rc = check_state(st);
    if (rc) return rc;
    if (n_rows < 0 || n_rows >= (1ll << 31) || C <= 0 || !src || !ids || !logits || !info || !scratch || !mlp || !wd || !bd || !wd2 ||
        !bd2)
        return TPNET_ERR_BAD_ARG;
    if (K < 1 || K > SCORE_TOPK_MAX) return TPNET_ERR_BAD_ARG;
    if (excl && (!n_excl || F < 1)) return TPNET_ERR_BAD_ARG;
    if (!aligned16({wd, mlp->w1, mlp->w2f, mlp->b2, scratch}) ||
        ((reinterpret_cast<uintptr_t>(ids) | reinterpret_cast<uintptr_t>(skip) | reinterpret_cast<uintptr_t>(excl)) & 7) ||
        ((reinterpret_cast<uintptr_t>(logits) | reinterpret_cast<uintptr_t>(info) | reinterpret_cast<uintptr_t>(n_excl) |
          reinterpret_cast<uintptr_t>(bd) | reinterpret_cast<uintptr_t>(wd2) | reinterpret_cast<uintptr_t>(bd2) |
          reinterpret_cast<uintptr_t>(mlp->b1)) & 3))
        return TPNET_ERR_BAD_ARG;
    if (flags & TPNET_FLAG_PACKED) return TPNET_ERR_BAD_ARG;   // packed rows exist for the one-pair readout only
    if (cand_lo < 0 || cand_lo > st->N - (int64_t)C) return TPNET_ERR_BAD_ARG;             // the range lies inside [0, N)
    if (!score_fanout_supported(*st, mlp, H, off, ldw)) return TPNET_ERR_BAD_ARG;       // (the caller takes the slices)
    if (n_rows == 0) return TPNET_OK;
    return launch_score_topk(*st, src, skip, excl, excl ? n_excl : nullptr, excl ? F : 0, cand_lo, n_rows, C, K, now_time, lambda, flags,
                             mlp, wd, ldw, off, bd, wd2, bd2, H, scratch, scratch_bytes, ids, logits, info, (hipStream_t)stream);
}

size_t tpnet_workspace_bytes(int64_t max_edges, int64_t batch) { return plan_bytes(max_edges, batch); }

// bytes for a stream of max_edges on the windowed schedule in chunks of at most chunk_cap edges: one chunk's plan, or -- several
// chunks -- their plans side by side in front of one version log (the layout a replay needs, window_chunk), up to ARENA_MAX_CHUNKS
static size_t windowed_workspace_bytes(int64_t N, int d, int L, int64_t max_edges, int64_t batch, int64_t chunk_cap) {
    int K = 0;
    int64_t Ew = 0;
    tpnet_state st{};
    st.N = N; st.d = d; st.L = L;
    int64_t lim = window_chunk_limit(st, max_edges, batch, 0u, &K, &Ew);
    if (lim == 0) return 0;
    if (chunk_cap > 0 && lim > chunk_cap) lim = chunk_cap;
    const size_t one = wplan_bytes(lim, batch, N, d, L);
    int64_t c = lim / Ew * Ew;                                          // chunks of a stream that takes several: whole windows,
    if (c == 0) c = lim / (Ew / K) * (Ew / K);                          // or, under a cap below one window of K batches, whole batches
    if (lim >= max_edges || c < 4 * batch || (max_edges + c - 1) / c > ARENA_MAX_CHUNKS) return one;
    const size_t all = arena_bytes(N, d, L, max_edges, c, batch);
    // bounded (include/tpnet_hip.h: TPNET_ARENA_MAX_RATIO): the chunks' plans side by side are ~0.9 KB per edge of the WHOLE stream --
    // without a bound a 100 M-edge C2 stream asked for 108 GB, a 64-chunk one for more than the GPU has
    if (all > (size_t)TPNET_ARENA_MAX_RATIO * one) return one;
    return all > one ? all : one;
}

size_t tpnet_stream_workspace_bytes_capped(int64_t N, int32_t d, int32_t L, int64_t max_edges, int64_t batch,
                                           size_t log_cap_bytes) {
    if (max_edges < 1) max_edges = 1;
    if (batch < 1) batch = 1;
    int64_t e = 0;                                         // the most edges the caller's version log lets a chunk cover (0: no cap)
    if (log_cap_bytes > 0 && L >= 1 && d >= 1) {
        e = (int64_t)(log_cap_bytes / (2 * (size_t)L * (size_t)d * 4)) / batch * batch;
        if (e < 4 * batch) e = 4 * batch;                  // (the windowed schedule needs at least four batches per chunk)
    }
    // a plan never covers more than a chunk: ~2 M edges on the per-batch schedule, what the version log allows on the
    // windowed one; longer streams are walked chunk by chunk
    const int64_t cap_a = (2000000 / batch > 0 ? 2000000 / batch : 1) * batch;
    const int64_t ea = (e > 0 && e < max_edges) ? e : max_edges;
    const size_t a = plan_bytes(ea < cap_a ? ea : cap_a, batch);
    const size_t b = windowed_workspace_bytes(N, d, L, max_edges, batch, e);
    return a > b ? a : b;
}

size_t tpnet_stream_workspace_bytes(int64_t N, int32_t d, int32_t L, int64_t max_edges, int64_t batch) {
    return tpnet_stream_workspace_bytes_capped(N, d, L, max_edges, batch, 0);
}

int tpnet_stream_schedule(int64_t N, int32_t d, int32_t L, int64_t E, int64_t batch, uint32_t flags, size_t ws_bytes) {
    if (N < 1 || d < 1 || L < 1 || L > TPNET_MAX_LAYERS || E < 0 || batch < 1) return TPNET_ERR_BAD_ARG;
    if (E == 0) return 0;
    tpnet_state st{};
    st.N = N; st.d = d; st.L = L;
    int K = 0;
    return window_chunk(st, ws_bytes, E, batch, flags, &K) > 0 ? 1 : 0;
}

int tpnet_update(const tpnet_state* st, const int64_t* src, const int64_t* dst, const double* t, int64_t B,
                 double now_time, double lambda, uint32_t launch_id, uint32_t flags, void* workspace, size_t ws_bytes,
                 void* stream) {
    int rc = check_state(st);
    if (rc) return rc;
    if (B < 1 || !src || !dst || !t) return TPNET_ERR_BAD_ARG;  // the reference raises on an empty batch (t[-1])
    if (launch_id == 0 || launch_id >= 0x7FFFFFFFu) return TPNET_ERR_BAD_ARG;
    if (plan_bytes(B, B) > ws_bytes) return TPNET_ERR_WORKSPACE;
    if (B <= plan_one_max_batch()) {
        // one batch: the plan is ONE single-workgroup kernel (plan.hip, k_plan_one) instead of keys + device sort + finish
        Plan p{};
        rc = plan_carve(workspace, ws_bytes, B, B, &p);
        if (rc) return rc;
        hipStream_t s = (hipStream_t)stream;
        rc = plan_one(*st, p, src, dst, t, B, now_time, lambda, flags, s);
        if (rc) return rc;
        if (flags & TPNET_FLAG_EAGER_DECAY) {
            rc = launch_decay_desc(*st, p, 0, s);
            if (rc) return rc;
        }
        return launch_step(*st, StreamArgs{}, p, 0, B, (int32_t)B, lambda, launch_id, flags | ROLE_UPDATE, s);
    }
    return run_stream_impl({*st, src, dst, nullptr, t, B, B, now_time, lambda, launch_id, flags, nullptr, nullptr, workspace, ws_bytes,
                            (hipStream_t)stream, nullptr, nullptr});
}

int tpnet_run_stream_tagged(const tpnet_state* st, const int64_t* src, const int64_t* dst, const int64_t* neg,
                            const double* t, int64_t E, int64_t batch, double now_time, double lambda,
                            uint32_t launch_id_base, uint32_t flags, float* out_pos, float* out_neg, void* workspace,
                            size_t ws_bytes, double* t_end_out, void* stream, tpnet_plan_tag* tag) {
    int rc = check_state(st);
    if (rc) return rc;
    if (E < 0 || batch < 1 || (E > 0 && (!src || !dst || !t))) return TPNET_ERR_BAD_ARG;
    if (out_neg && !neg) return TPNET_ERR_BAD_ARG;
    const int64_t nb = (E + batch - 1) / batch;
    if (launch_id_base == 0 || (uint64_t)launch_id_base + (uint64_t)nb >= 0x7FFFFFFFull) return TPNET_ERR_BAD_ARG;
    rc = run_stream_impl({*st, src, dst, neg, t, E, batch, now_time, lambda, launch_id_base, flags, out_pos, out_neg, workspace,
                          ws_bytes, (hipStream_t)stream, nullptr, tag});
    if (rc) return rc;
    if (t_end_out && E > 0) {
        TPNET_HIP_TRY(hipMemcpyAsync(t_end_out, t + E - 1, sizeof(double), hipMemcpyDeviceToHost, (hipStream_t)stream));
        TPNET_HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    }
    return TPNET_OK;
}

int tpnet_run_stream(const tpnet_state* st, const int64_t* src, const int64_t* dst, const int64_t* neg,
                     const double* t, int64_t E, int64_t batch, double now_time, double lambda,
                     uint32_t launch_id_base, uint32_t flags, float* out_pos, float* out_neg, void* workspace,
                     size_t ws_bytes, double* t_end_out, void* stream) {
    return tpnet_run_stream_tagged(st, src, dst, neg, t, E, batch, now_time, lambda, launch_id_base, flags, out_pos, out_neg, workspace,
                                   ws_bytes, t_end_out, stream, nullptr);
}

// a kernel that keeps its queue busy for `ticks` of the 100 MHz wall clock, and one that does nothing
__global__ void k_warm_spin(uint64_t ticks) {
    const uint64_t t0 = wall_clock64();
    while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(32);
}
struct WarmArgs { uint64_t w[64]; };                        // 512 bytes of kernel arguments, like the step kernels'
__global__ void k_warm_noop(WarmArgs a, uint64_t* sink) { if (sink && a.w[0] == 0x1234567ull) *sink = a.w[1]; }

int tpnet_runtime_warmup(int32_t launches, int32_t spin_us, void* stream) {
    if (launches < 0 || launches > 4096 || spin_us < 0 || spin_us > 5000) return TPNET_ERR_BAD_ARG;
    hipStream_t s = (hipStream_t)stream;
    if (spin_us > 0) hipLaunchKernelGGL(k_warm_spin, dim3(1), dim3(64), 0, s, (uint64_t)spin_us * 100ull);
    WarmArgs wa{};
    for (int i = 0; i < launches; ++i) hipLaunchKernelGGL(k_warm_noop, dim3(1), dim3(64), 0, s, wa, (uint64_t*)nullptr);
    TPNET_HIP_TRY(hipGetLastError());
    return TPNET_OK;
}

int tpnet_plan_stream(const tpnet_state* st, const int64_t* src, const int64_t* dst, const double* t, int64_t E,
                      int64_t batch, double now_time, double lambda, uint32_t flags, void* workspace, size_t ws_bytes,
                      void* stream) {
    int rc = check_state(st);
    if (rc) return rc;
    if (E < 1 || batch < 1 || !src || !dst || !t) return TPNET_ERR_BAD_ARG;
    if (E >= ((int64_t)1 << 30)) return TPNET_ERR_BAD_ARG;            // 32-bit contribution indices inside one plan
    if (plan_bytes(E, batch) > ws_bytes) return TPNET_ERR_WORKSPACE;
    Plan p{};
    rc = plan_carve(workspace, ws_bytes, E, batch, &p);
    if (rc) return rc;
    return plan_build(*st, p, src, dst, t, E, batch, now_time, nullptr, lambda, flags, (hipStream_t)stream);
}

int tpnet_step_batch(const tpnet_state* st, const int64_t* src, const int64_t* dst, const int64_t* neg,
                     const double* t, int64_t E, int64_t batch, int64_t b, double lambda, uint32_t launch_id,
                     uint32_t flags, int32_t own_mod, int32_t own_rem, float* out_pos, float* out_neg,
                     void* workspace, size_t ws_bytes, void* stream) {
    int rc = check_state(st);
    if (rc) return rc;
    const int64_t nb = (E + batch - 1) / batch;
    if (E < 1 || batch < 1 || b < 0 || b >= nb || !src || !dst || !t) return TPNET_ERR_BAD_ARG;
    if (own_mod < 0 || own_rem < 0 || (own_mod > 0 && own_rem >= own_mod)) return TPNET_ERR_BAD_ARG;
    if (out_neg && !neg) return TPNET_ERR_BAD_ARG;
    if (launch_id == 0 || launch_id >= 0x7FFFFFFFu) return TPNET_ERR_BAD_ARG;
    if (flags & TPNET_FLAG_EAGER_DECAY) return TPNET_ERR_BAD_ARG;   // the sharded path carries the decay lazily
    Plan p{};
    rc = plan_carve(workspace, ws_bytes, E, batch, &p);
    if (rc) return rc;
    const StreamArgs a = stream_args_at(src, dst, neg, t, out_pos, out_neg, 0, 0, own_mod, own_rem);
    const int32_t ne = (int32_t)((E - b * batch < batch) ? (E - b * batch) : batch);
    const bool have_readout = out_pos || out_neg;
    return launch_step(*st, a, p, b, batch, ne, lambda, launch_id,
                       flags | ROLE_UPDATE | (have_readout ? ROLE_READOUT : 0u), (hipStream_t)stream);
}

int tpnet_pack_rows(const tpnet_state* st, const int64_t* ids, int64_t n, double now_time, double lambda, float* out,
                    void* stream) {
    int rc = check_state(st);
    if (rc) return rc;
    if (n < 0 || (n > 0 && (!ids || !out))) return TPNET_ERR_BAD_ARG;
    return launch_pack_rows(*st, ids, n, now_time, lambda, out, (hipStream_t)stream);
}

int tpnet_unpack_rows(const tpnet_state* st, const int64_t* ids, int64_t n, double now_time, const float* in,
                      void* stream) {
    int rc = check_state(st);
    if (rc) return rc;
    if (n < 0 || (n > 0 && (!ids || !in))) return TPNET_ERR_BAD_ARG;
    return launch_unpack_rows(*st, ids, n, now_time, in, (hipStream_t)stream);
}

int tpnet_pack_bundles(const tpnet_state* st, const int64_t* ids, int64_t n, double now_time, double lambda, float* out,
                       void* stream) {
    int rc = check_state(st);
    if (rc) return rc;
    if (n < 0 || (n > 0 && (!ids || !out))) return TPNET_ERR_BAD_ARG;
    return launch_pack_bundles(*st, ids, n, now_time, lambda, out, (hipStream_t)stream);
}

int tpnet_unpack_bundles(const tpnet_state* st, const int64_t* local_ids, int64_t n, double now_time, const float* recv,
                         int64_t maxc, const int64_t* offs, int32_t G, void* stream) {
    int rc = check_state(st);
    if (rc) return rc;
    if (n < 0 || G < 1 || maxc < 0 || (n > 0 && (!local_ids || !recv || !offs))) return TPNET_ERR_BAD_ARG;
    return launch_unpack_bundles(*st, local_ids, n, now_time, recv, maxc, offs, G, (hipStream_t)stream);
}

int tpnet_unpack_gathered(const tpnet_state* st, const int64_t* ids, int64_t n, double now_time, const float* recv,
                          int64_t maxc, const int64_t* offs, int32_t G, int32_t me, void* stream) {
    int rc = check_state(st);
    if (rc) return rc;
    if (n < 0 || G < 1 || me < 0 || me >= G || maxc < 0 || (n > 0 && (!ids || !recv || !offs))) return TPNET_ERR_BAD_ARG;
    return launch_unpack_gathered(*st, ids, n, now_time, recv, maxc, offs, G, me, (hipStream_t)stream);
}

int tpnet_gram_finish(float* x, int64_t n, void* stream) {
    if (n < 0 || (n > 0 && !x)) return TPNET_ERR_BAD_ARG;
    return tpnet::launch_gram_finish(x, n, (hipStream_t)stream);
}

int tpnet_gram_unpack(const float* packed, int64_t n, int32_t L, uint32_t flags, float* out, void* stream) {
    if (n < 0 || L < 1 || L > TPNET_MAX_LAYERS || (n > 0 && (!packed || !out))) return TPNET_ERR_BAD_ARG;
    return tpnet::launch_gram_unpack(packed, n, L, flags, out, (hipStream_t)stream);
}

int tpnet_check_errors(const tpnet_state* st, void* stream) {
    int rc = check_state(st);
    if (rc) return rc;
    uint32_t h[4] = {0, 0, 0, 0};
    TPNET_HIP_TRY(hipMemcpyAsync(h, st->err, sizeof(h), hipMemcpyDeviceToHost, (hipStream_t)stream));
    TPNET_HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    if (h[0] != 0) {
        TPNET_HIP_TRY(hipMemsetAsync(st->err, 0, sizeof(h), (hipStream_t)stream));
        return TPNET_ERR_INDEX;
    }
    return TPNET_OK;
}

int tpnet_time_stream(const tpnet_state* st, const int64_t* src, const int64_t* dst, const int64_t* neg,
                      const double* t, int64_t E, int64_t batch, double now_time, double lambda,
                      uint32_t launch_id_base, uint32_t flags, float* out_pos, float* out_neg, void* workspace,
                      size_t ws_bytes, int reps, float* total_ms_out, float* kernel_ms_out, int64_t* launches_out,
                      int64_t* edges_out, void* stream) try {
    int rc = check_state(st);
    if (rc) return rc;
    if (reps < 1 || E < 1 || batch < 1) return TPNET_ERR_BAD_ARG;
    hipStream_t s = (hipStream_t)stream;
    const int64_t nb = (E + batch - 1) / batch;
    if ((uint64_t)launch_id_base + (uint64_t)nb * (uint64_t)(reps + 1) >= 0x7FFFFFFFull) return TPNET_ERR_BAD_ARG;
    // event pairs around the step-launch loop of every chunk of the LAST rep (at most 64 chunks), then the pair around the reps
    StepTimer tm;
    tm.cap = 256;
    EventSet evs((size_t)(2 * tm.cap) + 2);
    TPNET_HIP_TRY(evs.error());
    tm.ev = evs.data();
    const hipEvent_t e0 = evs[2 * tm.cap], e1 = evs[2 * tm.cap + 1];
    uint32_t lid = launch_id_base;
    TPNET_HIP_TRY(hipEventRecord(e0, s));
    for (int r = 0; r < reps; ++r) {
        rc = run_stream_impl({*st, src, dst, neg, t, E, batch, now_time, lambda, lid, flags, out_pos, out_neg, workspace, ws_bytes, s,
                              (kernel_ms_out && r == reps - 1) ? &tm : nullptr, nullptr});
        if (rc) return rc;
        lid += (uint32_t)nb;
    }
    TPNET_HIP_TRY(hipEventRecord(e1, s));
    TPNET_HIP_TRY(hipEventSynchronize(e1));
    float ms = 0.f;
    TPNET_HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
    if (total_ms_out) *total_ms_out = ms;
    if (kernel_ms_out) {
        double sum = 0.0;
        for (int64_t i = 0; i < tm.n; ++i) {
            float k = 0.f;
            TPNET_HIP_TRY(hipEventElapsedTime(&k, evs[2 * i], evs[2 * i + 1]));
            sum += k;
        }
        *kernel_ms_out = tm.launches ? (float)(sum / (double)tm.launches) : 0.f;
    }
    if (launches_out) *launches_out = tm.launches;
    if (edges_out) *edges_out = tm.edges;
    return TPNET_OK;
} TPNET_CATCH_BAD_ALLOC

}  // extern "C"
