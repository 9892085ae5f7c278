"""The host code that sequences a stream call (csrc/api.hip: which schedule, which planner, how the workspace is cut) answers
exactly what it answered before it was single-sourced.  CPU tests: the four sizing / scheduling queries of the C ABI need no
device, and their answers over the grid below are compared, with no tolerance, against a table recorded from the library as it
was before the refactor (tests/golden/stream_sequencing.npz, written by tests/golden/make_stream_sequencing.py).  What these
queries do not show of window_chunk -- the chunk and region sizes it picks -- is observed on the GPU through
tpnet_plan_tag::replayed (tests/test_stream_reuse.py, the multi-chunk replays)."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SCHED_WINDOWED, SCHED_BATCH, PLAN_SORTED, PLAN_HASHED, PACKED, SEQUENTIAL = 16, 32, 64, 128, 8, 4
FLAGS = (0, SCHED_WINDOWED, SCHED_BATCH, PLAN_SORTED, PLAN_HASHED, PACKED, SEQUENTIAL)
BATCHES = (1, 200, 1000, 2048, 2049, 8192, 80000)
NB = (1, 4, 15, 16, 20, 55, 56, 158, 480, 2000, 20000)        # stream lengths in batches ...
E_MAX = 200_000_000                                           # ... and the longest stream, in edges
HEADLINE = (9228, 128, 3)
C4 = (10_000_000, 256, 3)
# every other value the sequencing code branches on, one at a time around the headline shape
OTHER_SHAPES = [(300, 128, 3), (524288, 128, 3), (10_000_000, 128, 3)] + [(9228, d, 3) for d in (64, 140, 172, 512)] + \
               [(9228, 128, L) for L in (1, 2)] + [(300, 64, 1), (524288, 172, 2), (524288, 512, 3)]
F_WORKSPACE, F_CAPPED, F_SCHEDULE, F_WSHARD = 0, 1, 2, 3
COLUMNS = ("func", "N", "d", "L", "E", "batch", "flags", "ws_bytes", "G", "n_owned")


def edge_counts(batch, full):
    """One batch ... 200 M edges; every other length also with a ragged last batch."""
    out = []
    for i, nb in enumerate(NB if full else (1, 15, 16, 20, 56, 158, 2000)):
        e = nb * batch - (batch // 3 if i % 2 else 0)
        if 0 < e <= E_MAX:
            out.append(e)
    return out + [E_MAX]


def log_caps(d, L, batch):
    """Version-log caps (bytes): fewer batches than one window of the pipeline holds, a few windows, more than most streams."""
    row = 2 * L * d * 4
    return [5 * batch * row, 30 * batch * row, 500 * batch * row]


def grid(sizes):
    """The rows of the table: (func, N, d, L, E, batch, flags, ws_bytes, G, n_owned).  `sizes(N, d, L, E, batch)` answers
    tpnet_stream_workspace_bytes and `sizes(N, d, L, E, batch, cap)` the capped query: the workspaces offered to
    tpnet_stream_schedule are fractions of what the library itself asks for."""
    rows = []
    for shape in [HEADLINE, C4] + OTHER_SHAPES:
        N, d, L = shape
        full = shape in (HEADLINE, C4)                         # batch x E x flags x workspace crossed completely
        for batch in BATCHES if full else (200, 1000, 2049):
            for E in edge_counts(batch, full):
                rows.append((F_WORKSPACE, N, d, L, E, batch, 0, 0, 0, 0))
                want = sizes(N, d, L, E, batch)
                offered = [want, want // 2, want // 10]
                for cap in log_caps(d, L, batch):
                    rows.append((F_CAPPED, N, d, L, E, batch, 0, cap, 0, 0))
                offered.append(sizes(N, d, L, E, batch, log_caps(d, L, batch)[0]))     # a log of less than one window
                if full:
                    offered.append(sizes(N, d, L, E, batch, log_caps(d, L, batch)[1]))
                for flags in FLAGS if full else (0, SCHED_WINDOWED, PLAN_SORTED):
                    for ws in offered:
                        rows.append((F_SCHEDULE, N, d, L, E, batch, flags, ws, 0, 0))
            # a row shard of G ranks: n_owned rows of its own and as many halo rows again
            for G in (1, 2, 8):
                n_owned = (N + G - 1) // G
                n_local = min(N + 1, 2 * n_owned)
                for nb in (4, 16, 158):
                    rows.append((F_WSHARD, n_local, d, L, nb * batch, batch, 0, 0, G, n_owned))
    return np.asarray(rows, dtype=np.int64)


def answers(lib, rows=None):
    """(rows, answers): the library's answer to every row of the grid, as uint64."""
    def sizes(N, d, L, E, batch, cap=None):
        if cap is None:
            return int(lib.tpnet_stream_workspace_bytes(N, d, L, E, batch))
        return int(lib.tpnet_stream_workspace_bytes_capped(N, d, L, E, batch, cap))
    if rows is None:
        rows = grid(sizes)
    out = np.zeros(len(rows), dtype=np.uint64)
    for i, (func, N, d, L, E, batch, flags, ws, G, n_owned) in enumerate(rows.tolist()):
        if func == F_WORKSPACE:
            out[i] = sizes(N, d, L, E, batch)
        elif func == F_CAPPED:
            out[i] = sizes(N, d, L, E, batch, ws)
        elif func == F_SCHEDULE:
            out[i] = lib.tpnet_stream_schedule(N, d, L, E, batch, flags, ws)
        else:
            out[i] = lib.tpnet_wshard_workspace_bytes(N, d, L, E, batch, G, n_owned)
    return rows, out


def test_sizes_and_schedules_are_what_they_were(hip_lib, golden_dir):
    """tpnet_stream_workspace_bytes, _capped, tpnet_stream_schedule and tpnet_wshard_workspace_bytes over the grid: equal to the
    recorded answers, row for row."""
    g = np.load(os.path.join(golden_dir, "stream_sequencing.npz"))
    assert tuple(g["columns"].tolist()) == COLUMNS
    rows, got = answers(hip_lib)
    # the grid is built from the library's own sizes: a size that moved shows up here first
    assert rows.shape == g["rows"].shape and np.array_equal(rows, g["rows"])
    for func, name in ((F_WORKSPACE, "tpnet_stream_workspace_bytes"), (F_CAPPED, "tpnet_stream_workspace_bytes_capped"),
                       (F_SCHEDULE, "tpnet_stream_schedule"), (F_WSHARD, "tpnet_wshard_workspace_bytes")):
        m = rows[:, 0] == func
        assert m.sum() > 100, name
        bad = np.flatnonzero(m & (got != g["answers"]))
        assert bad.size == 0, f"{name}: {bad.size} rows differ, first {rows[bad[0]].tolist()}: {got[bad[0]]} != {g['answers'][bad[0]]}"
    sched = g["answers"][rows[:, 0] == F_SCHEDULE]
    assert 0 < int(sched.sum()) < sched.size                   # both schedules occur


def test_grid_covers_what_the_sequencing_code_branches_on(golden_dir):
    rows = np.load(os.path.join(golden_dir, "stream_sequencing.npz"))["rows"]
    col = {c: rows[:, i] for i, c in enumerate(COLUMNS)}
    stream = col["func"] != F_WSHARD
    assert {300, 9228, 524288, 10_000_000} <= set(col["N"][stream].tolist())
    assert {64, 128, 140, 172, 512} <= set(col["d"].tolist())
    assert {1, 2, 3} <= set(col["L"].tolist())
    assert set(BATCHES) <= set(col["batch"].tolist())
    assert set(FLAGS) <= set(col["flags"][col["func"] == F_SCHEDULE].tolist())
    assert col["E"].max() == E_MAX
    for shape in (HEADLINE, C4):
        m = (col["func"] == F_SCHEDULE) & (col["N"] == shape[0]) & (col["d"] == shape[1]) & (col["L"] == shape[2])
        for batch in BATCHES:
            nbs = set((-(-col["E"][m & (col["batch"] == batch)] // batch)).tolist())
            assert {15, 16, 20, 55, 56, 158} <= nbs, (shape, batch)
            for flags in FLAGS:
                assert (m & (col["batch"] == batch) & (col["flags"] == flags)).sum() >= 5 * 2


EVENT_SET_PROGRAM = r"""
#include "event_set.hpp"
#include <cstdio>
static int created = 0, destroyed = 0, fail_at = -1;
extern "C" hipError_t hipEventCreate(hipEvent_t* e) {
    if (created == fail_at) return hipErrorOutOfMemory;
    *e = reinterpret_cast<hipEvent_t>(static_cast<size_t>(++created));
    return hipSuccess;
}
extern "C" hipError_t hipEventDestroy(hipEvent_t e) { if (!e) return hipErrorInvalidHandle; ++destroyed; return hipSuccess; }
int main() {
    { tpnet::EventSet ev(514); if (ev.error() != hipSuccess || !ev[513]) return 1; }
    if (created != 514 || destroyed != 514) return 2;
    created = destroyed = 0; fail_at = 100;
    { tpnet::EventSet ev(514); if (ev.error() != hipErrorOutOfMemory) return 3; }
    if (created != 100 || destroyed != 100) return 4;
    { tpnet::EventSet none(0); if (none.error() != hipSuccess) return 5; }
    std::puts("ok");
    return 0;
}
"""


def test_event_set_frees_what_it_created(tmp_path):
    """csrc/event_set.hpp on its own, against counting stand-ins for hipEventCreate / hipEventDestroy: every event created is
    destroyed when the set leaves scope, also when a create fails half way (which the set reports)."""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    if not os.path.exists(os.path.join(rocm, "include", "hip", "hip_runtime_api.h")):
        pytest.fail("the HIP headers are needed to build the event set")
    src = tmp_path / "event_set_test.cpp"
    src.write_text(EVENT_SET_PROGRAM)
    exe = tmp_path / "event_set_test"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(rocm, "include"),
                    "-I", os.path.join(ROOT, "tpnet_amd", "csrc"), str(src), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout, r.stderr)



@pytest.mark.gpu
def test_time_stream_frees_its_events_on_every_way_out(hip_lib):
    """tpnet_time_stream refused for a workspace that is too small -- on the host, inside the repetitions, with its 514 events
    alive -- some tens of times in one process, then a normal timed call: it succeeds and computes what tpnet_run_stream
    computes on a twin state, bit for bit."""
    import ctypes as C
    import torch
    from tpnet_amd import _lib
    from test_gpu_parity import DEV, _need_gpu, _random_stream
    _need_gpu()
    N, d, L, B, nb, lam, t0 = 300, 64, 3, 40, 20, 1e-6, 1.0e6
    E, row = B * nb, (2 * L + 2) ** 2
    src, dst, neg, t = (torch.from_numpy(x).to(DEV) for x in _random_stream(np.random.RandomState(5), N, E, 4.0e5))
    P0 = torch.randn(N, d, device=DEV)
    stream = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    ws = torch.empty(hip_lib.tpnet_stream_workspace_bytes(N, d, L, E, B), dtype=torch.uint8, device=DEV)

    def table():
        keep = dict(p0=P0.clone(), q=torch.zeros(2, N, L, d, device=DEV), meta=torch.zeros(N * 32, dtype=torch.uint8, device=DEV),
                    err=torch.zeros(4, dtype=torch.int32, device=DEV), pos=torch.zeros(E, row, device=DEV),
                    neg=torch.zeros(E, row, device=DEV))
        st = _lib.State(p0=keep["p0"].data_ptr(), q=keep["q"].data_ptr(), meta=keep["meta"].data_ptr(), N=N, d=d, L=L,
                        err=keep["err"].data_ptr())
        _lib.check(hip_lib.tpnet_state_init(C.byref(st), t0, stream), "state_init")
        return st, keep

    def timed(st, keep, ws_bytes):
        total, kern, launches, edges = C.c_float(0), C.c_float(0), C.c_int64(0), C.c_int64(0)
        rc = hip_lib.tpnet_time_stream(C.byref(st), src.data_ptr(), dst.data_ptr(), neg.data_ptr(), t.data_ptr(), E, B, t0, lam, 1, 0,
                                       keep["pos"].data_ptr(), keep["neg"].data_ptr(), ws.data_ptr(), ws_bytes, 1, C.byref(total),
                                       C.byref(kern), C.byref(launches), C.byref(edges), stream)
        return rc, total.value, launches.value, edges.value

    st, keep = table()
    for _ in range(40):
        assert timed(st, keep, 256)[0] == -2                                # TPNET_ERR_WORKSPACE: nothing was launched
    rc, total_ms, launches, edges = timed(st, keep, ws.numel())
    assert rc == 0 and total_ms > 0 and 0 < launches <= nb and edges == E
    st2, twin = table()
    _lib.check(hip_lib.tpnet_run_stream(C.byref(st2), src.data_ptr(), dst.data_ptr(), neg.data_ptr(), t.data_ptr(), E, B, t0, lam, 1, 0,
                                        twin["pos"].data_ptr(), twin["neg"].data_ptr(), ws.data_ptr(), ws.numel(), None, stream),
               "run_stream")
    _lib.check(hip_lib.tpnet_check_errors(C.byref(st), stream), "check_errors")
    torch.cuda.synchronize()
    for k in ("pos", "neg", "q", "meta"):
        assert torch.equal(keep[k], twin[k]), k
