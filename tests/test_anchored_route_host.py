"""CPU tests of the anchored readout's route query (tpnet_anchored_route, csrc/encoder.hip: anchored_route): the table of
include/tpnet_hip.h stated once more here, independently, and compared with the library over a grid of states and flag words; the
five older queries against their documented rules on the same grid.  No kernel runs: the states are fakes and mlp is NULL, so no
HIP call is made.  What the route launches is tests/test_anchored_route.py (-m gpu)."""
import ctypes
import itertools
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOT_SCALE, PACKED, NO_MFMA, ROWS8, LAYERS = 1, 8, 256, 512, 1024
REFUSED, GENERIC, WALK, MFMA, LAYERS_MFMA = 0, 1, 2, 3, 4
DS, LS, KS, NS = range(1, 521), (1, 2, 3, 4), (1, 3, 4, 5, 20), (1, 7)
FLAG_WORDS = [sum(c) for r in range(6) for c in itertools.combinations((NOT_SCALE, PACKED, NO_MFMA, ROWS8, LAYERS), r)]


def _state(**kw):
    from tpnet_amd import _lib
    return _lib.State(**{**dict(p0=64, q=64, meta=64, N=10, d=64, L=3, err=64), **kw})


# ---- the table, from its words (include/tpnet_hip.h) -----------------------------------------------------------------------
def _steps_2_to_5(d):
    return 36 <= d <= 160


def _walk_rows(d):
    return d % 4 == 0 and 36 <= d <= 512


def _layers_rule(d, L, K):
    return L in (1, 2, 4) and d % 4 == 0 and _steps_2_to_5(d) and K >= 4


def _rows8_rule(d, L, K):
    return L == 3 and d % 4 == 2 and 38 <= d <= 158 and K >= 4


def _want_route(d, L, K, flags):
    """mlp NULL, aligned outputs, no pair lists: the Gram kernel alone (bits 4-5 are 0 without an mlp)."""
    if flags & PACKED:
        return REFUSED
    if flags & ROWS8 and d % 4 == 2:
        return MFMA if _rows8_rule(d, L, K) and not flags & NO_MFMA else REFUSED
    if not _walk_rows(d):
        return REFUSED
    if not flags & NO_MFMA:
        if L == 3 and _steps_2_to_5(d) and K >= 4:
            return MFMA
        if flags & LAYERS and _layers_rule(d, L, K):
            return LAYERS_MFMA
    return WALK


def test_route_equals_the_table_on_the_grid(hip_lib):
    """Every d in 1..520, L in 1..4, K in {1, 3, 4, 5, 20}, n_rows in {1, 7} and every subset of the five flags that the route
    reads (or must ignore: NOT_SCALE)."""
    route, seen, bad = hip_lib.tpnet_anchored_route, set(), []
    for d in DS:
        for L in LS:
            st = ctypes.byref(_state(d=d, L=L))
            for K in KS:
                want = [_want_route(d, L, K, f) for f in FLAG_WORDS]
                seen.update(want)
                for n in NS:
                    got = [route(st, n, K, f, None) for f in FLAG_WORDS]
                    if got != want:
                        bad.append((d, L, K, n, [(f, g, w) for f, g, w in zip(FLAG_WORDS, got, want) if g != w][:3]))
    assert not bad, f"{len(bad)} shapes off, first {bad[:3]}"
    assert seen == {REFUSED, WALK, MFMA, LAYERS_MFMA}                     # (GENERIC needs the encoder's pair lists: not this query)


def test_kept_queries_keep_their_rules_on_the_grid(hip_lib):
    """tpnet_pair_gram_anchored_supported, tpnet_encoder_fused_supported, tpnet_encoder_rows8_supported, tpnet_encoder_layers_supported
    and tpnet_encoder_wide_supported as include/tpnet_hip.h documents them (the one-launch queries answer 0 without an mlp)."""
    lib, bad = hip_lib, []
    for d in DS:
        for L in LS:
            st = ctypes.byref(_state(d=d, L=L))
            for K in KS:
                want = (int(_walk_rows(d)), 0, int(_rows8_rule(d, L, K)), int(_layers_rule(d, L, K)), 0)
                for n in NS:
                    got = (lib.tpnet_pair_gram_anchored_supported(st), lib.tpnet_encoder_fused_supported(st, n, K, None),
                           lib.tpnet_encoder_rows8_supported(st, n, K, None), lib.tpnet_encoder_layers_supported(st, n, K),
                           lib.tpnet_encoder_wide_supported(st, n, K, None))
                    if got != want:
                        bad.append((d, L, K, n, got, want))
    assert not bad, f"{len(bad)} shapes off, first {bad[:3]}"


def test_symbol_declared_exported_and_bound(hip_lib):
    from tpnet_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tpnet_hip.h")).read(), flags=re.S)
    assert "tpnet_anchored_route" in re.findall(r"\b(tpnet_[a-z_0-9]+)\s*\(", text)
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "tpnet_anchored_route")
    assert "tpnet_anchored_route" in _lib.SIGNATURES and hip_lib.tpnet_anchored_route.restype is ctypes.c_int
    assert hip_lib.tpnet_abi_version() == 7


@pytest.mark.parametrize("broken", [dict(p0=None), dict(q=None), dict(meta=None), dict(err=None), dict(N=0), dict(N=1 << 31), dict(d=0),
                                    dict(L=0), dict(L=5)])
def test_null_or_inconsistent_state_is_refused(hip_lib, broken):
    assert hip_lib.tpnet_anchored_route(None, 7, 20, 0, None) == 0
    assert hip_lib.tpnet_anchored_route(ctypes.byref(_state()), 7, 20, 0, None) == MFMA
    assert hip_lib.tpnet_anchored_route(ctypes.byref(_state(**broken)), 7, 20, 0, None) == 0
