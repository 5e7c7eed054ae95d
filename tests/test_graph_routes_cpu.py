"""CPU side of tests/test_gpu_graph_routes.py: the tie coverage of its lattice clouds is a checked condition, and the
point-count limit of the graph entries is refused before anything touches a device."""
import ctypes

import numpy as np
import pytest

import graph_route_cases as C
from oracle import oracle as O


@pytest.mark.parametrize("N", C.TIE_N)
def test_lattice_clouds_plant_a_tie_at_every_level_of_the_fps_argmax(N):
    """fps_kernel resolves "largest distance, lowest index" three times: in a thread (its descending select), in a wave (the two
    DPP reductions) and across waves (`better`).  A wrong tie rule at one level shows only if the clouds of the GPU test tie
    there — with the winner, at a step whose arg-max is used.  Re-run the recurrence in numpy on exactly those clouds (the
    lattice_shuffled launch of test_fps_vs_oracle: distances are exact, ties are exact ties) and count the tied holders by
    level under the kernel's map j -> (j mod T, j div T); every level must occur at every size, and the numpy recurrence must
    be the oracle's (so the counts describe the sequence the GPU test compares against)."""
    x, start = C.fps_case("lattice_shuffled", N)
    total = dict(thread=0, wave=0, block=0)
    for b in range(len(x)):
        order, counts = C.fps_numpy(x[b], int(start[b]), C.fps_threads(N))
        assert np.array_equal(order, O.fps(x[b], N, int(start[b]))), (N, b)
        assert np.array_equal(np.sort(order), np.arange(N)), (N, b)   # distinct points: the full order is a permutation
        for k in total:
            total[k] += counts[k]
    print("N=%d T=%d tied holders beside the winner: same thread %d, same wave %d, another wave %d"
          % (N, C.fps_threads(N), total["thread"], total["wave"], total["block"]))
    assert total["thread"] > 0 and total["wave"] > 0 and total["block"] > 0, (N, total)


def _graph_entries(lib, N, M):
    """(name, call) for every entry that builds a deformation graph, with placeholder non-null pointers and no workspace."""
    one = ctypes.c_void_p(16)
    w = [one] * 10
    out = [one] * 4
    return [
        ("dvm_dg_build_f32", lambda: lib.dvm_dg_build_f32(one, 1, N, one, one, one, one, one, one, one, None, 0, None)),
        ("dvm_pair_direction_fwd_f32",
         lambda: lib.dvm_pair_direction_fwd_f32(one, one, one, one, 1, N, M, -1.0, one, *w, 1, *out, None, 0, None)),
        ("dvm_pair_fwd_f32",
         lambda: lib.dvm_pair_fwd_f32(one, one, one, one, 1, N, M, -1.0, one, one, *w, 1, *out, *out, None, 0, None)),
        ("dvm_pair_fwd_cached_f32",
         lambda: lib.dvm_pair_fwd_cached_f32(one, one, one, one, 1, N, M, -1.0, one, one, *w, 1, *out, *out, None, 0, 0, None)),
        ("dvm_pair_geometry_f32", lambda: lib.dvm_pair_geometry_f32(one, one, 1, N, M, one, one, 1, None, 0, None)),
    ]


def test_point_count_limit_is_refused_without_gpu():
    """A cloud of more than 12288 points cannot have its graph built (fps_kernel holds the cloud in LDS).  Every entry that builds
    one refuses it as an argument error, before the workspace is carved and before any launch — nodes_idx would otherwise stay
    whatever the workspace held, and every later kernel gathers through it unchecked.  The limit itself passes the size check
    and stops at the workspace check.  (Placeholder pointers: these calls must never reach a device.)"""
    from dvm import _lib
    lib = _lib.load()
    LIMIT = 12288
    one = ctypes.c_void_p(16)
    rc = lib.dvm_fps_f32(one, 1, LIMIT + 1, 1, one, one, None)
    assert rc == -1 and b"12288" in lib.dvm_last_error() and b"12289" in lib.dvm_last_error()
    for name, call in _graph_entries(lib, LIMIT + 1, 600):
        rc = call()
        err = lib.dvm_last_error()
        assert rc == -1 and b"12288" in err and b"12289" in err and name.encode()[:12] in err, (name, rc, err)
    for name, call in _graph_entries(lib, 600, LIMIT + 1)[2:]:   # the two-direction entries and the geometry call: M as well
        rc = call()
        err = lib.dvm_last_error()
        assert rc == -1 and b"12288" in err and b"12289" in err, (name, rc, err)
    # dvm_pair_direction_fwd_f32 builds the graph of the N cloud only: M is not held to the limit
    rc = _graph_entries(lib, 600, LIMIT + 1)[1][1]()
    assert rc == -3 and b"too small" in lib.dvm_last_error()
    for N, M in ((LIMIT, LIMIT), (LIMIT, 600)):
        for name, call in _graph_entries(lib, N, M):
            rc = call()
            assert rc == -3 and b"too small" in lib.dvm_last_error(), (name, N, M, rc, lib.dvm_last_error())
