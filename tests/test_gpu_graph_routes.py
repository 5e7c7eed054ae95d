"""-m gpu: the deformation-graph half of the pair path — FPS, the graph build, rot6d / warp / ARAP — at every launch route up to
DVM_MAX_POINTS = 12288 points, against the oracle.

The launchers change kernel, template instance and memory form several times between the largest size the other tests run
(N = 4995) and the limit; every size below pins one of those routes (tests/graph_route_cases.py names them, and
profiles/notes_graph_routes.md lists route -> test).  Integer outputs are bit-equal to the oracle.  The FPS arg-max resolves
"largest distance, lowest index" in a thread, in a wave and across waves: tests/test_graph_routes_cpu.py proves on the CPU that
the lattice clouds used here tie at each of those levels at every size from 1025 up.  No size above the limit is ever passed
on a device (the refusal is tested without one).
"""
import numpy as np
import pytest
import torch

import graph_route_cases as C
from oracle import oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from dvm import ops as _ops
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _ops


def host(t):
    return t.detach().cpu().numpy()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---------------------------------------------------------------------------------------------------------------- FPS
# (the route each size pins: graph_route_cases.FPS_ROUTES; a cloud of one point has no second half to duplicate the first)
@pytest.mark.parametrize("kind,N", [(k, n) for k in C.FPS_KINDS for n in C.FPS_N if (k, n) != ("duplicates", 1)])
def test_fps_vs_oracle(ops, kind, N):
    """dvm_fps_f32, one launch of B = 3 with the starts 0, N // 2 and N - 1, for npoint = 1, N // 2 and N (the dataset code asks
    for the full order): every index bit-equal to the oracle's recurrence (the shorter orders are prefixes of the full one,
    which the oracle computes once), every entry the same bits when run alone, and the full order of a cloud of distinct
    points a permutation."""
    x, start = C.fps_case(kind, N)
    B = len(x)
    ref = np.stack([O.fps(x[b], N, int(start[b])) for b in range(B)])
    xd, sd = dev(x), dev(start)
    for npoint in sorted({1, max(1, N // 2), N}):
        got = host(ops.fps(xd, npoint, sd))
        assert got.shape == (B, npoint)
        for b in range(B):
            assert np.array_equal(got[b], ref[b, :npoint]), (kind, N, npoint, b, C.FPS_ROUTES[N])
    full = ops.fps(xd, N, sd)
    for b in range(B):
        assert torch.equal(ops.fps(xd[b:b + 1], N, sd[b:b + 1])[0], full[b]), (kind, N, b)
        if len(np.unique(x[b], axis=0)) == N:
            # while a point at a positive distance from every centre is left, the arg-max is one of those: no index repeats
            assert np.array_equal(np.sort(host(full[b])), np.arange(N)), (kind, N, b)
        else:
            assert kind in ("duplicates", "coincident", "mixed"), (kind, N, b)   # the other families are distinct points


# ---------------------------------------------------------------------------------------------------------------- graph build
def check_graph(g, o, b, tag):
    """tests/test_gpu_grid_search.py's check_graph: the same assertions."""
    for key in ("nodes_idx", "one_ring", "infl_idx", "dists"):
        assert np.array_equal(host(g[key])[b], o[key]), tag + (key,)
    np.testing.assert_allclose(host(g["weights"])[b], o["weights"], rtol=1e-5, atol=1e-7, equal_nan=True, err_msg=str(tag))
    np.testing.assert_allclose(host(g["sigma"])[b], o["sigma"], rtol=1e-12, equal_nan=True, err_msg=str(tag))


@pytest.mark.parametrize("N", C.DG_N)           # the route each size pins: graph_route_cases.DG_ROUTES
@pytest.mark.parametrize("kind", C.DG_KINDS)
def test_graph_build_vs_oracle(ops, kind, N):
    """dvm_dg_build_f32 around the size at which the node grid leaves LDS (3335 | 3336 nodes) and up to the limit: nodes, ring,
    influence nodes and distances bit-equal to the oracle, weights and sigma at check_graph's bars, a different FPS start per
    entry, every entry bit-equal to itself run alone."""
    x, start = C.dg_case(kind, N)
    B = len(x)
    xd, sd = dev(x), dev(start)
    g = ops.dg_build(xd, sd)
    for b in range(B):
        check_graph(g, O.dg_build(x[b], int(start[b])), b, (kind, N, b, C.DG_ROUTES[N]))
    for b in range(B):
        s = ops.dg_build(xd[b:b + 1], sd[b:b + 1])
        for key in s:
            assert torch.equal(s[key][0], g[key][b]) or (key in ("weights", "sigma") and
                                                        torch.equal(s[key][0].isnan(), g[key][b].isnan()) and
                                                        torch.equal(s[key][0].nan_to_num(), g[key][b].nan_to_num())), \
                (kind, N, b, key)


# ---------------------------------------------------------------------------------------------------------------- warp routes
# launch_dg_warp (csrc/dvm_graph.hip) runs rot6d + warp + ARAP as ONE kernel with the node tables in LDS while (N / 2) * 60 bytes
# <= 150 KB: N = 5120 (2560 nodes, 153600 B) is the last such size; from N = 5122 (2561 nodes) it launches rot6d_kernel,
# dg_warp_kernel and dg_arap_kernel.  launch_dg_warp_pair (both directions in one launch) returns false from the same size and
# pair_fwd_impl falls back to one launch_dg_warp per direction.
def pair_inputs(B, N, M, seed):
    g = torch.Generator().manual_seed(seed)
    f1 = 0.3 * torch.relu(torch.randn(B, N, 128, generator=g))
    f2 = 0.3 * torch.relu(torch.randn(B, M, 128, generator=g))
    v1 = torch.rand(B, N, 3, generator=g)
    v2 = torch.rand(B, M, 3, generator=g)
    s1 = torch.randint(0, N, (B,), generator=g).int()
    s2 = torch.randint(0, M, (B,), generator=g).int()
    return f1, f2, v1, v2, s1, s2


def check_direction(out, w, f1, f2, v1, v2, alpha, start, b):
    """tests/test_gpu_parity.py's test_pair_direction_vs_oracle: exactly its bars."""
    o = O.pair_direction(w, f1[b].numpy(), f2[b].numpy(), v1[b].numpy(), v2[b].numpy(), alpha, int(start[b]))
    assert np.array_equal(host(out["T12"])[b], o["T12"])
    np.testing.assert_allclose(host(out["verts12"])[b], o["verts12"], rtol=0, atol=5e-6)
    np.testing.assert_allclose(host(out["warped"])[b], o["warped"], rtol=0, atol=1e-4)
    L = host(out["losses"])[b]
    np.testing.assert_allclose(L, o["losses"], rtol=1e-3, atol=1e-7)
    np.testing.assert_allclose(L[[3, 4, 5]], o["losses"][[3, 4, 5]], rtol=1e-4)


@pytest.mark.parametrize("shape", [(2, 5120, 600),    # 2560 nodes: dg_warp_arap_fused_kernel at its last size
                                   (2, 5122, 600)],   # 2561 nodes: rot6d_kernel + dg_warp_kernel + dg_arap_kernel
                         ids=["fused_5120", "unfused_5122"])
def test_pair_direction_across_the_warp_switch_vs_oracle(ops, golden, shape):
    B, N, M = shape
    w = golden("deformer_scape_r_weights")
    wl = ops.deformer_weight_list(w, "cuda")
    f1, f2, v1, v2, s1, _ = pair_inputs(B, N, M, 500 + N)
    out = ops.pair_direction(wl, f1.cuda(), f2.cuda(), v1.cuda(), v2.cuda(), 40.0, s1.cuda())
    for b in range(B):
        check_direction(out, w, f1, f2, v1, v2, 40.0, s1, b)


def test_pair_forward_per_direction_warp_fallback(ops, golden):
    """ops.pair_forward at (1, 5122, 5122): launch_dg_warp_pair returns false and each direction takes the unfused launch_dg_warp.
    Every output bit-identical to the two ops.pair_direction calls; the 1 -> 2 direction also against the oracle."""
    B, N, M = 1, 5122, 5122
    w = golden("deformer_scape_r_weights")
    wl = ops.deformer_weight_list(w, "cuda")
    f1, f2, v1, v2, s1, s2 = pair_inputs(B, N, M, 911)
    d = [t.cuda() for t in (f1, f2, v1, v2)]
    r12 = ops.pair_direction(wl, d[0], d[1], d[2], d[3], 40.0, s1.cuda())
    r21 = ops.pair_direction(wl, d[1], d[0], d[3], d[2], 40.0, s2.cuda())
    o12, o21 = ops.pair_forward(wl, *d, 40.0, s1.cuda(), s2.cuda())
    for key in r12:
        assert torch.equal(o12[key], r12[key]), ("12", key)
        assert torch.equal(o21[key], r21[key]), ("21", key)
    check_direction(o12, w, f1, f2, v1, v2, 40.0, s1, 0)
