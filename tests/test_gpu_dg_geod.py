"""-m gpu: skinning and node rings by a caller-supplied distance matrix (dvm_dg_skin_geod_f32, dvm_dg_skin_weights_f32,
dvm_dg_build_geod_f32; ops.dg_skin_geod / dg_skin_weights / dg_build_geod) against the numpy statement of the rule
(tests/dg_geod_ref.py, pinned to the reference's fixtures by tests/test_dg_geod_ref_cpu.py).

Indices and distances are compared with array_equal; weights against the float64 formula at atol = 3e-7, the bar
tests/test_gpu_parity.py sets for these weights.  Sizes are named from the kernel's own constants (ops.dg_skin_geod_plan:
vertices per workgroup, waves that share a tile's node range, length of the per-lane list)."""
import ctypes

import numpy as np
import pytest
import torch

import dg_geod_ref as R

pytestmark = pytest.mark.gpu

W_ATOL = 3e-7
EINVAL, ENOSPACE = -1, -3
MESH = ("meshgraph_a", "meshgraph_b", "meshgraph_c")
DG = ("dg_rand_256", "dg_rand_2048", "dg_scape_512", "dg_scape_1024")


@pytest.fixture(scope="module")
def ops():
    from dvm import ops as _ops
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _ops


def host(t):
    return t.detach().cpu().numpy()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def check_skin(ops, dist, nodes, ring_k=0, slices=None, sigma=None):
    """dist (B,N,N), nodes (B,Nn) numpy -> the device result, compared with the statement."""
    infl, dists, ring = ops.dg_skin_geod(dev(dist), dev(nodes.astype(np.int32)), ring_k, slices=slices)
    ri, rd, rr = R.skin_batch(dist, nodes, ring_k)
    tag = "N=%d Nn=%d ring_k=%d slices=%s" % (dist.shape[1], nodes.shape[1], ring_k, slices)
    assert np.array_equal(host(infl), ri), tag
    assert np.array_equal(host(dists), rd, equal_nan=True), tag
    if ring_k:
        assert np.array_equal(host(ring), rr), tag
    else:
        assert ring is None
    if sigma is not None:
        w = host(ops.dg_skin_weights(dists, torch.as_tensor(sigma, dtype=torch.float64)))
        assert not np.isnan(w).any(), tag
        np.testing.assert_allclose(w, R.weights(rd, sigma), rtol=0, atol=W_ATOL, err_msg=tag)
        return host(infl), host(dists), w
    return host(infl), host(dists), None


def rand_case(seed, B, N, Nn, symmetric=False):
    g = np.random.default_rng(seed)
    d = g.random((B, N, N), dtype=np.float32)
    if symmetric:
        d = (d + d.transpose(0, 2, 1)) * np.float32(0.5)
    nodes = np.stack([g.permutation(N)[:Nn] for _ in range(B)])
    return d, nodes


# ------------------------------------------------------------------------------------------------------ reference fixtures
@pytest.mark.parametrize("name", MESH)
def test_mesh_fixtures(ops, golden, name):
    """The reference's construct_graph on real edge geodesics: Nn != N/2, V = 333 and 120 are not multiples of the vertex tile."""
    g = golden(name)
    infl, dists, ring = ops.dg_skin_geod(dev(g["geod"])[None], dev(g["nodes_idx"])[None])
    assert ring is None
    assert np.array_equal(host(infl)[0], g["infl_idx"])
    assert np.array_equal(host(dists)[0], g["dists"])
    w = host(ops.dg_skin_weights(dists, torch.tensor([float(g["sigma"])], dtype=torch.float64)))[0]
    np.testing.assert_allclose(w, R.weights(g["dists"], float(g["sigma"])), rtol=0, atol=W_ATOL)
    np.testing.assert_allclose(w, g["weights"], rtol=0, atol=W_ATOL)


@pytest.mark.parametrize("ring_metric", ["euclidean", "geodesic"])
@pytest.mark.parametrize("name", DG)
def test_point_cloud_fixtures(ops, golden, name, ring_metric):
    """The reference's construct_graph_euclidean, fed torch.cdist computed on the CPU as the fixtures' generator did."""
    g = golden(name)
    v = torch.from_numpy(g["verts"])
    cd = torch.cdist(v, v, p=2.0)
    start = torch.tensor([int(g["fps_start"])], dtype=torch.int32).cuda()
    b = ops.dg_build_geod(v.cuda()[None], cd.cuda()[None], start, ring_metric)
    plain = ops.dg_build(v.cuda()[None], start)
    for key in ("nodes_idx", "one_ring", "infl_idx"):
        assert np.array_equal(host(b[key])[0], g[key]), key
    # dists are the entries of the matrix that was passed, bit for bit: the fixture's own bits on a host whose matrix product
    # sums as the generator's did (printed), within the matmul form's rounding on every host (dg_geod_ref.CDIST_D2_TOL)
    dists = host(b["dists"])[0]
    assert np.array_equal(dists, cd.numpy()[g["nodes_idx"].astype(np.int64)[g["infl_idx"]], np.arange(len(v))[:, None]])
    print("%s: this host's cdist gives the fixture's dists bit for bit: %s" % (name, np.array_equal(dists, g["dists"])))
    assert R.same_up_to_cdist_rounding(dists, g["dists"])
    assert host(b["sigma"]).tobytes() == host(plain["sigma"]).tobytes()
    np.testing.assert_allclose(host(b["weights"])[0], R.weights(dists, host(b["sigma"])[0]), rtol=0, atol=W_ATOL)
    np.testing.assert_allclose(host(b["weights"])[0], g["weights"], rtol=0, atol=W_ATOL)


@pytest.mark.parametrize("name", MESH)
def test_construct_graph_with_device_geod(golden, name):
    """Mesh mode with `geod` a CUDA tensor: the top-k and the weights on the device, sigma the mesh-mode one."""
    from lib.deformation_graph_point import DeformationGraph_geod
    g = golden(name)
    dg = DeformationGraph_geod()
    dg.construct_graph(torch.from_numpy(g["verts"]).float(), g["faces"], torch.from_numpy(g["geod"]).cuda())
    assert np.array_equal(np.asarray(dg.nodes_idx), g["nodes_idx"])
    assert np.array_equal(host(dg.influence_nodes_idx), g["infl_idx"])
    assert np.array_equal(host(dg._g["infl_idx"])[0], g["infl_idx"])
    assert np.array_equal(host(dg._g["dists"])[0], g["dists"])
    np.testing.assert_allclose(float(dg.sigma), float(g["sigma"]), rtol=1e-12)
    np.testing.assert_allclose(host(dg.weights), g["weights"], rtol=0, atol=W_ATOL)
    assert np.array_equal(host(dg._g["one_ring"])[0], g["one_ring"])


# ------------------------------------------------------------------------------------------------------------ orientation
def test_orientation_of_a_non_symmetric_matrix(ops):
    d, nodes = rand_case(1, 1, 120, 60)
    infl, _, _ = check_skin(ops, d, nodes, ring_k=9, sigma=[0.3])
    ti, _, _ = R.skin_batch(d.transpose(0, 2, 1), nodes)
    assert (infl != ti).any(axis=-1).mean() > 0.5    # node rows read along v, not node columns


def test_batch_strides(ops):
    d, nodes = rand_case(2, 3, 120, 47)
    infl, _, _ = check_skin(ops, d, nodes, ring_k=9, sigma=[0.2, 0.3, 0.4])
    assert not np.array_equal(infl[0], infl[1]) and not np.array_equal(infl[1], infl[2])


# -------------------------------------------------------------------------------------------------------------------- ties
@pytest.mark.parametrize("ring_k,slices", [(9, None), (16, 1), (16, 8)])
def test_ties_go_to_the_lower_node_position(ops, ring_k, slices):
    g = np.random.default_rng(3)
    d = g.integers(0, 4, (1, 256, 256)).astype(np.float32)
    nodes = g.permutation(256)[:128][None]
    o = R.order(d[0], nodes[0])[:10]
    dv = d[0][nodes[0][o], np.arange(256)[None, :]]
    assert ((dv[1:] == dv[:-1]).sum(0) >= 5).mean() > 0.9     # most rows: many equal entries among their first ten
    check_skin(ops, d, nodes, ring_k=ring_k, slices=slices, sigma=[2.0])


def test_duplicate_nodes_at_distance_zero(ops):
    """A node list that names vertices twice: both positions are at distance 0 of that vertex (the lower one first), and both get
    the vertex's ring row."""
    d, _ = rand_case(4, 2, 130, 10, symmetric=True)
    for b in range(2):
        np.fill_diagonal(d[b], 0.0)
    g = np.random.default_rng(5)
    base = np.stack([g.permutation(130)[:40] for _ in range(2)])
    nodes = np.concatenate([base, base[:, :25][:, ::-1]], axis=1)    # 65 positions, 25 vertices twice
    infl, dists, _ = check_skin(ops, d, nodes, ring_k=9, sigma=[0.3, 0.3])
    for b in range(2):
        v = base[b, 3]
        assert dists[b, v, 0] == 0 and dists[b, v, 1] == 0 and infl[b, v, 0] == 3 and infl[b, v, 1] == 40 + 21


# -------------------------------------------------------------------------------------------------------------- non-finite
def test_non_finite_entries(ops):
    d, nodes = rand_case(6, 2, 100, 50)
    d = d + np.float32(0.5)
    rows0 = nodes[0]
    d[0, rows0[:, None], np.array([5, 6])[None, :]] = np.inf           # vertices 5, 6 of shape 0: every node at +inf ...
    d[0, rows0[7], 6] = 0.25                                            # ... but one for vertex 6
    d[0, rows0[::2], 9] = np.nan                                        # vertex 9: every other node NaN
    d[0, rows0, 11] = np.nan                                            # vertex 11: nothing but NaN
    d[0, rows0[3:], 12] = np.inf                                        # vertex 12: three finite nodes exactly
    d[0, rows0[2:], 13] = np.nan                                        # vertex 13: two finite nodes
    d[0, rows0[10], 14] = -0.0                                          # vertex 14: -0 and +0, the lower position first
    d[0, rows0[4], 14] = 0.0
    d[1, nodes[1][1::3], 20] = -np.inf                                  # -inf sorts in front of everything
    d[1, nodes[1][5], 21] = -1.5
    infl, dists, w = check_skin(ops, d, nodes, ring_k=9, sigma=[0.4, 0.4])
    assert w[0, 5].tolist() == [1.0, 0.0, 0.0] and infl[0, 5].tolist() == [0, 1, 2]
    assert w[0, 6].tolist() == [1.0, 0.0, 0.0] and infl[0, 6].tolist() == [7, 0, 1]
    assert w[0, 11].tolist() == [1.0, 0.0, 0.0] and infl[0, 11].tolist() == [0, 1, 2] and np.isnan(dists[0, 11]).all()
    assert np.isfinite(dists[0, 12]).all() and (w[0, 12] > 0).all()
    assert np.isfinite(dists[0, 13][:2]).all() and np.isnan(dists[0, 13][2]) and w[0, 13, 2] == 0
    assert infl[0, 14][:2].tolist() == [4, 10]
    assert np.signbit(dists[0, 14, 1]) and not np.signbit(dists[0, 14, 0])     # copied unchanged
    assert w[1, 20].tolist() == [1.0, 0.0, 0.0] and np.isneginf(dists[1, 20]).all()
    assert infl[1, 21, 0] == 5
    # the ring kernels share the lists: a second pass with longer lists and every split
    for s in (1, 2, 4, 8):
        check_skin(ops, d, nodes, ring_k=16, slices=s)


def test_weights_rule_alone(ops):
    d = np.array([[[0.0, np.inf, np.nan], [np.inf, np.inf, np.inf], [1.0, 1.0, 1.0], [0.0, 0.0, 0.0], [0.5, 1.5, -2.0]]], np.float32)
    for sg in (1.0, 0.0, float("nan"), float("inf")):
        w = host(ops.dg_skin_weights(dev(d), torch.tensor([sg], dtype=torch.float64)))
        assert not np.isnan(w).any()
        np.testing.assert_allclose(w, R.weights(d, [sg]), rtol=0, atol=W_ATOL)
        assert w[0, 1].tolist() == [1.0, 0.0, 0.0]
    far = np.array([[[30.0, 40.0, 50.0], [1e30, 2e30, 3e30]]], np.float32)     # every exp underflows to 0 (d * d overflows fp32 in the second)
    w = host(ops.dg_skin_weights(dev(far), torch.tensor([1.0], dtype=torch.float64)))
    assert w[0, 0].tolist() == [1.0, 0.0, 0.0] and w[0, 1].tolist() == [1.0, 0.0, 0.0]


# ------------------------------------------------------------------------------------ shapes where the kernel can go wrong
def test_plan_names_the_launch_shapes(ops):
    """The constants the sizes below are taken from."""
    tile, s, ln = ops.dg_skin_geod_plan(1, 64, 31)
    assert (tile, s, ln) == (64, 1, 3)
    # node slices: doubled while every wave keeps 16 node rows (32, 64, 128 nodes) and fewer than 4096 waves are in flight
    assert [ops.dg_skin_geod_plan(1, 256, n)[1] for n in (31, 32, 63, 64, 127, 128, 256)] == [1, 2, 2, 4, 4, 8, 8]
    assert [ops.dg_skin_geod_plan(b, 4096, 2048)[1] for b in (1, 15, 16, 31, 32, 63, 64)] == [8, 8, 4, 4, 2, 2, 1]   # 64 b tiles
    assert [ops.dg_skin_geod_plan(1, 256, 128, k)[2] for k in (0, 3, 4, 9, 10, 16)] == [3, 3, 9, 9, 16, 16]


@pytest.mark.parametrize("N", [64, 65, 127, 333, 1025])
def test_sizes_around_the_vertex_tile(ops, N):
    """One vertex tile exactly, one lane into the next, one short of two, and sizes that are no multiple of anything; every
    Nn of {3, 9, N/2, N} with every list length."""
    for Nn in (3, 9, N // 2, N):
        d, nodes = rand_case(100 + N + Nn, 2, N, Nn)
        for ring_k in (0, 9, 16):
            if ring_k <= Nn:
                check_skin(ops, d, nodes, ring_k=ring_k, sigma=[0.3, 0.2])


@pytest.mark.parametrize("slices", [1, 2, 4, 8])
def test_node_slice_boundaries(ops, slices):
    """Every wave count, with node counts on each side of a whole number of rows per wave (Nn = 16 slices and its neighbours), fewer
    nodes than waves (some waves walk nothing), and every list length (the merge is per list length)."""
    for Nn in sorted({3, slices - 1, slices, slices + 1, 16 * slices - 1, 16 * slices, 16 * slices + 1, 4 * slices + 3} - {0, 1, 2}):
        d, nodes = rand_case(200 + Nn, 1, 130, Nn)
        for ring_k in (0, 9, 16):
            if ring_k <= Nn:
                check_skin(ops, d, nodes, ring_k=ring_k, slices=slices)


@pytest.mark.parametrize("Nn", [31, 32, 63, 64, 127, 128])
def test_slice_choice_thresholds(ops, Nn):
    """The plain call on each side of the node counts at which it doubles the waves per tile."""
    d, nodes = rand_case(300 + Nn, 1, 200, Nn)
    check_skin(ops, d, nodes, ring_k=9, sigma=[0.3])


def test_split_and_merge_at_4096(ops):
    """B = 1, N = 4096: 64 vertex tiles, the node range of each split over 8 waves and merged in LDS."""
    assert ops.dg_skin_geod_plan(1, 4096, 2048, 9) == (64, 8, 9)
    d, nodes = rand_case(7, 1, 4096, 2048)
    check_skin(ops, d, nodes, ring_k=9, sigma=[0.05])


def test_build_geod_follows_the_matrix(ops):
    """dg_build_geod on a matrix that is not the Euclidean one: nodes, sigma and the Euclidean ring are dg_build's, the rest is
    the statement's on dg_build's nodes; B = 2, N = 333."""
    g = torch.Generator().manual_seed(11)
    xyz = torch.rand(2, 333, 3, generator=g)
    d, _ = rand_case(12, 2, 333, 3)
    start = torch.tensor([5, 300], dtype=torch.int32).cuda()
    plain = ops.dg_build(xyz.cuda(), start)
    nodes = host(plain["nodes_idx"])
    ri, rd, rr = R.skin_batch(d, nodes, 9)
    for metric in ("euclidean", "geodesic"):
        b = ops.dg_build_geod(xyz.cuda(), dev(d), start, metric)
        assert np.array_equal(host(b["nodes_idx"]), nodes)
        assert host(b["sigma"]).tobytes() == host(plain["sigma"]).tobytes()
        assert np.array_equal(host(b["infl_idx"]), ri) and np.array_equal(host(b["dists"]), rd)
        assert np.array_equal(host(b["one_ring"]), rr if metric == "geodesic" else host(plain["one_ring"]))
        np.testing.assert_allclose(host(b["weights"]), R.weights(rd, host(b["sigma"])), rtol=0, atol=W_ATOL)
    assert not np.array_equal(rr, host(plain["one_ring"]))


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_launch_nothing(ops):
    from dvm import _lib
    lib = _lib.load()
    N = 64
    d, nodes = rand_case(8, 1, N, 32)
    dd, nn = dev(d), dev(nodes.astype(np.int32))
    infl = torch.full((1, N, 3), -7, dtype=torch.int32).cuda()
    dists = torch.full((1, N, 3), -7.0).cuda()
    ring = torch.full((1, 32, 16), -7, dtype=torch.int32).cuda()
    st = torch.cuda.current_stream().cuda_stream
    p = lambda t: t.data_ptr()   # noqa: E731
    skin = lambda Nn, k: lib.dvm_dg_skin_geod_f32(p(dd), p(nn), 1, N, Nn, k, p(infl), p(dists), p(ring), st)   # noqa: E731
    assert skin(2, 0) == EINVAL                 # Nn < 3
    assert skin(8, 9) == EINVAL                 # ring_k > Nn
    assert skin(32, 17) == EINVAL               # ring_k > 16
    assert skin(N + 1, 0) == EINVAL             # Nn > N
    assert lib.dvm_dg_skin_geod_f32(p(dd), p(nn), 1, N, 32, 9, p(infl), p(dists), None, st) == EINVAL    # a ring asked for, nowhere to put it
    assert lib.dvm_dg_skin_geod_slices_f32(p(dd), p(nn), 1, N, 32, 0, 9, p(infl), p(dists), p(ring), st) == EINVAL   # more waves than the kernel has
    t = ctypes.c_int()
    assert lib.dvm_dg_skin_geod_plan(1, N, 2, 0, ctypes.byref(t), ctypes.byref(t), ctypes.byref(t)) == EINVAL
    # the build entry: N above dvm_fps_f32's limit (nothing of that size is read: refused in front of every launch), a bad
    # ring metric, a short workspace
    xyz = torch.rand(1, N, 3).cuda()
    start = torch.zeros(1, dtype=torch.int32).cuda()
    nodes_o = torch.full((1, N // 2), -7, dtype=torch.int32).cuda()
    w = torch.full((1, N, 3), -7.0).cuda()
    sg = torch.full((1,), -7.0, dtype=torch.float64).cuda()
    nb = lib.dvm_dg_build_geod_workspace_bytes(1, N)
    ws = torch.empty(nb, dtype=torch.uint8).cuda()
    build = lambda n, metric, nbytes: lib.dvm_dg_build_geod_f32(p(xyz), p(dd), 1, n, p(start), metric, p(nodes_o), p(ring), p(infl), p(dists),  # noqa: E731
                                                                p(w), p(sg), p(ws), nbytes, st)
    assert build(12289, 0, nb) == EINVAL
    assert build(N, 2, nb) == EINVAL
    assert build(N, 0, nb - 1) == ENOSPACE
    with pytest.raises(ops.DvmError):
        ops.dg_skin_geod(dd, nn[:, :2])
    with pytest.raises(ValueError):
        ops.dg_build_geod(xyz, dd, start, "surface")
    torch.cuda.synchronize()
    for t_ in (infl, dists, ring, nodes_o, w, sg):
        assert bool((t_ == -7).all()), "a refused call wrote its outputs"
    assert build(N, 1, nb) == 0                 # and the same arguments within the limits run
    torch.cuda.synchronize()
    assert bool((nodes_o >= 0).all())
