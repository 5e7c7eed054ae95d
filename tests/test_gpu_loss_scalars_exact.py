"""-m gpu: the loss scalars of the pair path (losses[B,6]) and of the training criterion (terms) BIT FOR BIT on inputs whose
every fp32 intermediate is exact (tests/exact_inputs.py; CPU half: tests/test_loss_scalars_exact_cpu.py).

No tolerance: summation order and FMA contraction cannot move a bit on these inputs, so ARAP, the two Chamfer means of the
Pi-mapped cloud and the map term must EQUAL the definition evaluated on integers and rounded to float32 once.  One missing, doubled
or misindexed row — a dropped last wave, a padding row, slot s of the wrong neighbour row, another node's T, a partial sum in the
wrong slot — moves them by many ulps (the CPU half proves that for every kind of row).  The Chamfer means of the WARPED cloud
(the skinning weights exp(-d^2 / 2 sigma^2) are not dyadic) are recomputed from the device's own `warped` with the oracle's
Chamfer distances (pinned bit for bit by the suite), float64 mean, one rounding: within 1 float32 ulp — derived, not measured:
the double accumulation errs by <= n 2^-53 relative on either side, far below 2^-24, so only a value on a rounding boundary can
move, and then by one ulp.

Which kernel form each planted shape (N sources, M targets; B = 3 different pairs per launch: the batch strides of losses,
partial and arap) reaches — conditions: map_term_lds_applies ((N + M) * 16 + M * 40 <= 150 KiB) in csrc/dvm_geom.hip and
launch_dg_warp / launch_dg_warp_pair (Nn * 60 B <= 150 KiB) in csrc/dvm_graph.hip:
  (64, 65), (65, 64)        map_term_lds_kernel, one thread per point: exactly one full wave / one lane in a second wave
  (1024, 1025), (1025, 1024) its 1024-point pass edge: one full pass / a second pass of one point, whose partial goes to
                            slot 16 under the `slot < nblk` guard (nblk = 41)
  (300, 170)                ragged: 5 waves, the last one 44 lanes; nblk = 12 < 16 waves, the guard cuts empty waves
  (300, 2700)               156 000 B > 150 KiB: ops.pair_direction takes map_term_kernel<10>, ops.pair_forward the
                            neighbour-table form (gather_nbr_xyz_kernel + map_term_nbr_kernel) in BOTH directions
  (2700, 300)               its mirror: map_term_lds_kernel with three passes in ops.pair_direction, the neighbour-table
                            form in ops.pair_forward
  (5200, 64)                Nn * 60 B = 156 000 B > 150 KiB: rot6d_kernel, dg_warp_kernel, dg_arap_kernel instead of
                            dg_warp_arap_fused_kernel (every other shape: fused; in ops.pair_forward blockIdx.y = direction);
                            map_term_lds_kernel with six passes
ops.pair_forward reduces its eight Chamfer vectors by one launch of mean_grouped_kernel, ops.pair_direction its four by one-input
launches of the same kernel (launch_mean); both sum the map
term's partials by reduce_partials_kernel.  A mirrored planting (exact in both directions) exists when max(N, M) <= 8 groups
<= 8 min(N, M): ops.pair_forward runs those, and the one-way plantings of (300, 2700) / (2700, 300) both straight (direction 12
is the planted one) and with the clouds swapped (direction 21 is); the unplanted direction's ARAP is still exact.
The training criterion (ops.criterion_dir_train_forward on every shape above, ops.criterion_train_forward — the swapped-halves
form, N == M, N % 4 == 0 — on mirrored plantings of 64, 300, 1028 points) takes map_term_kernel<10> with `resid`, the four-way
mean_grouped_kernel, and the same launch_dg_warp.
The direct entries (ops.map_term: map_term_kernel<10> / <16>; ops.dg_warp_arap, ops.dg_warp_arap_graph: dg_warp_kernel +
dg_arap_kernel at ring widths 9 / 18) take richer plantings: non-zero weights in every slot, per-node rotations."""
import numpy as np
import pytest
import torch

import exact_inputs as X
from oracle import oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from dvm import ops as _ops
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _ops


@pytest.fixture(scope="module")
def wl(ops):
    return ops.deformer_weight_list(X.deformer_weights(), "cuda")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def _ids(s):
    return "x".join(str(v) for v in s) if isinstance(s, tuple) else str(s)


def _check_exact_terms(what, got, ref):
    """got: {2: arap, 3: .., 4: .., 5: map} float32 from the device; == the rational values.  On a mismatch the difference of the
    sums, looked up in ref['rows'], names the row."""
    for t, v in got.items():
        r = ref["losses"][t]
        assert np.float32(v) == r, "%s term %d: device %r, exact %r (%d ulp)" % (what, t, float(v), float(r), int(X.ulp_distance(v, r)))


def _check_warped_means(what, l0, l1, warped, verts_t):
    """the Chamfer means of the warped cloud against their recomputation from the device's own `warped`: <= 1 ulp (module docstring)"""
    d1, d2, _, _ = O.chamfer(warped, verts_t)
    e0, e1 = X.f32(d1.astype(np.float64).sum() / d1.size), X.f32(d2.astype(np.float64).sum() / d2.size)
    assert np.isfinite(warped).all()
    assert X.ulp_distance(l0, e0) <= 1 and X.ulp_distance(l1, e1) <= 1, (what, float(l0), float(e0), float(l1), float(e1))


def _check_pair_output(what, out, b, ref, verts_t, with_map=True):
    L = host(out["losses"])[b]
    assert np.array_equal(host(out["T12"])[b], ref["T12"]), what + ": T12 is not the lowest column of the group"
    assert np.array_equal(host(out["verts12"])[b], ref["verts12"].astype(np.float32)), what + ": verts12 is not the exact group mean"
    _check_exact_terms(what, {2: L[2], 3: L[3], 4: L[4]}, ref)
    if with_map:
        _check_exact_terms(what, {5: L[5]}, ref)
    else:
        assert L[5] == 0.0 and not np.signbit(L[5])
    _check_warped_means(what, L[0], L[1], host(out["warped"])[b], verts_t)


# ------------------------------------------------------------------------------------------------------------------ pair path
@pytest.mark.parametrize("shape", X.PAIR_SHAPES, ids=_ids)
def test_pair_direction_losses_exact(ops, wl, shape):
    a, cases = X.planted_batch(*shape, X.PAIR_SEED)
    out = ops.pair_direction(wl, dev(a["feat1"]), dev(a["feat2"]), dev(a["verts1"]), dev(a["verts2"]), X.ALPHA, dev(a["start1"]))
    torch.cuda.synchronize()
    for b, (p, r12, _) in enumerate(cases):
        _check_pair_output("pair_direction %s pair %d" % (shape, b), out, b, r12, p["verts2"])


@pytest.mark.parametrize("shape", [(65, 64), (300, 2700)], ids=_ids)
def test_pair_direction_without_map_term(ops, wl, shape):
    a, cases = X.planted_batch(*shape, X.PAIR_SEED)
    out = ops.pair_direction(wl, dev(a["feat1"]), dev(a["feat2"]), dev(a["verts1"]), dev(a["verts2"]), X.ALPHA, dev(a["start1"]),
                             with_map=False)
    torch.cuda.synchronize()
    for b, (p, r12, _) in enumerate(cases):
        _check_pair_output("pair_direction (no map) %s pair %d" % (shape, b), out, b, r12, p["verts2"], with_map=False)


@pytest.mark.parametrize("shape,with_map", [(s, True) for s in X.MIRRORED_SHAPES] + [(s, False) for s in X.MIRRORED_NOMAP_SHAPES],
                         ids=lambda v: _ids(v) if isinstance(v, tuple) else ("map" if v else "nomap"))
def test_pair_forward_both_directions_exact(ops, wl, shape, with_map):
    """mirrored planting: both directions of ONE launch are exact"""
    a, cases = X.planted_batch(*shape, X.PAIR_SEED, both=True)
    o12, o21 = ops.pair_forward(wl, dev(a["feat1"]), dev(a["feat2"]), dev(a["verts1"]), dev(a["verts2"]), X.ALPHA, dev(a["start1"]),
                                dev(a["start2"]), with_map=with_map)
    torch.cuda.synchronize()
    for b, (p, r12, r21) in enumerate(cases):
        _check_pair_output("pair_forward %s 12 pair %d" % (shape, b), o12, b, r12, p["verts2"], with_map)
        _check_pair_output("pair_forward %s 21 pair %d" % (shape, b), o21, b, r21, p["verts1"], with_map)


@pytest.mark.parametrize("swapped", [False, True], ids=["straight", "swapped"])
@pytest.mark.parametrize("shape", [(300, 2700), (2700, 300), (5200, 64)], ids=_ids)
def test_pair_forward_one_way_planting(ops, wl, shape, swapped):
    """No mirrored planting exists at these shapes (more than 8 targets per source).  straight: direction 12 of the launch is the planted
    one; swapped: the clouds change places, so direction 21 is.  The other direction's ARAP does not depend on the correspondence."""
    a, cases = X.planted_batch(*shape, X.PAIR_SEED)
    s, t = ("2", "1") if swapped else ("1", "2")
    outs = ops.pair_forward(wl, dev(a["feat" + s]), dev(a["feat" + t]), dev(a["verts" + s]), dev(a["verts" + t]), X.ALPHA,
                            dev(a["start" + s]), dev(a["start" + t]))
    torch.cuda.synchronize()
    planted, other = (outs[1], outs[0]) if swapped else outs
    for b, (p, r12, _) in enumerate(cases):
        _check_pair_output("pair_forward %s %s pair %d" % (shape, "21" if swapped else "12", b), planted, b, r12, p["verts2"])
        arap = X.reference_arap(p["verts2"], p["start2"])
        assert host(other["losses"])[b, 2] == arap, (shape, b, float(host(other["losses"])[b, 2]), float(arap))


def test_deformer_returns_the_planted_rows(ops, wl):
    """def9 = [verts1[node], -1, 1, 0, -1, -1, 0] exactly from the device decoder (every MLP input is an integer <= 255: exact in
    fp16, the split's low plane is zero) — the piece to look at first if an ARAP value above is off."""
    a, cases = X.planted_batch(300, 170, X.PAIR_SEED)
    st = lambda k, dt: dev(np.stack([c[1][k] for c in cases]).astype(dt))  # noqa: E731
    nodes = dev(np.stack([c[1]["graph"]["nodes_idx"] for c in cases]))
    def9 = ops.deformer(wl, dev(a["feat1"]), dev(a["feat2"]), dev(a["verts1"]), st("verts12", np.float32), st("idx11", np.int32),
                        st("idx22", np.int32), st("pval", np.float32), st("pidx", np.int32), nodes)
    for b, (_, r12, _) in enumerate(cases):
        assert np.array_equal(host(def9)[b], r12["def9"].astype(np.float32))


# --------------------------------------------------------------------------------------------------------- training criterion
def _device_geometry(ops, verts, start, refs):
    """graph and xyz kNN from the device build (what the training loop feeds the node); they equal the oracle's"""
    g = ops.dg_build(verts, start)
    knn = ops.knn_cdist(verts, verts, X.K_XYZ)
    for b, r in enumerate(refs):
        for k in ("nodes_idx", "one_ring", "infl_idx"):
            assert np.array_equal(host(g[k])[b], r["graph"][k]), k
        assert np.array_equal(host(knn)[b], r["idx11"])
    return {k: g[k] for k in ("nodes_idx", "one_ring", "infl_idx", "weights")}, knn


def _check_terms(what, terms, b, ref, warped, verts_t, with_map=True):
    t = host(terms)[b]
    _check_exact_terms(what, {2: t[5], 3: t[3], 4: t[4]}, ref)
    if with_map:
        _check_exact_terms(what, {5: t[0]}, ref)
    else:
        assert t[0] == 0.0
    _check_warped_means(what, t[1], t[2], warped, verts_t)


@pytest.mark.parametrize("shape", X.PAIR_SHAPES, ids=_ids)
def test_criterion_dir_train_terms_exact(ops, wl, shape):
    """terms = [map, Chamfer means of warped (2) and verts12 (2), ARAP, dist].  The node keeps `warped` in its arena; it is
    launch_dg_warp on the same graph and the same (exact) def9 rows as in ops.pair_direction, whose `warped` output stands in."""
    a, cases = X.planted_batch(*shape, X.PAIR_SEED)
    d = {k: dev(v) for k, v in a.items()}
    g, knn_s = _device_geometry(ops, d["verts1"], d["start1"], [c[1] for c in cases])
    knn_t = ops.knn_cdist(d["verts2"], d["verts2"], X.K_XYZ)
    terms, _ = ops.criterion_dir_train_forward(wl, d["feat1"], d["feat2"], d["verts1"], d["verts2"], g, knn_s, knn_t, X.ALPHA, 10, True)
    warped = host(ops.pair_direction(wl, d["feat1"], d["feat2"], d["verts1"], d["verts2"], X.ALPHA, d["start1"])["warped"])
    for b, (p, r12, _) in enumerate(cases):
        assert np.array_equal(host(knn_t)[b], r12["idx22"])
        _check_terms("criterion_dir %s pair %d" % (shape, b), terms, b, r12, warped[b], p["verts2"])
    if shape == (300, 170):
        terms0, _ = ops.criterion_dir_train_forward(wl, d["feat1"], d["feat2"], d["verts1"], d["verts2"], g, knn_s, knn_t, X.ALPHA, 10, False)
        for b, (p, r12, _) in enumerate(cases):
            _check_terms("criterion_dir (no map) pair %d" % b, terms0, b, r12, warped[b], p["verts2"], with_map=False)


@pytest.mark.parametrize("N", X.SWAPPED_SIZES)
def test_criterion_train_swapped_halves_terms_exact(ops, wl, N):
    """feat / verts (2B, N, .): the B first shapes, then the B second shapes; row b is direction 12 of pair b, row B + b direction 21."""
    B = 3
    a, cases = X.planted_batch(N, N, X.PAIR_SEED, B, both=True)
    d = {k: dev(v) for k, v in a.items()}
    verts, feat = torch.cat([d["verts1"], d["verts2"]]), torch.cat([d["feat1"], d["feat2"]])
    g, knn = _device_geometry(ops, verts, torch.cat([d["start1"], d["start2"]]), [c[1] for c in cases] + [c[2] for c in cases])
    terms, _ = ops.criterion_train_forward(wl, feat, verts, g, knn, X.ALPHA, 10, True)
    w12 = host(ops.pair_direction(wl, d["feat1"], d["feat2"], d["verts1"], d["verts2"], X.ALPHA, d["start1"])["warped"])
    w21 = host(ops.pair_direction(wl, d["feat2"], d["feat1"], d["verts2"], d["verts1"], X.ALPHA, d["start2"])["warped"])
    for b, (p, r12, r21) in enumerate(cases):
        _check_terms("criterion %d 12 pair %d" % (N, b), terms, b, r12, w12[b], p["verts2"])
        _check_terms("criterion %d 21 pair %d" % (N, b), terms, B + b, r21, w21[b], p["verts1"])
    assert (host(terms)[:, 6] == 0).all()


# ------------------------------------------------------------------------------------------------------------- direct entries
@pytest.mark.parametrize("N", [1, 26, 300])
@pytest.mark.parametrize("k,topk", [(10, 10), (1, 1), (16, 16), (10, 16), (7, 3)])
def test_map_term_exact(ops, k, topk, N):
    """N * k is no multiple of 256 at any of these sizes; M != N."""
    B, M = 3, N + 11
    assert (N * k) % 256
    cs = [X.map_term_direct(N, M, k, topk, 50 + b) for b in range(B)]
    st = lambda key: dev(np.stack([c[key] for c in cs]))  # noqa: E731
    out = host(ops.map_term(st("verts12"), st("verts2"), st("idx11"), st("idx22"), st("pval"), st("pidx")))
    for b, c in enumerate(cs):
        assert c["value"] > 0 and out[b] == c["value"], (b, float(out[b]), float(c["value"]))


def _warp_batch(N, Nn, K, B=3):
    cs = [X.warp_direct(N, Nn, K, 70 + b) for b in range(B)]
    st = lambda key: dev(np.stack([c[key] for c in cs]))  # noqa: E731
    g = {key: st(key) for key in ("nodes_idx", "one_ring", "infl_idx", "weights")}
    return cs, st("xyz"), g, st("R"), st("T")


def _check_warp(cs, warped, arap, sr):
    for b, c in enumerate(cs):
        assert np.array_equal(host(warped)[b], c["warped"].astype(np.float32))
        assert host(arap)[b] == c["arap"], (b, float(host(arap)[b]), float(c["arap"]))
        assert host(sr)[b] == c["sr"], (b, float(host(sr)[b]), float(c["sr"]))


@pytest.mark.parametrize("Nn", [1, 255, 256, 257, 600])
def test_dg_warp_arap_graph_exact(ops, Nn):
    """ring width 18, Nn independent of N (N = Nn + 77: no multiple of 256)"""
    cs, xyz, g, R, T = _warp_batch(Nn + 77, Nn, 18)
    _check_warp(cs, *ops.dg_warp_arap_graph(xyz, g, R, T))


@pytest.mark.parametrize("Nn", [1, 255, 256, 257, 600])
def test_dg_warp_arap_exact(ops, Nn):
    """the point-cloud graph's entry: ring width 9, Nn = N // 2 (N odd)"""
    cs, xyz, g, R, T = _warp_batch(2 * Nn + 1, Nn, 9)
    _check_warp(cs, *ops.dg_warp_arap(xyz, g, R, T))
