"""-m gpu: the uniform-grid neighbour searches of csrc/dvm_grid.hip (xyz kNN, graph ring / influence nodes, Chamfer) on
adversarial clouds, at sizes that pin every routing path, against plain references in the kernels' own rounding.

The grid kernels promise results equal to brute force bit for bit.  That rests on the certification bound
(margin = 64 ulp * (scale2 + |q|^2)), on the fall-backs after the walk (exhaustion at R >= G, the whole-target scan, the exact
fall-back lanes) and on the (distance, index) ranking.  The clouds below are the inputs where such code breaks: all points in
one cell, extents far from unit scale, a cloud far from the origin (scale2 >> h^2: no query certifies at radius 1), exact ties
across cell faces, duplicated rows, empty balls, and batches whose entries differ in kind (per-entry grid parameters).
"""
import numpy as np
import pytest
import torch

from oracle import oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from dvm import ops as _ops
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _ops


def host(t):
    return t.detach().cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------- clouds
# the seeded families (one generator per family, `cloud`, `batch`): tests/cloud_families.py
from cloud_families import F, FAMILIES, FNAMES, KINDS, _translated, _unit, batch, cloud  # noqa: E402,F401


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---------------------------------------------------------------------------------------------------------------- Chamfer
# dvm_chamfer_fwd_f32 (csrc/dvm_geom.hip) takes the grid when N >= 64, M >= 64 and NOT
#   few = B * (N + M) <= 65536 && N * M <= 2^25;
# otherwise the brute-force kernels: chamfer_split_kernel (target staged in LDS) for a target of <= 8192 points.
# The grid kernel holds the target in LDS when P * 16 + (G^3 + 1) * 4 <= 64 KB (P <= 2048 here), else reads global memory;
# the grid build keeps its points in registers when P <= 2048 ("cached") and re-reads them otherwise.
CHAMFER_SHAPES = [
    (8, 512, 384),      # few: 8 * 896 = 7168 <= 65536, N * M = 196608 <= 2^25 -> small brute force
    (2, 3000, 2200),    # few: 2 * 5200 = 10400 <= 65536, N * M = 6.6e6 <= 2^25 -> brute force at sizes the grid also serves
    (20, 2048, 2048),   # B * (N + M) = 81920 > 65536 -> grid; P = 2048: cached build, LDS-resident target (G = 12)
    (1, 9000, 8000),    # N * M = 7.2e7 > 2^25 -> grid at B = 1; P > 2048: uncached build, global-memory target (G = 16)
    (10, 4995, 2200),   # B * (N + M) = 71950 > 65536 -> grid, unequal sizes, uncached build of both clouds, global target
]
# (The partial-shape pair 4995 x 2200 at B = 4 is 28780 queries and N * M = 1.1e7: it takes the brute force, so the uncached
# grid case runs it at B = 10.)


def chamfer_ref(q, t):
    """Brute force in the kernel's difference form, (dx^2 + dy^2) + dz^2 in fp32, per batch entry on the device: the minimum
    and the LOWEST index attaining it."""
    d, ix = [], []
    for b in range(q.shape[0]):
        diff = q[b][:, None, :] - t[b][None, :, :]
        D = (diff[..., 0] * diff[..., 0] + diff[..., 1] * diff[..., 1]) + diff[..., 2] * diff[..., 2]
        m = D.min(dim=1).values
        d.append(m)
        ix.append((D == m[:, None]).float().argmax(dim=1))   # first maximum of the indicator: the lowest minimiser
    return torch.stack(d), torch.stack(ix).int()


def check_chamfer(ops, a, b, tag):
    d1, d2, i1, i2 = ops.chamfer(a, b, want_idx=True)
    for q, t, d, ix, side in ((a, b, d1, i1, "a->b"), (b, a, d2, i2, "b->a")):
        rd, ri = chamfer_ref(q, t)
        bad = (d != rd).any(1) | (ix != ri).any(1)
        assert not bool(bad.any()), (tag, side, "entries", torch.nonzero(bad).flatten().tolist())
    return d1, d2, i1, i2


@pytest.mark.parametrize("shape", CHAMFER_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("kind", KINDS)
def test_chamfer_vs_brute_force(ops, kind, shape):
    B, N, M = shape
    if kind == "mixed":
        B = max(B, F)    # every family present; the routing of each shape is unchanged at B = 12 (see CHAMFER_SHAPES)
    seed = 11 + KINDS.index(kind) + 31 * N
    a, b = dev(batch(kind, B, N, seed)), dev(batch(kind, B, M, seed + 7))
    d1, d2, i1, i2 = check_chamfer(ops, a, b, (kind, shape))
    if kind == "mixed":
        # every entry bit-equal to the same clouds run alone (at B = 1 the first three shapes take the brute force)
        for e in range(B):
            s1, s2, j1, j2 = ops.chamfer(a[e:e + 1], b[e:e + 1], want_idx=True)
            assert torch.equal(s1[0], d1[e]) and torch.equal(s2[0], d2[e]), (shape, e)
            assert torch.equal(j1[0], i1[e]) and torch.equal(j2[0], i2[e]), (shape, e)


# ---------------------------------------------------------------------------------------------------------------- xyz kNN
# dvm_knn_cdist_f32 takes the grid for a 3-D cloud against itself when N >= 64 (else knn_cdist3_kernel, brute force);
# the build is cached for N <= 2048 (and the kNN kernel stages the grid in LDS: 2048 * 16 + 1729 * 4 bytes <= 64 KB), uncached
# and global-memory above.  k = 16 is the largest k the entry accepts; k <= 3 / <= 10 / <= 16 select the K = 3 / 10 / 16 lists.
KNN_N = [63, 64, 2048, 4995]   # brute (N < 64) | grid (N = 64) | grid, cached build | grid, uncached build
KNN_K = [1, 10, 16]


@pytest.mark.parametrize("k", KNN_K)
@pytest.mark.parametrize("N", KNN_N)
@pytest.mark.parametrize("kind", KINDS)
def test_knn_self_vs_oracle(ops, kind, N, k):
    """Indices bit-equal to the oracle's matmul-form (ATen cdist rounding) brute force, ranked by (distance, index).  On
    'translated' (|p|^2 ~ 1.6e6) the matmul form cancels to a few ulps of |p|^2: most keys are 0 or one quantum, the order
    is mostly the index order, and the grid cannot certify any radius (the margin exceeds the box): every query is served by
    exhaustion.  The oracle restates ATen's rounding; the kernel is pinned to it."""
    B = F if kind == "mixed" else 8
    x = batch(kind, B, N, 101 + KINDS.index(kind) + N)
    xd = dev(x)
    idx = host(ops.knn_cdist(xd, xd, k))
    for b in range(B):
        assert np.array_equal(idx[b], O.knn_cdist(x[b], x[b], k)), (kind, N, k, b)
    solo = range(B) if kind == "mixed" else [0, B - 1]
    for b in solo:   # B = 1: the same bits as inside the batch
        assert np.array_equal(host(ops.knn_cdist(xd[b:b + 1], xd[b:b + 1], k))[0], idx[b]), (kind, N, k, b)


# ---------------------------------------------------------------------------------------------------------------- graph build
# dvm_dg_build_f32: FPS, then a grid over the N vertices and one over the N / 2 nodes, the node ring (grid_ring) and the
# influence nodes + nearest-vertex distance (grid_infl).  Builds are cached for P <= 2048:
DG_N = [700, 2048, 4096, 4995]   # both cached | both cached (vertices at the limit) | vertex grid uncached | both uncached


def check_graph(g, o, b, tag):
    for key in ("nodes_idx", "one_ring", "infl_idx", "dists"):
        assert np.array_equal(host(g[key])[b], o[key]), tag + (key,)
    np.testing.assert_allclose(host(g["weights"])[b], o["weights"], rtol=1e-5, atol=1e-7, equal_nan=True, err_msg=str(tag))
    np.testing.assert_allclose(host(g["sigma"])[b], o["sigma"], rtol=1e-12, equal_nan=True, err_msg=str(tag))


@pytest.mark.parametrize("N", DG_N)
@pytest.mark.parametrize("kind", KINDS)
def test_graph_build_vs_oracle(ops, kind, N):
    B = F if kind == "mixed" else 3
    x = batch(kind, B, N, 202 + KINDS.index(kind) + N)
    start = np.array([(7919 * b + 13 * N + 5) % N for b in range(B)], np.int32)   # a different FPS start per entry
    xd, sd = dev(x), dev(start)
    g = ops.dg_build(xd, sd)
    for b in range(B):
        check_graph(g, O.dg_build(x[b], int(start[b])), b, (kind, N, b))
    for b in (range(B) if kind == "mixed" else [B - 1]):
        s = ops.dg_build(xd[b:b + 1], sd[b:b + 1])
        for key in s:
            assert torch.equal(s[key][0], g[key][b]) or (key in ("weights", "sigma") and
                                                        torch.equal(s[key][0].isnan(), g[key][b].isnan()) and
                                                        torch.equal(s[key][0].nan_to_num(), g[key][b].nan_to_num())), \
                (kind, N, b, key)


# ---------------------------------------------------------------------------------------------------------------- non-finite
def test_non_finite_entry_is_isolated_at_grid_size(ops):
    """One entry of a (20, 2048, 2048) batch with NaN / inf coordinates: every other entry's Chamfer, kNN and graph outputs
    are bit-equal to the batch without that entry, and every index the searches return stays a valid row (later kernels
    gather through them unchecked).  A slot a search leaves empty — every key of a NaN node's fp64 ring search is NaN, every
    matmul-form key of a query at y = -inf against points at y > 0 is +inf — used to come out as 0x7fffffff."""
    B, N, M, bad = 20, 2048, 2048, 7
    a, b = batch("mixed", B, N, 901), batch("mixed", B, M, 902)
    a[bad, 5] = np.nan
    a[bad, 9, 1] = np.inf
    a[bad, 11, 1] = -np.inf     # every matmul-form key of this query is +inf: its kNN / influence lists stay empty
    b[bad, 100] = -np.inf
    b[bad, 3, 2] = np.nan
    keep = [e for e in range(B) if e != bad]
    ad, bd, ak, bk = dev(a), dev(b), dev(a[keep]), dev(b[keep])
    start = dev(np.arange(B, dtype=np.int32) * 97 % N)

    def in_range(t, hi):
        return int(t.min()) >= 0 and int(t.max()) < hi

    full, part = ops.chamfer(ad, bd, want_idx=True), ops.chamfer(ak, bk, want_idx=True)   # (B = 19: still the grid)
    for u, v in zip(full, part):
        assert torch.equal(u[keep], v)
    assert in_range(full[2], M) and in_range(full[3], N)
    for k in (1, 10, 16):
        kf, kp = ops.knn_cdist(ad, ad, k), ops.knn_cdist(ak, ak, k)
        assert torch.equal(kf[keep], kp), k
        assert in_range(kf, N), k
    gf, gp = ops.dg_build(ad, start), ops.dg_build(ak, start[keep])
    for key in gf:
        u, v = gf[key][keep], gp[key]
        assert torch.equal(u, v) or (key in ("weights", "sigma") and torch.equal(u.isnan(), v.isnan()) and
                                     torch.equal(u.nan_to_num(), v.nan_to_num())), key
    assert in_range(gf["nodes_idx"], N) and in_range(gf["one_ring"], N // 2) and in_range(gf["infl_idx"], N // 2)


# ---------------------------------------------------------------------------------------------------------------- backward
def rel(a, ref):
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    return float((a - ref).norm() / (ref.norm() + 1e-300))


@pytest.mark.parametrize("kind", ["random", "translated"])
def test_chamfer_backward_at_grid_size_vs_fp64(ops, kind):
    """nn_ops.chamfer_nn forward + backward at (20, 2048, 2048) (grid forward) against fp64 autograd of the squared distances
    to the KERNEL's own nearest neighbours (ties cannot make the comparison ambiguous)."""
    from dvm import nn_ops
    B, N, M = 20, 2048, 2048
    rng = np.random.default_rng(4 + len(kind))
    fam = _unit if kind == "random" else _translated
    a0 = np.stack([fam(N, rng) for _ in range(B)]).astype(np.float32)
    b0 = np.stack([fam(M, rng) for _ in range(B)]).astype(np.float32)
    g1, g2 = dev(rng.standard_normal((B, N)).astype(np.float32)), dev(rng.standard_normal((B, M)).astype(np.float32))
    a, b = dev(a0).requires_grad_(True), dev(b0).requires_grad_(True)
    d1, d2 = nn_ops.chamfer_nn(a, b)
    ((d1 * g1).sum() + (d2 * g2).sum()).backward()
    _, _, i1, i2 = ops.chamfer(a.detach(), b.detach(), want_idx=True)
    a64, b64 = dev(a0).double().requires_grad_(True), dev(b0).double().requires_grad_(True)
    nb = torch.gather(b64, 1, i1.long()[..., None].expand(-1, -1, 3))
    na = torch.gather(a64, 1, i2.long()[..., None].expand(-1, -1, 3))
    r1, r2 = ((a64 - nb) ** 2).sum(-1), ((b64 - na) ** 2).sum(-1)
    ((r1 * g1.double()).sum() + (r2 * g2.double()).sum()).backward()
    assert rel(d1, r1) < 1e-5 and rel(d2, r2) < 1e-5, (rel(d1, r1), rel(d2, r2))
    assert rel(a.grad, a64.grad) < 1e-5 and rel(b.grad, b64.grad) < 1e-5, (rel(a.grad, a64.grad), rel(b.grad, b64.grad))


# ---------------------------------------------------------------------------------------------------------------- pair level
def test_pair_on_translated_and_lattice_clouds_vs_oracle(ops, golden):
    """ops.pair_direction and ops.pair_forward on a batch of a translated pair (offset [1e3, -7e2, 4e2]) and a shuffled-lattice
    pair, at N = M = 2048 (the pair path's own grids: the xyz kNN idx11 / idx22, the graph, and the distance-only grouped
    Chamfer), against the oracle with test_pair_direction_vs_oracle's bars.  The coordinate bars are absolute at unit scale
    and scale with the clouds' magnitude (one fp32 ulp at 1e3 is 6e-5)."""
    B, N, M = 2, 2048, 2048
    w = golden("deformer_scape_r_weights")
    wl = ops.deformer_weight_list(w, "cuda")
    rng = np.random.default_rng(55)
    f1 = (0.3 * np.maximum(rng.standard_normal((B, N, 128)), 0)).astype(np.float32)
    f2 = (0.3 * np.maximum(rng.standard_normal((B, M, 128)), 0)).astype(np.float32)
    v1 = np.stack([cloud("translated", N, 1), cloud("lattice_shuffled", N, 2)])
    v2 = np.stack([cloud("translated", M, 3), cloud("lattice_shuffled", M, 4)])
    s1, s2 = np.array([17, 2000], np.int32), np.array([0, 1500], np.int32)
    alpha = 40.0
    d = [dev(t) for t in (f1, f2, v1, v2)]
    r12 = ops.pair_direction(wl, d[0], d[1], d[2], d[3], alpha, dev(s1))
    r21 = ops.pair_direction(wl, d[1], d[0], d[3], d[2], alpha, dev(s2))
    o12, o21 = ops.pair_forward(wl, *d, alpha, dev(s1), dev(s2))
    for key in r12:
        assert torch.equal(o12[key], r12[key]), ("12", key)
        assert torch.equal(o21[key], r21[key]), ("21", key)
    for out, (fa, fb, va, vb, st) in ((r12, (f1, f2, v1, v2, s1)), (r21, (f2, f1, v2, v1, s2))):
        for b in range(B):
            o = O.pair_direction(w, fa[b], fb[b], va[b], vb[b], alpha, int(st[b]))
            scale = max(1.0, float(np.abs(va[b]).max()), float(np.abs(vb[b]).max()))
            assert np.array_equal(host(out["T12"])[b], o["T12"]), b
            np.testing.assert_allclose(host(out["verts12"])[b], o["verts12"], rtol=0, atol=5e-6 * scale)
            np.testing.assert_allclose(host(out["warped"])[b], o["warped"], rtol=0, atol=1e-4 * scale)
            L = host(out["losses"])[b]
            np.testing.assert_allclose(L, o["losses"], rtol=1e-3, atol=1e-7)
            np.testing.assert_allclose(L[[3, 4, 5]], o["losses"][[3, 4, 5]], rtol=1e-4)
