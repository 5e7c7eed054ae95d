"""-m gpu: the backward kernels of the training step, row by row, on inputs where they go wrong: K1's backward
(csrc/dvm_softcorr_bwd.hip) on near-duplicate, duplicate, clustered, offset and rescaled features; the gather and atomics forms
of apply's backward (csrc/dvm_geom.hip) on hub lists at and around the heavy-target threshold; and every in-edge list route of
the N2P core's backward (csrc/dvm_n2p_bwd.hip).  Every check is PER ROW against float64, so one broken row cannot hide in a
whole-tensor norm.

K1 (ops.softcorr_bwd, variants 0 / 2: matrix cores at d = 128, 1: scalar).  Reference: float64 with exact-difference distances and
a dense softmax over all columns, at the forward's top-k columns, in the analytic form W = -alpha dL/dS / D (0 where D = 0),
df1 = rowsum(W) f1 - W f2, df2 = colsum(W) f2 - W^T f1 (k1_ref64; checked once against oracle/torch_ref.py::softcorr_bwd).  Bar for
every row of df1 and of df2:  err <= max(3 err32, K 2^-24 s), where err32 is the same row's error of the reference's own fp32
formulation (softmax(-alpha cdist) gathered at the same columns, fp32 autograd) and s = alpha sum_j (|gp_ij| + P_ij |G_i|)
(1 + alpha D_ij) in float64 (for a df2 row: the same sum over the column's i).  s bounds the two terms of dL/dS BEFORE they cancel:
fp32 rounds each of them, and a relative error e of D moves the row by about e s.  On a one-hot row the combined dL/dS is ~0, so a
bar built from it would reject a correct kernel; a kernel that mixes two distances for one top-k entry errs by O(1) s there.
Families: randn / relu (calibration, K below is set from them), near-duplicate columns planted at delta in {1e-1 .. 1e-4} times
the median nearest distance, exact duplicates (a key equal to a query, two equal keys so that the top-k holds a tie),
clusters of 30 columns within 1e-3 of the median nearest distance of one query (its top-10 and 20 columns that only the dense term
carries: their D is redone from the difference, BW_TAU), a common offset of 8x the feature rms on every channel, features x 1e-3
and x 1e2 with alpha divided by the scale, and zero upstream gradients (every third row: its df1 row must be exactly 0; every slot
but the top-1).  Every case is run twice: on the forward's own val / row_smax / row_sum, and on float64-exact ones (the
exact-forward rerun, always at the plain bar).  For cluster, offset and zero rows the first run may add 3 |ref(forward's P) - ref|
per row: the float64 formula on exact distances fed the forward's statistics, a term that measures only how far the forward's
distances (pinned to the oracle's fp32 formulation) sit from exact ones and nothing the backward recomputes.

apply_bwd and n2p_core_bwd: float64 autograd, per row; the bar is K 2^-24 times the float64 sum of the absolute values of the
terms that reach the row (for N2P propagated through the softmax, with the attention's own rounding).  Indices: hubs of in-degree
95 / 96 / 97 / 150 / 400 around the gather's heavy threshold (AG_HEAVY = 96), four heavy targets in one workgroup, a heavy last
target with M % 4 != 0, one target holding every edge, out-of-range and negative indices (no contribution, d_val = 0); N2P: a hub,
self-loops, all slots equal, each in-edge list route by the shape that selects it.  Both also at the edges of the list
builder's workgroup scan (csrc/dvm_revlist.hip, block_scan_counts): 1, 1023, 1025 and 2049 targets against its 1024 threads.
"""
import zlib

import pytest
import torch

from attention_ref import n2p_ref64
from oracle import torch_ref as TR

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -24
# One constant for every bar of this file.  At K = 16 a few clean-family rows (randn, relu) went over by up to 1.5x; at 64 the
# largest err / bar over every case here is 0.98.
K = 64.0
ALPHAS = [10.0, 33.0, 60.0, 101.0]
K1_FAMILIES = ["randn", "relu", "near1e-1", "near1e-2", "near1e-3", "near1e-4", "dup", "cluster", "offset", "scale1e-3", "scale1e2",
               "gzero_rows", "gzero_top1"]
# families whose forward-statistics run carries the forward term (k1_check); their exact-forward rerun meets the plain bar
FWD_TERM = {"cluster", "offset", "gzero_rows"}


@pytest.fixture(scope="module")
def ops():
    from dvm import ops as _ops
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _ops


def rel(a, ref):
    a, ref = a.detach().double(), ref.detach().double().to(a.device)
    return float((a - ref).norm() / (ref.norm() + 1e-300))


# ------------------------------------------------------------------------------------------------------------- K1 backward
def k1_ref64(f1, f2, neg_alpha, idx, gval, rows=128, stats=None):
    """One batch entry, float64: (df1 (N,d), df2 (M,d), s1 (N,), s2 (M,), exact (val, smax, ssum)).  Distances by the norm
    expansion, redone from the exact difference wherever it cancels (v < 1e-3 (|a|^2 + |b|^2)); row chunks keep the working set
    near rows * M * 8 bytes.  With stats = (val, smax, ssum) of a forward, P is that forward's: exp(S - smax) / ssum on exact
    distances, val at the top-k columns (what the kernel is handed); s is always the exact one."""
    a, b = f1.double(), f2.double()
    na, nb = (a * a).sum(1), (b * b).sum(1)
    alpha = -float(neg_alpha)
    N, M = a.shape[0], b.shape[0]
    df1, df2 = torch.zeros_like(a), torch.zeros_like(b)
    s1, s2 = torch.zeros(N, dtype=torch.float64, device=a.device), torch.zeros(M, dtype=torch.float64, device=a.device)
    ex = [torch.zeros_like(gval, dtype=torch.float64), torch.zeros(N, dtype=torch.float64, device=a.device),
          torch.zeros(N, dtype=torch.float64, device=a.device)]
    for r0 in range(0, N, rows):
        R = slice(r0, r0 + rows)
        A, ix, gv = a[R], idx[R].long(), gval[R].double()
        den = na[R, None] + nb[None]
        v = den - 2.0 * (A @ b.T)
        D = v.clamp_min(0).sqrt()
        ii, jj = (v < 1e-3 * den).nonzero(as_tuple=True)
        D[ii, jj] = (A[ii] - b[jj]).norm(dim=1)
        S = float(neg_alpha) * D
        P = torch.softmax(S, dim=1)
        ex[0][R], ex[1][R] = P.gather(1, ix), S.max(1)[0]
        ex[2][R] = torch.exp(S - ex[1][R, None]).sum(1)
        Pe = P
        if stats is not None:
            P = torch.exp(S - stats[1][R].double()[:, None]) / stats[2][R].double()[:, None]
            P = P.scatter(1, ix, stats[0][R].double())
        gpt = gv * P.gather(1, ix)
        G = gpt.sum(1)
        gp = torch.zeros_like(P).scatter_add_(1, ix, gpt)
        W = float(neg_alpha) * (gp - P * G[:, None]) / torch.where(D > 0, D, torch.ones_like(D))
        W = torch.where(D > 0, W, torch.zeros_like(W))
        df1[R] = W.sum(1)[:, None] * A - W @ b
        df2 += W.sum(0)[:, None] * b - W.T @ A
        gpe = gv * Pe.gather(1, ix)
        Ge = gpe.sum(1)
        T = alpha * (torch.zeros_like(Pe).scatter_add_(1, ix, gpe).abs() + Pe * Ge.abs()[:, None]) * (1.0 + alpha * D)
        s1[R] = T.sum(1)
        s2 += T.sum(0)
    return df1, df2, s1, s2, ex


def k1_fp32_formulation(f1, f2, neg_alpha, idx, gval):
    """The reference's own formulation in fp32 (models/loss.py:110-114 + the top-k gather), one batch entry."""
    a = f1.detach().clone().requires_grad_(True)
    b = f2.detach().clone().requires_grad_(True)
    P = torch.softmax(torch.cdist(a[None], b[None])[0] * neg_alpha, dim=-1)
    (P.gather(1, idx.long()) * gval).sum().backward()
    return a.grad, b.grad


def test_k1_ref64_matches_oracle_autograd(ops):
    g = torch.Generator().manual_seed(11)
    f1, f2 = torch.randn(2, 40, 24, generator=g) * 0.3, torch.randn(2, 50, 24, generator=g) * 0.3
    f2[0, 7] = f1[0, 3]                                                     # one D = 0 entry
    idx = torch.stack([torch.randperm(50, generator=g)[:10] for _ in range(80)]).view(2, 40, 10).int()
    idx[0, 3, 0] = 7
    gval = torch.randn(2, 40, 10, generator=g)
    na = ops.neg_alpha_f32(33.0)
    _, r1, r2 = TR.softcorr_bwd(f1, f2, na, idx, gval)
    for e in range(2):
        d1, d2 = k1_ref64(f1[e], f2[e], na, idx[e], gval[e], rows=16)[:2]
        assert rel(d1, r1[e]) < 1e-12 and rel(d2, r2[e]) < 1e-12, (rel(d1, r1[e]), rel(d2, r2[e]))


def _unit(g, d):
    u = torch.randn(d, generator=g, dtype=torch.float64)
    return u / u.norm()


def k1_case(family, B, N, M, d, alpha, seed):
    """-> (f1, f2, gval, alpha) on the CPU (float32) for one family; `alpha` is rescaled for the scale families."""
    g = torch.Generator().manual_seed(seed)
    if family == "randn" or family == "offset":
        f1, f2 = torch.randn(B, N, d, generator=g) * 0.25, torch.randn(B, M, d, generator=g) * 0.25
        if family == "offset":                                              # 8 x the per-channel rms (0.25) on every channel
            f1, f2 = f1 + 2.0, f2 + 2.0
    else:
        f1, f2 = 0.3 * torch.relu(torch.randn(B, N, d, generator=g)), 0.3 * torch.relu(torch.randn(B, M, d, generator=g))
    gval = torch.randn(B, N, 10, generator=g)
    f1d, f2d = f1.double(), f2.double()
    plant_rows = [3, N // 2, N - 1] if N > 6 else [0]
    for e in range(B):
        q_nn = torch.cdist(f1d[e, plant_rows], f2d[e]).min(1)[0]
        med = float(q_nn.median())
        cols = torch.randperm(M, generator=g).tolist()
        if family.startswith("near"):                                       # one column at delta * med from each planted row
            delta = float(family[4:])
            for q in plant_rows:
                j = cols.pop()
                f2[e, j] = (f1d[e, q] + delta * med * _unit(g, d)).float()
        elif family == "dup":
            q0, q1 = plant_rows[0], plant_rows[-1]
            f2[e, cols.pop()] = f1[e, q0]                                   # D = 0: no gradient through this entry
            j1, j2 = cols.pop(), cols.pop()
            f2[e, j1] = (f1d[e, q1] + 0.2 * med * _unit(g, d)).float()
            f2[e, j2] = f2[e, j1]                                           # a tie inside q1's top-k
        elif family == "cluster":                                           # 30 columns within 1e-3 med of one query
            q = plant_rows[len(plant_rows) // 2]
            for _ in range(min(30, M // 2)):
                r = 1e-3 * med * (0.5 + 0.5 * float(torch.rand(1, generator=g)))
                f2[e, cols.pop()] = (f1d[e, q] + r * _unit(g, d)).float()
    if family == "scale1e-3":
        f1, f2, alpha = f1 * 1e-3, f2 * 1e-3, alpha * 1e3
    elif family == "scale1e2":
        f1, f2, alpha = f1 * 1e2, f2 * 1e2, alpha * 1e-2
    elif family == "gzero_rows":
        gval[:, ::3] = 0.0
    elif family == "gzero_top1":
        gval[:, :, 1:] = 0.0
    return f1, f2, gval, alpha


def k1_rows(got, ref, ref32, s, extra, what):
    """Per-row check; returns the largest err / bar."""
    err = (got.double() - ref).norm(dim=1)
    err32 = (ref32.double() - ref).norm(dim=1)
    bar = torch.maximum(3.0 * err32, K * EPS * s) + 3.0 * extra
    ratio = err / torch.where(bar > 0, bar, torch.full_like(bar, 1e-300))
    k = int(ratio.argmax())
    assert bool((err <= bar).all()), "%s row %d: err %.3e bar %.3e (3 err32 %.3e, K eps s %.3e, 3 fwd %.3e); %d rows over" % (
        what, k, err[k], bar[k], 3 * err32[k], K * EPS * s[k], 3 * extra[k], int((err > bar).sum()))
    return float(ratio[k])


def k1_check(ops, f1, f2, gval, alpha, variant, fwd_term=False):
    """Forward + backward on the GPU, every row checked; then the same backward on float64-exact val / row_smax / row_sum (the
    exact-forward rerun), which must meet the bar without any forward term.  fwd_term: the run on the forward's own statistics
    may add 3 |ref(forward's P) - ref| per row — the float64 formula on exact distances fed the forward's val / smax / ssum, so
    the term measures only how far the forward's distances sit from exact ones.  Returns the largest err / bar."""
    f1, f2, gval = f1.cuda(), f2.cuda(), gval.cuda()
    na = ops.neg_alpha_f32(alpha)
    val, idx, smax, ssum = ops.softcorr(f1, f2, alpha)
    df1, df2 = ops.softcorr_bwd(f1, f2, alpha, val, idx, smax, ssum, gval, variant=variant)
    torch.cuda.synchronize()
    assert torch.isfinite(df1).all() and torch.isfinite(df2).all()
    zero = (gval == 0).all(-1)
    assert bool((df1[zero] == 0).all()), "a row whose upstream gradients are all 0 must get an exactly-0 df1 row"
    tol = 1e-4 if alpha <= 40 else 1e-3                                     # tests/test_gpu_backward.py's whole-tensor bars
    worst, whole = 0.0, {}
    for e in range(f1.shape[0]):
        r1, r2, s1, s2, ex = k1_ref64(f1[e], f2[e], na, idx[e], gval[e])
        t1, t2 = k1_fp32_formulation(f1[e], f2[e], na, idx[e], gval[e])
        x1, x2 = torch.zeros_like(s1), torch.zeros_like(s2)
        if fwd_term:
            q1, q2 = k1_ref64(f1[e], f2[e], na, idx[e], gval[e], stats=(val[e], smax[e], ssum[e]))[:2]
            x1, x2 = (q1 - r1).norm(dim=1), (q2 - r2).norm(dim=1)
        exs = [x.float().contiguous()[None] for x in ex]
        g1, g2 = ops.softcorr_bwd(f1[e:e + 1], f2[e:e + 1], alpha, exs[0], idx[e:e + 1], exs[1], exs[2], gval[e:e + 1], variant=variant)
        for got, ref, ref32, s, extra, side in ((df1[e], r1, t1, s1, x1, "df1"), (df2[e], r2, t2, s2, x2, "df2"),
                                                (g1[0], r1, t1, s1, 0 * s1, "df1 exact-forward"), (g2[0], r2, t2, s2, 0 * s2, "df2 exact-forward")):
            worst = max(worst, k1_rows(got, ref, ref32, s, extra, "entry %d %s" % (e, side)))
            acc = whole.setdefault(side, [0.0, 0.0, 0.0])
            acc[0] += float((got.double() - ref).norm() ** 2)
            acc[1] += float(ref.norm() ** 2)
            acc[2] += float(extra.pow(2).sum())
    for side, (e2, r2, x2) in whole.items():
        assert e2 ** 0.5 <= tol * r2 ** 0.5 + 3 * x2 ** 0.5, (side, (e2 / max(r2, 1e-300)) ** 0.5)
    return worst


@pytest.mark.parametrize("variant", [0, 1, 2])
@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("family", K1_FAMILIES)
def test_k1_bwd_families(ops, family, alpha, variant):
    """1 x 1024 x 1024: split 4 (base 16 workgroups, 16 inner tiles)."""
    f1, f2, gval, a = k1_case(family, 1, 1024, 1024, 128, alpha, seed=zlib.crc32(family.encode()) % 10007 + int(alpha))
    k1_check(ops, f1, f2, gval, a, variant, fwd_term=family in FWD_TERM)


@pytest.mark.parametrize("variant", [2, 1])
@pytest.mark.parametrize("family", ["relu", "near1e-3", "dup", "cluster"])
@pytest.mark.parametrize("alpha", [33.0, 101.0])
@pytest.mark.parametrize("shape", [
    (2, 300, 250),     # split 1: 3 inner tiles on the short side
    (8, 2048, 2048),   # split 2: the training shape (256 workgroups before the split)
    (4, 2048, 2048),   # split 4
    (1, 2048, 2048),   # split 8
    (1, 4995, 2200),   # split 8: 35 inner tiles, ragged outer blocks on both sides
    (1, 129, 191),     # split 1: one row past an outer block, a partial inner tile
    (2, 191, 2049),    # split 1 (3 inner tiles on the short side), one column past a tile
    (1, 2049, 2049),   # split 8: one row and one column past the tiling
])
def test_k1_bwd_shapes(ops, shape, alpha, family, variant):
    B, N, M = shape
    f1, f2, gval, a = k1_case(family, B, N, M, 128, alpha, seed=N * 7 + M)
    k1_check(ops, f1, f2, gval, a, variant, fwd_term=family in FWD_TERM)


@pytest.mark.parametrize("family", ["relu", "near1e-3", "near1e-4", "dup", "cluster", "offset"])
@pytest.mark.parametrize("alpha", [33.0, 101.0])
@pytest.mark.parametrize("d", [36, 64, 132])
def test_k1_bwd_scalar_dims(ops, d, alpha, family):
    """The scalar kernel at d != 128 (variant 0 takes it there too): 2 x 300 x 250."""
    f1, f2, gval, a = k1_case(family, 2, 300, 250, d, alpha, seed=d)
    k1_check(ops, f1, f2, gval, a, 1, fwd_term=family in FWD_TERM)
    k1_check(ops, f1, f2, gval, a, 0, fwd_term=family in FWD_TERM)


# ------------------------------------------------------------------------------------------------------------- apply backward
def apply_check(ops, val, idx, V, gout, atomics):
    dval, dV = ops.apply_bwd(val.cuda(), idx.cuda(), V.cuda(), gout.cuda(), atomics=atomics)
    torch.cuda.synchronize()
    B, N, k = val.shape
    M, C = V.shape[1], V.shape[2]
    vd, Vd, gd, ix = val.double().cuda(), V.double().cuda(), gout.double().cuda(), idx.long().cuda()
    ok = (ix >= 0) & (ix < M)
    ixc = torch.where(ok, ix, torch.zeros_like(ix))
    rows = torch.gather(Vd, 1, ixc.reshape(B, N * k, 1).expand(-1, -1, C)).view(B, N, k, C)
    ref_dval = torch.where(ok, (rows * gd[:, :, None]).sum(-1), torch.zeros_like(vd))
    bar_dval = K * EPS * (rows.abs() * gd.abs()[:, :, None]).sum(-1)
    assert bool((dval.double()[~ok] == 0).all()), "d_val must be 0 at out-of-range indices"
    err = (dval.double() - ref_dval).abs()
    assert bool((err <= bar_dval).all()), "d_val: %d entries over, worst err %.3e" % (int((err > bar_dval).sum()), float(err.max()))
    # d_V[j] = sum over (i, t) with idx = j of val[i, t] gout[i]: scatter in float64 (signed terms and their magnitudes)
    w = torch.where(ok, vd, torch.zeros_like(vd))
    terms = (w[..., None] * gd[:, :, None, :]).reshape(B, N * k, C)
    ref = torch.zeros(B, M, C, dtype=torch.float64, device=terms.device).scatter_add_(1, ixc.reshape(B, N * k, 1).expand(-1, -1, C), terms)
    mag = torch.zeros_like(ref).scatter_add_(1, ixc.reshape(B, N * k, 1).expand(-1, -1, C), terms.abs())
    err = (dV.double() - ref).norm(dim=2)
    bar = K * EPS * mag.norm(dim=2)
    assert bool((err <= bar).all()), "d_V: rows %s over (err %s bar %s)" % (
        (err > bar).nonzero()[:4].tolist(), err[err > bar][:4].tolist(), bar[err > bar][:4].tolist())


def apply_inputs(B, N, M, k, C, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(B, N, k, generator=g), torch.randn(B, M, C, generator=g), torch.randn(B, N, C, generator=g), g)


def plant(idx, e, plan, g, M):
    """Exact in-degrees {target: deg} in entry e: every other edge is moved off the planted targets first, then each target gets
    its own disjoint set of edge positions.  Asserts the final in-degrees."""
    flat = idx[e].view(-1)
    planted = torch.tensor(sorted(plan), dtype=flat.dtype)
    free = [j for j in range(M) if j not in plan]
    hit = torch.isin(flat, planted)
    flat[hit] = torch.tensor(free, dtype=flat.dtype)[torch.randint(0, len(free), (int(hit.sum()),), generator=g)]
    pos = torch.randperm(flat.numel(), generator=g)
    k = 0
    for j, deg in plan.items():
        flat[pos[k:k + deg]] = j
        k += deg
    for j, deg in plan.items():
        assert int((flat == j).sum()) == deg


@pytest.mark.parametrize("atomics", [False, True])
@pytest.mark.parametrize("deg", [95, 96, 97, 150, 400])
def test_apply_bwd_hub_in_degree(ops, deg, atomics):
    """One target per entry at in-degree deg (AG_HEAVY = 96: 97 is the first heavy one; 97 and 150 split with a tail)."""
    B, N, M, k, C = 2, 300, 500, 10, 64
    val, V, gout, g = apply_inputs(B, N, M, k, C, deg)
    idx = torch.randint(0, M, (B, N, k), generator=g, dtype=torch.int32)
    plant(idx, 0, {7: deg}, g, M)
    plant(idx, 1, {M - 1: deg}, g, M)                  # the last target (its workgroup is full: 500 % 4 = 0)
    apply_check(ops, val, idx, V, gout, atomics)


@pytest.mark.parametrize("atomics", [False, True])
def test_apply_bwd_heavy_workgroup_and_tail(ops, atomics):
    """Targets 8..11 (one workgroup) all heavy with 97 / 98 / 99 / 101 in-edges; entry 1: a heavy last target at M - 1 = 502
    (M % 4 = 3: its workgroup has three rows)."""
    B, N, M, k, C = 2, 400, 503, 10, 200
    val, V, gout, g = apply_inputs(B, N, M, k, C, 3)
    idx = torch.randint(0, 20, (B, N, k), generator=g, dtype=torch.int32) * 25 + 1   # background: every 25th target, off 8..11
    idx = torch.where(idx >= M, idx - 25, idx)
    plant(idx, 0, {8: 97, 9: 98, 10: 99, 11: 101}, g, M)
    plant(idx, 1, {M - 1: 133}, g, M)
    apply_check(ops, val, idx, V, gout, atomics)


@pytest.mark.parametrize("atomics", [False, True])
def test_apply_bwd_single_target(ops, atomics):
    """Every one of the N k = 20480 edges into target 3 (N = 2048): one list, split four ways."""
    B, N, M, k, C = 1, 2048, 2048, 10, 128
    val, V, gout, g = apply_inputs(B, N, M, k, C, 4)
    apply_check(ops, val, torch.full((B, N, k), 3, dtype=torch.int32), V, gout, atomics)


@pytest.mark.parametrize("atomics", [False, True])
def test_apply_bwd_out_of_range(ops, atomics):
    B, N, M, k, C = 2, 333, 97, 10, 30
    val, V, gout, g = apply_inputs(B, N, M, k, C, 5)
    idx = torch.randint(-3 * M, 3 * M, (B, N, k), generator=g, dtype=torch.int32)
    idx[0, :, 0] = M
    idx[1, :, -1] = -1
    plant(idx, 1, {5: 150}, g, M)
    apply_check(ops, val, idx, V, gout, atomics)


@pytest.mark.parametrize("atomics", [False, True])
@pytest.mark.parametrize("C", [1, 3, 4, 64, 200, 256])
@pytest.mark.parametrize("k", [1, 10, 16, 64])
def test_apply_bwd_topk_channels(ops, k, C, atomics):
    """M = 5000 (not a multiple of the list scan's 1024 threads); skewed targets and one heavy row per entry."""
    B, N, M = 2, 700, 5000
    val, V, gout, g = apply_inputs(B, N, M, k, C, k * 1000 + C)
    idx = (torch.rand(B, N, k, generator=g) ** 3 * M).int().clamp_(0, M - 1)
    plant(idx, 0, {M - 1: min(N * k // 2, 197)}, g, M)
    apply_check(ops, val, idx, V, gout, atomics)


@pytest.mark.parametrize("atomics", [False, True])
@pytest.mark.parametrize("M", [1, 1023, 1025, 2049])
def test_apply_bwd_scan_edges(ops, M, atomics):
    """M at the edges of the list scan's 1024 threads (one target; one short of a counter per thread; 2 and 3 counters per
    thread with trailing threads that own none); the last target holds half of the entries."""
    B, N, k, C = 2, 64, 10, 8
    val, V, gout, g = apply_inputs(B, N, M, k, C, M)
    idx = torch.randint(0, M, (B, N, k), generator=g, dtype=torch.int32)
    if M > 1:                                          # (M = 1: target 0 = M - 1 holds every entry already)
        for e in range(B):
            plant(idx, e, {M - 1: N * k // 2}, g, M)
    apply_check(ops, val, idx, V, gout, atomics)


# ------------------------------------------------------------------------------------------------------------- N2P backward
def n2p_check(ops, qkv, idx, gout, H=4):
    """d_qkv per row against float64 autograd of models/model.py:339-350; bar: K 2^-24 times the float64 absolute terms of each
    channel's sum, carried through the softmax (a relative error of a logit moves the weights by a (|e| + sum a |e|))."""
    B, N, C3 = qkv.shape
    C, Kn, Dh = C3 // 3, idx.shape[-1], C3 // 3 // H
    q_, i_, g_ = qkv.cuda(), idx.cuda(), gout.cuda()
    out, attn = ops.n2p_core_fwd(q_, i_, H)
    dqkv = ops.n2p_core_bwd(q_, i_, attn, g_, H)
    torch.cuda.synchronize()
    for e in range(B):
        x = qkv[e:e + 1].double().cuda().requires_grad_(True)
        r = n2p_ref64(x, i_[e:e + 1], H)                                     # the float64 block shared with tests/attention_ref.py
        gi, kp, vp, kj, vj, qh, a, ref = r["gi"], r["kp"], r["vp"], r["kj"], r["vj"], r["qh"], r["a"], r["out"]
        gd = g_[e:e + 1].double()
        (ref * gd).sum().backward()
        with torch.no_grad():
            gh = gd.view(1, N, 1, H, Dh)
            ae = (qh.abs() * (kj.abs() + kp.abs()[:, :, None]).view(1, N, Kn, H, Dh)).sum(-1) / Dh ** 0.5   # |logit| terms
            ad = (gh.abs() * (vj.abs() + vp.abs()[:, :, None]).view(1, N, Kn, H, Dh)).sum(-1)              # |g . vp_j| terms
            da = (gh * vj.view(1, N, Kn, H, Dh)).sum(-1)
            dev = (da - (a * da).sum(2, keepdim=True)).abs()
            ade = a * (ad + (a * ad).sum(2, keepdim=True)) + a * dev * (ae + (a * ae).sum(2, keepdim=True))
            aa = a * (1.0 + ae + (a * ae).sum(2, keepdim=True))
            mq = (ade.unsqueeze(-1) * kj.abs().view(1, N, Kn, H, Dh)).sum(2).reshape(1, N, C) / Dh ** 0.5
            tk = (ade.unsqueeze(-1) * qh.abs()).reshape(1, N * Kn, C) / Dh ** 0.5
            tv = (aa.unsqueeze(-1) * gh.abs()).reshape(1, N * Kn, C)
            # + the self term -(sum_j de_ij) q_i / sqrt(Dh) of kp_i: 0 analytically (the kernel leaves it out), fp64 noise here
            mk = torch.zeros(1, N, C, dtype=torch.float64, device=x.device).scatter_add_(1, gi, tk)
            mk += (ade.sum(2).unsqueeze(-1) * qh.abs()[:, :, 0]).reshape(1, N, C) / Dh ** 0.5
            mv = torch.zeros(1, N, C, dtype=torch.float64, device=x.device).scatter_add_(1, gi, tv) + gd.abs()
            mag = torch.cat([mq, mk, mv], -1)[0].view(N, 3, C)
            err = (dqkv[e].double().view(N, 3, C) - x.grad[0].view(N, 3, C)).norm(dim=2)
            bar = K * EPS * mag.norm(dim=2)
            bad = err > bar
            assert not bool(bad.any()), "entry %d: %d (row, part) over; first %s err %.3e bar %.3e" % (
                e, int(bad.sum()), bad.nonzero()[0].tolist(), float(err[bad][0]), float(bar[bad][0]))
    return dqkv


def n2p_inputs(B, N, C, Kn, family, seed):
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B, N, 3 * C, generator=g)
    gout = torch.randn(B, N, C, generator=g)
    idx = torch.randint(0, N, (B, N, Kn), generator=g, dtype=torch.int32)
    if family == "hub":                       # every point lists point 5 (in-degree N), one entry also at its last point
        idx[:, :, 0] = min(5, N - 1)
        idx[-1, :, -1] = N - 1
    elif family == "self":                    # self-loops in every list (kd = vd = 0 on that slot)
        idx[:, :, Kn // 2] = torch.arange(N, dtype=torch.int32)
    elif family == "same":                    # all K slots equal: a uniform softmax over copies of one row
        idx[:] = idx[:, :, :1]
    return qkv, idx, gout


@pytest.mark.parametrize("C", [64, 128])
@pytest.mark.parametrize("family", ["random", "hub", "self", "same"])
@pytest.mark.parametrize("Kn", [1, 40, 64])
@pytest.mark.parametrize("B,N", [
    (2, 2048),      # global route: three kernels (B < 4)
    (4, 2048),      # LDS route: one workgroup per cloud (B >= 4, (2N + 1) 4 <= 96 KiB)
    (8, 2048),      # LDS route at the training shape
    (4, 1000),      # LDS route with N < 1024: one counter per scan thread
])
def test_n2p_bwd_routes(ops, B, N, Kn, family, C):
    assert not ops.is_deterministic()
    qkv, idx, gout = n2p_inputs(B, N, C, Kn, family, seed=B * N + Kn + C)
    n2p_check(ops, qkv, idx, gout)


@pytest.mark.parametrize("family", ["random", "hub"])
@pytest.mark.parametrize("N", [
    12287,          # LDS route: the largest N with (2N + 1) 4 <= 96 KiB
    12288,          # global route again, just above the LDS cap
])
def test_n2p_bwd_lds_cap(ops, N, family):
    qkv, idx, gout = n2p_inputs(4, N, 64, 8, family, seed=N)
    n2p_check(ops, qkv, idx, gout)


@pytest.mark.parametrize("family", ["random", "hub"])
@pytest.mark.parametrize("B,N,Kn,det", [(B, N, Kn, det) for det in (False, True) for B, N, Kn in [
    (1, 1, 1),      # one counter: every scan thread but the first owns an empty chunk
    (1, 1025, 8),   # 2 counters per scan thread, 511 trailing threads with none; global route
    (4, 1025, 8),   # the same on the LDS route
    (4, 2049, 8),   # 3 counters per thread: chunk boundaries off the wave boundaries
]] + [(4, 205, 40, False)])   # 8200 entries: one past the LDS build's 8 x 1024 stride
def test_n2p_bwd_scan_edges(ops, B, N, Kn, det, family):
    """The list builder's shared scan at its edges (block_scan_counts: per = ceil(N / 1024)), on every route: global and LDS by
    B, ordered under dvm_set_deterministic (det) with two calls bit for bit."""
    qkv, idx, gout = n2p_inputs(B, N, 64, Kn, family, seed=B * N + Kn)
    prev = ops.set_deterministic(det)
    try:
        d1 = n2p_check(ops, qkv, idx, gout)
        if det:
            out, attn = ops.n2p_core_fwd(qkv.cuda(), idx.cuda(), 4)
            assert torch.equal(d1, ops.n2p_core_bwd(qkv.cuda(), idx.cuda(), attn, gout.cuda(), 4))
    finally:
        ops.set_deterministic(prev)


@pytest.mark.parametrize("family", ["random", "hub", "same"])
@pytest.mark.parametrize("B,N,Kn,C", [(4, 2048, 40, 64), (2, 3001, 64, 128), (1, 12288, 8, 64)])
def test_n2p_bwd_deterministic_route(ops, B, N, Kn, C, family):
    """dvm_set_deterministic: the ordered in-edge lists (N 4 <= 96 KiB); two calls bit for bit."""
    qkv, idx, gout = n2p_inputs(B, N, C, Kn, family, seed=N + Kn)
    prev = ops.set_deterministic(True)
    try:
        d1 = n2p_check(ops, qkv, idx, gout)
        out, attn = ops.n2p_core_fwd(qkv.cuda(), idx.cuda(), 4)
        d2 = ops.n2p_core_bwd(qkv.cuda(), idx.cuda(), attn, gout.cuda(), 4)
        assert torch.equal(d1, d2)
    finally:
        ops.set_deterministic(prev)
