"""References, per-element bounds, hard input families and fp32 restatements for the geometric loss backward kernels
(csrc/dvm_loss_bwd.hip: rot6d_bwd / def9_bwd, dg_warp_bwd + dg_arap_bwd, chamfer_bwd).  Used by tests/test_gpu_geom_backward_rows.py
(device) and tests/test_geom_backward_rows_cpu.py (the same checks on the restatements, and on planted mutations of them).

Reference: float64 evaluation of the definition on the fp32 inputs — oracle/torch_ref.py::rot6d and ::dg_warp_arap under autograd,
and for Chamfer the gradient of sum(g1 * D[i, i1(i)]) + sum(g2 * D[i2(j), j]) with the index lists the kernel is handed.

Scatter sums (warp / ARAP, Chamfer).  Every output element is checked on its own:

    |dev - ref64| <= 2 u (n + c) A,      u = 2^-24

n  the number of addends that land on the element (atomics and the per-thread accumulator's adds alike);
A  the sum over those addends of the product of the factors' magnitudes, a cancelling difference counted as the sum of its operands'
   magnitudes: warp |w g| (d_T), |w g d_e| (d_R), d = v - g_s; ARAP, with m = |g_a| + |t_a| + |g_b| + |t_b| + |R_a| |d| componentwise
   and k = 2 g_arap / Nn: |k| m (d_T, on node a and on ring node b), |k| m |d_e| (d_R); Chamfer |2 g (src - oth)|;
c  the number of roundings on the longest chain that forms ONE addend, counted from the definition:
   warp-ARAP c = 8:  k = 2 g / Nn (1: the division); d = g_a - g_b (1); R d = two products' sum plus a third (1 + 2); the residual's
                     last subtraction (1; the sums g + t and their difference are shorter than the R d branch); k * residual (1);
                     times d_e for d_R (1).  The warp addends w g (1) and (w g) d_e (3 with d) are shorter.
   Chamfer   c = 2:  src - oth (1), times 2 g (1; the doubling is exact).
An addend's rounding error is then <= c u times its envelope, a sum of n terms adds <= n u A whatever the order, and the factor 2
covers the second-order terms: derived, not measured.  When A = 0 (Chamfer of a cloud against itself) the result must be exactly 0.

rot6d_bwd per row.  Error scale s = |g|_inf (kappa^2 / n1 + kappa / n2), kappa = |a2| / n2, n1 = |a1|, n2 = |a2 - (b1.a2) b1| from
the float64 reference: a relative perturbation u of the inputs moves b2 by ~kappa u (the projection cancels), the gradient w.r.t. a2
by ~kappa u |g| / n2 and, through -dot gu - pu a2, the one w.r.t. a1 by ~kappa^2 u |g| / n1.  The bar of a row is ROT6D_C u s with
ROT6D_C = 34: the largest err / (u s) that the numpy fp32 restatement below (one rounding per operation, applied to the fp32
inputs) reaches over every family and seeds 0..9 is 8.3 (measure_rot6d_c(); a row of the mixed-scale family), times 4 for the
device's different association in the cross products and projections, rounded up.  Never measured on the device.
No family goes near the 1e-12 clamp of the norms: below it the definition (F.normalize's eps) and the kernel legitimately differ in
how the clamp meets rounding, and a gradient there carries no information.
"""
import functools

import numpy as np

import exact_inputs as X

U = 2.0 ** -24
C_WARP_ARAP = 8
C_CHAMFER = 2
ROT6D_C = 34
IDEN6 = np.array([1, 0, 0, 0, 1, 0], np.float64)

MUTATIONS = ("ring8", "skip_slot2", "neighbour_R", "scatter_sign", "wrong_T", "hub_drop", "hub_double", "ga_entry0", "skip_last_vertex",
             "no_doth", "recompute_idx", "cross_swapped", "no_identity")


# ----------------------------------------------------------------------------------------------------------------------- checks
def check_equal(name, got, exact):
    """bit for bit (NaN never passes): got fp32, exact float64 whose rounding to fp32 is the expected value"""
    got, ref = np.asarray(got), np.asarray(exact).astype(np.float32)
    assert got.shape == ref.shape and got.dtype == np.float32, (name, got.shape, ref.shape, got.dtype)
    bad = np.flatnonzero(~(got.ravel() == ref.ravel()))
    assert bad.size == 0, "%s: %d of %d elements differ; first at %s: got %r, exact %r" % (
        name, bad.size, ref.size, np.unravel_index(bad[0], ref.shape), float(got.ravel()[bad[0]]), float(ref.ravel()[bad[0]]))


def check_bound(name, got, ref, bound):
    """per element |got - ref| <= bound (NaN never passes)"""
    got, ref, bound = np.asarray(got, np.float64), np.asarray(ref), np.broadcast_to(np.asarray(bound), np.shape(ref))
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    err = np.abs(got - ref)
    bad = np.flatnonzero(~(err.ravel() <= bound.ravel()))
    if bad.size:
        w = bad[np.argmax(np.nan_to_num(err.ravel()[bad] / np.maximum(bound.ravel()[bad], 1e-300), nan=np.inf))]
        raise AssertionError("%s: %d of %d elements outside their bound; worst at %s: got %r, ref %r, |err| %.3e, bound %.3e" % (
            name, bad.size, ref.size, np.unravel_index(w, ref.shape), float(got.ravel()[w]), float(ref.ravel()[w]), float(err.ravel()[w]),
            float(bound.ravel()[w])))


def nonvacuous_fraction(ref, bound):
    """share of the elements whose bound is <= 1e-3 |ref|"""
    return float((np.asarray(bound) <= 1e-3 * np.abs(np.asarray(ref))).mean())


# ------------------------------------------------------------------------------------------- restatements, one rounding per operation
def _dot3(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)


def rot6d_bwd_np(d6, g, dtype=np.float32, mut=None, trace=None):
    """d (sum R * g) / d d6 for R = rows (b1, b2, b1 x b2) of the Gram-Schmidt frame of d6 = (a1, a2); arrays (rows, 6), (rows, 9 | 3, 3).
    trace: a list that receives every intermediate (the CPU half checks that the plantings keep them exact)."""
    d6, g = np.asarray(d6, dtype), np.asarray(g, dtype).reshape(-1, 9)
    t = (lambda x: (trace.append(x), x)[1]) if trace is not None else (lambda x: x)
    eps = dtype(1e-12)
    a1, a2 = d6[:, :3], d6[:, 3:]
    n1 = np.maximum(t(np.sqrt(t(_dot3(a1, a1)))), eps)[:, None]
    b1 = t(a1 / n1)
    dot = t(_dot3(b1, a2))[:, None]
    u = t(a2 - t(dot * b1))
    n2 = np.maximum(t(np.sqrt(t(_dot3(u, u)))), eps)[:, None]
    b2 = t(u / n2)
    gb3 = g[:, 6:]
    gb1 = t(g[:, :3] + t(_cross(b2, gb3)))
    gb2 = t(g[:, 3:6] + t(_cross(b1, gb3) if mut == "cross_swapped" else _cross(gb3, b1)))
    p2 = t(_dot3(gb2, b2))[:, None]
    gu = t(t(gb2 - t(p2 * b2)) / n2)
    pu = t(_dot3(gu, b1))[:, None]
    o2 = t(gu - t(pu * b1))
    gb1 = t(gb1 + t(t(-dot * gu) - t(pu * a2)))
    p1 = t(_dot3(gb1, b1))[:, None]
    o1 = t(t(gb1 - t(p1 * b1)) / n1)
    return np.concatenate([o1, o2], 1)


def def9_bwd_np(def9, dR, dT, dtype=np.float32, mut=None):
    """the Deformer's output row def9 = [t | d6 - identity]: (d_R, d_T) -> d def9 (rows, 9)"""
    def9 = np.asarray(def9, dtype)
    d6 = def9[:, 3:] if mut == "no_identity" else def9[:, 3:] + IDEN6.astype(dtype)
    return np.concatenate([np.asarray(dT, dtype).reshape(-1, 3), rot6d_bwd_np(d6, dR, dtype, mut)], 1)


def _scatter(shape, idx, val, dtype, rng):
    """sequential accumulation in `dtype`, in a shuffled order (the atomics' order is not defined)"""
    idx, val = np.concatenate(idx), np.concatenate(val).astype(dtype)
    order = rng.permutation(idx.size)
    out = np.zeros(shape, dtype)
    np.add.at(out, idx[order], val[order])
    return out


def _tamper(idx, val, mut):
    """hub_drop / hub_double: ONE scalar addend on the most contended address is lost / lands twice"""
    if mut not in ("hub_drop", "hub_double"):
        return
    hub = np.bincount(np.concatenate(idx)).argmax()
    for i, v in zip(idx, val):
        hit = np.flatnonzero((i == hub) & (v.reshape(v.shape[0], -1)[:, 0] != 0))
        if hit.size:
            v.reshape(v.shape[0], -1)[hit[hit.size // 2], 0] *= 0 if mut == "hub_drop" else 2
            return
    raise AssertionError("no addend to tamper with")


def warp_arap_bwd_np(c, dtype=np.float32, rng=None, mut=None, ga=None):
    """dg_warp_bwd_kernel + dg_arap_bwd_kernel for one batch entry c (xyz, nodes_idx, one_ring, infl_idx, weights, R, T, gw, ga)
    -> d_R (Nn,3,3), d_T (Nn,3).  One thread per vertex / per node: the node's own sums go through a local accumulator in ring order,
    everything else is a scattered add."""
    rng = rng if rng is not None else np.random.default_rng(0)
    xyz, w, gw, R, T = (np.asarray(c[k], dtype) for k in ("xyz", "weights", "gw", "R", "T"))
    nodes, ring, infl = np.asarray(c["nodes_idx"]), np.asarray(c["one_ring"]), np.asarray(c["infl_idx"])
    N, Nn = xyz.shape[0], nodes.size
    g = xyz[nodes]
    verts = np.arange(N - 1 if mut == "skip_last_vertex" else N)
    ti, tv, ri, rv_ = [], [], [], []
    for s in ((0, 1) if mut == "skip_slot2" else (0, 1, 2)):
        nb = infl[verts, s]
        d = xyz[verts] - g[nb]
        wg = w[verts, s, None] * gw[verts]
        ti.append(nb), tv.append(wg), ri.append(nb), rv_.append(wg[:, :, None] * d[:, None, :])
    k = dtype(2) * dtype(c["ga"] if ga is None else ga) / dtype(Nn)
    accT, accR = np.zeros((Nn, 3), dtype), np.zeros((Nn, 3, 3), dtype)
    for q in range(8 if mut == "ring8" else ring.shape[1]):
        nb = ring[:, q]
        tb = T[(nb + 1) % Nn] if mut == "wrong_T" else T[nb]
        Ra = R[nb] if mut == "neighbour_R" else R
        d = g - g[nb]
        rv = (Ra[:, :, 0] * d[:, None, 0] + Ra[:, :, 1] * d[:, None, 1]) + Ra[:, :, 2] * d[:, None, 2]
        ge = k * (((g + T) - (g[nb] + tb)) - rv)
        accT = accT + ge
        accR = accR - ge[:, :, None] * d[:, None, :]
        ti.append(nb), tv.append(ge if mut == "scatter_sign" else -ge)
    own = np.arange(Nn)
    ti.append(own), tv.append(accT), ri.append(own), rv_.append(accR)
    tv, rv_ = [v.copy() for v in tv], [v.copy() for v in rv_]
    if mut == "hub_drop":
        _tamper(ti, tv, mut)
    if mut == "hub_double":
        _tamper(ri, rv_, mut)
    return _scatter((Nn, 3, 3), ri, rv_, dtype, rng), _scatter((Nn, 3), ti, tv, dtype, rng)


def warp_arap_bwd_batch_np(cases, dtype=np.float32, seed=0, mut=None):
    """the batch: g_arap is read per entry (ga_entry0: entry 0's value for all)"""
    rng = np.random.default_rng([seed, 31])
    out = [warp_arap_bwd_np(c, dtype, rng, mut, ga=cases[0]["ga"] if mut == "ga_entry0" else None) for c in cases]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def chamfer_bwd_np(c, dtype=np.float32, rng=None, mut=None):
    """chamfer_bwd_kernel for one batch entry c (a, b, i1, i2, g1, g2) -> d_a, d_b"""
    rng = rng if rng is not None else np.random.default_rng(0)
    a, b, g1, g2 = (np.asarray(c[k], dtype) for k in ("a", "b", "g1", "g2"))
    i1, i2 = np.asarray(c["i1"]), np.asarray(c["i2"])
    if mut == "recompute_idx":
        D = ((a.astype(np.float64)[:, None] - b.astype(np.float64)[None]) ** 2).sum(-1)
        i1, i2 = D.argmin(1), D.argmin(0)
    va, vb = (dtype(2) * g1)[:, None] * (a - b[i1]), (dtype(2) * g2)[:, None] * (b - a[i2])
    ia, ib = np.arange(a.shape[0]), np.arange(b.shape[0])
    if mut == "no_doth":
        return _scatter(a.shape, [ia], [va], dtype, rng), _scatter(b.shape, [ib], [vb], dtype, rng)
    return _scatter(a.shape, [ia, i2], [va, -vb], dtype, rng), _scatter(b.shape, [ib, i1], [vb, -va], dtype, rng)


def chamfer_bwd_batch_np(cases, dtype=np.float32, seed=0, mut=None):
    rng = np.random.default_rng([seed, 32])
    out = [chamfer_bwd_np(c, dtype, rng, mut) for c in cases]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def criterion_bwd_np(refs, g_arap, dtype=np.float32, seed=0, mut=None):
    """ARAP backward -> def9 backward -> the last decoder layer's bias / weight gradients (column sums in a shuffled order) for the planted
    pairs `refs` (exact_inputs.reference_direction) -> db3 (9,), dW3[:, :3] (9,3)"""
    rng = np.random.default_rng([seed, 33])
    rows, hs = [], []
    for r, ga in zip(refs, g_arap if mut != "ga_entry0" else [g_arap[0]] * len(refs)):
        Nn = r["Nn"]
        zero = np.zeros((Nn, 3), np.float32)
        c = dict(xyz=r["g"], nodes_idx=np.arange(Nn), one_ring=r["graph"]["one_ring"], infl_idx=zero.astype(np.int64), weights=zero, R=r["R"], T=r["T"],
                 gw=zero, ga=ga)
        dR, dT = warp_arap_bwd_np(c, dtype, rng, mut)
        rows.append(def9_bwd_np(r["def9"], dR, dT, dtype, mut))
        hs.append(np.asarray(r["g"], dtype))
    D, H = np.concatenate(rows), np.concatenate(hs)
    order = rng.permutation(D.shape[0])
    db3, dW3 = np.zeros(9, dtype), np.zeros((9, 3), dtype)
    for r in order:
        db3 = db3 + D[r]
        dW3 = dW3 + D[r][:, None] * H[r][None, :]
    return db3, dW3


# --------------------------------------------------------------------------------------------- float64 references with their bounds
def warp_arap_reference(cases):
    """-> dict(d_R (B,Nn,3,3), d_T (B,Nn,3) float64 by autograd of oracle/torch_ref.py, bound_R, bound_T = 2 u (n + c) A)"""
    import torch
    from oracle import torch_ref as TR
    st = lambda k, dt: torch.from_numpy(np.stack([np.asarray(c[k]) for c in cases]).astype(dt))  # noqa: E731
    R, T = st("R", np.float64).requires_grad_(True), st("T", np.float64).requires_grad_(True)
    g = dict(nodes_idx=st("nodes_idx", np.int64), one_ring=st("one_ring", np.int64), infl_idx=st("infl_idx", np.int64), weights=st("weights", np.float64))
    warped, arap = TR.dg_warp_arap(st("xyz", np.float64), g, R, T)
    ((warped * st("gw", np.float64)).sum() + (arap * st("ga", np.float64)).sum()).backward()
    out = dict(d_R=R.grad.numpy(), d_T=T.grad.numpy(), bound_R=[], bound_T=[])
    for c in cases:
        xyz, w, gw, Rm, Tm = (np.abs(np.asarray(c[k], np.float64)) for k in ("xyz", "weights", "gw", "R", "T"))
        nodes, ring, infl = np.asarray(c["nodes_idx"]), np.asarray(c["one_ring"]), np.asarray(c["infl_idx"])
        Nn, K = nodes.size, ring.shape[1]
        x64 = np.asarray(c["xyz"], np.float64)
        gpos = x64[nodes]
        wg = w[:, :, None] * gw[:, None, :]
        wgd = wg[..., None] * np.abs(x64[:, None] - gpos[infl])[:, :, None, :]
        k = abs(2.0 * float(c["ga"]) / Nn)
        df = np.abs(gpos[:, None] - gpos[ring])
        m = (np.abs(gpos) + Tm)[:, None] + (np.abs(gpos) + Tm)[ring] + np.einsum("aij,aqj->aqi", Rm, df)
        km = k * m
        own = np.broadcast_to(np.arange(Nn)[:, None], ring.shape).ravel()
        AT, _ = X.scatter_sum((Nn, 3), np.concatenate([infl.ravel(), own, ring.ravel()]), np.concatenate([wg.reshape(-1, 3), km.reshape(-1, 3), km.reshape(-1, 3)]))
        AR, _ = X.scatter_sum((Nn, 3, 3), np.concatenate([infl.ravel(), own]),
                              np.concatenate([wgd.reshape(-1, 3, 3), (km[..., None] * df[:, :, None, :]).reshape(-1, 3, 3)]))
        n_infl = np.bincount(infl.ravel(), minlength=Nn)
        nT, nR = n_infl + K + np.bincount(ring.ravel(), minlength=Nn), n_infl + K
        out["bound_T"].append(2 * U * (nT + C_WARP_ARAP)[:, None] * AT)
        out["bound_R"].append(2 * U * (nR + C_WARP_ARAP)[:, None, None] * AR)
    out["bound_T"], out["bound_R"] = np.stack(out["bound_T"]), np.stack(out["bound_R"])
    return out


def chamfer_reference(cases):
    """-> dict(d_a, d_b float64 with the cases' index lists held fixed, bound_a, bound_b = 2 u (n + c) A)"""
    out = dict(d_a=[], d_b=[], bound_a=[], bound_b=[])
    for c in cases:
        r = X.chamfer_bwd_rows(c["a"], c["b"], c["i1"], c["i2"], c["g1"], c["g2"])
        N, M = np.asarray(c["a"]).shape[0], np.asarray(c["b"]).shape[0]
        na, nb = 1 + np.bincount(np.asarray(c["i2"]), minlength=N), 1 + np.bincount(np.asarray(c["i1"]), minlength=M)
        out["d_a"].append(r["d_a"]), out["d_b"].append(r["d_b"])
        out["bound_a"].append(2 * U * (na + C_CHAMFER)[:, None] * r["mag_a"])
        out["bound_b"].append(2 * U * (nb + C_CHAMFER)[:, None] * r["mag_b"])
    return {k: np.stack(v) for k, v in out.items()}


def rot6d_reference(d6, gR):
    """-> (gradient (rows,6) float64, bar (rows,1) = ROT6D_C u s)"""
    d6, gR = np.asarray(d6, np.float64), np.asarray(gR, np.float64).reshape(-1, 9)
    a1, a2 = d6[:, :3], d6[:, 3:]
    n1 = np.sqrt((a1 * a1).sum(1))
    b1 = a1 / n1[:, None]
    u = a2 - (b1 * a2).sum(1, keepdims=True) * b1
    n2 = np.sqrt((u * u).sum(1))
    kappa = np.sqrt((a2 * a2).sum(1)) / n2
    s = np.abs(gR).max(1) * (kappa ** 2 / n1 + kappa / n2)
    return X.rot6d_grad64(d6, gR), (ROT6D_C * U * s)[:, None]


# --------------------------------------------------------------------------------------------------------------- the hard families
WARP_FAMILIES = ("device_uniform", "device_duplicates", "hub", "orphans", "rigid", "translated", "mixed_g")
WARP_SIZES = (64, 257, 600, 2048)
VACUITY_EXEMPT = ("rigid", "self")
REAL_SEED = 8100


def _frames(rng, n, sigma=0.3):
    """near-identity rotations: the float64 Gram-Schmidt frame of identity + sigma * noise"""
    d6 = IDEN6 + sigma * rng.standard_normal((n, 6))
    b1 = d6[:, :3] / np.linalg.norm(d6[:, :3], axis=1, keepdims=True)
    u = d6[:, 3:] - (b1 * d6[:, 3:]).sum(1, keepdims=True) * b1
    b2 = u / np.linalg.norm(u, axis=1, keepdims=True)
    return np.stack([b1, b2, np.cross(b1, b2)], 1)


def duplicates_cloud(n, rng):
    """tests/test_gpu_grid_search.py's `_duplicates`: the second half of the cloud repeats points of the first (zero offsets)"""
    x = rng.random((n, 3))
    h = n // 2
    x[h:] = x[rng.integers(0, h, n - h)]
    return x


def warp_family_entry(family, N, b, dg_build=None):
    """One batch entry of a real-valued family (module docstring of the GPU test lists them).  dg_build(xyz fp32 (N,3), start) -> graph
    dict, for the device_* families: the device's own build on the GPU, the oracle's in the CPU half."""
    rng = np.random.default_rng([REAL_SEED, WARP_FAMILIES.index(family), N, b])
    Nn = N // 2
    xyz = (duplicates_cloud(N, rng) if family == "device_duplicates" else rng.random((N, 3)))
    if family == "translated":
        xyz = xyz + np.array([1e3, -7e2, 4e2])
    xyz = xyz.astype(np.float32)
    if family.startswith("device"):
        gr = dg_build(xyz, int(rng.integers(0, N)))
        nodes, ring, infl, w = (np.asarray(gr[k]) for k in ("nodes_idx", "one_ring", "infl_idx", "weights"))
    else:
        nodes = rng.choice(N, size=Nn, replace=False).astype(np.int32)
        live = max(Nn // 2, 1) if family == "orphans" else Nn         # orphans: nodes live.. are in no infl row and in no other node's ring
        ring = rng.integers(0, live, (Nn, 9)).astype(np.int32)
        infl = rng.integers(0, live, (N, 3)).astype(np.int32)
        if family == "hub":
            infl[:, 0] = infl[:, 2] = 0
            ring[:, 0] = Nn // 2
            ring[:, 8] = np.arange(Nn)
        w = rng.random((N, 3)) + 0.05
        w = (w / w.sum(1, keepdims=True)).astype(np.float32)
    R, T = _frames(rng, Nn), 0.05 * rng.standard_normal((Nn, 3))
    if family == "rigid":
        Q, t = _frames(rng, 1, 0.8)[0], rng.standard_normal(3)
        g = xyz.astype(np.float64)[nodes]
        R, T = np.broadcast_to(Q, (Nn, 3, 3)), g @ Q.T + t - g
    gw = rng.standard_normal((N, 3))
    ga = (1.3, -0.7, 0.4)[b % 3]
    if family == "mixed_g":
        gw = gw * 10.0 ** rng.uniform(-6, 3, (N, 1))
        ga = (0.0, -2.5, 1.7)[b % 3]
    if family == "translated":
        ga = ga * 0.01            # the loss weight of ARAP in training (w_arap = 0.01); the envelope of its residual is ~1e3 here
    return dict(xyz=xyz, nodes_idx=nodes.astype(np.int32), one_ring=ring.astype(np.int32), infl_idx=infl.astype(np.int32), weights=w.astype(np.float32),
                R=np.ascontiguousarray(R, np.float32), T=T.astype(np.float32), gw=gw.astype(np.float32), ga=np.float32(ga))


def warp_family(family, N, dg_build=None, B=3):
    cases = [warp_family_entry(family, N, b, dg_build) for b in range(B)]
    return cases, warp_arap_reference(cases)


CHAMFER_FAMILIES = ("nn", "hub", "arbitrary", "self")


def chamfer_family(family, N, M, nn=None, B=3):
    """real clouds in [0,1)^3, g1 / g2 normal.  nn(a, b) -> (i1, i2): the true nearest neighbours from the forward under test (device) or
    the oracle (CPU half); self: b = a with the identity map (N == M), every gradient exactly 0."""
    cases = []
    for b in range(B):
        rng = np.random.default_rng([REAL_SEED, 50 + CHAMFER_FAMILIES.index(family), N, M, b])
        a, bb = rng.random((N, 3)).astype(np.float32), rng.random((M, 3)).astype(np.float32)
        g1, g2 = rng.standard_normal(N).astype(np.float32), rng.standard_normal(M).astype(np.float32)
        if family == "nn":
            i1, i2 = nn(a, bb)
        elif family == "hub":
            i1, i2 = np.full(N, rng.integers(0, M)), np.full(M, rng.integers(0, N))
        elif family == "arbitrary":
            i1, i2 = rng.integers(0, M, N), rng.integers(0, N, M)
        else:
            assert N == M
            bb, i1, i2 = a.copy(), np.arange(N), np.arange(N)
        cases.append(dict(a=a, b=bb, g1=g1, g2=g2, i1=np.asarray(i1, np.int32), i2=np.asarray(i2, np.int32)))
    return cases, chamfer_reference(cases)


ROT6D_FAMILIES = ("near_identity", "scaled_1e-4", "scaled_1e4", "mixed_scale", "parallel_1e-1", "parallel_1e-2", "parallel_1e-3", "zero_component")
ROT6D_ROWS = 300


def rot6d_family(family, seed=0, rows=ROT6D_ROWS):
    """-> d6 (rows,6), gR (rows,3,3) fp32"""
    rng = np.random.default_rng([REAL_SEED, 70 + ROT6D_FAMILIES.index(family), seed])
    d6 = IDEN6 + 0.3 * rng.standard_normal((rows, 6))
    if family.startswith("scaled"):
        d6 = d6 * float(family.split("_")[1])
    elif family == "mixed_scale":
        d6 = d6 * np.array([1e-3] * 3 + [1e2] * 3)
    elif family.startswith("parallel"):
        a1 = d6[:, :3]
        perp = np.cross(a1, rng.standard_normal((rows, 3)))
        perp = perp / np.linalg.norm(perp, axis=1, keepdims=True) * np.linalg.norm(a1, axis=1, keepdims=True)
        d6[:, 3:] = a1 * rng.uniform(0.5, 2.0, (rows, 1)) * rng.choice([-1.0, 1.0], (rows, 1)) + float(family.split("_")[1]) * perp
    elif family == "zero_component":
        d6[np.arange(rows), rng.integers(0, 6, rows)] = 0.0
    return d6.astype(np.float32), rng.standard_normal((rows, 3, 3)).astype(np.float32)


def measure_rot6d_c(seeds=range(10)):
    """how ROT6D_C was obtained: max over families and seeds of the fp32 restatement's err / (u s)"""
    worst = (0.0, None)
    for fam in ROT6D_FAMILIES:
        for seed in seeds:
            d6, gR = rot6d_family(fam, seed)
            ref, bar = rot6d_reference(d6, gR)
            r = float((np.abs(rot6d_bwd_np(d6, gR).astype(np.float64) - ref) / (bar / ROT6D_C)).max())
            worst = max(worst, (r, fam))
    return worst


@functools.lru_cache(maxsize=None)
def rot6d_case(family):
    d6, gR = rot6d_family(family)
    return (d6, gR) + rot6d_reference(d6, gR)
