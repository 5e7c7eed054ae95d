"""Planted inputs on which every fp32 operation of the loss scalars is exact, and their rational reference.

The pair path's losses[B,6] and the training criterion's terms are sums over thousands of rows.  On inputs whose every
intermediate is exactly representable in fp32 — small integer coordinates, dyadic correspondence weights, rotations with
entries 0 / +-1 — neither the summation order nor FMA contraction can move a bit: the device value must equal the definition
evaluated on integers, rounded to float32 once where the kernels round ((float)(sum / n) for the means and ARAP,
(float)sum for the map term).  A missing, doubled or misindexed row then moves the result by many float32 ulps.

Everything here is float64 arithmetic on values that are integers or multiples of 1/64 well below 2^53: exact, whatever the
order.  Index lists (FPS nodes, rings, xyz kNN) come from the CPU oracle; the device's tie contract ("lowest index") is pinned
against it on lattice clouds by tests/test_gpu_grid_search.py.  All randomness is seeded.

Planting of one pair (one batch element):
  clouds    distinct integer points in [0, 255]^3 (fp32);
  features  128-d; rows carry the code 8.0 * bit_b(g + 1) of their group g in 16 channels, so rows of different groups are at
            least 8 apart and rows of one group are identical.  With alpha = 20 every non-matching exp underflows to 0 and the
            matching ones are 1: a source row's top-10 weights are exactly 1 / size on the columns of its group (ascending),
            0 elsewhere.  The targets' groups have 1, 2, 4 or 8 rows.
            one-way planting (both=False): the targets' groups are scattered by a permutation, each source row copies the code
            of a randomly chosen group (hubs included): exact for the direction source -> target only;
            mirrored planting (both=True): every group has 1, 2, 4 or 8 rows in EACH cloud: exact in both directions;
  Deformer  pooling conv zero; W0..W3 zero except a unit diagonal on channels 0..2; b3[3:9] = [-1, 1, 0, -1, -1, 0]:
            def9 = [verts1[node], -1, 1, 0, -1, -1, 0], i.e. T_a = g_a and R = the 90 degree rotation about z, exactly.
"""
import functools
import itertools

import numpy as np

ALPHA = 20.0
GROUP_SIZES = (1, 2, 4, 8)
K_XYZ = 10
TOPK = 10
DEF9_TAIL = np.array([-1, 1, 0, -1, -1, 0], np.float64)
# rotation_6d_to_matrix([1, 0, 0, 0, 1, 0] + DEF9_TAIL): rows b1 = (0, 1, 0), b2 = (-1, 0, 0), b3 = b1 x b2 = (0, 0, 1)
R_PLANTED = np.array([[0, 1, 0], [-1, 0, 0], [0, 0, 1]], np.float64)


def f32(x):
    """the one rounding of a kernel's final store: double -> float"""
    return np.float32(np.float64(x))


def ulp_distance(a, b):
    """distance in float32 ulps between two finite floats of one sign"""
    ia = np.asarray(a, np.float32).view(np.int32).astype(np.int64)
    ib = np.asarray(b, np.float32).view(np.int32).astype(np.int64)
    return np.abs(ia - ib)


# ---------------------------------------------------------------------------------------------------------------- planting
def lattice_cloud(rng, n, hi=255):
    """n DISTINCT integer points in [0, hi]^3, fp32, in random order"""
    side = hi + 1
    code = np.empty(0, np.int64)
    while code.size < n:
        code = np.unique(np.concatenate([code, rng.integers(0, side ** 3, size=2 * n)]))
    code = rng.permutation(code)[:n]
    return np.stack([code // (side * side), (code // side) % side, code % side], 1).astype(np.float32)


def partition_sizes(rng, total, groups):
    """`groups` sizes from GROUP_SIZES that add up to `total`"""
    assert groups <= total <= 8 * groups, (total, groups)
    for _ in range(200):
        add = np.zeros(groups, np.int64)
        left = total - groups
        for g in rng.permutation(groups):
            if left == 0:
                break
            a = int(rng.choice([a for a in (0, 1, 3, 7) if a <= left]))
            add[g] = a
            left -= a
        singles = np.flatnonzero(add == 0)
        if left <= singles.size:
            add[singles[:left]] = 1
            return 1 + add
    raise AssertionError("no partition of %d into %d groups" % (total, groups))


def deformer_weights():
    """state dict (reference keys) of the pass-through Deformer of the module docstring"""
    w = {"conv_layer.weight": np.zeros((1, K_XYZ, 1, 1), np.float32), "conv_layer.bias": np.zeros(1, np.float32)}
    dims = [(512, 262), (256, 512), (128, 256), (9, 128)]
    for li, (o, i) in zip((0, 2, 4, 6), dims):
        W = np.zeros((o, i), np.float32)
        W[0, 0] = W[1, 1] = W[2, 2] = 1.0
        w["deformation_decoder_layer.linear.%d.weight" % li] = W
        w["deformation_decoder_layer.linear.%d.bias" % li] = np.zeros(o, np.float32)
    w["deformation_decoder_layer.linear.6.bias"][3:9] = DEF9_TAIL
    return w


def _features(grp, chans):
    f = np.zeros((grp.size, 128), np.float32)
    code = grp.astype(np.int64) + 1
    for b, c in enumerate(chans):
        f[:, c] = 8.0 * ((code >> b) & 1)
    return f


def plant_pair(N, M, seed, both=False, hi=255):
    """One planted pair: dict(verts1 (N,3), verts2 (M,3), feat1 (N,128), feat2 (M,128), grp1 (N,), grp2 (M,), start1, start2).
    hi: the clouds' coordinate range [0, hi] (the backward plantings need small residuals: criterion_bwd_reference)."""
    rng = np.random.default_rng([seed, N, M, int(both)])
    verts1, verts2 = lattice_cloud(rng, N, hi), lattice_cloud(rng, M, hi)
    if both:
        G = min(min(N, M), max(-(-max(N, M) // 3), min(N, M) // 2))
        n1, n2 = partition_sizes(rng, N, G), partition_sizes(rng, M, G)
        grp1 = rng.permutation(np.repeat(np.arange(G), n1))
        grp2 = rng.permutation(np.repeat(np.arange(G), n2))
    else:
        G = -(-2 * M // 5)
        grp2 = rng.permutation(np.repeat(np.arange(G), partition_sizes(rng, M, G)))
        grp1 = rng.integers(0, G, size=N)
    assert G + 1 < 1 << 16
    chans = np.sort(rng.choice(128, size=16, replace=False))
    return dict(N=N, M=M, verts1=verts1, verts2=verts2, feat1=_features(grp1, chans), feat2=_features(grp2, chans), grp1=grp1, grp2=grp2,
                start1=int(rng.integers(0, N)), start2=int(rng.integers(0, M)))


# ------------------------------------------------------------------------------------------- the definitions, per row, exact
def map_rows(verts12, verts2, idx11, idx22, pidx, pval):
    """(N, k): sum_c (verts12[idx11[i, s], c] - sum_t pval[i, t] * verts2[idx22[pidx[i, t], s], c])^2   (models/loss.py:1232-1238)"""
    v12, v2 = np.asarray(verts12, np.float64), np.asarray(verts2, np.float64)
    acc = np.einsum("nt,ntkc->nkc", np.asarray(pval, np.float64), v2[np.asarray(idx22)[np.asarray(pidx)]])
    e = v12[np.asarray(idx11)] - acc
    return (e * e).sum(-1)


def arap_rows(g, R, T, ring):
    """(Nn, K): |(g_a + t_a) - (g_b + t_b) - R_a (g_a - g_b)|^2, b = ring[a, q]   (lib/deformation_graph_point.py:233-261)"""
    g, R, T = np.asarray(g, np.float64), np.asarray(R, np.float64), np.asarray(T, np.float64)
    ring = np.asarray(ring)
    df = g[:, None] - g[ring]
    rv = np.einsum("aij,aqj->aqi", R, df)
    e = (g + T)[:, None] - (g + T)[ring] - rv
    return (e * e).sum(-1)


def sr_rows(R, ring):
    R = np.asarray(R, np.float64)
    e = R[:, None] - R[np.asarray(ring)]
    return (e * e).sum((-1, -2))


def warp_rows(xyz, nodes_idx, infl, weights, R, T):
    """(N, 3): sum_s w_s (R_s (v - g_s) + g_s + t_s)"""
    xyz, R, T, w = np.asarray(xyz, np.float64), np.asarray(R, np.float64), np.asarray(T, np.float64), np.asarray(weights, np.float64)
    infl = np.asarray(infl)
    g = xyz[np.asarray(nodes_idx)][infl]                        # (N, 3, 3)
    rv = np.einsum("nsij,nsj->nsi", R[infl], xyz[:, None] - g)
    return ((rv + g + T[infl]) * w[..., None]).sum(1)


def chamfer_rows(a, b):
    """squared nearest-neighbour distances both ways, brute force"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    d = np.zeros((a.shape[0], b.shape[0]))
    for c in range(3):
        d += (a[:, None, c] - b[None, :, c]) ** 2
    return d.min(1), d.min(0)


def planted_correspondence(grp_s, grp_t):
    """pidx (N, 10) int64, pval (N, 10) float64: the group's columns in ascending order at weight 1 / size; the remaining slots
    (whatever column the device puts there) weigh exactly 0 — here: the group's first column."""
    order = np.argsort(grp_t, kind="stable")
    counts = np.bincount(grp_t, minlength=int(max(grp_s.max(), grp_t.max())) + 1)
    first = np.concatenate([[0], np.cumsum(counts)[:-1]])
    n = counts[grp_s]
    assert np.isin(n, GROUP_SIZES).all(), "a source row's group has no valid target group"
    slot = np.arange(TOPK)[None]
    pidx = order[first[grp_s][:, None] + np.where(slot < n[:, None], slot, 0)]
    pval = np.where(slot < n[:, None], 1.0 / n[:, None], 0.0)
    return pidx, pval


def reference_direction(verts_s, verts_t, grp_s, grp_t, start):
    """The exact value of everything one direction (sources -> targets) computes from a planted pair, with the per-row tables."""
    from oracle import oracle as O
    N, M = verts_s.shape[0], verts_t.shape[0]
    Nn = N // 2
    pidx, pval = planted_correspondence(grp_s, grp_t)
    verts12 = np.einsum("nt,ntc->nc", pval, verts_t.astype(np.float64)[pidx])
    graph = O.dg_build(verts_s, start)
    idx11, idx22 = O.knn_cdist(verts_s, verts_s, K_XYZ), O.knn_cdist(verts_t, verts_t, K_XYZ)
    g = verts_s.astype(np.float64)[graph["nodes_idx"]]
    def9 = np.concatenate([g, np.broadcast_to(DEF9_TAIL, (Nn, 6))], 1)
    R, T = np.broadcast_to(R_PLANTED, (Nn, 3, 3)).copy(), g.copy()
    rows = dict(map=map_rows(verts12, verts_t, idx11, idx22, pidx, pval), arap=arap_rows(g, R, T, graph["one_ring"]))
    rows["d1"], rows["d2"] = chamfer_rows(verts12, verts_t)
    ref = dict(N=N, M=M, Nn=Nn, pidx=pidx, pval=pval, T12=pidx[:, 0].astype(np.int32), verts12=verts12, graph=graph, idx11=idx11,
               idx22=idx22, g=g, def9=def9, R=R, T=T, rows=rows)
    ref["losses"] = {2: f32(rows["arap"].sum() / Nn), 3: f32(rows["d1"].sum() / N), 4: f32(rows["d2"].sum() / M), 5: f32(rows["map"].sum())}
    assert np.array_equal(verts12.astype(np.float32), verts12)
    return ref


@functools.lru_cache(maxsize=None)
def planted_case(N, M, seed, both=False, hi=255):
    """-> (pair, ref12, ref21): ref21 (cloud 2 -> cloud 1) only for the mirrored planting, else None.  Shared, never modified."""
    p = plant_pair(N, M, seed, both, hi)
    r12 = reference_direction(p["verts1"], p["verts2"], p["grp1"], p["grp2"], p["start1"])
    r21 = reference_direction(p["verts2"], p["verts1"], p["grp2"], p["grp1"], p["start2"]) if both else None
    return p, r12, r21


def reference_arap(verts, start):
    """ARAP alone (it does not depend on the correspondence): the unplanted direction of a one-way planting"""
    from oracle import oracle as O
    graph = O.dg_build(verts, start)
    g = verts.astype(np.float64)[graph["nodes_idx"]]
    Nn = g.shape[0]
    return f32(arap_rows(g, np.broadcast_to(R_PLANTED, (Nn, 3, 3)), g, graph["one_ring"]).sum() / Nn)


def planted_batch(N, M, seed, B=3, both=False, hi=255):
    """B different planted pairs (seeds seed .. seed + B - 1) -> (stacked arrays, [(pair, ref12, ref21)])"""
    cases = [planted_case(N, M, seed + b, both, hi) for b in range(B)]
    arrays = {k: np.stack([c[0][k] for c in cases]) for k in ("verts1", "verts2", "feat1", "feat2")}
    arrays["start1"] = np.array([c[0]["start1"] for c in cases], np.int32)
    arrays["start2"] = np.array([c[0]["start2"] for c in cases], np.int32)
    return arrays, cases


# shapes (N, M) of the planted pair-path cases; tests/test_gpu_loss_scalars_exact.py says which kernel form each one reaches
PAIR_SHAPES = [(64, 65), (65, 64), (1024, 1025), (1025, 1024), (300, 170), (300, 2700), (2700, 300), (5200, 64)]
MIRRORED_SHAPES = [(64, 65), (1024, 1025), (300, 170)]       # ops.pair_forward, both directions exact in one launch
MIRRORED_NOMAP_SHAPES = [(65, 64), (170, 300)]               # the same with with_map=False
SWAPPED_SIZES = [64, 300, 1028]                              # ops.criterion_train_forward (N == M, N % 4 == 0)
PAIR_SEED = 4100


# ------------------------------------------------------------------------------------- richer planting for the direct entries
def map_term_direct(N, M, k, topk, seed):
    """ops.map_term: non-zero dyadic weights {1/2, 1/4} in every slot, integer coordinates in [0, 31] (every intermediate within
    24 bits: |acc| <= 16 * 31 / 2 with 2 fractional bits, e^2 < 2^17 with 4), random columns with repeats inside a row, random
    neighbour lists with self-entries and repeats."""
    rng = np.random.default_rng([seed, N, M, k, topk])
    d = dict(verts12=rng.integers(0, 32, (N, 3)).astype(np.float32), verts2=rng.integers(0, 32, (M, 3)).astype(np.float32),
             idx11=rng.integers(0, N, (N, k)).astype(np.int32), idx22=rng.integers(0, M, (M, k)).astype(np.int32),
             pidx=rng.integers(0, M, (N, topk)).astype(np.int32), pval=rng.choice([0.5, 0.25], (N, topk)).astype(np.float32))
    d["idx11"][::3, 0] = np.arange(N)[::3]                      # self
    d["idx22"][::2, 0] = np.arange(M)[::2]
    if k > 1:
        d["idx11"][1::4, k - 1] = d["idx11"][1::4, 0]           # repeats
    if topk > 1:
        d["pidx"][::2, topk - 1] = d["pidx"][::2, 0]            # a column twice in a row
    d["rows"] = map_rows(d["verts12"], d["verts2"], d["idx11"], d["idx22"], d["pidx"], d["pval"])
    d["value"] = f32(d["rows"].sum())
    return d


def _axis_aligned_rotations():
    """the 24 signed permutation matrices of determinant +1"""
    out = []
    for p in itertools.permutations(range(3)):
        for s in itertools.product((1.0, -1.0), repeat=3):
            m = np.eye(3)[list(p)] * np.array(s)[:, None]
            if np.linalg.det(m) > 0:
                out.append(m)
    return np.array(out)


ROTATIONS = _axis_aligned_rotations()
assert ROTATIONS.shape == (24, 3, 3)


def warp_direct(N, Nn, K, seed):
    """ops.dg_warp_arap / ops.dg_warp_arap_graph: per-node R from the 24 axis-aligned rotations, integer T, skinning weights
    (1/2, 1/4, 1/4) permuted per row, random valid infl / ring with self-entries, integer cloud in [0, 63]."""
    rng = np.random.default_rng([seed, N, Nn, K])
    xyz = rng.integers(0, 64, (N, 3)).astype(np.float32)
    nodes = rng.choice(N, size=Nn, replace=False).astype(np.int32)
    ring = rng.integers(0, Nn, (Nn, K)).astype(np.int32)
    ring[::2, 0] = np.arange(Nn)[::2]
    infl = rng.integers(0, Nn, (N, 3)).astype(np.int32)
    weights = rng.permuted(np.tile(np.array([0.5, 0.25, 0.25], np.float32), (N, 1)), axis=1)
    R = ROTATIONS[rng.integers(0, 24, Nn)].astype(np.float32)
    T = rng.integers(-32, 33, (Nn, 3)).astype(np.float32)
    d = dict(xyz=xyz, nodes_idx=nodes, one_ring=ring, infl_idx=infl, weights=weights, R=R, T=T)
    d["warped"] = warp_rows(xyz, nodes, infl, weights, R, T)
    d["arap_rows"], d["sr_rows"] = arap_rows(xyz[nodes], R, T, ring), sr_rows(R, ring)
    d["arap"], d["sr"] = f32(d["arap_rows"].sum() / Nn), f32(d["sr_rows"].sum() / (float(Nn) * K * 9.0))
    return d


# --------------------------------------------------------------------- backward plantings: exact gradients, no tolerance either
# The geometric backward kernels (csrc/dvm_loss_bwd.hip) scatter-add products of their inputs.  On the plantings below every
# addend is a multiple of 2^-4 and, per output element, the MAGNITUDES of its addends sum to less than 2^20: every partial sum, in
# any order and any grouping (atomics, per-thread accumulators), is then a multiple of 2^-4 below 2^20, i.e. at most 24 significant
# bits — exact in fp32.  exact_sums() is that condition; the CPU half (tests/test_geom_backward_rows_cpu.py) asserts it for every case.
SUM_GRID = 16.0
SUM_LIMIT = float(1 << 24)


def exact_sums(addends, mags):
    """every addend * 2^4 is an integer and every element's summed magnitudes * 2^4 stay below 2^24"""
    return all(np.array_equal(np.asarray(a) * SUM_GRID, np.rint(np.asarray(a) * SUM_GRID)) for a in addends) and \
        all((np.asarray(m) * SUM_GRID < SUM_LIMIT).all() for m in mags)


def scatter_sum(shape, idx, val):
    """(sum, sum of magnitudes) of the addends val[l] landing on rows idx[l] of a zero array (float64)"""
    out, mag = np.zeros(shape), np.zeros(shape)
    np.add.at(out, idx, val)
    np.add.at(mag, idx, np.abs(val))
    return out, mag


def warp_arap_bwd_rows(xyz, nodes_idx, ring, infl, weights, R, T, gw, g_arap):
    """The definition's gradient in float64: L = sum(warped * gw) + g_arap * arap (warp_rows, arap_rows / Nn) w.r.t. R and T:
      d_T[s] += w gw_i, d_R[s] += w gw_i (v_i - g_s)^T for the three slots s of vertex i;
      with e = (g_a + t_a) - (g_b + t_b) - R_a (g_a - g_b), k = 2 g_arap / Nn:  d_T[a] += k e, d_T[b] -= k e, d_R[a] -= k e (g_a - g_b)^T.
    -> dict(d_R (Nn,3,3), d_T (Nn,3), mag_R, mag_T (summed magnitudes of the addends), addends)"""
    xyz, R, T, w, gw = (np.asarray(x, np.float64) for x in (xyz, R, T, weights, gw))
    nodes_idx, ring, infl = np.asarray(nodes_idx), np.asarray(ring), np.asarray(infl)
    Nn = nodes_idx.size
    g = xyz[nodes_idx]
    wg = w[:, :, None] * gw[:, None, :]                                              # (N, 3, c)
    wgd = wg[..., None] * (xyz[:, None] - g[infl])[:, :, None, :]                     # (N, 3, c, e)
    k = 2.0 * float(g_arap) / Nn
    df = g[:, None] - g[ring]
    ge = k * ((g + T)[:, None] - (g + T)[ring] - np.einsum("aij,aqj->aqi", R, df))   # (Nn, K, c)
    ged = ge[..., None] * df[:, :, None, :]                                           # (Nn, K, c, e)
    own = np.broadcast_to(np.arange(Nn)[:, None], ring.shape).ravel()
    dT, mT = scatter_sum((Nn, 3), np.concatenate([infl.ravel(), own, ring.ravel()]),
                         np.concatenate([wg.reshape(-1, 3), ge.reshape(-1, 3), -ge.reshape(-1, 3)]))
    dR, mR = scatter_sum((Nn, 3, 3), np.concatenate([infl.ravel(), own]), np.concatenate([wgd.reshape(-1, 3, 3), -ged.reshape(-1, 3, 3)]))
    return dict(d_R=dR, d_T=dT, mag_R=mR, mag_T=mT, addends=(wg, wgd, ge, ged))


def warp_bwd_direct(N, seed, hub=False, sign=1):
    """ops.dg_warp_arap_bwd: warp_direct's graph at Nn = N // 2, K = 9, plus integer gw in [-8, 8] and g_arap = sign * Nn / 8
    (sign in {1, -1, 0}): 2 g_arap / Nn is exactly +-1/4 or 0 whatever Nn.  hub: slots 0 and 2 of EVERY row point at node 0 (in-degree
    2 N, two addends per vertex on one address), ring column 0 at node Nn // 2 (Nn contended -ge scatters), ring column 8 at the node
    itself (an exactly-zero residual)."""
    Nn = N // 2
    d = {k: v for k, v in warp_direct(N, Nn, 9, seed).items() if k in ("xyz", "nodes_idx", "one_ring", "infl_idx", "weights", "R", "T")}
    rng = np.random.default_rng([seed, N, 9, 77, int(hub)])
    if hub:
        d["one_ring"], d["infl_idx"] = d["one_ring"].copy(), d["infl_idx"].copy()
        d["infl_idx"][:, 0] = d["infl_idx"][:, 2] = 0
        d["one_ring"][:, 0] = Nn // 2
        d["one_ring"][:, 8] = np.arange(Nn)
    d["gw"] = rng.integers(-8, 9, (N, 3)).astype(np.float32)
    d["ga"] = np.float32(sign * Nn / 8.0)
    d.update(warp_arap_bwd_rows(d["xyz"], d["nodes_idx"], d["one_ring"], d["infl_idx"], d["weights"], d["R"], d["T"], d["gw"], d["ga"]))
    return d


def rot6d_grad64(d6, gR):
    """float64 autograd of the definition (oracle/torch_ref.py::rot6d): d sum(R * gR) / d d6"""
    import torch
    from oracle import torch_ref as TR
    x = torch.from_numpy(np.asarray(d6, np.float64)).requires_grad_(True)
    (TR.rot6d(x) * torch.from_numpy(np.asarray(gR, np.float64)).reshape(-1, 3, 3)).sum().backward()
    return x.grad.numpy()


ROT6D_C = (0.0, 0.5, -0.5, 0.25, -0.25, 1.0, -1.0, 1.5, -2.0, 0.0, 0.75)   # the a1 component of a2: small dyadics, 0 included


def rot6d_bwd_direct(seed):
    """ops.rot6d_bwd: frames a1 = 2^p s e_i, a2 = 2^q t e_j + c a1 (j != i; signs s, t; p, q in [-3, 3]; c from ROT6D_C): n1 = 2^p,
    dot = c 2^p, u = 2^q t e_j, n2 = 2^q are exact, every later value a short dyadic.  All 24 (i, j, s, t) orientations, each with every
    c (264 rows: two workgroups); gR small integers.  -> dict(d6 (264,6), gR (264,3,3), grad (264,6) float64)"""
    rng = np.random.default_rng([seed, 6])
    rows = []
    for i, j in itertools.permutations(range(3), 2):
        for s, t in itertools.product((1.0, -1.0), repeat=2):
            for c in ROT6D_C:
                p, q = rng.integers(-3, 4, 2)
                a1, a2 = np.zeros(3), np.zeros(3)
                a1[i] = s * 2.0 ** p
                a2[j] = t * 2.0 ** q
                rows.append(np.concatenate([a1, a2 + c * a1]))
    d6 = np.array(rows, np.float32)
    assert np.array_equal(d6, np.array(rows)) and d6.shape == (24 * len(ROT6D_C), 6)
    gR = rng.integers(-4, 5, (d6.shape[0], 3, 3)).astype(np.float32)
    return dict(d6=d6, gR=gR, grad=rot6d_grad64(d6, gR))


def chamfer_bwd_rows(a, b, i1, i2, g1, g2):
    """float64: L = sum(g1 * |a_i - b_i1(i)|^2) + sum(g2 * |b_j - a_i2(j)|^2) with the indices held fixed
    -> dict(d_a, d_b, mag_a, mag_b, addends)"""
    a, b, g1, g2 = (np.asarray(x, np.float64) for x in (a, b, g1, g2))
    i1, i2 = np.asarray(i1), np.asarray(i2)
    va, vb = 2.0 * g1[:, None] * (a - b[i1]), 2.0 * g2[:, None] * (b - a[i2])
    da, ma = scatter_sum(a.shape, np.concatenate([np.arange(a.shape[0]), i2]), np.concatenate([va, -vb]))
    db, mb = scatter_sum(b.shape, np.concatenate([np.arange(b.shape[0]), i1]), np.concatenate([vb, -va]))
    return dict(d_a=da, d_b=db, mag_a=ma, mag_b=mb, addends=(va, vb))


CHAMFER_VARIANTS = ("nn", "hub", "arbitrary")


def chamfer_bwd_direct(N, M, seed, variant):
    """ops.chamfer_bwd: integer clouds in [0, 63], g1 / g2 multiples of 1/4 in [-2, 2]; the index lists are
    nn: the true nearest neighbours (oracle; the clouds hold ties and coincident points); hub: every a_i -> one b, every b_j -> one a;
    arbitrary: any valid index.  The kernel must use the lists it is handed."""
    rng = np.random.default_rng([seed, N, M, CHAMFER_VARIANTS.index(variant)])
    a, b = rng.integers(0, 64, (N, 3)).astype(np.float32), rng.integers(0, 64, (M, 3)).astype(np.float32)
    g1, g2 = (rng.integers(-8, 9, N) / 4.0).astype(np.float32), (rng.integers(-8, 9, M) / 4.0).astype(np.float32)
    if variant == "nn":
        from oracle import oracle as O
        _, _, i1, i2 = O.chamfer(a, b)
    elif variant == "hub":
        i1, i2 = np.full(N, rng.integers(0, M), np.int32), np.full(M, rng.integers(0, N), np.int32)
    else:
        i1, i2 = rng.integers(0, M, N).astype(np.int32), rng.integers(0, N, M).astype(np.int32)
    d = dict(a=a, b=b, g1=g1, g2=g2, i1=i1, i2=i2)
    d.update(chamfer_bwd_rows(a, b, i1, i2, g1, g2))
    return d


BWD_SIZES = [2, 3, 64, 257, 513, 2048]
CHAMFER_BWD_SHAPES = [(1, 1), (255, 1), (256, 257), (300, 170), (2048, 2048)]
BWD_SEED = 5200


def warp_bwd_batch(N, hub, B=3):
    """B different entries, g_arap = +Nn/8, -Nn/8, 0"""
    return [warp_bwd_direct(N, BWD_SEED + b, hub, (1, -1, 0)[b % 3]) for b in range(B)]


def chamfer_bwd_batch(N, M, variant, B=3):
    return [chamfer_bwd_direct(N, M, BWD_SEED + b, variant) for b in range(B)]


# criterion level: (N, M, hi) — the coordinate range [0, hi] is small enough that the column sums of ddef9 over all P * Nn rows, and
# those of ddef9^T h2 (the first three input columns of W3), stay exact: criterion_bwd_reference, checked by the CPU half (at hi = 255
# the residuals are ~100 times larger and the sums leave 24 bits).  (64, 65) and (300, 170) take the fused warp forward, (5200, 64)
# the three-kernel one; CRIT_BWD_SWAPPED is the swapped-halves form (N == M, mirrored planting).
CRIT_BWD_CASES = [(64, 65, 7), (300, 170, 7), (5200, 64, 19)]
CRIT_BWD_SWAPPED = (300, 7)
DEF9_IDENTITY = np.array([1, 0, 0, 0, 1, 0], np.float64)


def criterion_bwd_reference(refs, g_arap):
    """g_terms zero except the ARAP column = g_arap[p] (+-Nn/8) for the directional pairs `refs` (reference_direction): dwarped and
    dv12 are exactly 0, so ddef9[p] = [d_T | rot6d gradient of (def9[3:] + identity) against d_R] from ARAP alone.  The last decoder
    layer's bias gradient is the column sum of ddef9 over all pairs' nodes, its weight gradient ddef9^T h2 with h2[:, :3] = the node
    positions (the pass-through Deformer) and 0 elsewhere.  -> dict(ddef9 [P x (Nn,9)], db3 (9,), dW3 (9,3), mag_b3, mag_W3, addends)"""
    dd, hs, adds = [], [], []
    for r, ga in zip(refs, g_arap):
        Nn = r["Nn"]
        zero = np.zeros((Nn, 3))      # no warp gradient: the nodes as a cloud of their own, weights and gw zero
        w = warp_arap_bwd_rows(r["g"], np.arange(Nn), r["graph"]["one_ring"], zero.astype(np.int64), zero, r["R"], r["T"], zero, ga)
        d6 = r["def9"][:, 3:] + DEF9_IDENTITY
        dd.append(np.concatenate([w["d_T"], rot6d_grad64(d6, w["d_R"])], 1))
        hs.append(r["g"])
        adds += [w["addends"][2], w["addends"][3]]
        assert exact_sums(w["addends"], (w["mag_R"], w["mag_T"]))
    D, H = np.concatenate(dd), np.concatenate(hs)
    prod = D[:, :, None] * H[:, None, :]
    return dict(ddef9=dd, db3=D.sum(0), mag_b3=np.abs(D).sum(0), dW3=prod.sum(0), mag_W3=np.abs(prod).sum(0), addends=adds + [D, prod])
