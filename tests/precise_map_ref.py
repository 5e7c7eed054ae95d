"""The precise (vertex-to-point) map in numpy: for every source feature p the closest point of the target's triangle mesh
embedded in feature space (include/dvm.h, dvm_precise_map_f32).

Per face (a,b,c), with w = f2[a] - p, e1 = f2[b] - f2[a], e2 = f2[c] - f2[a]: the closest point of each of the three edges as
a segment and, where the face's Gram determinant is positive beyond its own rounding (det > 8 eps e11 e22) and the three
weights are >= 0, the interior projection.  Every candidate is a point of the face, and its value is the squared norm of the
residual w + s e1 + t e2 itself — so a degenerate face (repeated index, collinear corners) is simply the union of its edges
and nothing here can produce a NaN from finite inputs.  The smallest value wins, ties to the candidate named first (ab, ac,
bc, interior) and to the lowest face index; a NaN counts as +inf.  Every dot product is a k-ordered sequential chain in the
working precision (float64, or float32 with every operation rounded), differences taken first.

closest(...) is that definition; brute(...) an independent dense sampling for tiny cases; the rest are the seeded input
families of tests/test_precise_map_ref_cpu.py and tests/test_gpu_precise_map.py."""
import functools

import numpy as np

import mesh_geodesic_ref as MG

REGIONS = ("a", "b", "c", "ab", "ac", "bc", "interior")


def _chain(xs, ys, dtype):
    """sum_k x_k y_k, k ascending, every product and sum rounded to dtype; xs, ys callables k -> array."""
    acc = None
    for k in range(xs.n):
        t = (xs(k) * ys(k)).astype(dtype)
        acc = t if acc is None else (acc + t).astype(dtype)
    return acc


class _Cols:
    def __init__(self, n, fn):
        self.n, self.fn = n, fn

    def __call__(self, k):
        return self.fn(k)


def closest(f1, f2, faces, dtype=np.float64):
    """f1 (N,d), f2 (M,d), faces (F,3) -> dict(dist (N,), bary (N,3), face (N,), region (N,), left_out).  A face with an index
    outside [0,M) is left out; a row with no admissible face gets face -1, bary 0, dist +inf (region -1)."""
    dtype = np.dtype(dtype).type
    f1, f2 = np.asarray(f1, dtype=dtype), np.asarray(f2, dtype=dtype)
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    N, d = f1.shape
    M = f2.shape[0]
    ok = ((faces >= 0) & (faces < M)).all(axis=1)
    fid = np.nonzero(ok)[0]
    out = dict(dist=np.full(N, np.inf, dtype), bary=np.zeros((N, 3), dtype), face=np.full(N, -1, np.int64),
               region=np.full(N, -1, np.int64), left_out=int((~ok).sum()))
    if fid.size == 0:
        return out
    fa = faces[fid]
    with np.errstate(all="ignore"):
        A, B, C = f2[fa[:, 0]], f2[fa[:, 1]], f2[fa[:, 2]]
        E1, E2, E3 = (B - A).astype(dtype), (C - A).astype(dtype), (C - B).astype(dtype)
        col = lambda X: _Cols(d, lambda k: X[:, k])
        e11, e12, e22, e33 = (_chain(col(E1), col(E1), dtype), _chain(col(E1), col(E2), dtype), _chain(col(E2), col(E2), dtype),
                              _chain(col(E3), col(E3), dtype))
        W = lambda k: (A[None, :, k] - f1[:, None, k]).astype(dtype)          # (N, F)
        wc, c1, c2 = _Cols(d, W), _Cols(d, lambda k: E1[None, :, k]), _Cols(d, lambda k: E2[None, :, k])
        d1, d2 = _chain(c1, wc, dtype), _chain(c2, wc, dtype)
        one, zero = dtype(1), dtype(0)

        def seg(num, den):
            t = np.where(den > 0, -num / np.where(den > 0, den, one), zero).astype(dtype)
            return np.clip(np.where(np.isnan(t), zero, t), zero, one).astype(dtype)

        t1, t2 = seg(d1, e11[None]), seg(d2, e22[None])
        nb = ((d2 - d1).astype(dtype) + (e12 - e11).astype(dtype)[None]).astype(dtype)
        t3 = seg(nb, e33[None])
        s3 = (one - t3).astype(dtype)
        pr = (e11 * e22).astype(dtype)
        det = (pr - (e12 * e12).astype(dtype)).astype(dtype)
        interior = det > dtype(8) * np.finfo(dtype).eps / 2 * pr
        dsafe = np.where(interior, det, one)[None]
        s = (((e12[None] * d2).astype(dtype) - (e22[None] * d1).astype(dtype)).astype(dtype) / dsafe).astype(dtype)
        t = (((e12[None] * d1).astype(dtype) - (e11[None] * d2).astype(dtype)).astype(dtype) / dsafe).astype(dtype)
        inside = interior[None] & (s >= 0) & (t >= 0) & ((s + t).astype(dtype) <= 1)
        s, t = np.where(inside, s, t1), np.where(inside, t, zero)
        cand = ((t1, np.zeros_like(t1)), (np.zeros_like(t2), t2), (s3, t3), (s, t))
        v = [None] * 4
        for k in range(d):
            w, u1, u2 = W(k), E1[None, :, k], E2[None, :, k]
            for c, (cs, ct) in enumerate(cand):
                r = (((cs * u1).astype(dtype) + w).astype(dtype) + (ct * u2).astype(dtype)).astype(dtype)
                r2 = (r * r).astype(dtype)
                v[c] = r2 if v[c] is None else (v[c] + r2).astype(dtype)
        best, which = v[0].copy(), np.zeros(v[0].shape, np.int64)
        for c in (1, 2, 3):
            take = (v[c] < best) & (inside if c == 3 else True)
            best, which = np.where(take, v[c], best), np.where(take, c, which)
        best = np.where(np.isnan(best), np.inf, best)
        j = np.argmin(best, axis=1)                       # the first of equals: the lowest face index
        n = np.arange(N)
        wch, vb = which[n, j], best[n, j]
        T1, T2, T3, S3, S, T = (x[n, j] for x in (t1, t2, t3, s3, s, t))
        bary = np.select([wch[:, None] == 0, wch[:, None] == 1, wch[:, None] == 2],
                         [np.stack([one - T1, T1, 0 * T1], 1), np.stack([one - T2, 0 * T2, T2], 1), np.stack([0 * T3, S3, T3], 1)],
                         np.stack([one - (S + T).astype(dtype), S, T], 1)).astype(dtype)
        fin = np.isfinite(vb)
        bary = np.where(fin[:, None], bary, np.array([1, 0, 0], dtype)[None])
        out["dist"], out["bary"], out["face"] = np.sqrt(vb).astype(dtype), bary, fid[j]
        out["region"] = np.where(fin, region_of(bary), -1)
    return out


def region_of(bary):
    """0..6 = REGIONS: which weights of (N,3) are exactly zero."""
    z = bary == 0
    code = {(False, True, True): 0, (True, False, True): 1, (True, True, False): 2, (False, False, True): 3, (False, True, False): 4,
            (True, False, False): 5, (False, False, False): 6}
    return np.array([code.get(tuple(bool(x) for x in row), -1) for row in z], np.int64)


def brute(f1, f2, faces, K=60):
    """Distance to the nearest of the (K+1)(K+2)/2 barycentric grid points of every face, float64 -> (N,): an upper bound of the
    true distance that exceeds it by at most the longest edge / K."""
    f1, f2 = np.asarray(f1, np.float64), np.asarray(f2, np.float64)
    ij = np.array([(i, j) for i in range(K + 1) for j in range(K + 1 - i)], np.float64) / K
    w = np.stack([1 - ij.sum(1), ij[:, 0], ij[:, 1]], 1)            # (G,3)
    best = np.full(len(f1), np.inf)
    for a, b, c in np.asarray(faces):
        pts = w @ f2[[a, b, c]]                                      # (G,d)
        best = np.minimum(best, np.sqrt(((f1[:, None, :] - pts[None]) ** 2).sum(-1)).min(1))
    return best


def point_distance(f1, f2, pi_idx, bary):
    """|p - sum_k bary_k f2[pi_idx_k]| in float64 -> (N,)."""
    f1, f2, bary = np.asarray(f1, np.float64), np.asarray(f2, np.float64), np.asarray(bary, np.float64)
    q = (bary[:, :, None] * f2[np.asarray(pi_idx)]).sum(1)
    return np.sqrt(((f1 - q) ** 2).sum(1))


# ---- the seeded input families: name -> (f1 (N,d), f2 (M,d), faces (F,3)), all float32 / int32 -------------------------

def _surface_points(g, verts, faces, n):
    f = g.integers(0, len(faces), n)
    w = g.dirichlet(np.ones(3), n)
    return (w[:, :, None] * verts[faces[f]]).sum(1)


def randn(seed=0, n=40, d=128, mesh=None):
    """Unit normal vertex features; a source is a vertex feature + 0.3 randn."""
    g = np.random.default_rng(seed)
    verts, faces = MG.icosphere(2) if mesh is None else mesh
    f2 = g.standard_normal((len(verts), d)).astype(np.float32)
    f1 = (f2[g.integers(0, len(verts), n)] + 0.3 * g.standard_normal((n, d))).astype(np.float32)
    return f1, f2, faces.astype(np.int32)


def smooth(seed=0, n=96, d=128, mesh=None, offset=0.0):
    """'Trained-like' features: verts @ A + 0.02 randn; sources likewise from jittered surface points.  offset: the size of one
    constant vector added to both sides."""
    g = np.random.default_rng(seed)
    verts, faces = MG.icosphere(2) if mesh is None else mesh
    verts = np.asarray(verts, np.float64)
    A = g.standard_normal((3, d)) / np.sqrt(3.0)
    c = g.standard_normal(d)
    c *= offset / np.linalg.norm(c)
    f2 = (verts @ A + 0.02 * g.standard_normal((len(verts), d)) + c).astype(np.float32)
    f1 = (_surface_points(g, verts, faces, n) @ A + 0.02 * g.standard_normal((n, d)) + c).astype(np.float32)
    return f1, f2, faces.astype(np.int32)


def offset(seed=0, n=96, d=128):
    """The smooth family moved by one constant vector of size 1e3: the Gram form |p|^2 - 2 p.x + |x|^2 cancels completely."""
    return smooth(seed + 100, n, d, offset=1.0e3)


def degenerate(seed=0, n=64, d=8):
    """Faces (a,a,b) and (a,a,a), corners with exactly collinear features (a midpoint of small integers), zero-feature vertices,
    beside a few ordinary faces."""
    g = np.random.default_rng(seed)
    M = 24
    f2 = g.integers(-8, 9, (M, d)).astype(np.float32) * 2.0
    f2[3] = (f2[1] + f2[2]) / 2                                # exactly collinear with 1, 2
    f2[4] = f2[1] + 3 * (f2[2] - f2[1])                        # ... and beyond the segment
    f2[5] = 0.0
    f2[6] = 0.0                                                # two zero-feature vertices (identical rows)
    f2[8] = f2[7]                                              # a duplicated vertex
    faces = np.array([(0, 0, 9), (10, 10, 10), (1, 2, 3), (1, 3, 4), (2, 1, 4), (5, 6, 11), (5, 5, 6), (7, 8, 12), (7, 12, 8),
                      (13, 14, 15), (14, 16, 15), (17, 18, 19), (20, 21, 22), (21, 23, 22), (9, 9, 0), (6, 5, 5)], np.int32)
    src = g.integers(0, M, n)
    f1 = (f2[src] + g.standard_normal((n, d)) * np.where(np.arange(n) % 4 == 0, 0.0, 1.5)[:, None]).astype(np.float32)
    return f1, f2, faces


def planted(seed=0, d=8):
    """Small-integer features that are zero in the last four coordinates; a source is a dyadic barycentric combination (weights
    in quarters) of one face plus an offset in the last four coordinates only, so face, weights and distance are exact in fp32.
    -> f1, f2, faces, expected dict(face, bary, dist).  The features are an injective linear image of a flat grid mesh, so the
    faces tile a plane and the planted point's own face is the nearest; a vertex or edge planting ties exactly between its
    incident faces and the lowest face index is expected."""
    g = np.random.default_rng(seed)
    m = 5
    verts, faces = MG.grid_mesh(m)
    verts = np.rint(np.asarray(verts)[:, :2] * (m - 1)).astype(np.int64)          # integer grid coordinates
    L = np.concatenate([np.array([[4, 0, 8, -4], [0, 4, 4, 8]], np.int64), g.integers(-2, 3, (2, d - 8)) * 4], 1)   # d >= 8
    f2 = np.zeros((len(verts), d), np.float32)
    f2[:, :d - 4] = verts @ L
    weights = np.array([(4, 0, 0), (0, 4, 0), (0, 0, 4), (2, 2, 0), (2, 0, 2), (0, 2, 2), (1, 3, 0), (2, 1, 1), (1, 1, 2), (1, 2, 1)],
                       np.float32) / 4
    rows, bary, face = [], [], []
    for i in range(40):
        f = int(g.integers(0, len(faces)))
        w = weights[i % len(weights)]
        off = np.zeros(d, np.float32)
        off[d - 4:] = g.integers(-3, 4, 4)
        if not off.any():
            off[d - 1] = 1.0
        rows.append((w[:, None] * f2[faces[f]]).sum(0) + off)
        bary.append(w), face.append(f)
    f1 = np.asarray(rows, np.float32)
    bary, face = np.asarray(bary, np.float32), np.asarray(face)
    dist = np.sqrt((f1[:, d - 4:].astype(np.float64) ** 2).sum(1)).astype(np.float32)
    # the expectation for plantings on a vertex or an edge: the lowest face that holds the same point, weights in ITS order
    for i in range(len(f1)):
        q = (bary[i][:, None] * f2[faces[face[i]]]).sum(0)
        for f in range(face[i]):
            tri = f2[faces[f]].astype(np.float64)
            sol, *_ = np.linalg.lstsq(np.vstack([tri.T, np.ones(3)]), np.append(q, 1.0), rcond=None)
            if np.abs(np.vstack([tri.T, np.ones(3)]) @ sol - np.append(q, 1.0)).max() < 1e-9 and (sol > -1e-9).all():
                face[i], bary[i] = f, np.rint(sol * 4) / 4
                break
    return f1, f2, faces.astype(np.int32), dict(face=face, bary=bary, dist=dist)


def nonfinite(seed=0, n=48, d=8):
    """The randn family (d = 8) with NaN / Inf planted: source rows 0 (a NaN), 1 (+Inf), 2 (-Inf and NaN); target vertices 0 (NaN),
    1 (+Inf).  -> f1, f2, faces, bad_rows."""
    f1, f2, faces = randn(seed + 7, n, d)
    f1, f2 = f1.copy(), f2.copy()
    f1[0, 3] = np.nan
    f1[1, 0] = np.inf
    f1[2, 1], f1[2, 5] = -np.inf, np.nan
    f2[0, 2] = np.nan
    f2[1, 4] = np.inf
    return f1, f2, faces, np.array([0, 1, 2])


def chain_error(f1, f2, faces, r64, r32):
    """The float32 chain's own error against float64 on one input, as the tests look at a result: the largest over the rows of
    |dist32 - dist64|, ||p - q32| - dist64| and |dist32 - |p - q32||, q32 = sum_k bary32_k f2[pi_idx_k] evaluated in float64 (so the
    fp32 grain of the weights, times the size of the features, is part of it).  Rows without a finite float64 distance are skipped."""
    fin = np.isfinite(r64["dist"]) & (r32["face"] >= 0)
    pq = point_distance(f1[fin], f2, np.asarray(faces)[r32["face"][fin]], r32["bary"][fin])
    d32, d64 = r32["dist"][fin].astype(np.float64), r64["dist"][fin]
    with np.errstate(all="ignore"):
        return float(max(np.abs(d32 - d64).max(), np.abs(pq - d64).max(), np.abs(d32 - pq).max()))


@functools.lru_cache(maxsize=None)
def family(name, d=None):
    """The named float family at its test size -> (f1, f2, faces, ref64, ref32, err), err = chain_error: the float32 chain's own
    error, from which the GPU test takes its bar."""
    make = dict(randn=randn, smooth=smooth, offset=offset, degenerate=degenerate)[name]
    f1, f2, faces = make() if d is None else make(d=d)
    r64, r32 = closest(f1, f2, faces, np.float64), closest(f1, f2, faces, np.float32)
    return f1, f2, faces, r64, r32, chain_error(f1, f2, faces, r64, r32)
