"""Shared by tests/test_mesh_geodesics_cpu.py and tests/test_gpu_mesh_geodesics.py: the triangle-front geodesic scheme stated once,
in float64 numpy, the meshes it is tried on, and what its values are judged against (edge paths, analytic distances).  A plain
module, like frob_term_common.py.

The scheme (first-order upwind update on triangles, relaxed to its fixed point).  For a source s: D[s] = 0, every other D[v] = +inf.
Sweep until a whole sweep accepts nothing.  For every corner (v; a, b) of every triangle (vertex v, opposite edge a b):
  edge candidate   e = min(D[a] + |a - v|, D[b] + |b - v|)
  front candidate  only when D[a] and D[b] are finite: X = [a - v, b - v] (3 x 2), Q = (X^T X)^-1, d = (D[a], D[b])^T, 1 = (1, 1)^T;
                   t = the larger root of (1^T Q 1) t^2 - 2 (1^T Q d) t + (d^T Q d - 1) = 0, valid only if the discriminant is >= 0
                   and both components of Q (d - t 1) are < 0 (the front enters the corner through the opposite edge)
  candidate        c = min(t, e) if t is valid, else e
  degenerate       det(X^T X) not a normal positive number: the corner has only its edge candidate
  acceptance       D[v] <- c only when D[v] is +inf and c finite, or c < D[v] (1 - 2^-40)
The margin makes every accepted update shrink a value by a fixed factor, so the sweeps end; two update orders then differ by
the margin's effect only.  Here a sweep is a Jacobi sweep (every corner reads the previous sweep's values; a vertex takes the
least of its corners' candidates, and the acceptance is applied to that least one).  Only the corners one of whose neighbours
changed in the previous sweep are evaluated: any other corner's candidate is the one it had, which its vertex has taken or
refused already and, values only ever falling, would refuse again; the result is the full sweep's, bit for bit.

The arithmetic is written out operation by operation (corner_table, _candidates): the HIP kernel evaluates the same expressions
in the same order without contraction."""
import numpy as np

MARGIN = 1.0 - 2.0 ** -40
TINY = np.finfo(np.float64).tiny


# ---------------------------------------------------------------- meshes
def grid_mesh(m, jitter=0.0, seed=0, stretch=1.0):
    """A flat m x m grid over [0, stretch] x [0, 1] (z = 0), the diagonal of cell (i, j) alternating with (i + j) % 2; with
    jitter > 0 every interior vertex is moved by jitter * spacing * U(-0.5, 0.5) in x and y before the stretch."""
    h = 1.0 / (m - 1)
    ii, jj = np.meshgrid(np.arange(m), np.arange(m), indexing="ij")
    xy = np.stack([ii * h, jj * h], -1).astype(np.float64)
    if jitter > 0:
        rng = np.random.default_rng(seed)
        xy[1:-1, 1:-1] += jitter * h * (rng.random((m - 2, m - 2, 2)) - 0.5)
    verts = np.zeros((m * m, 3))
    verts[:, 0] = xy[..., 0].reshape(-1) * stretch
    verts[:, 1] = xy[..., 1].reshape(-1)
    faces = []
    for i in range(m - 1):
        for j in range(m - 1):
            p00, p01, p10, p11 = i * m + j, i * m + j + 1, (i + 1) * m + j, (i + 1) * m + j + 1
            if (i + j) % 2 == 0:
                faces += [(p00, p10, p11), (p00, p11, p01)]
            else:
                faces += [(p00, p10, p01), (p10, p11, p01)]
    return verts, np.asarray(faces, dtype=np.int32)


def icosphere(subdivisions):
    """The unit icosphere: an icosahedron with every triangle split in four `subdivisions` times, vertices on the unit sphere."""
    p = (1.0 + np.sqrt(5.0)) / 2.0
    v = [(-1, p, 0), (1, p, 0), (-1, -p, 0), (1, -p, 0), (0, -1, p), (0, 1, p), (0, -1, -p), (0, 1, -p), (p, 0, -1), (p, 0, 1), (-p, 0, -1),
         (-p, 0, 1)]
    verts = [np.asarray(x, dtype=np.float64) / np.sqrt(1.0 + p * p) for x in v]
    faces = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4),
             (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(subdivisions):
        mid, out = {}, []

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                x = verts[a] + verts[b]
                verts.append(x / np.linalg.norm(x))
                mid[key] = len(verts) - 1
            return mid[key]

        for a, b, c in faces:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        faces = out
    return np.asarray(verts), np.asarray(faces, dtype=np.int32)


def stretched_grid(m, factor):
    """grid_mesh stretched `factor` times along x: every triangle gets an obtuse or near-degenerate corner"""
    return grid_mesh(m, stretch=float(factor))


def fan(valence):
    """one hub (vertex 0) at the apex of a shallow cone, `valence` rim vertices around it, `valence` triangles"""
    ang = 2.0 * np.pi * np.arange(valence) / valence
    verts = np.concatenate([[[0.0, 0.0, 0.25]], np.stack([np.cos(ang), np.sin(ang), np.zeros(valence)], -1)])
    rim = 1 + np.arange(valence)
    faces = np.stack([np.zeros(valence, dtype=np.int64), rim, 1 + (np.arange(valence) + 1) % valence], -1)
    return verts, faces.astype(np.int32)


def degenerate_mesh():
    """a 5 x 5 grid plus: a zero-area triangle on three collinear grid vertices, a face listed twice, a face that names one
    vertex twice, and one isolated vertex (the last)"""
    verts, faces = grid_mesh(5)
    extra = np.asarray([(0, 1, 2), tuple(faces[3]), tuple(faces[3]), (6, 6, 7)], dtype=np.int32)
    return np.concatenate([verts, [[0.5, 0.5, 1.0]]]), np.concatenate([faces, extra])


def two_spheres(subdivisions):
    """two disjoint icospheres in one mesh"""
    v, f = icosphere(subdivisions)
    return np.concatenate([v, v + [3.0, 0.0, 0.0]]), np.concatenate([f, f + len(v)]).astype(np.int32)


# ---------------------------------------------------------------- what the scheme is judged against
def analytic_plane(verts, sources):
    return np.linalg.norm(verts[None, :, :] - verts[np.asarray(sources)][:, None, :], axis=-1)


def analytic_sphere(verts, sources):
    return np.arccos(np.clip(verts[np.asarray(sources)] @ verts.T, -1.0, 1.0))


def edge_paths(verts, faces, sources):
    """exact shortest paths along the mesh edges (scipy's Dijkstra) -> (S, V)"""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import dijkstra
    faces = np.asarray(faces, dtype=np.int64)
    e = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]], 0)
    e = np.unique(np.sort(e[e[:, 0] != e[:, 1]], 1), axis=0)
    w = np.linalg.norm(verts[e[:, 0]] - verts[e[:, 1]], axis=1)
    n = len(verts)
    g = coo_matrix((w, (e[:, 0], e[:, 1])), shape=(n, n)).tocsr()
    return dijkstra(g, directed=False, indices=np.asarray(sources))


def mean_rel_error(D, exact):
    """mean over the vertices with exact > 0 of |D - exact| / exact, per source -> (S,)"""
    out = []
    for d, x in zip(D, exact):
        keep = x > 0
        out.append(float(np.mean(np.abs(d[keep] - x[keep]) / x[keep])))
    return np.asarray(out)


def star_of(faces, s):
    """the vertices that share a triangle with s (s excluded)"""
    faces = np.asarray(faces)
    ring = np.unique(faces[(faces == s).any(1)])
    return ring[ring != s]


# ---------------------------------------------------------------- the scheme
def corner_table(verts, faces):
    """every corner (v; a, b) of every triangle, grouped by v -> dict(v, a, b, la, lb, q11, q12, q22, ok): la = |a - v|, lb = |b - v|,
    Q = (X^T X)^-1 where ok (det a normal positive number)"""
    verts = np.asarray(verts, dtype=np.float64)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    v = np.concatenate([f[:, 0], f[:, 1], f[:, 2]])
    a = np.concatenate([f[:, 1], f[:, 2], f[:, 0]])
    b = np.concatenate([f[:, 2], f[:, 0], f[:, 1]])
    order = np.argsort(v, kind="stable")
    v, a, b = v[order], a[order], b[order]
    ea, eb = verts[a] - verts[v], verts[b] - verts[v]
    g11 = ea[:, 0] * ea[:, 0] + ea[:, 1] * ea[:, 1] + ea[:, 2] * ea[:, 2]
    g12 = ea[:, 0] * eb[:, 0] + ea[:, 1] * eb[:, 1] + ea[:, 2] * eb[:, 2]
    g22 = eb[:, 0] * eb[:, 0] + eb[:, 1] * eb[:, 1] + eb[:, 2] * eb[:, 2]
    det = g11 * g22 - g12 * g12
    ok = np.isfinite(det) & (det >= TINY)
    safe = np.where(ok, det, 1.0)
    t = dict(v=v, a=a, b=b, la=np.sqrt(g11), lb=np.sqrt(g22), q11=g22 / safe, q12=-g12 / safe, q22=g11 / safe, ok=ok)
    t["packed"] = np.stack([t[k] for k in ("la", "lb", "q11", "q12", "q22")])
    return t


def _candidates(t, ci, da, db):
    """the candidates of the corners `ci` of table `t` for their neighbours' values da, db"""
    with np.errstate(invalid="ignore", over="ignore"):
        la, lb, q11, q12, q22 = t["packed"][:, ci]
        e = np.minimum(da + la, db + lb)
        s1, s2 = q11 + q12, q12 + q22
        A = s1 + s2
        bb = s1 * da + s2 * db
        cc = q11 * da * da + 2.0 * q12 * da * db + q22 * db * db - 1.0
        disc = bb * bb - A * cc
        front = (bb + np.sqrt(disc)) / A
        ua, ub = da - front, db - front
        n1 = q11 * ua + q12 * ub
        n2 = q12 * ua + q22 * ub
        valid = t["ok"][ci] & np.isfinite(da) & np.isfinite(db) & (disc >= 0) & (n1 < 0) & (n2 < 0) & (front < e)
    return np.where(valid, front, e)


def solve(verts, faces, sources=None):
    """D (S, V) float64 of the scheme for `sources` (None: all vertices) -> (D, sweeps): sweeps = the number of sweeps until one
    accepted nothing, that one included"""
    V = len(verts)
    sources = np.arange(V) if sources is None else np.asarray(sources, dtype=np.int64)
    t = corner_table(verts, faces)
    rows = min(64, max(1, (1 << 23) // max(len(t["v"]), 1)))  # sources per pass: its scratch (a byte per source and corner) stays in cache
    parts = [_solve_rows(t, V, sources[lo:lo + rows]) for lo in range(0, len(sources), rows)]
    return np.concatenate([d for d, _ in parts]), max(n for _, n in parts)


def _solve_rows(t, V, sources):
    C, S = len(t["v"]), len(sources)
    mark = np.zeros(S * C, dtype=bool)
    D = np.full((S, V), np.inf)
    D[np.arange(S), sources] = 0.0
    flat = D.reshape(-1)
    # the corners that read vertex u: touch_c[touch_off[u] : touch_off[u + 1]]
    order = np.argsort(np.concatenate([t["a"], t["b"]]), kind="stable")
    touch_c = np.concatenate([np.arange(C), np.arange(C)])[order]
    touch_off = np.concatenate([[0], np.cumsum(np.bincount(np.concatenate([t["a"], t["b"]]), minlength=V))])
    cs, cu = np.arange(S), sources          # what changed in the sweep before: (source row, vertex)
    for sweep in range(1, 4 * V + 2):
        cnt = touch_off[cu + 1] - touch_off[cu]
        total = int(cnt.sum())
        first = np.repeat(touch_off[cu] - (np.cumsum(cnt) - cnt), cnt)
        mark[np.repeat(cs, cnt) * C + touch_c[first + np.arange(total)]] = True
        key = np.flatnonzero(mark)             # each such corner once, ascending
        mark[key] = False
        si, ci = key // C, key % C
        cand = _candidates(t, ci, flat[si * V + t["a"][ci]], flat[si * V + t["b"][ci]])
        vkey = si * V + t["v"][ci]             # ascending: the corners are grouped by v
        if not len(vkey):
            return D, sweep
        starts = np.flatnonzero(np.r_[True, vkey[1:] != vkey[:-1]])
        best, rows = np.minimum.reduceat(cand, starts), vkey[starts]
        old = flat[rows]
        take = np.where(np.isinf(old), np.isfinite(best), best < old * MARGIN)
        if not take.any():
            return D, sweep
        flat[rows[take]] = best[take]
        cs, cu = rows[take] // V, rows[take] % V
    raise RuntimeError("mesh_geodesic_ref.solve: no fixed point within 4 V = %d sweeps" % (4 * V))
