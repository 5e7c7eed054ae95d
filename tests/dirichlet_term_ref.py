"""The Dirichlet term's definitions in float64 numpy: the two operator builders (dvm_mesh_laplacian_f32, dvm_knn_laplacian_f32) with
their leave-out rules and the canonical row order, and the energy and its gradient (dvm_dirichlet_term_f32).  The kernels
evaluate these expressions in this order; the tests judge them against this file (profiles/notes_dirichlet.md derives the bars).

An operator is a dict: rowptr (N+1,) int32, col / w (Ecap,) int32 / float32 (behind rowptr[N]: -1 / 0), norm float32,
mass (N,) float32 or None, stats (4,) int32 = [left out for an index outside [0, N), left out for degenerate geometry, self entries,
entries kept].  THE CANONICAL ORDER of a row: its kept candidate entries in ascending candidate number, where
  mesh  candidates 6f+2c, 6f+2c+1 = (a, b, w), (b, a, w) for corner c of face f: v = face[c], a = face[(c+1)%3], b = face[(c+2)%3]
  list  candidates 2(iK+s), 2(iK+s)+1 = (i, j, w), (j, i, w) for slot s of point i, j = nbr[i, s]."""
import numpy as np

U = 2.0 ** -24
STAT_RANGE, STAT_DEGEN, STAT_SELF, STAT_KEPT = 0, 1, 2, 3


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross2(u, v):
    cx = u[..., 1] * v[..., 2] - u[..., 2] * v[..., 1]
    cy = u[..., 2] * v[..., 0] - u[..., 0] * v[..., 2]
    cz = u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]
    return (cx * cx + cy * cy) + cz * cz


def tree_sum(x):
    """The fixed-order sum of launch_reduce_partials: lane t adds x[t], x[t + 256], .. in turn, then red[t] += red[t + o] for
    o = 128 .. 1."""
    x = np.asarray(x, np.float64)
    pad = np.zeros((-len(x)) % 256)
    rows = np.concatenate([x, pad]).reshape(-1, 256)
    red = np.zeros(256)
    # the padding adds +0 behind a lane's last term: it changes no bit
    for r in rows:
        red = red + r
    o = 128
    while o > 0:
        red[:o] = red[:o] + red[o:2 * o]
        o //= 2
    return red[0]


def _csr(rowkey, colkey, wkey, N):
    """The counting sort: kept candidates (rowkey >= 0) grouped by row, ascending candidate number within a row."""
    E = len(rowkey)
    kept = np.flatnonzero(rowkey >= 0)
    order = kept[np.argsort(rowkey[kept], kind="stable")]
    rowptr = np.zeros(N + 1, np.int32)
    rowptr[1:] = np.cumsum(np.bincount(rowkey[kept], minlength=N))
    col = np.full(E, -1, np.int32)
    w = np.zeros(E, np.float32)
    col[:len(order)] = colkey[order]
    w[:len(order)] = wkey[order]
    return rowptr, col, w, order


def mesh_laplacian(verts, faces):
    """verts (N,3) float32, faces (F,3) int -> operator dict (+ 'cot_scale' (Ecap,): |u||v| / |u x v| of every entry, for the bars,
    and 'min_angle' in degrees over the kept faces)."""
    verts = np.asarray(verts, np.float32)
    faces = np.asarray(faces, np.int64)
    N, F = len(verts), len(faces)
    X = verts.astype(np.float64)
    in_range = ((faces >= 0) & (faces < N)).all(1)
    safe = np.where(in_range[:, None], faces, 0)
    P = X[safe]                                           # (F,3,3)
    cot = np.zeros((F, 3))
    scale = np.zeros((F, 3))
    angle = np.full((F, 3), 180.0)
    ok = in_range.copy()
    area = np.zeros(F)
    with np.errstate(all="ignore"):
        for c in range(3):
            u, v = P[:, (c + 1) % 3] - P[:, c], P[:, (c + 2) % 3] - P[:, c]
            c2 = _cross2(u, v)
            ok &= (c2 > 0) & (c2 < np.inf)
            ln = np.sqrt(c2)
            cot[:, c] = _dot(u, v) / ln
            scale[:, c] = np.sqrt(_dot(u, u)) * np.sqrt(_dot(v, v)) / ln
            angle[:, c] = np.degrees(np.arctan2(ln, _dot(u, v)))
            if c == 0:
                area = 0.5 * ln
    degenerate = in_range & ~ok
    area = np.where(ok, area, 0.0)
    rowkey = np.full(6 * F, -1, np.int64)
    colkey = np.full(6 * F, -1, np.int64)
    wkey = np.zeros(6 * F, np.float32)
    skey = np.zeros(6 * F)
    for c in range(3):
        a, b = faces[:, (c + 1) % 3], faces[:, (c + 2) % 3]
        wc = np.where(ok, 0.5 * cot[:, c], 0.0).astype(np.float32)
        for side, (r, q) in enumerate(((a, b), (b, a))):
            rowkey[2 * c + side::6] = np.where(ok, r, -1)
            colkey[2 * c + side::6] = np.where(ok, q, -1)
            wkey[2 * c + side::6] = wc
            skey[2 * c + side::6] = np.where(ok, scale[:, c], 0.0)
    rowptr, col, w, order = _csr(rowkey, colkey, wkey, N)
    mass = np.zeros(N)
    for f in np.flatnonzero(ok):                          # ascending face order = ascending even candidate number in the row
        for v in faces[f]:
            mass[v] = mass[v] + area[f] / 3.0
    cot_scale = np.zeros(6 * F)
    cot_scale[:len(order)] = skey[order]
    stats = np.array([int((~in_range).sum()), int(degenerate.sum()), 0, len(order)], np.int32)
    return dict(rowptr=rowptr, col=col, w=w, norm=np.float32(2.0 * tree_sum(area)), mass=mass.astype(np.float32), stats=stats,
                cot_scale=cot_scale, min_angle=float(angle[ok].min()) if ok.any() else 180.0, area=float(area.sum()))


def knn_laplacian(xyz, nbr, mode="stretch"):
    """xyz (N,3) float32, nbr (N,K) int, mode 'stretch' (w = 1 / |x_i - x_j|^2) or 'uniform' (w = 1) -> operator dict of W + W^T."""
    xyz = np.asarray(xyz, np.float32)
    nbr = np.asarray(nbr, np.int64)
    N, K = nbr.shape
    X = xyz.astype(np.float64)
    i = np.repeat(np.arange(N), K)
    j = nbr.reshape(-1)
    is_self = j == i
    out = ~is_self & ((j < 0) | (j >= N))
    ok = ~is_self & ~out
    d = X[i] - X[np.where(ok, j, 0)]
    d2 = _dot(d, d)
    bad = np.zeros_like(ok)
    wv = np.ones(N * K, np.float32)
    if mode == "stretch":
        bad = ok & ~((d2 > 0) & (d2 < np.inf))
        ok = ok & ~bad
        with np.errstate(all="ignore"):
            wv = (1.0 / d2).astype(np.float32)
    elif mode != "uniform":
        raise ValueError(mode)
    E = 2 * N * K
    rowkey, colkey, wkey = np.full(E, -1, np.int64), np.full(E, -1, np.int64), np.zeros(E, np.float32)
    rowkey[0::2], colkey[0::2] = np.where(ok, i, -1), np.where(ok, j, -1)
    rowkey[1::2], colkey[1::2] = np.where(ok, j, -1), np.where(ok, i, -1)
    wkey[0::2] = wkey[1::2] = np.where(ok, wv, np.float32(0))
    rowptr, col, w, order = _csr(rowkey, colkey, wkey, N)
    if mode == "stretch":
        norm = np.float32(len(order) // 2)
    else:
        rowsum = np.zeros(N)
        for r in range(N):
            s = 0.0
            for p in range(rowptr[r], rowptr[r + 1]):
                dd = X[r] - X[col[p]]
                s = s + float(w[p]) * float(_dot(dd, dd))
            rowsum[r] = s
        norm = np.float32(tree_sum(rowsum) * 0.5)
    stats = np.array([int(out.sum()), int(bad.sum()), int(is_self.sum()), len(order)], np.int32)
    return dict(rowptr=rowptr, col=col, w=w, norm=norm, mass=None, stats=stats)


def apply(val, idx, V):
    """Y = Pi V in float64 (slots with idx outside [0, M) add nothing)."""
    val, idx, V = np.asarray(val, np.float64), np.asarray(idx, np.int64), np.asarray(V, np.float64)
    ok = (idx >= 0) & (idx < len(V))
    return ((val * ok)[..., None] * V[np.where(ok, idx, 0)]).sum(1)


def energy(Y, op, grad_of=None):
    """E = 1/2 sum w |y_i - y_j|^2 over the CSR entries, in float64 (Y as given: feed the fp32 Y of ops.apply to judge the kernel);
    S = 1/2 sum |w| |y_i - y_j|^2; resid (N,C) = 2 sum_row w (y_i - y_j).  grad_of = (idx (N,k), V (M,C)) adds g (N,k) =
    resid_i . V[idx] (0 for idx outside [0, M)) and its scale A (N,k) = sum_c |resid|_c-wise bound (2 sum |w| |dy_c|) . |V[idx]|."""
    Y = np.asarray(Y, np.float64)
    N = len(Y)
    rowptr, col, w = op["rowptr"], np.asarray(op["col"], np.int64), np.asarray(op["w"], np.float64)
    used = int(rowptr[N])
    rows = np.repeat(np.arange(N), np.diff(rowptr))
    c, wv = col[:used], w[:used]
    ok = (c >= 0) & (c < N)
    rows, c, wv = rows[ok], c[ok], wv[ok]
    d = Y[rows] - Y[c]
    out = dict(E=0.5 * float((wv * (d * d).sum(1)).sum()), S=0.5 * float((np.abs(wv) * (d * d).sum(1)).sum()))
    resid, rabs = np.zeros_like(Y), np.zeros_like(Y)
    np.add.at(resid, rows, 2.0 * wv[:, None] * d)
    np.add.at(rabs, rows, 2.0 * np.abs(wv)[:, None] * np.abs(d))
    out["resid"] = resid
    if grad_of is not None:
        idx, V = np.asarray(grad_of[0], np.int64), np.asarray(grad_of[1], np.float64)
        okm = (idx >= 0) & (idx < len(V))
        Vg = V[np.where(okm, idx, 0)] * okm[..., None]
        out["g"] = (resid[:, None, :] * Vg).sum(-1)
        out["A"] = (rabs[:, None, :] * np.abs(Vg)).sum(-1)
    return out


def energy_of_map(val, idx, V, op):
    """The whole term in float64 from (val, idx): Y = Pi V without the fp32 rounding of ops.apply (for finite differences)."""
    return energy(apply(val, idx, V), op)["E"]


def dense_laplacian(op, N):
    """L (N,N) float64 with E = 1/2 tr(Y^T L Y) ... as x^T L x = 1/2 sum w (x_i - x_j)^2: L = D - A from the multiset of entries."""
    L = np.zeros((N, N))
    used = int(op["rowptr"][N])
    rows = np.repeat(np.arange(N), np.diff(op["rowptr"]))
    for r, c, w in zip(rows, op["col"][:used], op["w"][:used].astype(np.float64)):
        if 0 <= c < N:
            L[r, r] += 0.5 * w
            L[c, c] += 0.5 * w
            L[r, c] -= 0.5 * w
            L[c, r] -= 0.5 * w
    return L


# ---- meshes and plantings
def grid_mesh(nx, ny, noise=0.0, seed=0, scale=1.0):
    """An nx x ny vertex grid of right triangles in the plane z = 0 (integer coordinates x scale), optional Gaussian noise."""
    xs, ys = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    V = np.stack([xs.ravel(), ys.ravel(), np.zeros(nx * ny)], 1).astype(np.float64) * scale
    if noise:
        V = V + noise * np.random.default_rng(seed).standard_normal(V.shape)
    vid = lambda a, b: a * ny + b   # noqa: E731
    faces = []
    for a in range(nx - 1):
        for b in range(ny - 1):
            faces.append((vid(a, b), vid(a + 1, b), vid(a, b + 1)))
            faces.append((vid(a + 1, b), vid(a + 1, b + 1), vid(a, b + 1)))
    return V.astype(np.float32), np.array(faces, np.int32)


def interior(nx, ny):
    m = np.zeros((nx, ny), bool)
    m[1:-1, 1:-1] = True
    return m.ravel()


def builder_bounds(op):
    """|dw| <= 2^-23 |w| + 2^-40 |u||v| / |u x v| for every entry (mesh operators)."""
    return 2.0 ** -23 * np.abs(op["w"].astype(np.float64)) + 2.0 ** -40 * op["cot_scale"]


def loss_bound(ref):
    return 2.0 ** -23 * abs(ref["E"]) + 2.0 ** -40 * ref["S"]


def grad_bound(ref):
    return 2.0 ** -23 * np.abs(ref["g"]) + 2.0 ** -40 * ref["A"]
