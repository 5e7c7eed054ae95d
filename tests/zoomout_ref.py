"""The ZoomOut entries' definitions in float64 numpy (dvm_fmap_from_pmap_f64, dvm_fmap_embed_f64, dvm_spectral_nn_f64,
dvm_fmap_to_pmap_f64, dvm_zoomout_f64): what include/dvm.h states, restated, and the planted families the tests run on.  Shared by
tests/test_zoomout_ref_cpu.py and tests/test_gpu_zoomout.py; a plain module, like eigenbasis_ref.py.

  X has N vertices, Y has M; Phi_X (N,K), Phi_Y (M,K); a point map T (N,) into Y; C (k,k) with Phi_X[:, :k] C ~ Phi_Y[T, :k]
  d(i,j)   = (..((t_0 t_0) + t_1 t_1) + ..),  t_c = E[j,c] - A[i,c], c ascending, every operation rounded on its own (dist_seq)
  T[i]     = argmin_j d(i,j), ties to the lowest j, a NaN distance counts as +inf, a row of +inf returns 0
  E        = Phi_Y[:, :k] C^T
  adjoint  : C = Phi_X[:, :k]^T diag(m) Phi_Y[T, :k]   (a mass that is not positive and finite counts as 0)
  lstsq    : C = pinv(Phi_X[:, :k]) Phi_Y[T, :k]
  a row with T[i] outside [0, M) is a zero row of Phi_Y[T]"""
import numpy as np

import dirichlet_term_ref as D
import eigenbasis_ref as R
import mesh_geodesic_ref as G


# ---------------------------------------------------------------- the definitions
def dist_seq(A, E):
    """d (N,M): the squared distances summed coordinate by coordinate, one rounded operation at a time."""
    A, E = np.asarray(A, np.float64), np.asarray(E, np.float64)
    t = E[None, :, 0] - A[:, None, 0]
    d = t * t
    for c in range(1, A.shape[1]):
        t = E[None, :, c] - A[:, None, c]
        d = d + t * t
    return d


def spectral_nn(A, E):
    """-> T (N,) int32, dmin (N,)"""
    with np.errstate(invalid="ignore", over="ignore"):
        d = dist_seq(A, E)
    d = np.where(np.isnan(d), np.inf, d)
    T = np.argmin(d, axis=1)
    return T.astype(np.int32), d[np.arange(len(T)), T]


def gram_nn(A, E):
    """The same search by |a|^2 - 2 a.e + |e|^2 in float64: what the near-tie family defeats."""
    A, E = np.asarray(A, np.float64), np.asarray(E, np.float64)
    return np.argmin((A * A).sum(1)[:, None] - 2.0 * (A @ E.T) + (E * E).sum(1)[None, :], axis=1)


def embed(phi_y, C):
    k = C.shape[0]
    return phi_y[:, :k] @ C.T


def gathered(phi_y, T, k):
    """Phi_Y[T, :k] with zero rows where T is outside [0, M), and the number of those rows."""
    T = np.asarray(T, np.int64)
    ok = (T >= 0) & (T < len(phi_y))
    g = np.where(ok[:, None], phi_y[np.where(ok, T, 0), :k], 0.0)
    return g, int((~ok).sum())


def clean_mass(mass, N):
    m = np.ones(N) if mass is None else np.asarray(mass, np.float32).astype(np.float64)
    return np.where(np.isfinite(m) & (m > 0), m, 0.0)


def from_pmap(phi_x, mass, phi_y, T, k, solve="adjoint"):
    """-> C (k,k), the number of entries of T outside [0, M)"""
    g, outside = gathered(phi_y, T, k)
    if solve == "adjoint":
        return phi_x[:, :k].T @ (clean_mass(mass, len(phi_x))[:, None] * g), outside
    return np.linalg.lstsq(phi_x[:, :k], g, rcond=None)[0], outside


def to_pmap(phi_x, phi_y, C):
    return spectral_nn(phi_x[:, :C.shape[0]], embed(phi_y, C))[0]


def zoomout(phi_x, mass, phi_y, T0, k_init, k_final, k_step=1, n_inter=1, solve="adjoint"):
    """The loop -> C (k_final,k_final), T (the map that produced C), the nearest-neighbour steps run."""
    T, steps = np.asarray(T0, np.int32), 0
    for k in range(k_init, k_final, k_step):
        for _ in range(n_inter):
            T = to_pmap(phi_x, phi_y, from_pmap(phi_x, mass, phi_y, T, k, solve)[0])
            steps += 1
    return from_pmap(phi_x, mass, phi_y, T, k_final, solve)[0], T, steps


# ---------------------------------------------------------------- planted families
def near_tie(N, M, k, seed, plant=(), dup=()):
    """Rows whose pairwise squared distances are exact multiples of 2^-40 far below 2^13: base = 256 * integers in [-4, 4] (1,k),
    A and E = base + integers in [-8, 8] * 2^-20.  plant: (i, j) pairs, E[j] = A[i] (distance 0); dup: (j, j2) pairs, E[j2] = E[j]
    afterwards (equal target rows: the lower index must win).  -> A (N,k), E (M,k), the
    expected T (N,) by integer arithmetic (lowest index on a tie) and the exact distances dI * 2^-40 (N,M)."""
    rng = np.random.default_rng(seed)
    base = 256 * rng.integers(-4, 5, (1, k))
    a, e = rng.integers(-8, 9, (N, k)), rng.integers(-8, 9, (M, k))
    for i, j in plant:
        e[j] = a[i]
    for j, j2 in dup:
        e[j2] = e[j]
    dI = ((e[None, :, :] - a[:, None, :]) ** 2).sum(-1)
    A, E = base + a * 2.0 ** -20, base + e * 2.0 ** -20
    return A, E, np.argmin(dI, axis=1).astype(np.int32), dI * 2.0 ** -40


def basis(verts, faces, K):
    """The first K eigenpairs of a mesh's cotangent problem, dense, in float64 -> phi (N,K) with Phi^T M Phi = I, mass (N,) fp32"""
    op = D.mesh_laplacian(np.asarray(verts, np.float32), faces)
    _, Y = R.dense(op, op["mass"], K)
    return R.operator(op, op["mass"])[1][:, None] * Y, op["mass"]


def permuted_copy(verts, faces, seed):
    """The same mesh with its vertices renumbered: vertex j of the copy is vertex perm[j] of the original -> verts, faces, and
    the ground-truth map T (N,), T[i] = the copy's number of original vertex i."""
    perm = np.random.default_rng(seed).permutation(len(verts))
    inv = np.argsort(perm)
    return verts[perm], inv[np.asarray(faces)].astype(np.int32), inv.astype(np.int32)


def planted_meshes(name):
    """The two planted-permutation shapes -> verts (N,3), faces"""
    if name == "grid20":
        return G.grid_mesh(20, jitter=0.3, seed=1)
    if name == "ico2":
        v, f = G.icosphere(2)
        v = v * np.array([1.0, 1.3, 1.7]) + 0.02 * (np.random.default_rng(3).random(v.shape) - 0.5)
        return v, f
    raise KeyError(name)


def corrupted(T, M, share, seed):
    """T with `share` of its entries replaced by random indices into [0, M)"""
    rng = np.random.default_rng(seed)
    T = np.array(T, np.int32)
    at = rng.random(len(T)) < share
    T[at] = rng.integers(0, M, int(at.sum()))
    return T


def non_isometric_pair():
    """grid_mesh(24) against a differently jittered copy stretched 1.3 times: same connectivity, the identity is the true map"""
    vx, f = G.grid_mesh(24, jitter=0.3, seed=1)
    vy, _ = G.grid_mesh(24, jitter=0.3, seed=7, stretch=1.3)
    return vx, vy, f


def map_error(T, verts_y, T_true):
    """the mean Euclidean distance on Y between a map's images and the true ones"""
    return float(np.linalg.norm(verts_y[np.asarray(T, np.int64)] - verts_y[np.asarray(T_true, np.int64)], axis=1).mean())
