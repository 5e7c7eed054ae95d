"""The eigenbasis entries' definitions in float64 numpy / SciPy (dvm_eigenbasis_f64, dvm_basis_project_f64, functional_map): what
include/dvm.h states, restated.  The GPU tests recompute everything they assert from the inputs and the returned pairs with this file.

An operator is a dict as in dirichlet_term_ref: rowptr (N+1,), col / w (Ecap,); mass (N,) float32 or None (1 everywhere).
  active     mass finite and > 0;  an entry whose column lies outside [0, N) or is inactive contributes nothing
  (L x)_i  = sum over the entries e of row i of w_e (x_i - x_col(e))
  A        = S L S,  S = diag(s),  s_i = m_i^-1/2 on active rows;  phi = s * y,  Phi^T M Phi = I,  inactive rows of phi are 0
  beta     = max over active i of s_i^2 (|sum_e w_e| + sum_e |w_e|)      (a Gershgorin bound of A)
  res_j    = |A y_j - theta_j y_j|_2 / beta"""
import numpy as np

SLACK = 2.0 ** -40


def operator(op, mass=None):
    """-> A (Na,Na) dense float64 on the active vertices, s (N,) (0 on inactive rows), beta, active (N,) bool."""
    rowptr = np.asarray(op["rowptr"], np.int64)
    N = len(rowptr) - 1
    col, w = np.asarray(op["col"], np.int64), np.asarray(op["w"], np.float32).astype(np.float64)
    m = np.ones(N) if mass is None else np.asarray(mass, np.float32).astype(np.float64)
    active = np.isfinite(m) & (m > 0)
    s = np.zeros(N)
    s[active] = 1.0 / np.sqrt(m[active])
    used = int(rowptr[N])
    rows = np.repeat(np.arange(N), np.diff(rowptr))
    c, wv = col[:used], w[:used]
    ok = (c >= 0) & (c < N)
    ok &= active[np.where(ok, c, 0)] & active[rows]
    rows, c, wv = rows[ok], c[ok], wv[ok]
    L = np.zeros((N, N))
    np.add.at(L, (rows, rows), wv)
    np.add.at(L, (rows, c), -wv)
    rs, ra = np.zeros(N), np.zeros(N)
    np.add.at(rs, rows, wv)
    np.add.at(ra, rows, np.abs(wv))
    beta = float((s * s * (np.abs(rs) + ra))[active].max())
    A = (s[:, None] * L * s[None, :])[np.ix_(active, active)]
    return A, s, beta, active


def dense(op, mass, k):
    """The first k eigenpairs of the active principal problem by scipy.linalg.eigh -> (evals (k,), Y (Na,k) orthonormal)."""
    from scipy.linalg import eigh
    A = operator(op, mass)[0]
    lam, Y = eigh(0.5 * (A + A.T))
    return lam[:k], Y[:, :k]


def clusters(evals_ref, delta_min):
    """The reference spectrum split where consecutive gaps are at least delta_min -> list of (first, last + 1) index ranges."""
    cuts = [0] + [i + 1 for i in range(len(evals_ref) - 1) if evals_ref[i + 1] - evals_ref[i] >= delta_min] + [len(evals_ref)]
    return list(zip(cuts[:-1], cuts[1:]))


def residuals(A, beta, evals, Y):
    """res_j of the pairs (evals_j, Y[:, j]) on the active problem."""
    return np.linalg.norm(A @ Y - Y * np.asarray(evals)[None, :], axis=0) / beta


def sign_rule(phi):
    """Whether every column's entry of largest magnitude (lowest index on a tie) is positive."""
    i = np.argmax(np.abs(phi), axis=0)
    return bool((phi[i, np.arange(phi.shape[1])] > 0).all())


def functional_map(val, idx, phi_src, mass_src, phi_tgt):
    """C (k1,k2) = Phi1^T M1 (Pi Phi2) in float64 (slots with idx outside [0, M) add nothing) and the bound's scale
    S_ab = sum_i m_i |phi_a(i)| sum_s |val_is| |phi_b(idx_is)|."""
    val, idx = np.asarray(val, np.float64), np.asarray(idx, np.int64)
    M = len(phi_tgt)
    ok = (idx >= 0) & (idx < M)
    g = phi_tgt[np.where(ok, idx, 0)]
    PiPhi = ((val * ok)[..., None] * g).sum(1)
    PiAbs = ((np.abs(val) * ok)[..., None] * np.abs(g)).sum(1)
    m = np.ones(len(phi_src)) if mass_src is None else np.asarray(mass_src, np.float64)
    return phi_src.T @ (m[:, None] * PiPhi), np.abs(phi_src).T @ (m[:, None] * PiAbs)


def ring_operator(N):
    """The CSR the list builder emits for a ring of N points with K = 3 (self and both neighbours), uniform mode: every row holds
    both neighbours twice (a mutual pair appears twice), w = 1, so L = 2 (2 I - S - S^T)."""
    rowptr = 4 * np.arange(N + 1, dtype=np.int32)
    col = np.full(2 * N * 3, -1, np.int32)
    w = np.zeros(2 * N * 3, np.float32)
    for i in range(N):
        col[4 * i:4 * i + 4] = sorted([(i - 1) % N, (i - 1) % N, (i + 1) % N, (i + 1) % N])
    w[:4 * N] = 1.0
    return dict(rowptr=rowptr, col=col, w=w, mass=None)


def ring_eigenvalues(N, k):
    """The k smallest of 4 - 4 cos(2 pi j / N), ascending."""
    return np.sort(4.0 - 4.0 * np.cos(2.0 * np.pi * np.arange(N) / N))[:k]
