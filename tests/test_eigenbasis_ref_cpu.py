"""The eigenbasis reference (tests/eigenbasis_ref.py) against closed forms: the ring graph's spectrum, the sphere's l = 1 shell,
the cluster split and the functional map of a permutation.  No GPU."""
import numpy as np
import pytest

pytest.importorskip("scipy")

import dirichlet_term_ref as D  # noqa: E402
import eigenbasis_ref as R  # noqa: E402
import mesh_geodesic_ref as G  # noqa: E402


def ring_points(N):
    a = 2.0 * np.pi * np.arange(N) / N
    return np.stack([np.cos(a), np.sin(a), np.zeros(N)], 1).astype(np.float32)


def test_ring_graph_pin():
    """The hand-built CSR of the ring (K = 3, uniform, N = 64) is what the list builder's reference emits for 64 points of a
    circle (the same multiset of entries per row), its matrix is 2 (2 I - S - S^T), and the spectrum is 4 - 4 cos(2 pi j / N)."""
    N = 64
    op = R.ring_operator(N)
    nbr = np.stack([np.arange(N), (np.arange(N) + 1) % N, (np.arange(N) - 1) % N], 1)
    built = D.knn_laplacian(ring_points(N), nbr, mode="uniform")
    assert np.array_equal(built["rowptr"], op["rowptr"])
    for i in range(N):
        a, b = built["rowptr"][i], built["rowptr"][i + 1]
        assert sorted(built["col"][a:b]) == list(op["col"][a:b]) and np.all(built["w"][a:b] == 1.0)
    A, s, beta, active = R.operator(op, None)
    S = np.roll(np.eye(N), 1, axis=1)
    assert np.array_equal(A, 2.0 * (2.0 * np.eye(N) - S - S.T))
    assert np.array_equal(A, R.operator(built, None)[0])
    assert active.all() and np.all(s == 1.0) and beta == 8.0
    lam, Y = R.dense(op, None, N)
    assert np.abs(lam - R.ring_eigenvalues(N, N)).max() <= 64 * 8.0 * 2.0 ** -52
    assert R.residuals(A, beta, lam, Y).max() <= 2.0 ** -45


def test_icosphere_pin():
    """On icosphere(3) eigenvalues 2-4 of the cotangent problem lie within 2 % of l (l + 1) / r^2 = 2, and the first is 0."""
    v, f = G.icosphere(3)
    op = D.mesh_laplacian(v.astype(np.float32), f)
    lam, Y = R.dense(op, op["mass"], 5)
    A, s, beta, active = R.operator(op, op["mass"])
    assert abs(lam[0]) <= 2.0 ** -40 * beta
    assert np.abs(lam[1:4] - 2.0).max() <= 0.04, lam
    assert lam[4] > 5.0
    phi = s[:, None] * Y
    assert np.abs(phi.T @ (op["mass"].astype(np.float64)[:, None] * phi) - np.eye(5)).max() <= 2.0 ** -40


def test_inactive_vertices_drop_out():
    """A vertex without faces has mass 0: it is inactive, and the active principal problem is the mesh's own."""
    v, f = G.grid_mesh(6, jitter=0.2, seed=1)
    op = D.mesh_laplacian(v.astype(np.float32), f)
    v2 = np.concatenate([[[9.0, 9.0, 9.0]], v])
    op2 = D.mesh_laplacian(v2.astype(np.float32), f + 1)
    A, _, beta, _ = R.operator(op, op["mass"])
    A2, s2, beta2, active2 = R.operator(op2, op2["mass"])
    assert not active2[0] and active2[1:].all() and s2[0] == 0.0
    assert np.array_equal(A, A2) and beta == beta2


def test_clusters():
    lam = np.array([0.0, 2.0, 2.001, 2.002, 6.0, 6.0005, 12.0])
    assert R.clusters(lam, 0.01) == [(0, 1), (1, 4), (4, 6), (6, 7)]
    assert R.clusters(lam, 5.0) == [(0, 6), (6, 7)]


def test_functional_map_of_a_permutation():
    """For a basis that spans everything and a permutation, C is orthogonal; for the identity map it is I."""
    v, f = G.icosphere(1)
    op = D.mesh_laplacian(v.astype(np.float32), f)
    N = len(v)
    lam, Y = R.dense(op, op["mass"], N)
    s = R.operator(op, op["mass"])[1]
    phi = s[:, None] * Y
    ident = np.arange(N)[:, None]
    C, S = R.functional_map(np.ones((N, 1)), ident, phi, op["mass"], phi)
    assert np.abs(C - np.eye(N)).max() <= 2.0 ** -40 and (S >= np.abs(C) - 2.0 ** -40).all()
    perm = np.random.default_rng(0).permutation(N)[:, None]
    C, _ = R.functional_map(np.ones((N, 1)), perm, phi, op["mass"], phi)
    assert np.linalg.matrix_rank(C) == N
    C, _ = R.functional_map(np.ones((N, 2)), np.stack([ident[:, 0], np.full(N, -1)], 1), phi, op["mass"], phi)
    assert np.abs(C - np.eye(N)).max() <= 2.0 ** -40
    assert R.sign_rule(np.array([[1.0, -3.0], [-1.0, 3.0]])) is False and R.sign_rule(np.array([[1.0, 3.0], [-1.0, -3.0]])) is True
