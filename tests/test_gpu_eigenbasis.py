"""dvm_eigenbasis_f64 / dvm_basis_project_f64 / models.loss.functional_map on the MI355X against tests/eigenbasis_ref.py.
Every assertion recomputes A, beta and the residuals in numpy from the INPUTS (the operator and mass the solver was given) and the
RETURNED pairs; nothing is read from the code under test but its outputs.  The bars (profiles/notes_eigenbasis.md):
  residuals      |res - res_numpy| <= 2^-40, and res <= tol where info[1] == 1
  eigenvalues    |evals_j - lambda_j| <= (res_j + 2^-40) beta                  (the symmetric residual bound + float64 slack)
  orthonormality max |Phi^T M Phi - I| <= (k + guard) N 2^-52                  (Cholesky-QR twice, then an orthogonal rotation)
  subspaces      the part of M^1/2 phi_j outside the reference invariant subspace of its cluster <= 1e-6 + 2^-40, clusters cut at
                 gaps >= 1e6 sqrt(k) tol beta on the first k + guard + 2 reference values                        (Davis-Kahan)"""
import ctypes

import numpy as np
import pytest

pytest.importorskip("scipy")
torch = pytest.importorskip("torch")

import eigenbasis_ref as R  # noqa: E402
import mesh_geodesic_ref as G  # noqa: E402

pytestmark = pytest.mark.gpu
SLACK = 2.0 ** -40
TOL = 1e-10


def _ops():
    from dvm import ops
    return ops


def mesh_operator(verts, faces):
    """ops.mesh_laplacian of one mesh or a batch of meshes that share `faces` -> GraphOperator on the device"""
    ops = _ops()
    v = torch.as_tensor(np.asarray(verts, np.float32)).cuda()
    if v.dim() == 2:
        v = v[None]
    return ops.mesh_laplacian(v, torch.as_tensor(np.asarray(faces, np.int32)).cuda())


def element(op, b):
    """batch element b of a GraphOperator as the reference's dict and its mass"""
    d = dict(rowptr=op.rowptr[b].cpu().numpy(), col=op.col[b].cpu().numpy(), w=op.w[b].cpu().numpy())
    return d, None if op.mass is None else op.mass[b].cpu().numpy()


def sliced(op, b):
    ops = _ops()
    return ops.GraphOperator(op.rowptr[b:b + 1].contiguous(), op.col[b:b + 1].contiguous(), op.w[b:b + 1].contiguous(), op.norm[b:b + 1],
                             None if op.mass is None else op.mass[b:b + 1].contiguous(), op.stats[b:b + 1])


def check_element(op_np, mass, k, guard, eb, b, converged=True, min_clusters=0, inactive=0, tol=TOL):
    """every per-case assertion of the issue for batch element b of the result eb; converged=None accepts either outcome"""
    evals, phi = eb.evals[b].cpu().numpy(), eb.evecs[b].cpu().numpy()
    res, info = eb.res[b].cpu().numpy(), eb.info[b].cpu().numpy()
    A, s, beta, active = R.operator(op_np, mass)
    N = len(s)
    assert evals.shape == (k,) and phi.shape == (N, k) and res.shape == (k,)
    assert np.isfinite(evals).all() and np.isfinite(phi).all() and np.isfinite(res).all()
    print("iterations %d converged %d inactive %d applications %d beta %.6g max res %.3e" % (*info, beta, res.max()))
    if converged is not None:
        assert info[1] == int(converged), info
    assert info[0] >= 1 and info[2] == inactive == int((~active).sum())
    assert np.all(np.diff(evals) >= 0)
    # inactive rows are exactly 0; the rest is judged on the active problem
    assert np.all(phi[~active] == 0.0)
    Y = phi[active] / s[active][:, None]
    res_np = R.residuals(A, beta, evals, Y)
    assert np.abs(res - res_np).max() <= SLACK, (res, res_np)
    if info[1] == 1:
        assert res.max() <= tol, res
    nref = min(k + guard + 2, len(A))
    lam, Yref = R.dense(op_np, mass, nref)
    assert np.all(np.abs(evals - lam[:k]) <= (res + SLACK) * beta), (evals, lam[:k])
    m64 = np.ones(N) if mass is None else mass.astype(np.float64)
    gram = phi.T @ (np.where(active, m64, 0.0)[:, None] * phi)
    assert np.abs(gram - np.eye(k)).max() <= (k + guard) * N * 2.0 ** -52
    cl = R.clusters(lam, 1e6 * np.sqrt(k) * tol * beta)
    assert sum(1 for a, _ in cl if a < k) >= min_clusters, cl
    for a, e in cl:
        U = Yref[:, a:e]
        for j in range(a, min(e, k)):
            out = Y[:, j] - U @ (U.T @ Y[:, j])
            assert np.linalg.norm(out) <= 1e-6 + SLACK, (j, (a, e), np.linalg.norm(out))
    assert R.sign_rule(phi)


_cache = {}


def solved(name):
    """(op, k, guard, result) of a named case, computed once"""
    if name in _cache:
        return _cache[name]
    ops = _ops()
    kw = {}
    if name == "ico2":
        op, k = mesh_operator(*G.icosphere(2)), 30
    elif name == "two18":
        op, k = mesh_operator(*G.two_spheres(2)), 18
    elif name == "two20":
        op, k, kw = mesh_operator(*G.two_spheres(2)), 20, dict(degree=40, max_iter=100)
    elif name == "grid":
        op, k = mesh_operator(*G.grid_mesh(24, jitter=0.2, seed=1)), 30
    elif name == "grid_holes":
        v, f = G.grid_mesh(24, jitter=0.2, seed=1)
        n, mid = len(v), len(v) // 2
        # three unreferenced vertices: new index 0, the middle, the last
        v2 = np.concatenate([[[5.0, 5.0, 5.0]], v[:mid], [[6.0, 5.0, 5.0]], v[mid:], [[7.0, 5.0, 5.0]]])
        remap = np.concatenate([1 + np.arange(mid), 2 + np.arange(mid, n)])
        op, k = mesh_operator(v2, remap[f]), 30
    elif name in ("ring9", "ring10"):
        a = 2.0 * np.pi * np.arange(64) / 64
        xyz = torch.as_tensor(np.stack([np.cos(a), np.sin(a), np.zeros(64)], 1).astype(np.float32)).cuda()[None]
        op, k = ops.knn_laplacian(xyz, ops.knn_cdist(xyz, xyz, 3), mode="uniform"), int(name[4:])
    elif name == "batch":
        vs = [G.grid_mesh(16, jitter=0.3, seed=sd) for sd in (1, 2, 3)]
        op, k = mesh_operator(np.stack([v for v, _ in vs]), vs[0][1]), 12
    else:
        raise KeyError(name)
    eb = ops.eigenbasis(op, k, guard=8, **kw)
    _cache[name] = (op, k, 8, eb)
    return _cache[name]


@pytest.mark.parametrize("name,converged,inactive,min_clusters", [("ico2", True, 0, 4), ("two18", True, 0, 3), ("two20", None, 0, 4),
                                                                  ("grid", True, 0, 4), ("grid_holes", True, 3, 4)])
def test_mesh_cases(name, converged, inactive, min_clusters):
    """cases 1-4: the block edge cuts the l = 5 shell; a 2-dimensional null space (and at k = 20 a cut near-degenerate cluster,
    where either outcome is accepted); an open boundary with negative cotangents; three vertices of mass 0.  The reference's
    partition has at least 4 clusters that begin inside the first k — except on two spheres at k = 18, where the shells l = 0, 1, 2
    hold 2 + 6 + 10 = 18 values: exactly 3 clusters lie inside the first 18 and the fourth begins at index 18 (a fact of the
    reference spectrum alone, whatever the solver returns), so 3 is asserted there."""
    op, k, guard, eb = solved(name)
    op_np, mass = element(op, 0)
    check_element(op_np, mass, k, guard, eb, 0, converged=converged, min_clusters=min_clusters, inactive=inactive)
    if name == "grid_holes":
        n = op.N
        assert np.all(eb.evecs[0].cpu().numpy()[[0, (n - 3) // 2 + 1, n - 1]] == 0.0)
        assert np.array_equal(mass[[0, (n - 3) // 2 + 1, n - 1]], np.zeros(3, np.float32))


@pytest.mark.parametrize("name", ["ring9", "ring10"])
def test_ring_closed_form(name):
    """case 5: the ring operator of ops.knn_laplacian (mass None) against 4 - 4 cos(2 pi j / N); k = 9 ends on a pair, k = 10 cuts one"""
    op, k, guard, eb = solved(name)
    op_np, mass = element(op, 0)
    assert mass is None
    ref = R.ring_operator(64)
    assert np.array_equal(R.operator(op_np, None)[0], R.operator(ref, None)[0])
    check_element(op_np, None, k, guard, eb, 0)
    res = eb.res[0].cpu().numpy()
    assert np.all(np.abs(eb.evals[0].cpu().numpy() - R.ring_eigenvalues(64, k)) <= (res + SLACK) * 8.0)


def _bytes(eb, b=None):
    pick = (lambda t: t) if b is None else (lambda t: t[b])
    return [pick(t).cpu().numpy().tobytes() for t in (eb.evals, eb.evecs, eb.res, eb.info)]


def test_batch_elements_alone_and_again():
    """case 6: B = 3 jittered copies of one connectivity: every element passes, matches the same element run alone bit for bit,
    and a second run of the batch gives identical bytes"""
    ops = _ops()
    op, k, guard, eb = solved("batch")
    for b in range(3):
        check_element(*element(op, b), k, guard, eb, b)
        alone = ops.eigenbasis(sliced(op, b), k, guard=guard)
        assert _bytes(alone, 0) == _bytes(eb, b), b
    assert _bytes(ops.eigenbasis(op, k, guard=guard)) == _bytes(eb)


def test_invalid_arguments():
    """every limit exceeded by one: a size query of 0 where the query takes the size, DVM_EINVAL from the entry, DvmError from ops,
    and outputs that stay untouched"""
    from dvm import _lib
    ops = _ops()
    lib = _lib.load()
    op, k, guard, _ = solved("ico2")
    N, Ecap = op.N, op.Ecap
    assert ops.eigenbasis_max_block() == 128
    sizes = dict(B=1, N=N, Ecap=Ecap, k=k, guard=guard)
    assert lib.dvm_eigenbasis_workspace_bytes(*sizes.values()) > 0
    sentinel = -7.5
    f64 = dict(dtype=torch.float64, device="cuda")
    outs = [torch.full((k,), sentinel, **f64), torch.full((N, k), sentinel, **f64), torch.full((k,), sentinel, **f64),
            torch.full((4,), -7, dtype=torch.int32, device="cuda")]
    ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    bad = [dict(k=0), dict(guard=0), dict(k=121, guard=8), dict(N=37), dict(degree=0), dict(degree=257), dict(max_iter=0),
           dict(tol=0.0), dict(N=(1 << 24) + 1), dict(B=65536), dict(Ecap=0)]
    for change in bad:
        a = dict(sizes, degree=20, max_iter=200, tol=TOL)
        a.update(change)
        if set(change) & set(sizes):
            assert lib.dvm_eigenbasis_workspace_bytes(a["B"], a["N"], a["Ecap"], a["k"], a["guard"]) == 0, change
        rc = lib.dvm_eigenbasis_f64(op.rowptr.data_ptr(), op.col.data_ptr(), op.w.data_ptr(), op.mass.data_ptr(), a["B"], a["N"], a["Ecap"],
                                    a["k"], a["guard"], a["degree"], a["max_iter"], ctypes.c_double(a["tol"]), *[t.data_ptr() for t in outs],
                                    ws.data_ptr(), ws.numel(), None)
        assert rc == -1 and b"dvm_eigenbasis_f64" in lib.dvm_last_error(), (change, rc)
    torch.cuda.synchronize()
    assert all(bool((t == (sentinel if t.dtype == torch.float64 else -7)).all()) for t in outs)
    for kw in (dict(k=0), dict(k=30, guard=0), dict(k=121, guard=8), dict(k=30, degree=0), dict(k=30, degree=257), dict(k=30, max_iter=0),
               dict(k=30, tol=0.0)):
        with pytest.raises(_lib.DvmError):
            ops.eigenbasis(op, **kw)
    assert lib.dvm_basis_project_workspace_bytes(1, N, 129, 3) == 0 and lib.dvm_basis_project_workspace_bytes(1, N, 3, 129) == 0
    with pytest.raises(_lib.DvmError):
        ops.basis_project(torch.zeros(1, N, 129, **f64), None, torch.zeros(1, N, 3, device="cuda"))


def test_too_few_active_vertices():
    """10 active vertices (a fan of 9 triangles) among 20, k + guard = 16: the call raises"""
    from dvm import _lib
    v, f = G.fan(9)
    op = mesh_operator(np.concatenate([v, 3.0 + np.arange(30.0).reshape(10, 3)]), f)
    assert int((op.mass[0] > 0).sum()) == 10
    with pytest.raises(_lib.DvmError, match="active"):
        _ops().eigenbasis(op, 8, guard=8)
    # a block of 8 in a space of 10: theta_m is a large fraction of beta, so a low degree keeps the filtered block's Gram matrix
    # inside what Cholesky factorises (profiles/notes_eigenbasis.md, "small spaces")
    eb = _ops().eigenbasis(op, 4, guard=4, degree=4)
    check_element(*element(op, 0), 4, 4, eb, 0, inactive=10)


def _basis_np(name):
    op, k, guard, eb = solved(name)
    return eb, eb.evecs[0].cpu().numpy(), eb.mass[0].cpu().numpy().astype(np.float64)


def test_functional_map_identity():
    """the identity map on icosphere(2): C = I within the orthonormality bar plus the fp32 cast of Phi"""
    from models.loss import functional_map
    eb, phi, mass = _basis_np("ico2")
    N, k = phi.shape
    val = torch.ones(1, N, 1, device="cuda")
    idx = torch.arange(N, dtype=torch.int32, device="cuda").reshape(1, N, 1)
    C = functional_map(val, idx, eb, eb)
    assert C.dtype == torch.float64 and tuple(C.shape) == (1, k, k)
    ref, S = R.functional_map(np.ones((N, 1)), np.arange(N)[:, None], phi, mass, phi)
    bound = (k + 8) * N * 2.0 ** -52 + 2.0 ** -22 * S
    assert np.all(np.abs(C[0].cpu().numpy() - np.eye(k)) <= bound)
    assert np.all(np.abs(C[0].cpu().numpy() - ref) <= 2.0 ** -22 * S)


@pytest.mark.parametrize("kind", ["permutation", "top3"])
def test_functional_map_against_definition(kind):
    """a random permutation, and a random top-3 row-stochastic Pi (the shape of the precise map's (bary, pi_idx) rows, one slot out of
    range), from icosphere(2) to a jittered copy, k2 = 30 channels: |C - C_ref| <= 2^-22 sum_i m_i |phi_a(i)| sum_s |val_is| |phi_b(idx_is)|"""
    from models.loss import functional_map
    ops = _ops()
    eb1, phi1, mass1 = _basis_np("ico2")
    if "ico2_jitter" not in _cache:
        v, f = G.icosphere(2)
        v = v + 0.02 * np.random.default_rng(5).standard_normal(v.shape)
        op2 = mesh_operator(v, f)
        _cache["ico2_jitter"] = (op2, 30, 8, ops.eigenbasis(op2, 30, guard=8))
    eb2 = _cache["ico2_jitter"][3]
    assert int(eb2.info[0, 1]) == 1
    phi2 = eb2.evecs[0].cpu().numpy()
    N, M = len(phi1), len(phi2)
    rng = np.random.default_rng(11)
    if kind == "permutation":
        idx, val = rng.permutation(M)[:N, None].astype(np.int32), np.ones((N, 1), np.float32)
    else:
        idx = np.stack([rng.permutation(M)[:3] for _ in range(N)]).astype(np.int32)
        val = rng.random((N, 3)).astype(np.float32)
        val = (val / val.sum(1, keepdims=True)).astype(np.float32)
        idx[7, 2] = M
    C = functional_map(torch.as_tensor(val).cuda()[None], torch.as_tensor(idx).cuda()[None], eb1, eb2)[0].cpu().numpy()
    ref, S = R.functional_map(val, idx, phi1, mass1, phi2)
    assert C.shape == (30, 30)
    print("max |C - ref| / bound = %.3f" % (np.abs(C - ref) / (2.0 ** -22 * S)).max())
    assert np.all(np.abs(C - ref) <= 2.0 ** -22 * S)


def test_basis_project_plain():
    """ops.basis_project alone, with and without a mass, C = 128 channels and an odd row count: against float64 numpy, bar
    2^-50 sum_i m_i |phi_a(i)| |y_ic| (float64 sums of N terms, N 2^-53 < 2^-45 here, taken generously as 2^-44)"""
    ops = _ops()
    rng = np.random.default_rng(3)
    B, N, k, C = 2, 1031, 37, 128
    phi = rng.standard_normal((B, N, k))
    Y = rng.standard_normal((B, N, C)).astype(np.float32)
    mass = rng.random((B, N)).astype(np.float32) + 0.1
    for m in (mass, None):
        out = ops.basis_project(torch.as_tensor(phi).cuda(), None if m is None else torch.as_tensor(m).cuda(), torch.as_tensor(Y).cuda())
        mm = np.ones((B, N)) if m is None else m.astype(np.float64)
        ref = np.einsum("bnk,bn,bnc->bkc", phi, mm, Y.astype(np.float64))
        S = np.einsum("bnk,bn,bnc->bkc", np.abs(phi), mm, np.abs(Y).astype(np.float64))
        assert np.all(np.abs(out.cpu().numpy() - ref) <= 2.0 ** -44 * S)
