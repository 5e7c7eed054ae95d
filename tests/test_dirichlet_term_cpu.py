"""CPU-side checks of the Dirichlet term: the float64 reference itself (tests/dirichlet_term_ref.py) against closed forms, central
differences and a dense Laplacian; the torch fallback of models.loss.dirichlet_term against the reference; and the argument
handling of the three C entries, which happens before anything touches a device (the pointers handed in are never dereferenced)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import dirichlet_term_ref as D

ONE = ctypes.c_void_p(16)   # a pointer that must never be dereferenced
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


class Op:
    """the fields of ops.GraphOperator, on the CPU, batch of one, from a reference dict"""

    def __init__(self, ref):
        self.rowptr = torch.from_numpy(ref["rowptr"])[None]
        self.col, self.w = torch.from_numpy(ref["col"])[None], torch.from_numpy(ref["w"])[None]
        self.norm = torch.tensor([float(ref["norm"])])
        self.mass, self.stats = None, torch.from_numpy(ref["stats"])[None]


def _random_pi(rng, N, M, k):
    idx = np.stack([rng.choice(M, k, replace=False) for _ in range(N)]).astype(np.int32)
    val = rng.random((N, k)).astype(np.float32)
    return (val / val.sum(1, keepdims=True)).astype(np.float32), idx


def _meshes():
    out = [("grid", *D.grid_mesh(5, 5)), ("noisy grid", *D.grid_mesh(5, 5, noise=0.15, seed=3))]
    g = np.load(os.path.join(GOLDEN, "meshgraph_a.npz"))
    if "faces" in g.files:
        out.append(("meshgraph_a", g["verts"].astype(np.float32), g["faces"].astype(np.int32)))
    return out


@pytest.mark.parametrize("name,verts,faces", _meshes(), ids=lambda v: v if isinstance(v, str) else "")
def test_energy_of_the_embedding_is_twice_the_area(name, verts, faces):
    """E(X) = 2 area within 1e-6 relative (the weights are fp32), and norm is that closed form."""
    op = D.mesh_laplacian(verts, faces)
    assert op["stats"][:3].tolist() == [0, 0, 0] and op["stats"][3] == 6 * len(faces)
    E = D.energy(verts, op)["E"]
    print(name, "E", E, "2 area", 2 * op["area"], "norm", float(op["norm"]))
    assert abs(E - 2 * op["area"]) <= 1e-6 * 2 * op["area"]
    assert abs(float(op["norm"]) - 2 * op["area"]) <= 2.0 ** -23 * 2 * op["area"]
    assert abs(float(op["mass"].astype(np.float64).sum()) - op["area"]) <= 1e-6 * op["area"]


def test_affine_image_of_the_flat_grid_is_exact():
    """On the flat integer grid with Y = A X, A dyadic: E = area ||A[:, :2]||_F^2 exactly, the residual exactly 0 at interior vertices."""
    verts, faces = D.grid_mesh(5, 5)
    op = D.mesh_laplacian(verts, faces)
    assert set(np.unique(op["w"][:op["rowptr"][-1]]).tolist()) == {0.0, 0.5}
    A = np.array([[1.5, -0.25, 3.0], [0.5, 2.0, -1.0], [-4.0, 0.75, 0.125]])
    Y = verts.astype(np.float64) @ A.T
    ref = D.energy(Y, op)
    assert ref["E"] == 16.0 * (A[:, :2] ** 2).sum()
    inner = D.interior(5, 5)
    assert inner.sum() == 9 and (ref["resid"][inner] == 0).all() and (ref["resid"][~inner] != 0).any()


def test_gradient_against_central_differences():
    rng = np.random.default_rng(11)
    N, M, k = 40, 30, 4
    xyz = rng.standard_normal((N, 3)).astype(np.float32)
    nbr = np.argsort(((xyz[:, None] - xyz[None]) ** 2).sum(-1), 1)[:, :6]
    op = D.knn_laplacian(xyz, nbr, "stretch")
    V = rng.standard_normal((M, 3)).astype(np.float32)
    val, idx = _random_pi(rng, N, M, k)
    g = D.energy(D.apply(val, idx, V), op, grad_of=(idx, V))["g"]
    h = 1e-5
    num = np.zeros_like(g)
    for i in range(N):
        for s in range(k):
            vp, vm = val.astype(np.float64), val.astype(np.float64)
            vp[i, s] += h
            vm[i, s] -= h
            num[i, s] = (D.energy_of_map(vp, idx, V, op) - D.energy_of_map(vm, idx, V, op)) / (2 * h)
    # E is quadratic in val: the central difference is exact up to rounding, ~ u64 E / h
    assert np.abs(num - g).max() <= 1e-7 * np.abs(g).max()


def test_reference_against_dense_laplacian_in_torch():
    rng = np.random.default_rng(5)
    verts, faces = D.grid_mesh(6, 4, noise=0.2, seed=1)
    op = D.mesh_laplacian(verts, faces)
    N = len(verts)
    L = torch.from_numpy(D.dense_laplacian(op, N))
    assert torch.equal(L, L.T) and float(L.sum(1).abs().max()) <= 1e-12
    Y = torch.from_numpy(rng.standard_normal((N, 3)))
    E = float(torch.trace(Y.T @ L @ Y))
    ref = D.energy(Y.numpy(), op)
    assert abs(E - ref["E"]) <= 1e-12 * ref["S"]
    assert float((2 * (L @ Y) - torch.from_numpy(ref["resid"])).abs().max()) <= 1e-12 * ref["S"]


@pytest.mark.parametrize("K", [1, 6])
def test_stretch_operator_normalises_the_identity_to_one(K):
    rng = np.random.default_rng(2)
    xyz = rng.standard_normal((50, 3)).astype(np.float32)
    nbr = np.argsort(((xyz[:, None] - xyz[None]) ** 2).sum(-1), 1)[:, :K + 1]   # self included, as knn_cdist returns it
    nbr[7, -1] = -1
    xyz[13] = xyz[12]                                                            # a zero distance: left out where a list names it
    op = D.knn_laplacian(xyz, nbr, "stretch")
    kept = int(op["stats"][D.STAT_KEPT])
    assert op["stats"][D.STAT_SELF] >= 48 and op["stats"][D.STAT_RANGE] == 1 and kept == op["rowptr"][-1] and float(op["norm"]) == kept / 2
    assert abs(D.energy(xyz, op)["E"] / float(op["norm"]) - 1.0) <= 1e-6
    uni = D.knn_laplacian(xyz, nbr, "uniform")
    assert abs(D.energy(xyz, uni)["E"] / float(uni["norm"]) - 1.0) <= 1e-6
    # structural symmetry: the multiset of (i, j, w) equals the multiset of (j, i, w)
    rows = np.repeat(np.arange(50), np.diff(op["rowptr"]))
    fwd = sorted(zip(rows.tolist(), op["col"][:kept].tolist(), op["w"][:kept].tolist()))
    bwd = sorted(zip(op["col"][:kept].tolist(), rows.tolist(), op["w"][:kept].tolist()))
    assert fwd == bwd


def test_leave_out_rules_and_row_order_of_the_mesh_builder():
    verts, faces = D.grid_mesh(3, 3)
    faces = np.concatenate([faces, [[0, 1, 9]], [[0, 4, 8]], [[2, 2, 5]]]).astype(np.int32)   # out of range, collinear, repeated
    op = D.mesh_laplacian(verts, faces)
    assert op["stats"].tolist() == [1, 2, 0, 6 * 8]
    assert (op["col"][48:] == -1).all() and (op["w"][48:] == 0).all()
    # row 0 belongs to face 0 = (0, 3, 1) only.  Corner 1 (at 3: a = 1, b = 0) gives candidate 3 = (0, 1), corner 2 (at 1: a = 0,
    # b = 3) candidate 4 = (0, 3): ascending candidate number puts column 1 first.  Both corners are 45 degrees: w = 1/2
    assert faces[0].tolist() == [0, 3, 1]
    assert op["rowptr"][:2].tolist() == [0, 2] and op["col"][:2].tolist() == [1, 3] and op["w"][:2].tolist() == [0.5, 0.5]


def test_torch_fallback_against_the_reference():
    import models.loss as ml
    rng = np.random.default_rng(9)
    verts, faces = D.grid_mesh(6, 5, noise=0.1, seed=4)
    ref_op = D.mesh_laplacian(verts, faces)
    N, M, k = len(verts), 23, 3
    V = rng.standard_normal((M, 3)).astype(np.float32)
    val, idx = _random_pi(rng, N, M, k)
    idx[3, 1] = M       # contributes nothing
    idx[4, 0] = -1
    ref = D.energy(D.apply(val, idx, V), ref_op, grad_of=(idx, V))
    v = torch.from_numpy(val)[None].requires_grad_(True)
    E = ml._dirichlet_term_torch(v, torch.from_numpy(idx)[None], torch.from_numpy(V)[None], Op(ref_op))
    assert E.dtype == torch.float32 and tuple(E.shape) == (1,)
    assert abs(float(E.detach()) - ref["E"]) <= 2 * D.U * abs(ref["E"]) + 1e-12 * ref["S"]
    E.sum().backward()
    assert float((v.grad[0].double() - torch.from_numpy(ref["g"])).abs().max()) <= 1e-6 * np.abs(ref["g"]).max()
    assert float(v.grad[0, 3, 1]) == 0 and float(v.grad[0, 4, 0]) == 0
    # the public function on CPU tensors takes the fallback and normalises
    got = ml.dirichlet_term(torch.from_numpy(val)[None], torch.from_numpy(idx)[None], torch.from_numpy(V)[None], Op(ref_op))
    assert abs(float(got) - ref["E"] / float(ref_op["norm"])) <= 4 * D.U * ref["E"] / float(ref_op["norm"]) + 1e-12 * ref["S"]
    raw = ml.dirichlet_term(torch.from_numpy(val)[None], torch.from_numpy(idx)[None], torch.from_numpy(V)[None], Op(ref_op), normalize=False)
    assert torch.equal(raw, E.detach())


def test_entries_exported_and_sized():
    from dvm import _lib
    raw = ctypes.CDLL(_lib.SO_PATH)
    for entry in ("dvm_mesh_laplacian_f32", "dvm_mesh_laplacian_workspace_bytes", "dvm_knn_laplacian_f32", "dvm_knn_laplacian_workspace_bytes",
                  "dvm_dirichlet_term_f32", "dvm_dirichlet_term_workspace_bytes"):
        assert hasattr(raw, entry) and entry in _lib.SIGNATURES, entry
    lib = _lib.load()
    q = lib.dvm_dirichlet_term_workspace_bytes
    B, N, M, k, C, E = 2, 300, 170, 10, 3, 6000
    assert 0 < q(B, N, M, k, C, E) <= 64 * B * N * (k + C)       # nothing of size N x N or N x M
    for bad in ((0, N, M, k, C, E), (65536, N, M, k, C, E), (B, 0, M, k, C, E), (B, N, 0, k, C, E), (B, N, M, 0, C, E), (B, N, M, 17, C, E),
                (B, N, M, k, 0, E), (B, N, M, k, 17, E), (B, N, M, k, C, 0), (B, -1, M, k, C, E)):
        assert q(*bad) == 0, bad
    assert q(1, 1, 1, 1, 1, 1) > 0 and q(65535, 8192, 8192, 16, 16, 1 << 20) > 0
    qm, qk = lib.dvm_mesh_laplacian_workspace_bytes, lib.dvm_knn_laplacian_workspace_bytes
    assert 0 < qm(2, 300, 596) <= qm(2, 300, 597) <= qm(3, 301, 597)
    assert 0 < qk(2, 300, 10, 0) <= qk(2, 300, 11, 1) <= qk(3, 301, 11, 1)
    for bad in ((0, 300, 596), (2, 0, 596), (2, 300, 0), (65536, 300, 596), (2, 24577, 596), (2, 300, 1 << 28)):
        assert qm(*bad) == 0, bad
    assert qm(1, 24576, 1) > 0
    for bad in ((0, 300, 10, 0), (2, 0, 10, 0), (2, 300, 0, 0), (2, 300, 65, 0), (2, 300, 10, 2), (2, 300, 10, -1), (2, 24577, 10, 0)):
        assert qk(*bad) == 0, bad


def test_argument_validation_without_gpu():
    from dvm import _lib
    lib = _lib.load()
    err = lib.dvm_last_error

    def term(val=ONE, idx=ONE, V=ONE, rowptr=ONE, col=ONE, w=ONE, B=1, N=8, M=8, k=4, C=3, E=40, loss=ONE, g=None, ws=None, nb=0):
        return lib.dvm_dirichlet_term_f32(val, idx, V, rowptr, col, w, B, N, M, k, C, E, loss, g, ws, nb, None)

    assert term(val=None) == -1 and b"null pointer" in err()
    for name in ("idx", "V", "rowptr", "col", "w", "loss"):
        assert term(**{name: None}) == -1 and b"null pointer" in err(), name
    assert term(B=0) == -1 and term(N=0) == -1 and term(M=0) == -1 and b"empty" in err()
    assert term(B=65536) == -1 and b"B=65536" in err()
    big = 1 << 40
    assert term(k=0, ws=ONE, nb=big) == -1 and term(k=17, ws=ONE, nb=big) == -1 and b"topk=17" in err()   # over a limit: before any launch
    assert term(C=0, ws=ONE, nb=big) == -1 and term(C=17, ws=ONE, nb=big) == -1 and b"C=17" in err()
    assert term(E=0, ws=ONE, nb=big) == -1 and b"Ecap=0" in err()
    assert term() == -3 and b"workspace" in err()   # no workspace
    assert term(ws=ONE, nb=lib.dvm_dirichlet_term_workspace_bytes(1, 8, 8, 4, 3, 40) - 1, g=ONE) == -3 and b"workspace" in err()

    def mesh(verts=ONE, faces=ONE, B=1, N=8, F=6, rowptr=ONE, col=ONE, w=ONE, norm=ONE, mass=ONE, stats=ONE, ws=None, nb=0):
        return lib.dvm_mesh_laplacian_f32(verts, faces, B, N, F, rowptr, col, w, norm, mass, stats, ws, nb, None)

    for name in ("verts", "faces", "rowptr", "col", "w", "norm", "mass", "stats"):
        assert mesh(**{name: None}) == -1 and b"null pointer" in err(), name
    assert mesh(B=0) == -1 and mesh(N=0) == -1 and mesh(F=0) == -1 and b"empty" in err()
    assert mesh(N=24577, ws=ONE, nb=big) == -1 and b"N=24577" in err()
    assert mesh(B=65536, ws=ONE, nb=big) == -1 and b"B=65536" in err()
    assert mesh() == -3 and b"workspace" in err()
    assert mesh(ws=ONE, nb=lib.dvm_mesh_laplacian_workspace_bytes(1, 8, 6) - 1) == -3

    def knn(xyz=ONE, nbr=ONE, B=1, N=8, K=4, mode=0, rowptr=ONE, col=ONE, w=ONE, norm=ONE, stats=ONE, ws=None, nb=0):
        return lib.dvm_knn_laplacian_f32(xyz, nbr, B, N, K, mode, rowptr, col, w, norm, stats, ws, nb, None)

    for name in ("xyz", "nbr", "rowptr", "col", "w", "norm", "stats"):
        assert knn(**{name: None}) == -1 and b"null pointer" in err(), name
    assert knn(B=0) == -1 and knn(N=0) == -1 and b"empty" in err()
    assert knn(K=0, ws=ONE, nb=big) == -1 and knn(K=65, ws=ONE, nb=big) == -1 and b"K=65" in err()
    assert knn(mode=2, ws=ONE, nb=big) == -1 and b"mode" in err()
    assert knn(N=24577, ws=ONE, nb=big) == -1 and b"N=24577" in err()
    assert knn() == -3 and b"workspace" in err()
    assert knn(ws=ONE, nb=lib.dvm_knn_laplacian_workspace_bytes(1, 8, 4, 0) - 1) == -3


def test_wrappers_have_no_cpu_path():
    from dvm import nn_ops, ops
    from dvm._lib import DvmError
    verts, faces = D.grid_mesh(3, 3)
    v, f = torch.from_numpy(verts)[None], torch.from_numpy(faces)
    with pytest.raises(DvmError):
        ops.mesh_laplacian(v, f)
    with pytest.raises(DvmError):
        ops.knn_laplacian(v, torch.zeros(1, 9, 2, dtype=torch.int32))
    with pytest.raises(ValueError):
        ops.knn_laplacian(v, torch.zeros(1, 9, 2, dtype=torch.int32), mode="cotan")
    op = Op(D.mesh_laplacian(verts, faces))
    val, idx = torch.ones(1, 9, 1), torch.zeros(1, 9, 1, dtype=torch.int32)
    with pytest.raises(DvmError):
        ops.dirichlet_term(val, idx, v, op)
    with pytest.raises(DvmError):
        nn_ops.dirichlet_term(val.clone().requires_grad_(True), idx, v, op)
    with pytest.raises(ValueError, match="V is data"):
        nn_ops.dirichlet_term(val, idx, v.clone().requires_grad_(True), op)


def test_criterion_switch_defaults_off_and_driver_knows_it(capsys):
    import inspect

    import models.loss as ml
    import train_driver
    for cls in (ml.GraphDeformLoss_Neural, ml.GraphDeformLoss_Neural_Partial):
        crit = cls()
        assert crit.w_dirichlet == 0 and crit.dirichlet_mode == "stretch" and crit.dirichlet_loss == 0
        assert "w_dirichlet" not in inspect.signature(cls.__init__).parameters
    with pytest.raises(SystemExit) as e:
        train_driver.main(["--help"])
    assert e.value.code == 0
    out = capsys.readouterr().out
    assert "--w-dirichlet" in out and "--dirichlet-mode" in out
