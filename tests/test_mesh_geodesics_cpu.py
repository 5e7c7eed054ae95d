"""CPU-side checks of the triangle-front mesh geodesics: the scheme itself on its float64 numpy statement (mesh_geodesic_ref.py)
against analytic distances and edge paths, and the argument handling of dvm_mesh_geodesics_f64, which happens before anything
touches a device (the pointers handed in are never dereferenced)."""
import ctypes

import numpy as np
import pytest

import mesh_geodesic_ref as R

ONE = ctypes.c_void_p(16)   # a pointer that must never be dereferenced

MESHES = {
    "grid33": (lambda: R.grid_mesh(33), R.analytic_plane),
    "grid33_jitter": (lambda: R.grid_mesh(33, jitter=0.6, seed=1), R.analytic_plane),
    "icosphere3": (lambda: R.icosphere(3), R.analytic_sphere),
}


@pytest.mark.parametrize("name", sorted(MESHES))
def test_scheme_against_analytic_and_edge_paths(name):
    """Sources 0, V/2, V-1: mean relative error <= 0.03 and <= half the edge paths'; never above the edge path; the source's own
    triangles get exactly their edge lengths."""
    make, exact_of = MESHES[name]
    verts, faces = make()
    V = len(verts)
    sources = [0, V // 2, V - 1]
    D, sweeps = R.solve(verts, faces, sources)
    E = R.edge_paths(verts, faces, sources)
    exact = exact_of(verts, sources)
    err, err_edges = R.mean_rel_error(D, exact), R.mean_rel_error(E, exact)
    print(name, "V", V, "sweeps", sweeps, "mean rel err", err.tolist(), "edge paths", err_edges.tolist(), "ratio", (err / err_edges).tolist())
    assert np.isfinite(D).all() and (D[np.arange(3), sources] == 0).all()
    assert (err <= 0.03).all()
    assert (err <= 0.5 * err_edges).all()
    assert (D <= E * (1 + 1e-9)).all()
    for row, s in zip(D, sources):
        ring = R.star_of(faces, s)
        assert len(ring) >= 2
        assert np.array_equal(row[ring], np.linalg.norm(verts[ring] - verts[s], axis=1))


def test_scheme_on_degenerate_and_disconnected_input():
    """zero-area, repeated and duplicate faces and an isolated vertex change nothing but leave that vertex at +inf; two
    components stay at +inf from each other"""
    verts, faces = R.degenerate_mesh()
    V = len(verts)
    D, _ = R.solve(verts, faces)
    clean, _ = R.solve(*R.grid_mesh(5))
    assert np.array_equal(D[:V - 1, :V - 1], clean)
    assert np.isinf(D[V - 1, :V - 1]).all() and np.isinf(D[:V - 1, V - 1]).all() and D[V - 1, V - 1] == 0
    verts, faces = R.two_spheres(1)
    D, _ = R.solve(verts, faces, [0, len(verts) - 1])
    half = len(verts) // 2
    assert np.isfinite(D[0, :half]).all() and np.isinf(D[0, half:]).all()
    assert np.isinf(D[1, :half]).all() and np.isfinite(D[1, half:]).all()


def test_entries_exported_sized_and_limited():
    from dvm import _lib
    raw = ctypes.CDLL(_lib.SO_PATH)
    for entry in ("dvm_mesh_geodesics_max_v", "dvm_mesh_geodesics_workspace_bytes", "dvm_mesh_geodesics_f64"):
        assert hasattr(raw, entry) and entry in _lib.SIGNATURES, entry
    lib = _lib.load()
    vmax = lib.dvm_mesh_geodesics_max_v()
    assert vmax == 16384
    V, F = 642, 1280
    need = 48 * 3 * F + 4 * (4 * V + 2)   # the corner table, four int32 arrays over the vertices, the flag
    got = lib.dvm_mesh_geodesics_workspace_bytes(V, F)
    assert need <= got <= need + 6 * 256   # six arrays, each rounded up to 256 bytes: CSR, nothing of size V x valence or V x V
    assert lib.dvm_mesh_geodesics_workspace_bytes(vmax, 4) > 0 and lib.dvm_mesh_geodesics_workspace_bytes(8, 0) > 0
    for bad in ((0, 4), (-1, 4), (8, -1), (vmax + 1, 4)):
        assert lib.dvm_mesh_geodesics_workspace_bytes(*bad) == 0, bad


def test_argument_validation_without_gpu():
    """every refusal that comes before a launch: the invalid-argument code (a short workspace: the library's own code for that),
    with a message that names the entry"""
    from dvm import _lib
    lib = _lib.load()
    vmax = lib.dvm_mesh_geodesics_max_v()
    enough = lib.dvm_mesh_geodesics_workspace_bytes(8, 4)

    def call(verts=ONE, faces=ONE, V=8, F=4, sources=None, S=0, D=ONE, ws=ONE, nb=enough):
        return lib.dvm_mesh_geodesics_f64(verts, faces, V, F, sources, S, D, ws, nb, None)

    def err():
        msg = lib.dvm_last_error()
        assert b"dvm_mesh_geodesics_f64" in msg
        return msg

    assert call(verts=None) == -1 and b"null pointer" in err()
    assert call(faces=None) == -1 and b"null pointer" in err()
    assert call(D=None) == -1 and b"null pointer" in err()
    assert call(V=0) == -1 and b"V=0" in err()
    assert call(F=-1) == -1 and b"F=-1" in err()
    assert call(V=vmax + 1, nb=1 << 40) == -1 and b"V=%d" % (vmax + 1) in err()
    assert call(sources=ONE, S=0) == -1 and b"S=0" in err()
    assert call(sources=ONE, S=-3) == -1 and b"S=-3" in err()
    assert call(ws=None, nb=0) == -3 and b"workspace" in err()
    assert call(nb=enough - 1) == -3 and b"workspace" in err()


def test_python_layers_refuse_without_a_mesh_or_a_device(tmp_path):
    import torch
    from dvm import ops
    from dvm._lib import DvmError
    import eval_geodesic as eg
    import models.dataset as ds
    verts, faces = R.grid_mesh(3)
    with pytest.raises(DvmError):
        ops.mesh_geodesics(torch.from_numpy(verts), torch.from_numpy(faces))   # CPU tensors: there is no host path
    with pytest.raises(ValueError, match="faces"):
        ds.cal_geo(verts, method="mesh")
    with pytest.raises(ValueError, match="method"):
        ds.cal_geo(verts, faces, method="heat")
    with pytest.raises(ValueError, match="method"):
        eg.geodesic_distmat(verts, faces, method="heat")
    with pytest.raises(ValueError, match="point clouds"):
        ds.Dataset(str(tmp_path), name="spleen", geodesics="mesh")
    with pytest.raises(ValueError, match="geodesics"):
        ds.Dataset(str(tmp_path), name="scape_r", geodesics="heat")
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="HIP device"):
            ds.cal_geo(verts, faces, method="mesh")
