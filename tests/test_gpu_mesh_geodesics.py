"""-m gpu: the triangle-front mesh geodesics on the HIP kernel (dvm_mesh_geodesics_f64, ops.mesh_geodesics, models.dataset.cal_geo,
Dataset(geodesics="mesh"), eval_geodesic.geodesic_distmat) against the float64 numpy statement of the scheme
(tests/mesh_geodesic_ref.py).

The parity bar, relative 1e-9 on the finite entries with the same +inf pattern, is derived, not tuned: the kernel evaluates the
reference's expressions in the reference's order, so the two differ only through the order of the updates, and two update orders
of the reference differ by at most 3.4e-12 on these meshes (an effect of the 2^-40 acceptance margin).  1e-9 leaves a factor 300
over that and is seven orders below the scheme's own error.  A reference is computed once per mesh and shared."""
import numpy as np
import pytest
import torch

import mesh_geodesic_ref as R

pytestmark = pytest.mark.gpu

RTOL = 1e-9

# each the smallest mesh that reaches a distinct path of the kernel
SHAPES = {
    "grid9": lambda: R.grid_mesh(9),                              # fewer vertices than threads
    "grid33_jitter": lambda: R.grid_mesh(33, jitter=0.6, seed=1),  # V = 1089, no multiple of the block size: strided tail
    "icosphere3": lambda: R.icosphere(3),                         # curved surface
    "grid17_stretch4": lambda: R.stretched_grid(17, 4),           # obtuse corners: the upwind test fails, edge fallback
    "fan64": lambda: R.fan(64),                                   # one hub of valence 64: a long CSR row
    "degenerate": R.degenerate_mesh,                              # zero-area, repeated and duplicate faces, an isolated vertex
    "two_icospheres": lambda: R.two_spheres(2),                   # +inf between components
}
_MESH, _REF = {}, {}


def mesh(name):
    if name not in _MESH:
        _MESH[name] = SHAPES[name]()
    return _MESH[name]


def reference(name):
    """(D, sweeps) of the numpy scheme for all sources of a mesh, computed once"""
    if name not in _REF:
        D, sweeps = R.solve(*mesh(name))
        D.setflags(write=False)
        _REF[name] = (D, sweeps)
    return _REF[name]


def ops_():
    from dvm import ops
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return ops


def on_device(verts, faces):
    return torch.from_numpy(np.ascontiguousarray(verts)).cuda(), torch.from_numpy(np.ascontiguousarray(faces, dtype=np.int32)).cuda()


def spy_on_op(monkeypatch):
    """-> the list every ops.mesh_geodesics call from now on appends its output to.  The kernel's updates are made in place, so two
    runs may differ by the acceptance margin's effect (some 1e-12): what a layer above the op returns is compared with the very
    output it was given, not with a second run's."""
    from dvm import ops
    seen, real = [], ops.mesh_geodesics

    def spy(*args, **kw):
        seen.append(real(*args, **kw))
        return seen[-1]

    monkeypatch.setattr(ops, "mesh_geodesics", spy)
    return seen


def check_parity(label, got, want):
    got = np.asarray(got)
    assert got.shape == want.shape and not np.isnan(got).any()
    assert np.array_equal(np.isinf(got), np.isinf(want)), "%s: the +inf patterns differ" % label
    fin = np.isfinite(want)
    err = np.abs(got[fin] - want[fin])
    scale = np.abs(want[fin])
    worst = float(np.max(err / np.where(scale > 0, scale, 1.0))) if err.size else 0.0
    print(label, "shape", got.shape, "worst relative difference %.3e" % worst, "bar %.0e" % RTOL)
    assert (err <= RTOL * scale).all()


@pytest.mark.parametrize("name", list(SHAPES))
def test_parity_all_sources(name):
    ops = ops_()
    verts, faces = mesh(name)
    want, sweeps = reference(name)
    got = ops.mesh_geodesics(*on_device(verts, faces)).cpu().numpy()
    print(name, "V", len(verts), "F", len(faces), "reference sweeps", sweeps)
    check_parity(name, got, want)
    assert (np.diag(got) == 0).all()


@pytest.mark.parametrize("name", ["grid9", "degenerate", "two_icospheres"])
def test_poisoned_memory(name):
    """D and the workspace hold NaN bytes before the call (the C entry on the test's own buffers): no NaN survives in D, and the
    values are the reference's"""
    ops_()
    from dvm import _lib
    lib = _lib.load()
    verts, faces = mesh(name)
    V, F = len(verts), len(faces)
    v, f = on_device(verts, faces)
    nb = lib.dvm_mesh_geodesics_workspace_bytes(V, F)
    assert nb > 0
    for fill in ("ff", "nan"):
        ws = torch.full(((nb + 7) // 8 * 8,), 0xFF, dtype=torch.uint8, device="cuda")
        D = torch.full((V, V), float("nan"), dtype=torch.float64, device="cuda")
        if fill == "nan":
            ws.view(torch.float64).fill_(float("nan"))
        else:
            D.view(torch.uint8).fill_(0xFF)
        rc = lib.dvm_mesh_geodesics_f64(v.data_ptr(), f.data_ptr(), V, F, None, 0, D.data_ptr(), ws.data_ptr(), ws.numel(), None)
        torch.cuda.synchronize()
        assert rc == 0, lib.dvm_last_error()
        assert not bool(torch.isnan(D).any())
        check_parity("%s poisoned with %s" % (name, fill), D.cpu().numpy(), reference(name)[0])


def test_source_list():
    """five sources, one of them twice, the last vertex among them: the rows of the all-sources call"""
    ops = ops_()
    verts, faces = mesh("icosphere3")
    V = len(verts)
    v, f = on_device(verts, faces)
    sources = [3, V - 1, 3, 0, V // 2]
    full = ops.mesh_geodesics(v, f).cpu().numpy()
    some = ops.mesh_geodesics(v, f, torch.tensor(sources, device="cuda")).cpu().numpy()
    assert some.shape == (5, V)
    check_parity("source list against the all-sources rows", some, full[sources])
    check_parity("source list against the reference", some, reference("icosphere3")[0][sources])
    check_parity("int64 list", ops.mesh_geodesics(v, f, torch.tensor(sources, device="cuda", dtype=torch.int64)).cpu().numpy(), full[sources])


def test_size_limit_and_bad_indices():
    """V = the limit (a 128 x 128 grid, 4 sources) reaches parity; one vertex more is refused on the host; face and source indices
    outside [0, V) come back as the entry's error: the kernel checks an index before it uses it, so nothing faults and a later
    call is served"""
    ops = ops_()
    from dvm import _lib
    from dvm._lib import DvmError
    lib = _lib.load()
    vmax = ops.mesh_geodesics_max_v()
    assert vmax == 16384
    verts, faces = R.grid_mesh(128)
    V = len(verts)
    assert V == vmax
    sources = [0, V // 2 + 17, V - 1, 5000]
    v, f = on_device(verts, faces)
    got = ops.mesh_geodesics(v, f, torch.tensor(sources, device="cuda")).cpu().numpy()
    want, sweeps = R.solve(verts, faces, sources)
    print("V", V, "reference sweeps", sweeps)
    check_parity("128 x 128 grid", got, want)

    big = torch.zeros(vmax + 1, 3, dtype=torch.float64, device="cuda")
    out = torch.full((1, vmax + 1), -7.0, dtype=torch.float64, device="cuda")
    ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    one = torch.zeros(1, dtype=torch.int32, device="cuda")
    rc = lib.dvm_mesh_geodesics_f64(big.data_ptr(), f.data_ptr(), vmax + 1, len(faces), one.data_ptr(), 1, out.data_ptr(), ws.data_ptr(),
                                    ws.numel(), None)
    torch.cuda.synchronize()
    assert rc == -1 and b"V=%d" % (vmax + 1) in lib.dvm_last_error()
    assert bool((out == -7.0).all())   # nothing ran
    assert lib.dvm_mesh_geodesics_workspace_bytes(vmax + 1, 4) == 0
    with pytest.raises(DvmError, match="V=%d" % (vmax + 1)):
        ops.mesh_geodesics(big, f, one)

    verts, faces = mesh("grid9")
    V = len(verts)
    v, f = on_device(verts, faces)
    for bad in (V, -1, 1 << 30, -(1 << 31)):
        fb = f.clone()
        fb[5, 1] = bad
        with pytest.raises(DvmError, match="face"):
            ops.mesh_geodesics(v, fb)
        with pytest.raises(DvmError, match="source"):
            ops.mesh_geodesics(v, f, torch.tensor([0, bad, 3], dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()
    check_parity("grid9 after the refused calls", ops.mesh_geodesics(v, f).cpu().numpy(), reference("grid9")[0])


@pytest.mark.parametrize("name,exact_of", [("icosphere3", R.analytic_sphere), ("grid33", R.analytic_plane)])
def test_analytic_accuracy_through_the_kernel(name, exact_of):
    """the CPU file's conditions on the kernel's output: mean relative error <= 0.03 and <= half the edge paths'"""
    ops = ops_()
    verts, faces = R.grid_mesh(33) if name == "grid33" else mesh(name)
    V = len(verts)
    sources = [0, V // 2, V - 1]
    D = ops.mesh_geodesics(*on_device(verts, faces), torch.tensor(sources, device="cuda")).cpu().numpy()
    E = R.edge_paths(verts, faces, sources)
    exact = exact_of(verts, sources)
    err, err_edges = R.mean_rel_error(D, exact), R.mean_rel_error(E, exact)
    print(name, "mean rel err", err.tolist(), "edge paths", err_edges.tolist(), "ratio", (err / err_edges).tolist())
    assert (err <= 0.03).all()
    assert (err <= 0.5 * err_edges).all()
    assert (D <= E * (1 + 1e-9)).all()


def test_cal_geo_methods(monkeypatch):
    """method="mesh" is the float32 cast of the symmetrised op output, exactly symmetric, with +inf bridged; the default and
    method="graph" give the same bits, with and without faces"""
    ops_()
    import models.dataset as ds
    seen = spy_on_op(monkeypatch)
    verts, faces = mesh("icosphere3")
    got = ds.cal_geo(verts, faces, method="mesh")
    assert len(seen) == 1 and tuple(seen[0].shape) == (len(verts), len(verts)) and seen[0].dtype == torch.float64
    D = seen[0]
    check_parity("the op's output inside cal_geo", D.cpu().numpy(), reference("icosphere3")[0])
    want = ((D + D.t()) / 2).cpu().numpy().astype(np.float32)
    assert got.dtype == torch.float32 and np.array_equal(got.numpy(), want)
    assert torch.equal(got, got.t())
    asym = float(((D - D.t()).abs() / (D + D.t()).clamp_min(1e-300)).max())
    print("asymmetry |D - D^T| / (D + D^T), max: %.3e" % asym)
    assert torch.equal(ds.cal_geo(verts, faces), ds.cal_geo(verts, faces, method="graph"))
    assert torch.equal(ds.cal_geo(verts), ds.cal_geo(verts, method="graph"))
    assert len(seen) == 1   # the default never reaches the new op
    assert float((got - ds.cal_geo(verts, faces)).max()) <= 0   # never above the edge paths
    verts2, faces2 = mesh("two_icospheres")
    bridged = ds.cal_geo(verts2, faces2, method="mesh")
    half = len(verts2) // 2
    assert bool(torch.isfinite(bridged).all())
    eu = np.linalg.norm(verts2[:half, None] - verts2[None, half:], axis=-1).astype(np.float32)
    assert np.array_equal(bridged[:half, half:].numpy(), eu)


def _write_off(path, verts, faces):
    with open(path, "w") as fh:
        fh.write("OFF\n%d %d 0\n" % (len(verts), len(faces)))
        for p in verts:
            fh.write("%r %r %r\n" % tuple(float(x) for x in p))
        for t in faces:
            fh.write("3 %d %d %d\n" % tuple(int(x) for x in t))


def test_dataset_mesh_cache(tmp_path, monkeypatch):
    """Dataset(geodesics="mesh") on two shapes writes the `_meshgeo` cache, reloads it bit for bit and never reads the "graph" cache
    (nor the other way round)"""
    ops_()
    import os

    import models.dataset as ds
    shapes = tmp_path / "shapes_train"
    shapes.mkdir()
    _write_off(str(shapes / "a.off"), *R.icosphere(1))
    _write_off(str(shapes / "b.off"), *R.grid_mesh(7, jitter=0.4, seed=3))
    torch.manual_seed(0)
    seen = spy_on_op(monkeypatch)
    graph = ds.Dataset(str(tmp_path), name="faust", geodesics="graph")
    assert os.path.basename(graph.cache_path) == "cache_faust_train.pt" and os.path.exists(graph.cache_path) and not seen
    first = ds.Dataset(str(tmp_path), name="faust", geodesics="mesh")
    assert os.path.basename(first.cache_path) == "cache_faust_train_meshgeo.pt" and os.path.exists(first.cache_path)
    assert first.used_shapes == ["a", "b"] and len(seen) == 2          # computed, the "graph" cache was not picked up
    for i, D in enumerate(seen):
        assert np.array_equal(first.dist_list[i].numpy(), ((D + D.t()) / 2).cpu().numpy().astype(np.float32))
        assert not torch.equal(first.dist_list[i], graph.dist_list[i])
        assert bool((first.dist_list[i] <= graph.dist_list[i]).all())
    again = ds.Dataset(str(tmp_path), name="faust", geodesics="mesh")
    assert len(seen) == 2                                               # read back, not computed
    assert again.used_shapes == first.used_shapes
    for a, b in zip(again.dist_list, first.dist_list):
        assert a.dtype == torch.float32 and torch.equal(a, b)
    for a, b in zip(again.verts_list + again.fps_list, first.verts_list + first.fps_list):
        assert torch.equal(a, b)
    default = ds.Dataset(str(tmp_path), name="faust")
    assert default.cache_path == graph.cache_path
    assert all(torch.equal(a, b) for a, b in zip(default.dist_list, graph.dist_list))
    item = again[0]
    assert item["shape1"]["dist"].shape[0] == item["shape1"]["xyz"].shape[0]


def test_eval_distmat_mesh(monkeypatch):
    """geodesic_distmat(method="mesh"): the symmetrised op output, divided by the same sqrt(area) as the default"""
    ops_()
    import eval_geodesic as eg
    seen = spy_on_op(monkeypatch)
    verts, faces = mesh("icosphere3")
    root_area = np.sqrt(eg.mesh_area(verts, np.asarray(faces, dtype=np.int64)))
    raw = eg.geodesic_distmat(verts, faces, normalize=False, method="mesh")
    normed = eg.geodesic_distmat(verts, faces, method="mesh")
    assert len(seen) == 2
    sym = [((D + D.t()) / 2).cpu().numpy() for D in seen]
    assert np.array_equal(raw, sym[0]) and np.array_equal(normed, sym[1] / root_area)
    check_parity("the normalised matrix times sqrt(area)", normed * root_area, raw)
    edges_raw = eg.geodesic_distmat(verts, faces, normalize=False)
    assert np.array_equal(eg.geodesic_distmat(verts, faces), edges_raw / root_area)
    assert np.array_equal(eg.geodesic_distmat(verts, faces, method="edges"), edges_raw / root_area)
    assert len(seen) == 2   # the default never reaches the new op
    assert (raw <= edges_raw * (1 + 1e-9)).all() and raw.mean() < 0.97 * edges_raw.mean()
