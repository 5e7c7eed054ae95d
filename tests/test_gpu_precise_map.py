"""-m gpu: the precise (vertex-to-point) map, dvm_precise_map_f32 / ops.precise_map, against its definition in numpy
(tests/precise_map_ref.py, checked on the CPU by tests/test_precise_map_ref_cpu.py).

Every row of every case is checked, none excluded: with q = sum_k bary_k f2[pi_idx_k] evaluated in float64,
    |p - q| - d*_64 <= bar      and      |dist - |p - q|| <= bar,
d*_64 the float64 reference's distance and bar = 3 x the float32 chain's own error against float64 on the same input, measured by
the reference alone (precise_map_ref.chain_error), the convention of tests/test_gpu_deformer_mlp_adversarial.py.
What that error is: the largest over the rows of |dist32 - dist64|, ||p - q32| - dist64| and |dist32 - |p - q32||, q32 the point the
reference's own fp32 weights name, evaluated in float64 like q above — the float32 result looked at the way this file looks at
the device's, not the distance error alone.  The two agree to a few percent on every family but the offset one (7.9e-6 against
7.0e-8): there the fp32 grain of the weights, about 6e-8, is multiplied by |f| ~ 1e3 when q is formed, so the reference's own
fp32 answer misses a bar made from the distance error alone on |p - q|, and no fp32 weights can meet it; a wrong face would still
miss this bar by some 1e-2.  A launch-limit case hands the device a few of the rows drawn and keeps the bar of all of them: the
maximum over one or two rows says little about the chain (it can be 0).  Face indices are
not compared on the random families (shared edges tie by construction); the planted family, exact in fp32, compares face,
weights and distance with array_equal.  Sizes at the launch limits are named from ops.precise_map_plan."""
import os
import sys

import numpy as np
import pytest
import torch

import mesh_geodesic_ref as MG
import precise_map_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ULP1 = float(np.finfo(np.float32).eps)     # the spacing of fp32 above 1


@pytest.fixture(scope="module")
def ops():
    from dvm import ops as _ops
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _ops


def host(t):
    return None if t is None else t.detach().cpu().numpy()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run(ops, f1, f2, faces, check=True):
    """One batch entry (or a batch, for 3-D inputs) -> dict of numpy outputs, stats included."""
    batched = f1.ndim == 3
    a, b = (dev(f1), dev(f2)) if batched else (dev(f1)[None], dev(f2)[None])
    face, bary, pi_idx, dist, stats = ops.precise_map(a, b, dev(np.asarray(faces, np.int32)), check=check, want_stats=True)
    out = dict(face=host(face), bary=host(bary), pi_idx=host(pi_idx), dist=host(dist))
    if not batched:
        out = {k: v[0] for k, v in out.items()}
    out["stats"] = host(stats)
    return out


def check_structure(out, faces, tag):
    face, bary, pi_idx = out["face"], out["bary"], out["pi_idx"]
    has = face >= 0
    assert not np.isnan(bary).any(), tag
    assert (bary >= 0).all(), tag
    assert (np.abs(bary[has].astype(np.float64).sum(-1) - 1.0) <= 4 * ULP1).all(), tag
    assert np.array_equal(pi_idx[has], np.asarray(faces)[face[has]]), tag
    assert (face[has] < len(faces)).all(), tag


def check_rows(f1, f2, faces, out, r64, bar, tag):
    """All rows with a finite float64 distance against the two bars; prints the figures before it asserts."""
    check_structure(out, faces, tag)
    fin = np.isfinite(r64["dist"])
    assert (out["face"][fin] >= 0).all(), tag
    pq = R.point_distance(f1[fin], f2, out["pi_idx"][fin], out["bary"][fin])
    over, gap = (pq - r64["dist"][fin]).max(), np.abs(out["dist"][fin].astype(np.float64) - pq).max()
    print("%s: rows=%d  max(|p-q| - d64)=%.3e  max|dist - |p-q||=%.3e  bar=%.3e  exact evaluations=%d of %d"
          % (tag, fin.sum(), over, gap, bar, out["stats"][1], len(f1) * len(faces)))
    assert over <= bar, tag
    assert gap <= bar, tag


def check_case(ops, f1, f2, faces, tag, rows=None):
    """A case outside the named families: its own reference and its own bar.  rows: the device gets these rows only; the bar
    is still the reference's error over all the rows drawn (a maximum over one or two rows says little about the chain)."""
    r64, r32 = R.closest(f1, f2, faces, np.float64), R.closest(f1, f2, faces, np.float32)
    bar = 3 * R.chain_error(f1, f2, faces, r64, r32)
    if rows is not None:
        f1, r64 = f1[rows], {k: (v[rows] if isinstance(v, np.ndarray) else v) for k, v in r64.items()}
    out = run(ops, f1, f2, faces, check=False)
    check_rows(f1, f2, faces, out, r64, bar, tag)
    assert out["stats"][0] == r64["left_out"], tag
    return out


@pytest.mark.parametrize("name,d", [("randn", None), ("randn", 4), ("randn", 8), ("randn", 132), ("smooth", None), ("smooth", 132),
                                    ("offset", None), ("degenerate", None), ("degenerate", 4)])
def test_families_every_row(ops, name, d):
    f1, f2, faces, r64, _, err = R.family(name, d)
    assert err > 0
    out = run(ops, f1, f2, faces)
    check_rows(f1, f2, faces, out, r64, 3 * err, "%s d=%s" % (name, f1.shape[1]))
    assert out["stats"][0] == 0 and 0 < out["stats"][1] <= len(f1) * len(faces)


def test_all_seven_regions_reached(ops):
    """The randn family puts rows in every region (three vertices, three edges, interior), on the device as in the reference."""
    f1, f2, faces, r64, _, _ = R.family("randn")
    out = run(ops, f1, f2, faces)
    assert set(R.region_of(out["bary"]).tolist()) == set(range(7)) == set(r64["region"].tolist())


@pytest.mark.parametrize("d", [8, 128, 132])
def test_planted_rows_are_exact(ops, d):
    f1, f2, faces, want = R.planted(d=d)
    out = run(ops, f1, f2, faces)
    assert np.array_equal(out["face"], want["face"])
    assert np.array_equal(out["bary"], want["bary"])
    assert np.array_equal(out["dist"], want["dist"])
    assert np.array_equal(out["pi_idx"], faces[want["face"]])


def test_nonfinite_rows_and_vertices(ops):
    f1, f2, faces, bad = R.nonfinite()
    r64, r32 = R.closest(f1, f2, faces, np.float64), R.closest(f1, f2, faces, np.float32)
    out = run(ops, f1, f2, faces)
    check_rows(f1, f2, faces, out, r64, 3 * R.chain_error(f1, f2, faces, r64, r32), "nonfinite")
    fin = np.setdiff1d(np.arange(len(f1)), bad)
    assert np.isfinite(out["dist"][fin]).all()
    nan_faces = np.nonzero(np.isin(faces, (0, 1)).any(axis=1))[0]           # faces with a NaN or Inf corner
    assert not np.isin(out["face"][fin], nan_faces).any()
    # a non-finite row: every face is at +inf, so the lowest admissible face, weights (1,0,0), dist +inf — no NaN
    assert np.array_equal(out["face"][bad], np.zeros(len(bad), np.int32))
    assert np.array_equal(out["bary"][bad], np.tile(np.float32([1, 0, 0]), (len(bad), 1)))
    assert np.isposinf(out["dist"][bad]).all()


def test_faces_out_of_range(ops):
    f1, f2, faces, _, _, _ = R.family("smooth")
    M = len(f2)
    g = np.random.default_rng(5)
    faces = faces.copy()
    hit = g.choice(len(faces), 17, replace=False)
    faces[hit, g.integers(0, 3, 17)] = np.array([M, -1, 2 ** 31 - 1, M + 7, -2 ** 31] * 4, np.int64)[:17].astype(np.int32)
    out = check_case(ops, f1, f2, faces, "17 faces out of range")
    assert out["stats"][0] == 17 and not np.isin(out["face"], hit).any()
    with pytest.raises(ops.DvmError, match="17 of the %d faces" % len(faces)):
        ops.precise_map(dev(f1)[None], dev(f2)[None], dev(faces))
    # no admissible face at all
    none = run(ops, f1, f2, np.full((5, 3), M, np.int32), check=False)
    assert none["stats"][0] == 5 and none["stats"][1] == 0
    assert (none["face"] == -1).all() and (none["bary"] == 0).all() and (none["pi_idx"] == 0).all() and np.isposinf(none["dist"]).all()


def small_case(seed, M, F, d=8, N=48):
    g = np.random.default_rng(seed)
    f2 = g.standard_normal((M, d)).astype(np.float32)
    f1 = (f2[g.integers(0, M, N)] + 0.4 * g.standard_normal((N, d))).astype(np.float32)
    return f1, f2, g.integers(0, M, (F, 3)).astype(np.int32)


def test_launch_limits(ops):
    rows, threads, chunk, max_m = ops.precise_map_plan(1, 64, 64, 8, 64)
    assert ops.precise_map_max_m() == max_m
    for N in (1, rows - 1, rows, rows + 1):
        check_case(ops, *small_case(N, 40, 60), "N=%d" % N, rows=np.arange(N))
    for M in (1, 3, chunk - 1, chunk, chunk + 1):
        check_case(ops, *small_case(100 + M, M, 50), "M=%d" % M, rows=np.arange(9))
    for F in (1, threads - 1, threads, threads + 1):
        check_case(ops, *small_case(200 + F, 70, F), "F=%d" % F, rows=np.arange(9))
    check_case(ops, *small_case(7, max_m, 6, d=4), "M=max_m", rows=np.arange(2))
    f1, f2, faces = small_case(8, max_m + 1, 6, d=4, N=2)
    with pytest.raises(ops.DvmError, match=r"\(-1\).*exceeds"):
        ops.precise_map(dev(f1)[None], dev(f2)[None], dev(faces))
    with pytest.raises(ops.DvmError, match=r"\(-1\)"):
        ops.precise_map_plan(1, 2, max_m + 1, 4, 6)


def test_batch_shares_the_faces(ops):
    a = R.family("randn", 8)
    f1a, f2a, faces = a[0], a[1], a[2]
    g = np.random.default_rng(11)
    f2b = g.standard_normal(f2a.shape).astype(np.float32)
    f1b = (f2b[g.integers(0, len(f2b), len(f1a))] + 0.3 * g.standard_normal(f1a.shape)).astype(np.float32)
    out = run(ops, np.stack([f1a, f1b]), np.stack([f2a, f2b]), faces)
    for i, (f1, f2) in enumerate(((f1a, f2a), (f1b, f2b))):
        one = run(ops, f1, f2, faces)
        for k in ("face", "bary", "pi_idx", "dist"):
            assert np.array_equal(out[k][i], one[k]), (i, k)
    check_rows(f1a, f2a, faces, {k: (v[0] if k != "stats" else v) for k, v in out.items()}, a[3], 3 * a[5], "batch entry 0")


def test_rows_do_not_depend_on_their_place(ops):
    """A row's outputs are the same bits wherever it sits in a launch, for any N, across two runs, and with the workspace full of
    0xFF bytes before the call."""
    f1, f2, faces, _, _, _ = R.family("smooth")
    keys = ("face", "bary", "pi_idx", "dist")
    full = run(ops, f1, f2, faces)
    again = run(ops, f1, f2, faces)
    assert all(np.array_equal(full[k], again[k]) for k in keys) and np.array_equal(full["stats"], again["stats"])
    from dvm import _lib
    nb = _lib.load().dvm_precise_map_workspace_bytes(1, len(f1), len(f2), f1.shape[1], len(faces))
    ops.workspace(nb, torch.device("cuda", torch.cuda.current_device()), "precise_map").fill_(0xFF)
    poisoned = run(ops, f1, f2, faces)
    assert all(np.array_equal(full[k], poisoned[k]) for k in keys)
    for sel in (np.arange(len(f1))[::-1], np.arange(5, 6), np.arange(3, 3 + 7), np.random.default_rng(3).permutation(len(f1))[:50]):
        part = run(ops, f1[sel], f2, faces)
        assert all(np.array_equal(full[k][sel], part[k]) for k in keys), len(sel)


def test_capturable(ops):
    f1, f2, faces, _, _, _ = R.family("randn")
    a, b, f = dev(f1)[None], dev(f2)[None], dev(faces)
    eager = ops.precise_map(a, b, f, check=False, want_stats=True)
    sa, sb = (0.5 * a).contiguous(), (0.5 * b).contiguous()   # the captured call's static inputs, other contents at capture time
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            ops.precise_map(sa, sb, f, check=False)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.precise_map(sa, sb, f, check=False, want_stats=True)
    sa.copy_(a)
    sb.copy_(b)
    graph.replay()
    torch.cuda.synchronize()
    for e, o in zip(eager, out):
        assert torch.equal(e, o), "the replayed capture differs from the eager call"


def test_sparse_pi_of_the_loss_layer(ops):
    sys.path.insert(0, os.path.join(ROOT, "dv-matcher_amd"))
    from models import loss as L
    f1, f2, faces, _, _, _ = R.family("smooth")
    verts = np.random.default_rng(2).standard_normal((len(f2), 3)).astype(np.float32)
    pi = L.precise_map(dev(f1)[None], dev(f2)[None], dev(faces))
    one = run(ops, f1, f2, faces)
    assert np.array_equal(host(pi.val)[0], one["bary"]) and np.array_equal(host(pi.idx)[0], one["pi_idx"]) and pi.M == len(f2)
    assert np.array_equal(host(pi.face)[0], one["face"]) and np.array_equal(host(pi.dist)[0], one["dist"])
    got = host(pi.matmul(dev(verts)[None]))[0]
    want = (one["bary"].astype(np.float64)[:, :, None] * verts[one["pi_idx"]]).sum(1)
    np.testing.assert_allclose(got, want, rtol=0, atol=4 * ULP1 * np.abs(verts).max())   # three fp32 products and two sums


def test_driver_writes_precise_maps(tmp_path, ops):
    """precise_driver on a two-shape --pairs file with faces: the P files parse back to the operator's output on the features
    the inference driver saved, and the T files are the inference driver's own (it runs unchanged: the arg-min of those features)."""
    import scipy.io
    sys.path.insert(0, os.path.join(ROOT, "dv-matcher_amd"))
    import precise_driver
    g = np.random.default_rng(0)
    v1, fa1 = MG.icosphere(3)
    v2, fa2 = MG.grid_mesh(20, jitter=0.3, seed=1)
    pairs = str(tmp_path / "pair.npz")
    np.savez(pairs, verts1=np.asarray(v1, np.float32), verts2=np.asarray(v2, np.float32),
             dino1=g.standard_normal((len(v1), 1152)).astype(np.float32), dino2=g.standard_normal((len(v2), 1152)).astype(np.float32),
             name1="ico", name2="grid", faces1=fa1, faces2=fa2)
    out = str(tmp_path / "res")
    precise_driver.main(["--pairs", pairs, "--out", out])
    feat = {n: scipy.io.loadmat(os.path.join(out, "feature", "usefeature_%s.mat" % n))["uphi"].astype(np.float32) for n in ("ico", "grid")}
    tris = dict(ico=fa1, grid=fa2)
    for src, tgt in (("ico", "grid"), ("grid", "ico")):
        P = np.loadtxt(os.path.join(out, "P", "P_%s_%s.txt" % (src, tgt)))
        one = run(ops, feat[src], feat[tgt], tris[tgt])
        assert P.shape == (len(feat[src]), 4)
        assert np.array_equal(P[:, 0].astype(np.int64), one["face"].astype(np.int64) + 1)
        assert np.array_equal(P[:, 1:].astype(np.float32), one["bary"])
        T = np.loadtxt(os.path.join(out, "T", "T_%s_%s.txt" % (src, tgt)), dtype=np.int64)
        want = host(ops.argmin_exact(dev(feat[src])[None], dev(feat[tgt])[None]))[0].astype(np.int64) + 1
        assert np.array_equal(T, want)
    # no faces: a clear error, before anything is run
    with pytest.raises(ValueError, match="synthetic pairs have none"):
        precise_driver.main(["--synthetic", "1", "--points", "200", "--out", str(tmp_path / "syn")])
    assert not os.path.exists(str(tmp_path / "syn"))
    bare = str(tmp_path / "bare.npz")
    np.savez(bare, verts1=np.asarray(v1, np.float32), verts2=np.asarray(v2, np.float32), dino1=np.zeros((len(v1), 1152), np.float32),
             dino2=np.zeros((len(v2), 1152), np.float32), name1="ico", name2="grid", faces1=fa1)
    with pytest.raises(ValueError, match="grid has none"):
        precise_driver.main(["--pairs", bare, "--out", str(tmp_path / "bare")])


def test_dataset_keeps_the_faces(tmp_path):
    """models/dataset.py: faces_list holds the parsed triangles, built from the OFF files or asked of a set that came from its
    cache (which holds no faces); None for a point-cloud set; the items are what they were; precise_driver reads them."""
    import argparse
    sys.path.insert(0, os.path.join(ROOT, "dv-matcher_amd"))
    import precise_driver
    from models.dataset import testDataset
    os.makedirs(str(tmp_path / "shapes_test"))
    meshes = {"m0": MG.icosphere(2), "m1": MG.grid_mesh(12)}
    for n, (v, f) in meshes.items():
        with open(str(tmp_path / "shapes_test" / (n + ".off")), "w") as fh:
            fh.write("OFF\n%d %d 0\n" % (len(v), len(f)))
            fh.writelines("%r %r %r\n" % tuple(float(x) for x in p) for p in v)
            fh.writelines("3 %d %d %d\n" % tuple(t) for t in f)
    built = testDataset(str(tmp_path), name="scape_r", train=False)
    cached = testDataset(str(tmp_path), name="scape_r", train=False)
    assert os.path.exists(built.cache_path) and cached._faces_list is None          # the second one came from the cache
    for ds in (built, cached):
        assert ds.used_shapes == ["m0", "m1"]
        assert all(np.array_equal(got, meshes[n][1]) for got, n in zip(ds.faces_list, ds.used_shapes))
    for item in (built[0], cached[0]):
        assert sorted(item.keys()) == ["shape1", "shape2"] and all(sorted(x.keys()) == ["dist", "feat", "name", "xyz"] for x in item.values())
    assert testDataset(str(tmp_path), name="se-ornet-tosca", train=False).faces_list is None
    args = argparse.Namespace(data_root=str(tmp_path), pairs=None, data_name="scape_r")
    got = precise_driver.load_faces(args)
    assert sorted(got) == ["m0", "m1"] and all(np.array_equal(got[n], meshes[n][1]) and got[n].dtype == np.int32 for n in got)
    args.data_name = "se-ornet-tosca"
    with pytest.raises(ValueError, match="bare point clouds"):
        precise_driver.load_faces(args)
