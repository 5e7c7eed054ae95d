"""The numpy statement of the precise (vertex-to-point) map (tests/precise_map_ref.py), checked without a device: against a dense
sampling of the faces on tiny cases, on the planted family whose answers are exact, and for the quality of the input families the
GPU test (tests/test_gpu_precise_map.py) takes its bars from.  Also eval_geodesic.geodesic_errors_precise against its formula."""
import os
import sys

import numpy as np
import pytest

import precise_map_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dv-matcher_amd"))


@pytest.mark.parametrize("d", [4, 8])
def test_reference_against_dense_sampling(d):
    K = 80
    f1, f2, faces = R.randn(seed=3, n=12, d=d)
    faces = faces[:24]
    r = R.closest(f1, f2, faces)
    b = R.brute(f1, f2, faces, K)
    longest = max(np.linalg.norm(f2[a].astype(np.float64) - f2[c]) for tri in faces for a in tri for c in tri)
    assert (r["dist"] <= b + 1e-12).all()                      # a sample point is a point of the mesh
    assert (b - r["dist"] <= longest / K).all()                # ... and one of them lies within an edge / K of the closest point
    assert np.allclose(R.point_distance(f1, f2, faces[r["face"]], r["bary"]), r["dist"], rtol=0, atol=1e-12)


def test_degenerate_faces_against_dense_sampling():
    f1, f2, faces = R.degenerate()
    r = R.closest(f1, f2, faces)
    b = R.brute(f1[:16], f2, faces, 64)
    assert not np.isnan(r["dist"]).any() and not np.isnan(r["bary"]).any()
    assert (r["dist"][:16] <= b + 1e-9).all() and (b - r["dist"][:16] <= 64.0 * np.sqrt(f2.shape[1]) / 64).all()


def test_every_region_occurs_in_randn():
    _, _, _, r64, r32, _ = R.family("randn")
    assert np.bincount(r64["region"], minlength=7).min() >= 1, np.bincount(r64["region"], minlength=7)
    assert set(r32["region"].tolist()) == set(range(7))


@pytest.mark.parametrize("d", [8, 128, 132])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_planted_expectations(d, dtype):
    f1, f2, faces, want = R.planted(d=d)
    r = R.closest(f1, f2, faces, dtype)
    assert np.array_equal(r["face"], want["face"])
    assert np.array_equal(r["bary"], want["bary"])
    assert np.array_equal(r["dist"].astype(np.float32), want["dist"])
    # the plantings cover vertices, edges and interiors, and the vertex / edge ones do tie between faces
    assert {min(k // 3, 2) for k in R.region_of(want["bary"]).tolist()} == {0, 1, 2}     # a vertex, an edge, an interior
    tied = 0
    for i in np.nonzero(R.region_of(want["bary"]) < 6)[0]:
        others = R.closest(f1[i:i + 1], f2, np.delete(faces, want["face"][i], axis=0), np.float64)
        tied += int(np.float32(others["dist"][0]) == np.float32(r["dist"][i]))      # (the distances are exact in fp32)
    assert tied >= 10


@pytest.mark.parametrize("name,d", [("randn", None), ("randn", 4), ("randn", 8), ("randn", 132), ("smooth", None), ("smooth", 132),
                                    ("offset", None), ("degenerate", None), ("degenerate", 4)])
def test_families_are_well_posed(name, d):
    """The float32 chain's error against float64 is above zero and within the project's float bar, 1e-4 x max|f|: a
    family outside it would be ill-posed and has to be drawn again."""
    f1, f2, faces, r64, r32, err = R.family(name, d)
    scale = max(np.abs(f1).max(), np.abs(f2).max())
    assert 0 < err <= 1e-4 * scale, (err, scale)
    assert r64["left_out"] == 0 and (r64["face"] >= 0).all()
    w = r32["bary"].astype(np.float64)
    assert (w >= 0).all() and (np.abs(w.sum(1) - 1) <= 4 * np.finfo(np.float32).eps).all()


def test_nonfinite_and_left_out_faces():
    f1, f2, faces, bad = R.nonfinite()
    r = R.closest(f1, f2, faces, np.float32)
    assert not np.isnan(r["bary"]).any() and not np.isnan(r["dist"]).any()
    assert np.isposinf(r["dist"][bad]).all() and (r["face"][bad] == 0).all()
    fin = np.setdiff1d(np.arange(len(f1)), bad)
    assert np.isfinite(r["dist"][fin]).all()
    assert not np.isin(r["face"][fin], np.nonzero(np.isin(faces, (0, 1)).any(axis=1))[0]).any()
    cut = faces.copy()
    cut[[3, 9], [0, 2]] = (len(f2), -1)
    rc = R.closest(f1, f2, cut, np.float64)
    keep = np.delete(np.arange(len(faces)), [3, 9])
    rk = R.closest(f1, f2, faces[keep], np.float64)
    assert rc["left_out"] == 2 and np.array_equal(rc["face"], keep[rk["face"]]) and np.array_equal(rc["dist"], rk["dist"])
    none = R.closest(f1, f2, np.full((4, 3), len(f2)), np.float64)
    assert (none["face"] == -1).all() and np.isposinf(none["dist"]).all() and (none["bary"] == 0).all()


def test_geodesic_errors_precise():
    import eval_geodesic as E
    g = np.random.default_rng(0)
    V, F, N, L = 30, 40, 25, 12
    M_tgt = g.random((V, V))
    faces = g.integers(0, V, (F, 3))
    face = g.integers(0, F, N)
    bary = g.dirichlet(np.ones(3), N)
    vts_src, vts_tgt = g.integers(0, N, L), g.integers(0, V, L)
    got = E.geodesic_errors_precise(face, bary, faces, vts_src, vts_tgt, M_tgt)
    want = [sum(bary[s, k] * M_tgt[faces[face[s], k], t] for k in range(3)) for s, t in zip(vts_src, vts_tgt)]
    assert np.allclose(got, want, rtol=0, atol=1e-15)
    # one-hot weights: the vertex map's errors
    corner = g.integers(0, 3, N)
    onehot = np.eye(3)[corner]
    T = faces[face, corner]
    assert np.array_equal(E.geodesic_errors_precise(face, onehot, faces, vts_src, vts_tgt, M_tgt), E.geodesic_errors(T, vts_src, vts_tgt, M_tgt))
