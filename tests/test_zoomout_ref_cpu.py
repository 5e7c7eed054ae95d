"""The ZoomOut reference (tests/zoomout_ref.py) on its planted families, without a GPU: the near-tie rows defeat a float64 Gram-form
search while the sequential form is exact on them; the loop recovers a planted permutation on every vertex from a start map with
30 % random entries, with a margin many orders of magnitude above the nearest distance; it improves a non-isometric pair's map at
least fourfold; Cholesky on the normal equations agrees with pinv.  The GPU tests (tests/test_gpu_zoomout.py) run the device entries
on the same inputs.  Last: the entries' argument checks through the loaded library (no launch is reached)."""
import ctypes

import numpy as np
import pytest

pytest.importorskip("scipy")

import zoomout_ref as Z  # noqa: E402

NEAR_TIE_K = (1, 3, 4, 5, 30, 128)


def near_tie_seed(k):
    """a seed whose base row is not 0 in every coordinate (at k = 1 a zero base would leave the Gram form exact)"""
    return 100 + k


@pytest.mark.parametrize("k", NEAR_TIE_K)
def test_near_tie_family_defeats_the_gram_form(k):
    N, M = 65, 257
    A, E, T, d = Z.near_tie(N, M, k, near_tie_seed(k))
    # every distance is an exact multiple of 2^-40 below 2^53 * 2^-40: any summation order gives it without rounding
    q = d * 2.0 ** 40
    assert np.array_equal(q, np.round(q)) and q.max() < 2.0 ** 53
    assert np.array_equal(Z.dist_seq(A, E), d)
    Tn, dmin = Z.spectral_nn(A, E)
    assert np.array_equal(Tn, T) and np.array_equal(dmin, d[np.arange(N), T])
    wrong = int((Z.gram_nn(A, E) != T).sum())
    print("k=%d: the float64 Gram form picks the wrong column in %d of %d rows" % (k, wrong, N))
    assert wrong > N // 2
    if k == 1:   # the lowest-index rule is exercised: a row's minimum is shared by many columns
        assert (d == d.min(1, keepdims=True)).sum(1).max() >= 10


def test_nan_and_inf_rules():
    A, E, T, _ = Z.near_tie(9, 20, 3, 1)
    A[2, 1] = np.nan
    E[int(T[5]), 0] = np.nan
    Tn, dmin = Z.spectral_nn(A, E)
    assert Tn[2] == 0 and np.isinf(dmin[2])
    assert Tn[5] != T[5] and np.isfinite(dmin[5])


_planted = {}


def planted(name):
    if name not in _planted:
        v, f = Z.planted_meshes(name)
        vy, fy, truth = Z.permuted_copy(v, f, seed=5)
        px, mx = Z.basis(v, f, 40)
        py, _ = Z.basis(vy, fy, 40)
        _planted[name] = (px, mx, py, truth, Z.corrupted(truth, len(vy), 0.3, seed=11))
    return _planted[name]


@pytest.mark.parametrize("solve", ["adjoint", "lstsq"])
@pytest.mark.parametrize("k_init", [6, 10])
@pytest.mark.parametrize("name", ["grid20", "ico2"])
def test_planted_permutation_is_recovered(name, k_init, solve):
    px, mx, py, truth, T0 = planted(name)
    assert (T0 != truth).sum() >= 0.2 * len(truth)
    C, T, steps = Z.zoomout(px, mx, py, T0, k_init, 40, 2, 1, solve)
    assert steps == len(range(k_init, 40, 2))
    d = np.sort(Z.dist_seq(px, Z.embed(py, C)), axis=1)
    print("%s k_init=%d %s: nearest <= %.3g, margin to the second nearest >= %.3g" % (name, k_init, solve, d[:, 0].max(), (d[:, 1] - d[:, 0]).min()))
    assert np.array_equal(Z.to_pmap(px, py, C), truth)
    # the recovered map is far from any tie: the device's rounding cannot move it
    assert d[:, 0].max() <= 1e-20 and (d[:, 1] - d[:, 0]).min() >= 0.4


_pair = {}


def non_isometric(K=40):
    if K not in _pair:
        vx, vy, f = Z.non_isometric_pair()
        px, mx = Z.basis(vx, f, K)
        py, _ = Z.basis(vy, f, K)
        truth = np.arange(len(vx), dtype=np.int32)
        _pair[K] = (px, mx, py, vy, truth, Z.corrupted(truth, len(vy), 0.4, seed=13))
    return _pair[K]


@pytest.mark.parametrize("solve", ["adjoint", "lstsq"])
def test_non_isometric_pair_improves(solve):
    px, mx, py, vy, truth, T0 = non_isometric()
    C, _, _ = Z.zoomout(px, mx, py, T0, 8, 40, 2, 1, solve)
    before, after = Z.map_error(T0, vy, truth), Z.map_error(Z.to_pmap(px, py, C), vy, truth)
    print("%s: mean Euclidean error %.4f -> %.4f" % (solve, before, after))
    assert after <= before / 4.0


def test_normal_equations_agree_with_pinv():
    """cond(Phi^T Phi) stays below 2 on these bases, so Cholesky on the normal equations and pinv both carry errors of a few
    k 2^-53 |C|: the bar is the project's float64 slack 2^-40 times the largest entry."""
    px, _, py, _, _, T0 = non_isometric(60)
    gram, rhs = px.T @ px, px.T @ py[T0]
    assert np.linalg.cond(gram) < 2.0
    L = np.linalg.cholesky(gram)
    C = np.linalg.solve(L.T, np.linalg.solve(L, rhs))
    Cp = np.linalg.pinv(px) @ py[T0]
    print("Cholesky on the normal equations vs pinv: %.3g, cond %.3f" % (np.abs(C - Cp).max(), np.linalg.cond(gram)))
    assert np.abs(C - Cp).max() <= 2.0 ** -40 * np.abs(Cp).max()
    assert np.abs(Z.from_pmap(px, None, py, T0, 60, "lstsq")[0] - Cp).max() <= 2.0 ** -40 * np.abs(Cp).max()


def test_out_of_range_entries_are_zero_rows():
    px, mx, py, _, truth, _ = non_isometric()
    T = truth.copy()
    T[[3, 77]] = [-1, len(py)]
    C, outside = Z.from_pmap(px, mx, py, T, 12)
    keep = np.ones(len(T), bool)
    keep[[3, 77]] = False
    ref = px[keep, :12].T @ (Z.clean_mass(mx, len(px))[keep, None] * py[T[keep], :12])
    assert outside == 2 and np.abs(C - ref).max() <= 2.0 ** -40


# ---------------------------------------------------------------- argument checks of the loaded library
BIG = (1 << 24) + 1
BASE = dict(B=1, N=100, M=90, ldx=40, ldy=40, k_init=6, k_final=40, k_step=2, n_inter=1, mode=0)
CHANGES = [dict(B=0), dict(B=65536), dict(N=0), dict(N=BIG), dict(M=0), dict(M=BIG), dict(k_init=0), dict(k_init=41),
           dict(k_final=129, ldx=200, ldy=200), dict(k_final=0, k_init=0), dict(ldx=39), dict(ldy=39), dict(k_step=0), dict(n_inter=0),
           dict(mode=2), dict(mode=-1)]


@pytest.fixture(scope="module")
def lib():
    from dvm import _lib
    return _lib.load()


def _buffers():
    d = np.zeros(64)
    return d, d.ctypes.data


def test_zoomout_rejects_every_limit(lib):
    keep, p = _buffers()
    sizes = ("B", "N", "M", "k_init", "k_final", "k_step", "n_inter", "mode")
    assert lib.dvm_zoomout_workspace_bytes(*[BASE[s] for s in sizes]) > 0

    def call(a, ptrs=(p,) * 7):
        phi_x, mass, phi_y, T0, C, T, info = ptrs
        return lib.dvm_zoomout_f64(phi_x, a["ldx"], mass, phi_y, a["ldy"], T0, a["B"], a["N"], a["M"], a["k_init"], a["k_final"], a["k_step"],
                                   a["n_inter"], a["mode"], C, T, info, p, 1 << 40, None)
    for change in CHANGES:
        a = dict(BASE, **change)
        if not set(change) & {"ldx", "ldy"} or "k_final" in change:
            assert lib.dvm_zoomout_workspace_bytes(*[a[s] for s in sizes]) == 0, change
        assert call(a) == -1 and b"dvm_zoomout_f64" in lib.dvm_last_error(), change
    for hole in (0, 2, 3, 4, 5, 6):   # every pointer but the mass must be given
        ptrs = [p] * 7
        ptrs[hole] = None
        assert call(BASE, ptrs) == -1 and b"null pointer" in lib.dvm_last_error(), hole
    # a workspace that is too small: DVM_ENOSPACE = -3, before any launch
    assert lib.dvm_zoomout_f64(p, 40, p, p, 40, p, 1, 100, 90, 6, 40, 2, 1, 0, p, p, p, p, 16, None) == -3
    del keep


def test_stage_entries_reject_every_limit(lib):
    keep, p = _buffers()
    plan = (ctypes.c_int32 * 4)()
    base = dict(B=2, N=100, M=90, k=30, mode=1, ld1=40, ld2=40)
    assert lib.dvm_fmap_from_pmap_workspace_bytes(2, 100, 90, 30, 1) > lib.dvm_fmap_from_pmap_workspace_bytes(2, 100, 90, 30, 0) > 0
    assert lib.dvm_spectral_nn_workspace_bytes(2, 100, 90, 30) > 0 and lib.dvm_fmap_to_pmap_workspace_bytes(2, 100, 90, 30) > 0
    assert lib.dvm_spectral_nn_plan(2, 100, 90, 30, plan) == 0 and plan[0] > 0 and plan[1] > 0 and plan[2] >= 1 and plan[3] % plan[1] == 0
    changes = [dict(B=0), dict(B=65536), dict(N=0), dict(N=BIG), dict(M=0), dict(M=BIG), dict(k=0), dict(k=129, ld1=200, ld2=200), dict(ld1=29),
               dict(ld2=29), dict(mode=2)]
    for change in changes:
        a = dict(base, **change)
        sized = not set(change) & {"ld1", "ld2"} or "k" in change
        if "mode" not in change:
            if sized:
                assert lib.dvm_spectral_nn_workspace_bytes(a["B"], a["N"], a["M"], a["k"]) == 0, change
                assert lib.dvm_fmap_to_pmap_workspace_bytes(a["B"], a["N"], a["M"], a["k"]) == 0, change
                assert lib.dvm_spectral_nn_plan(a["B"], a["N"], a["M"], a["k"], plan) == -1, change
            assert lib.dvm_spectral_nn_f64(p, a["ld1"], p, a["ld2"], a["B"], a["N"], a["M"], a["k"], p, None, p, 1 << 40, None) == -1, change
            assert b"dvm_spectral_nn_f64" in lib.dvm_last_error()
            assert lib.dvm_fmap_to_pmap_f64(p, a["ld1"], p, a["ld2"], p, a["B"], a["N"], a["M"], a["k"], p, None, None, p, 1 << 40, None) == -1, change
            assert b"dvm_fmap_to_pmap_f64" in lib.dvm_last_error()
            if "N" not in change:
                assert lib.dvm_fmap_embed_f64(p, a["ld1"], p, a["B"], a["M"], a["k"], p, a["ld2"], None) == -1, change
                assert b"dvm_fmap_embed_f64" in lib.dvm_last_error()
        if sized:
            assert lib.dvm_fmap_from_pmap_workspace_bytes(a["B"], a["N"], a["M"], a["k"], a["mode"]) == 0, change
        assert lib.dvm_fmap_from_pmap_f64(p, a["ld1"], None, p, a["ld2"], p, a["B"], a["N"], a["M"], a["k"], a["mode"], p, p, p, 1 << 40,
                                          None) == -1, change
        assert b"dvm_fmap_from_pmap_f64" in lib.dvm_last_error()
    # null pointers, and a workspace that is too small (DVM_ENOSPACE = -3), before any launch
    assert lib.dvm_spectral_nn_f64(None, 40, p, 40, 2, 100, 90, 30, p, None, p, 1 << 40, None) == -1
    assert lib.dvm_spectral_nn_f64(p, 40, p, 40, 2, 100, 90, 30, None, None, p, 1 << 40, None) == -1
    assert lib.dvm_fmap_embed_f64(p, 40, None, 2, 90, 30, p, 30, None) == -1
    assert lib.dvm_fmap_to_pmap_f64(p, 40, p, 40, None, 2, 100, 90, 30, p, None, None, p, 1 << 40, None) == -1
    assert lib.dvm_fmap_from_pmap_f64(p, 40, None, p, 40, p, 2, 100, 90, 30, 0, p, None, p, 1 << 40, None) == -1
    assert lib.dvm_spectral_nn_plan(2, 100, 90, 30, None) == -1
    assert lib.dvm_spectral_nn_f64(p, 40, p, 40, 2, 100, 90, 30, p, None, p, 16, None) == -3
    assert lib.dvm_fmap_to_pmap_f64(p, 40, p, 40, p, 2, 100, 90, 30, p, None, None, None, 0, None) == -3
    assert lib.dvm_fmap_from_pmap_f64(p, 40, None, p, 40, p, 2, 100, 90, 30, 1, p, p, p, 16, None) == -3
    del keep
