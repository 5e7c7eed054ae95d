"""The ZoomOut entries on the MI355X against tests/zoomout_ref.py (dvm_spectral_nn_f64, dvm_fmap_embed_f64, dvm_fmap_from_pmap_f64,
dvm_fmap_to_pmap_f64, dvm_zoomout_f64; ops.*, models.loss.zoomout, eval_geodesic.match_zoomout).

The bars.  spectral_nn: T and dmin bit for bit against dist_seq (the entry rounds every operation on its own), on the near-tie
family also against integer arithmetic.  fmap_embed: k 2^-52 sum_a |Phi_Y[j,a]| |C[c,a]| (k FMA steps, one accumulator).
fmap_from_pmap, adjoint: 2^-44 sum_i m_i |phi_a(i)| |phi_b(T_i)|, basis_project's bar for the same kernel (fixed-order float64
sums of at most 1031 terms).  lstsq: with Gram
and RHS recomputed in numpy, |Gram C - RHS|_F <= 2^-40 (|Gram|_F |C|_F + |RHS|_F): the sums contribute <= N 2^-53 and Cholesky's
backward error ~ k 2^-52, both under the project's float64 slack 2^-40.  The loop: the same bytes as the stage entries in a Python
loop; the planted permutations on every vertex."""
import numpy as np
import pytest

pytest.importorskip("scipy")
torch = pytest.importorskip("torch")

import zoomout_ref as Z  # noqa: E402

pytestmark = pytest.mark.gpu
SLACK = 2.0 ** -40


def _ops():
    from dvm import ops
    return ops


def dev(x):
    return torch.as_tensor(np.ascontiguousarray(x)).cuda()


def padded(x, extra, fill):
    """x (B,R,k) as the leading k columns of a (B,R,k+extra) array whose other columns hold `fill` (never to be read)"""
    out = np.full(x.shape[:2] + (x.shape[2] + extra,), fill, np.float64)
    out[..., :x.shape[2]] = x
    return out


def boundary_columns(plan, M):
    """the last column, and both sides of every boundary of the kernel's target tiles and segments, inside [0, M)"""
    cols = {M - 1}
    for step in (plan["tile_m"], plan["seg_len"]):
        for j in range(step, M, step):
            cols |= {j - 1, j}
    return sorted(cols)


def near_tie_batch(B, N, M, k, plan, seed):
    """B different elements of the family: the best column planted at every boundary (one source row each) and, where the shape
    has room, target rows duplicated so that a planted best column has an equal at a higher and at a lower index."""
    cols = boundary_columns(plan, M)
    assert len(cols) <= N or N == 1
    out = []
    for b in range(B):
        rows = np.random.default_rng(seed + b).permutation(N)[:len(cols)]
        plant = list(zip(rows.tolist(), cols))
        dup = [(cols[0], M - 3), (M - 1, 2)] if M >= 8 else []   # (neither is a boundary column at the shapes used here)
        assert not {M - 3, 2} & set(cols) or not dup
        out.append(Z.near_tie(N, M, k, seed + 10 * b, plant, dup))
    return out


def run_nn(A, E, k, lda_extra=3, lde_extra=5):
    ops = _ops()
    T, d = ops.spectral_nn(dev(padded(A, lda_extra, 1e300)), dev(padded(E, lde_extra, -1e300)), k=k, want_dist=True)
    return T.cpu().numpy(), d.cpu().numpy()


@pytest.mark.parametrize("N,M", [(1, 1), (15, 17), (65, 257), (257, 63)])
@pytest.mark.parametrize("k", [1, 3, 4, 5, 30, 127, 128])
def test_spectral_nn_near_ties_bit_for_bit(k, N, M):
    B = 3
    plan = _ops().spectral_nn_plan(B, N, M, k)
    fam = near_tie_batch(B, N, M, k, plan, seed=1000 + k)
    A, E = np.stack([f[0] for f in fam]), np.stack([f[1] for f in fam])
    T, d = run_nn(A, E, k)
    for b, (a, e, T_exact, d_exact) in enumerate(fam):
        Tm, dm = Z.spectral_nn(a, e)
        assert np.array_equal(Tm, T_exact)                       # the model on exact inputs
        wrong = np.flatnonzero(T[b] != Tm)
        assert wrong.size == 0, (b, wrong[:5], T[b][wrong[:5]], Tm[wrong[:5]])
        assert d[b].tobytes() == dm.tobytes() and np.array_equal(dm, d_exact[np.arange(N), Tm])
    T1, d1 = run_nn(A[1:2], E[1:2], k, lda_extra=0, lde_extra=1)   # one element alone, other strides, another plan
    assert T1.tobytes() == T[1:2].tobytes() and d1.tobytes() == d[1:2].tobytes()


def test_spectral_nn_segments_of_several_tiles():
    """A shape whose plan has segments longer than one target tile and more than one segment: the best column planted at every
    boundary of both, and at M - 1."""
    N, M, k = 2100, 1100, 5
    plan = _ops().spectral_nn_plan(1, N, M, k)
    assert plan["seg_len"] > plan["tile_m"] and plan["segments"] > 1, plan
    (A, E, T_exact, d_exact), = near_tie_batch(1, N, M, k, plan, seed=77)
    T, d = run_nn(A[None], E[None], k)
    Tm, dm = Z.spectral_nn(A, E)
    assert np.array_equal(Tm, T_exact) and np.array_equal(T[0], Tm) and d[0].tobytes() == dm.tobytes()


def test_spectral_nn_nan_rules():
    N, M, k = 40, 150, 7
    plan = _ops().spectral_nn_plan(1, N, M, k)
    (A, E, T_exact, _), = near_tie_batch(1, N, M, k, plan, seed=5)
    A, E = A.copy(), E.copy()
    A[3, 2] = np.nan                    # a source row with a NaN: every distance is NaN = +inf, the row returns 0
    victim = 9 if T_exact[9] not in (T_exact[3],) else 10
    E[T_exact[victim], k - 1] = np.nan  # a target column with a NaN never wins
    E[0, 0] = np.inf                    # an infinite distance loses to every finite one
    T, d = run_nn(A[None], E[None], k)
    Tm, dm = Z.spectral_nn(A, E)
    assert T[0, 3] == 0 and np.isposinf(d[0, 3])
    assert T[0, victim] != T_exact[victim] and np.isfinite(d[0, victim])
    assert np.array_equal(T[0], Tm) and d[0].tobytes() == dm.tobytes()
    A[:] = np.nan
    T, d = run_nn(A[None], E[None], k)
    assert not T.any() and np.isposinf(d).all()


def test_spectral_nn_random_rows_bit_for_bit():
    """Random float64 rows: a contracted multiply-add in the kernel would change the distances' last bits."""
    rng = np.random.default_rng(11)
    A, E = rng.standard_normal((2, 300, 30)), rng.standard_normal((2, 300, 30))
    T, d = run_nn(A, E, 30)
    for b in range(2):
        Tm, dm = Z.spectral_nn(A[b], E[b])
        assert np.array_equal(T[b], Tm) and d[b].tobytes() == dm.tobytes()


@pytest.mark.parametrize("M,K,k", [(77, 45, 33), (130, 128, 128), (16, 3, 1)])
def test_fmap_embed(M, K, k):
    rng = np.random.default_rng(k)
    phi, C = rng.standard_normal((2, M, K)), rng.standard_normal((2, k, k))
    E = _ops().fmap_embed(dev(phi), dev(C)).cpu().numpy()
    for b in range(2):
        ref = Z.embed(phi[b], C[b])
        bar = k * 2.0 ** -52 * (np.abs(phi[b][:, :k]) @ np.abs(C[b]).T)
        assert (np.abs(E[b] - ref) <= bar).all(), float((np.abs(E[b] - ref) / bar).max())


def _from_pmap_inputs(N=1031, M=500, K=40, B=2, seed=3):
    rng = np.random.default_rng(seed)
    phi_x, phi_y = rng.standard_normal((B, N, K)), rng.standard_normal((B, M, K))
    T = rng.integers(0, M, (B, N)).astype(np.int32)
    T[0, [0, 17, N - 1]] = [-1, M, 2 ** 31 - 1]
    T[1, 5] = -7
    return phi_x, phi_y, T


@pytest.mark.parametrize("with_mass", [False, True])
def test_fmap_from_pmap_adjoint(with_mass):
    ops = _ops()
    phi_x, phi_y, T = _from_pmap_inputs()
    B, N, K = phi_x.shape
    k = 30
    mass = None
    if with_mass:
        mass = np.random.default_rng(1).uniform(0.5, 2.0, (B, N)).astype(np.float32)
        mass[0, [2, 3, 4]] = [0.0, np.nan, -1.0]
        mass[1, 9] = np.inf
    C, info = ops.fmap_from_pmap(dev(phi_x), None if mass is None else dev(mass), dev(phi_y), dev(T), k=k, want_info=True)
    C, info = C.cpu().numpy(), info.cpu().numpy()
    for b in range(B):
        ref, outside = Z.from_pmap(phi_x[b], None if mass is None else mass[b], phi_y[b], T[b], k)
        g, _ = Z.gathered(phi_y[b], T[b], k)
        bar = 2.0 ** -44 * (np.abs(phi_x[b][:, :k]).T @ (Z.clean_mass(None if mass is None else mass[b], N)[:, None] * np.abs(g)))
        assert (np.abs(C[b] - ref) <= bar).all(), float((np.abs(C[b] - ref) / bar).max())
        assert info[b].tolist() == [0, 0, outside, 0] and outside == (3, 1)[b]


def _lstsq_residual(phi_x, phi_y, T, k, C):
    g, _ = Z.gathered(phi_y, T, k)
    gram, rhs = phi_x[:, :k].T @ phi_x[:, :k], phi_x[:, :k].T @ g
    return np.linalg.norm(gram @ C - rhs), SLACK * (np.linalg.norm(gram) * np.linalg.norm(C) + np.linalg.norm(rhs))


@pytest.mark.parametrize("k", [30, 128])
def test_fmap_from_pmap_lstsq(k):
    ops = _ops()
    phi_x, phi_y, T = _from_pmap_inputs(K=max(k, 40))
    C, info = ops.fmap_from_pmap(dev(phi_x), None, dev(phi_y), dev(T), k=k, solve="lstsq", want_info=True)
    C, info = C.cpu().numpy(), info.cpu().numpy()
    for b in range(len(phi_x)):
        res, bar = _lstsq_residual(phi_x[b], phi_y[b], T[b], k, C[b])
        print("lstsq k=%d element %d: residual %.3g, bar %.3g" % (k, b, res, bar))
        assert res <= bar
        ref = Z.from_pmap(phi_x[b], None, phi_y[b], T[b], k, "lstsq")[0]
        assert np.abs(C[b] - ref).max() <= SLACK * np.abs(ref).max()
        assert info[b].tolist() == [0, 0, (3, 1)[b], 0]


def test_rank_deficient_basis_is_reported():
    """Two equal columns of Phi_X: the lstsq solve's Cholesky fails on that element alone; the loop returns NaN for it, and
    ops.zoomout raises unless check=False."""
    ops = _ops()
    phi_x, phi_y, T = _from_pmap_inputs(N=300, M=200, K=20, B=3)
    T = np.clip(T, 0, 199)
    phi_x[1, :, 7] = phi_x[1, :, 2]
    C, info = ops.fmap_from_pmap(dev(phi_x), None, dev(phi_y), dev(T), k=12, solve="lstsq", want_info=True)
    C, info = C.cpu().numpy(), info.cpu().numpy()
    assert info[:, 0].tolist() == [0, 1, 0] and info[1, 1] == 12 and np.isnan(C[1]).all() and np.isfinite(C[[0, 2]]).all()
    assert ops.fmap_from_pmap(dev(phi_x), None, dev(phi_y), dev(T), k=7, solve="lstsq", want_info=True)[1][:, 0].tolist() == [0, 0, 0]
    from dvm._lib import DvmError
    with pytest.raises(DvmError, match="rank-deficient"):
        ops.zoomout(dev(phi_x), None, dev(phi_y), dev(T), 4, 16, k_step=2, solve="lstsq")
    zo = ops.zoomout(dev(phi_x), None, dev(phi_y), dev(T), 4, 16, k_step=2, solve="lstsq", check=False)
    info = zo.info.cpu().numpy()
    # k = 4, 6 pass (column 7 is not in them), k = 8 holds both equal columns: two NN steps ran on the failing element
    assert info[:, 0].tolist() == [0, 1, 0] and info[1, 1] == 8 and info[:, 3].tolist() == [6, 2, 6]
    assert np.isnan(zo.C[1].cpu().numpy()).all() and np.isfinite(zo.C[[0, 2]].cpu().numpy()).all()
    alone = ops.zoomout(dev(phi_x[:1]), None, dev(phi_y[:1]), dev(T[:1]), 4, 16, k_step=2, solve="lstsq")
    assert torch.equal(alone.C[0], zo.C[0]) and torch.equal(alone.T[0], zo.T[0])
    assert ops.zoomout(dev(phi_x), None, dev(phi_y), dev(T), 4, 16, k_step=2).info[:, 0].tolist() == [0, 0, 0]   # adjoint: no solve


# ---------------------------------------------------------------- device bases
_cache = {}


def device_basis(key, verts, faces, K):
    """ops.mesh_eigenbasis of one mesh or a batch of meshes that share `faces`, convergence asserted (computed once per key)"""
    if key not in _cache:
        ops = _ops()
        v = torch.as_tensor(np.asarray(verts, np.float32)).cuda()
        eb = ops.mesh_eigenbasis(v[None] if v.dim() == 2 else v, dev(np.asarray(faces, np.int32)), K)
        assert eb.info[:, 1].cpu().numpy().all(), "the eigenbasis did not converge"
        _cache[key] = eb
    return _cache[key]


def non_isometric():
    vx, vy, f = Z.non_isometric_pair()
    truth = np.arange(len(vx), dtype=np.int32)
    return device_basis("noniso_x", vx, f, 40), device_basis("noniso_y", vy, f, 40), vy, truth


def python_loop(ops, ex, ey, T0, k_init, k_final, k_step, n_inter, solve):
    T = T0
    for k in range(k_init, k_final, k_step):
        for _ in range(n_inter):
            C = ops.fmap_from_pmap(ex.evecs, ex.mass, ey.evecs, T, k=k, solve=solve)
            T = ops.fmap_to_pmap(ex.evecs, ey.evecs, C)
    return ops.fmap_from_pmap(ex.evecs, ex.mass, ey.evecs, T, k=k_final, solve=solve), T


@pytest.mark.parametrize("solve,k_init,k_final,k_step,n_inter", [("adjoint", 8, 40, 2, 1), ("lstsq", 8, 40, 2, 1), ("adjoint", 8, 40, 3, 2),
                                                                 ("lstsq", 9, 39, 7, 2), ("adjoint", 40, 40, 1, 1)])
def test_zoomout_is_the_composition_of_its_stages(solve, k_init, k_final, k_step, n_inter):
    ops = _ops()
    ex, ey, vy, truth = non_isometric()
    T0 = dev(Z.corrupted(truth, len(vy), 0.4, seed=13))[None]
    zo = ops.zoomout(ex.evecs, ex.mass, ey.evecs, T0, k_init, k_final, k_step=k_step, n_inter=n_inter, solve=solve)
    C, T = python_loop(ops, ex, ey, T0, k_init, k_final, k_step, n_inter, solve)
    assert torch.equal(zo.C, C) and torch.equal(zo.T, T)
    steps = len(range(k_init, k_final, k_step)) * n_inter
    assert zo.info.cpu().numpy().tolist() == [[0, 0, 0, steps]]
    again = ops.zoomout(ex.evecs, ex.mass, ey.evecs, T0, k_init, k_final, k_step=k_step, n_inter=n_inter, solve=solve)
    assert torch.equal(zo.C, again.C) and torch.equal(zo.T, again.T)
    if steps:
        before = Z.map_error(T0[0].cpu().numpy(), vy, truth)
        after = Z.map_error(ops.fmap_to_pmap(ex.evecs, ey.evecs, zo.C)[0].cpu().numpy(), vy, truth)
        print("%s %d -> %d step %d x %d: mean Euclidean error %.4f -> %.4f" % (solve, k_init, k_final, k_step, n_inter, before, after))
        assert after < before


@pytest.mark.parametrize("solve", ["adjoint", "lstsq"])
def test_zoomout_batch_of_three_pairs(solve):
    """Three different pairs in one call (the pair, the pair reversed in role on a common start, and another start map), one of
    them also alone: the same bytes."""
    ops = _ops()
    ex, ey, vy, truth = non_isometric()
    px = torch.cat([ex.evecs, ey.evecs, ex.evecs])
    py = torch.cat([ey.evecs, ex.evecs, ey.evecs])
    mass = torch.cat([ex.mass, ey.mass, ex.mass])
    T0 = dev(np.stack([Z.corrupted(truth, len(truth), 0.4, seed=s) for s in (13, 14, 15)]))
    T0[2, :5] = -1                       # counted, and zero rows of the first step's gather
    zo = ops.zoomout(px, mass, py, T0, 8, 40, k_step=4, solve=solve)
    assert zo.info.cpu().numpy().tolist() == [[0, 0, 0, 8], [0, 0, 0, 8], [0, 0, 5, 8]]
    for b in (1, 2):
        alone = ops.zoomout(px[b:b + 1], mass[b:b + 1], py[b:b + 1], T0[b:b + 1], 8, 40, k_step=4, solve=solve)
        assert torch.equal(alone.C[0], zo.C[b]) and torch.equal(alone.T[0], zo.T[b]) and torch.equal(alone.info[0], zo.info[b])
    C, T = python_loop(ops, *[type("E", (), dict(evecs=e, mass=m))() for e, m in ((px, mass), (py, None))], T0, 8, 40, 4, 1, solve)
    assert torch.equal(zo.C, C) and torch.equal(zo.T, T)


@pytest.mark.parametrize("solve", ["adjoint", "lstsq"])
@pytest.mark.parametrize("k_init", [6, 10])
@pytest.mark.parametrize("name", ["grid20", "ico2"])
def test_planted_permutation_end_to_end(name, k_init, solve):
    """Device bases of a mesh and of its renumbered copy, 30 % of the start map random: the loop followed by the point map at
    k_final returns the permutation on every vertex (tests/test_zoomout_ref_cpu.py: the model does, with a margin >= 0.4 between
    the nearest and the second nearest against a nearest distance <= 1e-20)."""
    ops = _ops()
    from models.loss import pointwise_map, zoomout
    v, f = Z.planted_meshes(name)
    vy, fy, truth = Z.permuted_copy(v, f, seed=5)
    ex, ey = device_basis(name + "_x", v, f, 40), device_basis(name + "_y", vy, fy, 40)
    T0 = dev(Z.corrupted(truth, len(vy), 0.3, seed=11))[None]
    zo = zoomout(T0, ex, ey, k_init, 40, k_step=2, solve=solve)
    T, d = pointwise_map(zo.C, ex, ey, want_dist=True)
    wrong = np.flatnonzero(T[0].cpu().numpy() != truth)
    print("%s k_init=%d %s: %d wrong, nearest <= %.3g" % (name, k_init, solve, wrong.size, float(d.max())))
    assert wrong.size == 0, wrong[:10]
    assert torch.equal(ops.fmap_to_pmap(ex.evecs, ey.evecs, zo.C), T)


def test_zoomout_is_capturable():
    ops = _ops()
    ex, ey, vy, truth = non_isometric()
    T0 = dev(Z.corrupted(truth, len(vy), 0.4, seed=13))[None]
    args = dict(k_step=4, n_inter=1, solve="lstsq", check=False)
    eager = ops.zoomout(ex.evecs, ex.mass, ey.evecs, T0, 8, 40, **args)
    ws = ops.scratch(ops.zoomout_workspace_bytes(1, len(truth), len(vy), 8, 40, 4, 1, "lstsq"), T0.device)
    static_T0 = torch.zeros_like(T0)     # the captured call's static input, other contents at capture time
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            ops.zoomout(ex.evecs, ex.mass, ey.evecs, static_T0, 8, 40, workspace_buf=ws, **args)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.zoomout(ex.evecs, ex.mass, ey.evecs, static_T0, 8, 40, workspace_buf=ws, **args)
    static_T0.copy_(T0)
    graph.replay()
    torch.cuda.synchronize()
    for e, o in zip(eager, out):
        assert torch.equal(e, o), "the replayed capture differs from the eager call"


def test_match_zoomout_refines_the_feature_map():
    """Features = noisy coordinates on the non-isometric pair: the refined map's mean error is at most the unrefined map's, and
    mean_geodesic_error without zoomout= is what it was."""
    import eval_geodesic as EG
    ex, ey, vy, truth = non_isometric()
    vx = Z.non_isometric_pair()[0]
    rng = np.random.default_rng(21)
    pad = np.zeros((len(vx), 1))        # (match()'s arg-min entry takes feature widths that are multiples of 4)
    fx = np.concatenate([vx * np.array([1.3, 1.0, 1.0]) + 0.05 * rng.standard_normal(vx.shape), pad], 1).astype(np.float32)
    fy = np.concatenate([vy + 0.05 * rng.standard_normal(vy.shape), pad], 1).astype(np.float32)
    M_tgt = np.linalg.norm(vy[:, None, :] - vy[None, :, :], axis=-1)     # the target's distance matrix (flat shape: Euclidean)
    lm = np.arange(0, len(truth), 3)
    plain = EG.mean_geodesic_error(fx, fy, lm, truth[lm], M_tgt)
    assert plain == float(EG.geodesic_errors(EG.match(fx, fy), lm, truth[lm], M_tgt).mean())
    zo = dict(basis_src=ex, basis_tgt=ey, k_init=8, k_final=40, k_step=2)
    refined = EG.mean_geodesic_error(fx, fy, lm, truth[lm], M_tgt, zoomout=zo)
    T = EG.match_zoomout(fx, fy, **zo)
    assert T.dtype == np.int64 and T.shape == (len(truth),) and refined == float(EG.geodesic_errors(T, lm, truth[lm], M_tgt).mean())
    print("mean error on the target: features %.4f, after ZoomOut %.4f" % (plain, refined))
    assert refined <= plain
    with pytest.raises(ValueError):
        EG.mean_geodesic_error(fx, fy, lm, truth[lm], M_tgt, faces_tgt=np.zeros((1, 3), np.int32), zoomout=zo)
