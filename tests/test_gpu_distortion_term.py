"""-m gpu: the distortion term ||P D2 P^T - D1||_F on the HIP kernel (dvm_distortion_term_f32, ops.distortion_term,
nn_ops.distortion_term, models.loss.distortion_term) against a float64 evaluation of the definition on the same fp32 inputs
(tests/distortion_term_ref.py, where the bars are derived): loss within 4 (2k + 2) u ||S||_F + 2 u F, every element of the gradient
within 4 (2k + 2) u (A + |g| (||S||_F + ||D1||_F) / F) + 2 u |g|, all exactly 0 at F = 0.

The inputs are the smallest that reach each way the kernel can go wrong: N and M not multiples of the 64-lane wave or the
256-thread workgroup, N != M both ways, k = 1 / 3 / 10 / 16, columns that collect one entry of every row (hubs: more entries on one
LDS word than a wave, than the workgroup and than 1024), empty columns, a residual that is a thousandth of the product (near
isometry) and one that is exactly zero, and N = M = 4096, where the workgroup's LDS passes the 64 KB default."""
import numpy as np
import pytest
import torch

import distortion_term_ref as D
import frob_term_common as T

pytestmark = pytest.mark.gpu
_gen, _bits = T.gen, T.bits


@pytest.fixture(scope="module")
def ops():
    return T.load_ops()


def _run(ops, case):
    return T.run_both(ops.distortion_term, case)


def _check(ops, name, case):
    k = case[0].shape[-1]
    ref = D.dense_reference(*case)
    loss, g = _run(ops, case)
    assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(g).all())
    lerr, lbar = (loss.double() - ref["F"]).abs(), D.loss_bound(ref, k)
    gerr, gbar = (g.double() - ref["g"]).abs(), D.grad_bound(ref, k)
    worst = T.worst_ratio(gerr, gbar)
    print("%s: F %s ||S|| %s loss err %s bar %s err / bar %.4f; worst gradient err / bar %.4f" %
          (name, ref["F"].tolist(), ref["S_fro"].tolist(), lerr.tolist(), lbar.tolist(), float((lerr / lbar).max()), worst))
    assert bool((lerr <= lbar).all()), (name, lerr.tolist(), lbar.tolist())
    assert worst <= 1.0, (name, worst)
    return ref


@pytest.mark.parametrize("B,N,M,k", [(2, 160, 160, 10), (1, 300, 170, 10), (1, 170, 300, 16), (1, 257, 257, 16), (1, 64, 64, 1), (1, 70, 70, 3)])
def test_random_sets(ops, B, N, M, k):
    ref = _check(ops, "random (%d,%d,%d,%d)" % (B, N, M, k), D.plant("random", _gen(100 + N + k), B, N, M, k))
    assert bool((ref["F"] > 1).all()) and float(ref["g"].abs().max()) > 0


@pytest.mark.parametrize("N", [300, 1100])
def test_hubs(ops, N):
    """every row picks columns 0..k-1: each of the k columns collects N terms of q (more than a wave and than the workgroup; at
    1100 more than 1024), every other column none"""
    _check(ops, "hubs %d" % N, D.plant("hubs", _gen(200 + N), 1, N, N, 10))


def test_exact_isometry(ops):
    loss, g = _run(ops, D.plant_exact_isometry(_gen(31), 2, 160, 10))
    assert bool((_bits(loss) == 0).all()), loss
    assert bool(torch.isfinite(g).all()) and bool((g == 0).all())


def test_near_isometry(ops):
    ref = _check(ops, "near isometry 160", D.plant_near_isometry(_gen(32), 1, 160, 10))
    assert bool((ref["F"] > 0.01).all()) and bool((ref["F"] < 1e-3 * ref["S_fro"]).all())   # F ~ 0.08 against ||S||_F ~ 115


def test_asymmetric_matrices(ops):
    """models.loss.distortion_term(symmetric=False) on matrices that are not symmetric meets the reference on (D + D^T) / 2 (the
    fp32 halved sum is the same bits on either device)."""
    import models.loss as ml
    val, idx, D1, D2 = D.plant("random", _gen(41), 2, 160, 170, 10)
    gen = _gen(42)
    A1, A2 = D1 + 0.1 * torch.rand(D1.shape, generator=gen), D2 + 0.1 * torch.rand(D2.shape, generator=gen)
    assert not torch.equal(A1, A1.transpose(1, 2)) and not torch.equal(A2, A2.transpose(1, 2))
    ref = D.dense_reference(val, idx, 0.5 * (A1 + A1.transpose(1, 2)), 0.5 * (A2 + A2.transpose(1, 2)))
    v = val.cuda().requires_grad_(True)
    loss = ml.distortion_term(v, idx.cuda(), A1.cuda(), A2.cuda(), symmetric=False)
    loss.sum().backward()
    lerr, lbar = (loss.detach().cpu().double() - ref["F"]).abs(), D.loss_bound(ref, 10)
    gerr, gbar = (v.grad.cpu().double() - ref["g"]).abs(), D.grad_bound(ref, 10)
    worst = T.worst_ratio(gerr, gbar)
    print("asymmetric: F %s loss err / bar %.4f worst gradient err / bar %.4f" % (ref["F"].tolist(), float((lerr / lbar).max()), worst))
    assert bool((lerr <= lbar).all()) and worst <= 1.0


def _batch_160():
    B, N, k = 1, 160, 10
    gen = _gen(7)
    parts = [D.plant("random", gen, B, N, N, k), D.plant("hubs", gen, B, N, N, k), D.plant_near_isometry(gen, B, N, k)]
    return tuple(torch.cat([p[q] for p in parts]).contiguous() for q in range(4))


def test_batch_independence(ops):
    """A batch of the random, hub and near-isometry plantings: every element gets the bits it gets alone."""
    T.check_batch_independence(lambda case: _run(ops, case), _batch_160())


def test_scratch_hygiene(ops, monkeypatch):
    """The same call on a workspace that held 0xFF bytes (int32 -1, a NaN in every float format) and fp32 NaNs: the same bits."""
    T.check_scratch_hygiene(ops, monkeypatch, lambda case: _run(ops, case), _batch_160())


def test_route_and_autograd(ops):
    """models.loss.distortion_term on CUDA float32 is the kernel: ops.distortion_term's bits, and backward() gives g times the
    incoming gradient, to val only."""
    import models.loss as ml
    case = _batch_160()
    T.check_route_and_autograd(ops.distortion_term, lambda *a: ml.distortion_term(*a, symmetric=True), case, (0,))
    val, idx, D1, D2 = T.to_cuda(case)
    loss_k = ops.distortion_term(val, idx, D1, D2)
    with torch.no_grad():
        assert torch.equal(_bits(ml.distortion_term(val, idx, D1, D2)), _bits(loss_k))   # symmetric already: the same matrices
    d1 = D1.clone().requires_grad_(True)
    ml.distortion_term(val.clone().requires_grad_(True), idx, d1, D2, symmetric=True).sum().backward()
    assert d1.grad is None


def test_out_of_range_and_zero_slots(ops):
    """An index outside [0, M) and a slot of value 0 add nothing: the call gives the bits of the same rows with those slots moved
    to a valid column at value 0, and the gradient of an out-of-range slot is 0."""
    val, idx, D1, D2 = D.plant("random", _gen(51), 1, 160, 170, 10)
    val, idx = val.clone(), idx.clone()
    val[:, ::3, 4] = 0.0
    bad = idx.clone()
    bad[:, ::3, 4] = 170
    bad[:, 1::3, 4] = -1
    val_ok = val.clone()
    val_ok[:, 1::3, 4] = 0.0
    loss_bad, g_bad = _run(ops, (val, bad, D1, D2))
    loss_ok, g_ok = _run(ops, (val_ok, idx, D1, D2))
    assert torch.equal(_bits(loss_bad), _bits(loss_ok))
    assert bool((g_bad[:, ::3, 4] == 0).all()) and bool((g_bad[:, 1::3, 4] == 0).all())
    keep = torch.ones_like(g_ok, dtype=torch.bool)
    keep[:, ::3, 4] = keep[:, 1::3, 4] = False
    assert torch.equal(_bits(g_bad[keep]), _bits(g_ok[keep]))


@pytest.mark.parametrize("which", ["N", "M"])
def test_limit(ops, which):
    """One row or one column more than the kernel takes: the C entry refuses before any launch, models.loss.distortion_term
    answers through the torch formula (float64, rounded once: within 2 u F of the definition)."""
    import models.loss as ml
    from dvm import _lib
    lib = _lib.load()
    big, small, k = ops.distortion_term_max_n() + 1, 64, 1
    N, M = (big, small) if which == "N" else (small, big)
    gen = _gen(11)
    val = (0.25 + 0.75 * torch.rand(1, N, k, generator=gen)).contiguous()
    idx = torch.randint(0, M, (1, N, k), generator=gen).to(torch.int32).contiguous()
    D1, D2 = D.distances(gen, 1, N), D.distances(gen, 1, M)
    assert lib.dvm_distortion_term_workspace_bytes(1, N, M, k) == 0
    assert lib.dvm_distortion_term_workspace_bytes(1, min(N, big - 1), min(M, big - 1), k) > 0
    dev = [t.cuda() for t in (val, idx, D1, D2)]
    T.refused_before_launch(lib, "dvm_distortion_term_f32", (*dev, 1, N, M, k), 1, 1 << 20, b"%s=%d" % (which.encode(), big))
    with pytest.raises(_lib.DvmError):
        ops.distortion_term(*dev)
    T.check_fallback("limit: N %d M %d" % (N, M), ml.distortion_term(*dev, symmetric=True), D.dense_reference(val, idx, D1, D2, grad=False))


def test_memory(ops):
    """B = 2, N = M = 4096, k = 10, symmetric=True: forward and backward of the term, workspace included, raise the peak by at
    most 64 B (N + M) k bytes (10.5 MB) — a condition, not a measurement (a dense B x N x N float64 array is 268 MB).  At this size
    the workgroup's LDS (64 KB + the reduction words) is past the default limit for dynamic LDS."""
    import models.loss as ml
    B, N, M, k = 2, 4096, 4096, 10
    gen = torch.Generator(device="cuda").manual_seed(5)

    def dist(n):
        pts = torch.rand(B, n, 3, generator=gen, device="cuda")
        d = torch.cdist(pts, pts)
        d = 0.5 * (d + d.transpose(1, 2))
        d.diagonal(dim1=1, dim2=2).zero_()
        return d.contiguous()

    val, idx = T.bucketed_sets(gen, B, N, k, 32)
    D1, D2 = dist(N), dist(M)
    assert int(idx.min()) >= 0 and int(idx.max()) < M

    def step():
        loss = ml.distortion_term(val, idx, D1, D2, symmetric=True)
        loss.sum().backward()
        return loss

    rise, loss = T.peak_rise(step)
    bound = 64 * B * (N + M) * k
    print("memory: peak rise %d bytes, bound %d; loss %s" % (rise, bound, loss.tolist()))
    assert rise <= bound
    assert bool(torch.isfinite(loss).all()) and bool((loss > 1).all())
    assert bool(torch.isfinite(val.grad).all()) and float(val.grad.abs().max()) > 0
    # the same rows through the loss-only kernel (4 M bytes of LDS): the same bits
    with torch.no_grad():
        assert torch.equal(_bits(ml.distortion_term(val, idx, D1, D2, symmetric=True)), _bits(loss))


@pytest.mark.parametrize("N,M", [(256, 256), (256, 192)])
def test_criterion_step(ops, monkeypatch, N, M):
    """One criterion step with crit.w_distortion = 0.3 (N != M: the partial variant): crit.distortion_loss is (mean over the batch,
    direction 12 + direction 21) w_distortion / 2 of the float64 reference on the pval / pidx and the symmetrised matrices the
    criterion passed, within the mean of the loss bars (+ 4 u |distortion_loss| for the fp32 means, sum and product), and the
    features' gradient is finite and non-zero."""
    import models.loss as ml
    import models.model as mm
    seen = []
    kernel_term = ml.distortion_term

    def spy(pval, pidx, dist_src, dist_tgt, symmetric=False):
        seen.append(tuple(t.detach().cpu() for t in (pval, pidx, dist_src, dist_tgt)) +
                    (symmetric and all(t.is_cuda and t.dtype == torch.float32 for t in (pval, dist_src, dist_tgt)),))
        return kernel_term(pval, pidx, dist_src, dist_tgt, symmetric=symmetric)

    monkeypatch.setattr(ml, "distortion_term", spy)
    torch.manual_seed(3)
    B, w = 2, 0.3
    f1, f2, v1, v2 = T.criterion_inputs(B, N, M, 21)
    d = mm.Deformer(10).cuda().train()
    crit = T.make_criterion(ml, partial=N != M)
    assert crit.w_distortion == 0 and crit.distortion_loss == 0
    crit.w_distortion = w
    # matmul-form distances: symmetric only to rounding, as the criterion's real input
    dist1, dist2 = torch.cdist(v1, v1, compute_mode="use_mm_for_euclid_dist"), torch.cdist(v2, v2, compute_mode="use_mm_for_euclid_dist")
    with pytest.raises(ValueError):
        crit(f1, f2, dist1, None, v1, v2, np.float64(100.0), d)
    out = crit(f1, f2, dist1, dist2, v1, v2, np.float64(100.0), d)
    assert len(out) == 5
    assert len(seen) == 2 and all(s[4] for s in seen)   # both directions, symmetrised by the criterion, on the route the kernel takes
    assert tuple(seen[0][0].shape) == (B, N, 10) and tuple(seen[0][2].shape) == (B, N, N) and tuple(seen[0][3].shape) == (B, M, M)
    assert tuple(seen[1][0].shape) == (B, M, 10) and tuple(seen[1][2].shape) == (B, M, M) and tuple(seen[1][3].shape) == (B, N, N)
    for s in seen:
        assert torch.equal(s[2], s[2].transpose(1, 2)) and torch.equal(s[3], s[3].transpose(1, 2))
    assert torch.equal(seen[0][2], (0.5 * (dist1 + dist1.transpose(1, 2))).cpu()) and torch.equal(seen[0][3], seen[1][2])
    refs = [D.dense_reference(*s[:4], grad=False) for s in seen]
    T.check_criterion_term("criterion (%d,%d): distortion_loss" % (N, M), crit.distortion_loss,
                           [(ref, D.loss_bound(ref, s[0].shape[-1])) for ref, s in zip(refs, seen)], w, out, (f1, f2), (f1, f2))


def test_criterion_default_is_untouched(ops, monkeypatch):
    """w_distortion left at 0: the term is never computed and the native node (nn_ops.criterion_train) is still the route taken."""
    T.check_criterion_default_untouched(monkeypatch, "distortion")
