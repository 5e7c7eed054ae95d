"""-m gpu: the rank term ||P P^T - I||_F on the HIP kernel (dvm_rank_term_f32, ops.rank_term, nn_ops.rank_term,
models.loss.rank_term) against a float64 evaluation of the definition on the same fp32 inputs (tests/rank_term_ref.py, where the
bars are derived): loss within 4 (k + 2) u ||S||_F + 2 u F, every gradient element within
4 (k + 2) u (A + |g| ||S||_F / F) + 2 u |g|, both exactly 0 at F = 0.

The inputs are the smallest that reach each way the kernel can go wrong: N not a multiple of the 64-lane wave or the 256-thread
workgroup, N != M both ways, k = 1 / 3 / 10 / 16, column lists longer than a wave, than a workgroup's stride and than 1024 (hubs),
empty columns, a residual dominated by the diagonal (near-permutation) and one that is exactly zero."""
import numpy as np
import pytest
import torch

import frob_term_common as T
import rank_term_ref as R

pytestmark = pytest.mark.gpu
_gen, _bits = T.gen, T.bits


@pytest.fixture(scope="module")
def ops():
    return T.load_ops()


def _run(ops, val, idx, M):
    return T.run_both(ops.rank_term, (val, idx, M))


def _check(ops, name, val, idx, M):
    k = val.shape[-1]
    ref = R.dense_reference(val, idx, M)
    loss, g = _run(ops, val, idx, M)
    assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(g).all())
    lerr, lbar = (loss.double() - ref["F"]).abs(), R.loss_bound(ref, k)
    gerr, gbar = (g.double() - ref["g"]).abs(), R.grad_bound(ref, k)
    worst = T.worst_ratio(gerr, gbar)
    print("%s: F %s loss err %s bar %s; gradient: worst err / bar %.4f, max |g| %.3e" %
          (name, ref["F"].tolist(), lerr.tolist(), lbar.tolist(), worst, float(ref["g"].abs().max())))
    assert bool((lerr <= lbar).all()), (name, lerr.tolist(), lbar.tolist())
    assert bool((gerr <= gbar).all()), (name, worst)
    return ref, loss, g


@pytest.mark.parametrize("B,N,M,k", [(2, 160, 160, 10), (1, 300, 170, 10), (1, 170, 300, 10), (2, 257, 257, 16), (1, 64, 64, 1), (1, 70, 70, 3)])
def test_random_sets(ops, B, N, M, k):
    val, idx = R.plant_random(_gen(100 + N + k), B, N, M, k)
    ref, _, _ = _check(ops, "random (%d,%d,%d,%d)" % (B, N, M, k), val, idx, M)
    assert bool((ref["F"] > 0.1).all())


@pytest.mark.parametrize("N", [300, 1100])
def test_hubs(ops, N):
    """every row picks columns 0..k-1: the k lists hold N entries each (longer than a wave; at 1100 longer than 1024), S is dense"""
    val, idx = R.plant_hubs(_gen(200 + N), 1, N, N, 10)
    _check(ops, "hubs %d" % N, val, idx, N)


@pytest.mark.parametrize("N,M", [(160, 160), (170, 300)])
def test_near_permutation(ops, N, M):
    val, idx = R.plant_near_perm(1, N, M, 10)
    ref, _, _ = _check(ops, "near-permutation (%d,%d)" % (N, M), val, idx, M)
    assert bool((ref["F"] < 0.05).all()) and bool((ref["F"] > 0.01).all())   # the diagonal residual, 2e-3 per row, dominates


@pytest.mark.parametrize("N,M", [(160, 160), (170, 300)])
def test_exact_permutation(ops, N, M):
    val, idx = R.plant_exact_perm(2, N, M, 10)
    loss, g = _run(ops, val, idx, M)
    assert bool((_bits(loss) == 0).all()), loss
    assert bool(torch.isfinite(g).all()) and bool((g == 0).all())


def _batch_160():
    B, N, M, k = 1, 160, 160, 10
    gen = _gen(7)
    parts = [R.plant_random(gen, B, N, M, k), R.plant_hubs(gen, B, N, M, k), R.plant_near_perm(B, N, M, k)]
    return torch.cat([p[0] for p in parts]).contiguous(), torch.cat([p[1] for p in parts]).contiguous(), M


def test_batch_independence(ops):
    """A batch of the random, hub and near-permutation plantings: every element gets the bits it gets alone."""
    T.check_batch_independence(lambda case: _run(ops, *case), _batch_160())


def test_scratch_hygiene(ops, monkeypatch):
    """The same call on a workspace that held 0xFF bytes (int32 -1, a NaN in every float format) and fp32 NaNs: the same bits."""
    T.check_scratch_hygiene(ops, monkeypatch, lambda case: _run(ops, *case), _batch_160())


def test_route_and_autograd(ops):
    """models.loss.rank_term on CUDA float32 is the kernel: ops.rank_term's bits, and backward() gives g_val times the incoming gradient."""
    import models.loss as ml
    T.check_route_and_autograd(ops.rank_term, ml.rank_term, _batch_160(), (0,))


def test_limit(ops):
    """One row more than the kernel takes: the C entry refuses before any launch, models.loss.rank_term answers through the torch
    formula (float64, rounded once: within 2 u F of the definition)."""
    import models.loss as ml
    from dvm import _lib
    lib = _lib.load()
    N, M, k = ops.rank_term_max_n() + 1, 64, 1
    gen = _gen(11)
    val = (0.25 + 0.75 * torch.rand(1, N, k, generator=gen)).contiguous()
    idx = torch.randint(0, M, (1, N, k), generator=gen).to(torch.int32).contiguous()
    assert lib.dvm_rank_term_workspace_bytes(1, N, M, k) == 0
    assert lib.dvm_rank_term_workspace_bytes(1, N - 1, M, k) > 0
    vd, idd = val.cuda(), idx.cuda()
    T.refused_before_launch(lib, "dvm_rank_term_f32", (vd, idd, 1, N, M, k), 1, lib.dvm_rank_term_workspace_bytes(1, N - 1, M, k) * 2, b"N=%d" % N)
    with pytest.raises(_lib.DvmError):
        ops.rank_term(vd, idd, M)
    T.check_fallback("limit: N %d" % N, ml.rank_term(vd, idd, M), R.dense_reference(val, idx, M, grad=False))


def test_memory(ops):
    """B = 4, N = M = 8192, k = 10: forward and backward of the term raise the peak by at most 64 B N k bytes (21 MB) — a
    condition, not a measurement (the kernel's arrays are about 16 B N k bytes; a dense B x M x M float64 array is 2.1 GB)."""
    import models.loss as ml
    B, N, M, k = 4, 8192, 8192, 10
    val, idx = T.bucketed_sets(torch.Generator(device="cuda").manual_seed(5), B, N, k, 64)
    assert int(idx.min()) >= 0 and int(idx.max()) < M
    rise, _ = T.peak_rise(lambda: ml.rank_term(val, idx, M).sum().backward())
    print("memory: peak rise %d bytes, bound %d" % (rise, 64 * B * N * k))
    assert rise <= 64 * B * N * k
    assert bool(torch.isfinite(val.grad).all()) and float(val.grad.abs().max()) > 0


def test_criterion_step(ops, monkeypatch):
    """One GraphDeformLoss_Neural(w_rank=0.3) step: crit.rank_loss is (mean over the batch, direction 12 + direction 21) w_rank / 2
    of the float64 reference on the pval / pidx the criterion passed, within the mean of the loss bars (+ 4 u |rank_loss| for the
    fp32 means, sum and product), and the features' gradient is finite."""
    import models.loss as ml
    import models.model as mm
    seen = []
    kernel_term = ml.rank_term

    def spy(pval, pidx, M):
        seen.append((pval.detach().cpu(), pidx.detach().cpu(), M, pval.is_cuda and pval.dtype == torch.float32))
        return kernel_term(pval, pidx, M)

    monkeypatch.setattr(ml, "rank_term", spy)
    torch.manual_seed(3)
    B, N, w_rank = 2, 256, 0.3
    f1, f2, v1, v2 = T.criterion_inputs(B, N, N, 21)
    d = mm.Deformer(10).cuda().train()
    crit = T.make_criterion(ml, partial=False, w_rank=w_rank)
    out = crit(f1, f2, torch.cdist(v1, v1), torch.cdist(v2, v2), v1, v2, np.float64(100.0), d)
    assert len(seen) == 2 and all(s[3] for s in seen)   # both directions, on the route the kernel takes
    assert all(M == N for _, _, M, _ in seen)
    refs = [R.dense_reference(pval, pidx, M, grad=False) for pval, pidx, M, _ in seen]
    T.check_criterion_term("criterion: rank_loss", crit.rank_loss, [(ref, R.loss_bound(ref, s[0].shape[-1])) for ref, s in zip(refs, seen)], w_rank,
                           out, (f1, f2), (f1,))
