"""-m gpu: the cycle term ||P12 P21 - I||_F on the HIP kernel (dvm_cycle_term_f32, ops.cycle_term, nn_ops.cycle_term,
models.loss.cycle_term) against a float64 evaluation of the definition on the same fp32 inputs (tests/cycle_term_ref.py, where the
bars are derived): loss within 4 (k + 2) u ||C||_F + 2 u F, every element of both gradients within
4 (k + 2) u (A + |g| ||C||_F / F) + 2 u |g|, all exactly 0 at F = 0.

The inputs are the smallest that reach each way the kernel can go wrong: N and M not multiples of the 64-lane wave or the
256-thread workgroup, N != M both ways, k12 != k21 both ways, k = 1 / 3 / 10 / 16, column lists longer than a wave, than the
column kernel's stride and than 1024 (hubs), empty columns, a residual dominated by the diagonal (near inverse) and one that is
exactly zero."""
import numpy as np
import pytest
import torch

import cycle_term_ref as C
import frob_term_common as T

pytestmark = pytest.mark.gpu
_gen, _bits = T.gen, T.bits


@pytest.fixture(scope="module")
def ops():
    return T.load_ops()


def _run(ops, pair):
    return T.run_both(ops.cycle_term, pair)


def _check(ops, name, pair):
    k = pair[0].shape[-1]
    ref = C.dense_reference(*pair)
    loss, g12, g21 = _run(ops, pair)
    assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(g12).all()) and bool(torch.isfinite(g21).all())
    lerr, lbar = (loss.double() - ref["F"]).abs(), C.loss_bound(ref, k)
    worst = {}
    for side, g in (("12", g12), ("21", g21)):
        gerr, gbar = (g.double() - ref["g" + side]).abs(), C.grad_bound(ref, k, side)
        worst[side] = T.worst_ratio(gerr, gbar)
    print("%s: F %s loss err %s bar %s ratio %.4f; worst gradient err / bar: g12 %.4f g21 %.4f" %
          (name, ref["F"].tolist(), lerr.tolist(), lbar.tolist(), float((lerr / lbar).max()), worst["12"], worst["21"]))
    assert bool((lerr <= lbar).all()), (name, lerr.tolist(), lbar.tolist())
    assert worst["12"] <= 1.0 and worst["21"] <= 1.0, (name, worst)
    return ref


@pytest.mark.parametrize("B,N,M,k12,k21", [(2, 160, 160, 10, 10), (1, 300, 170, 10, 10), (1, 170, 300, 10, 10), (2, 257, 257, 16, 16),
                                           (1, 200, 130, 10, 16), (1, 130, 200, 16, 3), (1, 64, 64, 1, 1), (1, 70, 70, 3, 3)])
def test_random_sets(ops, B, N, M, k12, k21):
    pair = C.plant_pair("random", "random", _gen(100 + N + k12), B, N, M, k12, k21)
    ref = _check(ops, "random (%d,%d,%d,%d,%d)" % (B, N, M, k12, k21), pair)
    assert bool((ref["F"] > 0.1).all()) and float(ref["g12"].abs().max()) > 0 and float(ref["g21"].abs().max()) > 0


@pytest.mark.parametrize("N", [300, 1100])
@pytest.mark.parametrize("kind12,kind21", [("hubs", "random"), ("random", "hubs"), ("hubs", "hubs")])
def test_hubs(ops, kind12, kind21, N):
    """a hub side has every row picking columns 0..k-1: with P12 hubs the k lists g21 walks hold N entries each (longer than a wave
    and the walk's stride; at 1100 longer than 1024), with P21 hubs every row of C lives on k columns"""
    pair = C.plant_pair(kind12, kind21, _gen(200 + N), 1, N, N, 10, 10)
    _check(ops, "%s x %s %d" % (kind12, kind21, N), pair)


@pytest.mark.parametrize("N,M", [(160, 160), (170, 300)])
def test_near_inverse(ops, N, M):
    ref = _check(ops, "near inverse (%d,%d)" % (N, M), C.plant_near_inverse(1, N, M, 10))
    if N == M:
        assert abs(float(ref["F"]) - 0.02598) < 1e-5   # the diagonal residual, 2e-3 per row, dominates
    assert bool((ref["F"] < 0.05).all()) and bool((ref["F"] > 0.01).all())


@pytest.mark.parametrize("N,M", [(160, 160), (170, 300)])
def test_exact_inverse(ops, N, M):
    loss, g12, g21 = _run(ops, C.plant_exact_inverse(2, N, M, 10))
    assert bool((_bits(loss) == 0).all()), loss
    for g in (g12, g21):
        assert bool(torch.isfinite(g).all()) and bool((g == 0).all())


def _batch_160():
    B, N, M, k = 1, 160, 160, 10
    gen = _gen(7)
    parts = [C.plant_pair("random", "random", gen, B, N, M, k, k), C.plant_pair("hubs", "hubs", gen, B, N, M, k, k),
             C.plant_near_inverse(B, N, M, k)]
    return tuple(torch.cat([p[q] for p in parts]).contiguous() for q in range(4))


def test_batch_independence(ops):
    """A batch of the random, hub and near-inverse plantings: every element gets the bits it gets alone."""
    T.check_batch_independence(lambda pair: _run(ops, pair), _batch_160())


def test_scratch_hygiene(ops, monkeypatch):
    """The same call on a workspace that held 0xFF bytes (int32 -1, a NaN in every float format) and fp32 NaNs: the same bits."""
    T.check_scratch_hygiene(ops, monkeypatch, lambda pair: _run(ops, pair), _batch_160())


def test_route_and_autograd(ops):
    """models.loss.cycle_term on CUDA float32 is the kernel: ops.cycle_term's bits, and backward() gives g12 / g21 times the incoming
    gradient."""
    import models.loss as ml
    T.check_route_and_autograd(ops.cycle_term, ml.cycle_term, _batch_160(), (0, 2))


def test_limit(ops):
    """One row more than the kernel takes: the C entry refuses before any launch, models.loss.cycle_term answers through the torch
    formula (float64, rounded once: within 2 u F of the definition)."""
    import models.loss as ml
    from dvm import _lib
    lib = _lib.load()
    N, M, k = ops.cycle_term_max_n() + 1, 64, 1
    gen = _gen(11)
    val12 = (0.25 + 0.75 * torch.rand(1, N, k, generator=gen)).contiguous()
    idx12 = torch.randint(0, M, (1, N, k), generator=gen).to(torch.int32).contiguous()
    val21 = (0.25 + 0.75 * torch.rand(1, M, k, generator=gen)).contiguous()
    idx21 = torch.randint(0, N, (1, M, k), generator=gen).to(torch.int32).contiguous()
    assert lib.dvm_cycle_term_workspace_bytes(1, N, M, k, k) == 0
    assert lib.dvm_cycle_term_workspace_bytes(1, N - 1, M, k, k) > 0
    dev = [t.cuda() for t in (val12, idx12, val21, idx21)]
    T.refused_before_launch(lib, "dvm_cycle_term_f32", (*dev, 1, N, M, k, k), 2, lib.dvm_cycle_term_workspace_bytes(1, N - 1, M, k, k) * 2,
                            b"N=%d" % N)
    with pytest.raises(_lib.DvmError):
        ops.cycle_term(*dev)
    T.check_fallback("limit: N %d" % N, ml.cycle_term(*dev), C.dense_reference(val12, idx12, val21, idx21, grad=False))


def test_memory(ops):
    """B = 4, N = M = 8192, k = 10: forward and backward of the term, workspace included, raise the peak by at most
    8 B N k^2 + 64 B (N + M) k bytes (68 MB) — a condition, not a measurement (a dense B x N x N float64 array is 2.1 GB)."""
    import models.loss as ml
    B, N, M, k = 4, 8192, 8192, 10
    gen = torch.Generator(device="cuda").manual_seed(5)
    val12, idx12 = T.bucketed_sets(gen, B, N, k, 64)
    val21, idx21 = T.bucketed_sets(gen, B, N, k, 64)
    assert int(min(idx12.min(), idx21.min())) >= 0 and int(max(idx12.max(), idx21.max())) < M
    rise, _ = T.peak_rise(lambda: ml.cycle_term(val12, idx12, val21, idx21).sum().backward())
    bound = 8 * B * N * k * k + 64 * B * (N + M) * k
    print("memory: peak rise %d bytes, bound %d" % (rise, bound))
    assert rise <= bound
    for v in (val12, val21):
        assert bool(torch.isfinite(v.grad).all()) and float(v.grad.abs().max()) > 0


@pytest.mark.parametrize("N,M", [(256, 256), (256, 192)])
def test_criterion_step(ops, monkeypatch, N, M):
    """One criterion step with crit.w_cycle = 0.3 (N != M: the partial variant, a shape the rank term refuses): crit.cycle_loss is
    (mean over the batch, direction 12 + direction 21) w_cycle / 2 of the float64 reference on the pval / pidx the criterion passed,
    within the mean of the loss bars (+ 4 u |cycle_loss| for the fp32 means, sum and product), and the features' gradient is finite."""
    import models.loss as ml
    import models.model as mm
    seen = []
    kernel_term = ml.cycle_term

    def spy(pval12, pidx12, pval21, pidx21):
        seen.append(tuple(t.detach().cpu() for t in (pval12, pidx12, pval21, pidx21)) +
                    (all(p.is_cuda and p.dtype == torch.float32 for p in (pval12, pval21)),))
        return kernel_term(pval12, pidx12, pval21, pidx21)

    monkeypatch.setattr(ml, "cycle_term", spy)
    torch.manual_seed(3)
    B, w_cycle = 2, 0.3
    f1, f2, v1, v2 = T.criterion_inputs(B, N, M, 21)
    d = mm.Deformer(10).cuda().train()
    crit = T.make_criterion(ml, partial=N != M)
    assert crit.w_cycle == 0 and crit.cycle_loss == 0
    crit.w_cycle = w_cycle
    out = crit(f1, f2, torch.cdist(v1, v1), torch.cdist(v2, v2), v1, v2, np.float64(100.0), d)
    assert len(out) == 5
    assert len(seen) == 2 and all(s[4] for s in seen)   # both directions, on the route the kernel takes
    assert tuple(seen[0][0].shape) == (B, N, 10) and tuple(seen[0][2].shape) == (B, M, 10)
    assert tuple(seen[1][0].shape) == (B, M, 10) and tuple(seen[1][2].shape) == (B, N, 10)
    refs = [C.dense_reference(*pair[:4], grad=False) for pair in seen]
    T.check_criterion_term("criterion (%d,%d): cycle_loss" % (N, M), crit.cycle_loss,
                           [(ref, C.loss_bound(ref, pair[0].shape[-1])) for ref, pair in zip(refs, seen)], w_cycle, out, (f1, f2), (f1, f2))


def test_criterion_default_is_untouched(ops, monkeypatch):
    """w_cycle left at 0: the term is never computed and the native node (nn_ops.criterion_train) is still the route taken."""
    T.check_criterion_default_untouched(monkeypatch, "cycle")
