"""-m gpu: the criterion's opt-in Dirichlet term (GraphDeformLoss_Neural.w_dirichlet / dirichlet_mode) at B = 2, N = M = 256: the
loss is the w_dirichlet = 0 loss plus the term computed separately, the features' gradients are finite and change, and
w_dirichlet = 0 leaves the five returned scalars bit for bit."""
import random

import numpy as np
import pytest
import torch

import dirichlet_term_ref as D
import frob_term_common as T

pytestmark = pytest.mark.gpu
B, N = 2, 256


@pytest.fixture(scope="module")
def ops():
    return T.load_ops()


def criterion_step(w=None, mode=None):
    """one seeded criterion step -> (criterion, the five scalars, (f1, f2)); w None leaves the criterion's attributes untouched"""
    import models.loss as ml
    import models.model as mm
    torch.manual_seed(3)
    random.seed(3)
    f1, f2, v1, v2 = T.criterion_inputs(B, N, N, 21)
    d = mm.Deformer(10).cuda().train()
    crit = T.make_criterion(ml, partial=False)
    if w is not None:
        crit.w_dirichlet = w
    if mode is not None:
        crit.dirichlet_mode = mode
    rng = np.random.default_rng(5)
    starts = (torch.from_numpy(rng.integers(0, N, B)), torch.from_numpy(rng.integers(0, N, B)))
    anchors = (rng.permutation(N)[:60].tolist(), rng.permutation(N)[:60].tolist())
    out = crit(f1, f2, torch.cdist(v1, v1), torch.cdist(v2, v2), v1, v2, np.float64(100.0), d, fps_starts=starts, anchors=anchors)
    return crit, out, (f1, f2)


def scalars(out):
    return [float(torch.as_tensor(x).detach()) for x in out]


def bits(out):
    return [T.bits(torch.as_tensor(x, dtype=torch.float32).reshape(1)) for x in out]


@pytest.mark.parametrize("mode", ["stretch", "uniform"])
def test_loss_is_the_base_loss_plus_the_term(ops, monkeypatch, mode):
    import models.loss as ml
    w = 0.5
    seen = []
    real = ml.dirichlet_term

    def spy(pval, pidx, V, op, normalize=True):
        res = real(pval, pidx, V, op, normalize=normalize)
        seen.append((pval.detach().cpu().numpy(), pidx.detach().cpu().numpy(), V.detach().cpu().numpy(), op, normalize, res.detach().cpu().numpy()))
        return res

    monkeypatch.setattr(ml, "dirichlet_term", spy)
    crit, out, feats = criterion_step(w, mode)
    assert len(out) == 5 and len(seen) == 2 and all(s[4] for s in seen) and crit.dirichlet_mode == mode
    # the term computed separately: the reference on the pval / pidx the criterion formed, the operator rebuilt from its xyz lists
    want, bar = 0.0, 0.0
    for pval, pidx, V, op, _, res in seen:
        assert tuple(pval.shape) == (B, N, 10) and tuple(V.shape) == (B, N, 3) and tuple(op.col.shape) == (B, 2 * N * 10)
        Y = ops.apply(torch.from_numpy(pval).cuda(), torch.from_numpy(pidx.astype(np.int32)).cuda(), torch.from_numpy(V).cuda()).cpu().numpy()
        for b in range(B):
            ref_op = dict(rowptr=op.rowptr[b].cpu().numpy(), col=op.col[b].cpu().numpy(), w=op.w[b].cpu().numpy())
            assert int(op.stats[b, D.STAT_SELF]) == N and int(op.stats[b, D.STAT_KEPT]) == 2 * N * 9
            ref = D.energy(Y[b], ref_op)
            norm = float(op.norm[b])
            lbar = D.loss_bound(ref) / norm + 2.0 ** -23 * ref["E"] / norm       # the term's bar, one fp32 division
            assert abs(float(res[b]) - ref["E"] / norm) <= lbar
            want += ref["E"] / norm * w / 2 / B
            bar += lbar * w / 2 / B
    got = float(crit.dirichlet_loss.detach())
    bar += 4 * T.U * abs(want)                                                   # the fp32 means, sum and product
    print("criterion (%s): dirichlet_loss %.9g reference %.9g err %.3e bar %.3e" % (mode, got, want, abs(got - want), bar))
    assert want > 0 and abs(got - want) <= bar
    # the loss: the same route with a weight too small to reach the fp32 sum, plus the term — one fp32 addition
    tiny, out_tiny, _ = criterion_step(1e-30, mode)
    base = scalars(out_tiny)[0]
    total = scalars(out)[0]
    assert float(tiny.dirichlet_loss.detach()) < 1e-25
    print("loss %.9g = base %.9g + term %.9g (difference %.3e)" % (total, base, got, total - (base + got)))
    assert abs(total - (base + got)) <= 4 * T.U * abs(total)
    # ... and against the w_dirichlet = 0 loss itself, which the native node computes: the two routes agree to 2e-5 of the loss
    # (tests/test_gpu_criterion_native.py)
    _, out0, feats0 = criterion_step(0)
    assert abs(total - (scalars(out0)[0] + got)) <= 2e-5 * abs(total) + bar
    assert all(abs(a - c) <= 2e-5 * max(abs(c), 1e-3) for a, c in zip(scalars(out)[1:], scalars(out0)[1:]))   # the other four: unchanged
    out[0].backward()
    out0[0].backward()
    for f, f0 in zip(feats, feats0):
        assert bool(torch.isfinite(f.grad).all()) and float(f.grad.abs().max()) > 0
        change = float((f.grad - f0.grad).abs().max())
        print("feature gradient: max |change| %.3e of max %.3e" % (change, float(f0.grad.abs().max())))
        assert change > 1e-3 * float(f0.grad.abs().max())


def test_weight_zero_leaves_the_five_scalars_bit_for_bit(ops, monkeypatch):
    """w_dirichlet = 0 (set, with either mode) against a criterion whose attributes were never touched: the same bits, the term is
    never computed and the native node is still the route."""
    _, untouched, _ = criterion_step()
    for mode in ("stretch", "uniform"):
        crit, out, _ = criterion_step(0, mode)
        assert crit.dirichlet_loss == 0
        assert all(torch.equal(a, b) for a, b in zip(bits(out), bits(untouched))), mode
    T.check_criterion_default_untouched(monkeypatch, "dirichlet")
