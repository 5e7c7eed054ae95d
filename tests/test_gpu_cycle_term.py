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

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from dvm import ops as _ops
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _ops


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _run(ops, pair):
    dev = [t.cuda() for t in pair]
    loss, g12, g21 = ops.cycle_term(*dev, grad=True)
    loss_only = ops.cycle_term(*dev)
    torch.cuda.synchronize()
    assert torch.equal(_bits(loss), _bits(loss_only)), "the loss-only call gives other bits than the one that also forms the gradients"
    return loss.cpu(), g12.cpu(), g21.cpu()


def _check(ops, name, pair):
    k = pair[0].shape[-1]
    ref = C.dense_reference(*pair)
    loss, g12, g21 = _run(ops, pair)
    assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(g12).all()) and bool(torch.isfinite(g21).all())
    lerr, lbar = (loss.double() - ref["F"]).abs(), C.loss_bound(ref, k)
    worst = {}
    for side, g in (("12", g12), ("21", g21)):
        gerr, gbar = (g.double() - ref["g" + side]).abs(), C.grad_bound(ref, k, side)
        worst[side] = float((gerr / gbar.clamp_min(1e-300)).max())
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
    pair = _batch_160()
    out = _run(ops, pair)
    for b in range(pair[0].shape[0]):
        alone = _run(ops, tuple(t[b:b + 1].contiguous() for t in pair))
        for whole, one in zip(out, alone):
            assert torch.equal(_bits(whole[b:b + 1]), _bits(one)), b


def test_scratch_hygiene(ops, monkeypatch):
    """The same call on a workspace that held 0xFF bytes (int32 -1, a NaN in every float format) and fp32 NaNs: the same bits."""
    pair = _batch_160()
    clean = _run(ops, pair)
    again = _run(ops, pair)
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(clean, again))   # run to run
    kept = []

    def filled(fill):
        def workspace(nbytes, device, tag="ws"):
            n = (int(nbytes) + 3) // 4 * 4
            buf = torch.full((n,), 0xFF, dtype=torch.uint8, device=device)
            if fill == "nan":
                buf.view(torch.float32).fill_(float("nan"))
            kept.append(buf)
            return buf
        return workspace

    for fill in ("ff", "nan"):
        monkeypatch.setattr(ops, "workspace", filled(fill))
        out = _run(ops, pair)
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(clean, out)), fill
    assert len(kept) == 4


def test_route_and_autograd(ops):
    """models.loss.cycle_term on CUDA float32 is the kernel: ops.cycle_term's bits, and backward() gives g12 / g21 times the incoming
    gradient."""
    import models.loss as ml
    dev = [t.cuda() for t in _batch_160()]
    val12, idx12, val21, idx21 = dev
    loss_k, g12_k, g21_k = ops.cycle_term(*dev, grad=True)
    with torch.no_grad():
        assert torch.equal(_bits(ml.cycle_term(*dev)), _bits(loss_k))
    v12, v21 = val12.clone().requires_grad_(True), val21.clone().requires_grad_(True)
    loss = ml.cycle_term(v12, idx12, v21, idx21)
    assert loss.dtype == torch.float32 and loss.requires_grad
    assert torch.equal(_bits(loss), _bits(loss_k))
    loss.sum().backward()
    assert torch.equal(_bits(v12.grad), _bits(g12_k)) and torch.equal(_bits(v21.grad), _bits(g21_k))
    w = torch.tensor([0.5, -2.0, 3.0], device="cuda")
    u12, u21 = val12.clone().requires_grad_(True), val21.clone().requires_grad_(True)
    (ml.cycle_term(u12, idx12, u21, idx21) * w).sum().backward()
    assert torch.equal(_bits(u12.grad), _bits(g12_k * w[:, None, None]))
    assert torch.equal(_bits(u21.grad), _bits(g21_k * w[:, None, None]))
    with torch.no_grad():   # the criterion's own index dtype may be int64: same route, same bits
        assert torch.equal(_bits(ml.cycle_term(val12, idx12.long(), val21, idx21.long())), _bits(loss_k))


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
    out = torch.full((1,), -7.0, device="cuda")
    ws = torch.empty(lib.dvm_cycle_term_workspace_bytes(1, N - 1, M, k, k) * 2, dtype=torch.uint8, device="cuda")
    rc = lib.dvm_cycle_term_f32(dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), dev[3].data_ptr(), 1, N, M, k, k, out.data_ptr(),
                                None, None, ws.data_ptr(), ws.numel(), None)
    torch.cuda.synchronize()
    assert rc == -1 and b"N=%d" % N in lib.dvm_last_error()
    assert float(out) == -7.0   # nothing ran
    with pytest.raises(_lib.DvmError):
        ops.cycle_term(*dev)
    ref = C.dense_reference(val12, idx12, val21, idx21, grad=False)
    loss = ml.cycle_term(*dev).cpu()
    err = (loss.double() - ref["F"]).abs()
    print("limit: N %d F %s err %s bar %s" % (N, ref["F"].tolist(), err.tolist(), (2 * C.U * ref["F"]).tolist()))
    assert bool((err <= 2 * C.U * ref["F"]).all())


def test_memory(ops):
    """B = 4, N = M = 8192, k = 10: forward and backward of the term, workspace included, raise the peak by at most
    8 B N k^2 + 64 B (N + M) k bytes (68 MB) — a condition, not a measurement (a dense B x N x N float64 array is 2.1 GB)."""
    import models.loss as ml
    B, N, M, k = 4, 8192, 8192, 10
    gen = torch.Generator(device="cuda").manual_seed(5)

    def side():
        # k distinct buckets of 64 columns per row, one random column in each: random sets without an N x M draw
        bucket = torch.rand(B, N, 128, generator=gen, device="cuda").argsort(-1)[..., :k]
        idx = (bucket * 64 + torch.randint(0, 64, (B, N, k), generator=gen, device="cuda")).to(torch.int32).contiguous()
        val = torch.softmax(3.0 * torch.randn(B, N, k, generator=gen, device="cuda"), -1).contiguous().requires_grad_(True)
        return val, idx

    val12, idx12 = side()
    val21, idx21 = side()
    assert int(min(idx12.min(), idx21.min())) >= 0 and int(max(idx12.max(), idx21.max())) < M
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    ml.cycle_term(val12, idx12, val21, idx21).sum().backward()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    bound = 8 * B * N * k * k + 64 * B * (N + M) * k
    print("memory: peak rise %d bytes, bound %d" % (rise, bound))
    assert rise <= bound
    for v in (val12, val21):
        assert bool(torch.isfinite(v.grad).all()) and float(v.grad.abs().max()) > 0


def _criterion_inputs(B, N, M, seed):
    gen = _gen(seed)
    f1 = (0.3 * torch.relu(torch.randn(B, N, 128, generator=gen))).cuda().requires_grad_(True)
    f2 = (0.3 * torch.relu(torch.randn(B, M, 128, generator=gen))).cuda().requires_grad_(True)
    v1, v2 = torch.rand(B, N, 3, generator=gen).cuda(), torch.rand(B, M, 3, generator=gen).cuda()
    return f1, f2, v1, v2


def _criterion(ml, partial, w_rank=0):
    cls = ml.GraphDeformLoss_Neural_Partial if partial else ml.GraphDeformLoss_Neural
    return cls(save_name="t", k_deform=10, w_dist=0.02, w_map=0 if partial else 0.005, k_dist=30, N_dist=60, partial=partial, w_deform=0.5,
               w_img=0, w_rank=w_rank, w_self_rec=0.5, w_cd=0.1, w_arap=0.01)


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
    f1, f2, v1, v2 = _criterion_inputs(B, N, M, 21)
    d = mm.Deformer(10).cuda().train()
    crit = _criterion(ml, partial=N != M)
    assert crit.w_cycle == 0 and crit.cycle_loss == 0
    crit.w_cycle = w_cycle
    out = crit(f1, f2, torch.cdist(v1, v1), torch.cdist(v2, v2), v1, v2, np.float64(100.0), d)
    assert len(out) == 5
    assert len(seen) == 2 and all(s[4] for s in seen)   # both directions, on the route the kernel takes
    assert tuple(seen[0][0].shape) == (B, N, 10) and tuple(seen[0][2].shape) == (B, M, 10)
    assert tuple(seen[1][0].shape) == (B, M, 10) and tuple(seen[1][2].shape) == (B, N, 10)
    want, bar = 0.0, 0.0
    for pair in seen:
        ref = C.dense_reference(*pair[:4], grad=False)
        want += float(ref["F"].mean()) * w_cycle / 2
        bar += float(C.loss_bound(ref, pair[0].shape[-1]).mean()) * w_cycle / 2
    got = float(crit.cycle_loss.detach())
    bar += 4 * C.U * abs(want)
    print("criterion (%d,%d): cycle_loss %.9g reference %.9g err %.3e bar %.3e" % (N, M, got, want, abs(got - want), bar))
    assert abs(got - want) <= bar
    out[0].backward()
    assert bool(torch.isfinite(f1.grad).all()) and bool(torch.isfinite(f2.grad).all())
    assert float(f1.grad.abs().max()) > 0 and float(f2.grad.abs().max()) > 0


def test_criterion_default_is_untouched(ops, monkeypatch):
    """w_cycle left at 0: the term is never computed and the native node (nn_ops.criterion_train) is still the route taken."""
    import models.loss as ml
    import models.model as mm
    from dvm import nn_ops
    calls = {"cycle": 0, "native": 0}
    real_term, real_native = ml.cycle_term, nn_ops.criterion_train

    def spy_term(*a):
        calls["cycle"] += 1
        return real_term(*a)

    def spy_native(*a, **kw):
        calls["native"] += 1
        return real_native(*a, **kw)

    monkeypatch.setattr(ml, "cycle_term", spy_term)
    monkeypatch.setattr(nn_ops, "criterion_train", spy_native)
    torch.manual_seed(3)
    B, N = 2, 256
    f1, f2, v1, v2 = _criterion_inputs(B, N, N, 21)
    d = mm.Deformer(10).cuda().train()
    crit = _criterion(ml, partial=False)
    out = crit(f1, f2, torch.cdist(v1, v1), torch.cdist(v2, v2), v1, v2, np.float64(100.0), d)
    assert calls == {"cycle": 0, "native": 1}
    assert crit.cycle_loss == 0 and bool(torch.isfinite(out[0]))
