"""The frame the tests of the three sparse Frobenius-norm terms share (rank, cycle, distortion: test_gpu_*_term.py,
test_*_term_cpu.py and the *_term_ref.py they are judged against).  A plain module: what a test asserts is written here once and
called with the term's own `run(case)`, reference and bars.

A case is the tuple of a term's inputs (tensors, and for the rank term the int M); run(case) -> the tuple (loss, gradients...) on
the CPU."""
import numpy as np
import pytest
import torch

U = 2.0 ** -24


# ---- the bars' frame (the derivations are in the *_term_ref.py): c = the term's count of fp32 roundings per entry of its product,
# norm (B,) = the Frobenius norm its entry-wise relative error scales with
def loss_bound(ref, c, norm):
    return 4 * c * U * norm + 2 * U * ref["F"]


def grad_bound(ref, c, norm, g, A):
    F = ref["F"][:, None, None]
    g = g.abs()
    ratio = torch.where(F > 0, norm[:, None, None] / F.clamp_min(1e-300), torch.zeros_like(F))
    return 4 * c * U * (A + g * ratio) + 2 * U * g


def near_row(k):
    """val = (1 - 1e-3, 1e-3 / (k - 1), ...): the near-identity plantings' row"""
    row = torch.full((k,), 1e-3 / (k - 1), dtype=torch.float32)
    row[0] = 1.0 - 1e-3
    return row


def exact_row(k):
    """val = (1, 0, ...): the exact plantings' row"""
    row = torch.zeros(k, dtype=torch.float32)
    row[0] = 1.0
    return row


def worst_ratio(err, bar):
    return float((err / bar.clamp_min(1e-300)).max())


def check_fallback(label, loss, ref):
    """The torch fallback is the float64 definition rounded once: within 2 u F."""
    err = (loss.detach().cpu().double() - ref["F"]).abs()
    print(label, "F", ref["F"].tolist(), "err", err.tolist(), "bound", (2 * U * ref["F"]).tolist())
    assert bool((err <= 2 * U * ref["F"]).all())


def check_fallback_grad(grad, g_ref, bar):
    """the fallback's gradient: finite, every element within its bar of the float64 one"""
    assert bool(torch.isfinite(grad).all())
    gerr = (grad.double() - g_ref).abs()
    assert bool((gerr <= bar).all()), worst_ratio(gerr, bar)


# ---- GPU tests
def gen(seed):
    return torch.Generator().manual_seed(seed)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def load_ops():
    from dvm import ops
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return ops


def to_cuda(case):
    return [t.cuda() if torch.is_tensor(t) else t for t in case]


def run_both(term, case):
    """term(*case, grad=True) and term(*case) on the device: the loss-only call must give the loss's bits -> (loss, gradients...) on the CPU"""
    dev = to_cuda(case)
    loss, *grads = term(*dev, grad=True)
    loss_only = term(*dev)
    torch.cuda.synchronize()
    assert torch.equal(bits(loss), bits(loss_only)), "the loss-only call gives other bits than the one that also forms the gradients"
    return (loss.cpu(), *[g.cpu() for g in grads])


def same_bits(a, b):
    return all(torch.equal(bits(x), bits(y)) for x, y in zip(a, b))


def check_batch_independence(run, case):
    """every element of the batch gets the bits it gets alone"""
    out = run(case)
    for b in range(case[0].shape[0]):
        alone = run(tuple(t[b:b + 1].contiguous() if torch.is_tensor(t) else t for t in case))
        assert same_bits([whole[b:b + 1] for whole in out], alone), b


def poisoned_workspace(fill, kept):
    """a stand-in for ops.workspace whose buffers held 0xFF bytes (int32 -1, a NaN in every float format) or fp32 NaNs"""
    def workspace(nbytes, device, tag="ws"):
        n = (int(nbytes) + 3) // 4 * 4
        buf = torch.full((n,), 0xFF, dtype=torch.uint8, device=device)
        if fill == "nan":
            buf.view(torch.float32).fill_(float("nan"))
        kept.append(buf)
        return buf
    return workspace


def check_scratch_hygiene(ops, monkeypatch, run, case):
    """the same call on poisoned workspaces: the same bits, and one workspace request per call (run makes two calls)"""
    clean = run(case)
    assert same_bits(clean, run(case))   # run to run
    kept = []
    for fill in ("ff", "nan"):
        monkeypatch.setattr(ops, "workspace", poisoned_workspace(fill, kept))
        assert same_bits(clean, run(case)), fill
    assert len(kept) == 4


def check_route_and_autograd(ops_term, ml_term, case, diff):
    """ml_term on CUDA float32 is the kernel: ops_term's bits, backward() gives the kernel's gradients of the inputs at positions
    `diff` times the incoming gradient, and int64 indices (the criterion's own dtype) take the same route to the same bits."""
    dev = to_cuda(case)
    loss_k, *g_k = ops_term(*dev, grad=True)
    with torch.no_grad():
        assert torch.equal(bits(ml_term(*dev)), bits(loss_k))
        assert torch.equal(bits(ml_term(*[t.long() if torch.is_tensor(t) and t.dtype == torch.int32 else t for t in dev])), bits(loss_k))
    for w in (None, torch.tensor([0.5, -2.0, 3.0], device="cuda")):
        args = list(dev)
        for pos in diff:
            args[pos] = dev[pos].clone().requires_grad_(True)
        loss = ml_term(*args)
        assert loss.dtype == torch.float32 and loss.requires_grad
        assert torch.equal(bits(loss), bits(loss_k))
        (loss if w is None else loss * w).sum().backward()
        for pos, g in zip(diff, g_k):
            assert torch.equal(bits(args[pos].grad), bits(g if w is None else g * w[:, None, None])), pos


def refused_before_launch(lib, entry, args, ngrads, ws_bytes, needle):
    """the C entry on real device buffers over a limit: DVM_EINVAL with `needle` in the message, and the loss untouched"""
    out = torch.full((1,), -7.0, device="cuda")
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    rc = getattr(lib, entry)(*[a.data_ptr() if torch.is_tensor(a) else a for a in args], out.data_ptr(), *[None] * ngrads, ws.data_ptr(),
                             ws.numel(), None)
    torch.cuda.synchronize()
    assert rc == -1 and needle in lib.dvm_last_error()
    assert float(out) == -7.0   # nothing ran


def bucketed_sets(g, B, N, k, width):
    """k distinct buckets of `width` columns per row (of 128), one random column in each: random sets without an N x M draw, on the
    device -> val (requires grad), idx"""
    bucket = torch.rand(B, N, 128, generator=g, device="cuda").argsort(-1)[..., :k]
    idx = (bucket * width + torch.randint(0, width, (B, N, k), generator=g, device="cuda")).to(torch.int32).contiguous()
    val = torch.softmax(3.0 * torch.randn(B, N, k, generator=g, device="cuda"), -1).contiguous().requires_grad_(True)
    return val, idx


def peak_rise(step):
    """bytes by which step() raises the allocator's peak"""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = step()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base, out


def criterion_inputs(B, N, M, seed):
    g = gen(seed)
    f1 = (0.3 * torch.relu(torch.randn(B, N, 128, generator=g))).cuda().requires_grad_(True)
    f2 = (0.3 * torch.relu(torch.randn(B, M, 128, generator=g))).cuda().requires_grad_(True)
    v1, v2 = torch.rand(B, N, 3, generator=g).cuda(), torch.rand(B, M, 3, generator=g).cuda()
    return f1, f2, v1, v2


def make_criterion(ml, partial, w_rank=0):
    cls = ml.GraphDeformLoss_Neural_Partial if partial else ml.GraphDeformLoss_Neural
    return cls(save_name="t", k_deform=10, w_dist=0.02, w_map=0 if partial else 0.005, k_dist=30, N_dist=60, partial=partial, w_deform=0.5,
               w_img=0, w_rank=w_rank, w_self_rec=0.5, w_cd=0.1, w_arap=0.01)


def check_criterion_term(label, got, refs_and_bars, w, out, feats, nonzero):
    """crit.<term>_loss is (mean over the batch, direction 12 + direction 21) w / 2 of the float64 references, within the mean of the
    loss bars (+ 4 u |the term| for the fp32 means, sum and product); the features' gradient is finite, and non-zero for `nonzero`"""
    want, bar = 0.0, 0.0
    for ref, lbar in refs_and_bars:
        want += float(ref["F"].mean()) * w / 2
        bar += float(lbar.mean()) * w / 2
    got = float(got.detach())
    bar += 4 * U * abs(want)
    print("%s %.9g reference %.9g err %.3e bar %.3e" % (label, got, want, abs(got - want), bar))
    assert abs(got - want) <= bar
    out[0].backward()
    assert all(bool(torch.isfinite(f.grad).all()) for f in feats)
    assert all(float(f.grad.abs().max()) > 0 for f in nonzero)


def check_criterion_default_untouched(monkeypatch, name):
    """w_<name> left at 0: the term is never computed and the native node (nn_ops.criterion_train) is still the route taken."""
    import models.loss as ml
    import models.model as mm
    from dvm import nn_ops
    calls = {name: 0, "native": 0}
    real_term, real_native = getattr(ml, name + "_term"), nn_ops.criterion_train

    def spy_term(*a, **kw):
        calls[name] += 1
        return real_term(*a, **kw)

    def spy_native(*a, **kw):
        calls["native"] += 1
        return real_native(*a, **kw)

    monkeypatch.setattr(ml, name + "_term", spy_term)
    monkeypatch.setattr(nn_ops, "criterion_train", spy_native)
    torch.manual_seed(3)
    B, N = 2, 256
    f1, f2, v1, v2 = criterion_inputs(B, N, N, 21)
    d = mm.Deformer(10).cuda().train()
    crit = make_criterion(ml, partial=False)
    out = crit(f1, f2, torch.cdist(v1, v1), torch.cdist(v2, v2), v1, v2, np.float64(100.0), d)
    assert calls == {name: 0, "native": 1}
    assert getattr(crit, name + "_loss") == 0 and bool(torch.isfinite(out[0]))


# ---- CPU tests of the C entries
def check_entries_exported(name):
    """the three entries of dvm_<name>_term are exported and have signatures -> (lib, the row limit)"""
    import ctypes

    from dvm import _lib
    raw = ctypes.CDLL(_lib.SO_PATH)
    for entry in ("dvm_%s_term_max_n", "dvm_%s_term_workspace_bytes", "dvm_%s_term_f32"):
        assert hasattr(raw, entry % name) and entry % name in _lib.SIGNATURES, entry % name
    lib = _lib.load()
    return lib, getattr(lib, "dvm_%s_term_max_n" % name)()


def check_no_cpu_path(name, case):
    """ops.<name>_term and nn_ops.<name>_term refuse CPU tensors"""
    from dvm import nn_ops, ops
    from dvm._lib import DvmError
    with pytest.raises(DvmError):
        getattr(ops, name + "_term")(*case)
    with pytest.raises(DvmError):
        getattr(nn_ops, name + "_term")(case[0].clone().requires_grad_(True), *case[1:])
