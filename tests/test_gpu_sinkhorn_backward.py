"""-m gpu: the backward of the Sinkhorn-normalised soft correspondence (ops.sinkhorn_hist / ops.sinkhorn_bwd,
nn_ops.sinkhorn_topk, models.loss.sinkhorn_pi under grad, the criterion's sinkhorn_iters, train_driver.py --sinkhorn).

Reference for the gradient: float64 CPU autograd of the definition (float64 torch.cdist of the fp32 inputs cast up,
neg_alpha = float32(-alpha) cast up, torch.logsumexp, exp, gather at the GPU's pi_idx — the columns are an input of the backward
and are pinned by tests/test_gpu_sinkhorn.py — loss sum(gval * val) with a seeded gval).  Yardstick for rounding: the same lines
in fp32 on the CPU, gathered at the same columns.  Bar per tensor and case:
    rel_L2(gpu, f64) <= max(4 * rel_L2(cpu32, f64), 1e-4)
The factor is the forward test's convention (tile-wise summation order, 1-ulp hardware exp); the floor is the standing bar of this
project's backward kernels (tests/test_gpu_backward.py): phase B rebuilds the distances from the norm expansion like
softcorr_bwd_mfma_kernel.  Neither side is derived from the code under test.  Every case prints its figures (run with -s);
profiles/notes_sinkhorn.md section 1b records them."""
import json
import math
import random

import pytest
import torch

pytestmark = pytest.mark.gpu
KINDS = ("randn", "unit", "lowrank")
ALPHAS = (10.0, 100.0)
GRAD_CASES = ([(k, (1000, 440), a, n) for k in KINDS for a in ALPHAS for n in (0, 1, 5, 20)] +
              [(k, (2048, 2048), a, 5) for k in KINDS for a in ALPHAS])
SMALL_CASES = [c for c in GRAD_CASES if c[1] == (1000, 440)]


def case_id(c):
    return "%s-%dx%d-a%g-n%d" % (c[0], c[1][0], c[1][1], c[2], c[3])


@pytest.fixture(scope="module")
def ops():
    from dvm import ops as _ops
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _ops


def make_clouds(kind, N, M, d=128):
    """The families of tests/test_gpu_sinkhorn.py (same generator, same order of draws at d = 128)."""
    g = torch.Generator().manual_seed(1)

    def cloud(n):
        x = torch.randn(n, d, generator=g)
        if kind == "randn":
            return x
        if kind == "unit":
            return x / x.norm(dim=1, keepdim=True)
        z = torch.randn(n, 8, generator=g)
        A = torch.randn(8, d, generator=g) / math.sqrt(8)
        return ((z @ A) * 0.3 + 0.02 * x).contiguous()

    f1 = cloud(N)
    return f1, cloud(M)


def neg_alpha_of(alpha):
    return float(torch.tensor(-float(alpha), dtype=torch.float32).item())


def make_gval(N, topk=10, seed=7, B=None):
    g = torch.Generator().manual_seed(seed)
    return torch.randn((N, topk) if B is None else (B, N, topk), generator=g)


def reference_grads(f1, f2, alpha, n_iter, idx, gval, dtype):
    """Autograd of the definition in `dtype` on the CPU -> (df1, df2) as float64."""
    N, M = f1.shape[0], f2.shape[0]
    x1 = f1.to(dtype).clone().requires_grad_(True)
    x2 = f2.to(dtype).clone().requires_grad_(True)
    S = torch.cdist(x1[None], x2[None])[0] * torch.tensor(neg_alpha_of(alpha), dtype=dtype)
    v = torch.zeros(M, dtype=dtype)
    for _ in range(n_iter):
        u = -torch.logsumexp(S + v[None, :], dim=1)
        v = math.log(N / M) - torch.logsumexp(S + u[:, None], dim=0)
    uf = -torch.logsumexp(S + v[None, :], dim=1)
    P = torch.exp(S + uf[:, None] + v[None, :])
    loss = (gval.to(dtype) * P.gather(1, idx.long())).sum()
    loss.backward()
    return x1.grad.double(), x2.grad.double()


def rel(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-300))


def report(**kw):
    print("SINKHORN_BWD " + json.dumps(kw, sort_keys=True))


def bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def same_bits(a, b):
    return all(torch.equal(bits(x.cpu()), bits(y.cpu())) for x, y in zip(a, b))


def gpu_grads(ops, f1, f2, alpha, n_iter, gval, variant=0):
    """-> (idx (N,k) on the host, df1, df2 on the host) of one B = 1 forward-with-history + backward."""
    a, b = f1.cuda()[None], f2.cuda()[None]
    val, idx, _, _, uh, vh = ops.sinkhorn_hist(a, b, alpha, n_iter, variant=variant)
    df1, df2 = ops.sinkhorn_bwd(a, b, alpha, n_iter, val, idx, uh, vh, gval.cuda()[None], variant=variant)
    torch.cuda.synchronize()
    return idx[0].cpu(), df1[0].cpu(), df2[0].cpu()


def check_against_float64(ops, f1, f2, alpha, n_iter, variant, tag, gval=None):
    """Bar 2 of the module docstring for both tensors -> (df1, df2, bar1, bar2)."""
    gval = make_gval(f1.shape[0]) if gval is None else gval
    idx, df1, df2 = gpu_grads(ops, f1, f2, alpha, n_iter, gval, variant)
    assert torch.isfinite(df1).all() and torch.isfinite(df2).all(), tag
    r1, r2 = reference_grads(f1, f2, alpha, n_iter, idx, gval, torch.float64)
    c1, c2 = reference_grads(f1, f2, alpha, n_iter, idx, gval, torch.float32)
    assert torch.isfinite(c1).all() and torch.isfinite(c2).all(), "the fp32 CPU yardstick is not finite: " + tag
    e1, e2, y1, y2 = rel(df1, r1), rel(df2, r2), rel(c1, r1), rel(c2, r2)
    bar1, bar2 = max(4 * y1, 1e-4), max(4 * y2, 1e-4)
    report(case=tag, variant=variant, gpu_df1=e1, gpu_df2=e2, cpu32_df1=y1, cpu32_df2=y2, ratio_df1=e1 / max(y1, 1e-300),
           ratio_df2=e2 / max(y2, 1e-300), bar_df1=bar1, bar_df2=bar2, max_abs_df1=float(r1.abs().max()), max_abs_df2=float(r2.abs().max()))
    assert e1 <= bar1 and e2 <= bar2, (tag, variant, dict(gpu=(e1, e2), cpu32=(y1, y2), bars=(bar1, bar2)))
    return df1, df2, bar1, bar2


# ------------------------------------------------------------------ 1. the history entry is the forward
# (the scalar kernel is the small shapes' cross-check, as in tests/test_gpu_sinkhorn.py)
@pytest.mark.parametrize("shape,variant", [((1000, 440), 0), ((1000, 440), 1), ((2048, 2048), 0)], ids=lambda s: str(s).replace(" ", ""))
@pytest.mark.parametrize("kind", KINDS)
def test_history_entry_equals_forward(ops, kind, shape, variant):
    f1, f2 = make_clouds(kind, *shape)
    a, b = f1.cuda()[None], f2.cuda()[None]
    for alpha in ALPHAS:
        for n_iter in (0, 5, 20):
            fwd = ops.sinkhorn(a, b, alpha, n_iter, variant=variant, potentials=True)
            val, idx, lmax, lsum, uh, vh = ops.sinkhorn_hist(a, b, alpha, n_iter, variant=variant)
            assert uh.shape == (1, n_iter + 1, shape[0]) and vh.shape == (1, n_iter + 1, shape[1])
            assert same_bits([val, idx, lmax, lsum, uh[:, -1], vh[:, -1]], fwd), (kind, shape, alpha, n_iter, variant)
            assert bool((vh[:, 0] == 0).all())
            assert torch.isfinite(uh).all() and torch.isfinite(vh).all()


# ------------------------------------------------------------------ 2. the gradient against float64
@pytest.mark.parametrize("case", GRAD_CASES, ids=case_id)
def test_gradient_vs_float64_matrix_cores(ops, case):
    kind, (N, M), alpha, n_iter = case
    f1, f2 = make_clouds(kind, N, M)
    check_against_float64(ops, f1, f2, alpha, n_iter, 0, case_id(case))


@pytest.mark.parametrize("case", SMALL_CASES, ids=case_id)
def test_gradient_vs_float64_scalar_kernels(ops, case):
    kind, (N, M), alpha, n_iter = case
    f1, f2 = make_clouds(kind, N, M)
    check_against_float64(ops, f1, f2, alpha, n_iter, 1, case_id(case))


# ------------------------------------------------------------------ 3. large alpha
def test_large_alpha_small_meets_the_bar(ops):
    f1, f2 = make_clouds("randn", 1000, 440)
    check_against_float64(ops, f1, f2, 150.0, 20, 0, "randn-1000x440-a150-n20")


def test_large_alpha_full_size_stays_finite(ops):
    f1, f2 = make_clouds("randn", 2048, 2048)
    _, df1, df2 = gpu_grads(ops, f1, f2, 150.0, 20, make_gval(2048))
    assert torch.isfinite(df1).all() and torch.isfinite(df2).all()
    assert float(df1.abs().max()) > 0 and float(df2.abs().max()) > 0


# ------------------------------------------------------------------ 4. shapes that do not tile, other d, duplicates
@pytest.mark.parametrize("shape", [(257, 129), (130, 333), (64, 64)], ids=lambda s: "%dx%d" % s)
def test_shapes_that_do_not_tile(ops, shape):
    f1, f2 = make_clouds("unit", *shape)
    for alpha, n_iter in ((10.0, 5), (100.0, 3)):
        for variant in (0, 1):
            check_against_float64(ops, f1, f2, alpha, n_iter, variant, "unit-%dx%d-a%g-n%d" % (shape + (alpha, n_iter)))


def test_other_d_and_duplicates_on_the_scalar_kernel(ops):
    g = torch.Generator().manual_seed(11)
    f1, f2 = torch.randn(70, 36, generator=g), torch.randn(90, 36, generator=g)
    f2[3] = f1[5]   # an exact zero distance: no gradient through that entry, like cdist's backward
    for n_iter in (0, 4):
        check_against_float64(ops, f1, f2, 2.0, n_iter, 0, "d36-70x90-a2-n%d" % n_iter)


@pytest.mark.parametrize("alpha", ALPHAS)
def test_matrix_cores_against_scalar_kernels(ops, alpha):
    f1, f2 = make_clouds("lowrank", 1000, 440)
    a1, a2, ba1, ba2 = check_against_float64(ops, f1, f2, alpha, 5, 0, "lowrank-1000x440-a%g-n5" % alpha)
    s1, s2, bs1, bs2 = check_against_float64(ops, f1, f2, alpha, 5, 1, "lowrank-1000x440-a%g-n5" % alpha)
    assert rel(a1, s1) <= ba1 + bs1 and rel(a2, s2) <= ba2 + bs2, (rel(a1, s1), rel(a2, s2))


# ------------------------------------------------------------------ 5. n_iter = 0 is softcorr
def test_zero_iterations_is_softcorr(ops):
    from dvm import nn_ops
    f1, f2 = make_clouds("unit", 1000, 440)
    gval = make_gval(1000)
    outs = []
    for fn in (lambda a, b: nn_ops.sinkhorn_topk(a, b, 10.0, 0), lambda a, b: nn_ops.softcorr_topk(a, b, 10.0)):
        a, b = f1.cuda()[None].requires_grad_(True), f2.cuda()[None].requires_grad_(True)
        val, idx = fn(a, b)
        (val * gval.cuda()[None]).sum().backward()
        outs.append((val.detach(), idx, a.grad[0].cpu(), b.grad[0].cpu()))
    assert same_bits(outs[0][:2], outs[1][:2])
    idx = outs[0][1][0].cpu()
    r1, r2 = reference_grads(f1, f2, 10.0, 0, idx, gval, torch.float64)
    c1, c2 = reference_grads(f1, f2, 10.0, 0, idx, gval, torch.float32)
    for name, (_, _, g1, g2) in zip(("sinkhorn_topk", "softcorr_topk"), outs):
        e1, e2 = rel(g1, r1), rel(g2, r2)
        report(case="n0-" + name, gpu_df1=e1, gpu_df2=e2, cpu32_df1=rel(c1, r1), cpu32_df2=rel(c2, r2))
        assert e1 <= max(4 * rel(c1, r1), 1e-4) and e2 <= max(4 * rel(c2, r2), 1e-4), (name, e1, e2)


# ------------------------------------------------------------------ 6. reproducible, batched, capturable
def fwd_bwd(ops, a, b, alpha, gval, variant, n_iter=5):
    val, idx, lmax, lsum, uh, vh = ops.sinkhorn_hist(a, b, alpha, n_iter, variant=variant)
    df1, df2 = ops.sinkhorn_bwd(a, b, alpha, n_iter, val, idx, uh, vh, gval, variant=variant)
    return [val, idx, uh, vh, df1, df2]


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("alpha", [30.0, 100.0])
def test_reproducible_and_batched(ops, alpha, variant):
    g = torch.Generator().manual_seed(3)
    f1, f2 = torch.randn(3, 1000, 128, generator=g), torch.randn(3, 440, 128, generator=g)
    f2[1] *= 0.5
    gval = make_gval(1000, B=3).cuda()
    a, b = f1.cuda(), f2.cuda()
    whole = [t.cpu() for t in fwd_bwd(ops, a, b, alpha, gval, variant)]
    again = [t.cpu() for t in fwd_bwd(ops, a, b, alpha, gval, variant)]
    assert same_bits(whole, again), "two runs on the same inputs differ"
    for e in range(3):
        one = [t.cpu() for t in fwd_bwd(ops, a[e:e + 1].contiguous(), b[e:e + 1].contiguous(), alpha, gval[e:e + 1].contiguous(), variant)]
        assert same_bits([t[e:e + 1] for t in whole], one), "entry %d of a B = 3 call differs from its own B = 1 call" % e


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("alpha", [30.0, 100.0])
def test_result_does_not_depend_on_the_workspace_contents(ops, monkeypatch, alpha, variant):
    f1, f2 = make_clouds("randn", 1000, 440)
    a, b, gval = f1.cuda()[None], f2.cuda()[None], make_gval(1000).cuda()[None]
    res = []
    for fill in (0x00, 0xFF):   # 0xFF bytes: NaN bit patterns in every float, -1 in every word
        keep = []

        def workspace(nbytes, device, tag, fill=fill, keep=keep):
            keep.append(torch.full((max(int(nbytes), 1),), fill, dtype=torch.uint8, device=device))
            return keep[-1]

        monkeypatch.setattr(ops, "workspace", workspace)
        res.append([t.cpu() for t in fwd_bwd(ops, a, b, alpha, gval, variant)])
        torch.cuda.synchronize()
    assert same_bits(res[0], res[1]), "the result depends on what the workspace held"
    assert all(torch.isfinite(t).all() for t in res[1] if t.is_floating_point())


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("alpha", [30.0, 100.0])
def test_capturable(ops, alpha, variant):
    """No host synchronisation and no float atomics: forward-with-history + backward can be captured, and the replay on new input
    contents gives the eager calls' bits."""
    f1, f2 = make_clouds("randn", 1000, 440)
    a, b, gval = f1.cuda()[None], f2.cuda()[None], make_gval(1000).cuda()[None]
    eager = [t.clone() for t in fwd_bwd(ops, a, b, alpha, gval, variant)]
    sa, sb = (0.5 * a).contiguous(), (0.5 * b).contiguous()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            fwd_bwd(ops, sa, sb, alpha, gval, variant)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = fwd_bwd(ops, sa, sb, alpha, gval, variant)
    sa.copy_(a)
    sb.copy_(b)
    graph.replay()
    torch.cuda.synchronize()
    assert same_bits(out, eager), "the replayed capture differs from the eager calls"


# ------------------------------------------------------------------ 7. through the layers
def test_sinkhorn_pi_backpropagates(ops):
    import models.loss as ml
    from dvm._lib import DvmError
    f1, f2 = make_clouds("lowrank", 1000, 440)
    g = torch.Generator().manual_seed(5)
    verts2 = torch.rand(1, 440, 3, generator=g).cuda()
    gout = torch.randn(1, 1000, 3, generator=g).cuda()
    x, y = f1.cuda()[None].requires_grad_(True), f2.cuda()[None].requires_grad_(True)
    pi = ml.sinkhorn_pi(x, y)
    assert isinstance(pi, ml.SparsePi) and pi.val.requires_grad and not pi.idx.requires_grad
    (pi.matmul(verts2) * gout).sum().backward()
    val, idx, _, _, uh, vh = ops.sinkhorn_hist(x.detach(), y.detach(), 100, 5)
    dval, _ = ops.apply_bwd(val, idx, verts2, gout)
    df1, df2 = ops.sinkhorn_bwd(x.detach(), y.detach(), 100, 5, val, idx, uh, vh, dval)
    assert same_bits([pi.val.detach(), pi.idx], [val, idx])
    assert same_bits([x.grad, y.grad], [df1, df2])
    assert float(x.grad.abs().max()) > 0 and float(y.grad.abs().max()) > 0
    with pytest.raises(DvmError, match="forward only"):
        ops.sinkhorn(x, y, 100.0, 5)
    with torch.no_grad():   # unchanged without grad: ops.sinkhorn's bits
        pi0 = ml.sinkhorn_pi(x, y)
    assert same_bits([pi0.val, pi0.idx], list(ops.sinkhorn(x.detach(), y.detach(), 100, 5)[:2])) and not pi0.val.requires_grad


def criterion_setup(partial, N, M, seed=21):
    import models.loss as ml
    import models.model as mm
    B = 2
    g = torch.Generator().manual_seed(seed)
    v1 = (torch.rand(B, N, 3, generator=g) - 0.5).cuda()
    v2 = ((v1.cpu() + 0.05 * torch.randn(B, N, 3, generator=g)) if N == M else (torch.rand(B, M, 3, generator=g) - 0.5)).cuda()
    f1 = (0.3 * torch.relu(torch.randn(B, N, 128, generator=g))).cuda().requires_grad_(True)
    f2 = (0.3 * torch.relu(torch.randn(B, M, 128, generator=g))).cuda().requires_grad_(True)
    torch.manual_seed(seed + 1)
    d = mm.Deformer(10).cuda().train()
    cls = ml.GraphDeformLoss_Neural_Partial if partial else ml.GraphDeformLoss_Neural
    n = min(N, M)
    crit = cls(k_deform=10, w_dist=0.02, w_map=0.005, k_dist=min(50, n // 2), N_dist=min(40, n // 2), partial=partial, w_deform=0.5, w_img=0,
               w_rank=0, w_self_rec=0.5, w_cd=0.1, w_arap=0.01, save_name="t")
    starts = (torch.randint(0, N, (B,), generator=g), torch.randint(0, M, (B,), generator=g))
    anchors = (random.Random(seed).sample(range(N), crit.N_dist), random.Random(seed + 1).sample(range(M), crit.N_dist))
    return crit, d, f1, f2, v1, v2, starts, anchors


def composed_direction(crit, d, n_iter, feat1, feat2, verts1, verts2, alpha, g1, idx11, idx22, with_map, train):
    """One direction of deform(), written out from the per-op calls of GraphDeformLoss_Neural._direction_train (under grad) /
    _direction (without), with the Sinkhorn operator where they have the row softmax -> (map_sum, (cd_warp sides), arap, (cd_self sides))."""
    from dvm import nn_ops, ops
    from models.loss import rotation_6d_to_matrix
    B, N, _ = verts1.shape
    iden = torch.tensor([1, 0, 0, 0, 1, 0], dtype=torch.float32, device=verts1.device)
    if not train:
        pval, pidx, _, _ = ops.sinkhorn(feat1, feat2, alpha, n_iter, topk=10)
        verts12 = ops.apply(pval, pidx, verts2)
        def9 = d.forward_sparse(feat1, feat2, verts1, verts12, idx11, idx22, pval, pidx, g1["nodes_idx"])
        warped, arap, _ = ops.dg_warp_arap(verts1, g1, rotation_6d_to_matrix(def9[..., 3:] + iden), def9[..., :3].contiguous())
        cw = ops.chamfer(warped, verts2, want_idx=False)[:2]
        cs = ops.chamfer(verts12, verts2, want_idx=False)[:2]
        map_sum = ops.map_term(verts12, verts2, idx11, idx22, pval, pidx) if with_map else None
        return map_sum, cw, arap.sum(), cs
    pval, pidx = nn_ops.sinkhorn_topk(feat1, feat2, alpha, n_iter, 10)
    verts12 = nn_ops.sparse_apply(pval, pidx, verts2)
    g1p = nn_ops.pool_rows(feat1, idx11, d.conv_layer.weight, d.conv_layer.bias)
    g2p = nn_ops.pool_rows(feat2, idx22, d.conv_layer.weight, d.conv_layer.bias)
    g2t = nn_ops.sparse_apply(pval, pidx, g2p)
    nodes = g1["nodes_idx"].long()
    flat = (nodes + torch.arange(B, device=nodes.device).unsqueeze(1) * N).reshape(-1)
    pick = lambda t: t.reshape(B * N, t.shape[-1]).index_select(0, flat).view(B, nodes.shape[1], t.shape[-1])  # noqa: E731
    def9 = d.deformation_decoder_layer(torch.cat([pick(verts1), pick(g1p), pick(verts12), pick(g2t)], dim=-1))
    warped, arap = nn_ops.dg_warp_arap(verts1, g1, nn_ops.rot6d(def9[..., 3:] + iden), def9[..., :3])
    cw = nn_ops.chamfer_nn(warped, verts2)
    cs = nn_ops.chamfer_nn(verts12, verts2)
    map_sum = None
    if with_map:
        lhs = nn_ops.gather_rows(verts12, idx11)
        v2n = nn_ops.gather_rows(verts2, idx22).reshape(B, verts2.shape[1], -1)
        map_sum = ((lhs - nn_ops.sparse_apply(pval, pidx, v2n).view(B, N, -1, 3)) ** 2).sum(dim=(1, 2, 3))
    return map_sum, cw, arap.sum(), cs


def composed_terms(crit, d, n_iter, f1, f2, v1, v2, alpha, starts, partial, train):
    """(deform_loss, map_loss, self_rec_loss) as GraphDeformLoss_Neural.forward reduces the two directions (models/loss.py)."""
    B, N, _ = v1.shape
    M = v2.shape[1]
    g1, g2, idx11, idx22 = crit.geometry(v1, v2, starts)
    with_map = crit.w_map > 0 and not partial

    def cd(sides, n_src, n_tgt):
        if partial:   # one-sided: the smaller cloud's side
            return torch.mean(sides[0] if n_src <= n_tgt else sides[1])
        return torch.mean(sides[0]) + torch.mean(sides[1])

    m12, w12, a12, s12 = composed_direction(crit, d, n_iter, f1, f2, v1, v2, alpha, g1, idx11, idx22, with_map, train)
    m21, w21, a21, s21 = composed_direction(crit, d, n_iter, f2, f1, v2, v1, alpha, g2, idx22, idx11, with_map, train)
    scale = 1 if partial else N
    deform = ((cd(w12, N, M) * crit.w_cd + a12 * crit.w_arap) + (cd(w21, M, N) * crit.w_cd + a21 * crit.w_arap)) * scale * crit.w_deform / 2
    map_loss = crit.w_map * (m12.sum() / (3 * B) + m21.sum() / (3 * B)) / 2 if with_map else None
    self_rec = (cd(s12, N, M) + cd(s21, M, N)) * scale * crit.w_self_rec / 2
    return deform, map_loss, self_rec


@pytest.mark.parametrize("partial,N,M", [(False, 256, 256), (True, 256, 120)], ids=["full-256x256", "partial-256x120"])
def test_criterion_with_sinkhorn_iters(ops, partial, N, M):
    crit, d, f1, f2, v1, v2, starts, anchors = criterion_setup(partial, N, M)
    assert crit.sinkhorn_iters == 0
    alpha = 60.0
    dist1, dist2 = torch.cdist(v1, v1), torch.cdist(v2, v2)

    def step(iters):
        crit.sinkhorn_iters = iters
        d.zero_grad(set_to_none=True)
        f1.grad = f2.grad = None
        random.seed(5)
        out = crit(f1, f2, dist1, dist2, v1, v2, alpha, d, fps_starts=starts, anchors=anchors)
        out[0].backward()
        return [o.detach() if torch.is_tensor(o) else o for o in out], f1.grad.clone(), f2.grad.clone()

    out3, g1_3, g2_3 = step(3)
    out0, g1_0, g2_0 = step(0)
    crit.sinkhorn_iters = 3
    deform, map_loss, self_rec = composed_terms(crit, d, 3, f1, f2, v1, v2, alpha, starts, partial, True)
    close = lambda x, y: abs(float(x) - float(y)) <= 1e-6 * max(abs(float(y)), 1e-30)  # noqa: E731
    report(case="criterion-%s" % ("partial" if partial else "full"), deform=(float(out3[2]), float(deform)),
           map=(float(out3[3]), None if map_loss is None else float(map_loss)), self_rec=(float(out3[4]), float(self_rec)),
           grad_rel_diff_vs_softmax=(rel(g1_3, g1_0), rel(g2_3, g2_0)))
    assert close(out3[2], deform) and close(out3[4], self_rec), (out3, float(deform), float(self_rec))
    if map_loss is not None:
        assert close(out3[3], map_loss), (out3, float(map_loss))
    for g3, g0 in ((g1_3, g1_0), (g2_3, g2_0)):
        assert torch.isfinite(g3).all() and float(g3.abs().max()) > 0
        assert rel(g3, g0) > 1e-3, "sinkhorn_iters = 3 gave the row softmax's gradient"
    assert abs(float(out3[2]) - float(out0[2])) > 1e-6 * abs(float(out0[2])), "sinkhorn_iters = 3 gave the row softmax's loss"
    # without grad: the 5-tuple is the one built from ops.sinkhorn
    with torch.no_grad():
        random.seed(5)
        out = crit(f1, f2, dist1, dist2, v1, v2, alpha, d, fps_starts=starts, anchors=anchors)
        deform, map_loss, self_rec = composed_terms(crit, d, 3, f1, f2, v1, v2, alpha, starts, partial, False)
        import models.loss as ml
        dist_term = (crit._dist_term(f1, dist1, ml._host_draw_to_device(anchors[0], f1.device)) +
                     crit._dist_term(f2, dist2, ml._host_draw_to_device(anchors[1], f2.device))) * crit.w_dist
    total = dist_term + deform + self_rec + (map_loss if map_loss is not None else 0)
    assert close(out[2], deform) and close(out[4], self_rec) and close(out[1], dist_term), (out, float(deform), float(self_rec))
    if map_loss is not None:
        assert close(out[3], map_loss)
    assert abs(float(out[0]) - float(total)) <= 2e-6 * abs(float(total))


def test_train_driver_with_sinkhorn(capsys):
    import train_driver
    rc = train_driver.main(["--sinkhorn", "3", "--steps", "2", "--warmup", "0", "--batch", "2", "--points", "256"])
    assert rc in (0, None)
    line = json.loads(capsys.readouterr().out.strip().split("\n")[-1])
    assert line["sinkhorn_iters"] == 3 and line["steps"] == 2
    assert all(math.isfinite(float(x)) for x in line["last_losses"])
