"""-m gpu: the unbalanced (KL-relaxed) Sinkhorn correspondence (ops.sinkhorn_unbalanced / _hist / _bwd,
nn_ops.sinkhorn_unbalanced_topk, models.loss.sinkhorn_pi_unbalanced, the criterion's sinkhorn_tau).

The operator is not in the reference.  It is pinned to the balanced operator at tau = (1, 1) (bit for bit) and otherwise to a
float64 evaluation of its definition (include/dvm.h), written out below on the CPU: torch.cdist in float64 on the fp32 inputs cast
up, neg_alpha = float32(-alpha) cast up, torch.logsumexp; the gradient by float64 autograd of the same lines with the loss
sum(g * val) + sum(gl * lmass), gathered at the GPU's columns.  An fp32 run of the same lines is the yardstick for rounding.  The
bars are those of tests/test_gpu_sinkhorn.py and tests/test_gpu_sinkhorn_backward.py:
    potentials, row_lmass, pi_val on decided rows:  error(gpu) <= 4 * error(cpu32)   (pi_val: + 1e-7, as there)
    decided rows (every gap of the float64 top-11 logits >= 64 * 2^-24 * max |S|): 0 column mismatches; undecided <= 15 % of a case
    gradients, per tensor:  rel_L2(gpu, f64) <= max(4 * rel_L2(cpu32, f64), 1e-4)
Neither reference reads the code under test.  Every case prints its figures (run with -s); profiles/notes_sinkhorn.md records them."""
import functools
import json
import math
import random

import pytest
import torch

from test_gpu_sinkhorn import bits, make_clouds, ranked, scores

pytestmark = pytest.mark.gpu
SHAPES = ((64, 64), (257, 129), (130, 333), (1000, 440))
SMALL_SHAPES = SHAPES[:3]
# (features, alpha, tau): alpha 10 with the two relaxations on both families, unit features at alpha 100
SETTINGS = [(k, 10.0, t) for k in ("unit", "lowrank") for t in ((0.5, 0.5), (0.9, 0.7))] + [("unit", 100.0, (0.9, 0.9))]
FWD_ITERS = (0, 5, 20)
BWD_ITERS = (0, 1, 5, 20)


def weighted(setting, shape):
    """Seeded random log_a / log_b of scale 0.3 in half of the (setting, shape) groups, NULL in the rest."""
    return (SETTINGS.index(setting) + SHAPES.index(shape)) % 2 == 1


def group_id(setting, shape):
    return "%s-%dx%d-a%g-t%g_%g%s" % (setting[0], shape[0], shape[1], setting[1], setting[2][0], setting[2][1], "-w" if weighted(setting, shape) else "")


FWD_GROUPS = [(s, sh) for s in SETTINGS for sh in SHAPES]
FWD_CASES = [(s, sh, n) for s, sh in FWD_GROUPS for n in FWD_ITERS]
BWD_CASES = [(s, sh, n) for s, sh in FWD_GROUPS for n in (BWD_ITERS if s[1] == 10.0 else (3,))]


def case_id(c):
    return "%s-n%d" % (group_id(c[0], c[1]), c[2])


@pytest.fixture(scope="module")
def ops():
    from dvm import ops as _ops
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _ops


def report(**kw):
    print("SINKHORN_UB " + json.dumps(kw, sort_keys=True))


def same_bits(a, b):
    return all(torch.equal(bits(x), bits(y)) for x, y in zip(a, b))


def log_weights(N, M, seed=9, B=None):
    g = torch.Generator().manual_seed(seed)
    return (0.3 * torch.randn((N,) if B is None else (B, N), generator=g), 0.3 * torch.randn((M,) if B is None else (B, M), generator=g))


def inputs(setting, shape):
    f1, f2 = make_clouds(setting[0], *shape)
    la, lb = log_weights(*shape) if weighted(setting, shape) else (None, None)
    return f1, f2, la, lb


# ------------------------------------------------------------------ the definition, in S's dtype
def weights_of(log_a, log_b, N, M, dtype):
    la = torch.zeros(N, dtype=dtype) if log_a is None else log_a.to(dtype)
    lb = torch.full((M,), math.log(N / M), dtype=dtype) if log_b is None else log_b.to(dtype)
    return la, lb


def final_step(S, v, la, tau_row):
    mf = -torch.logsumexp(S + v[None, :], dim=1)
    uf = tau_row * (la + mf)
    return dict(L=S + v[None, :], mf=mf, uf=uf, v=v.clone(), lmass=uf - mf)


def reference(S, n_iters, tau, la, lb):
    """{n_iter: final step} for every n_iter asked for, from ONE run of the iteration in S's dtype."""
    v = torch.zeros(S.shape[1], dtype=S.dtype)
    out = {}
    for it in range(max(n_iters) + 1):
        if it in n_iters:
            out[it] = final_step(S, v, la, tau[0])
        u = tau[0] * (la - torch.logsumexp(S + v[None, :], dim=1))
        v = tau[1] * (lb - torch.logsumexp(S + u[:, None], dim=0))
    return out


def compare(S64, S32, n_iters, tau, log_a, log_b):
    """What the checks need of the float64 and the fp32 CPU runs of one group: {n_iter: dict}."""
    N, M = S64.shape
    smax = float(S64.abs().max())
    r64 = reference(S64, n_iters, tau, *weights_of(log_a, log_b, N, M, torch.float64))
    r32 = reference(S32, n_iters, tau, *weights_of(log_a, log_b, N, M, torch.float32))
    out = {}
    for n in n_iters:
        a, b = r64[n], r32[n]
        t11, _ = ranked(a["L"], 11)
        decided = ((t11[:, :-1] - t11[:, 1:]) >= 64 * 2.0 ** -24 * smax).all(dim=1)
        tv, ti = ranked(a["L"], 10)
        p64 = torch.exp(tv + a["uf"][:, None])
        p32 = torch.exp(b["L"].gather(1, ti) + b["uf"][:, None]).double()
        i32 = ranked(b["L"].double(), 10)[1]
        out[n] = dict(r64=a, decided=decided, idx64=ti, p64=p64,
                      e32=max(float((b["uf"].double() - a["uf"]).abs().max()), float((b["v"].double() - a["v"]).abs().max())),
                      lm32=float((b["lmass"].double() - a["lmass"]).abs().max()),
                      pe32=float((p32 - p64)[decided].abs().max()) if bool(decided.any()) else 0.0,
                      cpu32_mismatch=int((i32 != ti).any(dim=1)[decided].sum()))
    return out


@functools.lru_cache(maxsize=2)
def fwd_group(setting, shape):
    f1, f2, la, lb = inputs(setting, shape)
    return compare(scores(f1, f2, setting[1], torch.float64), scores(f1, f2, setting[1], torch.float32), FWD_ITERS, setting[2], la, lb)


def cu(t):
    return None if t is None else t.cuda()[None]


def gpu_forward(ops, f1, f2, alpha, n_iter, tau, la, lb, variant=0):
    out = ops.sinkhorn_unbalanced(cu(f1), cu(f2), alpha, n_iter, tau=tau, log_a=cu(la), log_b=cu(lb), variant=variant)
    torch.cuda.synchronize()
    return [t[0].cpu() for t in out]   # val, idx, lmax, lsum, lmass, u, v


def check_forward(tag, R, out, variant):
    val, idx, lmax, lsum, lmass, u, v = out
    for t in (val, lmax, lsum, lmass, u, v):
        assert bool(torch.isfinite(t).all()), tag
    assert bool((val >= 0).all())
    a = R["r64"]
    egpu = max(float((u.double() - a["uf"]).abs().max()), float((v.double() - a["v"]).abs().max()))
    lmgpu = float((lmass.double() - a["lmass"]).abs().max())
    dec = R["decided"]
    undecided = 1.0 - float(dec.double().mean())
    mismatch = int((idx.long() != R["idx64"]).any(dim=1)[dec].sum())
    pe = float((val.double() - R["p64"])[dec].abs().max()) if bool(dec.any()) else 0.0
    report(case=tag, variant=variant, e32=R["e32"], e_gpu=egpu, pot_ratio=egpu / R["e32"] if R["e32"] else 0.0, lmass_32=R["lm32"],
           lmass_gpu=lmgpu, lmass_ratio=lmgpu / R["lm32"] if R["lm32"] else 0.0, undecided=undecided, mismatch=mismatch,
           cpu32_mismatch=R["cpu32_mismatch"], pval_e32=R["pe32"], pval_gpu=pe)
    assert egpu <= 4 * R["e32"], "potentials: %g from float64, the fp32 CPU run %g" % (egpu, R["e32"])
    assert lmgpu <= 4 * R["lm32"], "row_lmass: %g from float64, the fp32 CPU run %g" % (lmgpu, R["lm32"])
    assert undecided <= 0.15, "%.1f %% of the rows are undecided" % (100 * undecided)
    assert mismatch == 0, "%d decided rows differ from the float64 columns" % mismatch
    assert pe <= 4 * R["pe32"] + 1e-7, "pi_val: %g from float64, the fp32 CPU run %g" % (pe, R["pe32"])


# ------------------------------------------------------------------ 2. tau = 1 is the balanced operator
@pytest.mark.parametrize("shape", [(257, 129), (1000, 440)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("kind", ["unit", "lowrank"])
def test_tau_one_is_the_balanced_operator(ops, kind, shape):
    f1, f2 = make_clouds(kind, *shape)
    a, b = cu(f1), cu(f2)
    for alpha in (10.0, 100.0):
        for n_iter in (0, 5):
            for variant in (0, 1):
                tag = (kind, shape, alpha, n_iter, variant)
                val, idx, lmax, lsum, u, v = ops.sinkhorn(a, b, alpha, n_iter, variant=variant, potentials=True)
                uval, uidx, ulmax, ulsum, ulmass, uu, uv = ops.sinkhorn_unbalanced(a, b, alpha, n_iter, tau=(1.0, 1.0), variant=variant)
                assert same_bits([uval, uidx, ulmax, ulsum, uu, uv], [val, idx, lmax, lsum, u, v]), tag
                assert bool((ulmass == 0).all()), tag
                hist = ops.sinkhorn_unbalanced_hist(a, b, alpha, n_iter, tau=(1.0, 1.0), variant=variant)
                assert same_bits(hist[:5], [val, idx, lmax, lsum, ulmass]), tag
                assert hist[5].shape == (1, n_iter + 1, shape[0]) and hist[6].shape == (1, n_iter + 1, shape[1])
                assert same_bits([hist[5][:, -1]], [u]), tag   # m^f = u^f at tau = 1
                assert bool((hist[6][:, 0] == 0).all())


# ------------------------------------------------------------------ 3. forward against float64
@pytest.mark.parametrize("case", FWD_CASES, ids=case_id)
def test_forward_against_float64(ops, case):
    setting, shape, n_iter = case
    f1, f2, la, lb = inputs(setting, shape)
    R = fwd_group(setting, shape)[n_iter]
    check_forward(case_id(case), R, gpu_forward(ops, f1, f2, setting[1], n_iter, setting[2], la, lb), 0)


@pytest.mark.parametrize("group", [(s, sh) for s, sh in FWD_GROUPS if sh in SMALL_SHAPES], ids=lambda g: group_id(*g))
def test_forward_scalar_kernel_and_history_entry(ops, group):
    setting, shape = group
    f1, f2, la, lb = inputs(setting, shape)
    R = fwd_group(setting, shape)[5]
    out = gpu_forward(ops, f1, f2, setting[1], 5, setting[2], la, lb, variant=1)
    check_forward(group_id(*group) + "-n5", R, out, 1)
    for variant in (0, 1):   # the history entry is the same run
        plain = ops.sinkhorn_unbalanced(cu(f1), cu(f2), setting[1], 5, tau=setting[2], log_a=cu(la), log_b=cu(lb), variant=variant)
        hist = ops.sinkhorn_unbalanced_hist(cu(f1), cu(f2), setting[1], 5, tau=setting[2], log_a=cu(la), log_b=cu(lb), variant=variant)
        assert same_bits(hist[:5], plain[:5]), (group_id(*group), variant)
        # the potentials re-made from the kept normalisers, a sum and then a product in fp32, are the plain entry's
        la32 = torch.zeros(shape[0]) if la is None else la
        lb32 = torch.full((shape[1],), math.log(shape[0] / shape[1])) if lb is None else lb
        tr, tc = (torch.tensor(t, dtype=torch.float32) for t in setting[2])
        assert same_bits([tr * (la32 + hist[5][0, -1].cpu()), tc * (lb32 + hist[6][0, -1].cpu())], [plain[5][0], plain[6][0]])


def test_other_feature_width_takes_the_scalar_kernel(ops):
    g = torch.Generator().manual_seed(36)
    f1, f2 = 0.3 * torch.randn(70, 36, generator=g), 0.3 * torch.randn(90, 36, generator=g)
    la, lb = log_weights(70, 90)
    tau = (0.9, 0.7)
    R = compare(scores(f1, f2, 10.0, torch.float64), scores(f1, f2, 10.0, torch.float32), (5,), tau, la, lb)[5]
    check_forward("d36-70x90-a10-t0.9_0.7-w-n5", R, gpu_forward(ops, f1, f2, 10.0, 5, tau, la, lb), 0)


def test_underflowing_mass(ops):
    """randn features at alpha = 100: the mass of every row is far below fp32's range (row_lmass ~ -700), which is why it is
    returned as a logarithm.  Every output is finite, row_lmass meets its bar, pi_val is 0 or more — never NaN."""
    f1, f2 = make_clouds("randn", 257, 129)
    tau = (0.5, 0.5)
    R = compare(scores(f1, f2, 100.0, torch.float64), scores(f1, f2, 100.0, torch.float32), (5,), tau, None, None)[5]
    val, idx, lmax, lsum, lmass, u, v = gpu_forward(ops, f1, f2, 100.0, 5, tau, None, None)
    for t in (val, lmax, lsum, lmass, u, v):
        assert bool(torch.isfinite(t).all())
    assert bool((val >= 0).all()) and bool((idx >= 0).all()) and bool((idx < 129).all())
    lmgpu = float((lmass.double() - R["r64"]["lmass"]).abs().max())
    report(case="randn-257x129-a100-t0.5_0.5-n5", lmass_32=R["lm32"], lmass_gpu=lmgpu, lmass_max=float(lmass.max()), val_max=float(val.max()))
    assert float(lmass.max()) < -100.0   # the case does underflow
    assert lmgpu <= 4 * R["lm32"]


# ------------------------------------------------------------------ 4. partial shapes are told apart
def planted_partial():
    g = torch.Generator().manual_seed(7)
    f1 = torch.randn(256, 128, generator=g)
    f1 = f1 / f1.norm(dim=1, keepdim=True)
    perm = torch.randperm(256, generator=g)[:128]
    f2 = f1[perm] + 0.05 * torch.randn(128, 128, generator=g) / math.sqrt(128)
    return f1.contiguous(), f2.contiguous(), perm


def test_partial_shapes_are_told_apart(ops):
    f1, f2, perm = planted_partial()
    matched = torch.zeros(256, dtype=torch.bool)
    matched[perm] = True
    log_b = torch.zeros(128)
    mass = torch.exp(gpu_forward(ops, f1, f2, 30.0, 5, (0.9, 0.9), None, log_b)[4].double())
    ref = compare(scores(f1, f2, 30.0, torch.float64), scores(f1, f2, 30.0, torch.float32), (5,), (0.9, 0.9), None, log_b)[5]["r64"]
    m64 = torch.exp(ref["lmass"])
    report(case="planted-256x128-a30-t0.9-n5", matched_min=float(mass[matched].min()), unmatched_max=float(mass[~matched].max()),
           matched_min_f64=float(m64[matched].min()), unmatched_max_f64=float(m64[~matched].max()))
    assert float(mass[matched].min()) > 0.5, "a matched row lost its mass"
    assert float(mass[~matched].max()) < 0.1, "a row without a partner kept its mass"
    balanced = gpu_forward(ops, f1, f2, 30.0, 5, (1.0, 1.0), None, log_b)[4]
    assert bool((balanced == 0).all()), "tau = (1, 1): every row has mass 1"


# ------------------------------------------------------------------ 5. backward against float64 autograd
def make_grads(N, topk=10, seed=7, B=None):
    g = torch.Generator().manual_seed(seed)
    return torch.randn((N, topk) if B is None else (B, N, topk), generator=g), torch.randn((N,) if B is None else (B, N), generator=g)


def reference_grads(f1, f2, alpha, n_iter, tau, log_a, log_b, idx, gval, gl, dtype):
    """Autograd of the definition in `dtype` on the CPU -> (df1, df2, d_log_a, d_log_b) as float64."""
    N, M = f1.shape[0], f2.shape[0]
    x1 = f1.to(dtype).clone().requires_grad_(True)
    x2 = f2.to(dtype).clone().requires_grad_(True)
    la, lb = (t.clone().requires_grad_(True) for t in weights_of(log_a, log_b, N, M, dtype))
    neg_alpha = float(torch.tensor(-float(alpha), dtype=torch.float32).item())
    S = torch.cdist(x1[None], x2[None])[0] * torch.tensor(neg_alpha, dtype=dtype)
    v = torch.zeros(M, dtype=dtype)
    for _ in range(n_iter):
        u = tau[0] * (la - torch.logsumexp(S + v[None, :], dim=1))
        v = tau[1] * (lb - torch.logsumexp(S + u[:, None], dim=0))
    mf = -torch.logsumexp(S + v[None, :], dim=1)
    uf = tau[0] * (la + mf)
    P = torch.exp(S + uf[:, None] + v[None, :])
    loss = (gval.to(dtype) * P.gather(1, idx.long())).sum() + (gl.to(dtype) * (uf - mf)).sum()
    loss.backward()
    # (at n_iter = 0 the column weights take no part: no gradient reaches them)
    return [torch.zeros_like(t, dtype=torch.float64) if t.grad is None else t.grad.double() for t in (x1, x2, la, lb)]


def rel(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-300))


def gpu_fwd_bwd(ops, f1, f2, alpha, n_iter, tau, la, lb, gval, gl, variant=0):
    """-> [val, idx, lmass, rn_hist, cn_hist, df1, df2, d_log_a, d_log_b] on the device (batched inputs)."""
    val, idx, _, _, lmass, rn, cn = ops.sinkhorn_unbalanced_hist(f1, f2, alpha, n_iter, tau=tau, log_a=la, log_b=lb, variant=variant)
    grads = ops.sinkhorn_unbalanced_bwd(f1, f2, alpha, n_iter, tau, la, lb, val, idx, lmass, rn, cn, gval, gl, variant=variant)
    return [val, idx, lmass, rn, cn] + list(grads)


def check_backward(ops, tag, f1, f2, alpha, n_iter, tau, la, lb, variant):
    gval, gl = make_grads(f1.shape[0])
    out = gpu_fwd_bwd(ops, cu(f1), cu(f2), alpha, n_iter, tau, cu(la), cu(lb), cu(gval), cu(gl), variant)
    torch.cuda.synchronize()
    idx = out[1][0].cpu()
    got = [t[0].cpu() for t in out[5:]]
    assert all(bool(torch.isfinite(t).all()) for t in got), tag
    r64 = reference_grads(f1, f2, alpha, n_iter, tau, la, lb, idx, gval, gl, torch.float64)
    r32 = reference_grads(f1, f2, alpha, n_iter, tau, la, lb, idx, gval, gl, torch.float32)
    assert all(bool(torch.isfinite(t).all()) for t in r32), "the fp32 CPU yardstick is not finite: " + tag
    fig, bad = {}, []
    for name, g, a, b in zip(("df1", "df2", "dla", "dlb"), got, r64, r32):
        e, y = rel(g, a), rel(b, a)
        bar = max(4 * y, 1e-4)
        fig.update({"gpu_" + name: e, "cpu32_" + name: y, "bar_" + name: bar})
        if not e <= bar:
            bad.append(name)
    report(case=tag, variant=variant, **fig)
    assert not bad, (tag, variant, bad, fig)
    return got


@pytest.mark.parametrize("case", BWD_CASES, ids=case_id)
def test_gradient_vs_float64_matrix_cores(ops, case):
    setting, shape, n_iter = case
    f1, f2, la, lb = inputs(setting, shape)
    check_backward(ops, case_id(case), f1, f2, setting[1], n_iter, setting[2], la, lb, 0)


@pytest.mark.parametrize("case", [c for c in BWD_CASES if c[1] in SMALL_SHAPES], ids=case_id)
def test_gradient_vs_float64_scalar_kernels(ops, case):
    setting, shape, n_iter = case
    f1, f2, la, lb = inputs(setting, shape)
    check_backward(ops, case_id(case), f1, f2, setting[1], n_iter, setting[2], la, lb, 1)


def test_gradient_at_tau_one_meets_the_float64_bar(ops):
    """The tau = 1 backward is not dispatched to dvm_sinkhorn_bwd_f32: it runs from the normalisers like every other case and is
    held to the same bar."""
    f1, f2 = make_clouds("lowrank", 257, 129)
    check_backward(ops, "lowrank-257x129-a10-t1_1-n5", f1, f2, 10.0, 5, (1.0, 1.0), None, None, 0)


@pytest.mark.parametrize("variant", [0, 1])
def test_null_g_lmass_is_a_zero_tensor_and_the_node_is_the_raw_call(ops, variant):
    from dvm import nn_ops
    setting, shape = SETTINGS[1], (130, 333)
    f1, f2 = make_clouds(setting[0], *shape)
    la, lb = log_weights(*shape)
    gval, gl = make_grads(shape[0])
    a, b, wa, wb, gv = cu(f1), cu(f2), cu(la), cu(lb), cu(gval)
    val, idx, _, _, lmass, rn, cn = ops.sinkhorn_unbalanced_hist(a, b, setting[1], 5, tau=setting[2], log_a=wa, log_b=wb, variant=variant)
    none = ops.sinkhorn_unbalanced_bwd(a, b, setting[1], 5, setting[2], wa, wb, val, idx, lmass, rn, cn, gv, None, variant=variant)
    zero = ops.sinkhorn_unbalanced_bwd(a, b, setting[1], 5, setting[2], wa, wb, val, idx, lmass, rn, cn, gv, torch.zeros_like(lmass), variant=variant)
    assert same_bits(none, zero)
    if variant == 0:   # (the node runs the automatic variant)
        raw = ops.sinkhorn_unbalanced_bwd(a, b, setting[1], 5, setting[2], wa, wb, val, idx, lmass, rn, cn, gv, cu(gl))
        leaves = [t.clone().requires_grad_(True) for t in (a, b, wa, wb)]
        nval, nidx, nlmass = nn_ops.sinkhorn_unbalanced_topk(leaves[0], leaves[1], setting[1], 5, tau=setting[2], log_a=leaves[2], log_b=leaves[3])
        assert same_bits([nval, nidx, nlmass], [val, idx, lmass]) and nval.requires_grad and nlmass.requires_grad and not nidx.requires_grad
        got = torch.autograd.grad((nval * gv).sum() + (nlmass * cu(gl)).sum(), leaves)
        assert same_bits(got, raw)
        got = torch.autograd.grad(nn_ops.sinkhorn_unbalanced_topk(*leaves[:2], setting[1], 5, tau=setting[2], log_a=leaves[2],
                                                                  log_b=leaves[3])[0].mul(gv).sum(), leaves)   # through val alone
        assert same_bits(got, none)
        with torch.no_grad():   # without grad: the forward-only entry, the same bits
            assert same_bits(nn_ops.sinkhorn_unbalanced_topk(a, b, setting[1], 5, tau=setting[2], log_a=wa, log_b=wb), [val, idx, lmass])
        # n_iter = 0 under grad is this node too (not softcorr_topk): lmass carries a gradient
        z = nn_ops.sinkhorn_unbalanced_topk(leaves[0], leaves[1], setting[1], 0, tau=setting[2])
        assert z[2].requires_grad and float(torch.autograd.grad(z[2].sum(), leaves[0])[0].abs().max()) > 0


# ------------------------------------------------------------------ 6. layout and hygiene, all bit-equal
def batch_inputs():
    g = torch.Generator().manual_seed(3)
    f1, f2 = 0.2 * torch.randn(3, 130, 128, generator=g), 0.2 * torch.randn(3, 333, 128, generator=g)
    f2[1] *= 0.5
    la, lb = log_weights(130, 333, B=3)
    gval, gl = make_grads(130, B=3)
    return [t.cuda() for t in (f1, f2, la, lb, gval, gl)]


def run_all(ops, t, variant, alpha=30.0, n_iter=5, tau=(0.9, 0.7)):
    f1, f2, la, lb, gval, gl = t
    return gpu_fwd_bwd(ops, f1, f2, alpha, n_iter, tau, la, lb, gval, gl, variant)


@pytest.mark.parametrize("variant", [0, 1])
def test_batch_entries_are_their_single_calls_and_runs_repeat(ops, variant):
    t = batch_inputs()
    whole = [x.cpu() for x in run_all(ops, t, variant)]
    again = [x.cpu() for x in run_all(ops, t, variant)]
    assert same_bits(whole, again), "two runs on the same inputs differ"
    for e in range(3):
        one = [x.cpu() for x in run_all(ops, [x[e:e + 1].contiguous() for x in t], variant)]
        assert same_bits([x[e:e + 1] for x in whole], one), "entry %d of a B = 3 call differs from its own B = 1 call" % e
    f1, f2, la, lb, _, _ = t
    plain = ops.sinkhorn_unbalanced(f1, f2, 30.0, 5, tau=(0.9, 0.7), log_a=la, log_b=lb, variant=variant)
    assert same_bits([plain[0], plain[1], plain[4]], whole[:3])


@pytest.mark.parametrize("variant", [0, 1])
def test_result_does_not_depend_on_the_workspace_contents(ops, monkeypatch, variant):
    t = batch_inputs()
    res = []
    for fill in (0x00, 0xFF):   # 0xFF bytes: NaN bit patterns in every float, -1 in every word
        keep = []

        def workspace(nbytes, device, tag, fill=fill, keep=keep):
            keep.append(torch.full((max(int(nbytes), 1),), fill, dtype=torch.uint8, device=device))
            return keep[-1]

        monkeypatch.setattr(ops, "workspace", workspace)
        f1, f2, la, lb, _, _ = t
        plain = ops.sinkhorn_unbalanced(f1, f2, 30.0, 5, tau=(0.9, 0.7), log_a=la, log_b=lb, variant=variant)
        res.append([x.cpu() for x in run_all(ops, t, variant) + list(plain)])
        torch.cuda.synchronize()
    assert same_bits(res[0], res[1]), "the result depends on what the workspace held"
    assert all(bool(torch.isfinite(x).all()) for x in res[1] if x.is_floating_point())


@pytest.mark.parametrize("variant", [0, 1])
def test_capturable(ops, variant):
    """No host synchronisation and no float atomics: forward-with-history + backward on one stream can be captured, and the
    replay on new input contents gives the eager calls' bits."""
    t = batch_inputs()
    eager = [x.clone() for x in run_all(ops, t, variant)]
    static = [(0.5 * x).contiguous() for x in t]   # the captured call's static inputs, other contents at capture time
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            run_all(ops, static, variant)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run_all(ops, static, variant)
    for s, x in zip(static, t):
        s.copy_(x)
    graph.replay()
    torch.cuda.synchronize()
    assert same_bits(out, eager), "the replayed capture differs from the eager calls"


# ------------------------------------------------------------------ 7. criterion
def composed_direction(d, n_iter, tau, feat1, feat2, verts1, verts2, alpha, g1, idx11, idx22, with_map, train):
    """One direction of deform(), written out from models.loss.sinkhorn_pi_unbalanced and the per-op calls of
    GraphDeformLoss_Neural._direction_train (under grad) / _direction (without) -> (map_sum, (cd_warp sides), arap, (cd_self sides))."""
    import models.loss as ml
    from dvm import nn_ops, ops
    B, N, _ = verts1.shape
    iden = torch.tensor([1, 0, 0, 0, 1, 0], dtype=torch.float32, device=verts1.device)
    pi = ml.sinkhorn_pi_unbalanced(feat1, feat2, alpha, n_iter, 10, tau=tau)
    assert pi.log_mass is not None and pi.val.requires_grad == train
    pval, pidx = pi.val, pi.idx
    if not train:
        verts12 = ops.apply(pval, pidx, verts2)
        def9 = d.forward_sparse(feat1, feat2, verts1, verts12, idx11, idx22, pval, pidx, g1["nodes_idx"])
        warped, arap, _ = ops.dg_warp_arap(verts1, g1, ml.rotation_6d_to_matrix(def9[..., 3:] + iden), def9[..., :3].contiguous())
        cw = ops.chamfer(warped, verts2, want_idx=False)[:2]
        cs = ops.chamfer(verts12, verts2, want_idx=False)[:2]
        map_sum = ops.map_term(verts12, verts2, idx11, idx22, pval, pidx) if with_map else None
        return map_sum, cw, arap.sum(), cs
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


def composed_terms(crit, d, n_iter, tau, f1, f2, v1, v2, alpha, starts, partial, train):
    """(deform_loss, map_loss, self_rec_loss) as GraphDeformLoss_Neural.forward reduces the two directions."""
    B, N, _ = v1.shape
    M = v2.shape[1]
    g1, g2, idx11, idx22 = crit.geometry(v1, v2, starts)
    with_map = crit.w_map > 0 and not partial

    def cd(sides, n_src, n_tgt):
        if partial:   # one-sided: the smaller cloud's side
            return torch.mean(sides[0] if n_src <= n_tgt else sides[1])
        return torch.mean(sides[0]) + torch.mean(sides[1])

    m12, w12, a12, s12 = composed_direction(d, n_iter, tau, f1, f2, v1, v2, alpha, g1, idx11, idx22, with_map, train)
    m21, w21, a21, s21 = composed_direction(d, n_iter, tau, f2, f1, v2, v1, alpha, g2, idx22, idx11, with_map, train)
    scale = 1 if partial else N
    deform = ((cd(w12, N, M) * crit.w_cd + a12 * crit.w_arap) + (cd(w21, M, N) * crit.w_cd + a21 * crit.w_arap)) * scale * crit.w_deform / 2
    map_loss = crit.w_map * (m12.sum() / (3 * B) + m21.sum() / (3 * B)) / 2 if with_map else None
    self_rec = (cd(s12, N, M) + cd(s21, M, N)) * scale * crit.w_self_rec / 2
    return deform, map_loss, self_rec


@pytest.mark.parametrize("partial,N,M", [(False, 256, 256), (True, 256, 120)], ids=["full-256x256", "partial-256x120"])
def test_criterion_with_sinkhorn_tau(ops, monkeypatch, partial, N, M):
    from dvm import nn_ops
    from test_gpu_sinkhorn_backward import criterion_setup
    crit, d, f1, f2, v1, v2, starts, anchors = criterion_setup(partial, N, M)
    assert crit.sinkhorn_tau is None
    alpha, tau = 60.0, (0.9, 0.9)
    dist1, dist2 = torch.cdist(v1, v1), torch.cdist(v2, v2)
    crit.sinkhorn_iters = 3

    def step(setting):
        crit.sinkhorn_tau = setting
        d.zero_grad(set_to_none=True)
        f1.grad = f2.grad = None
        random.seed(5)
        out = crit(f1, f2, dist1, dist2, v1, v2, alpha, d, fps_starts=starts, anchors=anchors)
        out[0].backward()
        return [o.detach() if torch.is_tensor(o) else o for o in out], f1.grad.clone(), f2.grad.clone()

    out_t, g1_t, g2_t = step(tau)
    deform, map_loss, self_rec = composed_terms(crit, d, 3, tau, f1, f2, v1, v2, alpha, starts, partial, True)
    close = lambda x, y: abs(float(x) - float(y)) <= 1e-6 * max(abs(float(y)), 1e-30)  # noqa: E731
    assert close(out_t[2], deform) and close(out_t[4], self_rec), (out_t, float(deform), float(self_rec))
    if map_loss is not None:
        assert close(out_t[3], map_loss), (out_t, float(map_loss))
    assert torch.isfinite(g1_t).all() and torch.isfinite(g2_t).all() and float(g1_t.abs().max()) > 0 and float(g2_t.abs().max()) > 0
    with torch.no_grad():   # without grad: the terms built from the forward-only entry
        random.seed(5)
        out = crit(f1, f2, dist1, dist2, v1, v2, alpha, d, fps_starts=starts, anchors=anchors)
        deform0, map0, self0 = composed_terms(crit, d, 3, tau, f1, f2, v1, v2, alpha, starts, partial, False)
    assert close(out[2], deform0) and close(out[4], self0) and (map0 is None or close(out[3], map0))
    # None and (1, 1) take the balanced path: the unbalanced node is never reached, and the two settings give the terms one set of
    # bits (not the gradients: the criterion's other backward nodes add with float atomics, in no fixed order)
    def refuse(*a, **k):
        raise AssertionError("sinkhorn_tau = None / (1, 1) reached the unbalanced operator")
    monkeypatch.setattr(nn_ops, "sinkhorn_unbalanced_topk", refuse)
    out_n, g1_n, g2_n = step(None)
    out_1, g1_1, g2_1 = step((1.0, 1.0))
    terms = lambda o: [x for x in o if torch.is_tensor(x)]  # noqa: E731
    assert same_bits(terms(out_n), terms(out_1))
    assert rel(g1_1, g1_n) < 1e-3 and rel(g2_1, g2_n) < 1e-3   # (the bound the tau = (0.9, 0.9) gradients must exceed below)
    report(case="criterion-%s" % ("partial" if partial else "full"), deform=(float(out_t[2]), float(deform)), deform_balanced=float(out_n[2]),
           self_rec=(float(out_t[4]), float(self_rec)), map=(float(out_t[3]) if map_loss is not None else None,
                                                            None if map_loss is None else float(map_loss)),
           grad_rel_diff_vs_balanced=(rel(g1_t, g1_n), rel(g2_t, g2_n)))
    assert abs(float(out_t[2]) - float(out_n[2])) > 1e-6 * abs(float(out_n[2])), "sinkhorn_tau = (0.9, 0.9) gave the balanced loss"
    assert rel(g1_t, g1_n) > 1e-3 and rel(g2_t, g2_n) > 1e-3, "sinkhorn_tau = (0.9, 0.9) gave the balanced gradient"


# ------------------------------------------------------------------ 8. the drivers' switch
def test_deform_driver_with_sinkhorn_tau(tmp_path, capsys):
    import deform_driver
    from test_gpu_sinkhorn import read_off
    pts = {}
    for tag, extra in (("balanced", []), ("one", ["--sinkhorn-tau", "1"]), ("relaxed", ["--sinkhorn-tau", "0.9,0.8"])):
        deform_driver.main(["--sinkhorn", "5"] + extra + ["--points", "1024", "--out", str(tmp_path / tag)])
        files = json.loads(capsys.readouterr().out.strip().split("\n")[-1])["files"]
        n, xyz = read_off(files[0])
        assert n == 1024 and bool(torch.isfinite(torch.from_numpy(xyz)).all())
        pts[tag] = xyz
    assert (pts["one"] == pts["balanced"]).all(), "--sinkhorn-tau 1 changed the deformation"
    assert abs(pts["relaxed"] - pts["balanced"]).max() > 1e-6, "--sinkhorn-tau 0.9,0.8 did not change the deformation"


def test_train_driver_with_sinkhorn_tau(capsys):
    import train_driver
    rc = train_driver.main(["--sinkhorn", "3", "--sinkhorn-tau", "0.9,0.8", "--steps", "2", "--warmup", "0", "--batch", "2", "--points", "256"])
    assert rc in (0, None)
    line = json.loads(capsys.readouterr().out.strip().split("\n")[-1])
    assert line["sinkhorn_iters"] == 3 and line["sinkhorn_tau"] == [0.9, 0.8] and line["steps"] == 2
    assert all(math.isfinite(float(x)) for x in line["last_losses"])
