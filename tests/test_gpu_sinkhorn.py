"""-m gpu: the Sinkhorn-normalised soft correspondence (ops.sinkhorn / dvm_sinkhorn_fwd_f32).

The operator is not in the reference, so it is pinned to two things: at n_iter = 0 to the existing row-softmax operator
(ops.softcorr, itself pinned to the reference), and otherwise to a float64 evaluation of its definition, computed here on
the CPU (torch.cdist in float64 on the fp32 inputs cast up, neg_alpha = float32(-alpha) cast up, torch.logsumexp).  An
fp32 run of the same lines is the yardstick for rounding: the GPU may be off by 4 x what that run is off by (tile-wise
summation order, 1-ulp hardware exp / log).  Neither reads the code under test.

Every case prints its measured figures (run with -s); profiles/notes_sinkhorn.md records them."""
import functools
import json
import math
import os

import numpy as np
import pytest
import torch

from oracle import oracle as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MiB = 1 << 20
KINDS = ("randn", "unit", "lowrank")
SHAPES = ((2048, 2048), (1000, 440))
ALPHAS = (10.0, 100.0)
ITERS = (0, 5, 20)
CASES = [(k, s, a, n) for k in KINDS for s in SHAPES for a in ALPHAS for n in ITERS]   # n_iter fastest: one float64 run per group
SMALL = [c for c in CASES if c[1] == (1000, 440)]


def case_id(c):
    return "%s-%dx%d-a%g-n%d" % (c[0], c[1][0], c[1][1], c[2], c[3])


@pytest.fixture(scope="module")
def ops():
    from dvm import ops as _ops
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _ops


def make_clouds(kind, N, M):
    g = torch.Generator().manual_seed(1)

    def cloud(n):
        x = torch.randn(n, 128, generator=g)
        if kind == "randn":
            return x
        if kind == "unit":
            return x / x.norm(dim=1, keepdim=True)
        z = torch.randn(n, 8, generator=g)
        A = torch.randn(8, 128, generator=g) / math.sqrt(8)
        return ((z @ A) * 0.3 + 0.02 * x).contiguous()

    f1 = cloud(N)
    return f1, cloud(M)


def neg_alpha_of(alpha):
    return float(torch.tensor(-float(alpha), dtype=torch.float32).item())


def scores(f1, f2, alpha, dtype, compute_mode="use_mm_for_euclid_dist_if_necessary"):
    D = torch.cdist(f1.to(dtype)[None], f2.to(dtype)[None], compute_mode=compute_mode)[0]
    return D * torch.tensor(neg_alpha_of(alpha), dtype=dtype)


def final_step(S, v):
    """The last row step of the definition: L, row_lmax, row_sum, u."""
    L = S + v[None, :]
    lmax = L.max(dim=1).values
    rsum = torch.exp(L - lmax[:, None]).sum(dim=1)
    return L, lmax, rsum, -(lmax + torch.log(rsum))


def sinkhorn_reference(S, n_iters, N, M):
    """{n_iter: (L, lmax, rsum, u, v)} for every n_iter asked for, from ONE run of the iteration in S's dtype."""
    v = torch.zeros(M, dtype=S.dtype)
    out = {}
    for it in range(max(n_iters) + 1):
        if it in n_iters:
            out[it] = final_step(S, v) + (v.clone(),)
        u = -torch.logsumexp(S + v[None, :], dim=1)
        v = math.log(N / M) - torch.logsumexp(S + u[:, None], dim=0)
    return out


def ranked(L, k):
    """Top-k logits per row, descending, ties -> lowest column (values that agree to 1e-9 count as tied: duplicated
    columns may differ in the last float64 bits)."""
    k = min(k, L.shape[1])
    val, idx = torch.topk(L, min(k + 2, L.shape[1]), dim=1)
    val, idx = val.numpy(), idx.numpy()
    for r in np.nonzero((np.abs(np.diff(val, axis=1)) < 1e-9).any(axis=1))[0]:
        t, ncol = 0, val.shape[1]
        while t < ncol:
            e = t
            while e + 1 < ncol and abs(val[r, e + 1] - val[r, e]) < 1e-9:
                e += 1
            seg = np.argsort(idx[r, t:e + 1], kind="stable")
            idx[r, t:e + 1] = idx[r, t:e + 1][seg]
            val[r, t:e + 1] = val[r, t:e + 1][seg]
            t = e + 1
    return torch.from_numpy(val[:, :k].copy()), torch.from_numpy(idx[:, :k].copy())


@functools.lru_cache(maxsize=2)
def group(kind, N, M, alpha, iters=ITERS):
    """Everything the checks need of the float64 and the fp32 CPU runs of one (features, shape, alpha) group."""
    f1, f2 = make_clouds(kind, N, M)
    S64 = scores(f1, f2, alpha, torch.float64)
    smax = float(S64.abs().max())
    r64 = sinkhorn_reference(S64, iters, N, M)
    r32 = sinkhorn_reference(scores(f1, f2, alpha, torch.float32), iters, N, M)
    out = {}
    for n in iters:
        L64, lmax64, rsum64, u64, v64 = r64[n]
        L32, lmax32, rsum32, u32, v32 = r32[n]
        t11, _ = ranked(L64, 11)
        decided = ((t11[:, :-1] - t11[:, 1:]) >= 64 * 2.0 ** -24 * smax).all(dim=1)
        tv, ti = ranked(L64, 10)
        p64 = torch.exp(tv - lmax64[:, None]) / rsum64[:, None]
        p32 = (torch.exp(L32.gather(1, ti) - lmax32[:, None]) / rsum32[:, None]).double()
        i32 = ranked(L32.double(), 10)[1]
        out[n] = dict(u64=u64, v64=v64, u32=u32.double(), v32=v32.double(), decided=decided, idx64=ti, p64=p64,
                      e32=max(float((u32.double() - u64).abs().max()), float((v32.double() - v64).abs().max())),
                      pe32=float((p32 - p64)[decided].abs().max()) if bool(decided.any()) else 0.0,
                      cpu32_mismatch=int((i32 != ti).any(dim=1)[decided].sum()))
    return dict(f1=f1, f2=f2, S64=S64, smax=smax, n=out)


def gpu_run(ops, f1, f2, alpha, n_iter, variant=0, topk=10):
    out = ops.sinkhorn(f1.cuda()[None], f2.cuda()[None], alpha, n_iter, topk=topk, variant=variant, potentials=True)
    torch.cuda.synchronize()
    return [t[0].cpu() for t in out]   # pi_val, pi_idx, row_lmax, row_sum, u, v


def marginals(S64, u, v, N, M):
    """(max |rowsum - 1|, max |colsum * M / N - 1|, max |colsum - 1|) of P = exp(S + u + v), float64 on the host."""
    P = torch.exp(S64 + u.double()[:, None] + v.double()[None, :])
    rs, cs = P.sum(dim=1), P.sum(dim=0)
    return float((rs - 1).abs().max()), float((cs * M / N - 1).abs().max()), float((cs - 1).abs().max())


def report(**kw):
    print("SINKHORN " + json.dumps(kw, sort_keys=True))


def bits(t):
    t = t.detach().contiguous().cpu()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def same_bits(a, b):
    return all(torch.equal(bits(x), bits(y)) for x, y in zip(a, b))


# ------------------------------------------------------------------ 1. n_iter = 0 is the existing operator
@pytest.mark.parametrize("case", [c for c in CASES if c[3] == 0], ids=case_id)
def test_zero_iterations_equal_softcorr(ops, case):
    kind, (N, M), alpha, _ = case
    f1, f2 = make_clouds(kind, N, M)
    val, idx, lmax, lsum, u, v = gpu_run(ops, f1, f2, alpha, 0)
    sval, sidx, ssmax, ssum = [t[0].cpu() for t in ops.softcorr(f1.cuda()[None], f2.cuda()[None], alpha, variant=2)]
    assert torch.equal(idx, sidx), "top-k columns differ from ops.softcorr"
    assert torch.equal(bits(lmax), bits(ssmax)), "row_lmax is not bit-equal to row_smax"
    np.testing.assert_allclose(lsum.numpy(), ssum.numpy(), rtol=2e-5)
    np.testing.assert_allclose(val.numpy(), sval.numpy(), rtol=5e-5, atol=1e-30)
    assert bool((v == 0).all())
    np.testing.assert_allclose(u.numpy(), -(lmax.double() + lsum.double().log()).numpy(), rtol=1e-6, atol=1e-6)
    if case == ("randn", (1000, 440), 100.0, 0):   # and against the C oracle directly
        oval, oidx, osmax, osum = O.softcorr(f1.numpy(), f2.numpy(), alpha, topk=10)
        assert np.array_equal(idx.numpy(), oidx)
        np.testing.assert_array_equal(lmax.numpy(), osmax)
        np.testing.assert_allclose(lsum.numpy(), osum, rtol=2e-5)
        np.testing.assert_allclose(val.numpy(), oval, rtol=5e-5, atol=1e-30)


# ------------------------------------------------------------------ 2. - 4. against float64
def check_against_float64(ops, case, variant):
    kind, (N, M), alpha, n_iter = case
    G = group(kind, N, M, alpha)
    R = G["n"][n_iter]
    val, idx, lmax, lsum, u, v = gpu_run(ops, G["f1"], G["f2"], alpha, n_iter, variant=variant)
    for t in (val, lmax, lsum, u, v):
        assert bool(torch.isfinite(t).all())
    # 2. potentials
    egpu = max(float((u.double() - R["u64"]).abs().max()), float((v.double() - R["v64"]).abs().max()))
    # 3. columns and values on decided rows
    dec = R["decided"]
    undecided = 1.0 - float(dec.double().mean())
    mismatch = int((idx.long() != R["idx64"]).any(dim=1)[dec].sum())
    pe = float((val.double() - R["p64"])[dec].abs().max())
    # 4. marginals of P = exp(S64 + u + v)
    row_gpu, colr_gpu, col_gpu = marginals(G["S64"], u, v, N, M)
    row_32, colr_32, col_32 = marginals(G["S64"], R["u32"], R["v32"], N, M)
    report(case=case_id(case), variant=variant, e32=R["e32"], e_gpu=egpu, pot_ratio=egpu / R["e32"] if R["e32"] else 0.0,
           undecided=undecided, mismatch=mismatch, cpu32_mismatch=R["cpu32_mismatch"], pval_e32=R["pe32"], pval_gpu=pe,
           row_32=row_32, row_gpu=row_gpu, colrel_32=colr_32, colrel_gpu=colr_gpu, col_gpu=col_gpu)
    assert egpu <= 4 * R["e32"], "potentials: %g from float64, the fp32 CPU run %g" % (egpu, R["e32"])
    assert undecided <= 0.15, "%.1f %% of the rows are undecided" % (100 * undecided)
    assert mismatch == 0, "%d decided rows differ from the float64 columns" % mismatch
    assert pe <= 4 * R["pe32"] + 1e-7, "pi_val: %g from float64, the fp32 CPU run %g" % (pe, R["pe32"])
    assert row_gpu <= 4 * row_32, "row sums: %g, the fp32 CPU run %g" % (row_gpu, row_32)
    if kind == "unit" and alpha == 10.0 and n_iter in (5, 20):   # the cases that converge
        assert colr_gpu <= 4 * colr_32, "column sums: %g, the fp32 CPU run %g" % (colr_gpu, colr_32)
    return idx, u, v, R


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_against_float64(ops, case):
    check_against_float64(ops, case, 0)


@pytest.mark.parametrize("case", SMALL, ids=case_id)
def test_scalar_variant_against_float64_and_matrix_cores(ops, case):
    kind, (N, M), alpha, n_iter = case
    idx1, u1, v1, R = check_against_float64(ops, case, 1)
    G = group(kind, N, M, alpha)
    _, idx0, _, _, u0, v0 = gpu_run(ops, G["f1"], G["f2"], alpha, n_iter, variant=0)
    dec = R["decided"]
    assert torch.equal(idx1[dec], idx0[dec])
    assert float((u1 - u0).abs().max()) <= 4 * R["e32"] and float((v1 - v0).abs().max()) <= 4 * R["e32"]


def test_columns_even_out_on_lowrank_features(ops):
    """The reason the operator exists: on low-rank features the row softmax piles the mass of ~170 rows on one column;
    the column sums of P must come down to 1."""
    N = M = 2048
    G = group("lowrank", N, M, 10.0)
    col = {}
    for n_iter in ITERS:
        _, _, _, _, u, v = gpu_run(ops, G["f1"], G["f2"], 10.0, n_iter)
        col[n_iter] = marginals(G["S64"], u, v, N, M)[2]
    report(case="lowrank-2048x2048-a10", colsum_err=col)
    assert col[0] > 1.0 and col[5] < col[0]
    assert col[5] < 0.2
    assert col[20] < 1e-3


# ------------------------------------------------------------------ 5. deterministic and hygienic
class PoisonedScratch:
    """The mechanism of tests/test_gpu_scratch_hygiene.py: every workspace is a fresh buffer of exactly the queried size,
    filled with one byte and framed by two 1 MiB guard bands of the same byte."""

    def __init__(self, fill):
        self.fill, self.bufs = fill, []

    def workspace(self, nbytes, device, tag="ws"):
        n = int(nbytes)
        full = torch.full((n + 2 * MiB,), self.fill, dtype=torch.uint8, device=device)
        self.bufs.append((full, n))
        return full[MiB:MiB + n]

    def check_guards(self):
        torch.cuda.synchronize()
        bad = [(i, n) for i, (full, n) in enumerate(self.bufs)
               if not (bool((full[:MiB] == self.fill).all()) and bool((full[MiB + n:] == self.fill).all()))]
        assert not bad, "writes past the queried workspace size (buffer #, bytes): %s" % bad


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("n_iter", [0, 5])
def test_deterministic_on_poisoned_scratch(ops, monkeypatch, n_iter, variant):
    f1, f2 = make_clouds("randn", 1000, 440)
    for potentials in (True, False):   # with the caller's u / v, and with the workspace's
        def call():
            out = ops.sinkhorn(f1.cuda()[None], f2.cuda()[None], 100.0, n_iter, variant=variant, potentials=potentials)
            torch.cuda.synchronize()
            return [t.cpu() for t in out]

        clean = PoisonedScratch(0x00)
        monkeypatch.setattr(ops, "workspace", clean.workspace)
        a, b = call(), call()
        clean.check_guards()
        assert same_bits(a, b), "two runs on the same inputs differ"
        poison = PoisonedScratch(0xFF)
        monkeypatch.setattr(ops, "workspace", poison.workspace)
        junk = [torch.full(t.shape, float("nan"), device="cuda") if t.is_floating_point()
                else torch.full(t.shape, 0x7f7f7f7f, dtype=t.dtype, device="cuda") for t in a]
        torch.cuda.synchronize()
        del junk   # the caching allocator hands these blocks back as the outputs
        c = call()
        poison.check_guards()
        assert same_bits(a, c), "the result depends on what the workspace / the outputs held"
        if not potentials:
            full = ops.sinkhorn(f1.cuda()[None], f2.cuda()[None], 100.0, n_iter, variant=variant, potentials=True)
            assert same_bits(a, [t.cpu() for t in full[:4]]), "the result depends on whether u / v are asked for"


def test_capturable(ops):
    """A fixed iteration count and no host synchronisation: the call can be captured, and the replay on new input contents
    gives the eager call's bits."""
    f1, f2 = make_clouds("randn", 1000, 440)
    a, b = f1.cuda()[None], f2.cuda()[None]
    eager = [t.clone() for t in ops.sinkhorn(a, b, 100.0, 5, potentials=True)]
    sa, sb = (0.5 * a).contiguous(), (0.5 * b).contiguous()   # the captured call's static inputs, other contents at capture time
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            ops.sinkhorn(sa, sb, 100.0, 5, potentials=True)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.sinkhorn(sa, sb, 100.0, 5, potentials=True)
    sa.copy_(a)
    sb.copy_(b)
    graph.replay()
    torch.cuda.synchronize()
    assert same_bits(out, eager), "the replayed capture differs from the eager call"


# ------------------------------------------------------------------ 6. edges
def test_batch_entries_are_independent(ops):
    g = torch.Generator().manual_seed(3)
    f1, f2 = torch.randn(3, 300, 128, generator=g), torch.randn(3, 200, 128, generator=g)
    f2[1] *= 0.5
    whole = [t.cpu() for t in ops.sinkhorn(f1.cuda(), f2.cuda(), 30.0, 5, potentials=True)]
    for b in range(3):
        one = [t.cpu() for t in ops.sinkhorn(f1[b:b + 1].cuda(), f2[b:b + 1].cuda(), 30.0, 5, potentials=True)]
        assert same_bits([t[b:b + 1] for t in whole], one), "entry %d of a B = 3 call differs from its own B = 1 call" % b


def small_case(ops, f1, f2, alpha, n_iter, variant, topk=10):
    """A small shape against float64 by the rules of points 2 - 4 (decided rows only for the columns)."""
    N, M = f1.shape[0], f2.shape[0]
    S64 = scores(f1, f2, alpha, torch.float64, "donot_use_mm_for_euclid_dist")
    r64 = sinkhorn_reference(S64, (n_iter,), N, M)[n_iter]
    r32 = sinkhorn_reference(scores(f1, f2, alpha, torch.float32), (n_iter,), N, M)[n_iter]
    val, idx, lmax, lsum, u, v = gpu_run(ops, f1, f2, alpha, n_iter, variant=variant, topk=topk)
    e32 = max(float((r32[3].double() - r64[3]).abs().max()), float((r32[4].double() - r64[4]).abs().max()))
    egpu = max(float((u.double() - r64[3]).abs().max()), float((v.double() - r64[4]).abs().max()))
    report(case="edge-%dx%d-a%g-n%d" % (N, M, alpha, n_iter), variant=variant, e32=e32, e_gpu=egpu)
    assert egpu <= 4 * e32
    k = min(topk, M)
    t, _ = ranked(r64[0], k + 1)
    gaps = t[:, :-1] - t[:, 1:]
    thr = 64 * 2.0 ** -24 * float(S64.abs().max())
    ok = ((gaps >= thr) | (gaps.abs() < 1e-9)).all(dim=1)   # decided, or an exact tie (duplicated columns)
    tv, ti = ranked(r64[0], k)
    assert float(ok.double().mean()) >= 0.85
    assert torch.equal(idx[:, :k].long()[ok], ti[ok]), "columns differ from float64 order (ties -> lowest column)"
    p64 = torch.exp(tv - r64[1][:, None]) / r64[2][:, None]
    p32 = (torch.exp(r32[0].gather(1, ti) - r32[1][:, None]) / r32[2][:, None]).double()
    assert float((val[:, :k].double() - p64)[ok].abs().max()) <= 4 * float((p32 - p64)[ok].abs().max()) + 1e-7
    if k < topk:   # slots beyond M: value 0, column 0, as ops.softcorr writes them
        assert bool((val[:, k:] == 0).all()) and bool((idx[:, k:] == 0).all())
    return val, idx


@pytest.mark.parametrize("variant", [0, 1])
def test_fewer_columns_than_topk(ops, variant):
    g = torch.Generator().manual_seed(7)
    f1, f2 = torch.randn(150, 128, generator=g), torch.randn(7, 128, generator=g)
    small_case(ops, f1, f2, 1.0, 5, variant)
    val, idx = small_case(ops, f1, f2, 1.0, 0, variant)
    sval, sidx, _, _ = ops.softcorr(f1.cuda()[None], f2.cuda()[None], 1.0, variant=2)
    assert torch.equal(idx, sidx[0].cpu()) and torch.equal(val[:, 7:], sval[0].cpu()[:, 7:])


@pytest.mark.parametrize("variant", [0, 1])
def test_ragged_tiles(ops, variant):
    g = torch.Generator().manual_seed(257)
    f1, f2 = torch.randn(257, 128, generator=g), torch.randn(63, 128, generator=g)
    for n_iter in (0, 5):
        small_case(ops, 0.2 * f1, 0.2 * f2, 10.0, n_iter, variant)
        small_case(ops, 0.2 * f1, 0.2 * f2, 10.0, n_iter, variant, topk=16)


def test_other_feature_widths_take_the_scalar_kernel(ops):
    g = torch.Generator().manual_seed(36)
    for d in (36, 64):
        f1, f2 = torch.randn(100, d, generator=g), torch.randn(90, d, generator=g)
        small_case(ops, 0.3 * f1, 0.3 * f2, 10.0, 5, 0)


@pytest.mark.parametrize("variant", [0, 1])
def test_duplicated_target_rows_tie_to_the_lowest_column(ops, variant):
    g = torch.Generator().manual_seed(11)
    f1, half = 0.2 * torch.randn(257, 128, generator=g), 0.2 * torch.randn(100, 128, generator=g)
    f2 = torch.cat([half, half], 0).contiguous()   # column j + 100 duplicates column j
    for n_iter in (0, 5):
        val, idx = small_case(ops, f1, f2, 10.0, n_iter, variant)
        # every row's list is pairs (j, j + 100) with equal values, the lower column first
        assert torch.equal(idx[:, 0::2] + 100, idx[:, 1::2]) and torch.equal(bits(val[:, 0::2]), bits(val[:, 1::2]))


def test_underflowing_tails(ops):
    """alpha = 150 on randn features: every row's tail underflows.  Nothing may turn into NaN / Inf on the way."""
    N = M = 2048
    G = group("randn", N, M, 150.0, (20,))
    R = G["n"][20]
    val, idx, lmax, lsum, u, v = gpu_run(ops, G["f1"], G["f2"], 150.0, 20)
    for t in (val, lmax, lsum, u, v):
        assert bool(torch.isfinite(t).all())
    assert bool((val >= 0).all()) and bool((idx >= 0).all()) and bool((idx < M).all())
    row_gpu = marginals(G["S64"], u, v, N, M)[0]
    row_32 = marginals(G["S64"], R["u32"], R["v32"], N, M)[0]
    report(case="randn-2048x2048-a150-n20", row_32=row_32, row_gpu=row_gpu)
    assert row_gpu <= 4 * row_32


# ------------------------------------------------------------------ 7. consumers
def test_sparse_consumers(ops):
    import models.loss as ml
    f1, f2 = make_clouds("lowrank", 1000, 440)
    g = torch.Generator().manual_seed(5)
    verts2 = torch.rand(1, 440, 3, generator=g)
    val, idx, _, _ = ops.sinkhorn(f1.cuda()[None], f2.cuda()[None], 100.0, 5)
    v12 = ops.apply(val, idx, verts2.cuda())
    np.testing.assert_array_equal(v12[0].cpu().numpy(), O.apply(val[0].cpu().numpy(), idx[0].cpu().numpy(), verts2[0].numpy()))
    pi = ml.sinkhorn_pi(f1.cuda()[None], f2.cuda()[None], alpha=100, n_iter=5, topk=10)
    assert isinstance(pi, ml.SparsePi) and pi.M == 440
    assert torch.equal(pi.idx, idx) and torch.equal(bits(pi.val), bits(val))
    dense = pi.to_dense()
    assert dense.shape == (1, 1000, 440)
    assert torch.equal(dense.gather(-1, idx.long()), val) and int((dense != 0).sum()) == int((val != 0).sum())
    np.testing.assert_array_equal(pi.matmul(verts2.cuda()).cpu().numpy(), v12.cpu().numpy())


def read_off(path):
    with open(path) as f:
        lines = f.read().split("\n")
    assert lines[0] == "OFF"
    n = int(lines[1].split()[0])
    return n, np.array([[float(x) for x in ln.split()] for ln in lines[2:2 + n]])


def test_deform_driver_with_sinkhorn(tmp_path, capsys):
    import deform_driver
    pts = {}
    for tag, extra in (("softmax", []), ("sinkhorn", ["--sinkhorn", "5"])):
        out = str(tmp_path / tag)
        deform_driver.main(extra + ["--points", "1024", "--out", out])
        files = json.loads(capsys.readouterr().out.strip().split("\n")[-1])["files"]
        assert len(files) == 1
        n, xyz = read_off(files[0])
        assert n == 1024 and xyz.shape == (1024, 3) and np.isfinite(xyz).all()
        pts[tag] = xyz
    assert np.abs(pts["sinkhorn"] - pts["softmax"]).max() > 1e-6, "--sinkhorn did not change the deformation"
