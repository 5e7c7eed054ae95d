"""-m gpu: the weight-gradient GEMM (csrc/dvm_gemm.hip::linear_wgrad_kernel, dW = gy^T x over the rows) per ELEMENT on every route it
takes — fp32 atomics over row chunks (dvm_linear_wgrad_f32), ordered per-chunk partials (dvm_linear_wgrad_ws_f32 under
dvm_set_deterministic), `out=` adding into a live buffer, and the batched launch behind the criterion node's dist term — and the
decoder backward's other uses of the GEMM kernels: the dX product (the forward GEMM, roles swapped) and the ELU epilogue.

Exact families (tests/wgrad_ref.py): integer-valued inputs whose every partial sum is below 2^24, so the answer is one bit pattern
whatever the order; rows planted on the edges of the library's row split decode a wrong element into the row that was dropped or
counted twice.  Float families: per element within R 2^-24 (|gy|^T |x|), the any-order summation bound.  Order: one chunk is the
row-ordered fmaf chain (oracle/dvm_oracle.c), the deterministic route adds the chunks' chains in chunk order, then once into dW.
Measured ratios: profiles/notes_wgrad_elements.md."""
import contextlib
import ctypes
import random

import numpy as np
import pytest
import torch

from oracle import oracle as O

import wgrad_ref as WR

pytestmark = pytest.mark.gpu

GUARD = 67            # floats on either side of `out` (an odd count: `out` starts off the 16-byte grid)
SENTINEL = 12345.0
ROUTES = ("atomic", "deterministic", "out", "out_deterministic")


@pytest.fixture(scope="module")
def ops():
    from dvm import ops as _ops
    assert torch.cuda.is_available()
    return _ops


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@contextlib.contextmanager
def _deterministic(ops, on):
    prev = ops.set_deterministic(on)
    try:
        yield
    finally:
        ops.set_deterministic(prev)


def _pattern(n):
    return ((np.arange(n) * 7) % 201 - 100).astype(np.float32)


def _run(ops, route, gy, x, base=None):
    """-> (dW as numpy (Co,K), what `out` held before (zeros without `out`)).  `out` is a view into a larger buffer whose guard
    elements must come back untouched."""
    Co, K = gy.shape[1], x.shape[1]
    with _deterministic(ops, route.endswith("deterministic")):
        assert ops.is_deterministic() == route.endswith("deterministic")
        if not route.startswith("out"):
            return ops.linear_wgrad(gy, x).cpu().numpy(), np.zeros((Co, K), np.float32)
        n = Co * K
        base = _pattern(n) if base is None else np.asarray(base, np.float32).reshape(-1)
        big = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
        big[GUARD:GUARD + n] = _cuda(base)
        out = big[GUARD:GUARD + n].view(Co, K)
        res = ops.linear_wgrad(gy, x, out=out)
        assert res.data_ptr() == out.data_ptr()
        host = big.cpu().numpy()
    assert (host[:GUARD] == SENTINEL).all() and (host[GUARD + n:] == SENTINEL).all(), "%s: guard elements around `out` were written" % route
    return host[GUARD:GUARD + n].reshape(Co, K).copy(), base.reshape(Co, K)


# ----------------------------------------------------------------------------------------------------------------------- the split
def test_row_split_is_the_librarys(ops):
    """wgrad_ref.row_split against dvm_linear_wgrad_workspace_bytes (one [Co][K] fp32 slice per chunk, rounded up to the arena's
    alignment): the rows the exact families plant sit on the edges of the split the library really uses."""
    from dvm import _lib
    lib = _lib.load()
    cases = WR.exact_cases() + [(R, Co, K) for Co, K in WR.SHAPES for R in WR.FLOAT_R] + [(16384, 1152, 384), (16384, 64, 64), (5000, 9, 262)]
    for R, Co, K in cases:
        rchunk, chunks = WR.row_split(R, Co, K)
        assert Co * K * 4 > WR.ARENA_ALIGN      # (so the byte count identifies the chunk count)
        nb = lib.dvm_linear_wgrad_workspace_bytes(R, Co, K)
        lo = chunks * Co * K * 4
        assert lo <= nb <= lo + WR.ARENA_ALIGN, (R, Co, K, rchunk, chunks, nb)


# ------------------------------------------------------------------------------------------------------------------ exact families
@pytest.mark.parametrize("R,Co,K", WR.exact_cases())
def test_exact_families_every_route(ops, R, Co, K):
    complaints = []
    for name in ("rows_bitmask", "outer_index", "ints"):        # the families that name the row or the element report first
        gy, x = WR.exact_family(name, R, Co, K)
        want = WR.exact_product(gy, x)
        gyd, xd = _cuda(gy), _cuda(x)
        for route in ROUTES:
            got, base = _run(ops, route, gyd, xd)
            expected = want + base.astype(np.int64)
            assert got.dtype == np.float32 and np.abs(expected).max() < 2 ** 24
            if not torch.equal(torch.from_numpy(got).double(), torch.from_numpy(expected).double()):
                complaints.append("%s route: %s" % (route, WR.explain(name, got, expected, R, Co, K)))
    assert not complaints, "\n".join(complaints)


# ------------------------------------------------------------------------------------------------------------------ float families
@pytest.mark.parametrize("R", WR.FLOAT_R)
@pytest.mark.parametrize("Co,K", WR.SHAPES)
def test_float_families_within_the_summation_bound(ops, Co, K, R):
    for name in WR.FLOAT_FAMILIES:
        gy, x = WR.float_family(name, R, Co, K)
        gyd, xd = _cuda(gy), _cuda(x)
        for route in ("atomic", "deterministic"):
            got, _ = _run(ops, route, gyd, xd)
            ratio, nonzero = WR.worst_ratio(got, gy, x)
            print("RATIO wgrad %s %s Co=%d K=%d R=%d: %.4f" % (name, route, Co, K, R, ratio))
            assert nonzero == 0, "%s %s: %d elements with bound 0 are not exactly 0" % (name, route, nonzero)
            if ratio > 1.0:
                err, b = np.abs(got.astype(np.float64) - WR.ref64(gy, x)), WR.bound(gy, x)
                co, k = np.unravel_index(np.argmax(np.where(b > 0, err / np.where(b > 0, b, 1), 0)), b.shape)
                pytest.fail("%s %s R=%d: dW[%d,%d] errs by %.3e, bound %.3e (ratio %.2f)" % (name, route, R, co, k, err[co, k], b[co, k], ratio))


# ------------------------------------------------------------------------------------------------------------------ order
def _chain(gy, x):
    """The row-ordered fmaf chain started at 0: dW[co][k] = fma(gy[r][co], x[r][k], acc) for r ascending — oracle.linear on the
    transposed operands while the reduction length is ONE K-block of dvo_linear (dvo_gemm_kblocks: R <= 384).  Longer chains (R = 511,
    the 512- and 488-row chunks of R = 1000) would come back as two blocks' totals added; they run on dvo_dot_chain, the oracle's raw
    chain fmaf(-2 a, b, acc), with a = -gy / 2 (both scalings exact)."""
    a, b = np.ascontiguousarray(gy.T), np.ascontiguousarray(x.T)
    starts = (ctypes.c_int * 34)()
    if O.lib().dvo_gemm_kblocks(gy.shape[0], starts, 33) == 1:
        return O.linear(a, b)
    assert np.abs(a[a != 0]).min() > 1e-30
    return O.dot_chain(np.float32(-0.5) * a, b)


def _ordered_partials(gy, x, Co, K):
    """p_0 + p_1 + ... in chunk order (float32), every p the chain of its chunk's rows"""
    t = None
    for b, e in WR.chunk_ranges(gy.shape[0], Co, K):
        p = _chain(gy[b:e], x[b:e])
        t = p if t is None else t + p
    assert t.dtype == np.float32
    return t


def _first_diff(got, want):
    bad = np.argwhere(got != want)
    return "%d elements differ, first dW[%d,%d] = %r, expected %r" % (len(bad), bad[0][0], bad[0][1], float(got[tuple(bad[0])]),
                                                                      float(want[tuple(bad[0])]))


@pytest.mark.parametrize("R", [1, 31, 32, 33, 511])
@pytest.mark.parametrize("Co,K", WR.SHAPES)
def test_one_chunk_is_the_row_ordered_chain_on_both_routes(ops, Co, K, R):
    assert WR.row_split(R, Co, K)[1] == 1
    gy, x = WR.float_family("randn", R, Co, K, seed=1)
    want = _chain(gy, x)
    for route in ("atomic", "deterministic"):
        got, _ = _run(ops, route, _cuda(gy), _cuda(x))
        assert np.array_equal(got, want), "%s: %s" % (route, _first_diff(got, want))


@pytest.mark.parametrize("R", [512, 513, 1000])
@pytest.mark.parametrize("Co,K", WR.SHAPES)
def test_deterministic_route_adds_chunk_chains_in_chunk_order(ops, Co, K, R):
    """dW = out0 + (p0 + p1) in float32 (wgrad_reduce_kernel: the partials first, then one add into dW).  With dW zeroed the atomic
    route gives the same bits while there are two chunks: 0 + p0 + p1 and 0 + p1 + p0 are one rounding of the same two numbers."""
    assert WR.row_split(R, Co, K)[1] == 2
    gy, x = WR.float_family("randn", R, Co, K, seed=1)
    out0 = np.random.default_rng(R).standard_normal((Co, K)).astype(np.float32)
    parts = _ordered_partials(gy, x, Co, K)
    gyd, xd = _cuda(gy), _cuda(x)
    got, base = _run(ops, "out_deterministic", gyd, xd, base=out0)
    want = base + parts
    assert want.dtype == np.float32 and np.array_equal(got, want), _first_diff(got, want)
    for route in ("atomic", "deterministic"):
        got, _ = _run(ops, route, gyd, xd)
        assert np.array_equal(got, parts), "%s: %s" % (route, _first_diff(got, parts))


@pytest.mark.parametrize("Co,K", [s for s in WR.SHAPES if WR.one_tile(*s)])
def test_deterministic_route_repeats_its_bits_at_57_chunks(ops, Co, K):
    R = 16401
    assert WR.row_split(R, Co, K) == (288, 57)
    gy, x = WR.float_family("randn", R, Co, K, seed=1)
    gyd, xd = _cuda(gy), _cuda(x)
    a, _ = _run(ops, "deterministic", gyd, xd)
    b, _ = _run(ops, "deterministic", gyd, xd)
    assert np.array_equal(a.view(np.int32), b.view(np.int32))
    want = _ordered_partials(gy, x, Co, K)
    assert np.array_equal(a, want), _first_diff(a, want)


def test_deterministic_route_refuses_a_short_workspace(ops):
    from dvm import _lib
    lib = _lib.load()
    R, Co, K = 1000, 65, 129
    gy, x = (_cuda(t) for t in WR.float_family("randn", R, Co, K))
    nb = lib.dvm_linear_wgrad_workspace_bytes(R, Co, K)
    ws = torch.zeros(nb, dtype=torch.uint8, device="cuda")
    dW = _cuda(_pattern(Co * K).reshape(Co, K))
    stream = torch.cuda.current_stream().cuda_stream
    with _deterministic(ops, True):
        rc = lib.dvm_linear_wgrad_ws_f32(gy.data_ptr(), x.data_ptr(), R, Co, K, dW.data_ptr(), ws.data_ptr(), nb - 1, stream)
        msg = lib.dvm_last_error().decode()
        torch.cuda.synchronize()
        assert rc == -3 and "too small" in msg and "dvm_linear_wgrad_ws_f32" in msg, (rc, msg)     # DVM_ENOSPACE
        assert np.array_equal(dW.cpu().numpy().ravel(), _pattern(Co * K)) and not ws.any()
        assert lib.dvm_linear_wgrad_ws_f32(gy.data_ptr(), x.data_ptr(), R, Co, K, dW.data_ptr(), ws.data_ptr(), nb, stream) == 0
        torch.cuda.synchronize()
    assert not np.array_equal(dW.cpu().numpy().ravel(), _pattern(Co * K))


# ------------------------------------------------------------------------------------------------------------------ decoder backward
@pytest.mark.parametrize("R", [33, 1000])
@pytest.mark.parametrize("Co,K", [(512, 262), (256, 512), (128, 256), (9, 128)])
def test_decoder_dx_product_bit_exact(ops, Co, K, R):
    """dX = dy W of a decoder layer y = x W^T: the forward GEMM with W as the channel-major operand (reduction length Co = 9 .. 512,
    output rows of K = 262 floats) against the oracle's chain."""
    g = torch.Generator().manual_seed(Co + K + R)
    W = torch.randn(Co, K, generator=g) / Co ** 0.5
    dy = torch.randn(R, Co, generator=g)
    got = ops.linear(W.reshape(1, Co, K).cuda(), dy.cuda(), channel_major=True)
    assert tuple(got.shape) == (1, R, K)
    ref = O.linear(dy.numpy(), W.t().contiguous().numpy())
    got = got[0].cpu().numpy()
    assert np.array_equal(got, ref), _first_diff(got, ref)


ELU_T = [0.0, -0.0, 1e-8, -1e-8, -1e-4, -1e-2, -1.0, -17.0, -88.0, -104.0, -1e4, 1e-4, 1e-2, 1.0, 17.0, 88.0, 104.0, 1e3, 1e4]


@pytest.mark.parametrize("C", [64, 70], ids=["vector_epilogue", "scalar_epilogue"])
def test_elu_epilogue(ops, C):
    """dvm_linear_f32 with slope < 0 (the training decoder's forward): y = t for t > 0, else exp(t) - 1 as dvm_deformer.hip::elu1
    documents.  The pre-activation t takes prescribed values (identity weights: the chain of one non-zero product is exact) and, in a
    second block, those of a randn product; slope = 1 returns t itself.  Bar for t <= 0: 3 x the largest absolute error of the
    float32 numpy exp(t) - 1 on the same values against expm1 in float64."""
    g = np.random.default_rng(C)
    M = 96
    vals = np.concatenate([ELU_T, -np.geomspace(1e-8, 1e4, 400), np.geomspace(1e-8, 1e4, 200), -g.random(400) * 20, g.standard_normal(400)])
    x_id = np.resize(vals, (M, C)).astype(np.float32)
    assert set(np.float32(ELU_T)) <= set(x_id.ravel())
    blocks = [("prescribed", x_id, np.eye(C, dtype=np.float32)),
              ("randn", (3 * g.standard_normal((M, C))).astype(np.float32), (g.standard_normal((C, C)) / C ** 0.5).astype(np.float32))]
    for name, x, w in blocks:
        xd, wd = _cuda(x), _cuda(w)
        t = ops.linear(xd, wd, slope=1.0).cpu().numpy()
        y = ops.linear(xd, wd, slope=-1.0).cpu().numpy()
        assert np.array_equal(t, O.linear(x, w))
        if name == "prescribed":
            assert np.array_equal(t, x)
        assert np.isfinite(y).all() and (y >= -1.0).all()
        pos = t > 0
        assert pos.any() and (~pos).any() and np.array_equal(y[pos].view(np.int32), t[pos].view(np.int32))
        tn = t[~pos]
        exact = np.expm1(tn.astype(np.float64))
        yard = float(np.abs((np.exp(tn) - np.float32(1)).astype(np.float64) - exact).max())
        err = float(np.abs(y[~pos].astype(np.float64) - exact).max())
        print("RATIO elu %s C=%d: kernel %.3e, float32 numpy exp(t) - 1 %.3e" % (name, C, err, yard))
        assert (np.exp(tn) - np.float32(1)).dtype == np.float32 and yard > 0
        assert err <= 3 * yard, (name, err, yard, float(tn[np.abs(y[~pos].astype(np.float64) - exact).argmax()]))


# ------------------------------------------------------------------------------------------------------------------ batched route
# launch_wgrad_batched (blockIdx.z; R = anchors, Co = N, K = 128) and launch_linear_bmm are reachable only through the criterion node's
# dist term: back-propagate column 6 of the node's terms alone, so the feature gradient it returns is the dist term's.
DIST_C = 128


def _dist_inputs(B, N, nA, kd, seed):
    g = torch.Generator().manual_seed(seed)
    v = torch.rand(2 * B, N, 3, generator=g) - 0.5
    feat = 0.3 * torch.relu(torch.randn(2 * B, N, DIST_C, generator=g))
    starts = torch.randint(0, N, (2 * B,), generator=g).int()
    a1 = torch.tensor(random.Random(seed).sample(range(N), nA), dtype=torch.int32)
    a2 = torch.tensor(random.Random(seed + 1).sample(range(N), nA), dtype=torch.int32)
    return v, feat, starts, a1, a2


def _near_ties(feat, anchors, kd):
    """float64 only.  -> (neighbour lists (S,nA,kd), [(shape, anchor number, rows it touches)] for the anchors whose kd-th and
    (kd+1)-th scores are closer than fp32 can tell).  A score -|a|^2 + 2 a.b - |b|^2 formed in fp32 errs by at most
    (C + 2) u (|a|^2 + 2 sum|a_i b_i| + |b|^2) in any order of its C-term sums (u = 2^-24); two candidates whose float64 scores differ
    by less than the sum of their two error bounds may swap places."""
    from oracle import torch_ref as TR
    f = feat.double()
    S, N, C = f.shape
    fa = f[:, anchors.long()]
    sc = TR.knn_scores(fa, f)                                              # (S,nA,N)
    idx = sc.topk(kd, dim=-1)[1]
    n2 = (f * f).sum(-1)
    eb = (C + 2) * WR.U * (n2[:, anchors.long(), None] + 2 * torch.matmul(fa.abs(), f.abs().transpose(1, 2)) + n2[:, None, :])
    out = []
    if kd < N:
        srt, order = sc.sort(dim=-1, descending=True)
        ebs = torch.gather(eb, 2, order)
        tie = (srt[..., kd - 1] - srt[..., kd]) <= ebs[..., kd - 1] + ebs[..., kd]
        for s, n in tie.nonzero().tolist():
            close = ((sc[s, n] - srt[s, n, kd - 1]).abs() <= 2 * eb[s, n]).nonzero().flatten().tolist()
            out.append((s, n, sorted(set(close) | set(idx[s, n].tolist()) | {int(anchors[n])})))
    return idx, out


def _dist_reference(dtype, feat, d1, d2, a1, a2, kd):
    from oracle import torch_ref as TR
    B = feat.shape[0] // 2
    f = feat.detach().clone().to(dtype).requires_grad_(True)
    t = torch.cat([TR.dist_loss_term(f[:B], d1.to(dtype), a1.long(), kd), TR.dist_loss_term(f[B:], d2.to(dtype), a2.long(), kd)])
    t.sum().backward()
    return t.detach(), f.grad


def _seeded_dist_case(B, N, nA, kd):
    """the first seed whose float64 reference leaves at most 2 % of the anchors on a near-tie"""
    cap = (2 * B * nA) // 50
    for seed in range(1000 * N + 100 * B + nA + kd, 1000 * N + 100 * B + nA + kd + 40):
        v, feat, starts, a1, a2 = _dist_inputs(B, N, nA, kd, seed)
        i1, t1 = _near_ties(feat[:B], a1, kd)
        i2, t2 = _near_ties(feat[B:], a2, kd)
        if len(t1) + len(t2) <= cap:
            return v, feat, starts, a1, a2, torch.cat([i1, i2]), t1 + [(s + B, n, rows) for s, n, rows in t2]
    raise AssertionError("no seed within the near-tie cap")


def _criterion_dist_grad(ops, v, feat, starts, a1, a2, kd):
    from dvm import nn_ops
    from dvm.ops import DEFORMER_KEYS
    import models.model as mm
    B = v.shape[0] // 2
    vd = v.cuda()
    fd = feat.cuda().requires_grad_(True)
    torch.manual_seed(5)
    named = dict(mm.Deformer(10).cuda().train().named_parameters())
    params = [named[k].detach() for k in DEFORMER_KEYS]
    graph = ops.dg_build(vd, starts.cuda())
    gj = {k: graph[k] for k in ("nodes_idx", "one_ring", "infl_idx", "weights")}
    knn = ops.knn_cdist(vd, vd, 10)
    d1, d2 = torch.cdist(vd[:B], vd[:B]).contiguous(), torch.cdist(vd[B:], vd[B:]).contiguous()
    terms = nn_ops.criterion_train((vd, gj, knn, 80.0, 10, True, (d1, d2, a1.cuda(), a2.cuda(), kd)), fd, params)
    terms[:, 6].sum().backward()
    return terms.detach().cpu(), fd.grad.cpu(), d1.cpu(), d2.cpu()


@pytest.mark.parametrize("kd", [5, 40])
@pytest.mark.parametrize("nA", [1, 33, 37])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("N", [64, 516, 132])
def test_batched_route_through_the_dist_term_row_by_row(ops, N, B, nA, kd):
    """Reference: float64 autograd of oracle/torch_ref.py::dist_loss_term.  Rows no anchor touches are exactly 0; every other row is
    within 3 x the largest per-row error of the same formulation in float32 (ATen, CPU), each row's error taken relative to that row's
    float64 max-abs.  N = 132: the node accepts only multiples of 4 (see the refusal test), so the product's Co = N is never off the
    16-byte grid; 132 is the accepted size nearest to 130 and leaves a ragged 4-wide tile edge.

    The bar of a case is 3 x the LARGEST per-row figure of the float32 formulation in that case (2.4e-06 .. 2.3e-04 over the 36 cases).
    This test found the node's weights W = g (y_j / (|x||y|) - cos x_j / |x|^2) / x_j, formed in float32, outside the bar in three cases
    (up to 4.8 x): the expression cancels where cos(x, y) is near 1.  dist_loss_bwd_weights_kernel now forms x_j and W in float64 and
    rounds W once; the node measures 0.9e-07 .. 3.2e-07 in every case (profiles/notes_wgrad_elements.md)."""
    v, feat, starts, a1, a2, idx, ties = _seeded_dist_case(B, N, nA, kd)
    assert len(ties) * 50 <= 2 * B * nA
    terms, got, d1, d2 = _criterion_dist_grad(ops, v, feat, starts, a1, a2, kd)
    t64, g64 = _dist_reference(torch.float64, feat, d1, d2, a1, a2, kd)
    t32, g32 = _dist_reference(torch.float32, feat, d1, d2, a1, a2, kd)
    S = 2 * B
    touched = torch.zeros(S, N, dtype=torch.bool)
    skip = torch.zeros(S, N, dtype=torch.bool)
    for s in range(S):
        touched[s, idx[s].reshape(-1)] = True
        touched[s, (a1 if s < B else a2).long()] = True
    for s, n, rows in ties:
        skip[s, rows] = True
    assert torch.isfinite(got).all()
    untouched = ~touched & ~skip
    assert (g64[untouched] == 0).all()
    bad = (got[untouched] != 0).any(-1).nonzero().flatten()
    assert bad.numel() == 0, "rows no anchor touches carry a gradient: (shape, row) %s" % untouched.nonzero()[bad[:4]].tolist()
    judged = touched & ~skip
    scale = g64.abs().amax(-1)
    assert (scale[judged] > 0).all()
    rel = lambda a: ((a.double() - g64).abs().amax(-1) / scale.clamp_min(1e-300))[judged]      # noqa: E731
    yard, err = float(rel(g32).max()), rel(got)
    print("RATIO dist N=%d B=%d nA=%d kd=%d: node %.3e, float32 formulation %.3e, rows judged %d, exactly zero %d, anchors left out %d"
          % (N, B, nA, kd, float(err.max()), yard, int(judged.sum()), int(untouched.sum()), len(ties)))
    assert yard > 0
    worst = int(err.argmax())
    assert float(err.max()) <= 3 * yard, ("(shape, row)", judged.nonzero()[worst].tolist(), float(err.max()), yard)


@pytest.mark.parametrize("kd", [5, 40])
@pytest.mark.parametrize("nA", [1, 33, 37])
@pytest.mark.parametrize("B,N", [(1, 64), (3, 516), (3, 132)])
def test_batched_products_per_element_from_the_librarys_own_weights(ops, N, B, nA, kd):
    """The two products alone, per element, with the weights taken as given.  W as the library forms
    it (ops.dist_loss_bwd_weights on the neighbour lists of ops.dist_loss: the kernels the node runs) goes through the node's formula in
    float64, d feat = diag(colsum W) feat - W^T fa and d feat[a_n] += rowsum(W)_n fa_n - (W feat)_n, and every ELEMENT of the node's
    gradient must lie within (nA + kd + 5) 2^-24 M of it, M the same formula on magnitudes: a row sees at most nA - 1 adds in its column
    sum, nA fma steps in W^T fa (launch_wgrad_batched: R = nA, Co = N, K = 128), a product and a subtraction; an anchor's row kd - 1 adds in
    its row sum, kd non-zero fma steps in W feat (launch_linear_bmm; a zero weight adds nothing), a product, a subtraction and the add
    into the row.  Derived; where M is 0 the gradient must be exactly 0."""
    v, feat, starts, a1, a2 = _dist_inputs(B, N, nA, kd, 7 * N + B + nA + kd)
    terms, got, d1, d2 = _criterion_dist_grad(ops, v, feat, starts, a1, a2, kd)
    ones = torch.ones(B, device="cuda")
    for side, (dm, an) in enumerate(((d1, a1), (d2, a2))):
        f = feat[side * B:(side + 1) * B].cuda()
        val, idx = ops.dist_loss(f, dm.cuda(), an.cuda(), kd, want_idx=True)
        assert torch.equal(val.cpu(), terms[side * B:(side + 1) * B, 6])
        W = ops.dist_loss_bwd_weights(f, dm.cuda(), an.cuda(), idx, ones).cpu().double()          # (B,nA,N)
        assert int((W != 0).sum(-1).max()) <= kd and torch.isfinite(W).all()
        f = f.cpu().double()
        fa = f[:, an.long()]                                                                      # (B,nA,C)
        want = W.sum(1).unsqueeze(-1) * f - W.transpose(1, 2) @ fa
        mag = W.abs().sum(1).unsqueeze(-1) * f.abs() + W.abs().transpose(1, 2) @ fa.abs()
        want[:, an.long()] += W.sum(2).unsqueeze(-1) * fa - W @ f
        mag[:, an.long()] += W.abs().sum(2).unsqueeze(-1) * fa.abs() + W.abs() @ f.abs()
        bound = (nA + kd + 5) * WR.U * mag
        err = (got[side * B:(side + 1) * B].double() - want).abs()
        ratio = float((err / bound.clamp_min(1e-300))[bound > 0].max())
        print("RATIO dist products N=%d B=%d nA=%d kd=%d side %d: worst err / bound %.4f" % (N, B, nA, kd, side, ratio))
        assert (got[side * B:(side + 1) * B][bound == 0] == 0).all()
        bad = (err > bound).nonzero()
        assert bad.numel() == 0, "%d elements outside the bound, first (shape, row, channel) %s: err %.3e, bound %.3e" % (
            len(bad), bad[0].tolist(), float(err[tuple(bad[0])]), float(bound[tuple(bad[0])]))


def test_criterion_node_refuses_point_counts_off_the_16_byte_grid(ops):
    """N = 130 would give the batched product Co = 130 (scalar loads); the node refuses it loudly, so that path of the kernel is
    reachable through dvm_linear_wgrad_f32 only (covered above at Co = 130, 65, 9, 7)."""
    from dvm._lib import DvmError
    v, feat, starts, a1, a2 = _dist_inputs(1, 130, 33, 5, 1)
    with pytest.raises(DvmError, match="multiple of 4"):
        _criterion_dist_grad(ops, v, feat, starts, a1, a2, 5)
