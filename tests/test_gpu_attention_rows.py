"""-m gpu: the two attention cores of LG-Net row by row on every launch route: the SA core's training forward
(dvm_sa_attention_train_fwd_f32: xr, stats, cinv) and backward (dvm_sa_attention_bwd_f32: dv, dp), and the N2P core's two forwards
(ops.n2p_core_fwd: out, attn; ops.n2p_attention_pm: out).  References, input families, shapes and bars are those of
tests/attention_ref.py (its docstring derives the bars and holds the measured err / bar); tests/test_attention_rows_cpu.py runs the
same drivers on an fp32 restatement of the kernels and on planted mutations of it.  The float64 references run on the card in torch,
the reference's own fp32 formulation (err32) on the CPU.

Exact plantings (bit for bit): SA with p = 0 at N in {1 .. 2048} through the C entries on the test's own NaN-filled outputs and
NaN-filled workspaces (the backward's memsets and the forward's partials are under test); N2P with K = 1, with q = 0, with all
slots equal and with kp offset by +-2^23 (exact differences that sum to 0) at K = 64 and integer vp.
Bars (every row of every output): the SA families randn / relu / peaked / hub10 / hub25 / hub100 / dup_pairs / dup_all / gzero /
voffset / vscale1e3 / vscale1e-3 at the forward's key-chunk routes (Z = 1, 2, 4, 8, Z < S, S = 2 with B > 1), the backward's splits
(1, 2, 4, 8, 8 with an empty last split, 16, 4 at the training shape, 1 in deterministic mode) and the tails N in {1 .. 129} at
B = 3; every backward twice, on the forward's own xr / stats / cinv and on float64-exact ones.  The shapes with N >= 2045 take randn
and hub25 only.  N2P: random / hub / self / same / peaked / wide / tie at C in {64, 128}, K in {1, 3, 40, 64}, (B, N) in {(1,1), (2,5),
(3,1030)}.
"""
import pytest
import torch

import attention_ref as R
from attention_ref import N2P_BN, N2P_CK, SA_BWD_SHAPES, SA_DET_N, SA_FLAT_N, SA_FWD_SHAPES, SA_TAIL_N
from test_gpu_backward_adversarial import n2p_inputs

pytestmark = pytest.mark.gpu
BIG = ["randn", "hub25"]          # the families of the shapes with N >= 2045 (every family runs at N <= 1030)
SA_FWD_CASES = [(BN, f) for BN in SA_FWD_SHAPES for f in (BIG if BN[1] >= 2045 else R.SA_FAMILIES)]
SA_BWD_CASES = [(BN, f) for BN in SA_BWD_SHAPES for f in (BIG if BN[1] >= 2045 else R.SA_FAMILIES)]


@pytest.fixture(scope="module")
def ops():
    from dvm import ops as _ops
    assert torch.cuda.is_available(), "these tests need the MI355X"
    yield _ops
    print("\nlargest err / bar on the GPU\n" + R.report("sa") + "\n" + R.report("n2p"))


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


def _nan_ws(nbytes):
    return torch.full((max(int(nbytes), 256),), 0xFF, dtype=torch.uint8, device="cuda") if nbytes else None   # 0xFFFFFFFF: a NaN


def c_entries(ops):
    """The two C entries on NaN-filled outputs and workspaces of the test's own."""
    from dvm import _lib
    lib, p_ = _lib.load(), ops._p

    def fwd(p, v):
        B, N, _ = p.shape
        xr, st, ci = _nan(B, N, 64), _nan(B, N, 2), _nan(B, N)
        nb = lib.dvm_sa_attention_train_fwd_workspace_bytes(B, N)
        ws = _nan_ws(nb)
        _lib.check(lib.dvm_sa_attention_train_fwd_f32(p_(p), p_(v), B, N, p_(xr), p_(st), p_(ci), p_(ws), nb, ops._stream()),
                   "dvm_sa_attention_train_fwd_f32")
        torch.cuda.synchronize()
        return xr, st, ci

    def bwd(p, v, xr, st, ci, G):
        B, N, _ = p.shape
        dp, dv = _nan(B, N, 16), _nan(B, N, 64)
        nb = lib.dvm_sa_attention_bwd_workspace_bytes(B, N)
        ws = _nan_ws(nb)
        _lib.check(lib.dvm_sa_attention_bwd_f32(p_(p), p_(v), p_(xr), p_(st), p_(ci), p_(G), B, N, p_(dp), p_(dv), p_(ws), nb, ops._stream()),
                   "dvm_sa_attention_bwd_f32")
        torch.cuda.synchronize()
        return dp, dv

    return fwd, bwd


# ------------------------------------------------------------------------------------------------------------- SA
@pytest.mark.parametrize("N", SA_FLAT_N)
def test_sa_flat_exact(ops, N):
    assert not ops.is_deterministic()
    fwd, bwd = c_entries(ops)
    R.sa_flat_case(fwd, bwd, 1, N, device="cuda")


@pytest.mark.parametrize("BN,family", SA_FWD_CASES, ids=str)
def test_sa_forward_chunks(ops, BN, family):
    B, N = BN
    R.sa_run_case(ops.sa_attention_train_fwd, None, family, B, N, seed=N + B, device="cuda", backward=False)


@pytest.mark.parametrize("BN,family", SA_BWD_CASES, ids=str)
def test_sa_backward_splits(ops, BN, family):
    B, N = BN
    assert not ops.is_deterministic()
    R.sa_run_case(ops.sa_attention_train_fwd, ops.sa_attention_bwd, family, B, N, seed=N + B, device="cuda")


@pytest.mark.parametrize("family", BIG)
@pytest.mark.parametrize("N", SA_DET_N)
def test_sa_backward_deterministic(ops, N, family):
    """set_deterministic(True): the inner loop is not split; the bars, and two calls bit for bit."""
    prev = ops.set_deterministic(True)
    try:
        R.sa_run_case(ops.sa_attention_train_fwd, ops.sa_attention_bwd, family, 1, N, seed=N, device="cuda")
        p, v, G = (t.cuda() for t in R.sa_inputs(family, 1, N, seed=N))
        xr, st, ci = ops.sa_attention_train_fwd(p, v)
        dp1, dv1 = ops.sa_attention_bwd(p, v, xr, st, ci, G)
        dp2, dv2 = ops.sa_attention_bwd(p, v, xr, st, ci, G)
        assert torch.equal(dp1, dp2) and torch.equal(dv1, dv2)
    finally:
        ops.set_deterministic(prev)


@pytest.mark.parametrize("family", R.SA_FAMILIES)
@pytest.mark.parametrize("N", SA_TAIL_N)
def test_sa_tails(ops, N, family):
    R.sa_run_case(ops.sa_attention_train_fwd, ops.sa_attention_bwd, family, 3, N, seed=N, device="cuda")


# ------------------------------------------------------------------------------------------------------------- N2P
@pytest.mark.parametrize("family", R.N2P_FAMILIES)
@pytest.mark.parametrize("C,Kn", N2P_CK)
@pytest.mark.parametrize("B,N", N2P_BN)
def test_n2p_forward_families(ops, B, N, C, Kn, family):
    R.n2p_run_case(n2p_inputs, ops.n2p_core_fwd, ops.n2p_attention_pm, family, B, N, C, Kn, seed=B * N + Kn + C, device="cuda")


@pytest.mark.parametrize("C", [64, 128])
@pytest.mark.parametrize("B,N", N2P_BN)
@pytest.mark.parametrize("kind", ["k1", "q0", "same", "offset"])
def test_n2p_forward_exact(ops, kind, B, N, C):
    R.n2p_exact_case(ops.n2p_core_fwd, ops.n2p_attention_pm, kind, B, N, C, seed=N + C, device="cuda")
