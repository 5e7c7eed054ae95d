"""CPU-side checks of the rank term (models.loss.rank_term, dvm_rank_term_f32): the torch fallback that CPU tensors take against
the dense float64 definition, its gradient at an exact permutation (0, not NaN), and the C entries' argument handling, which
happens before anything touches a device (the pointers handed in are never dereferenced)."""
import ctypes

import pytest
import torch

import frob_term_common as T
import rank_term_ref as R

ONE = ctypes.c_void_p(16)   # a pointer that must never be dereferenced
SHAPE = (1, 160, 160, 10)


def _plantings():
    B, N, M, k = SHAPE
    gen = torch.Generator().manual_seed(1234)
    return {"random": R.plant_random(gen, B, N, M, k), "hubs": R.plant_hubs(gen, B, N, M, k),
            "near_perm": R.plant_near_perm(B, N, M, k), "exact_perm": R.plant_exact_perm(B, N, M, k)}


@pytest.mark.parametrize("name", ["random", "hubs", "near_perm", "exact_perm"])
def test_cpu_fallback_matches_dense_float64(name):
    """The float64 three-term formula, rounded once to fp32: within 2 u F of the definition."""
    import models.loss as ml
    val, idx = _plantings()[name]
    M, k = SHAPE[2], SHAPE[3]
    ref = R.dense_reference(val, idx, M)
    v = val.clone().requires_grad_(True)
    loss = ml.rank_term(v, idx, M)
    assert loss.dtype == torch.float32 and tuple(loss.shape) == (SHAPE[0],)
    T.check_fallback(name, loss, ref)
    loss.sum().backward()
    T.check_fallback_grad(v.grad, ref["g"], R.grad_bound(ref, k))


def test_cpu_gradient_at_exact_permutation_is_zero():
    """F = 0: torch.norm's gradient at zero is 0, and so is the fallback's (a bare sqrt gives inf * 0 = NaN there)."""
    import models.loss as ml
    val, idx = _plantings()["exact_perm"]
    v = val.clone().requires_grad_(True)
    loss = ml.rank_term(v, idx, SHAPE[2])
    assert bool((loss == 0).all())
    loss.sum().backward()
    assert bool(torch.isfinite(v.grad).all()) and bool((v.grad == 0).all())


def test_entries_exported_sized_and_limited():
    lib, nmax = T.check_entries_exported("rank")
    assert nmax >= 8192   # the criterion's own gate
    B, N, M, k = 2, 300, 170, 10
    need = 4 * B * (2 * M + 1 + N * k) + 8 * B * N + 4 * B   # the reversed lists, one double per row, one float per element
    got = lib.dvm_rank_term_workspace_bytes(B, N, M, k)
    assert need <= got <= need + 5 * 256   # five arrays, each rounded up to 256 bytes: nothing of size N x N, M x M or N x M
    assert lib.dvm_rank_term_workspace_bytes(1, nmax, 1 << 20, 16) > 0   # any M
    for bad in ((0, N, M, k), (B, 0, M, k), (B, N, 0, k), (B, N, M, 0), (B, N, M, 17), (B, nmax + 1, M, k)):
        assert lib.dvm_rank_term_workspace_bytes(*bad) == 0, bad


def test_argument_validation_without_gpu():
    from dvm import _lib
    lib = _lib.load()
    err = lib.dvm_last_error
    nmax = lib.dvm_rank_term_max_n()

    def call(val=ONE, idx=ONE, B=1, N=8, M=8, k=4, loss=ONE, g=None, ws=None, nb=0):
        return lib.dvm_rank_term_f32(val, idx, B, N, M, k, loss, g, ws, nb, None)

    assert call(val=None) == -1 and b"null pointer" in err()
    assert call(idx=None) == -1 and call(loss=None) == -1
    assert call(B=0) == -1 and call(N=0) == -1 and call(M=0) == -1 and b"empty" in err()
    assert call(k=0) == -1 and call(k=17) == -1 and b"topk" in err()
    assert call(N=nmax + 1, M=64, k=1, ws=ONE, nb=1 << 40) == -1 and b"N=%d" % (nmax + 1) in err()   # over the limit: before any launch
    assert call() == -3 and b"workspace" in err()   # no workspace
    assert call(ws=ONE, nb=lib.dvm_rank_term_workspace_bytes(1, 8, 8, 4) - 1, g=ONE) == -3 and b"workspace" in err()


def test_wrappers_have_no_cpu_path():
    T.check_no_cpu_path("rank", (*R.plant_near_perm(1, 8, 8, 3), 8))
