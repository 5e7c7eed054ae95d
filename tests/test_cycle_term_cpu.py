"""CPU-side checks of the cycle term (models.loss.cycle_term, dvm_cycle_term_f32): the torch fallback that CPU tensors take against
the dense float64 definition, its gradients at an exact inverse (0, not NaN), and the C entries' argument handling, which happens
before anything touches a device (the pointers handed in are never dereferenced)."""
import ctypes

import pytest
import torch

import cycle_term_ref as C
import frob_term_common as T

ONE = ctypes.c_void_p(16)   # a pointer that must never be dereferenced
K = 10


def _planting(name, N, M):
    gen = torch.Generator().manual_seed(4321)
    if name == "random":
        return C.plant_pair("random", "random", gen, 1, N, M, K, K)
    if name == "hubs":
        return C.plant_pair("hubs", "hubs", gen, 1, N, M, K, K)
    if name == "near_inverse":
        return C.plant_near_inverse(1, N, M, K)
    return C.plant_exact_inverse(1, N, M, K)


@pytest.mark.parametrize("name,N,M", [("random", 160, 160), ("hubs", 160, 160), ("near_inverse", 160, 160), ("exact_inverse", 160, 160),
                                      ("random", 170, 300)])
def test_cpu_fallback_matches_dense_float64(name, N, M):
    """The float64 definition, rounded once to fp32: within 2 u F; both gradients within their bars; 0 and finite at F = 0."""
    import models.loss as ml
    val12, idx12, val21, idx21 = _planting(name, N, M)
    ref = C.dense_reference(val12, idx12, val21, idx21)
    v12, v21 = val12.clone().requires_grad_(True), val21.clone().requires_grad_(True)
    loss = ml.cycle_term(v12, idx12, v21, idx21)
    assert loss.dtype == torch.float32 and tuple(loss.shape) == (1,)
    T.check_fallback("%s %s" % (name, (N, M)), loss, ref)
    loss.sum().backward()
    for side, v in (("12", v12), ("21", v21)):
        T.check_fallback_grad(v.grad, ref["g" + side], C.grad_bound(ref, K, side))
    if name == "exact_inverse":
        assert bool((loss == 0).all()) and bool((v12.grad == 0).all()) and bool((v21.grad == 0).all())
    elif name == "near_inverse":
        assert abs(float(ref["F"]) - 0.02598) < 1e-5   # the diagonal residual, 2e-3 per row, dominates
    else:
        assert float(ref["F"]) > 1.0 and float(ref["g12"].abs().max()) > 0 and float(ref["g21"].abs().max()) > 0


def test_entries_exported_sized_and_limited():
    lib, nmax = T.check_entries_exported("cycle")
    assert nmax >= 8192
    B, N, M, k12, k21 = 2, 300, 170, 10, 10
    # the reversed lists of idx12, one double per row, one float per element, the k12 x k21 samples of every row
    need = 4 * B * (2 * M + 1 + N * k12) + 8 * B * N + 4 * B + 4 * B * N * k12 * k21
    got = lib.dvm_cycle_term_workspace_bytes(B, N, M, k12, k21)
    assert need <= got <= need + 6 * 256   # six arrays, each rounded up to 256 bytes: nothing of size N x N, M x M or N x M
    assert got <= 8 * B * N * k12 * k21 + 64 * B * (N + M) * max(k12, k21)
    assert lib.dvm_cycle_term_workspace_bytes(1, nmax, 1 << 20, 16, 16) > 0   # any M
    for bad in ((0, N, M, k12, k21), (65536, N, M, k12, k21), (B, 0, M, k12, k21), (B, N, 0, k12, k21), (B, N, M, 0, k21), (B, N, M, 17, k21),
                (B, N, M, k12, 0), (B, N, M, k12, 17), (B, nmax + 1, M, k12, k21)):
        assert lib.dvm_cycle_term_workspace_bytes(*bad) == 0, bad


def test_argument_validation_without_gpu():
    from dvm import _lib
    lib = _lib.load()
    err = lib.dvm_last_error
    nmax = lib.dvm_cycle_term_max_n()

    def call(val12=ONE, idx12=ONE, val21=ONE, idx21=ONE, B=1, N=8, M=8, k12=4, k21=4, loss=ONE, g12=None, g21=None, ws=None, nb=0):
        return lib.dvm_cycle_term_f32(val12, idx12, val21, idx21, B, N, M, k12, k21, loss, g12, g21, ws, nb, None)

    assert call(val12=None) == -1 and b"null pointer" in err()
    assert call(idx12=None) == -1 and call(val21=None) == -1 and call(idx21=None) == -1 and call(loss=None) == -1
    assert call(B=0) == -1 and call(N=0) == -1 and call(M=0) == -1 and b"empty" in err()
    assert call(k12=0) == -1 and call(k12=17) == -1 and b"k12" in err()
    assert call(k21=0) == -1 and call(k21=17) == -1 and b"k21" in err()
    big = 1 << 40
    assert call(N=nmax + 1, M=64, k12=1, k21=1, ws=ONE, nb=big) == -1 and b"N=%d" % (nmax + 1) in err()   # over the limit: before any launch
    assert call(g12=ONE, ws=ONE, nb=big) == -1 and b"both" in err()   # exactly one gradient
    assert call(g21=ONE, ws=ONE, nb=big) == -1 and b"both" in err()
    assert call() == -3 and b"workspace" in err()   # no workspace
    assert call(ws=ONE, nb=lib.dvm_cycle_term_workspace_bytes(1, 8, 8, 4, 4) - 1, g12=ONE, g21=ONE) == -3 and b"workspace" in err()


def test_wrappers_have_no_cpu_path():
    T.check_no_cpu_path("cycle", C.plant_near_inverse(1, 8, 8, 3))


def test_wrapper_shape_checks(monkeypatch):
    """ops.cycle_term reads N and M from the shapes and refuses a batch mismatch or an idx that is not its val's shape, before the
    library is called (the device check and the call are replaced here: the shape logic needs no GPU)."""
    from dvm import ops
    val12, idx12, val21, idx21 = C.plant_near_inverse(2, 8, 6, 3)
    calls = []
    monkeypatch.setattr(ops, "_need_gpu", lambda *ts: None)
    monkeypatch.setattr(ops, "_call_ws", lambda *a, **kw: calls.append(a))
    with pytest.raises(ValueError):
        ops.cycle_term(val12, idx12, val21[:1], idx21[:1])
    with pytest.raises(ValueError):
        ops.cycle_term(val12, idx12[:, :, :2], val21, idx21)
    with pytest.raises(ValueError):
        ops.cycle_term(val12, idx12, val21, idx21[:, :5])
    assert not calls
    ops.cycle_term(val12, idx12, val21, idx21)
    assert calls and calls[0][0] == "dvm_cycle_term_f32" and calls[0][1][4:9] == (2, 8, 6, 3, 3)


def test_criterion_switch_defaults_off():
    """w_cycle is an attribute, not a constructor argument (the constructor keeps the reference's signature), and starts at 0."""
    import inspect

    import models.loss as ml
    for cls in (ml.GraphDeformLoss_Neural, ml.GraphDeformLoss_Neural_Partial):
        crit = cls()
        assert crit.w_cycle == 0 and crit.cycle_loss == 0
        assert "w_cycle" not in inspect.signature(cls.__init__).parameters


def test_train_driver_knows_w_cycle(capsys):
    import train_driver
    with pytest.raises(SystemExit) as e:
        train_driver.main(["--help"])
    assert e.value.code == 0
    assert "--w-cycle" in capsys.readouterr().out
