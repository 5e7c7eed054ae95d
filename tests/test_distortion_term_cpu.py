"""CPU-side checks of the distortion term (models.loss.distortion_term, dvm_distortion_term_f32): the torch fallback that CPU
tensors take against the dense float64 definition, its gradient at an exact isometry (0, not NaN), and the C entries' argument
handling, which happens before anything touches a device (the pointers handed in are never dereferenced)."""
import ctypes

import pytest
import torch

import distortion_term_ref as D
import frob_term_common as T

ONE = ctypes.c_void_p(16)   # a pointer that must never be dereferenced
K = 10


def _planting(name, N, M):
    gen = torch.Generator().manual_seed(8765)
    if name in ("random", "hubs"):
        return D.plant(name, gen, 1, N, M, K)
    if name == "near_isometry":
        return D.plant_near_isometry(gen, 1, N, K)
    return D.plant_exact_isometry(gen, 1, N, K)


@pytest.mark.parametrize("name,N,M", [("random", 160, 160), ("hubs", 160, 160), ("near_isometry", 160, 160), ("exact_isometry", 160, 160),
                                      ("random", 170, 300), ("random", 300, 170)])
def test_cpu_fallback_matches_dense_float64(name, N, M):
    """The float64 definition, rounded once to fp32: within 2 u F; the gradient within its bar; 0 and finite at F = 0."""
    import models.loss as ml
    val, idx, D1, D2 = _planting(name, N, M)
    ref = D.dense_reference(val, idx, D1, D2)
    v = val.clone().requires_grad_(True)
    loss = ml.distortion_term(v, idx, D1, D2, symmetric=True)
    assert loss.dtype == torch.float32 and tuple(loss.shape) == (1,)
    T.check_fallback("%s %s" % (name, (N, M)), loss, ref)
    loss.sum().backward()
    T.check_fallback_grad(v.grad, ref["g"], D.grad_bound(ref, K))
    if name == "exact_isometry":
        assert bool((loss == 0).all()) and bool((v.grad == 0).all())
    elif name == "near_isometry":
        assert 0 < float(ref["F"]) < 1e-2 * float(ref["S_fro"])
    else:
        assert float(ref["F"]) > 1.0 and float(ref["g"].abs().max()) > 0
    # symmetric=False on matrices that already are symmetric: (D + D^T) / 2 is D, bit for bit
    with torch.no_grad():
        assert torch.equal(ml.distortion_term(val, idx, D1, D2), loss.detach())


def test_closed_form_gradient_matches_autograd():
    """The formula the kernel implements, (2/F) D2 P^T R[i,:] gathered at idx[i,t], against float64 autograd of the definition."""
    val, idx, D1, D2 = _planting("random", 170, 300)
    ref = D.dense_reference(val, idx, D1, D2)
    v, ix, d1, d2 = val.double(), idx.long(), D1.double(), D2.double()
    P = torch.zeros(1, 170, 300, dtype=torch.float64).scatter_add(-1, ix, v)
    Rm = P @ d2 @ P.transpose(1, 2) - d1
    g = (2.0 / ref["F"][:, None, None]) * ((Rm @ P) @ d2.transpose(1, 2)).gather(-1, ix)
    assert float((g - ref["g"]).abs().max()) <= 1e-10 * float(ref["g"].abs().max())


def test_fallback_symmetrises():
    """symmetric=False evaluates the term on (D + D^T) / 2 of both matrices."""
    import models.loss as ml
    val, idx, D1, D2 = _planting("random", 70, 90)
    gen = torch.Generator().manual_seed(5)
    A1, A2 = D1 + 0.1 * torch.rand(D1.shape, generator=gen), D2 + 0.1 * torch.rand(D2.shape, generator=gen)
    assert not torch.equal(A2, A2.transpose(1, 2))
    ref = D.dense_reference(val, idx, 0.5 * (A1 + A1.transpose(1, 2)), 0.5 * (A2 + A2.transpose(1, 2)), grad=False)
    err = (ml.distortion_term(val, idx, A1, A2).double() - ref["F"]).abs()
    assert bool((err <= 2 * D.U * ref["F"]).all())
    off = (ml.distortion_term(val, idx, A1, A2, symmetric=True).double() - ref["F"]).abs()
    assert bool((off > 2 * D.U * ref["F"]).all())   # the promise is not checked: the asymmetric matrices give another number


def test_entries_exported_sized_and_limited():
    lib, nmax = T.check_entries_exported("distortion")
    assert nmax == 8192
    B, N, M, k = 2, 300, 170, 10
    got = lib.dvm_distortion_term_workspace_bytes(B, N, M, k)
    assert 0 < got <= 64 * B * (N + M) * k   # nothing of size N x N, M x M or N x M
    assert lib.dvm_distortion_term_workspace_bytes(65535, nmax, nmax, 16) > 0
    for bad in ((0, N, M, k), (65536, N, M, k), (B, 0, M, k), (B, N, 0, k), (B, N, M, 0), (B, N, M, 17), (B, nmax + 1, M, k),
                (B, N, nmax + 1, k), (-1, N, M, k), (B, -1, M, k)):
        assert lib.dvm_distortion_term_workspace_bytes(*bad) == 0, bad
    # monotone inside the limits, in every argument
    q = lib.dvm_distortion_term_workspace_bytes
    for lo, hi in (((1, N, M, k), (2, N, M, k)), ((B, N, M, k), (B, N + 1, M, k)), ((B, N, M, k), (B, N, M + 1, k)),
                   ((B, N, M, k), (B, N, M, k + 1)), ((B, N, M, k), (B, nmax, nmax, 16)), ((1, 1, 1, 1), (B, N, M, k))):
        assert 0 < q(*lo) <= q(*hi), (lo, hi)


def test_argument_validation_without_gpu():
    from dvm import _lib
    lib = _lib.load()
    err = lib.dvm_last_error
    nmax = lib.dvm_distortion_term_max_n()

    def call(val=ONE, idx=ONE, d1=ONE, d2=ONE, B=1, N=8, M=8, k=4, loss=ONE, g=None, ws=None, nb=0):
        return lib.dvm_distortion_term_f32(val, idx, d1, d2, B, N, M, k, loss, g, ws, nb, None)

    assert call(val=None) == -1 and b"null pointer" in err()
    assert call(idx=None) == -1 and call(d1=None) == -1 and call(d2=None) == -1 and call(loss=None) == -1
    assert call(B=0) == -1 and call(N=0) == -1 and call(M=0) == -1 and b"empty" in err()
    assert call(B=65536) == -1 and b"B=65536" in err()
    assert call(k=0) == -1 and call(k=17) == -1 and b"topk" in err()
    big = 1 << 40
    assert call(N=nmax + 1, M=64, k=1, ws=ONE, nb=big) == -1 and b"N=%d" % (nmax + 1) in err()   # over a limit: before any launch
    assert call(N=64, M=nmax + 1, k=1, ws=ONE, nb=big) == -1 and b"M=%d" % (nmax + 1) in err()
    assert call() == -3 and b"workspace" in err()   # no workspace
    assert call(ws=ONE, nb=lib.dvm_distortion_term_workspace_bytes(1, 8, 8, 4) - 1, g=ONE) == -3 and b"workspace" in err()


def test_wrappers_have_no_cpu_path():
    T.check_no_cpu_path("distortion", D.plant_near_isometry(torch.Generator().manual_seed(1), 1, 8, 3))


def test_wrapper_shape_checks(monkeypatch):
    """ops.distortion_term reads N and M from the shapes and refuses a batch mismatch, an idx that is not val's shape and a
    distance matrix that is not square or not the source's size, before the library is called (the device check and the call are
    replaced here: the shape logic needs no GPU)."""
    from dvm import ops
    gen = torch.Generator().manual_seed(2)
    val, idx, D1, D2 = D.plant("random", gen, 2, 8, 6, 3)
    calls = []
    monkeypatch.setattr(ops, "_need_gpu", lambda *ts: None)
    monkeypatch.setattr(ops, "_call_ws", lambda *a, **kw: calls.append(a))
    for bad in ((val, idx[:, :, :2], D1, D2), (val, idx, D1[:1], D2), (val, idx, D1, D2[:1]), (val, idx, D2, D2),
                (val, idx, D1, D2[:, :5]), (val, idx, D1[0], D2), (val[0], idx[0], D1, D2)):
        with pytest.raises(ValueError):
            ops.distortion_term(*bad)
    assert not calls
    ops.distortion_term(val, idx, D1, D2)
    assert calls and calls[0][0] == "dvm_distortion_term_f32" and calls[0][1][4:8] == (2, 8, 6, 3)
    assert calls[0][4] == "dvm_distortion_term_workspace_bytes" and calls[0][5:] == (2, 8, 6, 3)


def test_criterion_switch_defaults_off():
    """w_distortion is an attribute, not a constructor argument (the constructor keeps the reference's signature), and starts at 0."""
    import inspect

    import models.loss as ml
    for cls in (ml.GraphDeformLoss_Neural, ml.GraphDeformLoss_Neural_Partial):
        crit = cls()
        assert crit.w_distortion == 0 and crit.distortion_loss == 0
        assert "w_distortion" not in inspect.signature(cls.__init__).parameters


def test_train_driver_knows_w_distortion(capsys):
    import train_driver
    with pytest.raises(SystemExit) as e:
        train_driver.main(["--help"])
    assert e.value.code == 0
    assert "--w-distortion" in capsys.readouterr().out
