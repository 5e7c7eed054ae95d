"""CPU-side checks of the Sinkhorn entry (dvm_sinkhorn_fwd_f32): exported, sized, and every argument error reported
before anything touches a device; the tensor wrapper has no CPU fallback and refuses inputs that require grad."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def lib():
    from dvm import _lib
    return _lib.load()


def test_exported_and_sized(lib):
    from dvm import _lib
    raw = ctypes.CDLL(_lib.SO_PATH)
    assert hasattr(raw, "dvm_sinkhorn_workspace_bytes") and hasattr(raw, "dvm_sinkhorn_fwd_f32")
    assert "dvm_sinkhorn_fwd_f32" in _lib.SIGNATURES and "dvm_sinkhorn_workspace_bytes" in _lib.SIGNATURES
    assert lib.dvm_sinkhorn_workspace_bytes(2, 100, 50, 128) >= 4 * 2 * (100 + 50)


def _call(lib, f1, f2, d=128, neg_alpha=-1.0, n_iter=5, topk=10, val=None, idx=None, ws=None, ws_bytes=0):
    return lib.dvm_sinkhorn_fwd_f32(f1, f2, 1, 8, 8, d, neg_alpha, n_iter, topk, val, idx, None, None, None, None, 0, ws, ws_bytes, None)


def test_argument_validation_without_gpu(lib):
    one = ctypes.c_void_p(16)
    assert _call(lib, None, None) == -1 and b"null pointer" in lib.dvm_last_error()
    assert _call(lib, one, one, val=one, idx=None) == -1 and b"null pointer" in lib.dvm_last_error()
    assert _call(lib, one, one, val=one, idx=one, d=130) == -1 and b"d=130" in lib.dvm_last_error()
    assert _call(lib, one, one, val=one, idx=one, topk=17) == -1 and b"topk=17" in lib.dvm_last_error()
    assert _call(lib, one, one, val=one, idx=one, n_iter=-1) == -1 and b"n_iter" in lib.dvm_last_error()
    assert _call(lib, one, one, val=one, idx=one, neg_alpha=0.0) == -1 and b"neg_alpha" in lib.dvm_last_error()
    assert _call(lib, one, one, val=one, idx=one) == -3 and b"workspace" in lib.dvm_last_error()
    nb = lib.dvm_sinkhorn_workspace_bytes(1, 8, 8, 128)
    assert _call(lib, one, one, val=one, idx=one, ws=one, ws_bytes=nb - 1) == -3 and b"workspace" in lib.dvm_last_error()


def test_no_cpu_fallback():
    import torch
    from dvm import ops
    from dvm._lib import DvmError
    f = torch.randn(1, 8, 128)
    with pytest.raises(DvmError):
        ops.sinkhorn(f, f, 10.0, 5)
    with pytest.raises(DvmError):
        ops.sinkhorn(f, f, 10.0, 0, potentials=True)


def test_refuses_inputs_that_require_grad(monkeypatch):
    """Forward only: with grad mode on, a feature tensor that requires grad is refused before any launch (the library is
    not even loaded), instead of returning values that autograd would treat as constants."""
    import torch
    from dvm import _lib, ops
    from dvm._lib import DvmError

    def no_launch():
        raise AssertionError("the library was reached")

    monkeypatch.setattr(_lib, "load", no_launch)
    f = torch.randn(1, 8, 128)
    g = torch.randn(1, 8, 128, requires_grad=True)
    for a, b in ((g, f), (f, g)):
        with pytest.raises(DvmError, match="forward only"):
            ops.sinkhorn(a, b, 10.0, 5)
    with torch.no_grad(), pytest.raises(DvmError, match="HIP device"):   # grad mode off: the usual device check answers
        ops.sinkhorn(g, f, 10.0, 5)


def test_module_layer_exports_sinkhorn_pi():
    import inspect
    import models.loss as ml
    sig = inspect.signature(ml.sinkhorn_pi)
    assert list(sig.parameters) == ["x", "y", "alpha", "n_iter", "topk"]
    assert (sig.parameters["alpha"].default, sig.parameters["n_iter"].default, sig.parameters["topk"].default) == (100, 5, 10)
