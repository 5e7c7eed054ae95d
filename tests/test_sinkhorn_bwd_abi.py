"""CPU-side checks of the differentiable Sinkhorn pair (dvm_sinkhorn_fwd_hist_f32 / dvm_sinkhorn_bwd_f32): exported, sized,
every argument error reported before anything touches a device; the tensor wrappers and the autograd node have no CPU
fallback; the criterion's and the training driver's switch exist and default to off."""
import ctypes

import pytest

NAMES = ("dvm_sinkhorn_hist_workspace_bytes", "dvm_sinkhorn_fwd_hist_f32", "dvm_sinkhorn_bwd_workspace_bytes", "dvm_sinkhorn_bwd_f32")


@pytest.fixture(scope="module")
def lib():
    from dvm import _lib
    return _lib.load()


def test_exported_and_sized(lib):
    from dvm import _lib
    raw = ctypes.CDLL(_lib.SO_PATH)
    for name in NAMES:
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES, name
    assert lib.dvm_sinkhorn_hist_workspace_bytes(2, 100, 50, 128) >= 4 * 2 * (100 + 50)
    assert lib.dvm_sinkhorn_hist_workspace_bytes(0, 100, 50, 128) == 0
    small, large = lib.dvm_sinkhorn_bwd_workspace_bytes(2, 100, 50, 128, 1), lib.dvm_sinkhorn_bwd_workspace_bytes(2, 100, 50, 128, 20)
    # the adjoints of the potentials (T (N + M) floats) and the top-k bit matrix (N ceil(M / 32) words), per entry
    assert small >= 4 * 2 * ((100 + 50) + 100 * 2) and large >= small + 4 * 2 * 19 * (100 + 50)
    assert lib.dvm_sinkhorn_bwd_workspace_bytes(2, 100, 50, 128, 33) == 0   # beyond the documented limit


def _hist(lib, f1, f2, d=128, neg_alpha=-1.0, n_iter=5, topk=10, val=None, idx=None, uh=None, vh=None, variant=0, ws=None, ws_bytes=0):
    return lib.dvm_sinkhorn_fwd_hist_f32(f1, f2, 1, 8, 8, d, neg_alpha, n_iter, topk, val, idx, None, None, uh, vh, variant, ws, ws_bytes, None)


def _bwd(lib, p, d=128, neg_alpha=-1.0, n_iter=5, topk=10, df2="p", variant=0, ws=None, ws_bytes=0, B=1):
    return lib.dvm_sinkhorn_bwd_f32(p, p, B, 8, 8, d, neg_alpha, n_iter, topk, p, p, p, p, p, p, p if df2 == "p" else df2, variant, ws, ws_bytes,
                                    None)


def test_hist_argument_validation_without_gpu(lib):
    one = ctypes.c_void_p(16)
    ok = dict(val=one, idx=one, uh=one, vh=one)
    assert _hist(lib, None, None) == -1 and b"null pointer" in lib.dvm_last_error()
    assert _hist(lib, one, one, val=one, idx=one, uh=one, vh=None) == -1 and b"null pointer" in lib.dvm_last_error()
    assert _hist(lib, one, one, d=130, **ok) == -1 and b"d=130" in lib.dvm_last_error()
    assert _hist(lib, one, one, topk=17, **ok) == -1 and b"topk=17" in lib.dvm_last_error()
    assert _hist(lib, one, one, n_iter=-1, **ok) == -1 and b"n_iter" in lib.dvm_last_error()
    assert _hist(lib, one, one, neg_alpha=0.0, **ok) == -1 and b"neg_alpha" in lib.dvm_last_error()
    assert _hist(lib, one, one, variant=2, **ok) == -1 and b"variant" in lib.dvm_last_error()
    assert _hist(lib, one, one, **ok) == -3 and b"workspace" in lib.dvm_last_error()
    nb = lib.dvm_sinkhorn_hist_workspace_bytes(1, 8, 8, 128)
    assert _hist(lib, one, one, ws=one, ws_bytes=nb - 1, **ok) == -3 and b"workspace" in lib.dvm_last_error()


def test_bwd_argument_validation_without_gpu(lib):
    one = ctypes.c_void_p(16)
    assert lib.dvm_sinkhorn_bwd_f32(None, None, 1, 8, 8, 128, -1.0, 5, 10, None, None, None, None, None, None, None, 0, None, 0, None) == -1
    assert b"null pointer" in lib.dvm_last_error()
    assert _bwd(lib, one, df2=None) == -1 and b"null pointer" in lib.dvm_last_error()
    assert _bwd(lib, one, B=0) == -1 and b"empty" in lib.dvm_last_error()
    assert _bwd(lib, one, d=130) == -1 and b"d=130" in lib.dvm_last_error()
    assert _bwd(lib, one, d=516) == -1 and b"d=516" in lib.dvm_last_error()
    assert _bwd(lib, one, topk=17) == -1 and b"topk=17" in lib.dvm_last_error()
    assert _bwd(lib, one, n_iter=-1) == -1 and b"n_iter" in lib.dvm_last_error()
    assert _bwd(lib, one, n_iter=33) == -1 and b"n_iter" in lib.dvm_last_error()   # the documented limit is 32
    assert _bwd(lib, one, neg_alpha=0.0) == -1 and b"neg_alpha" in lib.dvm_last_error()
    assert _bwd(lib, one, variant=2) == -1 and b"variant" in lib.dvm_last_error()
    assert _bwd(lib, one) == -3 and b"workspace" in lib.dvm_last_error()
    nb = lib.dvm_sinkhorn_bwd_workspace_bytes(1, 8, 8, 128, 5)
    assert _bwd(lib, one, ws=one, ws_bytes=nb - 1 - 256 * 6) == -3 and b"workspace" in lib.dvm_last_error()   # (the query sizes for topk = 16)
    assert _bwd(lib, one, ws=one, ws_bytes=lib.dvm_sinkhorn_bwd_workspace_bytes(1, 8, 8, 128, 0)) == -3


def test_no_cpu_fallback():
    import torch
    from dvm import nn_ops, ops
    from dvm._lib import DvmError
    f = torch.randn(1, 8, 128)
    with pytest.raises(DvmError):
        ops.sinkhorn_hist(f, f, 10.0, 5)
    z = torch.zeros(1, 8, 10)
    with pytest.raises(DvmError):
        ops.sinkhorn_bwd(f, f, 10.0, 5, z, z.int(), torch.zeros(1, 6, 8), torch.zeros(1, 6, 8), z)
    g = torch.randn(1, 8, 128, requires_grad=True)
    with pytest.raises(DvmError):
        nn_ops.sinkhorn_topk(g, f, 10.0, 5)
    with pytest.raises(DvmError):
        nn_ops.sinkhorn_topk(f, f, 10.0, 5)


def test_sinkhorn_pi_under_grad_reaches_the_differentiable_node():
    """models.loss.sinkhorn_pi no longer stops at ops.sinkhorn's 'forward only' refusal when a feature requires grad: it goes to
    the autograd node, whose device check answers on a CPU tensor."""
    import torch
    import models.loss as ml
    from dvm._lib import DvmError
    g = torch.randn(1, 8, 128, requires_grad=True)
    with pytest.raises(DvmError, match="HIP device"):
        ml.sinkhorn_pi(g, torch.randn(1, 8, 128))


def test_criterion_switch_defaults_off():
    import models.loss as ml
    assert ml.GraphDeformLoss_Neural().sinkhorn_iters == 0
    assert ml.GraphDeformLoss_Neural_Partial().sinkhorn_iters == 0


def test_train_driver_knows_sinkhorn(capsys):
    import train_driver
    with pytest.raises(SystemExit) as e:
        train_driver.main(["--help"])
    assert e.value.code == 0
    assert "--sinkhorn" in capsys.readouterr().out
