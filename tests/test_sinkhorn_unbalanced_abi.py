"""CPU-side checks of the unbalanced Sinkhorn entries (dvm_sinkhorn_ub_fwd_f32 / dvm_sinkhorn_ub_fwd_hist_f32 /
dvm_sinkhorn_ub_bwd_f32): exported, sized, every argument error reported before anything touches a device (the pointers handed
in are never dereferenced); the tensor wrappers and the autograd node have no CPU fallback; the criterion's and the drivers'
switches exist and default to off; the stand-alone host program that drives the same rejection paths under AddressSanitizer +
UBSan builds and exits clean."""
import ctypes
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dvm_sinkhorn_ub_workspace_bytes", "dvm_sinkhorn_ub_fwd_f32", "dvm_sinkhorn_ub_hist_workspace_bytes", "dvm_sinkhorn_ub_fwd_hist_f32",
         "dvm_sinkhorn_ub_bwd_workspace_bytes", "dvm_sinkhorn_ub_bwd_f32")
ONE = ctypes.c_void_p(16)   # a pointer that must never be dereferenced


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
    for query in (lib.dvm_sinkhorn_ub_workspace_bytes, lib.dvm_sinkhorn_ub_hist_workspace_bytes):
        assert query(2, 100, 50, 128) >= 4 * 2 * 2 * (100 + 50)   # norms and potentials of both sides
        assert query(0, 100, 50, 128) == 0
    small, large = lib.dvm_sinkhorn_ub_bwd_workspace_bytes(2, 100, 50, 128, 1), lib.dvm_sinkhorn_ub_bwd_workspace_bytes(2, 100, 50, 128, 20)
    # per iterate and entry: the adjoints (N + M), the re-made potentials (N + M) and three planes per side (3 (N + M)), in seven
    # arrays whose sizes are each rounded up to 256 bytes
    assert large >= small + 4 * 2 * 19 * 5 * (100 + 50) - 7 * 256
    assert small > lib.dvm_sinkhorn_bwd_workspace_bytes(2, 100, 50, 128, 1)
    assert lib.dvm_sinkhorn_ub_bwd_workspace_bytes(0, 100, 50, 128, 5) == 0
    assert lib.dvm_sinkhorn_ub_bwd_workspace_bytes(2, 100, 50, 128, 33) == 0   # beyond the documented limit


def _fwd(lib, hist, p=ONE, B=1, d=128, neg_alpha=-1.0, n_iter=5, topk=10, tau=(0.9, 0.9), val="p", last="p", variant=0, ws=None, ws_bytes=0):
    fn = lib.dvm_sinkhorn_ub_fwd_hist_f32 if hist else lib.dvm_sinkhorn_ub_fwd_f32
    # the last pointer: cn_hist (required) of the history form, v (optional) of the plain one
    return fn(p, p, B, 8, 8, d, neg_alpha, n_iter, topk, tau[0], tau[1], None, None, p if val == "p" else val, p, None, None, None, p,
              p if last == "p" else last, variant, ws, ws_bytes, None)


def _bwd(lib, p=ONE, B=1, d=128, neg_alpha=-1.0, n_iter=5, topk=10, tau=(0.9, 0.9), lmass="p", df2="p", variant=0, ws=None, ws_bytes=0):
    return lib.dvm_sinkhorn_ub_bwd_f32(p, p, B, 8, 8, d, neg_alpha, n_iter, topk, tau[0], tau[1], None, None, p, p, p if lmass == "p" else lmass,
                                       p, p, p, None, p, p if df2 == "p" else df2, None, None, variant, ws, ws_bytes, None)


@pytest.mark.parametrize("hist", [False, True], ids=["fwd", "fwd_hist"])
def test_forward_argument_validation_without_gpu(lib, hist):
    err = lib.dvm_last_error
    assert _fwd(lib, hist, p=None) == -1 and b"null pointer" in err()
    assert _fwd(lib, hist, val=None) == -1 and b"null pointer" in err()
    if hist:
        assert _fwd(lib, hist, last=None) == -1 and b"null pointer" in err()
    assert _fwd(lib, hist, B=0) == -1 and b"empty" in err()
    assert _fwd(lib, hist, d=130) == -1 and b"d=130" in err()
    assert _fwd(lib, hist, d=516) == -1 and b"d=516" in err()
    assert _fwd(lib, hist, topk=17) == -1 and b"topk=17" in err()
    assert _fwd(lib, hist, topk=0) == -1 and b"topk=0" in err()
    assert _fwd(lib, hist, n_iter=-1) == -1 and b"n_iter" in err()
    assert _fwd(lib, hist, neg_alpha=0.0) == -1 and b"neg_alpha" in err()
    for tau in ((0.0, 0.9), (0.9, 0.0), (1.5, 0.9), (0.9, 1.0001), (-0.5, 0.5), (float("nan"), 0.5)):
        assert _fwd(lib, hist, tau=tau) == -1 and b"tau" in err(), tau
    assert _fwd(lib, hist, variant=2) == -1 and b"variant" in err()
    assert _fwd(lib, hist) == -3 and b"workspace" in err()
    nb = (lib.dvm_sinkhorn_ub_hist_workspace_bytes if hist else lib.dvm_sinkhorn_ub_workspace_bytes)(1, 8, 8, 128)
    assert _fwd(lib, hist, ws=ONE, ws_bytes=nb - 1) == -3 and b"workspace" in err()
    assert _fwd(lib, hist, tau=(1.0, 1.0), ws=ONE, ws_bytes=nb - 1) == -3   # tau = 1 is inside the range


def test_backward_argument_validation_without_gpu(lib):
    err = lib.dvm_last_error
    assert _bwd(lib, p=None) == -1 and b"null pointer" in err()
    assert _bwd(lib, lmass=None) == -1 and b"null pointer" in err()
    assert _bwd(lib, df2=None) == -1 and b"null pointer" in err()
    assert _bwd(lib, B=0) == -1 and b"empty" in err()
    assert _bwd(lib, d=130) == -1 and b"d=130" in err()
    assert _bwd(lib, d=516) == -1 and b"d=516" in err()
    assert _bwd(lib, topk=17) == -1 and b"topk=17" in err()
    assert _bwd(lib, n_iter=-1) == -1 and b"n_iter" in err()
    assert _bwd(lib, n_iter=33) == -1 and b"n_iter" in err()   # the documented limit is 32
    assert _bwd(lib, neg_alpha=0.0) == -1 and b"neg_alpha" in err()
    for tau in ((0.0, 0.9), (0.9, 0.0), (1.5, 0.9), (0.9, 2.0)):
        assert _bwd(lib, tau=tau) == -1 and b"tau" in err(), tau
    assert _bwd(lib, variant=2) == -1 and b"variant" in err()
    assert _bwd(lib) == -3 and b"workspace" in err()
    assert _bwd(lib, ws=ONE, ws_bytes=lib.dvm_sinkhorn_ub_bwd_workspace_bytes(1, 8, 8, 128, 0)) == -3 and b"workspace" in err()
    # (the query sizes for topk = 16; a buffer for the balanced backward is too small as well)
    assert _bwd(lib, topk=16, ws=ONE, ws_bytes=lib.dvm_sinkhorn_ub_bwd_workspace_bytes(1, 8, 8, 128, 5) - 1) == -3
    assert _bwd(lib, ws=ONE, ws_bytes=lib.dvm_sinkhorn_bwd_workspace_bytes(1, 8, 8, 128, 5) - 256 * 6) == -3


def test_no_cpu_fallback():
    import torch
    from dvm import nn_ops, ops
    from dvm._lib import DvmError
    f = torch.randn(1, 8, 128)
    z = torch.zeros(1, 8, 10)
    with pytest.raises(DvmError):
        ops.sinkhorn_unbalanced(f, f, 10.0, 5, tau=(0.9, 0.9))
    with pytest.raises(DvmError):
        ops.sinkhorn_unbalanced_hist(f, f, 10.0, 5, tau=(0.9, 0.9), log_a=torch.zeros(1, 8))
    with pytest.raises(DvmError):
        ops.sinkhorn_unbalanced_bwd(f, f, 10.0, 5, (0.9, 0.9), None, None, z, z.int(), torch.zeros(1, 8), torch.zeros(1, 6, 8), torch.zeros(1, 6, 8), z)
    g = torch.randn(1, 8, 128, requires_grad=True)
    with pytest.raises(DvmError):
        nn_ops.sinkhorn_unbalanced_topk(g, f, 10.0, 5, tau=(0.9, 0.9))
    with pytest.raises(DvmError):
        nn_ops.sinkhorn_unbalanced_topk(f, f, 10.0, 0, tau=(0.9, 0.9))
    with pytest.raises(DvmError):   # the log weights alone reach the node too
        nn_ops.sinkhorn_unbalanced_topk(f, f, 10.0, 5, log_a=torch.zeros(1, 8, requires_grad=True))


def test_sinkhorn_pi_unbalanced_reaches_the_operator():
    import inspect
    import torch
    import models.loss as ml
    from dvm._lib import DvmError
    sig = inspect.signature(ml.sinkhorn_pi_unbalanced)
    assert list(sig.parameters) == ["x", "y", "alpha", "n_iter", "topk", "tau", "log_a", "log_b"]
    assert [sig.parameters[k].default for k in ("alpha", "n_iter", "topk")] == [inspect.signature(ml.sinkhorn_pi).parameters[k].default
                                                                              for k in ("alpha", "n_iter", "topk")]
    f = torch.randn(1, 8, 128)
    for kw in (dict(tau=(0.9, 0.9)), dict(log_a=torch.zeros(1, 8)), dict(log_b=torch.zeros(1, 8)), {}):
        with pytest.raises(DvmError, match="HIP device"):
            ml.sinkhorn_pi_unbalanced(f, f, **kw)
    pi = ml.SparsePi(torch.zeros(1, 8, 10), torch.zeros(1, 8, 10, dtype=torch.int32), 8)
    assert pi.log_mass is None


def test_tau_helpers():
    from dvm import ops
    assert ops.unbalanced_tau(30.0, 0.3) == pytest.approx(0.3 / (0.3 + 1 / 30.0))
    assert ops.unbalanced_tau(10.0, float("inf")) == 1.0
    assert 0 < ops.unbalanced_tau(100.0, 1e-3) < ops.unbalanced_tau(100.0, 1.0) < 1
    with pytest.raises(ValueError):
        ops.unbalanced_tau(0.0, 1.0)
    assert ops.tau_pair(0.5) == (0.5, 0.5) and ops.tau_pair((0.9, 0.7)) == (0.9, 0.7) and ops.tau_pair("0.9,0.7") == (0.9, 0.7)
    assert ops.tau_pair("1") == (1.0, 1.0)
    for bad in (0.0, 1.5, (0.9, 0.0), "0.9,1.2", "-1"):
        with pytest.raises(ValueError):
            ops.tau_pair(bad)


def test_criterion_switch_defaults_off():
    import models.loss as ml
    assert ml.GraphDeformLoss_Neural().sinkhorn_tau is None
    assert ml.GraphDeformLoss_Neural_Partial().sinkhorn_tau is None


@pytest.mark.parametrize("driver", ["train_driver", "deform_driver"])
def test_drivers_know_sinkhorn_tau(capsys, driver):
    import importlib
    mod = importlib.import_module(driver)
    with pytest.raises(SystemExit) as e:
        mod.main(["--help"])
    assert e.value.code == 0
    assert "--sinkhorn-tau" in capsys.readouterr().out
    with pytest.raises(SystemExit) as e:   # refused without --sinkhorn
        mod.main(["--sinkhorn-tau", "0.9"])
    assert e.value.code == 2 and "--sinkhorn" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:   # and outside (0, 1]
        mod.main(["--sinkhorn", "3", "--sinkhorn-tau", "0.9,1.5"])
    assert e.value.code == 2


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_host_program_under_asan_ubsan_drives_the_new_entries():
    """csrc/san/san_host.cpp, a stand-alone program with the host code compiled under -fsanitize=address,undefined, calls the
    three workspace queries and every rejection path of the three entries (the build is shared with tests/test_sanitizers.py)."""
    src = open(os.path.join(ROOT, "dv-matcher_amd", "csrc", "san", "san_host.cpp")).read()
    for name in NAMES:
        assert name in src, name
    csrc = os.path.join(ROOT, "dv-matcher_amd", "csrc")
    b = subprocess.run(["make", "-C", csrc, "-s", "-j8", "san"], capture_output=True, text=True, timeout=900)
    assert b.returncode == 0, b.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([os.path.join(csrc, "build_san", "san_host")], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0 and "san_host: ok" in r.stdout and "runtime error" not in r.stderr and "ERROR: AddressSanitizer" not in r.stderr, \
        (r.stdout[-500:], r.stderr[-3000:])
