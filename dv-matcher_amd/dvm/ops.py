"""Tensor-level wrappers over the C ABI (include/dvm.h).

torch is used for device memory and streams only: every function takes
contiguous fp32 / int32 tensors that live on a HIP device, allocates the outputs
and the scratch there, and enqueues the kernels on torch's current stream.
"""
import ctypes

import torch

from . import _lib
from ._lib import DvmError, check

_ws_cache = {}
_pair_ctx = set()


def _need_gpu(*ts):
    """Every wrapper starts here: all tensors on ONE HIP device, which becomes the current device (the C ABI launches on
    `torch.cuda.current_stream()` and keeps its per-device state — kernel attributes, helper streams — by current device).
    (This and the two casts below run ~1500 times per training step on the host: they stay on attribute reads.)"""
    dev = -1
    for t in ts:
        if t is None:
            continue
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise DvmError("dvm ops need tensors on a HIP device (got %s); there is no CPU fallback"
                           % (t.device if isinstance(t, torch.Tensor) else type(t)))
        d = t.get_device()
        if dev < 0:
            dev = d
        elif d != dev:
            raise DvmError("dvm ops need all tensors on one device (got cuda:%d and cuda:%d)" % (dev, d))
    if dev >= 0 and dev != torch.cuda.current_device():
        torch.cuda.set_device(dev)


def _f(t):
    """A contiguous fp32 tensor without autograd history (the same object when it already is one)."""
    if t.dtype is torch.float32 and not t.requires_grad and t.is_contiguous():
        return t
    return t.detach().contiguous().float()


def _i(t):
    if t.dtype is torch.int32 and t.is_contiguous():
        return t
    return t.detach().contiguous().to(torch.int32)


def _p(t):
    return None if t is None else t.data_ptr()


def _new(dev, *shape, dtype=torch.float32):
    """An uninitialised output tensor on `dev`: fp32, or the int32 of the index outputs."""
    return torch.empty(shape, dtype=dtype, device=dev)


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream():
    """torch's current stream on the current device as the raw hipStream_t (no Stream object: this runs per launch)."""
    if _raw_stream is not None:
        return _raw_stream(torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream


def workspace(nbytes, device, tag="ws"):
    """Grow-only scratch buffer per (device, current stream, tag): calls on one stream are ordered and may share it,
    calls on different streams (or devices) never do."""
    dev_index = device.index if isinstance(device, torch.device) and device.index is not None else torch.cuda.current_device()
    key = (dev_index, _raw_stream(dev_index) if _raw_stream is not None else torch.cuda.current_stream(device).cuda_stream, tag)
    buf = _ws_cache.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)
        _ws_cache[key] = buf
    return buf


def scratch(nbytes, device):
    """A dedicated, uninitialised scratch buffer of `nbytes` bytes owned by the caller (training arenas, geometry-cache entries,
    pipeline workspaces): with workspace() the only allocation of library scratch, so one replacement reaches all of it."""
    return torch.empty(int(nbytes), dtype=torch.uint8, device=device)


def _call(name, *args):
    """The entry point `name` of the library on torch's current stream: `args` are its arguments in front of the last one, the
    stream.  A failure raises under `name`."""
    check(getattr(_lib.load(), name)(*args, _stream()), name)


def _call_ws(name, args, dev, tag, size_query, *size_args, null_if_empty=False):
    """_call for an entry whose arguments end (.., ws, ws_bytes, stream): the size is what `size_query(*size_args)` answers, the
    buffer workspace(size, dev, tag).  A size of 0 still passes the (256-byte minimum) buffer, except with null_if_empty: those
    entries read ws == NULL as "no workspace" and must get it."""
    lib = _lib.load()
    nb = getattr(lib, size_query)(*size_args)
    ws = None if null_if_empty and not nb else workspace(nb, dev, tag)
    check(getattr(lib, name)(*args, _p(ws), nb, _stream()), name)


def neg_alpha_f32(alpha):
    """`-alpha * distance`: ATen casts the python/numpy scalar to fp32 (models/loss.py:112)."""
    return float(torch.tensor(-float(alpha), dtype=torch.float32).item())


def rownorm2(x):
    _need_gpu(x)
    x = _f(x)
    rows, K = x.numel() // x.shape[-1], x.shape[-1]
    out = _new(x.device, *x.shape[:-1])
    _call("dvm_rownorm2_f32", _p(x), rows, K, _p(out))
    return out


def linear(x, w, bias=None, res=None, bn=None, slope=1.0, channel_major=False, out=None, prefix=None, post=None):
    """1x1 conv / linear layer with its fused epilogue (dvm_linear_f32): act(bn(x W^T + bias + res)).
    point-major (default): x (..., K) -> (..., Co); channel_major: x (B,K,N) -> (B,Co,N) (nn.Conv1d's layout).
    w (Co,K[,1]); bn = (alpha, beta) of the eval-mode BatchNorm (models.model._bn_affine); slope 1 = no activation,
    0 = ReLU, else LeakyReLU.  The contraction is the reference's single-thread fp32 chain, bit for bit.
    post = (scale, r): the JBU "fixup" form r + scale * (x W^T + bias) in the same launch (dvm_linear_scaled_residual_f32;
    excludes res / bn / slope / prefix)."""
    _need_gpu(x, w, bias, res)
    x, w = _f(x), _f(w)
    Co = w.shape[0]
    w = w.reshape(Co, -1)
    K = w.shape[1]
    Cg = 0
    if channel_major:
        B, Kx, N = x.shape
        shape = (B, Co, N)
    elif prefix is not None:   # rows [prefix[b] | x[b, n]]: a conv over cat((g broadcast over the points, x), channels)
        _need_gpu(prefix)
        B, N, Kx = x.shape
        prefix = _f(prefix).reshape(B, -1)
        Cg = prefix.shape[1]
        Kx += Cg
        shape = (B, N, Co)
    else:
        Kx = x.shape[-1]
        B, N = 1, x.numel() // Kx
        shape = x.shape[:-1] + (Co,)
    if Kx != K:
        raise DvmError("linear: x has %d input channels, w expects %d" % (Kx, K))
    if out is None:
        out = _new(x.device, *shape)
    elif tuple(out.shape) != tuple(shape) or not out.is_contiguous() or out.dtype != torch.float32:
        raise DvmError("linear: bad `out`")
    bias = None if bias is None else _f(bias)
    res = None if res is None else _f(res)
    if res is not None and tuple(res.shape) != tuple(shape):
        raise DvmError("linear: residual shape %s != output shape %s" % (tuple(res.shape), tuple(shape)))
    al, be = (None, None) if bn is None else (_f(bn[0]), _f(bn[1]))
    if post is not None:
        if res is not None or bn is not None or slope != 1.0 or Cg:
            raise DvmError("linear: `post` excludes res / bn / slope / prefix")
        scale, r = post
        _need_gpu(r)
        r = _f(r)
        if tuple(r.shape) != tuple(shape):
            raise DvmError("linear: post residual shape %s != output shape %s" % (tuple(r.shape), tuple(shape)))
        _call("dvm_linear_scaled_residual_f32", _p(x), _p(w), B, N, K, Co, 1 if channel_major else 0, _p(bias), float(scale),
              _p(r), _p(out))
    elif Cg:
        _call("dvm_linear_prefix_f32", _p(prefix), Cg, _p(x), _p(w), B, N, K, Co, _p(bias), _p(res), _p(al), _p(be),
              float(slope), _p(out))
    else:
        _call("dvm_linear_f32", _p(x), _p(w), B, N, K, Co, 1 if channel_major else 0, _p(bias), _p(res), _p(al), _p(be),
              float(slope), _p(out))
    return out


def set_deterministic(on=True):
    """Fixed summation order in LG-Net's backward (dvm_set_deterministic: ordered weight-gradient partials, SA backward without its
    split, sorted in-edge lists): parameter gradients are bit-reproducible from run to run.  Returns the previous setting."""
    return bool(_lib.load().dvm_set_deterministic(1 if on else 0))


def is_deterministic():
    """The library's current setting (dvm_get_deterministic: the flag lives in the library — DVM_DETERMINISTIC, dvm_set_deterministic
    from any caller — and is only READ here)."""
    return bool(_lib.load().dvm_get_deterministic())


def linear_wgrad(gy, x, out=None):
    """dW = gy^T x over the rows: gy (R,Co), x (R,K) -> (Co,K) (dvm_linear_wgrad_f32; fp32 atomics over row chunks).
    With `out` (Co,K) the product is ADDED to it in place."""
    _need_gpu(gy, x, out)
    gy, x = _f(gy), _f(x)
    R, Co = gy.shape
    K = x.shape[1]
    if out is None:
        dW = torch.zeros(Co, K, dtype=torch.float32, device=gy.device)
    else:
        dW = out
        if dW.dtype != torch.float32 or not dW.is_contiguous() or dW.numel() != Co * K:
            raise ValueError("linear_wgrad: out must be a contiguous float32 tensor of %d x %d elements" % (Co, K))
    args = (_p(gy), _p(x), R, Co, K, _p(dW))
    if _lib.load().dvm_get_deterministic():   # per-chunk partial tiles added in chunk order (needs scratch)
        _call_ws("dvm_linear_wgrad_ws_f32", args, gy.device, "wgrad", "dvm_linear_wgrad_workspace_bytes", R, Co, K)
    else:
        _call("dvm_linear_wgrad_f32", *args)
    return dW


_bn_pm_sizes = {}


def _bn_pm_bytes(R, C):
    nb = _bn_pm_sizes.get((R, C))
    if nb is None:
        nb = _bn_pm_sizes[(R, C)] = _lib.load().dvm_bn_pm_workspace_bytes(R, C)
    return nb


def bn_act_train_fwd_pm(x, res, gamma, beta, eps, slope, momentum, running_mean=None, running_var=None):
    """Fused training-mode BatchNorm on point-major x (..., C): y = act(bn(x + res)); returns (y, mean, invstd)."""
    _need_gpu(x, res, gamma, beta)
    x = _f(x)
    C = x.shape[-1]
    R = x.numel() // C
    res = None if res is None else _f(res)
    y = torch.empty_like(x)
    mean = _new(x.device, C)
    invstd = torch.empty_like(mean)
    nb = _bn_pm_bytes(R, C)
    ws = workspace(nb, x.device, "bn_pm")
    _call("dvm_bn_act_train_fwd_pm_f32", _p(x), _p(res), _p(gamma), _p(beta), R, C, float(eps), float(slope), float(momentum), _p(y),
          _p(mean), _p(invstd), _p(running_mean), _p(running_var), _p(ws), nb)
    return y, mean, invstd


def bn_act_train_bwd_pm(dy, y, x, res, gamma, mean, invstd, slope, grads=None):
    """-> (dx, dgamma, dbeta); with grads = (dgamma, dbeta) given, the parameter gradients are ADDED to those tensors."""
    _need_gpu(dy, y, x)
    dy, x = _f(dy), _f(x)
    C = x.shape[-1]
    R = x.numel() // C
    dx = torch.empty_like(x)
    if grads is None:
        dgamma = _new(x.device, C)
        dbeta = torch.empty_like(dgamma)
    else:
        dgamma, dbeta = grads
        for t in grads:
            if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != C:
                raise ValueError("bn_act_train_bwd_pm: grads must be contiguous float32 tensors of %d elements" % C)
    nb = _bn_pm_bytes(R, C)
    ws = workspace(nb, x.device, "bn_pm")
    _call("dvm_bn_act_train_bwd_pm_f32", _p(dy), _p(y), _p(x), _p(res), _p(gamma), _p(mean), _p(invstd), R, C, float(slope), _p(dx),
          _p(dgamma), _p(dbeta), int(grads is not None), _p(ws), nb)
    return dx, dgamma, dbeta


def _bn_pm_rows(x, groups):
    """-> (C, rows per group) of a merged batch of `groups` blocks; a group count the library refuses is passed on for it to refuse."""
    C = x.shape[-1]
    rows = x.numel() // C
    if groups >= 1 and rows % groups:
        raise DvmError("bn_act_train_*_pm_groups: %d rows do not split into %d groups" % (rows, groups))
    return C, rows // max(int(groups), 1)


def bn_act_train_fwd_pm_sync(x, res, gamma, beta, eps, slope, momentum, groups, coll, sync_buf, want_var=False, running_mean=None,
                             running_var=None, y=None):
    """bn_act_train_fwd_pm_groups with the statistics taken over all ranks (dvm_bn_act_train_fwd_pm_sync_f32): coll is the address
    of a dvm_collective (None: the plain call), sync_buf a device tensor of dvm_bn_pm_sync_bytes(C, groups) bytes that the
    collective's all-reduce is handed."""
    _need_gpu(x, res, gamma, beta, sync_buf)
    x = _f(x)
    C, R = _bn_pm_rows(x, groups)
    res = None if res is None else _f(res)
    y = torch.empty_like(x) if y is None else y
    mean = _new(x.device, max(int(groups), 1), C)
    invstd = torch.empty_like(mean)
    var = torch.empty_like(mean) if want_var else None
    lib = _lib.load()
    nb = lib.dvm_bn_pm_groups_workspace_bytes(R, C, int(groups))
    ws = workspace(nb, x.device, "bn_pm")
    if coll is not None and sync_buf.numel() * sync_buf.element_size() < lib.dvm_bn_pm_sync_bytes(C, int(groups)):
        raise DvmError("bn_act_train_fwd_pm_sync: sync_buf is smaller than dvm_bn_pm_sync_bytes")
    _call("dvm_bn_act_train_fwd_pm_sync_f32", _p(x), _p(res), _p(gamma), _p(beta), R, C, int(groups), float(eps), float(slope),
          float(momentum), _p(y), _p(mean), _p(invstd), _p(var), _p(running_mean), _p(running_var), _p(ws), nb, coll, _p(sync_buf))
    return (y, mean, invstd, var) if want_var else (y, mean, invstd)


def bn_act_train_fwd_pm_groups(x, res, gamma, beta, eps, slope, momentum, groups, want_var=False, running_mean=None, running_var=None,
                               y=None):
    """bn_act_train_fwd_pm on `groups` consecutive row blocks of x, each normalised with its own statistics
    (dvm_bn_act_train_fwd_pm_var_f32): -> (y, mean [groups][C], invstd [groups][C]) and, with want_var, the unbiased batch variance
    [groups][C]; the running statistics take the groups' updates one after the other.  `y`: an output tensor to fill."""
    _need_gpu(x, res, gamma, beta)
    x = _f(x)
    C, R = _bn_pm_rows(x, groups)
    res = None if res is None else _f(res)
    y = torch.empty_like(x) if y is None else y
    mean = _new(x.device, max(int(groups), 1), C)
    invstd = torch.empty_like(mean)
    var = torch.empty_like(mean) if want_var else None
    nb = _lib.load().dvm_bn_pm_groups_workspace_bytes(R, C, int(groups))
    ws = workspace(nb, x.device, "bn_pm")
    _call("dvm_bn_act_train_fwd_pm_var_f32", _p(x), _p(res), _p(gamma), _p(beta), R, C, int(groups), float(eps), float(slope),
          float(momentum), _p(y), _p(mean), _p(invstd), _p(var), _p(running_mean), _p(running_var), _p(ws), nb)
    return (y, mean, invstd, var) if want_var else (y, mean, invstd)


def _bn_pm_grads(grads, C, dev):
    if grads is None:
        return _new(dev, C), _new(dev, C)
    for t in grads:
        if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != C:
            raise ValueError("bn_act_train_bwd_pm: grads must be contiguous float32 tensors of %d elements" % C)
    return grads


def bn_act_train_bwd_pm_groups(dy, y, x, res, gamma, mean, invstd, slope, groups, grads=None, dx=None):
    """bn_act_train_bwd_pm for a merged batch (dvm_bn_act_train_bwd_pm_groups_f32): mean / invstd [groups][C]; dgamma / dbeta are
    the groups' sums added in group order, ADDED to grads = (dgamma, dbeta) when given."""
    _need_gpu(dy, y, x)
    dy, x = _f(dy), _f(x)
    C, R = _bn_pm_rows(x, groups)
    dx = torch.empty_like(x) if dx is None else dx
    dgamma, dbeta = _bn_pm_grads(grads, C, x.device)
    nb = _lib.load().dvm_bn_pm_groups_workspace_bytes(R, C, int(groups))
    ws = workspace(nb, x.device, "bn_pm")
    _call("dvm_bn_act_train_bwd_pm_groups_f32", _p(dy), _p(y), _p(x), _p(res), _p(gamma), _p(mean), _p(invstd), R, C, int(groups),
          float(slope), _p(dx), _p(dgamma), _p(dbeta), int(grads is not None), _p(ws), nb)
    return dx, dgamma, dbeta


def bn_act_train_bwd_pm_sync(dy, y, x, res, gamma, mean, invstd, slope, groups, coll, sync_buf, grads=None):
    """bn_act_train_bwd_pm_groups with the means of dz and dz xhat taken over all ranks (dvm_bn_act_train_bwd_pm_sync_f32; coll and
    sync_buf as in bn_act_train_fwd_pm_sync); dgamma / dbeta stay this rank's own sums."""
    _need_gpu(dy, y, x, sync_buf)
    dy, x = _f(dy), _f(x)
    C, R = _bn_pm_rows(x, groups)
    dx = torch.empty_like(x)
    dgamma, dbeta = _bn_pm_grads(grads, C, x.device)
    lib = _lib.load()
    nb = lib.dvm_bn_pm_groups_workspace_bytes(R, C, int(groups))
    ws = workspace(nb, x.device, "bn_pm")
    if coll is not None and sync_buf.numel() * sync_buf.element_size() < lib.dvm_bn_pm_sync_bytes(C, int(groups)):
        raise DvmError("bn_act_train_bwd_pm_sync: sync_buf is smaller than dvm_bn_pm_sync_bytes")
    _call("dvm_bn_act_train_bwd_pm_sync_f32", _p(dy), _p(y), _p(x), _p(res), _p(gamma), _p(mean), _p(invstd), R, C, int(groups),
          float(slope), _p(dx), _p(dgamma), _p(dbeta), int(grads is not None), _p(ws), nb, coll, _p(sync_buf))
    return dx, dgamma, dbeta


def softcorr(f1, f2, alpha, topk=10, variant=0, stats=True):
    """f1 (B,N,d), f2 (B,M,d) -> pi_val (B,N,topk), pi_idx (B,N,topk) int32, row_smax (B,N), row_sum (B,N)."""
    _need_gpu(f1, f2)
    f1, f2 = _f(f1), _f(f2)
    B, N, d = f1.shape
    M = f2.shape[1]
    dev = f1.device
    val = _new(dev, B, N, topk)
    idx = _new(dev, B, N, topk, dtype=torch.int32)
    smax = _new(dev, B, N) if stats else None
    ssum = _new(dev, B, N) if stats else None
    _call_ws("dvm_softcorr_fwd_f32", (_p(f1), _p(f2), B, N, M, d, neg_alpha_f32(alpha), topk, _p(val), _p(idx), _p(smax), _p(ssum),
                                      variant), dev, "softcorr", "dvm_softcorr_workspace_bytes", B, N, M, d)
    return val, idx, smax, ssum


def sinkhorn(f1, f2, alpha, n_iter, topk=10, variant=0, potentials=False):
    """Sinkhorn-normalised soft correspondence (dvm_sinkhorn_fwd_f32; not in the reference): n_iter row / column normalisations
    of exp(-alpha * cdist(f1, f2)) in the log domain, a final row step, the top-k of every row.  n_iter = 0 is softcorr.
    f1 (B,N,d), f2 (B,M,d) -> pi_val (B,N,topk), pi_idx (B,N,topk) int32, row_lmax (B,N), row_sum (B,N)[, u (B,N), v (B,M)].
    Forward only: this entry keeps no history of the potentials, so inputs that require grad are refused while grad mode is on;
    the differentiable entry is nn_ops.sinkhorn_topk (sinkhorn_hist + sinkhorn_bwd)."""
    if torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in (f1, f2)):
        raise DvmError("sinkhorn is forward only (it keeps no history for a backward): use nn_ops.sinkhorn_topk to differentiate, "
                       "or detach the features / call it under torch.no_grad()")
    _need_gpu(f1, f2)
    f1, f2 = _f(f1), _f(f2)
    B, N, d = f1.shape
    M = f2.shape[1]
    dev = f1.device
    val = _new(dev, B, N, topk)
    idx = _new(dev, B, N, topk, dtype=torch.int32)
    lmax, lsum = _new(dev, B, N), _new(dev, B, N)
    u = _new(dev, B, N) if potentials else None
    v = _new(dev, B, M) if potentials else None
    _call_ws("dvm_sinkhorn_fwd_f32", (_p(f1), _p(f2), B, N, M, d, neg_alpha_f32(alpha), int(n_iter), topk, _p(val), _p(idx), _p(lmax),
                                      _p(lsum), _p(u), _p(v), variant), dev, "sinkhorn", "dvm_sinkhorn_workspace_bytes", B, N, M, d)
    return (val, idx, lmax, lsum, u, v) if potentials else (val, idx, lmax, lsum)


def sinkhorn_hist(f1, f2, alpha, n_iter, topk=10, variant=0):
    """ops.sinkhorn with the history of its potentials kept for sinkhorn_bwd (dvm_sinkhorn_fwd_hist_f32): the same sweeps on the
    same operands, so val / idx / lmax / lsum and the last slices of the histories carry ops.sinkhorn's bits.
    -> pi_val, pi_idx, row_lmax, row_sum, u_hist (B,n_iter+1,N) = u^1..u^T, u^final, v_hist (B,n_iter+1,M) = v^0 (= 0)..v^T.
    Takes no part in autograd itself (nn_ops.sinkhorn_topk is the node)."""
    _need_gpu(f1, f2)
    f1, f2 = _f(f1), _f(f2)
    B, N, d = f1.shape
    M = f2.shape[1]
    n_iter = int(n_iter)
    dev = f1.device
    val = _new(dev, B, N, topk)
    idx = _new(dev, B, N, topk, dtype=torch.int32)
    lmax, lsum = _new(dev, B, N), _new(dev, B, N)
    u_hist = _new(dev, B, max(n_iter, 0) + 1, N)
    v_hist = _new(dev, B, max(n_iter, 0) + 1, M)
    _call_ws("dvm_sinkhorn_fwd_hist_f32", (_p(f1), _p(f2), B, N, M, d, neg_alpha_f32(alpha), n_iter, topk, _p(val), _p(idx), _p(lmax),
                                           _p(lsum), _p(u_hist), _p(v_hist), variant),
             dev, "sinkhorn_hist", "dvm_sinkhorn_hist_workspace_bytes", B, N, M, d)
    return val, idx, lmax, lsum, u_hist, v_hist


def sinkhorn_bwd(f1, f2, alpha, n_iter, val, idx, u_hist, v_hist, gval, variant=0):
    """Backward of the unrolled Sinkhorn operator (dvm_sinkhorn_bwd_f32): gval (B,N,topk) -> (d_f1 (B,N,d), d_f2 (B,M,d)).
    val / idx / u_hist / v_hist are sinkhorn_hist's outputs for the same f1, f2, alpha, n_iter.  No float atomics: two calls give
    the same bits."""
    _need_gpu(f1, f2, gval)
    f1, f2, gval, val, idx, u_hist, v_hist = _f(f1), _f(f2), _f(gval), _f(val), _i(idx), _f(u_hist), _f(v_hist)
    B, N, d = f1.shape
    M = f2.shape[1]
    n_iter = int(n_iter)
    topk = val.shape[-1]
    if n_iter >= 0 and (tuple(u_hist.shape) != (B, n_iter + 1, N) or tuple(v_hist.shape) != (B, n_iter + 1, M)):
        raise ValueError("sinkhorn_bwd: u_hist / v_hist must be (B, n_iter + 1, N) / (B, n_iter + 1, M), got %s / %s"
                         % (tuple(u_hist.shape), tuple(v_hist.shape)))
    df1, df2 = torch.empty_like(f1), torch.empty_like(f2)
    _call_ws("dvm_sinkhorn_bwd_f32", (_p(f1), _p(f2), B, N, M, d, neg_alpha_f32(alpha), n_iter, topk, _p(val), _p(idx), _p(u_hist),
                                      _p(v_hist), _p(gval), _p(df1), _p(df2), variant),
             f1.device, "sinkhorn_bwd", "dvm_sinkhorn_bwd_workspace_bytes", B, N, M, d, n_iter)
    return df1, df2


def unbalanced_tau(alpha, rho):
    """The damping factor of unbalanced Sinkhorn with marginal penalty rho * KL at regularisation 1 / alpha:
    rho / (rho + 1 / alpha), in (0, 1); rho = inf gives 1, the balanced operator."""
    alpha, rho = float(alpha), float(rho)
    if not (alpha > 0 and rho > 0):
        raise ValueError("unbalanced_tau: alpha and rho must be positive (got %g, %g)" % (alpha, rho))
    return 1.0 if rho == float("inf") else rho / (rho + 1.0 / alpha)


def tau_pair(tau):
    """(tau_row, tau_col) from a pair, one number for both, or the drivers' text form "R[,C]"; each must lie in (0, 1]."""
    if isinstance(tau, str):
        tau = [float(x) for x in tau.split(",")]
        tau = tau[0] if len(tau) == 1 else tau
    tr, tc = (tau, tau) if isinstance(tau, (int, float)) else tau
    tr, tc = float(tr), float(tc)
    if not (0.0 < tr <= 1.0 and 0.0 < tc <= 1.0):
        raise ValueError("tau = (%g, %g): each factor must lie in (0, 1]" % (tr, tc))
    return tr, tc


def _log_weight(t, B, n, name):
    if t is None:
        return None
    t = _f(t)
    if tuple(t.shape) != (B, n):
        raise ValueError("%s must be (B, %d) = (%d, %d), got %s" % (name, n, B, n, tuple(t.shape)))
    return t


def sinkhorn_unbalanced(f1, f2, alpha, n_iter, tau=(1.0, 1.0), log_a=None, log_b=None, topk=10, variant=0):
    """Unbalanced (KL-relaxed) Sinkhorn correspondence (dvm_sinkhorn_ub_fwd_f32; the definition is in include/dvm.h): every
    potential update is damped by tau = (tau_row, tau_col) in (0, 1], log_a (B,N) / log_b (B,M) are the log weights of the two
    sides (None = 0 / log(N/M)), and a row whose matches are all expensive ends with a small mass.
    -> pi_val (B,N,topk), pi_idx int32, row_lmax, row_sum, row_lmass (B,N) = log sum_j P_ij, u (B,N), v (B,M).
    tau = (1, 1) without weights is ops.sinkhorn, bit for bit (row_lmass = 0).  Forward only, like ops.sinkhorn: the
    differentiable entry is nn_ops.sinkhorn_unbalanced_topk."""
    if torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in (f1, f2, log_a, log_b)):
        raise DvmError("sinkhorn_unbalanced is forward only (it keeps no history for a backward): use "
                       "nn_ops.sinkhorn_unbalanced_topk to differentiate, or detach the inputs / call it under torch.no_grad()")
    _need_gpu(f1, f2, log_a, log_b)
    f1, f2 = _f(f1), _f(f2)
    B, N, d = f1.shape
    M = f2.shape[1]
    tr, tc = tau_pair(tau)
    log_a, log_b = _log_weight(log_a, B, N, "log_a"), _log_weight(log_b, B, M, "log_b")
    dev = f1.device
    val = _new(dev, B, N, topk)
    idx = _new(dev, B, N, topk, dtype=torch.int32)
    lmax, lsum, lmass, u = (_new(dev, B, N) for _ in range(4))
    v = _new(dev, B, M)
    _call_ws("dvm_sinkhorn_ub_fwd_f32", (_p(f1), _p(f2), B, N, M, d, neg_alpha_f32(alpha), int(n_iter), topk, tr, tc, _p(log_a), _p(log_b),
                                         _p(val), _p(idx), _p(lmax), _p(lsum), _p(lmass), _p(u), _p(v), variant),
             dev, "sinkhorn_ub", "dvm_sinkhorn_ub_workspace_bytes", B, N, M, d)
    return val, idx, lmax, lsum, lmass, u, v


def sinkhorn_unbalanced_hist(f1, f2, alpha, n_iter, tau=(1.0, 1.0), log_a=None, log_b=None, topk=10, variant=0):
    """ops.sinkhorn_unbalanced with the normalisers of every iterate kept for sinkhorn_unbalanced_bwd
    (dvm_sinkhorn_ub_fwd_hist_f32): the same sweeps on the same operands, so the same bits.
    -> pi_val, pi_idx, row_lmax, row_sum, row_lmass, rn_hist (B,n_iter+1,N) = m^1..m^T, m^final, cn_hist (B,n_iter+1,M) = 0, n^1..n^T.
    Takes no part in autograd itself (nn_ops.sinkhorn_unbalanced_topk is the node)."""
    _need_gpu(f1, f2, log_a, log_b)
    f1, f2 = _f(f1), _f(f2)
    B, N, d = f1.shape
    M = f2.shape[1]
    n_iter = int(n_iter)
    tr, tc = tau_pair(tau)
    log_a, log_b = _log_weight(log_a, B, N, "log_a"), _log_weight(log_b, B, M, "log_b")
    dev = f1.device
    val = _new(dev, B, N, topk)
    idx = _new(dev, B, N, topk, dtype=torch.int32)
    lmax, lsum, lmass = (_new(dev, B, N) for _ in range(3))
    rn_hist = _new(dev, B, max(n_iter, 0) + 1, N)
    cn_hist = _new(dev, B, max(n_iter, 0) + 1, M)
    _call_ws("dvm_sinkhorn_ub_fwd_hist_f32", (_p(f1), _p(f2), B, N, M, d, neg_alpha_f32(alpha), n_iter, topk, tr, tc, _p(log_a), _p(log_b),
                                              _p(val), _p(idx), _p(lmax), _p(lsum), _p(lmass), _p(rn_hist), _p(cn_hist), variant),
             dev, "sinkhorn_ub_hist", "dvm_sinkhorn_ub_hist_workspace_bytes", B, N, M, d)
    return val, idx, lmax, lsum, lmass, rn_hist, cn_hist


def sinkhorn_unbalanced_bwd(f1, f2, alpha, n_iter, tau, log_a, log_b, val, idx, lmass, rn_hist, cn_hist, gval, glmass=None, variant=0):
    """Backward of the unrolled unbalanced operator (dvm_sinkhorn_ub_bwd_f32): gval (B,N,topk) = dL/d pi_val and glmass (B,N) =
    dL/d row_lmass (None = 0) -> (d_f1 (B,N,d), d_f2 (B,M,d), d_log_a (B,N), d_log_b (B,M)).  val / idx / lmass / rn_hist /
    cn_hist are sinkhorn_unbalanced_hist's outputs for the same inputs.  No float atomics: two calls give the same bits."""
    _need_gpu(f1, f2, gval, glmass, log_a, log_b)
    f1, f2, gval, val, lmass, rn_hist, cn_hist = _f(f1), _f(f2), _f(gval), _f(val), _f(lmass), _f(rn_hist), _f(cn_hist)
    idx = _i(idx)
    B, N, d = f1.shape
    M = f2.shape[1]
    n_iter = int(n_iter)
    topk = val.shape[-1]
    tr, tc = tau_pair(tau)
    log_a, log_b = _log_weight(log_a, B, N, "log_a"), _log_weight(log_b, B, M, "log_b")
    glmass = _log_weight(glmass, B, N, "glmass")
    if n_iter >= 0 and (tuple(rn_hist.shape) != (B, n_iter + 1, N) or tuple(cn_hist.shape) != (B, n_iter + 1, M)):
        raise ValueError("sinkhorn_unbalanced_bwd: rn_hist / cn_hist must be (B, n_iter + 1, N) / (B, n_iter + 1, M), got %s / %s"
                         % (tuple(rn_hist.shape), tuple(cn_hist.shape)))
    df1, df2 = torch.empty_like(f1), torch.empty_like(f2)
    dla, dlb = _new(f1.device, B, N), _new(f1.device, B, M)
    _call_ws("dvm_sinkhorn_ub_bwd_f32", (_p(f1), _p(f2), B, N, M, d, neg_alpha_f32(alpha), n_iter, topk, tr, tc, _p(log_a), _p(log_b), _p(val),
                                         _p(idx), _p(lmass), _p(rn_hist), _p(cn_hist), _p(gval), _p(glmass), _p(df1), _p(df2), _p(dla),
                                         _p(dlb), variant),
             f1.device, "sinkhorn_ub_bwd", "dvm_sinkhorn_ub_bwd_workspace_bytes", B, N, M, d, n_iter)
    return df1, df2, dla, dlb


def softcorr_bwd(f1, f2, alpha, val, idx, smax, ssum, gval, variant=0):
    """Backward of softcorr: gval (B,N,topk) -> (d_f1 (B,N,d), d_f2 (B,M,d)).  val / idx / smax / ssum are softcorr's outputs for
    the same f1, f2, alpha: a row's in-range columns must be distinct (repeated slots carry val 0, as softcorr writes them at
    M < topk), since each slot's entry takes both terms of dL/dS."""
    _need_gpu(f1, f2, gval)
    f1, f2, gval, val, idx = _f(f1), _f(f2), _f(gval), _f(val), _i(idx)
    B, N, d = f1.shape
    M = f2.shape[1]
    topk = val.shape[-1]
    df1, df2 = torch.empty_like(f1), torch.empty_like(f2)
    _call_ws("dvm_softcorr_bwd_f32", (_p(f1), _p(f2), B, N, M, d, neg_alpha_f32(alpha), topk, _p(val), _p(idx), _p(smax), _p(ssum),
                                      _p(gval), _p(df1), _p(df2), variant),
             f1.device, "softcorr_bwd", "dvm_softcorr_bwd_workspace_bytes", B, N, M, d)
    return df1, df2


def n2p_core_fwd(qkv, idx, heads=4):
    """qkv (B,N,3C), idx (B,N,K) int32 -> out (B,N,C), attn (B,N,K,heads)."""
    _need_gpu(qkv, idx)
    qkv, idx = _f(qkv), _i(idx)
    B, N, C3 = qkv.shape
    C, K = C3 // 3, idx.shape[-1]
    out = _new(qkv.device, B, N, C)
    attn = _new(qkv.device, B, N, K, heads)
    _call("dvm_n2p_core_fwd_f32", _p(qkv), _p(idx), B, N, C, K, heads, _p(out), _p(attn))
    return out, attn


def n2p_core_bwd(qkv, idx, attn, gout, heads=4):
    """-> d_qkv (B,N,3C)."""
    _need_gpu(qkv, idx, attn, gout)
    qkv, idx, gout = _f(qkv), _i(idx), _f(gout)
    B, N, C3 = qkv.shape
    C, K = C3 // 3, idx.shape[-1]
    dqkv = torch.empty_like(qkv)
    _call_ws("dvm_n2p_core_bwd_f32", (_p(qkv), _p(idx), _p(attn), _p(gout), B, N, C, K, heads, _p(dqkv)),
             qkv.device, "n2p_bwd", "dvm_n2p_core_bwd_workspace_bytes", B, N, K)
    return dqkv


def argmin_exact(f1, f2, want_dist=False, screen=True):
    """Hard map T[b,i] = argmin_j of the exact-difference distance (ties -> lowest j).  screen=False evaluates every
    column in that form; the default screens the columns on the matrix cores first (same result)."""
    _need_gpu(f1, f2)
    f1, f2 = _f(f1), _f(f2)
    B, N, d = f1.shape
    M = f2.shape[1]
    T = _new(f1.device, B, N, dtype=torch.int32)
    dm = _new(f1.device, B, N) if want_dist else None
    args = (_p(f1), _p(f2), B, N, M, d, _p(T), _p(dm))
    if screen:
        _call_ws("dvm_argmin_exact_f32", args, f1.device, "argmin", "dvm_argmin_workspace_bytes", B, N, M, d, 0, null_if_empty=True)
    else:
        _call("dvm_argmin_exact_f32", *args, None, 0)   # no workspace: every column
    return (T, dm) if want_dist else T


def precise_map_max_m():
    """The largest M precise_map takes (a row's products with every target vertex are held in LDS).  No device is needed."""
    return int(_lib.load().dvm_precise_map_max_m())


def precise_map_plan(B, N, M, d, F):
    """How precise_map launches at these sizes -> (source rows per workgroup, threads per workgroup, target rows per step of the
    LDS fill, the cap on M).  No device is needed."""
    r, t, c, m = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    check(_lib.load().dvm_precise_map_plan(B, N, M, d, F, ctypes.byref(r), ctypes.byref(t), ctypes.byref(c), ctypes.byref(m)),
          "dvm_precise_map_plan")
    return r.value, t.value, c.value, m.value


def precise_map(f1, f2, faces, want_dist=True, check=True, want_stats=False):
    """The precise (vertex-to-point) map: for every f1[b,i] the closest point of the triangle mesh (f2[b], faces) in feature space
    -> (face (B,N) int32, bary (B,N,3), pi_idx (B,N,3) int32 = faces[face], dist (B,N) or None).  (bary, pi_idx) is a sparse row
    of three entries: ops.apply and the loss terms take it as (pi_val, pi_idx).  faces (F,3), one connectivity for the B entries;
    a face with an index outside [0,M) is left out: check=True reads the count back (one synchronisation) and raises DvmError if
    there is one, check=False never synchronises.  want_stats appends the device tensor stats (2,) int64: faces left out, exact
    evaluations made.  Definition, ties and limits: include/dvm.h."""
    read_back = check   # (the parameter, named by the interface, hides the module's check() in this body: use this name here)
    _need_gpu(f1, f2, faces)
    f1, f2, faces = _f(f1), _f(f2), _i(faces)
    if f1.dim() != 3 or f2.dim() != 3 or f2.shape[0] != f1.shape[0] or f2.shape[2] != f1.shape[2] or faces.dim() != 2 or faces.shape[1] != 3:
        raise DvmError("precise_map: f1 must be (B,N,d), f2 (B,M,d) and faces (F,3) (got %s, %s, %s)"
                       % (tuple(f1.shape), tuple(f2.shape), tuple(faces.shape)))
    B, N, d = f1.shape
    M, F = f2.shape[1], faces.shape[0]
    dev = f1.device
    face, bary, pi_idx = _new(dev, B, N, dtype=torch.int32), _new(dev, B, N, 3), _new(dev, B, N, 3, dtype=torch.int32)
    dist = _new(dev, B, N) if want_dist else None
    stats = _new(dev, 2, dtype=torch.int64)
    _call_ws("dvm_precise_map_f32", (_p(f1), _p(f2), _p(faces), B, N, M, d, F, _p(face), _p(bary), _p(pi_idx), _p(dist), _p(stats)), dev,
             "precise_map", "dvm_precise_map_workspace_bytes", B, N, M, d, F)
    if read_back:
        bad = int(stats[0].item())
        if bad:
            raise DvmError("precise_map: %d of the %d faces hold an index outside [0, %d) and were left out" % (bad, F, M))
    return (face, bary, pi_idx, dist, stats) if want_stats else (face, bary, pi_idx, dist)


def argmin_pair(f1, f2):
    """Both hard maps of a pair from one sweep: (T12 (B,N) into f2, T21 (B,M) into f1)."""
    _need_gpu(f1, f2)
    f1, f2 = _f(f1), _f(f2)
    B, N, d = f1.shape
    M = f2.shape[1]
    T12 = _new(f1.device, B, N, dtype=torch.int32)
    T21 = _new(f1.device, B, M, dtype=torch.int32)
    _call_ws("dvm_argmin_pair_f32", (_p(f1), _p(f2), B, N, M, d, _p(T12), _p(T21), None, None),
             f1.device, "argmin", "dvm_argmin_workspace_bytes", B, N, M, d, 1, null_if_empty=True)
    return T12, T21


def knn_cdist(x, y, k):
    _need_gpu(x, y)
    x, y = _f(x), _f(y)
    B, N, C = x.shape
    M = y.shape[1]
    idx = _new(x.device, B, N, k, dtype=torch.int32)
    _call_ws("dvm_knn_cdist_f32", (_p(x), _p(y), B, N, M, C, k, _p(idx)), x.device, "knn_cdist", "dvm_knn_cdist_workspace_bytes", B, N, M, C)
    return idx


def apply(pi_val, pi_idx, V):
    _need_gpu(pi_val, pi_idx, V)
    pi_val, pi_idx, V = _f(pi_val), _i(pi_idx), _f(V)
    B, N, topk = pi_val.shape
    M, C = V.shape[1], V.shape[2]
    out = _new(V.device, B, N, C)
    _call("dvm_softcorr_apply_f32", _p(pi_val), _p(pi_idx), _p(V), B, N, M, topk, C, _p(out))
    return out


def apply_bwd(pi_val, pi_idx, V, gout, atomics=False):
    """Backward of apply: -> (d_val (B,N,topk), d_V (B,M,C)).  atomics=True: the scatter-add variant (no workspace)."""
    _need_gpu(pi_val, pi_idx, V, gout)
    pi_val, pi_idx, V, gout = _f(pi_val), _i(pi_idx), _f(V), _f(gout)
    B, N, topk = pi_val.shape
    M, C = V.shape[1], V.shape[2]
    dval = torch.empty_like(pi_val)
    dV = torch.empty_like(V)
    args = (_p(pi_val), _p(pi_idx), _p(V), _p(gout), B, N, M, topk, C, _p(dval), _p(dV))
    if atomics:
        _call("dvm_softcorr_apply_bwd_f32", *args, None, 0)
    else:
        _call_ws("dvm_softcorr_apply_bwd_f32", args, V.device, "apply_bwd", "dvm_softcorr_apply_bwd_workspace_bytes", B, N, M, topk,
                 null_if_empty=True)
    return dval, dV


def fps(xyz, npoint, start):
    _need_gpu(xyz, start)
    xyz, start = _f(xyz), _i(start)
    B, N, _ = xyz.shape
    out = _new(xyz.device, B, npoint, dtype=torch.int32)
    _call("dvm_fps_f32", _p(xyz), B, N, npoint, _p(start), _p(out))
    return out


def dg_build(xyz, start):
    """xyz (B,N,3), start (B,) -> dict(nodes_idx, one_ring, infl_idx, dists, weights, sigma)."""
    _need_gpu(xyz, start)
    xyz, start = _f(xyz), _i(start)
    B, N, _ = xyz.shape
    Nn = N // 2
    dev = xyz.device
    out = dict(nodes_idx=_new(dev, B, Nn, dtype=torch.int32),
               one_ring=_new(dev, B, Nn, 9, dtype=torch.int32),
               infl_idx=_new(dev, B, N, 3, dtype=torch.int32),
               dists=_new(dev, B, N, 3),
               weights=_new(dev, B, N, 3),
               sigma=_new(dev, B, dtype=torch.float64))
    _call_ws("dvm_dg_build_f32", (_p(xyz), B, N, _p(start), _p(out["nodes_idx"]), _p(out["one_ring"]), _p(out["infl_idx"]),
                                  _p(out["dists"]), _p(out["weights"]), _p(out["sigma"])), dev, "dg_build", "dvm_dg_build_workspace_bytes", B, N)
    return out


_RING_METRICS = {"euclidean": 0, "geodesic": 1}


def dg_skin_geod_plan(B, N, Nn, ring_k=0):
    """How dg_skin_geod launches at these sizes -> (vertices per workgroup, waves that share a tile's node range, length of the
    per-lane list).  No device is needed."""
    t, s, ln = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    check(_lib.load().dvm_dg_skin_geod_plan(B, N, Nn, ring_k, ctypes.byref(t), ctypes.byref(s), ctypes.byref(ln)), "dvm_dg_skin_geod_plan")
    return t.value, s.value, ln.value


def dg_skin_geod(dist, nodes_idx, ring_k=0, slices=None):
    """Skinning by a distance matrix: dist (B,N,N), nodes_idx (B,Nn) -> (infl_idx (B,N,3) int32, dists (B,N,3), ring (B,Nn,ring_k)
    int32 or None).  Vertex v meets node position j at dist[b, nodes_idx[b,j], v]; the order is (d, j) with NaN as +inf, -0 == +0
    and ties to the lower j (include/dvm.h).  slices: the waves per vertex tile, None = the library's choice."""
    _need_gpu(dist, nodes_idx)
    dist, nodes_idx = _f(dist), _i(nodes_idx)
    B, N, N2 = dist.shape
    if N2 != N or nodes_idx.dim() != 2 or nodes_idx.shape[0] != B:
        raise DvmError("dg_skin_geod: dist must be (B,N,N) and nodes_idx (B,Nn) (got %s, %s)" % (tuple(dist.shape), tuple(nodes_idx.shape)))
    Nn = nodes_idx.shape[1]
    dev = dist.device
    ring_k = int(ring_k)
    infl, dists = _new(dev, B, N, 3, dtype=torch.int32), _new(dev, B, N, 3)
    ring = _new(dev, B, Nn, ring_k, dtype=torch.int32) if ring_k > 0 else None
    if slices is None:
        _call("dvm_dg_skin_geod_f32", _p(dist), _p(nodes_idx), B, N, Nn, ring_k, _p(infl), _p(dists), _p(ring))
    else:
        _call("dvm_dg_skin_geod_slices_f32", _p(dist), _p(nodes_idx), B, N, Nn, ring_k, int(slices), _p(infl), _p(dists), _p(ring))
    return infl, dists, ring


def dg_skin_weights(dists, sigma):
    """dists (B,N,3), sigma (B,) -> weights (B,N,3) = exp(-d^2 / float(2 sigma^2)) row-normalised; an infinite d weighs 0 and a row
    without weight becomes (1,0,0)."""
    _need_gpu(dists)
    dists = _f(dists)
    B, N, _ = dists.shape
    sigma = torch.as_tensor(sigma, dtype=torch.float64).reshape(-1).to(dists.device).contiguous()
    if sigma.numel() != B:
        raise DvmError("dg_skin_weights: sigma must hold one value per batch element (got %d for B=%d)" % (sigma.numel(), B))
    out = torch.empty_like(dists)
    _call("dvm_dg_skin_weights_f32", _p(dists), _p(sigma), B, N, _p(out))
    return out


def dg_build_geod(xyz, dist, start, ring_metric="euclidean"):
    """dg_build with the skinning taken from dist (B,N,N) -> the same dict.  nodes_idx, sigma and (ring_metric "euclidean") one_ring
    are dg_build's; infl_idx, dists, weights — and under ring_metric "geodesic" one_ring — follow dist (dg_skin_geod's rules)."""
    if ring_metric not in _RING_METRICS:
        raise ValueError("ring_metric must be 'euclidean' or 'geodesic' (got %r)" % (ring_metric,))
    _need_gpu(xyz, dist, start)
    xyz, dist, start = _f(xyz), _f(dist), _i(start)
    B, N, _ = xyz.shape
    if tuple(dist.shape) != (B, N, N):
        raise DvmError("dg_build_geod: dist must be (B,N,N) = %s (got %s)" % ((B, N, N), tuple(dist.shape)))
    Nn = N // 2
    dev = xyz.device
    out = dict(nodes_idx=_new(dev, B, Nn, dtype=torch.int32),
               one_ring=_new(dev, B, Nn, 9, dtype=torch.int32),
               infl_idx=_new(dev, B, N, 3, dtype=torch.int32),
               dists=_new(dev, B, N, 3),
               weights=_new(dev, B, N, 3),
               sigma=_new(dev, B, dtype=torch.float64))
    _call_ws("dvm_dg_build_geod_f32", (_p(xyz), _p(dist), B, N, _p(start), _RING_METRICS[ring_metric], _p(out["nodes_idx"]),
                                       _p(out["one_ring"]), _p(out["infl_idx"]), _p(out["dists"]), _p(out["weights"]), _p(out["sigma"])),
             dev, "dg_build", "dvm_dg_build_geod_workspace_bytes", B, N)
    return out


def rot6d(d6):
    """rotation_6d_to_matrix: d6 (...,6) -> (...,3,3)."""
    _need_gpu(d6)
    d6 = _f(d6)
    rows = d6.numel() // 6
    R = _new(d6.device, *d6.shape[:-1], 3, 3)
    _call("dvm_rot6d_f32", _p(d6), rows, _p(R))
    return R


def rot6d_bwd(d6, gR):
    _need_gpu(d6, gR)
    d6, gR = _f(d6), _f(gR)
    out = torch.empty_like(d6)
    _call("dvm_rot6d_bwd_f32", _p(d6), _p(gR), d6.numel() // 6, _p(out))
    return out


def dg_warp_arap_bwd(xyz, g, R, T, gw, ga):
    """-> (d_R (B,Nn,3,3), d_T (B,Nn,3))."""
    _need_gpu(xyz, R, T, gw, ga)
    xyz, R, T, gw, ga = _f(xyz), _f(R), _f(T), _f(gw), _f(ga)
    B, N, _ = xyz.shape
    dR, dT = torch.empty_like(R), torch.empty_like(T)
    _call("dvm_dg_warp_arap_bwd_f32", _p(xyz), B, N, _p(_i(g["nodes_idx"])), _p(_i(g["one_ring"])), _p(_i(g["infl_idx"])),
          _p(_f(g["weights"])), _p(R), _p(T), _p(gw), _p(ga), _p(dR), _p(dT))
    return dR, dT


def chamfer_bwd(a, b, i1, i2, g1, g2):
    _need_gpu(a, b, g1, g2)
    a, b, g1, g2 = _f(a), _f(b), _f(g1), _f(g2)
    B, N, _ = a.shape
    M = b.shape[1]
    da, db = torch.empty_like(a), torch.empty_like(b)
    _call("dvm_chamfer_bwd_f32", _p(a), _p(b), _p(_i(i1)), _p(_i(i2)), _p(g1), _p(g2), B, N, M, _p(da), _p(db))
    return da, db


def dg_warp_arap(xyz, g, R, T):
    """xyz (B,N,3), graph dict, R (B,Nn,3,3), T (B,Nn,3) -> warped (B,N,3), arap (B,), sr (B,)."""
    _need_gpu(xyz, R, T)
    xyz, R, T = _f(xyz), _f(R), _f(T)
    B, N, _ = xyz.shape
    dev = xyz.device
    warped, arap, sr = _new(dev, B, N, 3), _new(dev, B), _new(dev, B)
    _call("dvm_dg_warp_arap_fwd_f32", _p(xyz), B, N, _p(_i(g["nodes_idx"])), _p(_i(g["one_ring"])), _p(_i(g["infl_idx"])),
          _p(_f(g["weights"])), _p(R), _p(T), _p(warped), _p(arap), _p(sr))
    return warped, arap, sr


def dg_warp_arap_graph(xyz, g, R, T):
    """As dg_warp_arap for a graph whose node count and ring width are whatever g holds (the mesh-mode graph:
    nodes_idx (B,Nn), one_ring (B,Nn,K), infl_idx / weights (B,N,3))."""
    _need_gpu(xyz, R, T)
    xyz, R, T = _f(xyz), _f(R), _f(T)
    B, N, _ = xyz.shape
    nodes, ring = _i(g["nodes_idx"]), _i(g["one_ring"])
    Nn, K = nodes.shape[1], ring.shape[2]
    dev = xyz.device
    warped, arap, sr = _new(dev, B, N, 3), _new(dev, B), _new(dev, B)
    _call("dvm_dg_warp_arap_graph_f32", _p(xyz), B, N, Nn, K, _p(nodes), _p(ring), _p(_i(g["infl_idx"])), _p(_f(g["weights"])),
          _p(R), _p(T), _p(warped), _p(arap), _p(sr))
    return warped, arap, sr


def chamfer(a, b, want_idx=True):
    _need_gpu(a, b)
    a, b = _f(a), _f(b)
    B, N, _ = a.shape
    M = b.shape[1]
    dev = a.device
    d1, d2 = _new(dev, B, N), _new(dev, B, M)
    i1 = _new(dev, B, N, dtype=torch.int32) if want_idx else None
    i2 = _new(dev, B, M, dtype=torch.int32) if want_idx else None
    _call_ws("dvm_chamfer_fwd_f32", (_p(a), _p(b), B, N, M, _p(d1), _p(d2), _p(i1), _p(i2)), dev, "chamfer", "dvm_chamfer_workspace_bytes", B, N, M)
    return d1, d2, i1, i2


DEFORMER_KEYS = ["conv_layer.weight", "conv_layer.bias"] + [
    "deformation_decoder_layer.linear.%d.%s" % (li, wb) for li in (0, 2, 4, 6) for wb in ("weight", "bias")]


def deformer_weight_list(weights, device):
    """state_dict (reference key names; '.' may be '__') -> the 10 contiguous fp32 device tensors of the ABI."""
    out = []
    for k in DEFORMER_KEYS:
        v = weights[k] if k in weights else weights[k.replace(".", "__")]
        v = torch.as_tensor(v)
        out.append(v.detach().to(device=device, dtype=torch.float32).contiguous().reshape(-1) if "conv_layer" in k
                   else v.detach().to(device=device, dtype=torch.float32).contiguous())
    return out


def deformer(wl, feat1, feat2, verts1, verts12, idx11, idx22, pi_val, pi_idx, fps1, variant=0):
    _need_gpu(feat1, feat2, verts1, verts12, idx11, idx22, pi_val, pi_idx, fps1, *wl)
    feat1, feat2, verts1, verts12, pi_val = _f(feat1), _f(feat2), _f(verts1), _f(verts12), _f(pi_val)
    idx11, idx22, pi_idx, fps1 = _i(idx11), _i(idx22), _i(pi_idx), _i(fps1)
    B, N, _ = feat1.shape
    M = feat2.shape[1]
    Nn, k, topk = fps1.shape[1], idx11.shape[2], pi_val.shape[2]
    out = _new(feat1.device, B, Nn, 9)
    _call_ws("dvm_deformer_fwd_f32", (_p(feat1), _p(feat2), _p(verts1), _p(verts12), _p(idx11), _p(idx22), _p(pi_val), _p(pi_idx), _p(fps1),
                                      B, N, M, Nn, k, topk, *[_p(w) for w in wl], _p(out), variant),
             feat1.device, "deformer", "dvm_deformer_workspace_bytes", B, N, M, Nn)
    return out


def map_term(verts12, verts2, idx11, idx22, pi_val, pi_idx):
    _need_gpu(verts12, verts2, idx11, idx22, pi_val, pi_idx)
    verts12, verts2, pi_val = _f(verts12), _f(verts2), _f(pi_val)
    idx11, idx22, pi_idx = _i(idx11), _i(idx22), _i(pi_idx)
    B, N, _ = verts12.shape
    M, k, topk = verts2.shape[1], idx11.shape[2], pi_val.shape[2]
    out = _new(verts12.device, B)
    _call_ws("dvm_map_term_f32", (_p(verts12), _p(verts2), _p(idx11), _p(idx22), _p(pi_val), _p(pi_idx), B, N, M, k, topk, _p(out)),
             verts12.device, "map", "dvm_map_term_workspace_bytes", B, N)
    return out


def _frob_max_n(name):
    return int(getattr(_lib.load(), "dvm_%s_term_max_n" % name)())


def _frob_term(name, ptrs, dims, grad_of, grad):
    """The call of dvm_<name>_term_f32(*ptrs, *dims, loss, *gradients): loss (dims[0],) and, under grad, one gradient like each tensor
    of grad_of (NULL otherwise); `dims` are also the sizes of its workspace query -> loss, or (loss, *gradients) under grad."""
    dev = grad_of[0].device
    loss = _new(dev, dims[0])
    gs = [torch.empty_like(t) if grad else None for t in grad_of]
    _call_ws("dvm_%s_term_f32" % name, (*ptrs, *dims, _p(loss), *[_p(g) for g in gs]), dev, name, "dvm_%s_term_workspace_bytes" % name, *dims)
    return (loss, *gs) if grad else loss


def rank_term_max_n():
    """The largest N dvm_rank_term_f32 takes (a row of P P^T must fit LDS); models.loss.rank_term falls back to torch beyond it."""
    return _frob_max_n("rank")


def rank_term(pi_val, pi_idx, M, grad=False):
    """||P P^T - I_N||_F per batch element for the sparse top-k P (pi_val / pi_idx (B,N,k), M columns; indices in [0, M),
    distinct within a row) -> loss (B,), and with grad=True also g_val (B,N,k) = d loss[b] / d pi_val (0 where loss[b] == 0).
    dvm_rank_term_f32: row by row over the reversed column lists, no dense matrix, no float atomics.  Takes no part in autograd
    itself (nn_ops.rank_term is the node)."""
    _need_gpu(pi_val, pi_idx)
    pi_val, pi_idx = _f(pi_val), _i(pi_idx)
    B, N, topk = pi_val.shape
    if tuple(pi_idx.shape) != (B, N, topk):
        raise ValueError("rank_term: pi_idx must have pi_val's shape %s, got %s" % ((B, N, topk), tuple(pi_idx.shape)))
    return _frob_term("rank", (_p(pi_val), _p(pi_idx)), (B, N, int(M), topk), (pi_val,), grad)


def cycle_term_max_n():
    """The largest N dvm_cycle_term_f32 takes (a row of P12 P21 must fit LDS); models.loss.cycle_term falls back to torch beyond it."""
    return _frob_max_n("cycle")


def cycle_term(val12, idx12, val21, idx21, grad=False):
    """||P12 P21 - I_N||_F per batch element for the sparse top-k P12 (val12 / idx12 (B,N,k12), columns in [0, M)) and P21 (val21 /
    idx21 (B,M,k21), columns in [0, N)); indices distinct within a row -> loss (B,), and with grad=True also g12 (B,N,k12) =
    d loss[b] / d val12 and g21 (B,M,k21) = d loss[b] / d val21 (both 0 where loss[b] == 0).  dvm_cycle_term_f32: row by row, no
    dense matrix, no float atomics.  Takes no part in autograd itself (nn_ops.cycle_term is the node)."""
    _need_gpu(val12, idx12, val21, idx21)
    val12, idx12, val21, idx21 = _f(val12), _i(idx12), _f(val21), _i(idx21)
    if val12.dim() != 3 or val21.dim() != 3 or val12.shape[0] != val21.shape[0]:
        raise ValueError("cycle_term: val12 (B,N,k12) and val21 (B,M,k21) must share B, got %s and %s" % (tuple(val12.shape), tuple(val21.shape)))
    if idx12.shape != val12.shape or idx21.shape != val21.shape:
        raise ValueError("cycle_term: idx12 / idx21 must have the shapes of val12 / val21, %s / %s, got %s / %s"
                         % (tuple(val12.shape), tuple(val21.shape), tuple(idx12.shape), tuple(idx21.shape)))
    B, N, k12 = val12.shape
    M, k21 = val21.shape[1], val21.shape[2]
    return _frob_term("cycle", (_p(val12), _p(idx12), _p(val21), _p(idx21)), (B, N, M, k12, k21), (val12, val21), grad)


def distortion_term_max_n():
    """The largest N and M dvm_distortion_term_f32 takes (the rows it keeps must fit LDS); models.loss.distortion_term falls back to
    torch beyond it."""
    return _frob_max_n("distortion")


def distortion_term(val, idx, dist_src, dist_tgt, grad=False):
    """||P D2 P^T - D1||_F per batch element for the sparse top-k P (val / idx (B,N,k), columns in [0, M), distinct within a row),
    D1 = dist_src (B,N,N) and D2 = dist_tgt (B,M,M), both SYMMETRIC (not checked) -> loss (B,), and with grad=True also g_val
    (B,N,k) = d loss[b] / d val (0 where loss[b] == 0).  dvm_distortion_term_f32: row by row, no dense product, no float atomics.
    Takes no part in autograd itself (nn_ops.distortion_term is the node)."""
    _need_gpu(val, idx, dist_src, dist_tgt)
    val, idx, dist_src, dist_tgt = _f(val), _i(idx), _f(dist_src), _f(dist_tgt)
    if val.dim() != 3 or idx.shape != val.shape:
        raise ValueError("distortion_term: val and idx must share a shape (B,N,k), got %s and %s" % (tuple(val.shape), tuple(idx.shape)))
    B, N, topk = val.shape
    if dist_src.dim() != 3 or tuple(dist_src.shape) != (B, N, N):
        raise ValueError("distortion_term: dist_src must be %s, got %s" % ((B, N, N), tuple(dist_src.shape)))
    if dist_tgt.dim() != 3 or dist_tgt.shape[0] != B or dist_tgt.shape[1] != dist_tgt.shape[2]:
        raise ValueError("distortion_term: dist_tgt must be (%d,M,M), got %s" % (B, tuple(dist_tgt.shape)))
    M = dist_tgt.shape[1]
    return _frob_term("distortion", (_p(val), _p(idx), _p(dist_src), _p(dist_tgt)), (B, N, M, topk), (val,), grad)


class GraphOperator:
    """A weighted neighbour matrix of B source shapes in CSR (mesh_laplacian, knn_laplacian; the layout and the row order are in
    include/dvm.h): rowptr (B,N+1) int32, col (B,Ecap) int32, w (B,Ecap), norm (B,) = the energy of the shape's own coordinates,
    mass (B,N) or None, stats (B,4) int32 = entries' owners left out for an index out of range, for degenerate geometry, self
    entries, entries kept.  Constants: no gradient flows into them."""
    __slots__ = ("rowptr", "col", "w", "norm", "mass", "stats")

    def __init__(self, rowptr, col, w, norm, mass, stats):
        self.rowptr, self.col, self.w, self.norm, self.mass, self.stats = rowptr, col, w, norm, mass, stats

    @property
    def N(self):
        return self.rowptr.shape[1] - 1

    @property
    def Ecap(self):
        return self.col.shape[1]


LAPLACIAN_MODES = {"stretch": 0, "uniform": 1}


def mesh_laplacian(verts, faces):
    """The cotangent operator of the triangle meshes (verts (B,N,3), faces (F,3) shared by the batch) -> GraphOperator with
    Ecap = 6 F, mass = one third of the incident face areas, norm = 2 x the total area.  Faces with an index outside [0,N) or a
    degenerate corner are left out and counted in stats (never read back here: no synchronisation).  dvm_mesh_laplacian_f32."""
    _need_gpu(verts, faces)
    verts, faces = _f(verts), _i(faces)
    if verts.dim() != 3 or verts.shape[2] != 3 or faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError("mesh_laplacian: verts must be (B,N,3) and faces (F,3), got %s and %s" % (tuple(verts.shape), tuple(faces.shape)))
    B, N, _ = verts.shape
    F = faces.shape[0]
    dev = verts.device
    op = GraphOperator(_new(dev, B, N + 1, dtype=torch.int32), _new(dev, B, 6 * F, dtype=torch.int32), _new(dev, B, 6 * F), _new(dev, B),
                       _new(dev, B, N), _new(dev, B, 4, dtype=torch.int32))
    _call_ws("dvm_mesh_laplacian_f32", (_p(verts), _p(faces), B, N, F, _p(op.rowptr), _p(op.col), _p(op.w), _p(op.norm), _p(op.mass),
                                        _p(op.stats)), dev, "laplacian", "dvm_mesh_laplacian_workspace_bytes", B, N, F)
    return op


def knn_laplacian(xyz, nbr, mode="stretch"):
    """The operator W + W^T of a neighbour list (xyz (B,N,3), nbr (B,N,K) as knn_cdist returns it, self included) -> GraphOperator
    with Ecap = 2 N K, mass None.  mode "stretch": w = 1 / |x_i - x_j|^2, norm = half the kept entries; "uniform": w = 1,
    norm = 1/2 sum w |x_i - x_j|^2.  Self entries, indices outside [0,N) and (stretch) zero distances are left out and counted.
    dvm_knn_laplacian_f32."""
    if mode not in LAPLACIAN_MODES:
        raise ValueError("knn_laplacian: mode must be 'stretch' or 'uniform', got %r" % (mode,))
    _need_gpu(xyz, nbr)
    xyz, nbr = _f(xyz), _i(nbr)
    if xyz.dim() != 3 or xyz.shape[2] != 3 or nbr.dim() != 3 or tuple(nbr.shape[:2]) != tuple(xyz.shape[:2]):
        raise ValueError("knn_laplacian: xyz must be (B,N,3) and nbr (B,N,K), got %s and %s" % (tuple(xyz.shape), tuple(nbr.shape)))
    B, N, K = nbr.shape
    dev = xyz.device
    E = 2 * N * K
    op = GraphOperator(_new(dev, B, N + 1, dtype=torch.int32), _new(dev, B, E, dtype=torch.int32), _new(dev, B, E), _new(dev, B), None,
                       _new(dev, B, 4, dtype=torch.int32))
    m = LAPLACIAN_MODES[mode]
    _call_ws("dvm_knn_laplacian_f32", (_p(xyz), _p(nbr), B, N, K, m, _p(op.rowptr), _p(op.col), _p(op.w), _p(op.norm), _p(op.stats)), dev,
             "laplacian", "dvm_knn_laplacian_workspace_bytes", B, N, K, m)
    return op


def dirichlet_term_takes(B, N, M, k, C, Ecap):
    """Whether dvm_dirichlet_term_f32 takes these sizes (its workspace query answers 0 exactly when it refuses).  No device is needed."""
    return int(_lib.load().dvm_dirichlet_term_workspace_bytes(B, N, M, k, C, Ecap)) > 0


def dirichlet_term(val, idx, V, op, grad=False):
    """The Dirichlet energy E = 1/2 sum_entries w |y_i - y_j|^2 of Y = Pi V per batch element, for the sparse Pi (val / idx (B,N,k),
    columns in [0, M)), the target's values V (B,M,C), C <= 16, and the source's GraphOperator op -> loss (B,), and with grad=True
    also g_val (B,N,k) = d loss[b] / d val.  V and op are constants.  dvm_dirichlet_term_f32: Y has ops.apply's bits, the rest is
    float64 in CSR order, no float atomics.  Takes no part in autograd itself (nn_ops.dirichlet_term is the node)."""
    _need_gpu(val, idx, V, op.rowptr, op.col, op.w)
    val, idx, V = _f(val), _i(idx), _f(V)
    rowptr, col, w = _i(op.rowptr), _i(op.col), _f(op.w)
    if val.dim() != 3 or idx.shape != val.shape:
        raise ValueError("dirichlet_term: val and idx must share a shape (B,N,k), got %s and %s" % (tuple(val.shape), tuple(idx.shape)))
    B, N, topk = val.shape
    if V.dim() != 3 or V.shape[0] != B:
        raise ValueError("dirichlet_term: V must be (%d,M,C), got %s" % (B, tuple(V.shape)))
    if tuple(rowptr.shape) != (B, N + 1) or col.dim() != 2 or col.shape[0] != B or col.shape != w.shape:
        raise ValueError("dirichlet_term: the operator must have rowptr %s and col / w (%d,Ecap), got %s, %s, %s"
                         % ((B, N + 1), B, tuple(rowptr.shape), tuple(col.shape), tuple(w.shape)))
    M, C = V.shape[1], V.shape[2]
    return _frob_term("dirichlet", (_p(val), _p(idx), _p(V), _p(rowptr), _p(col), _p(w)), (B, N, M, topk, C, col.shape[1]), (val,), grad)


class Eigenbasis:
    """The result of eigenbasis: evals (B,k) ascending, evecs (B,N,k) with Phi^T M Phi = I (rows of inactive vertices 0, every
    column's largest entry positive), res (B,k) = |A y - theta y| / beta of the returned pairs — all float64 — info (B,4) int32 =
    outer iterations, converged, inactive vertices, operator applications, and mass (B,N) fp32 or None as given."""
    __slots__ = ("evals", "evecs", "res", "info", "mass")

    def __init__(self, evals, evecs, res, info, mass):
        self.evals, self.evecs, self.res, self.info, self.mass = evals, evecs, res, info, mass

    @property
    def k(self):
        return self.evals.shape[1]


def eigenbasis_max_block():
    """The widest block k + guard dvm_eigenbasis_f64 takes (one m x m float64 matrix stays in LDS)."""
    return int(_lib.load().dvm_eigenbasis_max_block())


def eigenbasis(op, k, guard=None, degree=20, max_iter=200, tol=1e-10):
    """The first k eigenpairs of L phi = lambda M phi for the GraphOperator op (M = diag(op.mass), or I without a mass) by
    Chebyshev-filtered subspace iteration on a block of k + guard columns -> Eigenbasis (the definition is in include/dvm.h).
    guard defaults to max(8, k // 4), clipped to the entry's limits.  The call waits for its stream (it reads the convergence
    flags back once per outer iteration) and raises DvmError when the entry fails; a basis that has not converged within max_iter
    is RETURNED with info[:, 1] == 0 and truthful res: the caller decides.  dvm_eigenbasis_f64."""
    _need_gpu(op.rowptr, op.col, op.w, op.mass)
    rowptr, col, w = _i(op.rowptr), _i(op.col), _f(op.w)
    mass = None if op.mass is None else _f(op.mass)
    if rowptr.dim() != 2 or col.dim() != 2 or col.shape != w.shape or col.shape[0] != rowptr.shape[0]:
        raise ValueError("eigenbasis: the operator must have rowptr (B,N+1) and col / w (B,Ecap), got %s, %s, %s"
                         % (tuple(rowptr.shape), tuple(col.shape), tuple(w.shape)))
    B, N, Ecap = rowptr.shape[0], rowptr.shape[1] - 1, col.shape[1]
    if mass is not None and tuple(mass.shape) != (B, N):
        raise ValueError("eigenbasis: mass must be %s, got %s" % ((B, N), tuple(mass.shape)))
    k = int(k)
    if guard is None:
        guard = max(1, min(max(8, k // 4), min(N, eigenbasis_max_block()) - k))
    guard = int(guard)
    dev = rowptr.device
    f64 = torch.float64
    out = Eigenbasis(_new(dev, B, max(k, 0), dtype=f64), _new(dev, B, N, max(k, 0), dtype=f64), _new(dev, B, max(k, 0), dtype=f64),
                     _new(dev, B, 4, dtype=torch.int32), op.mass)
    _call_ws("dvm_eigenbasis_f64", (_p(rowptr), _p(col), _p(w), _p(mass), B, N, Ecap, k, guard, int(degree), int(max_iter), float(tol),
                                    _p(out.evals), _p(out.evecs), _p(out.res), _p(out.info)), dev, "eigenbasis",
             "dvm_eigenbasis_workspace_bytes", B, N, Ecap, k, guard)
    return out


def mesh_eigenbasis(verts, faces, k, **kw):
    """mesh_laplacian followed by eigenbasis: the Laplace-Beltrami basis of the triangle meshes (verts (B,N,3), faces (F,3))."""
    return eigenbasis(mesh_laplacian(verts, faces), k, **kw)


def basis_project(evecs, mass, Y):
    """Phi^T diag(mass) Y per batch element: evecs (B,N,k) float64, mass (B,N) fp32 or None (1), Y (B,N,C) fp32 -> (B,k,C) float64,
    k, C <= 128; summed in a fixed order, no synchronisation.  dvm_basis_project_f64."""
    _need_gpu(evecs, mass, Y)
    evecs, Y = evecs.detach().contiguous().double(), _f(Y)
    mass = None if mass is None else _f(mass)
    if evecs.dim() != 3 or Y.dim() != 3 or tuple(Y.shape[:2]) != tuple(evecs.shape[:2]):
        raise ValueError("basis_project: evecs must be (B,N,k) and Y (B,N,C), got %s and %s" % (tuple(evecs.shape), tuple(Y.shape)))
    B, N, k = evecs.shape
    C = Y.shape[2]
    if mass is not None and tuple(mass.shape) != (B, N):
        raise ValueError("basis_project: mass must be %s, got %s" % ((B, N), tuple(mass.shape)))
    out = _new(evecs.device, B, k, C, dtype=torch.float64)
    _call_ws("dvm_basis_project_f64", (_p(evecs), _p(mass), _p(Y), B, N, k, C, _p(out)), evecs.device, "basis_project",
             "dvm_basis_project_workspace_bytes", B, N, k, C)
    return out


_FMAP_MODES = {"adjoint": 0, "lstsq": 1}


def _f64(t):
    """A contiguous float64 tensor without autograd history (the same object when it already is one)."""
    if t.dtype is torch.float64 and not t.requires_grad and t.is_contiguous():
        return t
    return t.detach().contiguous().double()


def _fmap_mode(solve, who):
    if solve not in _FMAP_MODES:
        raise ValueError("%s: solve must be 'adjoint' or 'lstsq', got %r" % (who, solve))
    return _FMAP_MODES[solve]


def _basis_pair(phi_src, phi_tgt, who):
    """The two bases as contiguous float64 (B,N,K1) / (B,M,K2): a truncation to k columns is the same buffer with its row stride."""
    phi_src, phi_tgt = _f64(phi_src), _f64(phi_tgt)
    if phi_src.dim() != 3 or phi_tgt.dim() != 3 or phi_src.shape[0] != phi_tgt.shape[0]:
        raise ValueError("%s: the bases must be (B,N,K) and (B,M,K), got %s and %s" % (who, tuple(phi_src.shape), tuple(phi_tgt.shape)))
    return phi_src, phi_tgt


def _ws_arg(lib, size_query, size_args, dev, tag, workspace_buf):
    """(buffer, bytes) of an entry's workspace: the caller's own buffer (a capture must not allocate) or the cached one."""
    nb = getattr(lib, size_query)(*size_args)
    ws = workspace(nb, dev, tag) if workspace_buf is None else workspace_buf
    return ws, (nb if workspace_buf is None else workspace_buf.numel())


def spectral_nn_plan(B, N, M, k):
    """How dvm_spectral_nn_f64 tiles a search: dict(tile_n, tile_m, segments, seg_len) — source rows per workgroup, target rows per
    tile, the number of target segments and their length.  The result of a search does not depend on it."""
    plan = (ctypes.c_int32 * 4)()
    check(_lib.load().dvm_spectral_nn_plan(int(B), int(N), int(M), int(k), plan), "dvm_spectral_nn_plan")
    return dict(tile_n=plan[0], tile_m=plan[1], segments=plan[2], seg_len=plan[3])


def spectral_nn(A, E, k=None, want_dist=False):
    """T (B,N) int32 = argmin_j |E[j,:k] - A[i,:k]|^2 in float64, every pair in the exact sequential form (sub, mul, add rounded
    separately, coordinates ascending), ties to the lowest j, NaN distances never win; with want_dist also the winning distances
    (B,N) float64.  A (B,N,K1), E (B,M,K2) float64; k defaults to min(K1, K2) and is at most 128.  dvm_spectral_nn_f64."""
    _need_gpu(A, E)
    A, E = _basis_pair(A, E, "spectral_nn")
    B, N, M = A.shape[0], A.shape[1], E.shape[1]
    k = min(A.shape[2], E.shape[2]) if k is None else int(k)
    T = _new(A.device, B, N, dtype=torch.int32)
    dmin = _new(A.device, B, N, dtype=torch.float64) if want_dist else None
    _call_ws("dvm_spectral_nn_f64", (_p(A), A.shape[2], _p(E), E.shape[2], B, N, M, k, _p(T), _p(dmin)), A.device, "spectral_nn",
             "dvm_spectral_nn_workspace_bytes", B, N, M, k)
    return (T, dmin) if want_dist else T


def fmap_from_pmap(phi_src, mass_src, phi_tgt, T, k=None, solve="adjoint", want_info=False):
    """The functional map of a point map T (B,N) int32 into the target: C (B,k,k) float64 with phi_src[:, :k] C ~ phi_tgt[T, :k].
    solve="adjoint": C = phi_src[:, :k]^T diag(mass_src) phi_tgt[T, :k] (mass_src (B,N) fp32 or None for 1), the weighted
    least-squares solution for a mass-orthonormal basis; solve="lstsq": pinv(phi_src[:, :k]) phi_tgt[T, :k] by Cholesky on the normal
    equations (the reference's pMap2fMap; mass_src is not used).  An entry of T outside [0, M) adds nothing.  want_info also returns
    info (B,4) int32 = status (1: a Cholesky pivot was not positive and finite, C is NaN), that k, the entries of T outside
    [0, M), 0.  No synchronisation.  dvm_fmap_from_pmap_f64."""
    _need_gpu(phi_src, mass_src, phi_tgt, T)
    mode = _fmap_mode(solve, "fmap_from_pmap")
    phi_src, phi_tgt = _basis_pair(phi_src, phi_tgt, "fmap_from_pmap")
    T = _i(T)
    mass = None if mass_src is None else _f(mass_src)
    B, N, M = phi_src.shape[0], phi_src.shape[1], phi_tgt.shape[1]
    if tuple(T.shape) != (B, N) or (mass is not None and tuple(mass.shape) != (B, N)):
        raise ValueError("fmap_from_pmap: T and mass_src must be %s, got %s and %s"
                         % ((B, N), tuple(T.shape), None if mass is None else tuple(mass.shape)))
    k = min(phi_src.shape[2], phi_tgt.shape[2]) if k is None else int(k)
    C = _new(phi_src.device, B, max(k, 0), max(k, 0), dtype=torch.float64)
    info = _new(phi_src.device, B, 4, dtype=torch.int32)
    _call_ws("dvm_fmap_from_pmap_f64", (_p(phi_src), phi_src.shape[2], _p(mass), _p(phi_tgt), phi_tgt.shape[2], _p(T), B, N, M, k, mode,
                                        _p(C), _p(info)), phi_src.device, "fmap_from_pmap", "dvm_fmap_from_pmap_workspace_bytes", B, N, M, k, mode)
    return (C, info) if want_info else C


def fmap_embed(phi_tgt, C):
    """E (B,M,k) float64 = phi_tgt[:, :k] C^T for C (B,k,k): the target's vertices in the source's spectral coordinates (what the
    nearest-neighbour search of fmap_to_pmap runs against).  dvm_fmap_embed_f64."""
    _need_gpu(phi_tgt, C)
    phi_tgt, C = _f64(phi_tgt), _f64(C)
    if phi_tgt.dim() != 3 or C.dim() != 3 or C.shape[0] != phi_tgt.shape[0] or C.shape[1] != C.shape[2]:
        raise ValueError("fmap_embed: phi_tgt must be (B,M,K) and C (B,k,k), got %s and %s" % (tuple(phi_tgt.shape), tuple(C.shape)))
    B, M, k = phi_tgt.shape[0], phi_tgt.shape[1], C.shape[1]
    E = _new(phi_tgt.device, B, M, k, dtype=torch.float64)
    _call("dvm_fmap_embed_f64", _p(phi_tgt), phi_tgt.shape[2], _p(C), B, M, k, _p(E), k)
    return E


def fmap_to_pmap(phi_src, phi_tgt, C, want_dist=False, want_embedding=False):
    """The point map of a functional map C (B,k,k): T (B,N) int32, T[i] = the target vertex whose embedded row (fmap_embed) is
    nearest to phi_src[i, :k] (spectral_nn; the reference's fMap2pMap).  Returns T, then the winning squared distances (B,N)
    with want_dist, then the embedding (B,M,k) with want_embedding.  No synchronisation.  dvm_fmap_to_pmap_f64."""
    _need_gpu(phi_src, phi_tgt, C)
    phi_src, phi_tgt = _basis_pair(phi_src, phi_tgt, "fmap_to_pmap")
    C = _f64(C)
    if C.dim() != 3 or C.shape[0] != phi_src.shape[0] or C.shape[1] != C.shape[2]:
        raise ValueError("fmap_to_pmap: C must be (%d,k,k), got %s" % (phi_src.shape[0], tuple(C.shape)))
    B, N, M, k = phi_src.shape[0], phi_src.shape[1], phi_tgt.shape[1], C.shape[1]
    dev = phi_src.device
    T = _new(dev, B, N, dtype=torch.int32)
    dmin = _new(dev, B, N, dtype=torch.float64) if want_dist else None
    E = _new(dev, B, M, k, dtype=torch.float64) if want_embedding else None
    _call_ws("dvm_fmap_to_pmap_f64", (_p(phi_src), phi_src.shape[2], _p(phi_tgt), phi_tgt.shape[2], _p(C), B, N, M, k, _p(T), _p(dmin), _p(E)),
             dev, "fmap_to_pmap", "dvm_fmap_to_pmap_workspace_bytes", B, N, M, k)
    out = (T,) + ((dmin,) if want_dist else ()) + ((E,) if want_embedding else ())
    return out if len(out) > 1 else T


class ZoomOut:
    """The result of zoomout: C (B,k_final,k_final) float64, T (B,N) int32 — the map that produced C — and info (B,4) int32 =
    status (0 ok, 1 a Cholesky pivot that was not positive and finite), the k at which it failed, the entries of T0 outside
    [0, M), the nearest-neighbour steps run.  Unpacks as (C, T, info)."""
    __slots__ = ("C", "T", "info")

    def __init__(self, C, T, info):
        self.C, self.T, self.info = C, T, info

    def __iter__(self):
        return iter((self.C, self.T, self.info))


def zoomout_workspace_bytes(B, N, M, k_init, k_final, k_step=1, n_inter=1, solve="adjoint"):
    """The bytes of scratch zoomout takes for these sizes (0 outside the entry's limits): for a caller that brings its own."""
    return int(_lib.load().dvm_zoomout_workspace_bytes(int(B), int(N), int(M), int(k_init), int(k_final), int(k_step), int(n_inter),
                                                       _fmap_mode(solve, "zoomout")))


def zoomout(phi_src, mass_src, phi_tgt, T0, k_init, k_final, k_step=1, n_inter=1, solve="adjoint", check=True, workspace_buf=None):
    """ZoomOut spectral refinement of a point map T0 (B,N) int32 (the reference's zo_fmap): for k = k_init, k_init + k_step, ..
    below k_final, n_inter times { C = fmap_from_pmap(T, k); T = fmap_to_pmap(C) }, then C = fmap_from_pmap(T, k_final) -> ZoomOut
    (C, T, info), bit for bit what those calls give in that order.  The bases are (B,N,K) / (B,M,K) float64 with K >= k_final
    (ops.eigenbasis' evecs); mass_src (B,N) fp32 or None.  The entry only enqueues launches (capturable with check=False and a
    workspace_buf of zoomout_workspace_bytes bytes).  check=True reads info back (one synchronisation) and raises DvmError when an
    element's Cholesky failed (solve="lstsq" on a rank-deficient basis); with check=False such an element returns NaN in C, its
    last T and info[:, 0] == 1.  dvm_zoomout_f64."""
    _need_gpu(phi_src, mass_src, phi_tgt, T0, workspace_buf)
    mode = _fmap_mode(solve, "zoomout")
    phi_src, phi_tgt = _basis_pair(phi_src, phi_tgt, "zoomout")
    T0 = _i(T0)
    mass = None if mass_src is None else _f(mass_src)
    B, N, M = phi_src.shape[0], phi_src.shape[1], phi_tgt.shape[1]
    if tuple(T0.shape) != (B, N) or (mass is not None and tuple(mass.shape) != (B, N)):
        raise ValueError("zoomout: T0 and mass_src must be %s, got %s and %s"
                         % ((B, N), tuple(T0.shape), None if mass is None else tuple(mass.shape)))
    k_init, k_final, k_step, n_inter = int(k_init), int(k_final), int(k_step), int(n_inter)
    dev = phi_src.device
    out = ZoomOut(_new(dev, B, max(k_final, 0), max(k_final, 0), dtype=torch.float64), _new(dev, B, N, dtype=torch.int32),
                  _new(dev, B, 4, dtype=torch.int32))
    lib = _lib.load()
    ws, nb = _ws_arg(lib, "dvm_zoomout_workspace_bytes", (B, N, M, k_init, k_final, k_step, n_inter, mode), dev, "zoomout", workspace_buf)
    _lib.check(lib.dvm_zoomout_f64(_p(phi_src), phi_src.shape[2], _p(mass), _p(phi_tgt), phi_tgt.shape[2], _p(T0), B, N, M, k_init, k_final,
                                   k_step, n_inter, mode, _p(out.C), _p(out.T), _p(out.info), _p(ws), nb, _stream()), "dvm_zoomout_f64")
    if check:
        bad = out.info[:, 0].nonzero().flatten().tolist()
        if bad:
            raise DvmError("zoomout: a Cholesky pivot of Phi^T Phi was not positive and finite in element(s) %s at k = %s: the truncated "
                           "source basis is rank-deficient" % (bad, [int(out.info[b, 1]) for b in bad]))
    return out


def _pair_out(B, n, dev):
    """One direction's outputs of the pair calls: dict(warped, verts12, T12, losses[B,6])."""
    return dict(warped=_new(dev, B, n, 3), verts12=_new(dev, B, n, 3), T12=_new(dev, B, n, dtype=torch.int32), losses=_new(dev, B, 6))


def _pair_out_ptrs(o):
    return _p(o["warped"]), _p(o["verts12"]), _p(o["T12"]), _p(o["losses"])


def pair_direction(wl, feat1, feat2, verts1, verts2, alpha, fps_start, with_map=True, out=None):
    """Config-2 path for B pairs, one direction. Returns dict(warped, verts12, T12, losses[B,6])."""
    _need_gpu(feat1, feat2, verts1, verts2, fps_start, *wl)
    feat1, feat2, verts1, verts2, fps_start = _f(feat1), _f(feat2), _f(verts1), _f(verts2), _i(fps_start)
    B, N, _ = feat1.shape
    M = feat2.shape[1]
    dev = feat1.device
    if out is None:
        out = _pair_out(B, N, dev)
    _call_ws("dvm_pair_direction_fwd_f32", (_p(feat1), _p(feat2), _p(verts1), _p(verts2), B, N, M, neg_alpha_f32(alpha), _p(fps_start),
                                            *[_p(w) for w in wl], int(with_map), *_pair_out_ptrs(out)),
             dev, "pair", "dvm_pair_direction_workspace_bytes", B, N, M)
    return out


def knn_neg(a, b, k):
    """knn_new / knn: a (B,N,C), b (B,M,C) -> idx (B,N,k) int32, nearest (largest score) first."""
    _need_gpu(a, b)
    a, b = _f(a), _f(b)
    B, N, C = a.shape
    M = b.shape[1]
    idx = _new(a.device, B, N, k, dtype=torch.int32)
    _call_ws("dvm_knn_neg_f32", (_p(a), _p(b), B, N, M, C, k, _p(idx)), a.device, "knn_neg", "dvm_knn_neg_workspace_bytes", B, N, M, C, k)
    return idx


def softcorr_dense(f1, f2, alpha):
    _need_gpu(f1, f2)
    f1, f2 = _f(f1), _f(f2)
    B, N, d = f1.shape
    M = f2.shape[1]
    P = _new(f1.device, B, N, M)
    _call_ws("dvm_softcorr_dense_f32", (_p(f1), _p(f2), B, N, M, d, neg_alpha_f32(alpha), _p(P)),
             f1.device, "softcorr_dense", "dvm_softcorr_dense_workspace_bytes", B, N, M, d)
    return P


def deformer_mlp(wl, z):
    """z (..., 262) -> (..., 9) with the Deformer's decoder weights wl (deformer_weight_list)."""
    _need_gpu(z, *wl)
    z = _f(z)
    rows = z.numel() // 262
    out = _new(z.device, *z.shape[:-1], 9)
    _call_ws("dvm_deformer_mlp_fwd_f32", (_p(z), rows, *[_p(w) for w in wl[2:]], _p(out)), z.device, "mlp", "dvm_deformer_mlp_workspace_bytes", rows)
    return out


def pos_encoding(x, minmax=None):
    """x (B,3,N) -> (B,384,N).  minmax: optional device tensor (min, max) replacing the tensor's own range."""
    _need_gpu(x)
    x = _f(x)
    B, _, N = x.shape
    out = _new(x.device, B, 384, N)
    if minmax is not None:
        _need_gpu(minmax)
        mm = _f(minmax).reshape(2)
        _call("dvm_pos_encoding_minmax_f32", _p(x), _p(mm), B, N, _p(out))
    else:
        _call_ws("dvm_pos_encoding_f32", (_p(x), B, N, _p(out)), x.device, "posenc", "dvm_pos_encoding_workspace_bytes")
    return out


def bn_act_train_fwd(x, res, gamma, beta, eps, slope, momentum, running_mean=None, running_var=None):
    """Training-mode BatchNorm over (B,C,N) of x (+ res) with the activation fused -> (y, save_mean, save_invstd);
    running_mean / running_var (device tensors) are updated in place."""
    _need_gpu(x)
    x = _f(x)
    res = None if res is None else _f(res)
    gamma = None if gamma is None else _f(gamma)
    beta = None if beta is None else _f(beta)
    B, C, N = x.shape
    y = torch.empty_like(x)
    mean, invstd = _new(x.device, C), _new(x.device, C)
    if running_mean is not None:
        assert running_mean.is_contiguous() and running_var.is_contiguous() and running_mean.dtype == torch.float32
    _call_ws("dvm_bn_act_train_fwd_f32", (_p(x), _p(res), _p(gamma), _p(beta), B, C, N, float(eps), float(slope), float(momentum), _p(y),
                                          _p(mean), _p(invstd), _p(running_mean), _p(running_var)),
             x.device, "bn", "dvm_bn_workspace_bytes", B, C, N)
    return y, mean, invstd


def bn_act_train_bwd(dy, y, x, res, gamma, mean, invstd, slope):
    """-> (dx (also the gradient of res), dgamma, dbeta)."""
    _need_gpu(dy, y, x)
    dy, y, x = _f(dy), _f(y), _f(x)
    res = None if res is None else _f(res)
    gamma = None if gamma is None else _f(gamma)
    B, C, N = x.shape
    dx = torch.empty_like(x)
    dgamma, dbeta = _new(x.device, C), _new(x.device, C)
    _call_ws("dvm_bn_act_train_bwd_f32", (_p(dy), _p(y), _p(x), _p(res), _p(gamma), _p(mean), _p(invstd), B, C, N, float(slope), _p(dx),
                                          _p(dgamma), _p(dbeta)), x.device, "bn", "dvm_bn_workspace_bytes", B, C, N)
    return dx, dgamma, dbeta


def graph_geodesics(nbr, w):
    """nbr (N,K) int32 neighbour lists (-1 padded), w (N,K) float64 edge lengths, on the device -> (N,N) float64."""
    _need_gpu(nbr, w)
    nbr, w = nbr.contiguous().int(), w.contiguous().double()
    N, K = nbr.shape
    D = _new(nbr.device, N, N, dtype=torch.float64)
    _call("dvm_graph_geodesics_f64", _p(nbr), _p(w), N, K, _p(D))
    return D


def mesh_geodesics_max_v():
    """The largest vertex count dvm_mesh_geodesics_f64 takes (a source's V distances stay in LDS)."""
    return int(_lib.load().dvm_mesh_geodesics_max_v())


def mesh_geodesics(verts, faces, sources=None):
    """Geodesic distances on a triangle mesh by the triangle-front (fast-marching) update, dvm_mesh_geodesics_f64: verts (V,3),
    faces (F,3) on the device, sources (S,) vertex ids or None = every vertex -> (S or V, V) float64, row r = distances from
    source r (+inf between components).  Asymmetric at the 0.5 % level; never above the edge-path distance.  The call waits for
    its own result (the entry reports bad indices as its return value)."""
    _need_gpu(verts, faces, sources)
    verts, faces = verts.detach().contiguous().double(), _i(faces)
    if verts.dim() != 2 or verts.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError("mesh_geodesics: verts must be (V,3) and faces (F,3), got %s and %s" % (tuple(verts.shape), tuple(faces.shape)))
    V, F = verts.shape[0], faces.shape[0]
    S = 0
    if sources is not None:
        sources = _i(sources).reshape(-1)
        S = sources.numel()
        if S < 1:
            raise ValueError("mesh_geodesics: an empty list of sources (pass None for every vertex)")
    D = _new(verts.device, S if sources is not None else V, V, dtype=torch.float64)
    _call_ws("dvm_mesh_geodesics_f64", (_p(verts), _p(faces), V, F, _p(sources), S, _p(D)), verts.device, "mesh_geo",
             "dvm_mesh_geodesics_workspace_bytes", V, F)
    return D


def proj2img(pts):
    """One view's point cloud (B,N,3) -> (img (B,3,224,224), pc_min (B,2), grid_size (B,), offsets (B,2))."""
    _need_gpu(pts)
    pts = _f(pts)
    B, N, _ = pts.shape
    dev = pts.device
    img = _new(dev, B, 3, 224, 224)
    pc_min, grid, off = _new(dev, B, 2), _new(dev, B), _new(dev, B, 2)
    _call_ws("dvm_proj2img_f32", (_p(pts), B, N, _p(img), _p(pc_min), _p(grid), _p(off)), dev, "proj2img", "dvm_proj2img_workspace_bytes", B)
    return img, pc_min, grid, off


def i2p(pts, f, pc_min, grid, offsets, normalize=False, out=None, col=0):
    """Image features f (B,C,H,W) sampled at every point's pixel: (B,N,C), or columns [col, col+C) of `out` (B,N,ldo)."""
    _need_gpu(pts, f, pc_min, grid, offsets)
    pts, f, pc_min, grid, offsets = _f(pts), _f(f), _f(pc_min), _f(grid), _f(offsets)
    B, N, _ = pts.shape
    C, H, W = f.shape[1:]
    if out is None:
        out, col = _new(pts.device, B, N, C), 0
    assert out.is_contiguous() and out.dtype == torch.float32 and out.shape[:2] == (B, N) and col + C <= out.shape[2]
    _call("dvm_i2p_f32", _p(pts), _p(f), _p(pc_min), _p(grid), _p(offsets), B, N, C, H, W, int(bool(normalize)),
          ctypes.c_void_p(out.data_ptr() + 4 * col), out.shape[2])
    return out


def adaptive_conv(x_padded, kernel, tap_major=False):
    """FeatUp's AdaptiveConv: x_padded (B,C,H+d-1,W+d-1), kernel (B,H,W,d,d) — or (B,d*d,H,W) with tap_major — -> (B,C,H,W)."""
    _need_gpu(x_padded, kernel)
    x_padded, kernel = _f(x_padded), _f(kernel)
    B, C, Hp, Wp = x_padded.shape
    if tap_major:
        _, d2, H, W = kernel.shape
        d = int(round(d2 ** 0.5))
        ok = d * d == d2
    else:
        _, H, W, d, dd = kernel.shape
        ok = d == dd
    if not ok or Hp != H + d - 1 or Wp != W + d - 1 or kernel.shape[0] != B:
        raise DvmError("adaptive_conv: shapes %s and %s do not match" % (tuple(x_padded.shape), tuple(kernel.shape)))
    out = _new(x_padded.device, B, C, H, W)
    _call("dvm_adaptive_conv_f32", _p(x_padded), _p(kernel), B, C, H, W, d, 1 if tap_major else 0, _p(out))
    return out


def bicubic_resize_pad(x, size, pad=0):
    """F.pad(F.interpolate(x, size, mode='bicubic', align_corners=False), [pad]*4, mode='reflect') in one kernel:
    x (B,C,Hi,Wi) -> (B,C,Ho+2pad,Wo+2pad)."""
    _need_gpu(x)
    x = _f(x)
    B, C, Hi, Wi = x.shape
    Ho, Wo = size
    out = _new(x.device, B, C, Ho + 2 * pad, Wo + 2 * pad)
    _call("dvm_bicubic_resize_pad_f32", _p(x), B * C, Hi, Wi, Ho, Wo, pad, _p(out))
    return out


def jbu_kernel(proj, range_temp, sigma_spatial, d=7):
    """Normalised range x spatial kernel of a joint-bilateral stage: proj (B,32,H,W) -> (B,d*d,H,W) (dvm_jbu_kernel_f32)."""
    _need_gpu(proj, range_temp, sigma_spatial)
    proj = _f(proj)
    B, Kd, H, W = proj.shape
    out = _new(proj.device, B, d * d, H, W)
    _call("dvm_jbu_kernel_f32", _p(proj), _p(_f(range_temp)), _p(_f(sigma_spatial)), B, Kd, H, W, d, _p(out))
    return out


def sa_attention_pm(p, v):
    """point-major p (B,N,16), v (B,N,64) -> x_r (B,N,64)."""
    _need_gpu(p, v)
    p, v = _f(p), _f(v)
    B, N, _ = p.shape
    xr = _new(p.device, B, N, 64)
    _call_ws("dvm_sa_attention_fwd_f32", (_p(p), _p(v), B, N, _p(xr)), p.device, "sa", "dvm_sa_attention_workspace_bytes", B, N)
    return xr


def sa_attention_train_fwd(p, v):
    """-> xr (B,N,64), stats (B,N,2), cinv (B,N)."""
    _need_gpu(p, v)
    p, v = _f(p), _f(v)
    B, N, _ = p.shape
    dev = p.device
    xr, stats, cinv = _new(dev, B, N, 64), _new(dev, B, N, 2), _new(dev, B, N)
    _call_ws("dvm_sa_attention_train_fwd_f32", (_p(p), _p(v), B, N, _p(xr), _p(stats), _p(cinv)),
             dev, "sa_train", "dvm_sa_attention_train_fwd_workspace_bytes", B, N, null_if_empty=True)
    return xr, stats, cinv


def sa_attention_bwd(p, v, xr, stats, cinv, gxr):
    """-> d_p (B,N,16), d_v (B,N,64)."""
    _need_gpu(p, v, gxr)
    p, v, gxr = _f(p), _f(v), _f(gxr)
    B, N, _ = p.shape
    dp, dv = torch.empty_like(p), torch.empty_like(v)
    _call_ws("dvm_sa_attention_bwd_f32", (_p(p), _p(v), _p(xr), _p(stats), _p(cinv), _p(gxr), B, N, _p(dp), _p(dv)),
             p.device, "sa_bwd", "dvm_sa_attention_bwd_workspace_bytes", B, N)
    return dp, dv


def sa_attention(x, w_qk, w_v, b_v):
    """x (B,64,N) channel-major like the reference; returns x_r (B,64,N)."""
    xt = x.transpose(1, 2).contiguous()
    return sa_attention_pm(linear(xt, w_qk), linear(xt, w_v, bias=b_v)).transpose(1, 2)


def n2p_attention_pm(q, kp, vp, idx, heads=4):
    _need_gpu(q, kp, vp, idx)
    q, kp, vp, idx = _f(q), _f(kp), _f(vp), _i(idx)
    B, N, C = q.shape
    K = idx.shape[2]
    out = _new(q.device, B, N, C)
    _call("dvm_n2p_attention_fwd_f32", _p(q), _p(kp), _p(vp), _p(idx), B, N, C, K, heads, _p(out))
    return out


def n2p_attention(x, K, wq, wk, wv, heads=4):
    """x (B,C,N) channel-major like the reference; returns the attention output (B,C,N)."""
    C = x.shape[1]
    xt = x.transpose(1, 2).contiguous()
    idx = knn_neg(xt, xt, K)
    w = torch.cat([wq.reshape(C, C), wk.reshape(C, C), wv.reshape(C, C)], 0)
    qkv = linear(xt, w)
    out = n2p_attention_pm(qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:], idx, heads)
    return out.transpose(1, 2)


def dist_loss(feat, dist, anchors, k, want_idx=False):
    """feat (B,N,C), dist (B,N,N), anchors (nA,) -> (B,) sum over anchors of 1-|cos|."""
    _need_gpu(feat, dist, anchors)
    feat, dist, anchors = _f(feat), _f(dist), _i(anchors)
    B, N, C = feat.shape
    nA = anchors.shape[0]
    out = _new(feat.device, B)
    idx = _new(feat.device, B, nA, k, dtype=torch.int32) if want_idx else None
    _call_ws("dvm_dist_loss_fwd_f32", (_p(feat), _p(dist), _p(anchors), B, N, C, nA, k, _p(out), _p(idx)),
             feat.device, "dist", "dvm_dist_loss_workspace_bytes", B, N, C, nA, k)
    return (out, idx) if want_idx else out


def dist_loss_bwd_weights(feat, dist, anchors, idx, gout):
    """-> W (B,nA,N), see include/dvm.h."""
    _need_gpu(feat, dist, anchors, idx, gout)
    feat, dist, anchors, idx, gout = _f(feat), _f(dist), _i(anchors), _i(idx), _f(gout)
    B, N, C = feat.shape
    nA, k = idx.shape[1], idx.shape[2]
    W = _new(feat.device, B, nA, N)
    _call("dvm_dist_loss_bwd_weights_f32", _p(feat), _p(dist), _p(anchors), _p(idx), _p(gout), B, N, C, nA, k, _p(W))
    return W


U3_NWEIGHTS = 101


def uni3fc_weight_table(tensors):
    """The host array of DVM_U3_NWEIGHTS device pointers dvm_uni3fc_fwd_f32 takes (order: include/dvm.h) from a list of
    fp32 CUDA tensors; returns (kept-alive tensors, ctypes array)."""
    ts = [_f(t) for t in tensors]
    if len(ts) != U3_NWEIGHTS:
        raise DvmError("uni3fc_weight_table: %d tensors, expected %d" % (len(ts), U3_NWEIGHTS))
    _need_gpu(*ts)
    return ts, (ctypes.c_void_p * U3_NWEIGHTS)(*[t.data_ptr() for t in ts])


def _ensure_pair_ctx(dev):
    """-> (device index, stream), with the library's helper streams / events for it made (once, outside the compute call)."""
    ctx = (dev.index, _stream())
    if ctx not in _pair_ctx:
        _call("dvm_pair_init")
        _pair_ctx.add(ctx)
    return ctx


def uni3fc_forward(table, x, dino, k=40):
    """LG-Net's eval-mode forward in ONE native call (dvm_uni3fc_fwd_f32): x (B,3,N), dino (B,N,1152) -> feat (B,N,128),
    tmp (B,N,64).  `table` = uni3fc_weight_table(...)."""
    _need_gpu(x, dino)
    x, dino = _f(x), _f(dino)
    B, _, N = x.shape
    if tuple(dino.shape) != (B, N, 1152):
        raise DvmError("uni3fc_forward: dino features %s, expected %s" % (tuple(dino.shape), (B, N, 1152)))
    dev = x.device
    feat, tmp = _new(dev, B, N, 128), _new(dev, B, N, 64)
    nb = _lib.load().dvm_uni3fc_fwd_workspace_bytes(B, N, int(k))
    ws = workspace(nb, dev, "uni3fc")
    _ensure_pair_ctx(dev)
    _call("dvm_uni3fc_fwd_f32", _p(x), _p(dino), B, N, ctypes.cast(table[1], ctypes.c_void_p), U3_NWEIGHTS, int(k), _p(feat), _p(tmp),
          _p(ws), nb)
    return feat, tmp


U3_TRAIN_NPARAMS = 167   # DVM_U3_TRAIN_NPARAMS (include/dvm.h)


def _ptr_table(tensors, n):
    if len(tensors) != n:
        raise DvmError("pointer table: %d tensors, expected %d" % (len(tensors), n))
    return (ctypes.c_void_p * n)(*[None if t is None else t.data_ptr() for t in tensors])


def knn_tap():
    """Test handle on the feature-space kNN layers.  tests/test_gpu_network.py replaces `ops.knn_neg` by a callable object with
    the attributes `forced` (None, or per-layer index arrays (B,N,k) to use INSTEAD of our own sets: teacher forcing with the
    reference's neighbours), `log` (list that receives our own sets, layer by layer) and `i` (cursor into `forced`).  The
    layer-by-layer Python path goes through that object call by call; a native whole-network call has no Python between its
    layers, so it hands the same object's `forced` entries to the library and appends the library's own sets to `log`
    (dvm_uni3fc_train_fwd_f32's knn_forced / knn_log).  Returns the object, or None when knn_neg is the plain function."""
    import inspect
    fn = globals()["knn_neg"]
    return None if inspect.isfunction(fn) else (fn if hasattr(fn, "log") and hasattr(fn, "forced") else None)


def _call_sync(name, coll, *args):
    """_call for a *_sync_f32 entry, `args` ending with the collective it is handed (coll.bind(..), or None): an exception that
    the collective's all-reduce raised during the call is reported in place of the return code."""
    rc = getattr(_lib.load(), name)(*args, _stream())
    if coll is not None and coll.error is not None:
        err, coll.error = coll.error, None
        raise DvmError("%s: the collective failed: %r" % (name, err))
    check(rc, name)


def uni3fc_train_forward(params, x, dino, k, eps, momentum, defer_stats=False, groups=1, coll=None):
    """LG-Net's training-mode forward in ONE native call (dvm_uni3fc_train_fwd_f32).  params: the U3_TRAIN_NPARAMS tensors of
    include/dvm.h's table (raw parameters + BatchNorm running statistics, updated in place); x (B,3,N), dino (B,N,1152)
    -> feat (B,N,128), tmp (B,N,64), arena (uint8 tensor holding what dvm_uni3fc_train_bwd_f32 needs)."""
    _need_gpu(x, dino)
    x, dino = _f(x), _f(dino)
    B, _, N = x.shape
    if tuple(dino.shape) != (B, N, 1152):
        raise DvmError("uni3fc_train_forward: dino features %s, expected %s" % (tuple(dino.shape), (B, N, 1152)))
    dev = x.device
    feat, tmp = _new(dev, B, N, 128), _new(dev, B, N, 64)
    nb = _lib.load().dvm_uni3fc_train_workspace_bytes(B, N, int(k))
    arena = scratch(nb, dev)
    _ensure_pair_ctx(dev)
    table = _ptr_table(params, U3_TRAIN_NPARAMS)
    tap = knn_tap()
    forced = logs = ftab = ltab = None
    if tap is not None:
        logs = [_new(dev, B, N, int(k), dtype=torch.int32) for _ in range(7)]
        ltab = ctypes.cast(_ptr_table(logs, 7), ctypes.c_void_p)
        if tap.forced is not None:
            import numpy as np
            forced = [torch.from_numpy(np.ascontiguousarray(tap.forced[tap.i + l]).astype(np.int32)).to(dev) for l in range(7)]
            if any(tuple(f.shape) != (B, N, int(k)) for f in forced):
                raise DvmError("uni3fc_train_forward: forced neighbour sets must be (B, N, k)")
            ftab = ctypes.cast(_ptr_table(forced, 7), ctypes.c_void_p)
    # coll (dvm.dist.TorchCollective): BatchNorm statistics and the position-encoding range over ALL ranks of a data-parallel step
    _call_sync("dvm_uni3fc_train_fwd_sync_f32", coll, _p(x), _p(dino), B, N, ctypes.cast(table, ctypes.c_void_p), U3_TRAIN_NPARAMS, int(k),
               float(eps), float(momentum), int(groups), 1 if defer_stats else 0, ftab, ltab, _p(feat), _p(tmp), _p(arena), nb,
               coll.bind(arena) if coll is not None else None)
    if tap is not None:
        tap.log.extend(logs)
        if forced is not None:
            tap.i += 7
    return feat, tmp, arena


CRIT_TRAIN_NPARAMS = 10


def _graph_c(g):
    """The batched graph dict as the C ABI wants it: int32 / fp32, contiguous (the same tensors when they already are — dg_build's
    always are; a caller-supplied `geometry=` with int64 or strided indices is converted instead of being reinterpreted)."""
    return {"nodes_idx": _i(g["nodes_idx"]), "one_ring": _i(g["one_ring"]), "infl_idx": _i(g["infl_idx"]), "weights": _f(g["weights"])}


def _graph_ptrs(g):
    return _p(g["nodes_idx"]), _p(g["one_ring"]), _p(g["infl_idx"]), _p(g["weights"])


def criterion_train_forward(params, feat, verts, g, knn_idx, alpha, topk=10, with_map=True, dist=None):
    """The training criterion for B pairs as ONE native call (dvm_criterion_train_fwd_f32).  feat (2B,N,128), verts (2B,N,3): the B first
    shapes followed by the B second shapes; g = their batched graph dict (dg_build), knn_idx (2B,N,k) their xyz-kNN; params: the
    Deformer's 10 tensors (conv weight, bias, then the decoder's weight / bias pairs); dist = None or (dist1 (B,N,N), dist2 (B,N,N),
    anchors1 (nA,) int32, anchors2 (nA,) int32, k_dist): the dist term of all 2B shapes.
    -> terms (2B,7) [map numerator, Chamfer side means of warped (2) and verts12 (2), ARAP, dist term], arena (uint8 tensor for the backward)."""
    _need_gpu(feat, verts, knn_idx, *[g[k_] for k_ in ("nodes_idx", "one_ring", "infl_idx", "weights")])
    feat, verts, knn_idx, g = _f(feat), _f(verts), _i(knn_idx), _graph_c(g)
    P, N, C = feat.shape
    k = knn_idx.shape[-1]
    terms = _new(feat.device, P, 7)
    d1, d2, a1, a2, kd = dist if dist is not None else (None, None, None, None, 0)
    nA = 0 if dist is None else int(a1.numel())
    if dist is not None and not (d1.dtype is torch.float32 and d1.is_contiguous() and d2.dtype is torch.float32 and d2.is_contiguous()
                                 and a1.dtype is torch.int32 and a2.dtype is torch.int32 and tuple(d1.shape) == (P // 2, N, N)
                                 and tuple(d2.shape) == (P // 2, N, N) and a2.numel() == nA):
        raise DvmError("criterion_train_forward: dist term inputs must be contiguous fp32 (B,N,N) matrices and int32 anchor lists of one length")
    nb = _lib.load().dvm_criterion_train_workspace_bytes(P // 2, N, k, topk, nA, int(kd))
    arena = scratch(nb, feat.device)
    if nA:
        _ensure_pair_ctx(feat.device)
    table = _ptr_table(params, CRIT_TRAIN_NPARAMS)
    _call("dvm_criterion_train_fwd_f32", _p(feat), _p(verts), *_graph_ptrs(g), _p(knn_idx), P // 2, N, C, k, topk, neg_alpha_f32(alpha),
          ctypes.cast(table, ctypes.c_void_p), CRIT_TRAIN_NPARAMS, 1 if with_map else 0, _p(d1), _p(d2), _p(a1), _p(a2), nA, int(kd),
          _p(terms), _p(arena), nb)
    return terms, arena


def criterion_train_backward(params, grads, g_terms, feat, verts, g, knn_idx, alpha, arena, topk=10, with_map=True, dist=None):
    """dvm_criterion_train_bwd_f32: -> d_feat (2B,N,128); the Deformer's parameter gradients are ADDED into `grads`."""
    _need_gpu(feat, g_terms, knn_idx)
    feat, verts, knn_idx, g = _f(feat), _f(verts), _i(knn_idx), _graph_c(g)
    P, N, C = feat.shape
    k = knn_idx.shape[-1]
    d_feat = torch.empty_like(feat)
    _, _, a1, a2, kd = dist if dist is not None else (None, None, None, None, 0)
    nA = 0 if dist is None else int(a1.numel())
    if nA:
        _ensure_pair_ctx(feat.device)
    ptab, gtab = _ptr_table(params, CRIT_TRAIN_NPARAMS), _ptr_table(grads, CRIT_TRAIN_NPARAMS)
    _call("dvm_criterion_train_bwd_f32", _p(_f(g_terms)), _p(feat), _p(verts), *_graph_ptrs(g), _p(knn_idx), P // 2, N, C, k, topk,
          neg_alpha_f32(alpha), ctypes.cast(ptab, ctypes.c_void_p), ctypes.cast(gtab, ctypes.c_void_p), CRIT_TRAIN_NPARAMS,
          1 if with_map else 0, _p(a1), _p(a2), nA, int(kd), _p(d_feat), _p(arena), arena.numel())
    return d_feat


def criterion_dir_train_forward(params, feat_s, feat_t, verts_s, verts_t, g, knn_s, knn_t, alpha, topk=10, with_map=False):
    """ONE direction of the training criterion's deformation part for P pairs with N source and M target points
    (dvm_criterion_dir_train_fwd_f32): g = the SOURCES' graph dict, knn_s (P,N,k) / knn_t (P,M,k) the xyz-kNN of both sides.
    -> terms (P,7), arena."""
    _need_gpu(feat_s, feat_t, verts_s, verts_t, knn_s, knn_t)
    feat_s, feat_t, verts_s, verts_t = _f(feat_s), _f(feat_t), _f(verts_s), _f(verts_t)
    knn_s, knn_t, g = _i(knn_s), _i(knn_t), _graph_c(g)
    P, N, C = feat_s.shape
    M, k = feat_t.shape[1], knn_s.shape[-1]
    terms = _new(feat_s.device, P, 7)
    nb = _lib.load().dvm_criterion_dir_train_workspace_bytes(P, N, M, k, topk)
    arena = scratch(nb, feat_s.device)
    table = _ptr_table(params, CRIT_TRAIN_NPARAMS)
    _call("dvm_criterion_dir_train_fwd_f32", _p(feat_s), _p(feat_t), _p(verts_s), _p(verts_t), *_graph_ptrs(g), _p(knn_s), _p(knn_t),
          P, N, M, C, k, topk, neg_alpha_f32(alpha), ctypes.cast(table, ctypes.c_void_p), CRIT_TRAIN_NPARAMS, 1 if with_map else 0,
          _p(terms), _p(arena), nb)
    return terms, arena


def criterion_dir_train_backward(params, grads, g_terms, feat_s, feat_t, verts_s, verts_t, g, knn_s, knn_t, alpha, arena, topk=10, with_map=False):
    """dvm_criterion_dir_train_bwd_f32: -> (d_feat_s (P,N,128), d_feat_t (P,M,128)); parameter gradients ADDED into `grads`."""
    _need_gpu(feat_s, g_terms, knn_s, knn_t)
    feat_s, feat_t, verts_s, verts_t = _f(feat_s), _f(feat_t), _f(verts_s), _f(verts_t)
    knn_s, knn_t, g = _i(knn_s), _i(knn_t), _graph_c(g)
    P, N, C = feat_s.shape
    M, k = feat_t.shape[1], knn_s.shape[-1]
    d_s, d_t = torch.empty_like(feat_s), torch.empty_like(feat_t)
    ptab, gtab = _ptr_table(params, CRIT_TRAIN_NPARAMS), _ptr_table(grads, CRIT_TRAIN_NPARAMS)
    _call("dvm_criterion_dir_train_bwd_f32", _p(_f(g_terms)), _p(feat_s), _p(feat_t), _p(verts_s), _p(verts_t), *_graph_ptrs(g),
          _p(knn_s), _p(knn_t), P, N, M, C, k, topk, neg_alpha_f32(alpha), ctypes.cast(ptab, ctypes.c_void_p),
          ctypes.cast(gtab, ctypes.c_void_p), CRIT_TRAIN_NPARAMS, 1 if with_map else 0, _p(d_s), _p(d_t), _p(arena), arena.numel())
    return d_s, d_t


def uni3fc_train_running_stats(params, arena, B, N, k, momentum, groups=1):
    """The 26 running-statistics updates of a forward that ran with defer_stats=True (dvm_uni3fc_train_running_stats_f32), on the
    current stream."""
    table = _ptr_table(params, U3_TRAIN_NPARAMS)
    _call("dvm_uni3fc_train_running_stats_f32", ctypes.cast(table, ctypes.c_void_p), U3_TRAIN_NPARAMS, int(B), int(N), int(k), int(groups),
          float(momentum), _p(arena), arena.numel())


def uni3fc_train_backward(params, grads, dino, feat, tmp, arena, g_feat, g_tmp, k, groups=1, coll=None):
    """dvm_uni3fc_train_bwd_f32: ADDS the parameter gradients into `grads` (tensors aligned with `params`; None for the
    running statistics)."""
    _need_gpu(g_feat, dino)
    B, N, _ = feat.shape
    _ensure_pair_ctx(feat.device)
    g_feat = _f(g_feat)
    g_tmp = None if g_tmp is None else _f(g_tmp)
    ptab, gtab = _ptr_table(params, U3_TRAIN_NPARAMS), _ptr_table(grads, U3_TRAIN_NPARAMS)
    _call_sync("dvm_uni3fc_train_bwd_sync_f32", coll, _p(g_feat), _p(g_tmp), _p(dino), _p(feat), _p(tmp), B, N,
               ctypes.cast(ptab, ctypes.c_void_p), ctypes.cast(gtab, ctypes.c_void_p), U3_TRAIN_NPARAMS, int(k), int(groups), _p(arena),
               arena.numel(), coll.bind(arena) if coll is not None else None)


class GeometryCache:
    """Opt-in per-shape graph cache of the pair forward (the reference rebuilds both deformation graphs on every
    call, models/loss.py:1325-1337).  An entry is a DEDICATED workspace in which a dvm_pair_fwd_cached_f32 call left the
    coordinate-only products of a batch (graphs, grids, xyz kNN); it is keyed by whatever identifies the batch's geometry —
    the caller's shape ids AND FPS start indices (a different start gives a different graph) — plus the sizes.  A hit skips the
    geometry chain; outputs are bit-identical.  Least-recently-used entries are dropped beyond `max_entries`."""

    def __init__(self, max_entries=16):
        import collections
        self.max_entries, self.entries, self.hits, self.misses = max_entries, collections.OrderedDict(), 0, 0

    def lookup(self, key, nbytes, device):
        """-> (workspace, reuse flag)"""
        ent = self.entries.get(key)
        if ent is not None and ent.numel() >= nbytes and ent.device == device:
            self.entries.move_to_end(key)
            self.hits += 1
            return ent, 1
        ent = scratch(max(int(nbytes), 256), device)
        self.entries[key] = ent
        self.misses += 1
        while len(self.entries) > self.max_entries:
            self.entries.popitem(last=False)
        return ent, 0

    def clear(self):
        self.entries.clear()


def pair_forward(wl, feat1, feat2, verts1, verts2, alpha, start1, start2, with_map=True, out=None, cache=None, key=None):
    """Config-2 path for B pairs, BOTH directions in one call.
    Returns (out12, out21), each dict(warped, verts12, T12, losses[B,6]).
    cache / key: a GeometryCache and the hashable identity of this batch's geometry (shape ids + FPS starts): on a hit the
    graphs / grids / xyz kNN of the cached call are reused (same bits, no geometry chain)."""
    _need_gpu(feat1, feat2, verts1, verts2, start1, start2, *wl)
    feat1, feat2, verts1, verts2 = _f(feat1), _f(feat2), _f(verts1), _f(verts2)
    start1, start2 = _i(start1), _i(start2)
    B, N, _ = feat1.shape
    M = feat2.shape[1]
    dev = feat1.device
    o12, o21 = out if out is not None else (_pair_out(B, N, dev), _pair_out(B, M, dev))
    nb = _lib.load().dvm_pair_workspace_bytes(B, N, M)
    ctx = _ensure_pair_ctx(dev)
    args = (_p(feat1), _p(feat2), _p(verts1), _p(verts2), B, N, M, neg_alpha_f32(alpha), _p(start1), _p(start2), *[_p(w) for w in wl],
            int(with_map), *_pair_out_ptrs(o12), *_pair_out_ptrs(o21))
    if cache is None:
        ws = workspace(nb, dev, "pair2")
        _call("dvm_pair_fwd_f32", *args, _p(ws), nb)
        return o12, o21
    if key is None:
        raise DvmError("pair_forward: a GeometryCache needs the key of this batch's geometry (shape ids + FPS starts)")
    ws, reuse = cache.lookup((key, B, N, M, bool(with_map), ctx), nb, dev)
    _call("dvm_pair_fwd_cached_f32", *args, _p(ws), nb, reuse)   # `reuse` stands between the size and the stream
    return o12, o21


def _cu_count():
    """Compute units of the current device."""
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


class PairPipeline:
    """The pair forward as a two-stage software pipeline over a stream of batches: stage 1 = the coordinate-only geometry of a
    batch (dvm_pair_geometry_f32: FPS -> node grid -> ring -> influence -> skinning, vertex grid, xyz kNN) on a stream of its own,
    stage 2 = everything that needs the features (dvm_pair_fwd_cached_f32 with reuse_geometry = 1) on torch's current stream.
    While stage 2 of batch t runs, stage 1 of batch t + 1 does: the N / 2 dependent FPS steps (0.65 us each, a latency chain that
    no batch size hides) leave the critical path.  NOTHING is cached — every batch's graphs are built exactly once, as in the
    reference (models/loss.py:1325-1337), only one stage earlier; outputs are bit-identical to pair_forward.

        pipe = PairPipeline(wl, B, N, M)
        tk = pipe.prefetch(v1, v2, s1, s2, ready=ev)          # batch 0
        for each batch:  (o12, o21), tk = pipe.step(tk, f1, f2, alpha, next_coords=(v1', v2', s1', s2'), ready=ev')

    step() enqueues the two stages in the order (`schedule`) that measured faster for the batch size (bench.py --pairs 32 ... 512,
    profiles/r6_pipeline_order.txt): "geometry first" while its FPS workgroups (one per cloud) fit the compute units once — the
    dependent FPS chain is then the long pole and must start at once —, "features first" beyond (the chip is throughput-bound and
    the sweep, enqueued first, is disturbed less).  `depth` workspaces (default 2) rotate; a ticket must be consumed by forward()
    before `depth` further prefetches."""

    def __init__(self, wl, B, N, M, with_map=True, depth=2, device=None):
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else device
        self.wl, self.B, self.N, self.M, self.with_map, self.dev = wl, int(B), int(N), int(M), bool(with_map), dev
        self.nb = _lib.load().dvm_pair_workspace_bytes(self.B, self.N, self.M)
        self.ws = [scratch(max(int(self.nb), 256), dev) for _ in range(depth)]
        self.free = [None] * depth           # event: the stage-2 call that last used the workspace has finished
        self.geo = torch.cuda.Stream(device=dev)
        with torch.cuda.stream(self.geo):
            _call("dvm_pair_init")           # the geometry stream's own helper stream / events
        self.n = 0
        self.slot_gen = [0] * depth          # which prefetch last wrote the workspace (a ticket is valid while it is the one)
        self.schedule = "geometry first" if 2 * self.B <= _cu_count() else "features first"

    def close(self):
        """The current stream waits for whatever the geometry stream still has in flight (a prefetch that no forward() consumed writes
        into a workspace this object owns: its memory must not return to the allocator before that)."""
        if getattr(self, "geo", None) is not None:
            torch.cuda.current_stream(self.dev).wait_stream(self.geo)
            self.geo = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001  (interpreter shutdown)
            pass

    def prefetch(self, verts1, verts2, start1, start2, ready=None):
        """Enqueue stage 1 for a batch; -> ticket for forward().  ready: a torch.cuda.Event behind which the coordinates and starts are
        valid (e.g. recorded when the batch was loaded); None = behind everything enqueued on the current stream so far — which, called
        after a forward(), is the END of that forward: no overlap with it (pass `ready` to pipeline)."""
        _need_gpu(verts1, verts2, start1, start2)
        cur = torch.cuda.current_stream(self.dev)
        converted = not (all(t.dtype is torch.float32 and not t.requires_grad and t.is_contiguous() for t in (verts1, verts2))
                         and all(t.dtype is torch.int32 and t.is_contiguous() for t in (start1, start2)))
        if converted and ready is not None:
            cur.wait_event(ready)                       # the conversions below read the inputs on the current stream
        verts1, verts2, start1, start2 = _f(verts1), _f(verts2), _i(start1), _i(start2)
        if tuple(verts1.shape) != (self.B, self.N, 3) or tuple(verts2.shape) != (self.B, self.M, 3):
            raise DvmError("PairPipeline.prefetch: coordinates %s / %s, built for B=%d N=%d M=%d"
                           % (tuple(verts1.shape), tuple(verts2.shape), self.B, self.N, self.M))
        if self.geo is None:
            raise DvmError("PairPipeline.prefetch: the pipeline was closed")
        slot = self.n % len(self.ws)
        self.n += 1
        self.slot_gen[slot] = self.n
        if ready is None or converted:
            self.geo.wait_stream(cur)                   # the coordinates (or their fp32 / int32 copies) were produced on the caller's stream
        else:
            self.geo.wait_event(ready)
        if self.free[slot] is not None:
            self.geo.wait_event(self.free[slot])        # the workspace's previous consumer is done
        with torch.cuda.stream(self.geo):
            _call("dvm_pair_geometry_f32", _p(verts1), _p(verts2), self.B, self.N, self.M, _p(start1), _p(start2), int(self.with_map),
                  _p(self.ws[slot]), self.nb)
            ready = torch.cuda.Event()
            ready.record()
        return dict(pipe=self, slot=slot, gen=self.n, ready=ready, verts1=verts1, verts2=verts2, start1=start1, start2=start2)

    def forward(self, ticket, feat1, feat2, alpha, out=None):
        """Stage 2 of the ticket's batch on the current stream -> (out12, out21) as pair_forward."""
        _need_gpu(feat1, feat2, *self.wl)
        feat1, feat2 = _f(feat1), _f(feat2)
        B, N, M, dev = self.B, self.N, self.M, self.dev
        if tuple(feat1.shape) != (B, N, 128) or tuple(feat2.shape) != (B, M, 128):
            raise DvmError("PairPipeline.forward: features %s / %s, built for B=%d N=%d M=%d" % (tuple(feat1.shape), tuple(feat2.shape), B, N, M))
        if ticket.get("pipe") is not self:
            raise DvmError("PairPipeline.forward: the ticket was issued by another pipeline (its geometry is in that pipeline's workspace)")
        slot = ticket["slot"]
        if self.slot_gen[slot] != ticket["gen"]:
            raise DvmError("PairPipeline.forward: this ticket's workspace has been rewritten by a later prefetch (%d workspaces rotate: "
                           "consume a ticket before %d further prefetches)" % (len(self.ws), len(self.ws)))
        o12, o21 = out if out is not None else (_pair_out(B, N, dev), _pair_out(B, M, dev))
        _ensure_pair_ctx(dev)
        cur = torch.cuda.current_stream(dev)
        cur.wait_event(ticket["ready"])
        _call("dvm_pair_fwd_cached_f32", _p(feat1), _p(feat2), _p(ticket["verts1"]), _p(ticket["verts2"]), B, N, M, neg_alpha_f32(alpha),
              _p(ticket["start1"]), _p(ticket["start2"]), *[_p(w) for w in self.wl], int(self.with_map), *_pair_out_ptrs(o12),
              *_pair_out_ptrs(o21), _p(self.ws[slot]), self.nb, 1)
        ev = torch.cuda.Event()
        ev.record(cur)
        self.free[slot] = ev
        return o12, o21

    def step(self, ticket, feat1, feat2, alpha, next_coords=None, ready=None, out=None):
        """forward(ticket, ...) and prefetch(*next_coords, ready=ready) in the order that suits the batch size
        -> ((out12, out21), next ticket or None)."""
        if next_coords is None:
            return self.forward(ticket, feat1, feat2, alpha, out=out), None
        if self.schedule == "geometry first":
            nxt = self.prefetch(*next_coords, ready=ready)
            return self.forward(ticket, feat1, feat2, alpha, out=out), nxt
        outs = self.forward(ticket, feat1, feat2, alpha, out=out)
        return outs, self.prefetch(*next_coords, ready=ready)
