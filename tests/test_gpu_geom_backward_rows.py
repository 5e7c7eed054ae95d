"""-m gpu: the geometric loss backward kernels of csrc/dvm_loss_bwd.hip — rot6d_bwd / def9_bwd, dg_warp_bwd + dg_arap_bwd, chamfer_bwd
— per ELEMENT (CPU half: tests/test_geom_backward_rows_cpu.py, which runs the same checks on fp32 restatements and shows that every
planted mutation of them — a dropped ring neighbour, another node's R or T, a lost or doubled atomic on a hub, a skipped last
vertex, recomputed indices, ... — fails at least one of them).

(1) Exact plantings (tests/exact_inputs.py): integer clouds and gradients, axis-aligned rotations, dyadic weights, 2 g_arap / Nn =
    +-1/4 or 0.  Every addend and every partial sum is exact in fp32, so neither the atomics' order nor rounding can move a bit: the
    device result must EQUAL the definition evaluated in float64.  N in {2, 3, 64, 257, 513, 2048} (Nn = 1: a single thread; 257 / 513:
    one vertex resp. one node in a second workgroup), plain and hub graphs (in-degree 2 N on node 0, duplicate slots in a row, ring
    self-entries); all 24 frame orientations; Chamfer with true nearest neighbours, one hub, arbitrary valid indices at (1,1), (255,1),
    (256,257): N + M = 513, (300,170), (2048,2048).  B = 3 different entries with g_arap = +, -, 0.  Outputs are NaN-filled by the test
    (the C entries are called with the test's own buffers): the memsets are under test.
    Criterion level (ops.criterion_dir_train_* and the swapped form): g_terms zero except ARAP = +-Nn/8 per pair; the gradients of the
    last decoder layer's bias (column sums of ddef9) and of the first three input columns of its weight must equal the integer
    reference: def9_bwd_kernel's identity offset, garap_stride = 7, the zeroing of dwarped / dv12.
    The nn_ops autograd wrappers on the same plantings: expanded (stride-0) and transposed grad outputs, the materialised zero g_arap.
(2) Real-valued hard families against float64 with the derived bound 2 u (n + c) A per element, and rot6d_bwd per row against
    ROT6D_C u s (tests/geom_backward_ref.py states both): device-built graphs on uniform and duplicated clouds, hubs, orphan nodes,
    a rigid motion (ARAP residual = rounding noise), a cloud far from the origin, gradients over nine decades; near-parallel,
    badly scaled and zero-component frames.
All indices handed to the kernels are valid rows."""
import numpy as np
import pytest
import torch

import exact_inputs as X
import geom_backward_ref as G
from oracle import oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from dvm import ops as _ops
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _ops


@pytest.fixture(scope="module")
def wl(ops):
    return ops.deformer_weight_list(X.deformer_weights(), "cuda")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def _st(cases, key, dt=None):
    a = np.stack([np.asarray(c[key]) for c in cases])
    return dev(a if dt is None else a.astype(dt))


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


def _graph(cases):
    return {k: _st(cases, k, np.int32) for k in ("nodes_idx", "one_ring", "infl_idx")} | {"weights": _st(cases, "weights", np.float32)}


# ------------------------------------------------------------------------------------- the C entries on the test's own NaN-filled outputs
def warp_bwd_raw(ops, cases):
    from dvm import _lib
    p = ops._p
    xyz, R, T, gw, ga = (_st(cases, k, np.float32) for k in ("xyz", "R", "T", "gw", "ga"))
    g = _graph(cases)
    B, N, _ = xyz.shape
    dR, dT = _nan(B, N // 2, 3, 3), _nan(B, N // 2, 3)
    _lib.check(_lib.load().dvm_dg_warp_arap_bwd_f32(p(xyz), B, N, p(g["nodes_idx"]), p(g["one_ring"]), p(g["infl_idx"]), p(g["weights"]), p(R), p(T),
                                                    p(gw), p(ga), p(dR), p(dT), ops._stream()), "dvm_dg_warp_arap_bwd_f32")
    torch.cuda.synchronize()
    return host(dR), host(dT)


def chamfer_bwd_raw(ops, cases):
    from dvm import _lib
    p = ops._p
    a, b, g1, g2 = (_st(cases, k, np.float32) for k in ("a", "b", "g1", "g2"))
    i1, i2 = _st(cases, "i1", np.int32), _st(cases, "i2", np.int32)
    B, N, _ = a.shape
    M = b.shape[1]
    da, db = _nan(B, N, 3), _nan(B, M, 3)
    _lib.check(_lib.load().dvm_chamfer_bwd_f32(p(a), p(b), p(i1), p(i2), p(g1), p(g2), B, N, M, p(da), p(db), ops._stream()), "dvm_chamfer_bwd_f32")
    torch.cuda.synchronize()
    return host(da), host(db)


def rot6d_bwd_raw(ops, d6, gR):
    from dvm import _lib
    d6, gR = dev(d6), dev(gR)
    out = _nan(*d6.shape)
    _lib.check(_lib.load().dvm_rot6d_bwd_f32(ops._p(d6), ops._p(gR), d6.shape[0], ops._p(out), ops._stream()), "dvm_rot6d_bwd_f32")
    torch.cuda.synchronize()
    return host(out)


def _ids(v):
    return "x".join(str(x) for x in v) if isinstance(v, tuple) else str(v)


# ------------------------------------------------------------------------------------------------------------- (1) exact plantings
@pytest.mark.parametrize("hub", [False, True], ids=["plain", "hub"])
@pytest.mark.parametrize("N", X.BWD_SIZES)
def test_warp_arap_bwd_exact(ops, N, hub):
    cases = X.warp_bwd_batch(N, hub)
    dR, dT = warp_bwd_raw(ops, cases)
    for b, c in enumerate(cases):
        G.check_equal("d_T entry %d" % b, dT[b], c["d_T"])
        G.check_equal("d_R entry %d" % b, dR[b], c["d_R"])


def test_rot6d_bwd_exact(ops):
    r = X.rot6d_bwd_direct(X.BWD_SEED)
    G.check_equal("rot6d_bwd", rot6d_bwd_raw(ops, r["d6"], r["gR"]), r["grad"])


@pytest.mark.parametrize("variant", X.CHAMFER_VARIANTS)
@pytest.mark.parametrize("shape", X.CHAMFER_BWD_SHAPES, ids=_ids)
def test_chamfer_bwd_exact(ops, shape, variant):
    cases = X.chamfer_bwd_batch(*shape, variant)
    da, db = chamfer_bwd_raw(ops, cases)
    for b, c in enumerate(cases):
        G.check_equal("d_a entry %d" % b, da[b], c["d_a"])
        G.check_equal("d_b entry %d" % b, db[b], c["d_b"])


def _arap_grads(Nn, P):
    return [(Nn / 8.0) * (1, -1)[p % 2] for p in range(P)]


def _check_decoder_grads(what, grads, cr):
    """grads: the ten parameter gradient buffers (zero before the call); W3 is entry 8 (9,128), b3 entry 9"""
    G.check_equal(what + " d b3", host(grads[9]), cr["db3"])
    W3 = host(grads[8])
    G.check_equal(what + " d W3[:, :3]", W3[:, :3], cr["dW3"])
    assert (W3[:, 3:] == 0).all(), what + ": the decoder's other hidden channels are exactly 0"
    assert np.abs(cr["dW3"]).max() > 0 and np.abs(cr["db3"]).max() > 0


def _oracle_geometry(refs):
    """the sources' graph and both xyz-kNN tables as the reference built them (the device's builds are pinned against these elsewhere;
    the dense lattices used here are full of ties, which this test is not about)"""
    g = {k: dev(np.stack([r["graph"][k] for r in refs])) for k in ("nodes_idx", "one_ring", "infl_idx", "weights")}
    return g, dev(np.stack([r["idx11"] for r in refs])), dev(np.stack([r["idx22"] for r in refs]))


@pytest.mark.parametrize("case", X.CRIT_BWD_CASES, ids=_ids)
def test_criterion_dir_backward_decoder_grads_exact(ops, wl, case):
    N, M, hi = case
    a, cases = X.planted_batch(N, M, X.PAIR_SEED, hi=hi)
    refs = [c[1] for c in cases]
    d = {k: dev(v) for k, v in a.items()}
    g, knn_s, knn_t = _oracle_geometry(refs)
    args = (d["feat1"], d["feat2"], d["verts1"], d["verts2"], g, knn_s, knn_t, X.ALPHA)
    terms, arena = ops.criterion_dir_train_forward(wl, *args, 10, True)
    ga = _arap_grads(N // 2, len(refs))
    g_terms = torch.zeros(len(refs), 7, device="cuda")
    g_terms[:, 5] = torch.tensor(ga)
    grads = [torch.zeros_like(p) for p in wl]
    ops.criterion_dir_train_backward(wl, grads, g_terms, *args, arena, 10, True)
    torch.cuda.synchronize()
    for b, r in enumerate(refs):
        assert host(terms)[b, 5] == r["losses"][2]
    _check_decoder_grads("criterion_dir %s" % (case,), grads, X.criterion_bwd_reference(refs, ga))


def test_criterion_swapped_backward_decoder_grads_exact(ops, wl):
    N, hi = X.CRIT_BWD_SWAPPED
    a, cases = X.planted_batch(N, N, X.PAIR_SEED, both=True, hi=hi)
    refs = [c[1] for c in cases] + [c[2] for c in cases]
    d = {k: dev(v) for k, v in a.items()}
    verts, feat = torch.cat([d["verts1"], d["verts2"]]), torch.cat([d["feat1"], d["feat2"]])
    g, knn, _ = _oracle_geometry(refs)
    terms, arena = ops.criterion_train_forward(wl, feat, verts, g, knn, X.ALPHA, 10, True)
    ga = _arap_grads(N // 2, len(refs))
    g_terms = torch.zeros(len(refs), 7, device="cuda")
    g_terms[:, 5] = torch.tensor(ga)
    grads = [torch.zeros_like(p) for p in wl]
    ops.criterion_train_backward(wl, grads, g_terms, feat, verts, g, knn, X.ALPHA, arena, 10, True)
    torch.cuda.synchronize()
    for b, r in enumerate(refs):
        assert host(terms)[b, 5] == r["losses"][2]
    _check_decoder_grads("criterion (swapped halves) %d" % N, grads, X.criterion_bwd_reference(refs, ga))


# ----------------------------------------------------------------------------------------------- the nn_ops wrappers, same plantings
def test_nn_ops_rot6d_autograd_exact(ops):
    from dvm import nn_ops
    r = X.rot6d_bwd_direct(X.BWD_SEED)
    d6 = dev(r["d6"]).requires_grad_(True)
    gR = dev(r["gR"])
    (nn_ops.rot6d(d6) * gR).sum().backward()
    G.check_equal("nn_ops.rot6d", host(d6.grad), r["grad"])
    assert torch.equal(d6.grad, ops.rot6d_bwd(d6.detach(), gR))
    # a transposed (non-contiguous) grad output handed to the node as it is
    d6b = dev(r["d6"]).requires_grad_(True)
    gT = gR.transpose(1, 2).contiguous().transpose(1, 2)
    assert not gT.is_contiguous()
    torch.autograd.backward([nn_ops.rot6d(d6b)], [gT])
    G.check_equal("nn_ops.rot6d, strided grad", host(d6b.grad), r["grad"])


@pytest.mark.parametrize("N", [3, 257, 2048])
def test_nn_ops_dg_warp_arap_autograd_exact(ops, N):
    from dvm import nn_ops
    cases = X.warp_bwd_batch(N, True)
    xyz, gw, ga = (_st(cases, k, np.float32) for k in ("xyz", "gw", "ga"))
    g = _graph(cases)

    def leaves():
        return _st(cases, "R", np.float32).requires_grad_(True), _st(cases, "T", np.float32).requires_grad_(True)

    # (a) loss = warped.sum(): gw is an expanded (stride-0) ones tensor, g_arap the materialised zero
    R, T = leaves()
    warped, arap = nn_ops.dg_warp_arap(xyz, g, R, T)
    warped.sum().backward()
    dR0, dT0 = ops.dg_warp_arap_bwd(xyz, g, R.detach(), T.detach(), torch.ones_like(xyz), torch.zeros_like(ga))
    assert torch.equal(R.grad, dR0) and torch.equal(T.grad, dT0)
    for b, c in enumerate(cases):
        ref = X.warp_arap_bwd_rows(c["xyz"], c["nodes_idx"], c["one_ring"], c["infl_idx"], c["weights"], c["R"], c["T"], np.ones_like(c["gw"]), 0.0)
        G.check_equal("warped.sum() d_R entry %d" % b, host(R.grad)[b], ref["d_R"])
        G.check_equal("warped.sum() d_T entry %d" % b, host(T.grad)[b], ref["d_T"])
    # (b) a transposed view as gw, the planted g_arap
    R, T = leaves()
    gwT = gw.transpose(1, 2).contiguous().transpose(1, 2)
    assert not gwT.is_contiguous()
    warped, arap = nn_ops.dg_warp_arap(xyz, g, R, T)
    torch.autograd.backward([warped, arap], [gwT, ga])
    dR1, dT1 = ops.dg_warp_arap_bwd(xyz, g, R.detach(), T.detach(), gw, ga)
    assert torch.equal(R.grad, dR1) and torch.equal(T.grad, dT1)
    for b, c in enumerate(cases):
        G.check_equal("strided gw d_R entry %d" % b, host(R.grad)[b], c["d_R"])
        G.check_equal("strided gw d_T entry %d" % b, host(T.grad)[b], c["d_T"])


@pytest.mark.parametrize("shape", X.CHAMFER_BWD_SHAPES, ids=_ids)
def test_nn_ops_chamfer_nn_autograd_exact(ops, shape):
    """The node searches its own neighbours; the reference takes the lists the device found (valid arg-mins: checked against the oracle's
    distances).  Per-entry mean losses — stride-0 expanded grad outputs 1/N, 1/M — where both are powers of two ((1,1), (2048,2048): every addend
    a multiple of 2^-10), the planted dyadic g1 / g2 elsewhere (1/257 is not representable: the sum would depend on the atomics' order)."""
    from dvm import nn_ops
    N, M = shape
    cases = X.chamfer_bwd_batch(N, M, "nn")
    means = (N & (N - 1)) == 0 and (M & (M - 1)) == 0
    a, b = _st(cases, "a").requires_grad_(True), _st(cases, "b").requires_grad_(True)
    d1, d2 = nn_ops.chamfer_nn(a, b)
    _, _, i1, i2 = ops.chamfer(a.detach(), b.detach())
    if means:
        (d1.mean(1).sum() + d2.mean(1).sum()).backward()
        g1, g2 = torch.full((3, N), 1.0 / N, device="cuda"), torch.full((3, M), 1.0 / M, device="cuda")
    else:
        g1, g2 = _st(cases, "g1"), _st(cases, "g2")
        torch.autograd.backward([d1, d2], [g1, g2])
    da, db = ops.chamfer_bwd(a.detach(), b.detach(), i1, i2, g1, g2)
    for bi, c in enumerate(cases):
        o1, o2, _, _ = O.chamfer(c["a"], c["b"])
        assert np.array_equal(host(d1)[bi], o1) and np.array_equal(host(d2)[bi], o2)
        ref = X.chamfer_bwd_rows(c["a"], c["b"], host(i1)[bi], host(i2)[bi], host(g1)[bi], host(g2)[bi])
        grid = 1024 if means else X.SUM_GRID          # the addends' grid: 2 / N * integer, resp. the planting's 2^-4
        assert (ref["mag_a"] * grid < X.SUM_LIMIT).all() and (ref["mag_b"] * grid < X.SUM_LIMIT).all()
        G.check_equal("chamfer_nn d_a entry %d" % bi, host(a.grad)[bi], ref["d_a"])
        G.check_equal("chamfer_nn d_b entry %d" % bi, host(b.grad)[bi], ref["d_b"])
    assert torch.equal(a.grad, da) and torch.equal(b.grad, db)


# ------------------------------------------------------------------------------------------- (2) real-valued families, derived bounds
def _device_dg_build(ops):
    def build(xyz, start):
        g = ops.dg_build(dev(xyz)[None], torch.tensor([start], dtype=torch.int32, device="cuda"))
        return {k: host(g[k])[0] for k in ("nodes_idx", "one_ring", "infl_idx", "weights")}
    return build


@pytest.mark.parametrize("N", G.WARP_SIZES)
@pytest.mark.parametrize("family", G.WARP_FAMILIES)
def test_warp_arap_bwd_rows_within_derived_bound(ops, family, N):
    cases, ref = G.warp_family(family, N, _device_dg_build(ops))
    if family == "orphans":
        used = np.unique(np.concatenate([cases[0]["infl_idx"].ravel(), cases[0]["one_ring"].ravel()]))
        assert used.size <= N // 4 + 1
    dR, dT = warp_bwd_raw(ops, cases)
    assert np.isfinite(dR).all() and np.isfinite(dT).all()
    G.check_bound("%s N=%d d_T" % (family, N), dT, ref["d_T"], ref["bound_T"])
    G.check_bound("%s N=%d d_R" % (family, N), dR, ref["d_R"], ref["bound_R"])


def _device_nn(ops):
    def nn(a, b):
        _, _, i1, i2 = ops.chamfer(dev(a)[None], dev(b)[None])
        return host(i1)[0], host(i2)[0]
    return nn


@pytest.mark.parametrize("shape", X.CHAMFER_BWD_SHAPES, ids=_ids)
@pytest.mark.parametrize("family", G.CHAMFER_FAMILIES)
def test_chamfer_bwd_rows_within_derived_bound(ops, family, shape):
    N, M = shape
    if family == "self":
        M = N                   # a = b needs equal sizes: (1,1), (255,255), (256,256), (300,300), (2048,2048)
    cases, ref = G.chamfer_family(family, N, M, _device_nn(ops))
    da, db = chamfer_bwd_raw(ops, cases)
    G.check_bound("%s %dx%d d_a" % (family, N, M), da, ref["d_a"], ref["bound_a"])
    G.check_bound("%s %dx%d d_b" % (family, N, M), db, ref["d_b"], ref["bound_b"])
    if family == "self":
        assert (da == 0).all() and (db == 0).all()


@pytest.mark.parametrize("family", G.ROT6D_FAMILIES)
def test_rot6d_bwd_rows_within_measured_bar(ops, family):
    d6, gR, ref, bar = G.rot6d_case(family)
    G.check_bound("rot6d_bwd %s" % family, rot6d_bwd_raw(ops, d6, gR), ref, bar)
