"""Soft-correspondence / deformation-graph criterion — MI355X path behind the reference's API.

Mirrors the public names and signatures of the reference's `models/loss.py` on this path:
GraphDeformLoss_Neural (1075-1435), GraphDeformLoss_Neural_Partial (726-1073), knnsearch_t /
search_t (91-95, 121-124), knnsearch_t_grad (110-114), knn_grad (97-101), knn (451-462),
index_points (464-473), rotation_6d_to_matrix (39-45), FrobeniusLoss (476-482).
The N x M matrices of the reference are never formed: the criterion runs on the fused kernels
of dv-matcher_amd/csrc through the C ABI (include/dvm.h).  RNG draws are made with the same
calls in the same order as the reference (random.sample anchors, torch.randint FPS starts,
random.randint dump suffix), so seeding both gives the same draws.
"""
import os
import random

import numpy as np
import torch
import torch.nn as nn

from dvm import nn_ops, ops
from lib.deformation_graph_point import DeformationGraph_geod
from models.model import Deformer, index_points  # noqa: F401  (re-exported like the reference)


def rotation_6d_to_matrix(d6):
    return ops.rot6d(d6)


def knnsearch_t(x, y):
    """Hard map: argmin_j of the exact-difference cdist, (B,N,1) int64, 0-based."""
    return ops.argmin_exact(x, y).long().unsqueeze(-1)


def search_t(A1, A2):
    return knnsearch_t(A1, A2)


def knn_grad(x, y, k):
    return ops.knn_cdist(x, y, k).long()


def knn(a, b, k):
    return ops.knn_neg(a, b, k).long()


def knnsearch_t_grad(x, y, alpha=100):
    """Dense softmax(-alpha * cdist(x, y)) (B,N,M).  Only for callers that need the full matrix
    (the criterion itself uses the fused sparse form)."""
    return ops.softcorr_dense(x, y, alpha)


def save_off_file(filename, points):
    with open(filename, 'w') as f:
        f.write('OFF\n%d 0 0\n' % points.shape[0])
        for p in points:
            f.write('%s %s %s\n' % (p[0], p[1], p[2]))


class FrobeniusLoss(nn.Module):
    def forward(self, a, b):
        return torch.mean(torch.sum(torch.abs(a - b) ** 2, axis=(1, 2)))


def _host_draw_to_device(values, device):
    """The host's random draws (dist-loss anchors, FPS starts) as a device tensor WITHOUT stalling the host: a copy from
    pageable memory blocks until the stream has drained, which would serialise the host behind the whole network forward
    every step; a pinned staging buffer and a non-blocking copy keep it enqueueing.  Device tensors pass through untouched
    (no host-to-device copy inside a captured step)."""
    if torch.is_tensor(values) and values.device.type == "cuda":
        return values
    t = torch.as_tensor(np.asarray(values))
    if torch.device(device).type != "cuda":
        return t.to(device)
    return t.pin_memory().to(device, non_blocking=True)


_crit_side = {}


def _crit_streams(device, cur):
    key = (device, cur.cuda_stream)
    if key not in _crit_side:
        _crit_side[key] = (torch.cuda.Stream(device), torch.cuda.Stream(device))
    return _crit_side[key]


def _joint(u, v):
    """cat([u, v], 0) — without the copy when u and v are the two halves of one contiguous tensor (LG-Net's merged training call and
    the batched graph build return such views); autograd then flows straight into that tensor."""
    base = u._base
    if (base is not None and base is v._base and base.is_contiguous() and base.shape[0] == 2 * u.shape[0] and base.shape[1:] == u.shape[1:]
            and u.shape == v.shape and u.is_contiguous() and v.is_contiguous() and u.data_ptr() == base.data_ptr()
            and v.data_ptr() == base.data_ptr() + u.numel() * u.element_size()):
        return base
    return torch.cat([u, v], 0)


class SparsePi:
    """Top-k rows of the soft correspondence: val/idx (B,N,k); stands in for the dense (B,N,M) Pi."""

    def __init__(self, val, idx, M, log_mass=None):
        self.val, self.idx, self.M = val, idx, M
        self.log_mass = log_mass   # (B,N) log of every row's mass: the unbalanced Sinkhorn operator only (sinkhorn_pi_unbalanced)

    def to_dense(self):
        B, N, _ = self.val.shape
        out = torch.zeros(B, N, self.M, dtype=self.val.dtype, device=self.val.device)
        return out.scatter_(-1, self.idx.long(), self.val)

    def matmul(self, V):
        if torch.is_grad_enabled() and self.val.requires_grad:   # a differentiable correspondence (sinkhorn_pi under grad)
            return nn_ops.sparse_apply(self.val, self.idx, V)
        return ops.apply(self.val, self.idx, V)


def precise_map(x, y, faces):
    """The precise (vertex-to-point) map of x (B,N,d) onto the triangle mesh (y (B,M,d), faces (F,3)) in feature space as a
    SparsePi of three entries per row (val = the barycentric weights, idx = the face's vertices; not in the reference): matmul(V)
    gives the mapped coordinates on the target surface, and the rank / cycle / distortion terms take it as any other SparsePi.
    It also carries .face (B,N) and .dist (B,N).  No gradient flows through it (ops.precise_map)."""
    face, bary, pi_idx, dist = ops.precise_map(x, y, faces)
    pi = SparsePi(bary, pi_idx, y.shape[1])
    pi.face, pi.dist = face, dist
    return pi


def _relaxed(tau):
    """Whether a sinkhorn_tau setting leaves the balanced operator: None and (1, 1) do not."""
    return tau is not None and tuple(ops.tau_pair(tau)) != (1.0, 1.0)


def sinkhorn_pi(x, y, alpha=100, n_iter=5, topk=10):
    """Sinkhorn-normalised counterpart of topk_pi(knnsearch_t_grad(x, y, alpha)) as a SparsePi (not in the reference): n_iter
    row / column normalisations keep many source points from sharing one target point.  When x or y requires grad the
    SparsePi's val carries the graph (nn_ops.sinkhorn_topk: the exact gradient of the unrolled iterations); otherwise it is
    ops.sinkhorn.  Every row of it carries mass 1; sinkhorn_pi_unbalanced relaxes that."""
    val, idx = nn_ops.sinkhorn_topk(x, y, alpha, n_iter, topk=topk)
    return SparsePi(val, idx, y.shape[1])


def sinkhorn_pi_unbalanced(x, y, alpha=100, n_iter=5, topk=10, tau=(1.0, 1.0), log_a=None, log_b=None):
    """sinkhorn_pi with relaxed marginals and per-point weights (nn_ops.sinkhorn_unbalanced_topk; not in the reference):
    tau = (tau_row, tau_col) in (0, 1] damps every potential update, log_a (B,N) / log_b (B,M) are the log weights of the two
    sides.  The SparsePi carries .log_mass (B,N), the log of every row's mass: small where a source point has no partner.
    Differentiable in x, y, log_a and log_b through val and log_mass; tau = (1, 1) without weights gives sinkhorn_pi's values."""
    val, idx, lmass = nn_ops.sinkhorn_unbalanced_topk(x, y, alpha, n_iter, tau, log_a, log_b, topk=topk)
    return SparsePi(val, idx, y.shape[1], log_mass=lmass)


class _SafeSqrt(torch.autograd.Function):
    """sqrt(x) for x >= 0 whose gradient at x == 0 is 0 (torch.norm's subgradient at zero), not inf."""

    @staticmethod
    def forward(ctx, x):
        r = torch.sqrt(x)
        ctx.save_for_backward(r)
        return r

    @staticmethod
    def backward(ctx, g):
        r, = ctx.saved_tensors
        return torch.where(r > 0, g / (2 * r).clamp_min(torch.finfo(r.dtype).tiny), torch.zeros_like(g))


def _frob_norm(R):
    """||R||_F per batch element of float64 residuals (B, ...) in fp32; the gradient where it is 0 is 0, as the kernels'."""
    return _SafeSqrt.apply(R.square().flatten(1).sum(1)).float()


def _frob_kernel_takes(max_n, pvals, others=(), rows_of=None):
    """What the sparse Frobenius-norm kernels take: CUDA float32 3-D tensors with a batch, 1 <= k <= 16 for every pval, and
    1 <= rows <= max_n() for every tensor of rows_of (default: the first pval).  max_n is asked last: it loads the library."""
    ts = (*pvals, *others)
    return (all(t.is_cuda and t.dtype == torch.float32 and t.dim() == 3 for t in ts) and ts[0].shape[0] >= 1
            and all(1 <= p.shape[2] <= 16 for p in pvals) and all(1 <= t.shape[1] <= max_n() for t in (rows_of or pvals[:1])))


def _rank_term_torch(pval, pidx, M):
    """rank_term with plain torch ops, for what the kernel does not take (CPU tensors, other dtypes, N over its limit):
        ||P P^T - I||_F^2 = ||P^T P||_F^2 - sum_i d_i^2 + sum_i (d_i - 1)^2,   d_i = sum_t val[i,t]^2 = (P P^T)_ii,
    with G = P^T P (M x M) accumulated from the k x k outer product of every row.  Accumulated in float64: for a
    near-permutation P the two large terms cancel.  The gradient where the term is 0 is 0, as the kernel's."""
    B, N, k = pval.shape
    v = pval.double()
    i = pidx.long()
    outer = (v.unsqueeze(-1) * v.unsqueeze(-2)).reshape(B, -1)
    flat = (i.unsqueeze(-1) * M + i.unsqueeze(-2)).reshape(B, -1)
    G = torch.zeros(B, M * M, dtype=torch.float64, device=pval.device).scatter_add_(1, flat, outer)
    d = (v * v).sum(-1)
    frob2 = (G * G).sum(1) - (d * d).sum(1) + ((d - 1) ** 2).sum(1)
    return _SafeSqrt.apply(frob2.clamp_min(0)).float()


def rank_term(pval, pidx, M):
    """||P P^T - I||_F per batch element for the sparse top-k correspondence P (val/idx (B,N,k), M columns) —
    models/loss.py:1427-1433 — without the dense (B,N,M) P or the (B,N,N) product.  Differentiable w.r.t. pval; the gradient
    where the term is 0 (an exact permutation) is 0.  CUDA float32 input within the kernel's limits (N <= ops.rank_term_max_n(),
    k <= 16) runs on dvm_rank_term_f32 (nn_ops.rank_term: row by row, no dense array, no float atomics); anything else on the
    torch formula of _rank_term_torch, which forms an M x M float64 matrix."""
    if _frob_kernel_takes(ops.rank_term_max_n, (pval,)) and M >= 1:
        return nn_ops.rank_term(pval, pidx, M)
    return _rank_term_torch(pval, pidx, M)


def _cycle_term_torch(pval12, pidx12, pval21, pidx21):
    """cycle_term with plain torch ops, for what the kernel does not take (CPU tensors, other dtypes, N over its limit): the
    definition in float64 on dense arrays (P12 N x M, P21 M x N, their N x N product), rounded once to fp32.  The gradient where
    the term is 0 is 0, as the kernel's."""
    B, N, _ = pval12.shape
    M = pval21.shape[1]
    P12 = torch.zeros(B, N, M, dtype=torch.float64, device=pval12.device).scatter_add(-1, pidx12.long(), pval12.double())
    P21 = torch.zeros(B, M, N, dtype=torch.float64, device=pval21.device).scatter_add(-1, pidx21.long(), pval21.double())
    R = torch.bmm(P12, P21)
    R.diagonal(dim1=1, dim2=2).sub_(1.0)
    return _frob_norm(R)


def cycle_term(pval12, pidx12, pval21, pidx21):
    """||P12 P21 - I_N||_F per batch element for the two sparse top-k correspondences of a pair, P12 (val/idx (B,N,k12), M columns)
    and P21 (val/idx (B,M,k21), N columns): 0 where the two maps are mutual inverses; N != M is allowed (not in the reference).
    Differentiable w.r.t. both pval; the gradient where the term is 0 is 0.  CUDA float32 input within the kernel's limits
    (N <= ops.cycle_term_max_n(), k <= 16) runs on dvm_cycle_term_f32 (nn_ops.cycle_term: row by row, no dense array, no float
    atomics); anything else on the torch formula of _cycle_term_torch, which forms dense float64 arrays."""
    if _frob_kernel_takes(ops.cycle_term_max_n, (pval12, pval21)) and pval21.shape[1] >= 1:
        return nn_ops.cycle_term(pval12, pidx12, pval21, pidx21)
    return _cycle_term_torch(pval12, pidx12, pval21, pidx21)


def _symmetrised(dist):
    """(D + D^T) / 2 of a batch of square matrices: exactly symmetric in fp32 (the sum commutes, the halving is exact)."""
    return 0.5 * (dist + dist.transpose(1, 2))


def _distortion_term_torch(pval, pidx, dist_src, dist_tgt):
    """distortion_term with plain torch ops, for what the kernel does not take (CPU tensors, other dtypes, N or M over its limit):
    the definition in float64 on dense arrays (P N x M, P D2 N x M, the N x N product), rounded once to fp32.  The distance matrices
    are constants; the gradient where the term is 0 is 0, as the kernel's."""
    B, N, _ = pval.shape
    M = dist_tgt.shape[1]
    P = torch.zeros(B, N, M, dtype=torch.float64, device=pval.device).scatter_add(-1, pidx.long(), pval.double())
    R = torch.bmm(torch.bmm(P, dist_tgt.detach().double()), P.transpose(1, 2)) - dist_src.detach().double()
    return _frob_norm(R)


def distortion_term(pval, pidx, dist_src, dist_tgt, symmetric=False):
    """||P D2 P^T - D1||_F per batch element for the sparse top-k correspondence P (val/idx (B,N,k), M columns), the source shape's
    distance matrix D1 = dist_src (B,N,N) and the target's D2 = dist_tgt (B,M,M): the metric distortion of the map, 0 for an
    isometry; N != M is allowed (not in the reference).  The term is defined on symmetric matrices: symmetric=False takes
    (D + D^T) / 2 of both first (heat-method geodesics and a matmul-form cdist are symmetric only to rounding), symmetric=True is
    the caller's promise that they already are, bit for bit.  Differentiable w.r.t. pval only; the gradient where the term is 0 is
    0.  CUDA float32 input within the kernel's limits (N, M <= ops.distortion_term_max_n(), k <= 16) runs on
    dvm_distortion_term_f32 (nn_ops.distortion_term: row by row, no dense product, no float atomics); anything else on the torch
    formula of _distortion_term_torch, which forms dense float64 arrays."""
    if not symmetric:
        dist_src, dist_tgt = _symmetrised(dist_src), _symmetrised(dist_tgt)
    if _frob_kernel_takes(ops.distortion_term_max_n, (pval,), (dist_src, dist_tgt), rows_of=(pval, dist_tgt)):
        return nn_ops.distortion_term(pval, pidx, dist_src, dist_tgt)
    return _distortion_term_torch(pval, pidx, dist_src, dist_tgt)


def _dirichlet_term_torch(pval, pidx, V, op):
    """dirichlet_term's energy (not normalised) with plain torch ops, for what the kernel does not take (CPU tensors, other dtypes,
    refused sizes): Y = Pi V and 1/2 sum_entries w |y_i - y_j|^2 in float64 over the operator's CSR entries, rounded once to fp32.
    op: anything with rowptr (B,N+1), col / w (B,Ecap) (ops.GraphOperator).  Slots and entries with an index out of range add
    nothing.  The used length of every batch element is read back (one synchronisation per element on a device)."""
    B, N, _ = pval.shape
    Vd = V.detach().double()
    M = Vd.shape[1]
    ix = pidx.long()
    ok = (ix >= 0) & (ix < M)
    rows_of_V = Vd[torch.arange(B, device=ix.device)[:, None, None], torch.where(ok, ix, torch.zeros_like(ix))]   # (B,N,k,C)
    Y = ((pval.double() * ok).unsqueeze(-1) * rows_of_V).sum(2)
    out = []
    for b in range(B):
        rp = op.rowptr[b].long()
        used = int(rp[N])
        rows = torch.repeat_interleave(torch.arange(N, device=pval.device), rp[1:] - rp[:-1])[:used]
        c, w = op.col[b, :used].long(), op.w[b, :used].double()
        keep = (c >= 0) & (c < N)
        d = Y[b][rows[keep]] - Y[b][c[keep]]
        out.append(0.5 * (w[keep] * (d * d).sum(-1)).sum())
    return torch.stack(out).float()


def dirichlet_term(pval, pidx, V, op, normalize=True):
    """The Dirichlet energy of the pulled-back target values Y = Pi V under the source shape's neighbour operator op
    (ops.mesh_laplacian / ops.knn_laplacian): E = 1/2 sum_entries w |y_i - y_j|^2 per batch element — the smoothness of the map
    (not in the reference).  normalize=True returns E / op.norm, which is 1 for a map that preserves local lengths.  Differentiable
    w.r.t. pval only (V and the operator are data).  CUDA float32 input within the kernel's limits (k, C <= 16) runs on
    dvm_dirichlet_term_f32 (nn_ops.dirichlet_term: float64 in CSR order, no float atomics); anything else on the torch formula of
    _dirichlet_term_torch."""
    ts = (pval, V, op.w)
    if (all(t.is_cuda and t.dtype == torch.float32 for t in ts) and pval.dim() == 3 and V.dim() == 3 and op.col.dim() == 2
            and ops.dirichlet_term_takes(pval.shape[0], pval.shape[1], V.shape[1], pval.shape[2], V.shape[2], op.col.shape[1])):
        E = nn_ops.dirichlet_term(pval, pidx, V, op)
    else:
        E = _dirichlet_term_torch(pval, pidx, V, op)
    return E / op.norm.to(E.dtype) if normalize else E


def functional_map(pi_val, pi_idx, basis_src, basis_tgt):
    """The functional map of a sparse correspondence (not in the reference's loss): C (B,k1,k2) = Phi1^T M1 (Pi Phi2) in float64
    for Pi (N,M) given as pi_val / pi_idx (B,N,topk) — a soft correspondence's rows or the precise map's (bary, pi_idx) — and the
    two shapes' ops.Eigenbasis (basis_src on the N source vertices with its mass, basis_tgt on the M target vertices).  Pi Phi2 is
    ops.apply on Phi2 cast to fp32 (dvm_softcorr_apply_f32 takes any number of channels: no slicing), the projection
    ops.basis_project.  A slot with an index outside [0, M) adds nothing.  Forward only: no gradient flows into pi_val."""
    phi2 = basis_tgt.evecs
    M = phi2.shape[1]
    ix = pi_idx.long()
    ok = (ix >= 0) & (ix < M)
    val = torch.where(ok, pi_val.detach().float(), torch.zeros((), dtype=torch.float32, device=pi_val.device))
    idx = torch.where(ok, ix, torch.zeros_like(ix)).int()
    return ops.basis_project(basis_src.evecs, basis_src.mass, ops.apply(val, idx, phi2.float()))


def zoomout(T, basis_src, basis_tgt, k_init, k_final=None, k_step=1, n_inter=1, solve="adjoint", check=True):
    """ZoomOut spectral refinement of a hard map T (B,N) int32 into the target (the reference's Tools/utils.py::zo_fmap; not in its
    loss) over the two shapes' ops.Eigenbasis: for k = k_init, k_init + k_step, .. below k_final the map is turned into a k x k
    functional map (ops.fmap_from_pmap, with basis_src's mass for solve="adjoint") and back into a map (ops.fmap_to_pmap) ->
    ops.ZoomOut (C (B,k_final,k_final) float64, the map T that produced it, info).  k_final defaults to the smaller basis.  The point
    map of the returned C is pointwise_map(C, basis_src, basis_tgt).  Forward only.  dvm_zoomout_f64."""
    if k_final is None:
        k_final = min(basis_src.k, basis_tgt.k)
    return ops.zoomout(basis_src.evecs, basis_src.mass, basis_tgt.evecs, T, k_init, k_final, k_step=k_step, n_inter=n_inter, solve=solve,
                       check=check)


def pointwise_map(C, basis_src, basis_tgt, want_dist=False):
    """The point map of a functional map C (B,k,k) between two ops.Eigenbasis (the reference's fMap2pMap): T (B,N) int32, the target
    vertex whose row of Phi_tgt[:, :k] C^T lies nearest to the source vertex's row of Phi_src[:, :k]; with want_dist also the
    squared distances.  ops.fmap_to_pmap."""
    return ops.fmap_to_pmap(basis_src.evecs, basis_tgt.evecs, C, want_dist=want_dist)


class GraphDeformLoss_Neural(nn.Module):
    partial_variant = False

    def __init__(self, k_deform=10, w_dist=1, w_map=1, k_dist=1000, N_dist=1000, partial=False, w_deform=1, w_img=1,
                 w_rank=1, w_self_rec=1, w_cd=1, w_arap=1, save_name=None, dump=False, graph_cache=None):
        super().__init__()
        # opt-in per-shape graph cache: a dict filled by geometry(..., shape_ids=...); the reference rebuilds
        # every graph on every call (models/loss.py:1325-1337).  Entries are keyed by (shape id, FPS start, point count,
        # graph_metric, graph_ring_metric)
        self.graph_cache = graph_cache
        self.graph_cache_max = 4096     # entries kept when graph_cache is an OrderedDict (~60 KB each at N = 2048)
        self.device = 'cuda:0'
        self.w_dist, self.w_map, self.w_deform, self.w_self_rec = w_dist, w_map, w_deform, w_self_rec
        self.w_cd, self.w_arap, self.w_rank, self.w_img = w_cd, w_arap, w_rank, w_img
        self.k_dist, self.N_dist, self.k_deform = k_dist, N_dist, k_deform
        self.dist_loss = self.deform_loss = self.self_rec_loss = self.img_loss = self.rank_loss = self.map_loss = 0
        self.partial = partial
        self.frob_loss = FrobeniusLoss()
        self.save_name = save_name
        self.dump = dump  # the reference writes 4 OFF files + a print per deform() call; opt-in here
        # training, equal point counts: the deformation part as ONE native autograd node (nn_ops.criterion_train); False = the
        # autograd path over the per-op nodes (the two agree to fp32 rounding, tests/test_gpu_criterion_native.py)
        self.native_train = True
        # opt-in: Pi from this many Sinkhorn iterations (ops.sinkhorn / nn_ops.sinkhorn_topk; not in the reference) in place of the
        # row softmax.  0 = the reference's operator, on exactly the paths above; > 0 leaves the native nodes (they have the row
        # softmax built in) for the per-op paths
        self.sinkhorn_iters = 0
        # with sinkhorn_iters > 0: (tau_row, tau_col) of the unbalanced operator (ops.sinkhorn_unbalanced: rows without a partner
        # keep little mass); None or (1, 1) = the balanced operator, on exactly the paths of sinkhorn_iters alone
        self.sinkhorn_tau = None
        # opt-in: weight of the cycle term ||Pi12 Pi21 - I||_F (cycle_term; not in the reference), which ties the two directions'
        # correspondences together and, unlike the rank term, takes N != M.  0 = off, on exactly the paths above; > 0 takes the
        # paths w_rank > 0 takes (the term stays on the per-op path)
        self.w_cycle = 0
        self.cycle_loss = 0
        # opt-in: weight of the geodesic distortion term ||Pi D_target Pi^T - D_source||_F of both directions (distortion_term; not
        # in the reference), on the symmetrised dist1 / dist2 the criterion is handed anyway; N != M is allowed.  0 = off, on
        # exactly the paths above; > 0 takes the paths w_cycle > 0 takes
        self.w_distortion = 0
        self.distortion_loss = 0
        # opt-in: weight of the Dirichlet energy of both directions' pulled-back coordinates (dirichlet_term; not in the reference):
        # Pi12 with verts2 under the operator of verts1 built from idx11, the xyz kNN list the criterion holds anyway
        # (ops.knn_laplacian, dirichlet_mode "stretch" or "uniform"), and the mirror image with idx22; each E / norm, 1 for a map
        # that keeps local lengths.  0 = off, on exactly the paths above; > 0 takes the paths w_distortion > 0 takes
        self.w_dirichlet = 0
        self.dirichlet_mode = "stretch"
        self.dirichlet_loss = 0
        # opt-in: "geodesic" skins every vertex to the 3 nodes nearest by the distance matrices the criterion is handed (dist1 /
        # dist2; ops.dg_build_geod — what the reference's construct_graph_euclidean does with a `geod` that is not cdist);
        # graph_ring_metric = "geodesic" takes the ARAP rings from them as well.  Nodes (Euclidean FPS) and sigma stay.
        # "euclidean" = the graphs of ops.dg_build, on exactly the paths above; everything behind geometry() is the same either way
        self.graph_metric = "euclidean"
        self.graph_ring_metric = "euclidean"

    def _graph_kind(self):
        """(graph_metric, graph_ring_metric), checked: part of every graph-cache key."""
        if self.graph_metric not in ("euclidean", "geodesic") or self.graph_ring_metric not in ("euclidean", "geodesic"):
            raise ValueError("graph_metric / graph_ring_metric must be 'euclidean' or 'geodesic' (got %r, %r)"
                             % (self.graph_metric, self.graph_ring_metric))
        if self.graph_metric == "euclidean" and self.graph_ring_metric != "euclidean":
            raise ValueError("graph_ring_metric = 'geodesic' needs graph_metric = 'geodesic'")
        return self.graph_metric, self.graph_ring_metric

    def _identity6(self, device):
        """[1,0,0,0,1,0]: the identity rotation in the 6D parametrisation (models/loss.py:1258-1262), made once per device."""
        key = str(device)
        cache = self.__dict__.setdefault("_iden6", {})
        if key not in cache:
            cache[key] = torch.tensor([1, 0, 0, 0, 1, 0], dtype=torch.float32, device=device)
        return cache[key]

    # ---- pieces with the reference's names -------------------------------------------------
    def chamfer_loss(self, pos1, pos2):
        d1, d2, _, _ = ops.chamfer(pos1, pos2, want_idx=False)
        if self.partial_variant:  # one-sided: the smaller cloud's side (models/loss.py:875-880)
            return torch.mean(d1 if d1.shape[1] <= d2.shape[1] else d2)
        return torch.mean(d1) + torch.mean(d2)

    def topk_pi(self, A):
        if isinstance(A, SparsePi):
            return A
        v, i = torch.topk(A, 10, dim=-1)
        return torch.zeros_like(A).scatter_(-1, i, v)

    def _build_graphs(self, verts, starts, dist=None):
        """ops.dg_build, or under graph_metric = "geodesic" ops.dg_build_geod on the shapes' distance matrices dist (B,N,N)."""
        metric, ring_metric = self._graph_kind()
        if metric == "euclidean":
            return ops.dg_build(verts, starts)
        if dist is None:
            raise ValueError("graph_metric = 'geodesic' needs the shapes' distance matrices")
        return ops.dg_build_geod(verts, dist, starts, ring_metric)

    def deformation_graph_node(self, verts1, starts=None, dist=None):
        """-> (nodes_idx (B,Nn) float like the reference, [graph objects], batched graph dict)."""
        B, N, _ = verts1.shape
        if starts is None:  # one torch.randint(0,N,(1,)) per batch element, in order, like the reference
            starts = torch.cat([torch.randint(0, N, (1,), dtype=torch.long) for _ in range(B)])
        g = self._build_graphs(verts1, _host_draw_to_device(starts, verts1.device), dist)
        dg_list = [DeformationGraph_geod.from_batch(g, b, verts1[b]) for b in range(B)] if self.dump else []
        return g["nodes_idx"].float(), dg_list, g

    def _dist_term(self, feat, dist, anchors):
        return ops.dist_loss(feat, dist, anchors, self.k_dist).sum()

    def _direction(self, feat1, feat2, verts1, verts2, alpha, g1, deformer, idx11, idx22):
        """deform() of the reference for one direction -> (map_sum (B,), cd_warp, arap_sum, cd_self, extras)."""
        if self.sinkhorn_iters > 0 and _relaxed(self.sinkhorn_tau):
            pval, pidx = ops.sinkhorn_unbalanced(feat1, feat2, alpha, self.sinkhorn_iters, self.sinkhorn_tau, topk=10)[:2]
        elif self.sinkhorn_iters > 0:
            pval, pidx, _, _ = ops.sinkhorn(feat1, feat2, alpha, self.sinkhorn_iters, topk=10)
        else:
            pval, pidx, _, _ = ops.softcorr(feat1, feat2, alpha, topk=10, stats=False)
        verts12 = ops.apply(pval, pidx, verts2)
        def9 = deformer.forward_sparse(feat1, feat2, verts1, verts12, idx11, idx22, pval, pidx, g1["nodes_idx"])
        R = rotation_6d_to_matrix(def9[..., 3:] + self._identity6(def9.device))
        warped, arap, _ = ops.dg_warp_arap(verts1, g1, R, def9[..., :3].contiguous())
        cd_warp = self.chamfer_loss(warped, verts2)
        cd_self = self.chamfer_loss(verts12, verts2)
        map_sum = ops.map_term(verts12, verts2, idx11, idx22, pval, pidx) if (self.w_map > 0 and not self.partial_variant) else None
        return map_sum, cd_warp, arap.sum(), cd_self, dict(warped=warped, verts12=verts12, pval=pval, pidx=pidx)

    def _chamfer_train(self, a, b, per_pair=False):
        d1, d2 = nn_ops.chamfer_nn(a, b)
        if per_pair:   # (B,2): the two sides' means of every pair (the batch mean of each column is torch.mean(d*))
            return torch.stack([d1.mean(1), d2.mean(1)], 1)
        if self.partial_variant:
            return torch.mean(d1 if d1.shape[1] <= d2.shape[1] else d2)
        return torch.mean(d1) + torch.mean(d2)

    def _dist_term_train(self, feat, dist, anchors):
        """dist-loss term with autograd (HIP forward, HIP weights + GEMM backward)."""
        return nn_ops.dist_loss(feat, dist, anchors, self.k_dist).sum()

    def _direction_train(self, feat1, feat2, verts1, verts2, alpha, g1, deformer, idx11, idx22, per_pair=False):
        """deform() with autograd (models/loss.py:1228-1296).  per_pair: Chamfer terms as (B,2) per-pair side means and ARAP as (B,)
        instead of batch scalars (for a caller that has merged several calls into one batch)."""
        B, N, _ = verts1.shape
        M = verts2.shape[1]
        if (self.native_train and self.sinkhorn_iters <= 0 and not per_pair and not self.dump and self.w_rank <= 0 and self.w_cycle <= 0 and self.w_distortion <= 0 and self.w_dirichlet <= 0 and feat1.is_cuda and feat1.dtype == torch.float32
                and feat2.dtype == torch.float32 and feat1.shape[-1] == 128 and 64 <= N <= 8192 and 64 <= M <= 8192 and self.k_deform <= 16
                and idx11.shape[-1] == self.k_deform and all(torch.is_tensor(g1[k]) for k in ("nodes_idx", "one_ring", "infl_idx", "weights"))
                and all(p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() for p in deformer.parameters())):
            # this direction as ONE native autograd node (sources of N, targets of M points: the partial-shape configs, whose directions
            # cannot be merged); the reductions below are those of the per-op path, on the node's table of per-pair terms
            from dvm.ops import DEFORMER_KEYS
            named = dict(deformer.named_parameters())
            with_map = self.w_map > 0 and not self.partial_variant
            meta = (verts1, verts2, {k: g1[k] for k in ("nodes_idx", "one_ring", "infl_idx", "weights")}, idx11, idx22, alpha, 10, with_map)
            terms = nn_ops.criterion_dir_train(meta, feat1, feat2, [named[k] for k in DEFORMER_KEYS])
            tm = terms.mean(0)
            if self.partial_variant:   # one-sided Chamfer: the smaller cloud's side (models/loss.py:875-880)
                cd_warp, cd_self = (tm[1], tm[3]) if N <= M else (tm[2], tm[4])
            else:
                cd_warp, cd_self = tm[1] + tm[2], tm[3] + tm[4]
            return (terms[:, 0] if with_map else None), cd_warp, terms[:, 5].sum(), cd_self, None
        if self.sinkhorn_iters > 0 and _relaxed(self.sinkhorn_tau):
            pval, pidx, _ = nn_ops.sinkhorn_unbalanced_topk(feat1, feat2, alpha, self.sinkhorn_iters, self.sinkhorn_tau, topk=10)
        elif self.sinkhorn_iters > 0:
            pval, pidx = nn_ops.sinkhorn_topk(feat1, feat2, alpha, self.sinkhorn_iters, 10)
        else:
            pval, pidx = nn_ops.softcorr_topk(feat1, feat2, alpha, 10)
        verts12 = nn_ops.sparse_apply(pval, pidx, verts2)
        g1p = nn_ops.pool_rows(feat1, idx11, deformer.conv_layer.weight, deformer.conv_layer.bias)
        g2p = nn_ops.pool_rows(feat2, idx22, deformer.conv_layer.weight, deformer.conv_layer.bias)
        g2t = nn_ops.sparse_apply(pval, pidx, g2p)
        # the rows at the graph nodes: index_select on the flattened batch (whole rows, ~10 us per call and for its index_add_
        # backward) instead of torch.gather with an expanded index (element-wise: 50 - 90 us per call at 16 x 1024 x 128, and as
        # much again for the scatter_add of its backward); the nodes of a shape are distinct, so the backward adds nothing twice
        nodes = g1["nodes_idx"].long()
        flat = (nodes + torch.arange(B, device=nodes.device).unsqueeze(1) * N).reshape(-1)
        pick = lambda t: t.reshape(B * N, t.shape[-1]).index_select(0, flat).view(B, nodes.shape[1], t.shape[-1])  # noqa: E731
        z = torch.cat([pick(verts1), pick(g1p), pick(verts12), pick(g2t)], dim=-1)
        def9 = deformer.deformation_decoder_layer(z)
        R = nn_ops.rot6d(def9[..., 3:] + self._identity6(def9.device))
        warped, arap = nn_ops.dg_warp_arap(verts1, g1, R, def9[..., :3])
        cd_warp = self._chamfer_train(warped, verts2, per_pair)
        cd_self = self._chamfer_train(verts12, verts2, per_pair)
        map_sum = None
        if self.w_map > 0 and not self.partial_variant:
            lhs = nn_ops.gather_rows(verts12, idx11)                                   # (B,N,k,3)
            v2n = nn_ops.gather_rows(verts2, idx22).reshape(B, verts2.shape[1], -1)    # (B,M,k*3)
            rhs = nn_ops.sparse_apply(pval, pidx, v2n).view(B, N, -1, 3)
            map_sum = ((lhs - rhs) ** 2).sum(dim=(1, 2, 3))
        return map_sum, cd_warp, (arap if per_pair else arap.sum()), cd_self, dict(warped=warped, verts12=verts12, pval=pval, pidx=pidx)

    def _term_weights(self, B, N, device, with_dist=False):
        """(2B*7, 7) matrix taking the native node's table [map, cd_warp (2), cd_self (2), arap, dist] x 2B (directional pairs / shapes) to
        [deform_loss, map_loss, self_rec_loss, sum-type share, mean-type share, total, dist_loss] (models/loss.py:1398-1437;
        data_parallel_loss)."""
        key = (B, N, str(device), self.w_cd, self.w_arap, self.w_deform, self.w_map, self.w_self_rec, self.w_dist if with_dist else 0)
        cache = self.__dict__.setdefault("_term_w", {})
        if key not in cache:
            half = N * self.w_deform / 2        # (non-partial criterion: scale = N)
            row = torch.zeros(7, 7, dtype=torch.float64)
            row[1, 0] = row[2, 0] = self.w_cd * half / B            # Chamfer: mean over the B pairs of each direction
            row[5, 0] = self.w_arap * half                          # ARAP: sum over the pairs
            row[5, 3] = self.w_arap * half
            row[1, 4] = row[2, 4] = self.w_cd * half / B
            if self.w_map > 0:
                row[0, 1] = row[0, 4] = self.w_map / (3 * B) / 2    # FrobeniusLoss: sum over (N,k), mean over (B,3)
            if self.w_self_rec > 0:
                row[3, 2] = row[4, 2] = row[3, 4] = row[4, 4] = N * self.w_self_rec / 2 / B
            if with_dist:
                row[6, 6] = row[6, 3] = self.w_dist                 # dist term: sum over all 2B shapes
            row[:, 5] = row[:, 0] + row[:, 1] + row[:, 2] + row[:, 6]
            cache[key] = row.repeat(2 * B, 1).float().to(device)
        return cache[key]

    def _dump(self, ex, verts1, verts2, n, cd, arap):
        print("Rand:%s, Deform_Result: cd_loss:%s, arap_loss:%s" % (n, cd, arap))
        path = 'visual_result/' + str(self.save_name)
        os.makedirs(path, exist_ok=True)
        for name, t in (("deform_", ex["warped"][0]), ("target_", verts2[0]), ("source_", verts1[0]),
                        ("pi_verts2_", ex["verts12"][0])):
            save_off_file(path + '/' + name + n + '.off', t.detach().cpu().numpy())

    # ---- forward ------------------------------------------------------------------------------
    def _cached_side(self, verts, starts, ids, dist=None):
        """Graph + xyz kNN of a batch of shapes assembled from per-shape cache entries; shapes not yet seen are built in ONE
        batched call and stored.  Bit-identical to building the batch (every kernel of the build works per shape).  The keys
        carry (graph_metric, graph_ring_metric): graphs of different kinds never mix."""
        B, N, _ = verts.shape
        kind = self._graph_kind()
        keys = [(ids[b], int(starts[b]), N) + kind for b in range(B)]
        miss = [b for b in range(B) if keys[b] not in self.graph_cache]
        if miss:
            sel = torch.as_tensor(miss, device=verts.device)
            sub = verts.index_select(0, sel).contiguous()
            st = torch.as_tensor([int(starts[b]) for b in miss], dtype=torch.int32)
            g = self._build_graphs(sub, _host_draw_to_device(st, verts.device), dist.index_select(0, sel) if dist is not None else None)
            idx = ops.knn_cdist(sub, sub, self.k_deform)
            for j, b in enumerate(miss):
                ent = {name: t[j].clone() for name, t in g.items()}
                ent["_idx"] = idx[j].clone()
                self.graph_cache[keys[b]] = ent
        ents = [self.graph_cache[k] for k in keys]
        if hasattr(self.graph_cache, "move_to_end"):   # an OrderedDict is kept least-recently-used first and bounded
            for k in keys:
                self.graph_cache.move_to_end(k)
            while len(self.graph_cache) > max(self.graph_cache_max, B):
                self.graph_cache.popitem(last=False)
        g = {name: torch.stack([e[name] for e in ents]) for name in ents[0] if name != "_idx"}
        return g, torch.stack([e["_idx"] for e in ents])

    def geometry(self, verts1, verts2, fps_starts=None, shape_ids=None, dists=None):
        """The part of the criterion that depends on the COORDINATES only — both shapes' deformation graphs (FPS nodes, node
        rings, skinning) and their xyz kNN — as (g1, g2, idx11, idx22).  forward() calls it itself; a driver may call it
        earlier, on another stream, while the network is still computing the features (FPS is a chain of N/2 dependent
        steps on one workgroup per shape: 0.65 ms during which nothing else of the criterion can start), and hand the
        result to forward(geometry=...).  The FPS start indices are drawn here, in the reference's order.
        dists = (dist1 (B,N,N), dist2 (B,M,M)): the matrices that skin the graphs under graph_metric = "geodesic" (unused
        otherwise)."""
        B, N, _ = verts1.shape
        M = verts2.shape[1]
        geod = self._graph_kind()[0] == "geodesic"
        if geod and (dists is None or dists[0] is None or dists[1] is None):
            raise ValueError("graph_metric = 'geodesic' needs both distance matrices (dists=(dist1, dist2))")
        d1, d2 = dists if geod else (None, None)
        s1, s2 = fps_starts if fps_starts is not None else (None, None)
        k = self.k_deform
        if self.graph_cache is not None and shape_ids is not None and not self.dump:
            # the cache needs the start index of every shape on the host: drawn here in the reference's order when not given
            if s1 is None:
                s1 = torch.cat([torch.randint(0, N, (1,), dtype=torch.long) for _ in range(B)])
            if s2 is None:
                s2 = torch.cat([torch.randint(0, M, (1,), dtype=torch.long) for _ in range(B)])
            if not any(torch.is_tensor(t) and t.is_cuda for t in (s1, s2)):
                g1, idx11 = self._cached_side(verts1, list(torch.as_tensor(s1).reshape(-1).tolist()), list(shape_ids[0]), d1)
                g2, idx22 = self._cached_side(verts2, list(torch.as_tensor(s2).reshape(-1).tolist()), list(shape_ids[1]), d2)
                return g1, g2, idx11, idx22
        if verts1.shape == verts2.shape and not self.dump:
            # both shapes' graphs and xyz-kNN in ONE batched call each (FPS is a sequential 1-workgroup-per-shape
            # kernel: 2B shapes cost what B do); the start indices are drawn in the reference's order
            if s1 is None:
                s1 = torch.cat([torch.randint(0, N, (1,), dtype=torch.long) for _ in range(B)])
            if s2 is None:
                s2 = torch.cat([torch.randint(0, M, (1,), dtype=torch.long) for _ in range(B)])
            both = torch.cat([verts1, verts2], dim=0)
            if geod:   # one call per side: joining the two (B,N,N) matrices would copy them (every kernel of the build works per shape)
                _, _, g1 = self.deformation_graph_node(verts1, s1, d1)
                _, _, g2 = self.deformation_graph_node(verts2, s2, d2)
            else:
                _, _, g = self.deformation_graph_node(both, torch.cat([torch.as_tensor(s1).reshape(-1), torch.as_tensor(s2).reshape(-1)]))
                g1 = {key: (v[:B] if torch.is_tensor(v) and v.dim() > 0 and v.shape[0] == 2 * B else v) for key, v in g.items()}
                g2 = {key: (v[B:] if torch.is_tensor(v) and v.dim() > 0 and v.shape[0] == 2 * B else v) for key, v in g.items()}
            idx = ops.knn_cdist(both, both, k)
            idx11, idx22 = idx[:B], idx[B:]
        else:
            _, _, g1 = self.deformation_graph_node(verts1, s1, d1)
            _, _, g2 = self.deformation_graph_node(verts2, s2, d2)
            idx11, idx22 = ops.knn_cdist(verts1, verts1, k), ops.knn_cdist(verts2, verts2, k)
        return g1, g2, idx11, idx22

    def forward(self, feat1, feat2, dist1, dist2, verts1, verts2, alpha_i, deformer, fps_starts=None, anchors=None, geometry=None,
                shape_ids=None):
        """-> (loss, dist_loss, deform_loss, map_loss, self_rec_loss), like the reference.
        fps_starts=(s1 (B,), s2 (B,)) and anchors=(a1, a2) pin the draws the reference makes at random; geometry = what
        self.geometry(verts1, verts2, fps_starts) returned, when the caller made it ahead of time; shape_ids = (ids of the B
        source shapes, ids of the B target shapes) lets a criterion built with graph_cache={} reuse per-shape graphs."""
        loss = 0
        native = False
        self._sum_part = self._mean_part = 0
        B, N, _ = verts1.shape
        M = verts2.shape[1]
        if self.w_distortion > 0 and (dist1 is None or dist2 is None):
            raise ValueError("w_distortion > 0 needs both distance matrices (dist1, dist2)")
        if self._graph_kind()[0] == "geodesic" and (dist1 is None or dist2 is None):
            raise ValueError("graph_metric = 'geodesic' needs both distance matrices (dist1, dist2)")
        train = torch.is_grad_enabled() and (feat1.requires_grad or feat2.requires_grad or
                                             any(p.requires_grad for p in deformer.parameters()))
        dist_term = self._dist_term_train if train else self._dist_term
        direction = self._direction_train if train else self._direction
        # The dist term and the two directions of the deformation part are independent of each other: on a GPU they run on
        # three streams (forked from / joined into the caller's stream; autograd replays each branch's backward on the stream its
        # forward ran on).  At 8 pairs their kernels fill a fraction of the chip each.
        par = feat1.is_cuda and not self.dump
        cur = torch.cuda.current_stream(feat1.device) if par else None
        side = _crit_streams(feat1.device, cur) if par else None

        def on(k, fn):
            if not par:
                return fn()
            st = side[k]
            st.wait_stream(cur)
            with torch.cuda.stream(st):
                return fn()

        def joined(k, out):
            if par:
                cur.wait_stream(side[k])
                for t in (out if isinstance(out, (tuple, list)) else (out,)):
                    for u in (t.values() if isinstance(t, dict) else (t,)):
                        if torch.is_tensor(u) and u.is_cuda:
                            u.record_stream(cur)
            return out
        if self.w_dist > 0:
            if anchors is None:
                anchors = (random.sample(range(dist1.shape[1]), self.N_dist), random.sample(range(dist2.shape[1]), self.N_dist))
            # (device tensors pass through untouched: no host-to-device copy inside a captured step)
            a1, a2 = _host_draw_to_device(anchors[0], feat1.device), _host_draw_to_device(anchors[1], feat2.device)
        native_dist = False
        if self.w_deform > 0 or not self.partial_variant:
            g1, g2, idx11, idx22 = geometry if geometry is not None else self.geometry(verts1, verts2, fps_starts, shape_ids, (dist1, dist2))
            merged = (train and N == M and not self.dump and not self.partial_variant and self.w_rank <= 0 and self.w_cycle <= 0
                      and self.w_distortion <= 0 and self.w_dirichlet <= 0 and all(torch.is_tensor(g1[k]) for k in g1))
            native = (merged and self.native_train and self.sinkhorn_iters <= 0 and feat1.is_cuda and feat1.dtype == torch.float32 and feat1.shape[-1] == 128 and N % 4 == 0
                      and 64 <= N <= 8192 and self.k_deform <= 16 and idx11.shape[-1] == self.k_deform
                      and all(p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() for p in deformer.parameters()))
            # ... and the dist term of all 2B shapes inside the same node (on its helper stream)
            native_dist = (native and self.w_dist > 0 and self.k_dist <= 512 and a1.numel() == a2.numel() and a1.numel() <= N
                           and all(d.is_cuda and d.dtype == torch.float32 and d.is_contiguous() and tuple(d.shape) == (B, N, N) for d in (dist1, dist2)))
        if self.w_dist > 0 and not native_dist:
            dterm = on(0, lambda: (dist_term(feat1, dist1, a1) + dist_term(feat2, dist2, a2)) * self.w_dist)
        if self.w_deform > 0 or not self.partial_variant:
            if native:
                # Both directions of deform() for the B pairs = 2B directional pairs [(1 -> 2) x B | (2 -> 1) x B] through ONE native
                # autograd node; its table of per-pair terms is weighted by one small matrix product (the reductions of
                # models/loss.py:1413-1432 are linear in the table: sums over the pairs for ARAP, batch means for the rest)
                from dvm.ops import DEFORMER_KEYS
                named = dict(deformer.named_parameters())
                gj = {k: _joint(g1[k], g2[k]) for k in ("nodes_idx", "one_ring", "infl_idx", "weights")}
                dmeta = (dist1, dist2, ops._i(a1), ops._i(a2), self.k_dist) if native_dist else None
                meta = (_joint(verts1, verts2), gj, _joint(idx11, idx22), alpha_i, 10, bool(self.w_map > 0), dmeta)
                terms = nn_ops.criterion_train(meta, _joint(feat1, feat2), [named[k] for k in DEFORMER_KEYS])
                parts = terms.reshape(-1) @ self._term_weights(B, N, terms.device, native_dist)
                n12 = str(random.randint(0, 10))
                n21 = str(random.randint(0, 10))
            elif merged:
                # Both directions are the SAME function of (source, target): with equal point counts they run as ONE batch of 2B
                # pairs — [(1 -> 2) x B | (2 -> 1) x B] — through every kernel of deform() and its backward: half the launches of two
                # calls (which at 8 pairs fill a fraction of the chip each).  Chamfer / self-reconstruction are means over the batch
                # and enter the loss as c12 + c21 = 2 mean over both; ARAP and the map term are sums.
                cat = lambda u, v: torch.cat([u, v], 0)  # noqa: E731
                gm = {k: cat(g1[k], g2[k]) for k in g1}
                mm_, cm, am, sm, exm = direction(cat(feat1, feat2), cat(feat2, feat1), cat(verts1, verts2), cat(verts2, verts1), alpha_i, gm,
                                                 deformer, cat(idx11, idx22), cat(idx22, idx11), per_pair=True)
                m12, m21 = (mm_[:B], mm_[B:]) if mm_ is not None else (None, None)
                c12, c21 = cm[:B].mean(0).sum(), cm[B:].mean(0).sum()
                s12, s21 = sm[:B].mean(0).sum(), sm[B:].mean(0).sum()
                a12, a21 = am[:B].sum(), am[B:].sum()
                ex12 = {k: v[:B] for k, v in exm.items()}
                ex21 = {k: v[B:] for k, v in exm.items()}
                n12 = str(random.randint(0, 10))
                n21 = str(random.randint(0, 10))
            else:
                r21 = on(1, lambda: direction(feat2, feat1, verts2, verts1, alpha_i, g2, deformer, idx22, idx11))
                m12, c12, a12, s12, ex12 = direction(feat1, feat2, verts1, verts2, alpha_i, g1, deformer, idx11, idx22)
                n12 = str(random.randint(0, 10))
                m21, c21, a21, s21, ex21 = joined(1, r21)
                n21 = str(random.randint(0, 10))
        if self.w_dist > 0 and not native_dist:
            self.dist_loss = joined(0, dterm)
            loss = loss + self.dist_loss
            self._sum_part = self._sum_part + self.dist_loss
        if (self.w_deform > 0 or not self.partial_variant) and native:
            # parts = [deform, map, self_rec, the sum-type share, the mean-type share, their total, dist] (the last three with the dist term
            # when the node computed it)
            if native_dist:
                self.dist_loss = parts[6]
            self.deform_loss = parts[0]
            if self.w_map > 0:
                self.map_loss = parts[1]
            if self.w_self_rec > 0:
                self.self_rec_loss = parts[2]
            loss = loss + parts[5]
            self._sum_part = self._sum_part + parts[3]
            self._mean_part = self._mean_part + parts[4]
        elif self.w_deform > 0 or not self.partial_variant:
            cross12 = c12 * self.w_cd + a12 * self.w_arap
            cross21 = c21 * self.w_cd + a21 * self.w_arap
            if self.dump:
                self._dump(ex12, verts1, verts2, n12, c12 * self.w_cd, a12 * self.w_arap)
                self._dump(ex21, verts2, verts1, n21, c21 * self.w_cd, a21 * self.w_arap)
            scale = 1 if self.partial_variant else N
            self.deform_loss = (cross12 + cross21) * scale * self.w_deform / 2
            loss = loss + self.deform_loss
            self._sum_part = self._sum_part + (a12 + a21) * (self.w_arap * scale * self.w_deform / 2)
            self._mean_part = self._mean_part + (c12 + c21) * (self.w_cd * scale * self.w_deform / 2)
            if self.w_map > 0 and not self.partial_variant:
                # FrobeniusLoss: sum over (N,k), mean over (B,3)
                self.map_loss = self.w_map * (m12.sum() / (3 * B) + m21.sum() / (3 * B)) / 2
                loss = loss + self.map_loss
                self._mean_part = self._mean_part + self.map_loss
            if self.w_self_rec > 0:
                self.self_rec_loss = (s12 + s21) * scale * self.w_self_rec / 2
                loss = loss + self.self_rec_loss
                self._mean_part = self._mean_part + self.self_rec_loss
            if self.w_rank > 0:
                if N != M:   # the reference compares the M x M product of the reverse direction with an N x N identity
                    raise ValueError("w_rank > 0 needs N == M (got %d, %d), as in the reference" % (N, M))
                self.rank_loss = self._pair_mean_term(self.w_rank, rank_term(ex12["pval"], ex12["pidx"], M), rank_term(ex21["pval"], ex21["pidx"], N))
                loss = loss + self.rank_loss
            if self.w_cycle > 0:
                self.cycle_loss = self._pair_mean_term(self.w_cycle, cycle_term(ex12["pval"], ex12["pidx"], ex21["pval"], ex21["pidx"]),
                                                       cycle_term(ex21["pval"], ex21["pidx"], ex12["pval"], ex12["pidx"]))
                loss = loss + self.cycle_loss
            if self.w_distortion > 0:
                sym1, sym2 = _symmetrised(dist1), _symmetrised(dist2)   # once per call, for both directions
                self.distortion_loss = self._pair_mean_term(self.w_distortion, distortion_term(ex12["pval"], ex12["pidx"], sym1, sym2, symmetric=True),
                                                            distortion_term(ex21["pval"], ex21["pidx"], sym2, sym1, symmetric=True))
                loss = loss + self.distortion_loss
            if self.w_dirichlet > 0:
                op1, op2 = ops.knn_laplacian(verts1, idx11, self.dirichlet_mode), ops.knn_laplacian(verts2, idx22, self.dirichlet_mode)
                self.dirichlet_loss = self._pair_mean_term(self.w_dirichlet, dirichlet_term(ex12["pval"], ex12["pidx"], verts2, op1),
                                                           dirichlet_term(ex21["pval"], ex21["pidx"], verts1, op2))
                loss = loss + self.dirichlet_loss
        return loss, self.dist_loss, self.deform_loss, self.map_loss, self.self_rec_loss

    def _pair_mean_term(self, w, t12, t21):
        """A per-pair term of both directions (each (B,)) as the criterion counts it: the two batch means, weighted and halved; a
        mean-type term for data_parallel_loss."""
        term = (t12.mean() + t21.mean()) * w / 2
        self._mean_part = self._mean_part + term
        return term

    def data_parallel_loss(self, fraction):
        """The loss to back-propagate on ONE SHARD of a data-parallel batch (call after forward): the reference's
        criterion mixes reductions over the batch — the dist term and ARAP are SUMS over the pairs (models/loss.py:1392-1394,
        1269-1273), Chamfer / map / self-reconstruction / rank are MEANS (1216-1226, 476-482) — so with
        fraction = B_shard / B_global the sum-type terms enter as they are and the mean-type terms are weighted by the
        shard's share; the SUM of the shards' gradients (one all-reduce) is then the gradient of this same criterion
        evaluated on the whole batch by one process.  fraction = 1 gives the plain loss."""
        return self._sum_part + fraction * self._mean_part


class GraphDeformLoss_Neural_Partial(GraphDeformLoss_Neural):
    """Partial-shape variant: no map loss, one-sided Chamfer, no xN scaling (models/loss.py:986-1073)."""
    partial_variant = True
