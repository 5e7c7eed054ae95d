"""Shared by tests/test_gpu_distortion_term.py and tests/test_distortion_term_cpu.py: the plantings of the distortion-term tests
(rank_term_ref's generators plus isometries) and the float64 evaluation of the definition they are judged against.

Reference: val.double() scattered into a dense P (N x M), S = P D2 P^T, R = S - D1, F = ||R||_F, float64 autograd for d F / d val
(torch.norm: a zero gradient at F = 0).  All inputs are non-negative; D1 and D2 are exactly symmetric in fp32 with a zero diagonal.
With u = 2^-24 the bars are

    loss      |F^ - F|  <=  4 (2k + 2) u ||S||_F  +  2 u F
    g[i,t]    |g^ - g|  <=  4 (2k + 2) u (A + |g| (||S||_F + ||D1||_F) / F)  +  2 u |g|,   A = (2/F) (((S + D1) P) D2^T)[i, idx[i,t]]

Where they come from (the kernel's chains, dvm_distortion.hip): u_i[m] = sum_t val[i,t] D2[idx[i,t], m] is an fp32 fma chain of k
non-negative terms in slot order, so it carries a relative error of at most k u; S[i,j] = sum_s val[j,s] u_i[idx[j,s]] is a second
chain of k non-negative terms over those values: every entry of S^ is within 2 k u S[i,j] of S[i,j] (first order).  The residual
S^ - D1 is formed in float64 from two fp32 numbers and its squares are summed in float64, so |F^ - F| <= ||S^ - S||_F <= 2 k u ||S||_F;
F^2 passes through fp32 once and the loss is rounded to fp32: the 2 u F.  The factor 4 and the + 2 are the slack the sibling terms
keep (rank_term_ref, cycle_term_ref: summation order, second-order terms).
The gradient is (2/F) times a sum over m and over the entries (j,s) of column m of D2[c,m] val[j,s] R[i,j].  Its R[i,j] comes from
S^ (absolute error 2 k u S[i,j]) and is kept as fp32 (u |R[i,j]|), and |R| <= S + D1 entry-wise, so the sum moves by at most
(2k + 1) u times the same sum with S + D1 in place of R: that is A.  The sum itself is exact to float64 (q in 64-bit fixed point,
at most N 2^-50 of a column's largest term; the dot with the row of D2 in float64).  The factor 1/F moves by |F^ - F| / F relative,
bounded by the loss bar over F, for which (||S||_F + ||D1||_F) / F is the cover the bar keeps; g is rounded to fp32 before and after
the scaling: the 2 u |g|.  At F = 0 loss and gradient are exactly 0.
An fp32 emulation of the two chains on the CPU (torch fp32 multiply-adds in slot order, float64 after them) sits at 1.2 % of the
bars at most on the plantings used here (k = 1 the largest, 0.1 - 0.6 % at k >= 10): a kernel near a bar has a bug."""
import torch

import frob_term_common as T
import rank_term_ref as R

U = T.U


def distances(gen, B, n):
    """(B,n,n) fp32 Euclidean distances of seeded random points in the unit cube: exactly symmetric, zero diagonal."""
    pts = torch.rand(B, n, 3, generator=gen)
    d = torch.cdist(pts, pts)
    d = 0.5 * (d + d.transpose(1, 2))
    d.diagonal(dim1=1, dim2=2).zero_()
    return d.contiguous()


def plant(kind, gen, B, N, M, k):
    """(val, idx, D1, D2) with P "random" or "hubs" (rank_term_ref.plant_random / plant_hubs) and independent distance matrices."""
    make = {"random": R.plant_random, "hubs": R.plant_hubs}
    val, idx = make[kind](gen, B, N, M, k)
    return val, idx, distances(gen, B, N), distances(gen, B, M)


def _isometry(gen, B, N, k, row):
    """idx[i,t] = (pi(i) + t) mod N for a random permutation pi, D1 = D2[pi][:, pi]: slot 0 alone is an exact isometry"""
    D2 = distances(gen, B, N)
    perm = torch.stack([torch.randperm(N, generator=gen) for _ in range(B)])
    idx = ((perm[:, :, None] + torch.arange(k)[None, None, :]) % N).to(torch.int32).contiguous()
    D1 = torch.stack([D2[b][perm[b]][:, perm[b]] for b in range(B)]).contiguous()
    return row.expand(B, N, k).contiguous(), idx, D1, D2


def plant_exact_isometry(gen, B, N, k):
    """val = (1, 0, ...): S[i,j] = D2[pi(i), pi(j)] = D1[i,j] with no rounding anywhere, F is exactly 0 in fp32"""
    return _isometry(gen, B, N, k, T.exact_row(k))


def plant_near_isometry(gen, B, N, k):
    """val = (1 - 1e-3, 1e-3 / (k - 1), ...): F is a thousandth of ||S||_F, the cancellation case"""
    return _isometry(gen, B, N, k, T.near_row(k))


def dense_reference(val, idx, D1, D2, grad=True):
    """float64 evaluation of the definition on the CPU -> dict(F, S_fro, D1_fro (B,), and with grad g, A (B,N,k))."""
    v = val.detach().cpu().double().requires_grad_(grad)
    ix = idx.detach().cpu().long()
    d1, d2 = D1.detach().cpu().double(), D2.detach().cpu().double()
    B, N, _ = v.shape
    M = d2.shape[1]
    P = torch.zeros(B, N, M, dtype=torch.float64).scatter_add(-1, ix, v)
    S = P @ d2 @ P.transpose(1, 2)
    F = (S - d1).flatten(1).norm(dim=1)
    out = {"S_fro": S.detach().flatten(1).norm(dim=1), "D1_fro": d1.flatten(1).norm(dim=1), "F": F.detach()}
    if not grad:
        return out
    out["g"], = torch.autograd.grad(F.sum(), v)
    Fd = F.detach()[:, None, None]
    Q = (((S.detach() + d1) @ P.detach()) @ d2.transpose(1, 2)).gather(-1, ix)
    out["A"] = torch.where(Fd > 0, 2.0 * Q / Fd.clamp_min(1e-300), torch.zeros_like(Q))
    return out


def loss_bound(ref, k):
    return T.loss_bound(ref, 2 * k + 2, ref["S_fro"])


def grad_bound(ref, k):
    return T.grad_bound(ref, 2 * k + 2, ref["S_fro"] + ref["D1_fro"], ref["g"], ref["A"])
