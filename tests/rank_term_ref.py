"""Shared by tests/test_gpu_rank_term.py and tests/test_rank_term_cpu.py: the plantings of the rank-term tests and the float64
evaluation of the definition they are judged against.

Reference: pi_val.double() scattered into a dense P (N x M), S = P P^T, F = ||S - I_N||_F, float64 autograd for d F / d pi_val
(torch.norm: a zero gradient at F = 0).  With u = 2^-24 the bars are

    loss      |loss - F|  <=  4 (k + 2) u ||S||_F  +  2 u F
    gradient  |g^ - g|    <=  4 (k + 2) u (A + |g| ||S||_F / F)  +  2 u |g|     per element,
              A[i,t] = (2 / F) sum_i' (S_ii' + delta_ii') P[i', pi_idx[i,t]]

|F^ - F| <= ||S^ - S||_F, every entry of S a k-term fp32 dot of non-negative terms; the factor 4 covers the summation order, the
last term the fp32 output.  At F = 0 loss and gradient are exactly 0."""
import torch

import frob_term_common as T

U = T.U


def random_sets(gen, B, N, M, k):
    """k distinct columns per row, uniformly at random, as int32 (B,N,k)."""
    return torch.rand(B, N, M, generator=gen).argsort(-1)[..., :k].to(torch.int32).contiguous()


def plant_random(gen, B, N, M, k):
    val = torch.softmax(3.0 * torch.randn(B, N, k, generator=gen), -1)
    return val.contiguous(), random_sets(gen, B, N, M, k)


def plant_hubs(gen, B, N, M, k):
    """every row picks columns 0..k-1: k column lists of N entries, every other column empty"""
    val = torch.softmax(3.0 * torch.randn(B, N, k, generator=gen), -1)
    idx = torch.arange(k, dtype=torch.int32).expand(B, N, k).contiguous()
    return val.contiguous(), idx


def _shift_idx(B, N, M, k):
    return ((torch.arange(N)[:, None] + torch.arange(k)[None, :]) % M).to(torch.int32).expand(B, N, k).contiguous()


def plant_near_perm(B, N, M, k):
    """idx[i,t] = (i + t) mod M, val = (1 - 1e-3, 1e-3 / (k - 1), ...): F ~ 0.026, the diagonal residual dominates"""
    return T.near_row(k).expand(B, N, k).contiguous(), _shift_idx(B, N, M, k)


def plant_exact_perm(B, N, M, k):
    """the same indices, val = (1, 0, ...): P P^T = I exactly"""
    return T.exact_row(k).expand(B, N, k).contiguous(), _shift_idx(B, N, M, k)


def dense_reference(val, idx, M, grad=True):
    """float64 evaluation of the definition on the CPU -> dict(F (B,), S_fro (B,), g (B,N,k), A (B,N,k)) (g, A: grad=True only)."""
    v = val.detach().cpu().double().requires_grad_(grad)
    ix = idx.detach().cpu().long()
    B, N, k = v.shape
    P = torch.zeros(B, N, M, dtype=torch.float64).scatter_add(-1, ix, v)
    S = P @ P.transpose(1, 2)
    out = {"S_fro": S.detach().flatten(1).norm(dim=1)}
    if not grad:
        S = S.detach()
        S.diagonal(dim1=1, dim2=2).sub_(1.0)
        out["F"] = S.flatten(1).norm(dim=1)
        return out
    eye = torch.eye(N, dtype=torch.float64)
    F = (S - eye).flatten(1).norm(dim=1)
    g, = torch.autograd.grad(F.sum(), v)
    Fd = F.detach()
    out["F"], out["g"] = Fd, g
    Q = ((S.detach() + eye) @ P.detach()).gather(-1, ix)
    out["A"] = torch.where(Fd[:, None, None] > 0, 2.0 * Q / Fd[:, None, None].clamp_min(1e-300), torch.zeros_like(Q))
    return out


def loss_bound(ref, k):
    return T.loss_bound(ref, k + 2, ref["S_fro"])


def grad_bound(ref, k):
    return T.grad_bound(ref, k + 2, ref["S_fro"], ref["g"], ref["A"])
