"""Shared by tests/test_gpu_cycle_term.py and tests/test_cycle_term_cpu.py: the plantings of the cycle-term tests (rank_term_ref's
generators, paired) and the float64 evaluation of the definition they are judged against.

Reference: val12.double() / val21.double() scattered into dense P12 (N x M), P21 (M x N), C = P12 P21, F = ||C - I_N||_F, float64
autograd for d F / d val12 and d F / d val21 (torch.norm: a zero gradient at F = 0).  With u = 2^-24 and k = k12 the bars are

    loss      |loss - F|  <=  4 (k + 2) u ||C||_F  +  2 u F
    g12[i,t]  |g^ - g|    <=  4 (k + 2) u (A12 + |g| ||C||_F / F)  +  2 u |g|,   A12 = (1/F) ((C + I) P21^T)[i, idx12[i,t]]
    g21[j,s]  |g^ - g|    <=  4 (k + 2) u (A21 + |g| ||C||_F / F)  +  2 u |g|,   A21 = (1/F) (P12^T (C + I))[j, idx21[j,s]]

|F^ - F| <= ||C^ - C||_F, every entry of C a dot of at most k12 fp32 terms, each an fp32 product of non-negative values; the factor 4
covers the summation order, the last term the fp32 output.  A12 / A21 are the gradient's own sums with |R| <= C + I in place of R:
what an entry-wise relative error of C can move.  At F = 0 loss and gradients are exactly 0."""
import torch

import frob_term_common as T
import rank_term_ref as R

U = T.U


def plant_pair(kind12, kind21, gen, B, N, M, k12, k21):
    """(val12, idx12, val21, idx21) with each side "random" or "hubs" (rank_term_ref.plant_random / plant_hubs)."""
    make = {"random": R.plant_random, "hubs": R.plant_hubs}
    val12, idx12 = make[kind12](gen, B, N, M, k12)
    val21, idx21 = make[kind21](gen, B, M, N, k21)
    return val12, idx12, val21, idx21


def _inverse_idx(B, N, M, k):
    """idx12[i,t] = (i + t) mod M, idx21[j,s] = (j - s) mod N: slot 0 of both is the identity on the first min(N, M) points"""
    idx12 = ((torch.arange(N)[:, None] + torch.arange(k)[None, :]) % M).to(torch.int32).expand(B, N, k).contiguous()
    idx21 = ((torch.arange(M)[:, None] - torch.arange(k)[None, :]) % N).to(torch.int32).expand(B, M, k).contiguous()
    return idx12, idx21


def plant_near_inverse(B, N, M, k):
    """val = (1 - 1e-3, 1e-3 / (k - 1), ...) on both sides: at N == M, F ~ 0.026 and the diagonal residual dominates"""
    row = T.near_row(k)
    idx12, idx21 = _inverse_idx(B, N, M, k)
    return row.expand(B, N, k).contiguous(), idx12, row.expand(B, M, k).contiguous(), idx21


def plant_exact_inverse(B, N, M, k):
    """the same indices, val = (1, 0, ...): P12 P21 = I exactly (N <= M)"""
    row = T.exact_row(k)
    idx12, idx21 = _inverse_idx(B, N, M, k)
    return row.expand(B, N, k).contiguous(), idx12, row.expand(B, M, k).contiguous(), idx21


def dense_reference(val12, idx12, val21, idx21, grad=True):
    """float64 evaluation of the definition on the CPU -> dict(F (B,), C_fro (B,), and with grad g12, g21, A12, A21)."""
    v12 = val12.detach().cpu().double().requires_grad_(grad)
    v21 = val21.detach().cpu().double().requires_grad_(grad)
    i12, i21 = idx12.detach().cpu().long(), idx21.detach().cpu().long()
    B, N, _ = v12.shape
    M = v21.shape[1]
    P12 = torch.zeros(B, N, M, dtype=torch.float64).scatter_add(-1, i12, v12)
    P21 = torch.zeros(B, M, N, dtype=torch.float64).scatter_add(-1, i21, v21)
    C = P12 @ P21
    eye = torch.eye(N, dtype=torch.float64)
    F = (C - eye).flatten(1).norm(dim=1)
    out = {"C_fro": C.detach().flatten(1).norm(dim=1), "F": F.detach()}
    if not grad:
        return out
    out["g12"], out["g21"] = torch.autograd.grad(F.sum(), (v12, v21))
    Fd = F.detach()[:, None, None]
    Cp = C.detach() + eye
    Q12 = (Cp @ P21.detach().transpose(1, 2)).gather(-1, i12)
    Q21 = (P12.detach().transpose(1, 2) @ Cp).gather(-1, i21)
    for name, Q in (("A12", Q12), ("A21", Q21)):
        out[name] = torch.where(Fd > 0, Q / Fd.clamp_min(1e-300), torch.zeros_like(Q))
    return out


def loss_bound(ref, k):
    return T.loss_bound(ref, k + 2, ref["C_fro"])


def grad_bound(ref, k, side):
    """side = "12" or "21"; k = k12 for both"""
    return T.grad_bound(ref, k + 2, ref["C_fro"], ref["g" + side], ref["A" + side])
