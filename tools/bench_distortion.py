"""The distortion term alone: ops.distortion_term(grad=True) — the HIP kernel, loss and gradient from one call — against the dense
float64 route it replaces (models.loss._distortion_term_torch, forward plus backward: P scattered dense, two bmm, what autograd
keeps), on the same GPU and the same inputs: the pval / pidx that ops.softcorr gives on randn features, and exactly symmetric
Euclidean distance matrices of random points.  Both are timed in one process, alternating, with warm-up and device events around
windows of at least MIN_S seconds of work each; the peak memory of one call of each is read from torch's allocator.  Prints one
JSON line per shape (and keeps them in --out; profiles/notes_distortion.md).

    python tools/bench_distortion.py [--shapes 2x2048x2048,1x4995x2200] [--alpha 100] [--rounds 5] [--out FILE]
"""
import argparse

import term_bench as tb
import torch

import models.loss as ml  # noqa: E402  (term_bench puts the package on sys.path)
from dvm import ops  # noqa: E402


def inputs(B, N, M, alpha, dev):
    """(val, idx, D1, D2) on `dev`: softcorr of seeded randn features, symmetric distance matrices of seeded random points."""
    g = torch.Generator().manual_seed(0)
    f1 = torch.randn(B, N, 128, generator=g).to(dev)
    f2 = torch.randn(B, M, 128, generator=g).to(dev)
    val, idx, _, _ = ops.softcorr(f1, f2, alpha)
    mats = []
    for n in (N, M):
        pts = torch.rand(B, n, 3, generator=g).to(dev)
        d = torch.cdist(pts, pts)
        d = 0.5 * (d + d.transpose(1, 2))
        d.diagonal(dim1=1, dim2=2).zero_()
        mats.append(d.contiguous())
    return val, idx, mats[0], mats[1]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="2x2048x2048,1x4995x2200", help="BxNxM[,BxNxM...]")
    ap.add_argument("--alpha", type=float, default=100.0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "bench_distortion needs the MI355X: there is no CPU path to time"
    dev = torch.device("cuda", 0)
    lines = []
    for shape in args.shapes.split(","):
        B, N, M = (int(x) for x in shape.split("x"))
        val, idx, D1, D2 = inputs(B, N, M, args.alpha, dev)
        counts = tb.column_counts(idx, M)
        v = val.clone().requires_grad_(True)

        def dense():
            v.grad = None
            loss = ml._distortion_term_torch(v, idx, D1, D2)
            loss.sum().backward()
            return loss.detach(), v.grad

        def kernel():
            return ops.distortion_term(val, idx, D1, D2, grad=True)

        lk, gk = kernel()
        ld, gd = dense()
        line = dict(B=B, N=N, M=M, k=int(idx.shape[-1]), alpha=args.alpha, **tb.compare({"kernel": kernel, "dense": dense}, args.rounds),
                    largest_column=int(counts.max()), loss_kernel=lk.tolist(), loss_dense=ld.tolist(),
                    g_max_abs_diff=float((gk - gd).abs().max()), g_max_abs=float(gd.abs().max()))
        tb.emit(line, lines)
    tb.write_lines(args.out, lines)


if __name__ == "__main__":
    main()
