"""The Dirichlet term alone: ops.dirichlet_term(grad=True) — the HIP kernel, loss and gradient from one call — against the torch
composition (models.loss._dirichlet_term_torch, forward plus backward through autograd), on the same GPU and the same inputs: the
pval / pidx that ops.softcorr gives on randn features, the target's random coordinates, and the source's xyz kNN operator
(ops.knn_cdist, ops.knn_laplacian); with --hub one source point is also named by every list (a row of N - 1 + K entries).  The two
builders are timed beside them.  Timed in one process, alternating, with warm-up and device events around windows of at least
MIN_S seconds of work each (term_bench).  Prints one JSON line per shape (and keeps them in --out; profiles/notes_dirichlet.md).

    python tools/bench_dirichlet.py [--shapes 8x2048x2048] [--k 10] [--alpha 100] [--mode stretch] [--hub] [--rounds 5] [--out FILE]
"""
import argparse

import term_bench as tb
import torch

import models.loss as ml  # noqa: E402  (term_bench puts the package on sys.path)
from dvm import ops  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="8x2048x2048", help="BxNxM[,BxNxM...]")
    ap.add_argument("--k", type=int, default=10, help="neighbours per list (self included)")
    ap.add_argument("--alpha", type=float, default=100.0)
    ap.add_argument("--mode", default="stretch", choices=("stretch", "uniform"))
    ap.add_argument("--hub", action="store_true", help="every list also names point 0")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "bench_dirichlet needs the MI355X: there is no CPU path to time"
    dev = torch.device("cuda", 0)
    lines = []
    for shape in args.shapes.split(","):
        B, N, M = (int(x) for x in shape.split("x"))
        g = torch.Generator().manual_seed(0)
        f1, f2 = torch.randn(B, N, 128, generator=g).to(dev), torch.randn(B, M, 128, generator=g).to(dev)
        xyz, V = torch.rand(B, N, 3, generator=g).to(dev), torch.rand(B, M, 3, generator=g).to(dev)
        val, idx, _, _ = ops.softcorr(f1, f2, args.alpha)
        nbr = ops.knn_cdist(xyz, xyz, args.k)
        if args.hub:
            nbr = nbr.clone()
            nbr[:, 1:, -1] = 0
        op = ops.knn_laplacian(xyz, nbr, args.mode)
        v = val.clone().requires_grad_(True)

        def composed():
            v.grad = None
            loss = ml._dirichlet_term_torch(v, idx, V, op)
            loss.sum().backward()
            return loss.detach(), v.grad

        def kernel():
            return ops.dirichlet_term(val, idx, V, op, grad=True)

        lk, gk = kernel()
        lt, gt = composed()
        line = dict(B=B, N=N, M=M, k=int(idx.shape[-1]), C=3, K=args.k, mode=args.mode, hub=args.hub,
                    longest_row=int((op.rowptr[:, 1:] - op.rowptr[:, :-1]).max()), entries=op.stats[:, 3].tolist(),
                    **tb.compare({"kernel": kernel, "torch": composed}, args.rounds), loss_kernel=lk.tolist(), loss_torch=lt.tolist(),
                    g_max_abs_diff=float((gk - gt).abs().max()), g_max_abs=float(gt.abs().max()))
        tb.emit(line, lines)
        build = tb.compare({"kernel": lambda: ops.knn_laplacian(xyz, nbr, args.mode), "knn_cdist": lambda: ops.knn_cdist(xyz, xyz, args.k)},
                           args.rounds)
        tb.emit(dict(what="knn_laplacian beside the knn_cdist that feeds it", B=B, N=N, K=args.k, **build), lines)
    tb.write_lines(args.out, lines)


if __name__ == "__main__":
    main()
