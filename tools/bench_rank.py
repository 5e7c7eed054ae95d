"""The rank term alone, forward plus backward (models.loss.rank_term(...).sum().backward()): the HIP kernel's route against the
torch formula it replaced (models.loss._rank_term_torch: a dense B x M x M float64 Gram matrix filled by scatter_add_ atomics),
on the pval / pidx that ops.softcorr gives on randn features.  Both are timed in one process, alternating, with warm-up and
device events around windows of at least MIN_S seconds of work each; the peak memory of one step of each is read from torch's
allocator.  Prints one JSON line per (shape, alpha) (and keeps them in --out; profiles/notes_rank.md).

    python tools/bench_rank.py [--shapes 8x2048,2x4995] [--alphas 10,100] [--rounds 5] [--out FILE]
"""
import argparse

import term_bench as tb
import torch

import models.loss as ml  # noqa: E402  (term_bench puts the package on sys.path)
from dvm import ops  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="8x2048,2x4995", help="BxN[,BxN...] (M = N)")
    ap.add_argument("--alphas", default="10,100")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "bench_rank needs the MI355X: there is no CPU path to time"
    dev = torch.device("cuda", 0)
    lines = []
    for shape in args.shapes.split(","):
        B, N = (int(x) for x in shape.split("x"))
        g = torch.Generator().manual_seed(0)
        f1 = torch.randn(B, N, 128, generator=g).to(dev)
        f2 = torch.randn(B, N, 128, generator=g).to(dev)
        for alpha in [float(x) for x in args.alphas.split(",")]:
            val, idx, _, _ = ops.softcorr(f1, f2, alpha)
            col_counts = tb.column_counts(idx, N)
            v = val.clone().requires_grad_(True)

            def step(term):
                v.grad = None
                term(v, idx, N).sum().backward()

            step(ml.rank_term)
            gk, lk = v.grad.clone(), ml.rank_term(v.detach(), idx, N)
            step(ml._rank_term_torch)
            gt, lt = v.grad.clone(), ml._rank_term_torch(v.detach(), idx, N)
            line = dict(B=B, N=N, M=N, k=10, alpha=alpha,
                        **tb.compare({"kernel": lambda: step(ml.rank_term), "torch": lambda: step(ml._rank_term_torch)}, args.rounds),
                        largest_column=int(col_counts.max()), sum_cj2=int((col_counts * col_counts).sum()),
                        loss_kernel=lk.tolist(), loss_torch=lt.tolist(),
                        grad_max_abs_diff=float((gk - gt).abs().max()), grad_max_abs=float(gt.abs().max()))
            tb.emit(line, lines)
    tb.write_lines(args.out, lines)


if __name__ == "__main__":
    main()
