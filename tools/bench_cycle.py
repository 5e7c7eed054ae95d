"""The cycle term alone, forward plus backward (models.loss.cycle_term(...).sum().backward()): the HIP kernel's route against the
dense torch route a user would otherwise write (SparsePi.to_dense() of both correspondences, one bmm, torch.norm: two dense
B x N x M arrays and one B x N x N array, plus what autograd keeps), on the pval / pidx that ops.softcorr gives on randn features in
both directions.  Both are timed in one process, alternating, with warm-up and device events around windows of at least MIN_S
seconds of work each; the peak memory of one step of each is read from torch's allocator.  Prints one JSON line per (shape, alpha)
(and keeps them in --out; profiles/notes_cycle.md).

    python tools/bench_cycle.py [--shapes 8x2048x2048,2x4995x2200] [--alphas 10,100] [--rounds 5] [--out FILE]
"""
import argparse

import term_bench as tb
import torch

import models.loss as ml  # noqa: E402  (term_bench puts the package on sys.path)
from dvm import ops  # noqa: E402


def dense_term(val12, idx12, val21, idx21):
    """||P12 P21 - I||_F through the dense arrays, in the inputs' fp32."""
    N, M = val12.shape[1], val21.shape[1]
    C = torch.bmm(ml.SparsePi(val12, idx12, M).to_dense(), ml.SparsePi(val21, idx21, N).to_dense())
    return (C - torch.eye(N, dtype=C.dtype, device=C.device)).flatten(1).norm(dim=1)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="8x2048x2048,2x4995x2200", help="BxNxM[,BxNxM...]")
    ap.add_argument("--alphas", default="10,100")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "bench_cycle needs the MI355X: there is no CPU path to time"
    dev = torch.device("cuda", 0)
    lines = []
    for shape in args.shapes.split(","):
        B, N, M = (int(x) for x in shape.split("x"))
        g = torch.Generator().manual_seed(0)
        f1 = torch.randn(B, N, 128, generator=g).to(dev)
        f2 = torch.randn(B, M, 128, generator=g).to(dev)
        for alpha in [float(x) for x in args.alphas.split(",")]:
            val12, idx12, _, _ = ops.softcorr(f1, f2, alpha)
            val21, idx21, _, _ = ops.softcorr(f2, f1, alpha)
            col_counts = tb.column_counts(idx12, M)
            v12, v21 = val12.clone().requires_grad_(True), val21.clone().requires_grad_(True)

            def step(term):
                v12.grad = v21.grad = None
                term(v12, idx12, v21, idx21).sum().backward()

            res = {}
            for k, term in (("kernel", ml.cycle_term), ("dense", dense_term)):
                step(term)
                res[k] = (v12.grad.clone(), v21.grad.clone(), term(v12.detach(), idx12, v21.detach(), idx21))
            line = dict(B=B, N=N, M=M, k=10, alpha=alpha,
                        **tb.compare({"kernel": lambda: step(ml.cycle_term), "dense": lambda: step(dense_term)}, args.rounds),
                        largest_column=int(col_counts.max()),
                        loss_kernel=res["kernel"][2].tolist(), loss_dense=res["dense"][2].tolist(),
                        g12_max_abs_diff=float((res["kernel"][0] - res["dense"][0]).abs().max()), g12_max_abs=float(res["dense"][0].abs().max()),
                        g21_max_abs_diff=float((res["kernel"][1] - res["dense"][1]).abs().max()), g21_max_abs=float(res["dense"][1].abs().max()))
            tb.emit(line, lines)
    tb.write_lines(args.out, lines)


if __name__ == "__main__":
    main()
