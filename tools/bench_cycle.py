"""The cycle term alone, forward plus backward (models.loss.cycle_term(...).sum().backward()): the HIP kernel's route against the
dense torch route a user would otherwise write (SparsePi.to_dense() of both correspondences, one bmm, torch.norm: two dense
B x N x M arrays and one B x N x N array, plus what autograd keeps), on the pval / pidx that ops.softcorr gives on randn features in
both directions.  Both are timed in one process, alternating, with warm-up and device events around windows of at least MIN_S
seconds of work each; the peak memory of one step of each is read from torch's allocator.  Prints one JSON line per (shape, alpha)
(and keeps them in --out; profiles/notes_cycle.md).

    python tools/bench_cycle.py [--shapes 8x2048x2048,2x4995x2200] [--alphas 10,100] [--rounds 5] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dv-matcher_amd"))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import models.loss as ml  # noqa: E402
from dvm import ops  # noqa: E402

MIN_S = 0.3


def window(fn, reps):
    """Seconds per call over `reps` back-to-back calls, by device events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / reps


def peak_of(fn):
    """Bytes by which one call raises the allocator's peak."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


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
            col_counts = torch.zeros(B, M, dtype=torch.int64, device=dev).scatter_add_(1, idx12.long().flatten(1), torch.ones(B, N * 10, dtype=torch.int64, device=dev))
            v12, v21 = val12.clone().requires_grad_(True), val21.clone().requires_grad_(True)

            def step(term):
                v12.grad = v21.grad = None
                term(v12, idx12, v21, idx21).sum().backward()

            fns = {"kernel": lambda: step(ml.cycle_term), "dense": lambda: step(dense_term)}
            res = {}
            for k, term in (("kernel", ml.cycle_term), ("dense", dense_term)):
                step(term)
                res[k] = (v12.grad.clone(), v21.grad.clone(), term(v12.detach(), idx12, v21.detach(), idx21))
            reps, peak = {}, {}
            for k, fn in fns.items():   # warm-up, and the repetition count that fills MIN_S
                fn()
                torch.cuda.synchronize()
                reps[k] = max(3, int(MIN_S / window(fn, 3)) + 1)
                peak[k] = peak_of(fn)
            rounds = {k: [] for k in fns}
            for _ in range(args.rounds):   # alternate the candidates; report every round
                for k, fn in fns.items():
                    rounds[k].append(window(fn, reps[k]))
            med = {k: statistics.median(x) for k, x in rounds.items()}
            line = dict(B=B, N=N, M=M, k=10, alpha=alpha, t_kernel_ms=med["kernel"] * 1e3, t_dense_ms=med["dense"] * 1e3,
                        speedup=med["dense"] / med["kernel"],
                        spread_ms={k: (max(x) - min(x)) * 1e3 for k, x in rounds.items()},
                        rounds_ms={k: [round(t * 1e3, 4) for t in x] for k, x in rounds.items()}, reps=reps,
                        peak_bytes=peak, largest_column=int(col_counts.max()),
                        loss_kernel=res["kernel"][2].tolist(), loss_dense=res["dense"][2].tolist(),
                        g12_max_abs_diff=float((res["kernel"][0] - res["dense"][0]).abs().max()), g12_max_abs=float(res["dense"][0].abs().max()),
                        g21_max_abs_diff=float((res["kernel"][1] - res["dense"][1]).abs().max()), g21_max_abs=float(res["dense"][1].abs().max()))
            print(json.dumps(line))
            lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
