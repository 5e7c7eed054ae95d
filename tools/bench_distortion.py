"""The distortion term alone: ops.distortion_term(grad=True) — the HIP kernel, loss and gradient from one call — against the dense
float64 route it replaces (models.loss._distortion_term_torch, forward plus backward: P scattered dense, two bmm, what autograd
keeps), on the same GPU and the same inputs: the pval / pidx that ops.softcorr gives on randn features, and exactly symmetric
Euclidean distance matrices of random points.  Both are timed in one process, alternating, with warm-up and device events around
windows of at least MIN_S seconds of work each; the peak memory of one call of each is read from torch's allocator.  Prints one
JSON line per shape (and keeps them in --out; profiles/notes_distortion.md).

    python tools/bench_distortion.py [--shapes 2x2048x2048,1x4995x2200] [--alpha 100] [--rounds 5] [--out FILE]
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


def compare(fns, rounds):
    """fns: name -> callable.  -> (median seconds, spread, the rounds, repetitions, peak bytes) per name; the candidates alternate."""
    reps, peak = {}, {}
    for k, fn in fns.items():   # warm-up, and the repetition count that fills MIN_S
        fn()
        torch.cuda.synchronize()
        reps[k] = max(3, int(MIN_S / window(fn, 3)) + 1)
        peak[k] = peak_of(fn)
    times = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            times[k].append(window(fn, reps[k]))
    med = {k: statistics.median(x) for k, x in times.items()}
    return med, {k: max(x) - min(x) for k, x in times.items()}, times, reps, peak


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
        counts = torch.zeros(B, M, dtype=torch.int64, device=dev).scatter_add_(1, idx.long().flatten(1), torch.ones(B, N * idx.shape[-1], dtype=torch.int64, device=dev))
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
        med, spread, times, reps, peak = compare({"kernel": kernel, "dense": dense}, args.rounds)
        line = dict(B=B, N=N, M=M, k=int(idx.shape[-1]), alpha=args.alpha, t_kernel_ms=med["kernel"] * 1e3, t_dense_ms=med["dense"] * 1e3,
                    speedup=med["dense"] / med["kernel"], spread_ms={k: x * 1e3 for k, x in spread.items()},
                    rounds_ms={k: [round(t * 1e3, 4) for t in x] for k, x in times.items()}, reps=reps, peak_bytes=peak,
                    largest_column=int(counts.max()), loss_kernel=lk.tolist(), loss_dense=ld.tolist(),
                    g_max_abs_diff=float((gk - gd).abs().max()), g_max_abs=float(gd.abs().max()))
        print(json.dumps(line))
        lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
