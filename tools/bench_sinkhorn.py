"""ops.sinkhorn(n_iter) against its yardstick, ops.softcorr(variant=2): one sweep of the same fp32 matrix-core product with
a lighter epilogue.  Both are timed in one process, alternating, with warm-up and device events around windows of at
least MIN_S seconds of work each; the per-sweep share of the fp32-matrix bound (2 N M d B flop over 157.3 TF) is derived
from the shapes.  Prints one JSON line per alpha (and keeps it in --out).

--backward times ops.sinkhorn_bwd (on a history made once by ops.sinkhorn_hist) and ops.sinkhorn_hist instead, beside the two
yardsticks that do not depend on them, from the same run: t_fwd = ops.sinkhorn(n_iter) and t_scb = ops.softcorr_bwd(variant=2).
The expectation t_bwd <= 1.25 (t_fwd + (1 + x) t_scb) is stated with x = 0.049 * 2 n_iter (profiles/notes_sinkhorn.md 2b).

--tau R[,C] adds the unbalanced operator at those factors as one more candidate of the same run: ops.sinkhorn_unbalanced beside
ops.sinkhorn, or with --backward ops.sinkhorn_unbalanced_bwd / _hist beside ops.sinkhorn_bwd / _hist.  It adds no sweep, so the
expectation is a ratio of at most 1.05 (profiles/notes_sinkhorn.md 2c).

    python tools/bench_sinkhorn.py [--B 64] [--N 2048] [--M 2048] [--n-iter 5] [--alphas 100,10] [--rounds 3] [--backward] [--tau R[,C]]
                                   [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dv-matcher_amd"))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from dvm import ops  # noqa: E402
from term_bench import window  # noqa: E402

FP32_MATRIX_TFLOPS = 157.3
MIN_S = 0.5


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--N", type=int, default=2048)
    ap.add_argument("--M", type=int, default=2048)
    ap.add_argument("--n-iter", type=int, default=5)
    ap.add_argument("--alphas", default="100,10")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--backward", action="store_true")
    ap.add_argument("--tau", type=ops.tau_pair, default=None, metavar="R[,C]")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "bench_sinkhorn needs the MI355X: there is no CPU path to time"
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(0)
    f1 = torch.randn(args.B, args.N, 128, generator=g).to(dev)
    f2 = torch.randn(args.B, args.M, 128, generator=g).to(dev)
    sweeps = 2 * args.n_iter + 1
    bound = 2.0 * args.N * args.M * 128 * args.B / (FP32_MATRIX_TFLOPS * 1e12)   # seconds per sweep at the matrix peak
    lines = []
    for alpha in [float(x) for x in args.alphas.split(",")] if args.backward else []:
        gv = torch.randn(args.B, args.N, 10, generator=g).to(dev)
        val, idx, _, _, uh, vh = ops.sinkhorn_hist(f1, f2, alpha, args.n_iter)
        sval, sidx, smax, ssum = ops.softcorr(f1, f2, alpha, variant=2)
        fns = {"bwd": lambda: ops.sinkhorn_bwd(f1, f2, alpha, args.n_iter, val, idx, uh, vh, gv),
               "hist": lambda: ops.sinkhorn_hist(f1, f2, alpha, args.n_iter),
               "fwd": lambda: ops.sinkhorn(f1, f2, alpha, args.n_iter),
               "scb": lambda: ops.softcorr_bwd(f1, f2, alpha, sval, sidx, smax, ssum, gv, variant=2)}
        if args.tau:
            uval, uidx, _, _, ulm, rn, cn = ops.sinkhorn_unbalanced_hist(f1, f2, alpha, args.n_iter, tau=args.tau)
            glm = torch.randn(args.B, args.N, generator=g).to(dev)
            fns["ub_bwd"] = lambda: ops.sinkhorn_unbalanced_bwd(f1, f2, alpha, args.n_iter, args.tau, None, None, uval, uidx, ulm, rn, cn, gv, glm)
            fns["ub_hist"] = lambda: ops.sinkhorn_unbalanced_hist(f1, f2, alpha, args.n_iter, tau=args.tau)
        reps = {}
        for k, fn in fns.items():
            fn()
            torch.cuda.synchronize()
            reps[k] = max(3, int(MIN_S / window(fn, 3)) + 1)
        best = {k: [] for k in fns}
        for _ in range(args.rounds):
            for k, fn in fns.items():
                best[k].append(window(fn, reps[k]))
        t = {k: min(v) for k, v in best.items()}
        x = 0.049 * 2 * args.n_iter
        expected = 1.25 * (t["fwd"] + (1 + x) * t["scb"])
        line = dict(B=args.B, N=args.N, M=args.M, alpha=alpha, n_iter=args.n_iter, t_bwd_ms=t["bwd"] * 1e3, t_hist_ms=t["hist"] * 1e3,
                    t_fwd_ms=t["fwd"] * 1e3, t_scb_ms=t["scb"] * 1e3, x=x, expected_t_bwd_max_ms=expected * 1e3,
                    expectation_held=bool(t["bwd"] <= expected), rounds_ms={k: [round(v * 1e3, 3) for v in vs] for k, vs in best.items()},
                    reps=reps)
        if args.tau:
            line.update(tau=args.tau, t_ub_bwd_ms=t["ub_bwd"] * 1e3, t_ub_hist_ms=t["ub_hist"] * 1e3, ub_bwd_ratio=t["ub_bwd"] / t["bwd"],
                        ub_hist_ratio=t["ub_hist"] / t["hist"], ub_expected_ratio_max=1.05)
        print(json.dumps(line))
        lines.append(line)
    for alpha in [float(x) for x in args.alphas.split(",")] if not args.backward else []:
        fns = {"sinkhorn": lambda: ops.sinkhorn(f1, f2, alpha, args.n_iter), "sinkhorn0": lambda: ops.sinkhorn(f1, f2, alpha, 0),
               "softcorr_v2": lambda: ops.softcorr(f1, f2, alpha, variant=2)}
        if args.tau:
            fns["unbalanced"] = lambda: ops.sinkhorn_unbalanced(f1, f2, alpha, args.n_iter, tau=args.tau)
        reps = {}
        for k, fn in fns.items():   # warm-up, and the repetition count that fills MIN_S
            fn()
            torch.cuda.synchronize()
            reps[k] = max(3, int(MIN_S / window(fn, 3)) + 1)
        best = {k: [] for k in fns}
        for _ in range(args.rounds):   # alternate the candidates; report every round
            for k, fn in fns.items():
                best[k].append(window(fn, reps[k]))
        t = {k: min(v) for k, v in best.items()}
        per_sweep = (t["sinkhorn"] - t["sinkhorn0"]) / (2 * args.n_iter) if args.n_iter else t["sinkhorn0"]
        line = dict(B=args.B, N=args.N, M=args.M, alpha=alpha, n_iter=args.n_iter, sweeps=sweeps,
                    t_sinkhorn_ms=t["sinkhorn"] * 1e3, t_sinkhorn_n0_ms=t["sinkhorn0"] * 1e3, t_softcorr_v2_ms=t["softcorr_v2"] * 1e3,
                    rounds_ms={k: [round(x * 1e3, 3) for x in v] for k, v in best.items()}, reps=reps,
                    ratio=t["sinkhorn"] / t["softcorr_v2"], expected_ratio_max=1.25 * sweeps,
                    potential_sweep_ms=per_sweep * 1e3, matrix_bound_per_sweep_ms=bound * 1e3,
                    potential_sweep_share_of_fp32_matrix_bound=bound / per_sweep,
                    softcorr_v2_share_of_fp32_matrix_bound=bound / t["softcorr_v2"])
        if args.tau:
            line.update(tau=args.tau, t_unbalanced_ms=t["unbalanced"] * 1e3, unbalanced_ratio=t["unbalanced"] / t["sinkhorn"],
                        ub_expected_ratio_max=1.05)
        print(json.dumps(line))
        lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
