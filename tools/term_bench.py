"""What the loss terms' stand-alone benchmarks share (bench_rank.py, bench_cycle.py, bench_distortion.py; bench_sinkhorn.py takes
`window`): candidates timed in one process, alternating, with warm-up and device events around windows of at least MIN_S seconds
of work each; the peak memory of one call of each from torch's allocator; one JSON line per case, printed and kept in --out."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dv-matcher_amd"))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

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


def compare(fns, rounds):
    """fns: name -> callable, the first one "kernel".  -> the JSON fields every tool reports: t_<name>_ms (medians), speedup (of
    the kernel over the other candidate), spread_ms, rounds_ms, reps, peak_bytes.  The candidates alternate; every round is kept."""
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
    other, = [k for k in fns if k != "kernel"]
    out = {"t_%s_ms" % k: m * 1e3 for k, m in med.items()}
    out.update(speedup=med[other] / med["kernel"], spread_ms={k: (max(x) - min(x)) * 1e3 for k, x in times.items()},
               rounds_ms={k: [round(t * 1e3, 4) for t in x] for k, x in times.items()}, reps=reps, peak_bytes=peak)
    return out


def column_counts(idx, M):
    """(B,M) int64: how many entries of idx (B,N,k) pick each column"""
    B = idx.shape[0]
    flat = idx.long().flatten(1)
    return torch.zeros(B, M, dtype=torch.int64, device=idx.device).scatter_add_(1, flat, torch.ones_like(flat))


def emit(line, lines):
    print(json.dumps(line))
    lines.append(line)


def write_lines(path, lines):
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")
