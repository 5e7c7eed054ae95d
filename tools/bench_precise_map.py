"""The precise map at evaluation size against the two things it can be compared with, for profiles/notes_precise_map.md:
ops.precise_map at N = M = 4995, d = 128 on a closed mesh of 9986 triangles (the convex hull of 4995 points of the sphere), for
the randn and the smooth feature families of tests/precise_map_ref.py; ops.argmin_exact(screen=False) at the same N, M (the same
N M d products, no faces); and a chunked torch formulation of the definition on the same GPU (rows in chunks, every face's six dot
products by einsum over the gathered differences, the four candidates by the quadratic's formula).  Candidates alternate inside
one process; every call is bracketed by device events; medians with the spread (min .. max); stats[1] / (N F) per family.

Usage: python tools/bench_precise_map.py [rounds=10] [out.json]"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dv-matcher_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from dvm import ops  # noqa: E402

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 10
assert torch.cuda.is_available(), "a measurement needs the MI355X"
N = M = 4995
D = 128


def sphere_mesh(n, seed):
    from scipy.spatial import ConvexHull
    g = np.random.default_rng(seed)
    v = g.standard_normal((n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return v, ConvexHull(v).simplices.astype(np.int32)


def families():
    g = np.random.default_rng(0)
    verts, faces = sphere_mesh(M, 1)
    f2 = g.standard_normal((M, D)).astype(np.float32)
    yield "randn", (f2[g.integers(0, M, N)] + 0.3 * g.standard_normal((N, D))).astype(np.float32), f2, faces
    A = g.standard_normal((3, D)) / np.sqrt(3.0)
    w = g.dirichlet(np.ones(3), N)
    pts = (w[:, :, None] * verts[faces[g.integers(0, len(faces), N)]]).sum(1)
    yield ("smooth", (pts @ A + 0.02 * g.standard_normal((N, D))).astype(np.float32),
           (verts @ A + 0.02 * g.standard_normal((M, D))).astype(np.float32), faces)


def torch_definition(f1, f2, faces, chunk=32):
    """(dist (N,), face (N,)) by the formula on gathered differences, rows in chunks."""
    a, b, c = (f2[faces[:, k].long()] for k in range(3))
    e1, e2, e3 = b - a, c - a, c - b
    e11, e12, e22, e33 = (e1 * e1).sum(1), (e1 * e2).sum(1), (e2 * e2).sum(1), (e3 * e3).sum(1)
    det = e11 * e22 - e12 * e12
    ok = det > 4.76837158e-7 * e11 * e22
    dist, face = [], []
    for i in range(0, f1.shape[0], chunk):
        w = a[None] - f1[i:i + chunk, None]                                  # (c, F, d)
        ww, d1, d2 = (w * w).sum(2), torch.einsum("fd,cfd->cf", e1, w), torch.einsum("fd,cfd->cf", e2, w)
        t1 = torch.where(e11 > 0, -d1 / e11, torch.zeros_like(d1)).clamp(0, 1)
        t2 = torch.where(e22 > 0, -d2 / e22, torch.zeros_like(d2)).clamp(0, 1)
        nb = (d2 - d1) + (e12 - e11)
        t3 = torch.where(e33 > 0, -nb / e33, torch.zeros_like(nb)).clamp(0, 1)
        q = torch.minimum(ww + t1 * (2 * d1 + t1 * e11), ww + t2 * (2 * d2 + t2 * e22))
        q = torch.minimum(q, (ww + 2 * d1 + e11) + t3 * (2 * nb + t3 * e33))
        s, t = (e12 * d2 - e22 * d1) / det, (e12 * d1 - e11 * d2) / det
        qi = ww + s * (2 * d1 + s * e11 + 2 * t * e12) + t * (2 * d2 + t * e22)
        q = torch.where(ok & (s >= 0) & (t >= 0) & (s + t <= 1), torch.minimum(q, qi), q)
        v, j = q.min(1)
        dist.append(v.clamp_min(0).sqrt()), face.append(j)
    return torch.cat(dist), torch.cat(face)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3   # us


rows = []
for name, f1, f2, faces in families():
    F = len(faces)
    a, b, f = torch.from_numpy(f1).cuda()[None], torch.from_numpy(f2).cuda()[None], torch.from_numpy(faces).cuda()
    cands = {"precise_map": lambda: ops.precise_map(a, b, f, check=False),
             "argmin_exact(screen=False)": lambda: ops.argmin_exact(a, b, want_dist=True, screen=False),
             "torch definition, 32-row chunks": lambda: torch_definition(a[0], b[0], f)}
    for fn in cands.values():
        fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in cands}
    for r in range(rounds):
        for k, fn in cands.items():
            if k.startswith("torch") and r >= 3:
                continue
            ts[k].append(timed(fn))
    face, bary, pi_idx, dist, stats = ops.precise_map(a, b, f, want_stats=True)
    _, dv = ops.argmin_exact(a, b, want_dist=True, screen=False)
    dt, _ = torch_definition(a[0], b[0], f)
    row = dict(family=name, N=N, M=M, d=D, F=F, exact_evaluations=int(stats[1]), exact_share=float(stats[1]) / (N * F),
               mean_dist=float(dist.mean()), mean_vertex_dist=float(dv.mean()), dist_over_vertex_dist=float((dist / dv).mean()),
               max_abs_diff_to_torch=float((dist[0] - dt).abs().max()))
    for k, v in ts.items():
        row[k] = dict(median_us=statistics.median(v), min_us=min(v), max_us=max(v), rounds=len(v))
    rows.append(row)
    print(json.dumps(row), flush=True)
if len(sys.argv) > 2:
    with open(sys.argv[2], "w") as fh:
        json.dump(rows, fh, indent=1)
