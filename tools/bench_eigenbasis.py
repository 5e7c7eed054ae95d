"""The Laplace-Beltrami eigenbasis at dataset size, for profiles/notes_eigenbasis.md: ops.mesh_eigenbasis on a jittered 64 x 64 grid
mesh (N = 4096, 7938 triangles, open boundary) for k = 30, 64 and 100 with the default guard, degree and tolerance.  Every call is
bracketed by device events after a warm-up call; medians with the spread (min .. max), the outer iterations, the operator
applications and the largest residual of each k.  The two tall-skinny products of the solver are timed alone at N = 4096, m = 80
(ops.basis_project is the weighted X^T Y).  If SciPy is importable, the wall time of scipy.sparse.linalg.eigsh(L, k, M,
sigma=-1e-8) on the same operator is reported beside it — for orientation only, no threshold rests on these times.
One JSON line.

Usage: python tools/bench_eigenbasis.py [rounds=5] [out.json]"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dv-matcher_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from dvm import ops  # noqa: E402

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
assert torch.cuda.is_available(), "a measurement needs the MI355X"
G = 64


def jittered_grid(m, jitter=0.2, seed=1):
    h = 1.0 / (m - 1)
    ii, jj = np.meshgrid(np.arange(m), np.arange(m), indexing="ij")
    xy = np.stack([ii * h, jj * h], -1).astype(np.float64)
    xy[1:-1, 1:-1] += jitter * h * (np.random.default_rng(seed).random((m - 2, m - 2, 2)) - 0.5)
    verts = np.concatenate([xy.reshape(-1, 2), np.zeros((m * m, 1))], 1)
    faces = []
    for i in range(m - 1):
        for j in range(m - 1):
            p00, p01, p10, p11 = i * m + j, i * m + j + 1, (i + 1) * m + j, (i + 1) * m + j + 1
            faces += [(p00, p10, p11), (p00, p11, p01)] if (i + j) % 2 == 0 else [(p00, p10, p01), (p10, p11, p01)]
    return verts.astype(np.float32), np.asarray(faces, np.int32)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out   # ms


def spread(v):
    return dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), rounds=len(v))


verts, faces = jittered_grid(G)
N = len(verts)
v, f = torch.from_numpy(verts).cuda()[None], torch.from_numpy(faces).cuda()
op = ops.mesh_laplacian(v, f)
row = dict(N=N, F=len(faces), degree=20, tol=1e-10, cases=[])
for k in (30, 64, 100):
    ops.mesh_eigenbasis(v, f, k)
    ts = []
    for _ in range(rounds):
        t, eb = timed(lambda: ops.mesh_eigenbasis(v, f, k))
        ts.append(t)
    info = eb.info[0].tolist()
    case = dict(k=k, guard=max(8, k // 4), iterations=info[0], converged=info[1], applications=info[3], max_res=float(eb.res.max()),
                **spread(ts))
    try:
        from scipy.sparse import csr_matrix, diags
        from scipy.sparse.linalg import eigsh
        rp, used = op.rowptr[0].cpu().numpy(), int(op.rowptr[0, N])
        col, w = op.col[0, :used].cpu().numpy(), op.w[0, :used].cpu().numpy().astype(np.float64)
        W = csr_matrix((w, col, rp), shape=(N, N))
        L = diags(np.asarray(W.sum(1)).ravel()) - W
        Mm = diags(op.mass[0].cpu().numpy().astype(np.float64))
        t0 = time.perf_counter()
        lam = eigsh(L.tocsc(), k, Mm.tocsc(), sigma=-1e-8)[0]
        case["scipy_eigsh_wall_ms"] = (time.perf_counter() - t0) * 1e3
        case["max_abs_diff_to_scipy"] = float(np.abs(np.sort(lam) - eb.evals[0].cpu().numpy()).max())
    except ImportError:
        pass
    row["cases"].append(case)

# the tall-skinny product alone at N = 4096, m = 80: X^T diag(mass) Y through the public entry (plain FMA form)
m = 80
X = torch.randn(1, N, m, dtype=torch.float64, device="cuda")
Y = torch.randn(1, N, m, device="cuda")
ops.basis_project(X, op.mass, Y)
row["tn_product_m80"] = spread([timed(lambda: ops.basis_project(X, op.mass, Y))[0] for _ in range(4 * rounds)])
print(json.dumps(row), flush=True)
if len(sys.argv) > 2:
    with open(sys.argv[2], "w") as fh:
        json.dump(row, fh, indent=1)
