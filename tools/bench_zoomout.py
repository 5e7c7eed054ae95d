"""ZoomOut spectral refinement at dataset size, for profiles/notes_zoomout.md: two differently jittered 64 x 64 grid meshes
(N = M = 4096, the grid of tools/bench_eigenbasis.py and a second draw), their bases from ops.mesh_eigenbasis at K = 100, a start
map with 40 % random entries.  Every call is bracketed by device events after a warm-up call; medians with the spread.
  - the nearest-neighbour step alone (ops.spectral_nn on Phi_X[:, :k] against the embedded target) at k = 30, 64, 128 columns
    (k = 128: random float64 rows, the bases stop at 100), with the rate 3 N M k / t, beside what a caller would write without
    it: torch.cdist in float64 followed by argmin on the same device, which materialises the N x M array; the rows on which the two
    disagree are counted (cdist is free to use the Gram form);
  - the other stages alone at k = 64: ops.fmap_from_pmap in both modes, ops.fmap_embed;
  - ops.zoomout for 30 -> 100 step 2, both modes, with the map's mean Euclidean error before and after;
  - with `host`: the wall time of the same loop on the host, once — tests/zoomout_ref.py's from_pmap (numpy lstsq) and embed with
    scipy.spatial.cKDTree for the query, as the reference does it — for orientation only, on a shared CPU.
One JSON line.

Usage: python tools/bench_zoomout.py [rounds=5] [out.json] [host]"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dv-matcher_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from dvm import ops  # noqa: E402

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
assert torch.cuda.is_available(), "a measurement needs the MI355X"
G, K = 64, 100


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


def spread(fn):
    fn()
    v = [timed(fn)[0] for _ in range(rounds)]
    return dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), rounds=len(v))


def map_error(T, verts_y):
    T = T.reshape(-1).cpu().numpy().astype(np.int64)
    return float(np.linalg.norm(verts_y[T] - verts_y, axis=1).mean())   # the true map is the identity


vx, faces = jittered_grid(G, seed=1)
vy, _ = jittered_grid(G, seed=7)
N = M = len(vx)
f = torch.from_numpy(faces).cuda()
ex = ops.mesh_eigenbasis(torch.from_numpy(vx).cuda()[None], f, K)
ey = ops.mesh_eigenbasis(torch.from_numpy(vy).cuda()[None], f, K)
assert int(ex.info[0, 1]) == 1 and int(ey.info[0, 1]) == 1, "the bases did not converge"
rng = np.random.default_rng(13)
T0 = np.arange(N, dtype=np.int32)
at = rng.random(N) < 0.4
T0[at] = rng.integers(0, M, int(at.sum()))
T0 = torch.from_numpy(T0).cuda()[None]
row = dict(N=N, M=M, K=K, start_error=map_error(T0, vy.astype(np.float64)), nn=[], stages_k64={}, zoomout=[])

for k in (30, 64, 128):
    if k <= K:
        A = ex.evecs
        E = ops.fmap_embed(ey.evecs, ops.fmap_from_pmap(ex.evecs, ex.mass, ey.evecs, T0, k=k))
    else:
        g = torch.Generator(device="cuda").manual_seed(k)
        A = torch.randn(1, N, k, dtype=torch.float64, device="cuda", generator=g)
        E = torch.randn(1, M, k, dtype=torch.float64, device="cuda", generator=g)
    Ak = A[:, :, :k].contiguous()
    case = dict(k=k, plan=ops.spectral_nn_plan(1, N, M, k), kernel=spread(lambda: ops.spectral_nn(A, E, k=k)),
                cdist_argmin=spread(lambda: torch.cdist(Ak, E).argmin(-1)))
    case["kernel_gop_per_s"] = 3.0 * N * M * k / (case["kernel"]["median_ms"] * 1e-3) / 1e9
    case["rows_differing_from_cdist"] = int((ops.spectral_nn(A, E, k=k).long() != torch.cdist(Ak, E).argmin(-1)).sum())
    row["nn"].append(case)

C64 = ops.fmap_from_pmap(ex.evecs, ex.mass, ey.evecs, T0, k=64)
row["stages_k64"] = dict(from_pmap_adjoint=spread(lambda: ops.fmap_from_pmap(ex.evecs, ex.mass, ey.evecs, T0, k=64)),
                         from_pmap_lstsq=spread(lambda: ops.fmap_from_pmap(ex.evecs, None, ey.evecs, T0, k=64, solve="lstsq")),
                         embed=spread(lambda: ops.fmap_embed(ey.evecs, C64)),
                         to_pmap=spread(lambda: ops.fmap_to_pmap(ex.evecs, ey.evecs, C64)))

for solve in ("adjoint", "lstsq"):
    def run():
        return ops.zoomout(ex.evecs, ex.mass, ey.evecs, T0, 30, K, k_step=2, solve=solve, check=False)
    zo = run()
    T = ops.fmap_to_pmap(ex.evecs, ey.evecs, zo.C)
    row["zoomout"].append(dict(solve=solve, k_init=30, k_final=K, k_step=2, info=zo.info[0].tolist(), final_error=map_error(T, vy.astype(np.float64)),
                               **spread(run)))

if "host" in sys.argv[3:]:
    from scipy.spatial import cKDTree

    import zoomout_ref as Z
    px, py = ex.evecs[0].cpu().numpy(), ey.evecs[0].cpu().numpy()
    T = T0[0].cpu().numpy()
    t0 = time.perf_counter()
    for k in range(30, K, 2):
        C = Z.from_pmap(px, None, py, T, k, "lstsq")[0]
        T = cKDTree(Z.embed(py, C)).query(px[:, :k])[1].astype(np.int32)
    C = Z.from_pmap(px, None, py, T, K, "lstsq")[0]
    row["host_loop_lstsq_wall_s"] = time.perf_counter() - t0
    row["host_loop_final_error"] = map_error(torch.from_numpy(cKDTree(Z.embed(py, C)).query(px[:, :K])[1]), vy.astype(np.float64))

print(json.dumps(row), flush=True)
if len(sys.argv) > 2:
    with open(sys.argv[2], "w") as fh:
        json.dump(row, fh, indent=1)
