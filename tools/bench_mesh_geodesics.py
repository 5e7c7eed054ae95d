"""All-sources geodesic matrices of one mesh: the triangle-front solver (ops.mesh_geodesics: dvm_mesh_geodesics_f64, corner-table
prologue and flag read-back included) against the edge-path kernel (ops.graph_geodesics: dvm_graph_geodesics_f64) on the same
mesh's edge graph.  Both are timed in one process, alternating, with warm-up and device events around windows of at least MIN_S
seconds of work each.  Also reported: the solver's sweeps per source (min / median / max, read from the workspace, include/dvm.h),
the time of a call whose one source is a vertex in no face (the prologue, one sweep and the read-back: what a call costs before
its first real source), the mean difference of the two matrices, and what a symmetrised float32 matrix costs end to end through
models.dataset.cal_geo (host copies included).  Prints one JSON line per mesh (and keeps them in --out;
profiles/notes_mesh_geodesics.md).

    python tools/bench_mesh_geodesics.py [--meshes grid71,icosphere4] [--rounds 5] [--out FILE]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import term_bench as tb
import torch

sys.path.insert(0, os.path.join(tb.ROOT, "tests"))
import mesh_geodesic_ref as R  # noqa: E402  (the mesh generators live with the scheme's statement)
import models.dataset as ds  # noqa: E402
from dvm import _lib, ops  # noqa: E402


def make(name):
    if name.startswith("grid"):
        return R.grid_mesh(int(name[4:]), jitter=0.4, seed=0)
    if name.startswith("icosphere"):
        return R.icosphere(int(name[9:]))
    raise SystemExit("unknown mesh %r (gridM, icosphereS)" % name)


def edge_graph(verts, faces, dev):
    """the padded neighbour lists dvm_graph_geodesics_f64 takes, as models.dataset.cal_geo builds them"""
    F = np.asarray(faces, dtype=np.int64)
    src = np.concatenate([F[:, 0], F[:, 1], F[:, 2]])
    dst = np.concatenate([F[:, 1], F[:, 2], F[:, 0]])
    g = ds._dedup_min(src, dst, np.linalg.norm(verts[src] - verts[dst], axis=1), len(verts)).tocsr()
    deg = np.diff(g.indptr)
    K = int(deg.max())
    nbr = np.full((len(verts), K), -1, dtype=np.int32)
    wts = np.zeros((len(verts), K))
    row, col = np.repeat(np.arange(len(verts)), deg), np.arange(len(g.indices)) - np.repeat(g.indptr[:-1], deg)
    nbr[row, col], wts[row, col] = g.indices, g.data
    return torch.from_numpy(nbr).to(dev), torch.from_numpy(wts).to(dev)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--meshes", default="grid71,icosphere4")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "bench_mesh_geodesics needs the MI355X: there is no CPU path to time"
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    lines = []
    for name in args.meshes.split(","):
        verts, faces = make(name)
        V, F = len(verts), len(faces)
        v, f = torch.from_numpy(verts).to(dev), torch.from_numpy(np.ascontiguousarray(faces, dtype=np.int32)).to(dev)
        nbr, wts = edge_graph(verts, faces, dev)
        D = ops.mesh_geodesics(v, f)
        ws = ops.workspace(lib.dvm_mesh_geodesics_workspace_bytes(V, F), dev, "mesh_geo")
        sweeps = ws[256:256 + 4 * V].view(torch.int32).cpu().numpy()
        E = ops.graph_geodesics(nbr, wts)
        off = ~torch.eye(V, dtype=torch.bool, device=dev)
        # one more vertex, in no face: a call on it alone runs the prologue, one sweep and the read-back
        v1 = torch.cat([v, v[:1] + 10.0])
        lone = torch.tensor([V], dtype=torch.int32, device=dev)
        ops.mesh_geodesics(v1, f, lone)
        torch.cuda.synchronize()
        reps = 20
        prologue = [tb.window(lambda: ops.mesh_geodesics(v1, f, lone), reps) for _ in range(args.rounds)]
        t0 = time.perf_counter()
        ds.cal_geo(verts, faces, method="mesh")
        t_cal_mesh = time.perf_counter() - t0
        t0 = time.perf_counter()
        ds.cal_geo(verts, faces)
        t_cal_graph = time.perf_counter() - t0
        line = dict(mesh=name, V=V, F=F, graph_K=int(nbr.shape[1]),
                    **tb.compare({"kernel": lambda: ops.mesh_geodesics(v, f), "edges": lambda: ops.graph_geodesics(nbr, wts)}, args.rounds),
                    sweeps_min=int(sweeps.min()), sweeps_median=float(np.median(sweeps)), sweeps_max=int(sweeps.max()),
                    t_prologue_call_ms=statistics.median(prologue) * 1e3, prologue_rounds_ms=[round(t * 1e3, 4) for t in prologue],
                    cal_geo_mesh_s=t_cal_mesh, cal_geo_graph_s=t_cal_graph,
                    mean_mesh_over_edges=float((D[off] / E[off]).mean()), max_mesh_over_edges=float((D[off] / E[off]).max()),
                    asymmetry_max=float(((D - D.t()).abs()[off] / (D + D.t())[off]).max()))
        tb.emit(line, lines)
    tb.write_lines(args.out, lines)


if __name__ == "__main__":
    main()
