"""Geodesic graph build against the Euclidean one, and the skinning pass alone against its floor (one read of the node rows,
B * Nn * N * 4 bytes), at the sizes of profiles/notes_geod_graph.md.  Candidates alternate inside one process; every call is
bracketed by device events; medians with the spread (min .. max) over the rounds.

Usage: python tools/bench_dg_geod.py [rounds=30] [out.json]"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dv-matcher_amd"))
import torch  # noqa: E402

from dvm import ops  # noqa: E402

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 30
assert torch.cuda.is_available(), "a measurement needs the MI355X"
rows = []


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3   # us


def compare(tag, cands, floor_bytes=None):
    for fn in cands.values():      # warm-up: code objects, workspaces
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in cands}
    for _ in range(rounds):
        for k, fn in cands.items():
            ts[k].append(timed(fn))
    for k, v in ts.items():
        med = statistics.median(v)
        row = {"case": tag, "candidate": k, "median_us": round(med, 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2), "rounds": rounds}
        if floor_bytes:
            row["floor_bytes"] = floor_bytes
            row["GB_per_s_of_floor"] = round(floor_bytes / med * 1e-3, 1)
        rows.append(row)
        print(json.dumps(row), flush=True)


for B, N in ((16, 2048), (2, 4995)):
    g = torch.Generator().manual_seed(N)
    xyz = torch.rand(B, N, 3, generator=g).cuda()
    dist = torch.cdist(xyz, xyz).contiguous()
    start = torch.zeros(B, dtype=torch.int32).cuda()
    Nn = N // 2
    nodes = ops.fps(xyz, Nn, start)
    compare("build B=%d N=%d" % (B, N),
            {"dg_build": lambda: ops.dg_build(xyz, start),
             "dg_build_geod ring=euclidean": lambda: ops.dg_build_geod(xyz, dist, start, "euclidean"),
             "dg_build_geod ring=geodesic": lambda: ops.dg_build_geod(xyz, dist, start, "geodesic")})
    floor = B * Nn * N * 4
    for ring_k in (0, 9):
        auto = ops.dg_skin_geod_plan(B, N, Nn, ring_k)[1]
        cands = {"skin ring_k=%d auto (S=%d)" % (ring_k, auto): lambda rk=ring_k: ops.dg_skin_geod(dist, nodes, rk)}
        for S in (1, 2, 4, 8):
            cands["skin ring_k=%d S=%d" % (ring_k, S)] = lambda rk=ring_k, s=S: ops.dg_skin_geod(dist, nodes, rk, slices=s)
        compare("skin B=%d N=%d" % (B, N), cands, floor)
if len(sys.argv) > 2:
    with open(sys.argv[2], "w") as f:
        json.dump(rows, f, indent=1)
