"""The inputs of tests/test_gpu_graph_routes.py, shared with the CPU test that proves their tie coverage
(tests/test_graph_routes_cpu.py), and the numpy restatement of the FPS recurrence that classifies the ties.  No test lives here."""
import numpy as np

from cloud_families import F, FNAMES, batch, cloud

# launch_fps (csrc/dvm_graph.hip): T = 256 threads per cloud up to N = 4096 and 512 above; fps_kernel<PPT, T> with PPT the first of
# 2, 4, 6, 8, 10, 12, 16, 20, 24 that holds ceil(N / T).  N -> the route it pins:
FPS_ROUTES = {
    1: "<2,256>: one point, three waves of padding only",
    2: "<2,256>: two points in wave 0",
    63: "<2,256>: wave 0 short of one lane, waves 1-3 padding only",
    65: "<2,256>: one point in wave 1, waves 2-3 padding only",
    193: "<2,256>: one point in wave 3 (192 is the last size with a wave of padding only)",
    300: "<2,256>: second register column partly filled",
    1025: "<6,256>  (N 1025..1536)",
    2561: "<12,256> (N 2561..3072)",
    4096: "<16,256>: the last size at T = 256",
    4097: "<10,512>: the first size at T = 512",
    5121: "<12,512> (N 5121..6144)",
    6145: "<16,512> (N 6145..8192)",
    8193: "<20,512> (N 8193..10240)",
    10241: "<24,512> (N 10241..12288)",
    12288: "<24,512>: DVM_MAX_POINTS, every register column full, 144 KiB of LDS",
}
FPS_N = list(FPS_ROUTES)
FPS_KINDS = ["unit", "lattice_shuffled", "duplicates", "coincident", "translated", "one_outlier", "mixed"]
TIE_N = [n for n in FPS_N if n >= 1025]   # the sizes at which the lattice clouds must plant a tie at every level of the arg-max


def fps_threads(n):
    return 256 if n <= 4096 else 512


def fps_case(kind, n):
    """One FPS launch of the GPU test: x (3, n, 3) float32 and the starts 0, n // 2, n - 1."""
    x = batch(kind, 3, n, 4000 + 17 * FPS_KINDS.index(kind) + n)
    return x, np.array([0, n // 2, n - 1], np.int32)


def fps_numpy(x, start, threads):
    """The recurrence of lib/deformation_graph_point.py:18-33 in the kernels' rounding ((dx^2 + dy^2) + dz^2 in fp32, running
    minimum, the largest distance at its lowest index) for the full order, and the ties that decided it: for every step at which
    more than one index holds the maximum, the holders other than the winner are counted by where fps_kernel meets them under its
    map j -> (thread j mod T, register j div T): in the winner's thread (the descending select), in another thread of the
    winner's wave (the two DPP reductions), or in another wave (`better`).
    -> order (n,) int32, counts dict(thread=, wave=, block=)."""
    n = len(x)
    xs, ys, zs = (np.ascontiguousarray(x[:, c], dtype=np.float32) for c in range(3))
    dx, dy, dz = np.empty(n, np.float32), np.empty(n, np.float32), np.empty(n, np.float32)
    dist = np.full(n, 1e10, np.float32)
    tid = np.arange(n) % threads
    order = np.empty(n, np.int32)
    counts = dict(thread=0, wave=0, block=0)
    far = int(start)
    for it in range(n):
        order[it] = far
        np.subtract(xs, xs[far], out=dx), np.subtract(ys, ys[far], out=dy), np.subtract(zs, zs[far], out=dz)
        np.multiply(dx, dx, out=dx), np.multiply(dy, dy, out=dy), np.multiply(dz, dz, out=dz)
        np.add(dx, dy, out=dx), np.add(dx, dz, out=dx)   # (dx^2 + dy^2) + dz^2, every operation rounded to fp32
        np.minimum(dist, dx, out=dist)
        m = dist.max()
        hold = np.flatnonzero(dist == m)
        far = int(hold[0])
        if len(hold) > 1 and it + 1 < n:   # (the last step's arg-max is never used)
            t = tid[hold[1:]]
            same_thread = t == tid[far]
            same_wave = (t >> 6) == (tid[far] >> 6)
            counts["thread"] += int(same_thread.sum())
            counts["wave"] += int((same_wave & ~same_thread).sum())
            counts["block"] += int((~same_wave).sum())
    return order, counts


# dvm_dg_build_f32: launch_grid_ring / launch_grid_infl (csrc/dvm_grid.hip) stage the NODE grid (N / 2 nodes) in LDS while
# grid_lds_bytes = P * 18 + (G^3 + 1) * 2 <= 64 KB: with G = 14 that ends at P = 3335 nodes.  N -> the route it pins:
DG_ROUTES = {
    6670: "3335 nodes: grid_ring_kernel<512,true>, grid_infl_kernel<512,1>, the last LDS size; FPS <16,512>",
    6671: "3335 nodes again (odd N): still LDS",
    6672: "3336 nodes: grid_ring_kernel<128,false> and grid_infl_kernel<128,0>, the first global-memory size",
    8193: "4096 nodes, G = 15: global-memory forms; FPS <20,512>",
    12288: "6144 nodes, G = 16: global-memory forms at DVM_MAX_POINTS; FPS <24,512>",
}
DG_N = list(DG_ROUTES)
DG_KINDS = ["unit", "lattice_shuffled", "duplicates", "translated", "one_outlier", "mixed"]


def dg_case(kind, n):
    """One graph-build launch: x (B, n, 3), a different FPS start per entry.  B = 3; the mixed batch has B = 4 and walks the twelve
    families of cloud_families.FNAMES over the sizes, so that each family meets the global-memory forms (the last three sizes)."""
    si = DG_N.index(n)
    seed = 7000 + 13 * DG_KINDS.index(kind) + n
    if kind == "mixed":
        x = np.stack([cloud(FNAMES[(4 * si + b) % F], n, seed * 1000 + b) for b in range(4)])
    else:
        x = batch(kind, 3, n, seed)
    B = len(x)
    return x, np.array([(7919 * b + 13 * n + 5) % n for b in range(B)], np.int32)
