"""-m gpu: the whole-target scan of grid_chamfer_kernel (chamfer_scan_wave, csrc/dvm_grid.hip) at the smallest sizes that reach it.

The scan screens |p|^2 - 2 p.q per 32-point tile on the matrix cores, keeps the two smallest tile minima and a bound on all the
others, evaluates the best two tiles exactly and falls back to an exact scan of everything where the bound does not certify them.
Outputs must equal brute force bit for bit: float32, the difference form (dx^2 + dy^2) + dz^2, lowest original index on exact ties
(the yardstick of test_chamfer_grid_scan_path_equals_brute_force).  Every case runs through ops.chamfer, with and without indices.

Two batches per case and shape:
  * STATED: 3 clouds, targets of P in {33, 64, 96, 100} points, 64 and 100 queries.  ops.chamfer sends a batch this small to the
    brute-force kernels (dvm_chamfer_fwd_f32 takes the grid from B (N + M) > 65536 and N, M >= 64 on), so these pin the same
    inputs on the route a small call really takes - they do not reach the scan.
  * GRID: the same three clouds repeated until B (N + M) > 65536, P in {64, 65, 96, 100} (two full tiles, two tiles and a
    one-point tile, three tiles, three tiles and a ragged fourth; a 33-point target cannot take the grid route at all), 64 and
    100 queries (a full and a partly filled last wave).  These reach the scan.

Why every wave of the a -> b direction scans in the GRID batches: a wave goes to the scan when 24 or more of its lanes are not
certified in the radius-1 cube of cells around the query.  Every target below leaves the cube of the far queries empty (the
octant of the target's box that faces the queries holds no point), or is collapsed to a cluster 1e-5 wide seen from a distance
of more than 2 (the cube's certification asks for best < 0.9999 bound, and best and bound differ by ~1e-5 relative): no lane is
certified there.  DVM_DEBUG is read once when the library is loaded, so the statistics hook cannot be switched on inside this
process; test_scan_ran_in_every_case runs the GRID batches once more in one child process under DVM_DEBUG=4 and reads the counts.
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

STATED = [(P, Q) for P in (33, 64, 96, 100) for Q in (64, 100)]
GRID = [(P, Q) for P in (64, 65, 96, 100) for Q in (64, 100)]
CASES = ["collapsed_k1", "collapsed_k3", "collapsed_k40", "far_10", "far_1e3", "far_1e5", "tile_ties_exact", "tile_ties_ulp",
         "mag_1e-6", "mag_mixed", "nonfinite_query", "nonfinite_target"]
BAD = 1   # the batch entry that the non-finite cases poison


def hollow(P, rng):
    """P points spanning the unit box exactly, none in the octant x, y, z > 0.4 (the cells that face a query far along +x+y+z)."""
    x = rng.random((P, 3))
    x[(x > 0.4).all(1), 0] -= 0.4
    x[:4] = [[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]]
    return x


def symmetric(P, rng):
    """Points in fours (x, y, z), (x, 1 - y, z), (x, y, 1 - z), (x, 1 - y, 1 - z) on a 2^-10 lattice, x <= 0.375, y, z <= 0.25:
    a query with y = z = 0.5 is exactly as far from all four, which lie in different (z, y) quarters of the storage order -
    at P >= 96 in three or four different 32-point tiles.  Rows in random order: the lowest index of a tie may sit anywhere."""
    n = (P + 3) // 4
    p = np.concatenate([rng.integers(0, 385, (n, 1)), rng.integers(0, 257, (n, 2))], 1) / 1024.0
    p[0, 1:] = 0.0                                       # the box is [.., ..] x [0, 1] x [0, 1]
    four = np.concatenate([p, p * [1, -1, 1] + [0, 1, 0], p * [1, 1, -1] + [0, 0, 1], p * [1, -1, -1] + [0, 1, 1]])
    return four[rng.permutation(4 * n)[:P]] if 4 * n != P else four[rng.permutation(P)]


def make(case, P, Q, seed):
    """(a, b): three query clouds (3, Q, 3) and three targets (3, P, 3), float32."""
    rng = np.random.default_rng(seed)
    a, b = np.empty((3, Q, 3)), np.empty((3, P, 3))
    for e in range(3):
        if case.startswith("collapsed"):
            k = int(case[len("collapsed_k"):])
            loc = 0.5 + 1e-5 * rng.random((k, 3))
            b[e] = loc[np.arange(P) % k] + 1e-6 * rng.integers(0, 2, (P, 1)) * rng.random((P, 3))   # near-duplicates 1e-6 apart
            a[e] = rng.random((Q, 3)) + 2.0
        elif case.startswith("tile_ties"):
            b[e] = symmetric(P, rng)
            a[e] = np.concatenate([10.0 + rng.integers(0, 1024, (Q, 1)) / 1024.0, np.full((Q, 2), 0.5)], 1)
            if case == "tile_ties_ulp":                  # one ulp of 0.5 off the mirror planes, either way
                a[e, :, 1:] = np.nextafter(np.float32(0.5), np.float32(rng.integers(0, 2, (Q, 2))))
        else:
            off = {"far_1e3": 1e3, "far_1e5": 1e5}.get(case, 10.0)
            b[e] = hollow(P, rng)
            a[e] = rng.random((Q, 3)) + off
            if case == "mag_mixed":                      # half of the target a cluster of order 1e-4, the rest of order 1
                b[e, 4::2] *= 1e-4
    if case == "mag_1e-6":
        a, b = a * 1e-6, b * 1e-6
    a, b = a.astype(np.float32), b.astype(np.float32)
    if case == "nonfinite_query":
        a[BAD, 5, 0], a[BAD, 9, 1] = np.nan, np.inf
    if case == "nonfinite_target":
        b[BAD, 3, 1], b[BAD, 7, 2] = np.nan, -np.inf
    return a, b


def brute(q, t):
    """float32 (dx^2 + dy^2) + dz^2, minimum and its lowest index, per query of (E, Q, 3) against (E, P, 3)."""
    with np.errstate(invalid="ignore", over="ignore"):
        d = q[:, :, None, :] - t[:, None, :, :]
        D = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    assert D.dtype == np.float32
    return D.min(2), D.argmin(2).astype(np.int32)


def grid_batch(P, Q):
    return 3 * ((65536 // (P + Q)) // 3 + 1)


_made = {}


def inputs(case, P, Q):
    """The three clouds of a case and their brute-force results, made once and shared (read-only)."""
    key = (case, P, Q)
    if key not in _made:
        a, b = make(case, P, Q, 1000 * CASES.index(case) + 10 * P + Q)
        ref = brute(a, b) + brute(b, a)
        for x in (a, b) + ref:
            x.setflags(write=False)
        _made[key] = (a, b, ref)
    return _made[key]


def run_case(ops, torch, case, P, Q, B):
    a3, b3, (rd1, ri1, rd2, ri2) = inputs(case, P, Q)
    rep = lambda x: np.tile(x, (B // 3,) + (1,) * (x.ndim - 1))   # noqa: E731
    a, b = torch.from_numpy(rep(a3)).cuda(), torch.from_numpy(rep(b3)).cuda()
    d1, d2, i1, i2 = ops.chamfer(a, b, want_idx=True)
    n1, n2, j1, j2 = ops.chamfer(a, b, want_idx=False)
    assert j1 is None and j2 is None
    got = [x.cpu().numpy() for x in (d1, i1, d2, i2, n1, n2)]
    clean = np.ones(B, bool)
    if case.startswith("nonfinite"):
        # (the semantics of the existing non-finite Chamfer tests: the other entries are untouched, the poisoned entry gives the
        # same bit patterns in both forms and indices that are valid rows)
        clean[BAD::3] = False
        assert np.array_equal(got[4][~clean].view(np.int32), got[0][~clean].view(np.int32)), (case, P, Q, "a->b, both forms")
        assert np.array_equal(got[5][~clean].view(np.int32), got[2][~clean].view(np.int32)), (case, P, Q, "b->a, both forms")
        assert got[1].min() >= 0 and got[1].max() < P and got[3].min() >= 0 and got[3].max() < Q
        if case == "nonfinite_query":
            # the FINITE queries of the poisoned clouds against their clean target: brute force as everywhere (in the GRID batches
            # their waves hold an infinite |q|^2 and take the scan's fp32 form)
            rows = np.ones(Q, bool)
            rows[[5, 9]] = False
            assert np.array_equal(got[0][BAD::3][:, rows], rep(rd1)[BAD::3][:, rows]), (case, P, Q, "finite queries of the poisoned clouds")
            assert np.array_equal(got[1][BAD::3][:, rows], rep(ri1)[BAD::3][:, rows]), (case, P, Q, "finite queries of the poisoned clouds")
            assert np.array_equal(got[4][BAD::3][:, rows], rep(rd1)[BAD::3][:, rows]), (case, P, Q, "finite queries of the poisoned clouds")
    for name, x, ref in (("d a->b", got[0], rd1), ("i a->b", got[1], ri1), ("d b->a", got[2], rd2), ("i b->a", got[3], ri2),
                         ("d a->b, no indices", got[4], rd1), ("d b->a, no indices", got[5], rd2)):
        bad = (x != rep(ref))[clean]
        assert not bad.any(), (case, P, Q, B, name, int(bad.sum()), "entries differ from brute force, first at", np.argwhere(bad)[0].tolist())


@pytest.fixture(scope="module")
def ops():
    import torch
    from dvm import ops as _ops
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _ops


@pytest.mark.parametrize("case", CASES)
def test_stated_shapes_equal_brute_force(ops, case):
    import torch
    for P, Q in STATED:
        run_case(ops, torch, case, P, Q, 3)


@pytest.mark.parametrize("case", CASES)
def test_scan_equals_brute_force(ops, case):
    import torch
    for P, Q in GRID:
        run_case(ops, torch, case, P, Q, grid_batch(P, Q))


_STATS = re.compile(r"chamfer group (\d+): (\d+) queries.* (\d+) waves scanned for (\d+) lanes, (\d+) exact fallbacks")


def test_scan_ran_in_every_case():
    """One child process under DVM_DEBUG=4 runs every GRID batch once (the form with indices) and the kernel's own counts are
    read from its stderr: in the a -> b direction (group 0) every wave of every clean entry scans; with ties among four points
    in three or more tiles (P >= 96) some lanes take the exact fall-back."""
    env = dict(os.environ, DVM_DEBUG="4")
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    seen, cur = {}, None
    for line in r.stderr.splitlines():
        if line.startswith("CASE "):
            cur = tuple(line.split()[1:])
        m = _STATS.search(line)
        if m and cur and m.group(1) == "0":
            seen[cur] = tuple(int(m.group(k)) for k in (2, 3, 4, 5))
    for case in CASES:
        for P, Q in GRID:
            B = grid_batch(P, Q)
            queries, waves, lanes, fallbacks = seen[(case, str(P), str(Q))]
            dirty = B // 3 if case.startswith("nonfinite") else 0
            assert queries == B * Q
            assert waves >= (B - dirty) * ((Q + 63) // 64), (case, P, Q, "waves scanned", waves)
            assert lanes >= (B - dirty) * Q, (case, P, Q, "lanes served by a scan", lanes)
            if case.startswith("tile_ties") and P >= 96:
                assert fallbacks > 0, (case, P, Q, "no exact fall-back on ties across tiles")


if __name__ == "__main__":   # the child of test_scan_ran_in_every_case
    sys.path[:0] = [os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dv-matcher_amd")]
    import torch
    from dvm import ops as _ops
    for case in CASES:
        for P, Q in GRID:
            a3, b3, _ = inputs(case, P, Q)
            B = grid_batch(P, Q)
            sys.stderr.write("CASE %s %d %d\n" % (case, P, Q))
            sys.stderr.flush()
            _ops.chamfer(torch.from_numpy(np.tile(a3, (B // 3, 1, 1))).cuda(), torch.from_numpy(np.tile(b3, (B // 3, 1, 1))).cuda())
    torch.cuda.synchronize()
