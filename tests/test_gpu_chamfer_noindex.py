"""-m gpu: the index-free form of grid_chamfer_kernel (csrc/dvm_grid.hip) against the form with indices.

launch_grid_chamfer picks the index-free kernel when no group of the launch asks for indices (ops.chamfer(want_idx=False), and
every Chamfer launch of the pair forward).  That form keeps the running minimum alone: no sorted position, no tie flag, no tie
resolution, no read of the original indices, a walk whose list is the key.  Its distances must equal the with-index form's bit
for bit, and the with-index form (whose walk tracks the sorted position and reads indices on exact ties only) must still equal
brute force in distances AND indices.

Shapes (ops.chamfer reaches the grid only when B * (N + M) > 65536):
  (33, 1024, 1024)  G = 9, LDS-resident target, grids large enough for radius 2 - 3 walks
  (32, 1000, 1100)  unequal sizes, a ragged last wave and a ragged last 32-point tile
  (9, 4000, 4000)   grid route with the target in global memory (P > 2048)
"""
import numpy as np
import pytest
import torch

from test_gpu_grid_search import KINDS, batch, chamfer_ref, dev, ops  # noqa: F401  (ops: the module-scoped fixture)

pytestmark = pytest.mark.gpu

LDS_SHAPES = [(33, 1024, 1024), (32, 1000, 1100)]
SHAPES = LDS_SHAPES + [(9, 4000, 4000)]
sid = lambda s: "x".join(map(str, s))   # noqa: E731


def check_both_forms(ops, a, b, tag):
    """want_idx=False distances torch.equal to want_idx=True's; want_idx=True equal to brute force, distances and indices."""
    B, N, M = a.shape[0], a.shape[1], b.shape[1]
    assert B * (N + M) > 65536, "not on the grid route"
    d1, d2, i1, i2 = ops.chamfer(a, b, want_idx=True)
    n1, n2, j1, j2 = ops.chamfer(a, b, want_idx=False)
    assert j1 is None and j2 is None
    assert torch.equal(n1, d1) and torch.equal(n2, d2), (tag, "index-free distances differ",
                                                         int((n1 != d1).sum()), int((n2 != d2).sum()))
    for q, t, d, ix, side in ((a, b, d1, i1, "a->b"), (b, a, d2, i2, "b->a")):
        rd, ri = chamfer_ref(q, t)
        bad = (d != rd).any(1) | (ix != ri).any(1)
        assert not bool(bad.any()), (tag, side, "entries", torch.nonzero(bad).flatten().tolist())
    return d1, d2


@pytest.mark.parametrize("shape", LDS_SHAPES, ids=sid)
@pytest.mark.parametrize("kind", KINDS)
def test_all_families(ops, kind, shape):
    B, N, M = shape
    seed = 301 + KINDS.index(kind) + 17 * N
    check_both_forms(ops, dev(batch(kind, B, N, seed)), dev(batch(kind, B, M, seed + 5)), (kind, shape))


def regime(name, B, N, M, seed):
    """The bench's two Chamfer regimes on unit clouds.  one_hot: the target is the query cloud gathered through a random map
    with repeats (exact duplicates, exact zero distances: every wave sees ties).  far: b = 3 a + 2, most queries are not
    certified at radius 1 (walk and scan)."""
    rng = np.random.default_rng(seed)
    c = rng.random((B, max(N, M), 3)).astype(np.float32)
    a = c[:, :N]
    if name == "one_hot":
        return a, a[:, rng.integers(0, N, M)]
    return a, (3.0 * c[:, :M] + 2.0).astype(np.float32)


@pytest.mark.parametrize("shape", SHAPES, ids=sid)
@pytest.mark.parametrize("name", ["one_hot", "far"])
def test_bench_regimes(ops, name, shape):
    B, N, M = shape
    a, b = regime(name, B, N, M, 77 + N)
    d1, d2 = check_both_forms(ops, dev(a), dev(b), (name, shape))
    if name == "one_hot":
        assert float(d2.max()) == 0.0    # every target point IS a query point


@pytest.mark.parametrize("shape", SHAPES, ids=sid)
def test_non_finite_entry(ops, shape):
    """One entry with a NaN and an inf coordinate in a and in b.  Clean entries: index-free distances bit-equal to the same batch
    with the poisoned entry's clouds left clean (same B: still the grid).  Poisoned entry: the same bit patterns as the form
    with indices (int32 views: NaN and inf compare as bits)."""
    B, N, M = shape
    bad = B // 2
    a0, b0 = batch("mixed", B, N, 911 + N), batch("mixed", B, M, 912 + M)
    a, b = a0.copy(), b0.copy()
    a[bad, 5, 0] = np.nan
    a[bad, 9, 1] = np.inf
    b[bad, 100, 2] = -np.inf
    b[bad, 3, 1] = np.nan
    keep = [e for e in range(B) if e != bad]
    n1, n2, _, _ = ops.chamfer(dev(a), dev(b), want_idx=False)
    c1, c2, _, _ = ops.chamfer(dev(a0), dev(b0), want_idx=False)
    assert torch.equal(n1[keep], c1[keep]) and torch.equal(n2[keep], c2[keep])
    d1, d2, i1, i2 = ops.chamfer(dev(a), dev(b), want_idx=True)
    assert torch.equal(n1[keep], d1[keep]) and torch.equal(n2[keep], d2[keep])
    assert torch.equal(n1[bad].view(torch.int32), d1[bad].view(torch.int32))
    assert torch.equal(n2[bad].view(torch.int32), d2[bad].view(torch.int32))
    assert int(i1.min()) >= 0 and int(i1.max()) < M and int(i2.min()) >= 0 and int(i2.max()) < N
