"""Seeded point-cloud families shared by the GPU tests of the geometry kernels (grid searches, FPS, graph build): the inputs
where such code breaks — all points in one cell, extents far from unit scale, a cloud far from the origin, exact ties, duplicated
rows, empty balls — and batches whose entries differ in kind.  Plain numpy; no test lives here."""
import numpy as np


# One seeded generator per family: (n, rng) -> float32 (n, 3).
def _unit(n, rng):
    return rng.random((n, 3))


def _coincident(n, rng):
    return np.tile(rng.random((1, 3)), (n, 1))


def _two_points(n, rng):
    return rng.random((2, 3))[rng.permutation(np.arange(n) % 2)]


def _line(n, rng):
    return rng.random((n, 1)) * np.array([[1.0, 2.0, 3.0]])


def _plane(n, rng):
    return np.concatenate([rng.random((n, 2)), np.zeros((n, 1))], 1)


def _huge_extent(n, rng):
    return rng.random((n, 3)) * 1e4


def _tiny_extent(n, rng):
    return rng.random((n, 3)) * 1e-5


def _translated(n, rng):
    return rng.random((n, 3)) + np.array([1e3, -7e2, 4e2])


def _translated_30(n, rng):
    return rng.random((n, 3)) + 30.0


def _one_outlier(n, rng):
    x = rng.random((n, 3))
    x[rng.integers(n)] = 1e3           # the box grows to 1e3: every other point lands in the first cell
    return x


def _lattice_shuffled(n, rng):
    # an integer lattice at a power-of-two spacing (coordinates, differences and the matmul form's |p|^2 are exact: ties are
    # exact ties), about the unit box, a random subset in random row order, shifted by half a step along a random set of axes
    # (a query of one such cloud against another sits exactly half way between lattice points: ties across cell faces)
    s = int(np.ceil(n ** (1.0 / 3.0))) + 1
    h = 2.0 ** -int(np.ceil(np.log2(s - 1)))
    g = np.stack(np.meshgrid(np.arange(s), np.arange(s), np.arange(s), indexing="ij"), -1).reshape(-1, 3)
    return (g[rng.permutation(len(g))[:n]] + 0.5 * rng.integers(0, 2, (1, 3))) * h


def _duplicates(n, rng):
    x = rng.random((n, 3))
    h = n // 2
    x[h:] = x[rng.integers(0, h, n - h)]
    return x


def _clustered_with_holes(n, rng):
    # empty balls of ~1.5 cells radius; the points that fell inside are stacked onto others (exact ties on the rims)
    x = rng.random((n, 3))
    c = rng.random((12, 3))
    for _ in range(3):
        inside = (np.linalg.norm(x[:, None] - c[None], axis=-1) < 0.12).any(-1)
        if not inside.any():
            break
        outside = np.flatnonzero(~inside)
        x[inside] = x[outside[rng.integers(0, len(outside), int(inside.sum()))]]
    return x


FAMILIES = {
    "coincident": _coincident, "two_points": _two_points, "line": _line, "plane": _plane, "huge_extent": _huge_extent,
    "tiny_extent": _tiny_extent, "translated": _translated, "translated_30": _translated_30, "one_outlier": _one_outlier,
    "lattice_shuffled": _lattice_shuffled, "duplicates": _duplicates, "clustered_with_holes": _clustered_with_holes,
}
FNAMES = list(FAMILIES)
F = len(FNAMES)
KINDS = FNAMES + ["mixed"]
# `unit` (plain random) is a family by name as well, outside FAMILIES: the mixed batch and KINDS stay the adversarial twelve
GENERATORS = dict(FAMILIES, unit=_unit)


def cloud(family, n, seed):
    return GENERATORS[family](n, np.random.default_rng(seed)).astype(np.float32)


def batch(kind, B, n, seed):
    """(B, n, 3) float32: B clouds of one family (different seeds), or for 'mixed' entry b from family b mod F."""
    return np.stack([cloud(FNAMES[b % F] if kind == "mixed" else kind, n, seed * 1000 + b) for b in range(B)])
