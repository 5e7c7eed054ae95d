"""The skinning rule of dvm_dg_skin_geod_f32 / dvm_dg_skin_weights_f32 (include/dvm.h), stated in numpy.

Vertex v and node position j meet at d(v, j) = dist[nodes_idx[j], v] (node rows, read along v).  Candidates are ordered by the
key (d, j): d compares as fp32 with NaN ranked as +inf and -0 == +0, the lower j first among equals.  The influences are the
first 3 entries of that order, the ring of node i the first K entries for the vertex nodes_idx[i].  The selected distances are
the matrix entries themselves.  Shared by the CPU test that pins this statement to the reference's fixtures and by the GPU tests.
"""
import numpy as np


def order(dist, nodes_idx):
    """dist (N,N), nodes_idx (Nn,) -> (Nn,N) int: column v lists the node positions in the key's order for vertex v."""
    d = np.asarray(dist, dtype=np.float32)[np.asarray(nodes_idx, dtype=np.int64)]      # (Nn, N): row j = node j, read along v
    d = np.where(np.isnan(d), np.float32(np.inf), d) + np.float32(0.0)                 # NaN -> +inf; -0 + 0 = +0
    j = np.broadcast_to(np.arange(d.shape[0])[:, None], d.shape)
    return np.lexsort((j, d), axis=0)                                                 # primary key d, then j


def skin(dist, nodes_idx, ring_k=0, k=3):
    """-> infl_idx (N,k) int64, dists (N,k) float32 (the matrix entries, unchanged), ring (Nn,ring_k) int64 or None."""
    nodes_idx = np.asarray(nodes_idx, dtype=np.int64)
    o = order(dist, nodes_idx)
    infl = o[:k].T.copy()
    raw = np.asarray(dist, dtype=np.float32)
    dists = raw[nodes_idx[infl], np.arange(raw.shape[0])[:, None]]
    ring = o[:ring_k, nodes_idx].T.copy() if ring_k > 0 else None
    return infl, dists, ring


def skin_batch(dist, nodes_idx, ring_k=0):
    """The same for dist (B,N,N), nodes_idx (B,Nn): stacked results."""
    parts = [skin(dist[b], nodes_idx[b], ring_k) for b in range(len(dist))]
    return (np.stack([p[0] for p in parts]), np.stack([p[1] for p in parts]),
            np.stack([p[2] for p in parts]) if ring_k > 0 else None)


def weights(dists, sigma):
    """exp(-d^2 / (2 sigma^2)) row-normalised in float64; an infinite or NaN d weighs 0, a row whose sum is 0 or not finite
    becomes (1, 0, 0)."""
    d = np.asarray(dists, dtype=np.float64)
    sg = np.asarray(sigma, dtype=np.float64).reshape((-1,) + (1,) * (d.ndim - 1)) if np.ndim(sigma) else np.float64(sigma)
    with np.errstate(all="ignore"):
        w = np.exp(-(d * d) / (2.0 * sg * sg))
        w = np.where(np.isfinite(d), w, 0.0)
        tot = w.sum(-1, keepdims=True)
        ok = np.isfinite(tot) & (tot > 0)
        out = np.where(ok, w / tot, 0.0)
    out[..., 0] = np.where(ok[..., 0], out[..., 0], 1.0)
    return out


# torch.cdist forms d^2 = |a|^2 + |b|^2 - 2 a.b in fp32 through the host's matrix product, whose summation order differs from
# host to host: a fixture's `dists` are the generator's roundings.  For coordinates in the unit cube every term is at most 6
# and each of the at most 4 roundings at most 6 * 2^-24, so two hosts' d^2 differ by at most twice that.
CDIST_D2_TOL = 2 * 4 * 6 * 2.0 ** -24


def same_up_to_cdist_rounding(dists, fixture_dists):
    """True if two hosts' roundings of the same matmul-form distances can differ this much (compared as squares in float64)."""
    a, b = np.asarray(dists, np.float64), np.asarray(fixture_dists, np.float64)
    return bool(np.abs(a * a - b * b).max() <= CDIST_D2_TOL)


def tie_free(dist, nodes_idx, first):
    """True if no vertex has two equal keys d among the first `first` entries of its order (and the next one)."""
    nodes_idx = np.asarray(nodes_idx, dtype=np.int64)
    o = order(dist, nodes_idx)[:first + 1]
    d = np.asarray(dist, dtype=np.float32)[nodes_idx[o], np.arange(np.asarray(dist).shape[0])[None, :]]
    return bool(np.all(d[1:] != d[:-1]))
