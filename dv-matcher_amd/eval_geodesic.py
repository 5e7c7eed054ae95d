#!/usr/bin/env python3
"""Geodesic-error evaluation of hard correspondence maps — restatement of the reference's
eval/geo_mat.py:15-41 (geodesic matrix = Dijkstra over the mesh edges) and eval/main.m:16-45 (per pair: nearest
neighbour of the source features among the target's, error = geodesic distance on the target between the matched
vertex and the ground-truth vertex, averaged).

The nearest-neighbour search is the hot-path operator `knnsearch_t` (exact-difference arg-min, HIP kernel); the
geodesic matrices are preprocessing on the host, like the reference's own script.  Ground-truth files (`.vts`,
`M_*.mat`) are not shipped with the reference: this module takes arrays.

  err = mean_geodesic_error(phi_src, phi_tgt, vts_src, vts_tgt, M_tgt)
  err = mean_geodesic_error(.., zoomout=dict(basis_src=.., basis_tgt=.., k_init=20, k_final=100))   # ZoomOut-refined map
"""
import numpy as np


def mesh_area(verts, faces):
    """eval/surfaceArea.m: sum of triangle areas."""
    v = np.cross(verts[faces[:, 0]] - verts[faces[:, 1]], verts[faces[:, 0]] - verts[faces[:, 2]])
    return float(np.sqrt((v ** 2).sum(1)).sum() / 2)


def geodesic_distmat(verts, faces, normalize=True, method="edges"):
    """eval/geo_mat.py:15-41: shortest paths over the mesh edges weighted by their Euclidean lengths; with
    `normalize` divided by sqrt(surface area) (the M matrices the MATLAB evaluation loads).
    method="mesh" instead takes the symmetrised triangle-front distances (models.dataset.cal_geo's "mesh": dvm.ops.mesh_geodesics,
    needs a HIP device), which cut across triangles; the default stays the reference's Dijkstra."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import shortest_path
    if method not in ("edges", "mesh"):
        raise ValueError("geodesic_distmat: method must be 'edges' or 'mesh', got %r" % (method,))
    verts = np.asarray(verts, np.float64)
    faces = np.asarray(faces, np.int64)
    if method == "mesh":
        from models.dataset import _mesh_geodesics_gpu
        geo = _mesh_geodesics_gpu(verts.reshape(-1, 3), faces)
        if np.isinf(geo).any():
            raise ValueError("mesh graph is not connected")
        return geo / np.sqrt(mesh_area(verts, faces)) if normalize else geo
    e = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]], 0)
    e = np.unique(np.sort(e, 1), axis=0)
    w = np.linalg.norm(verts[e[:, 0]] - verts[e[:, 1]], axis=1)
    n = verts.shape[0]
    adj = coo_matrix((np.concatenate([w, w]), (np.concatenate([e[:, 0], e[:, 1]]), np.concatenate([e[:, 1], e[:, 0]]))), shape=(n, n))
    import torch
    if torch.cuda.is_available() and n * 8 <= 150 * 1024:   # same values as scipy's Dijkstra, one workgroup per source
        from models.dataset import _shortest_paths_gpu
        geo = _shortest_paths_gpu(adj.tocsr(), n)
    else:
        geo = shortest_path(adj.tocsr(), directed=False)
    if np.isinf(geo).any():
        raise ValueError("mesh graph is not connected")
    return geo / np.sqrt(mesh_area(verts, faces)) if normalize else geo


def match(phi_src, phi_tgt):
    """T[i] = argmin_j |phi_src[i] - phi_tgt[j]| (0-based), on the device (models/loss.py:91-95 semantics)."""
    import torch
    from dvm import ops
    a = torch.as_tensor(np.ascontiguousarray(phi_src), dtype=torch.float32).cuda()[None]
    b = torch.as_tensor(np.ascontiguousarray(phi_tgt), dtype=torch.float32).cuda()[None]
    return ops.argmin_exact(a, b)[0].cpu().numpy().astype(np.int64)


def geodesic_errors(T, vts_src, vts_tgt, M_tgt):
    """eval/main.m:34-41 with a precomputed map T (source vertex -> target vertex, 0-based): for every ground-truth
    landmark l, error_l = M_tgt[T[vts_src[l]], vts_tgt[l]]."""
    T = np.asarray(T).reshape(-1)
    return np.asarray(M_tgt)[T[np.asarray(vts_src)], np.asarray(vts_tgt)]


def match_precise(phi_src, phi_tgt, faces_tgt):
    """The precise map of the source features onto the target mesh in feature space (ops.precise_map) ->
    (face (N,) int64, bary (N,3) float64): source point i lands in the target triangle faces_tgt[face[i]] with those weights."""
    import torch
    from dvm import ops
    a = torch.as_tensor(np.ascontiguousarray(phi_src), dtype=torch.float32).cuda()[None]
    b = torch.as_tensor(np.ascontiguousarray(phi_tgt), dtype=torch.float32).cuda()[None]
    f = torch.as_tensor(np.ascontiguousarray(np.asarray(faces_tgt).reshape(-1, 3)), dtype=torch.int32).cuda()
    face, bary, _, _ = ops.precise_map(a, b, f, want_dist=False)
    return face[0].cpu().numpy().astype(np.int64), bary[0].cpu().numpy().astype(np.float64)


def geodesic_errors_precise(face, bary, faces_tgt, vts_src, vts_tgt, M_tgt):
    """geodesic_errors for a precise map: the landmark's image is a point of a target triangle, and its distance to the true
    partner is interpolated from the triangle's corners,
    error_l = sum_k bary[vts_src[l], k] * M_tgt[faces_tgt[face[vts_src[l]], k], vts_tgt[l]].
    A map with one-hot weights gives geodesic_errors of the vertex it names."""
    face, bary = np.asarray(face).reshape(-1), np.asarray(bary, dtype=np.float64).reshape(-1, 3)
    vts_src, vts_tgt = np.asarray(vts_src), np.asarray(vts_tgt)
    corners = np.asarray(faces_tgt).reshape(-1, 3)[face[vts_src]]                      # (L,3)
    return (bary[vts_src] * np.asarray(M_tgt)[corners, vts_tgt[:, None]]).sum(axis=1)


def match_zoomout(phi_src, phi_tgt, basis_src, basis_tgt, k_init, k_final, k_step=1, n_inter=1, solve="adjoint"):
    """match() refined by ZoomOut (the reference's Tools/utils.py::zo_fmap as a post-process): the features' nearest-neighbour map
    is the start map, models.loss.zoomout grows the functional map from k_init to k_final over the two shapes' Laplace-Beltrami
    bases (dvm.ops.Eigenbasis of one shape each, e.g. ops.mesh_eigenbasis), and the returned map is the point map of the final C
    (models.loss.pointwise_map) -> T (N,) int64, 0-based."""
    import torch
    from models.loss import pointwise_map, zoomout
    T0 = torch.as_tensor(match(phi_src, phi_tgt).astype(np.int32)).cuda()[None]
    zo = zoomout(T0, basis_src, basis_tgt, k_init, k_final, k_step=k_step, n_inter=n_inter, solve=solve)
    return pointwise_map(zo.C, basis_src, basis_tgt)[0].cpu().numpy().astype(np.int64)


def mean_geodesic_error(phi_src, phi_tgt, vts_src, vts_tgt, M_tgt, faces_tgt=None, zoomout=None):
    """The vertex map's mean error; with faces_tgt the precise map's (match_precise, geodesic_errors_precise); with zoomout — a dict
    of match_zoomout's arguments after the features (basis_src, basis_tgt, k_init, k_final, ..) — the refined vertex map's."""
    if zoomout is not None:
        if faces_tgt is not None:
            raise ValueError("mean_geodesic_error: zoomout refines the vertex map; it cannot be combined with faces_tgt")
        return float(geodesic_errors(match_zoomout(phi_src, phi_tgt, **zoomout), vts_src, vts_tgt, M_tgt).mean())
    if faces_tgt is not None:
        face, bary = match_precise(phi_src, phi_tgt, faces_tgt)
        return float(geodesic_errors_precise(face, bary, faces_tgt, vts_src, vts_tgt, M_tgt).mean())
    return float(geodesic_errors(match(phi_src, phi_tgt), vts_src, vts_tgt, M_tgt).mean())


def map_dirichlet_energy(verts_src, faces_src, verts_tgt, T=None, face=None, bary=None, faces_tgt=None):
    """The smoothness of a map beside its geodesic error: the Dirichlet energy of the target coordinates pulled back to the source
    mesh, under the source's cotangent operator, over the energy of the source's own coordinates (2 x its area) — 1 for a map
    that preserves local lengths, larger the more neighbouring source points are torn apart on the target.  Either a vertex map
    T (N,) (0-based: one entry of value 1 per row) or a precise map face (N,), bary (N,3) with the target's faces_tgt (three
    entries per row, the triangle's corners; a row without a face, face < 0, contributes nothing).  On the device
    (dvm.ops.mesh_laplacian, dvm.ops.dirichlet_term)."""
    import torch
    from dvm import ops
    vs = torch.as_tensor(np.ascontiguousarray(verts_src), dtype=torch.float32).cuda()[None]
    vt = torch.as_tensor(np.ascontiguousarray(verts_tgt), dtype=torch.float32).cuda()[None]
    fs = torch.as_tensor(np.ascontiguousarray(np.asarray(faces_src).reshape(-1, 3)), dtype=torch.int32).cuda()
    if (T is None) == (face is None):
        raise ValueError("map_dirichlet_energy: give either T or (face, bary, faces_tgt)")
    if T is not None:
        idx = torch.as_tensor(np.asarray(T).reshape(1, -1, 1).astype(np.int32)).cuda()
        val = torch.ones(idx.shape, dtype=torch.float32, device=idx.device)
    else:
        if bary is None or faces_tgt is None:
            raise ValueError("map_dirichlet_energy: a precise map needs face, bary and faces_tgt")
        face = np.asarray(face).reshape(-1)
        corners = np.asarray(faces_tgt).reshape(-1, 3)[np.maximum(face, 0)]
        idx = torch.as_tensor(np.where(face[:, None] >= 0, corners, -1).astype(np.int32)).cuda()[None]
        val = torch.as_tensor(np.ascontiguousarray(np.asarray(bary, dtype=np.float32).reshape(-1, 3))).cuda()[None]
    if idx.shape[1] != vs.shape[1]:
        raise ValueError("map_dirichlet_energy: the map has %d rows, the source mesh %d vertices" % (idx.shape[1], vs.shape[1]))
    op = ops.mesh_laplacian(vs, fs)
    E = ops.dirichlet_term(val, idx, vt, op)
    return float((E.double() / op.norm.double())[0])
