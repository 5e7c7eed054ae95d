"""-m gpu: the Dirichlet term on its HIP kernels — the operator builders (dvm_mesh_laplacian_f32, dvm_knn_laplacian_f32), the term
(dvm_dirichlet_term_f32), its autograd node and the evaluation helper — against the float64 definitions of
tests/dirichlet_term_ref.py.  The bars are derived in profiles/notes_dirichlet.md: rowptr / col / stats exact; w, mass and norm
bit-equal on integer-coordinate plantings, else within 2^-23 |w| + 2^-40 |u||v| / |u x v| (meshes with every angle >= 20 degrees);
loss within 2^-23 |E| + 2^-40 S and every gradient element within the analogous bar, bit-equal on exact plantings."""
import os
import sys

import numpy as np
import pytest
import torch

import dirichlet_term_ref as D
import frob_term_common as T

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ops():
    return T.load_ops()


def host(t):
    return None if t is None else t.detach().cpu().numpy()


def bits0(x):
    """the bit patterns of an fp32 array, a zero of either sign as +0"""
    return (np.asarray(x, np.float32) + np.float32(0)).view(np.int32)


def op_fields(op):
    return [t for t in (op.rowptr, op.col, op.w, op.norm, op.mass, op.stats) if t is not None]


def same_bytes(a, b):
    return all(x.dtype == y.dtype and torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(op_fields(a), op_fields(b)))


def device_op(ops, refs):
    """reference dicts (one per batch element, one Ecap) -> ops.GraphOperator on the device"""
    stack = lambda k: torch.from_numpy(np.stack([r[k] for r in refs])).cuda()   # noqa: E731
    return ops.GraphOperator(stack("rowptr"), stack("col"), stack("w"), torch.tensor([float(r["norm"]) for r in refs]).cuda(), None, stack("stats"))


def check_structure(got, refs):
    """rowptr, col and stats equal the reference exactly, for every batch element"""
    for b, ref in enumerate(refs):
        assert np.array_equal(host(got.rowptr)[b], ref["rowptr"]), b
        assert np.array_equal(host(got.col)[b], ref["col"]), b
        assert np.array_equal(host(got.stats)[b], ref["stats"]), (b, host(got.stats)[b], ref["stats"])


# ---- the mesh builder
def planted_mesh():
    """Integer coordinates, N = F = 257 (one past the workgroup width): a closed fan of valence 100, a strip of right triangles
    (weight 0 at the right angles), an obtuse corner, a collinear face, a face with an index out of range, an edge shared by three
    faces, isolated vertices -> verts (3,N,3) (three batch elements with other heights), faces."""
    ring = [(x, -12) for x in range(-12, 13)] + [(13, y) for y in range(-12, 13)] + [(x, 13) for x in range(13, -12, -1)] + \
           [(-12, y) for y in range(13, -12, -1)]
    assert len(ring) == 100
    P = [(0, 0)] + ring                                                   # vertex 0: the fan's centre
    faces = [(0, 1 + t, 1 + (t + 1) % 100) for t in range(100)]
    base = len(P)
    gv, gf = D.grid_mesh(7, 12)
    P += [(40 + int(x), int(y)) for x, y, _ in gv]
    faces += [tuple(int(i) + base for i in f) for f in gf]
    o = len(P)
    P += [(60, 0), (64, 0), (59, 1)]                                      # the corner at (60, 0) is obtuse: u . v = -4
    faces.append((o, o + 1, o + 2))
    faces.append((base, base + 1, base + 2))                              # three collinear grid vertices: left out, counted
    a = len(P)
    P += [(70, 0), (70, 4), (73, 2), (67, 1), (75, 9)]                    # the edge (a, a + 1) in three faces
    faces += [(a, a + 1, a + 2), (a + 1, a, a + 3), (a, a + 1, a + 4)]
    N = 257
    faces.append((0, 1, N))                                               # an index out of range: left out, counted
    P += [(90 + i, 5) for i in range(N - len(P))]                         # isolated vertices
    faces += faces[100:100 + 257 - len(faces)]                            # repeated grid faces: the entries are a multiset
    faces = np.array(faces, np.int32)
    assert len(P) == N and len(faces) == 257
    rng = np.random.default_rng(7)
    verts = np.zeros((3, N, 3), np.float32)
    verts[:, :, :2] = np.array(P, np.float32)
    verts[1:, :, 2] = rng.integers(-3, 4, (2, N))                         # batch elements 1 and 2 leave the plane, on integers
    verts[:, base:base + 3, 2] = 0                                        # (the collinear face stays collinear)
    return verts, faces


def test_mesh_builder_on_integer_plantings_is_bit_equal(ops):
    verts, faces = planted_mesh()
    got = ops.mesh_laplacian(torch.from_numpy(verts).cuda(), torch.from_numpy(faces).cuda())
    again = ops.mesh_laplacian(torch.from_numpy(verts).cuda(), torch.from_numpy(faces).cuda())
    torch.cuda.synchronize()
    assert same_bytes(got, again), "two runs of the mesh builder differ"
    refs = [D.mesh_laplacian(verts[b], faces) for b in range(3)]
    check_structure(got, refs)
    for b, ref in enumerate(refs):
        assert ref["stats"][:3].tolist() == [1, 1, 0]
        w = ref["w"][:ref["rowptr"][-1]]
        assert b > 0 or ((w == 0).any() and (w < 0).any())                # in the plane: right angles and the obtuse corner
        assert np.diff(ref["rowptr"]).max() == 200 and (np.diff(ref["rowptr"]) == 0).sum() >= 60   # the fan's row, the isolated ones
        assert np.array_equal(host(got.w)[b].view(np.int32), ref["w"].view(np.int32)), b
        assert np.array_equal(host(got.mass)[b].view(np.int32), ref["mass"].view(np.int32)), b
        assert host(got.norm)[b] == ref["norm"], (b, host(got.norm)[b], ref["norm"])
    assert not np.array_equal(refs[0]["w"], refs[1]["w"])


def test_mesh_builder_on_a_curved_mesh(ops):
    """Non-integer coordinates, B = 3, N = 17 x 15 = 255 (one short of the workgroup width): structure exact, the weights within
    2^-23 |w| + 2^-40 |u||v| / |u x v| on a mesh whose angles are all >= 20 degrees; mass and norm within one fp32 rounding."""
    built = [D.grid_mesh(17, 15, noise=0.06, seed=s) for s in (1, 2, 3)]
    verts, faces = np.stack([v for v, _ in built]), built[0][1]
    got = ops.mesh_laplacian(torch.from_numpy(verts).cuda(), torch.from_numpy(faces).cuda())
    torch.cuda.synchronize()
    refs = [D.mesh_laplacian(verts[b], faces) for b in range(3)]
    check_structure(got, refs)
    for b, ref in enumerate(refs):
        assert ref["min_angle"] >= 20.0, ref["min_angle"]                 # the bound's precondition
        dw = np.abs(host(got.w)[b].astype(np.float64) - ref["w"].astype(np.float64))
        bar = D.builder_bounds(ref)
        print("mesh %d: worst |dw| / bar %.3g, min angle %.1f" % (b, float((dw / np.maximum(bar, 1e-300)).max()), ref["min_angle"]))
        assert (dw <= bar).all()
        m, mr = host(got.mass)[b].astype(np.float64), ref["mass"].astype(np.float64)
        assert (np.abs(m - mr) <= (2.0 ** -23 + 2.0 ** -40) * mr).all()
        assert abs(float(host(got.norm)[b]) - float(ref["norm"])) <= (2.0 ** -23 + 2.0 ** -40) * float(ref["norm"])
        E = D.energy(verts[b], dict(rowptr=host(got.rowptr)[b], col=host(got.col)[b], w=host(got.w)[b]))["E"]
        assert abs(E / float(host(got.norm)[b]) - 1.0) <= 1e-6


# ---- the list builder
def planted_lists(K, integer=True):
    """N = 300: every list names itself first; 299 of the 300 points name the hub 0; a -1 entry; points 5 and 6 coincide and 5
    names 6 (a zero distance)."""
    rng = np.random.default_rng(100 + K)
    N = 300
    if integer:
        xyz = np.stack(np.unravel_index(rng.permutation(20 ** 3)[:N], (20, 20, 20)), 1).astype(np.float32)
    else:
        xyz = rng.standard_normal((N, 3)).astype(np.float32)
    xyz[6] = xyz[5]
    nbr = rng.integers(0, N, (N, K)).astype(np.int32)
    nbr[:, 0] = np.arange(N)
    col = min(1, K - 1)
    nbr[1:, col] = 0                                                      # the hub (with K = 1 in place of the self entry)
    nbr[5, K - 1] = 6
    nbr[9, K - 1] = -1
    nbr[11, K - 1] = N
    return xyz, nbr


@pytest.mark.parametrize("mode", ["stretch", "uniform"])
@pytest.mark.parametrize("K", [1, 10, 16])
def test_list_builder_on_plantings(ops, K, mode):
    a, b = planted_lists(K), planted_lists(K, integer=False)
    xyz, nbr = np.stack([a[0], b[0]]), np.stack([a[1], b[1]])
    run = lambda: ops.knn_laplacian(torch.from_numpy(xyz).cuda(), torch.from_numpy(nbr).cuda(), mode)   # noqa: E731
    got, again = run(), run()
    torch.cuda.synchronize()
    assert same_bytes(got, again), "two runs of the list builder differ"
    assert got.mass is None and tuple(got.col.shape) == (2, 2 * 300 * K)
    refs = [D.knn_laplacian(xyz[e], nbr[e], mode) for e in range(2)]
    check_structure(got, refs)
    for e, ref in enumerate(refs):
        assert ref["stats"][D.STAT_RANGE] == 2 and ref["stats"][D.STAT_DEGEN] == (1 if mode == "stretch" else 0)
        assert np.diff(ref["rowptr"]).max() >= (299 if K > 1 else 296)    # the hub's row (K = 1: the three planted slots name no hub)
        # the reference evaluates the kernel's float64 expressions in its order: the same bits, integer coordinates or not
        assert np.array_equal(host(got.w)[e].view(np.int32), ref["w"].view(np.int32)), e
        assert host(got.norm)[e] == ref["norm"], (e, host(got.norm)[e], ref["norm"])
        E = D.energy(xyz[e], ref)["E"]
        assert abs(E / float(ref["norm"]) - 1.0) <= 1e-6


def test_list_builder_on_the_lists_of_knn_cdist(ops):
    """the criterion's own input: ops.knn_cdist's lists of a random cloud, N = 257"""
    xyz = torch.randn(2, 257, 3, generator=T.gen(4)).cuda()
    nbr = ops.knn_cdist(xyz, xyz, 10)
    got = ops.knn_laplacian(xyz, nbr)
    torch.cuda.synchronize()
    refs = [D.knn_laplacian(host(xyz)[b], host(nbr)[b]) for b in range(2)]
    check_structure(got, refs)
    for b, ref in enumerate(refs):
        assert ref["stats"].tolist() == [0, 0, 257, 2 * 257 * 9]
        assert np.array_equal(host(got.w)[b].view(np.int32), ref["w"].view(np.int32)) and host(got.norm)[b] == 257 * 9


# ---- the term
def crafted_operator(rng, B, N, lengths, Ecap, weight=lambda rng, n: rng.standard_normal(n).astype(np.float32)):
    """CSR arrays with the given row lengths (B lists; the rest of the rows random in 0..40), random columns and weights: the
    energy's and the residual's definitions need no symmetry -> reference dicts"""
    refs = []
    for b in range(B):
        ln = rng.integers(0, 41, N)
        ln[:len(lengths[b])] = lengths[b]
        rowptr = np.zeros(N + 1, np.int32)
        rowptr[1:] = np.cumsum(ln)
        used = int(rowptr[-1])
        assert used <= Ecap
        col, w = np.full(Ecap, -1, np.int32), np.zeros(Ecap, np.float32)
        col[:used] = rng.integers(0, N, used)
        w[:used] = weight(rng, used)
        refs.append(dict(rowptr=rowptr, col=col, w=w, norm=np.float32(1), stats=np.zeros(4, np.int32)))
    return refs


def reference_for(ops, val, idx, V, refs):
    """the reference fed the fp32 Y of ops.apply (slots out of range made (0, column 0) first: apply turns an index into an address)"""
    M = V.shape[1]
    ok = (idx >= 0) & (idx < M)
    Y = host(ops.apply(torch.from_numpy(np.where(ok, val, 0).astype(np.float32)).cuda(), torch.from_numpy(np.where(ok, idx, 0).astype(np.int32)).cuda(),
                       torch.from_numpy(V).cuda()))
    return [D.energy(Y[b], refs[b], grad_of=(idx[b], V[b])) for b in range(len(refs))]


def check_against_reference(label, out, want):
    loss, g = host(out[0]).astype(np.float64), host(out[1]).astype(np.float64)
    for b, ref in enumerate(want):
        lbar, gbar = D.loss_bound(ref), D.grad_bound(ref)
        err, gerr = abs(loss[b] - ref["E"]), np.abs(g[b] - ref["g"])
        print("%s b=%d E %.9g err %.3e bar %.3e; worst gradient ratio %.3g" % (label, b, ref["E"], err, lbar,
                                                                            float((gerr / np.maximum(gbar, 1e-300)).max())))
        assert err <= lbar
        assert (gerr <= gbar).all()


@pytest.mark.parametrize("C,k", [(1, 1), (3, 10), (16, 16), (5, 3)])
def test_term_against_reference(ops, C, k):
    """N != M (300 x 170), rows of 0, 1, 100 and 299 entries, B = 3 with different used lengths under one Ecap, a column and a slot
    index out of range; the loss-only call and a second run give the same bits."""
    rng = np.random.default_rng(10 * C + k)
    B, N, M, Ecap = 3, 300, 170, 300 * 40 + 1000
    refs = crafted_operator(rng, B, N, [[0, 1, 100, 299], [299, 0, 0, 1, 100], [1]], Ecap)
    assert len({int(r["rowptr"][-1]) for r in refs}) == 3
    refs[0]["col"][5] = N         # inside the row of 100: contributes nothing
    refs[1]["col"][7] = -1
    V = rng.standard_normal((B, M, C)).astype(np.float32)
    val = rng.random((B, N, k)).astype(np.float32)
    idx = np.stack([np.stack([rng.choice(M, k, replace=False) for _ in range(N)]) for _ in range(B)]).astype(np.int32)
    idx[0, 2, k - 1] = M          # inside the row of 100 entries
    idx[2, 17, 0] = -1
    case = (torch.from_numpy(val), torch.from_numpy(idx), torch.from_numpy(V), device_op(ops, refs))
    out = T.run_both(ops.dirichlet_term, case)
    assert T.same_bits(out, T.run_both(ops.dirichlet_term, case)), "two runs differ"
    want = reference_for(ops, val, idx, V, refs)
    check_against_reference("C=%d k=%d" % (C, k), out, want)
    assert float(out[1][0, 2, k - 1]) == 0 and float(out[1][2, 17, 0]) == 0
    # the entries and slots out of range contribute nothing: the same bits with the entry's weight zeroed / the slot's value zeroed
    refs[0]["w"][5] = 0
    refs[1]["w"][7] = 0
    val[0, 2, k - 1] = 0
    val[2, 17, 0] = 0
    clean = T.run_both(ops.dirichlet_term, (torch.from_numpy(val), torch.from_numpy(idx), torch.from_numpy(V), device_op(ops, refs)))
    assert T.same_bits(out, clean)


def grid_case(k):
    """the 9 x 9 integer grid's operator (weights 0 and 1/2), integer V (M = 100, C = 3), a permutation (k = 1) or a two-slot
    dyadic blend (k = 2)"""
    verts, faces = D.grid_mesh(9, 9)
    ref_op = D.mesh_laplacian(verts, faces)
    rng = np.random.default_rng(k)
    N, M = 81, 100
    V = rng.integers(-8, 9, (1, M, 3)).astype(np.float32)
    idx = np.stack([rng.permutation(M)[:N], rng.permutation(M)[:N]], 1)[None, :, :k].astype(np.int32)
    val = np.array([[1.0], [0.75, 0.25]][k - 1], np.float32)[None, None].repeat(N, 1)
    return verts, ref_op, val, idx, V


@pytest.mark.parametrize("k", [1, 2])
def test_exact_plantings_are_bit_equal(ops, k):
    _, ref_op, val, idx, V = grid_case(k)
    assert set(np.unique(ref_op["w"][:ref_op["rowptr"][-1]]).tolist()) == {0.0, 0.5}
    ref = D.energy(D.apply(val[0], idx[0], V[0]), ref_op, grad_of=(idx[0], V[0]))
    assert ref["E"] > 0 and ref["E"] == float(np.float32(ref["E"]))       # the planting is exact in fp32 as well
    out = T.run_both(ops.dirichlet_term, (torch.from_numpy(val), torch.from_numpy(idx), torch.from_numpy(V), device_op(ops, [ref_op])))
    assert np.array_equal(bits0(host(out[0])), bits0([ref["E"]]))
    assert np.array_equal(bits0(host(out[1])[0]), bits0(ref["g"]))
    assert np.array_equal(ref["g"].astype(np.float32).astype(np.float64), ref["g"])


def test_gradient_is_zero_inside_the_flat_grid_under_an_affine_map(ops):
    verts, ref_op, _, _, _ = grid_case(1)
    A = np.array([[2.0, -1.0, 0.0], [0.5, 3.0, 0.0], [-4.0, 0.25, 1.0]], np.float32)
    V = (verts @ A.T + np.float32(3))[None]
    idx = np.arange(81, dtype=np.int32)[None, :, None]
    val = np.ones((1, 81, 1), np.float32)
    loss, g = T.run_both(ops.dirichlet_term, (torch.from_numpy(val), torch.from_numpy(idx), torch.from_numpy(V), device_op(ops, [ref_op])))
    inner = D.interior(9, 9)
    assert float(loss) == 64.0 * float((A[:, :2] ** 2).sum())             # area x ||A[:, :2]||_F^2
    assert (host(g)[0, inner, 0] == 0).all() and (host(g)[0, ~inner, 0] != 0).any()


def test_capture_and_replay(ops):
    rng = np.random.default_rng(3)
    B, N, M, k, C = 2, 300, 170, 10, 3
    refs = crafted_operator(rng, B, N, [[299, 0, 1], [100]], N * 40 + 300)
    op = device_op(ops, refs)
    V = torch.from_numpy(rng.standard_normal((B, M, C)).astype(np.float32)).cuda()
    val = torch.from_numpy(rng.random((B, N, k)).astype(np.float32)).cuda()
    idx = torch.from_numpy(rng.integers(0, M, (B, N, k)).astype(np.int32)).cuda()
    eager = ops.dirichlet_term(val, idx, V, op, grad=True)
    sval = (0.5 * val).contiguous()                                       # the captured call's static input, other contents at capture time
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            ops.dirichlet_term(sval, idx, V, op, grad=True)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.dirichlet_term(sval, idx, V, op, grad=True)
    sval.copy_(val)
    graph.replay()
    torch.cuda.synchronize()
    assert T.same_bits(eager, out), "the replayed capture differs from the eager call"


def test_autograd_node_and_loss_layer(ops):
    """nn_ops.dirichlet_term through torch.autograd.grad against the reference gradient; models.loss.dirichlet_term on CUDA float32 is
    the kernel (E / norm), and V is refused as a differentiable input."""
    sys.path.insert(0, os.path.join(ROOT, "dv-matcher_amd"))
    import models.loss as ml
    from dvm import nn_ops
    rng = np.random.default_rng(21)
    B, N, M, k, C = 3, 300, 170, 10, 3
    xyz = rng.standard_normal((B, N, 3)).astype(np.float32)
    nbr = ops.knn_cdist(torch.from_numpy(xyz).cuda(), torch.from_numpy(xyz).cuda(), 8)
    op = ops.knn_laplacian(torch.from_numpy(xyz).cuda(), nbr)
    refs = [dict(rowptr=host(op.rowptr)[b], col=host(op.col)[b], w=host(op.w)[b]) for b in range(B)]
    V = rng.standard_normal((B, M, C)).astype(np.float32)
    val = rng.random((B, N, k)).astype(np.float32)
    idx = np.stack([np.stack([rng.choice(M, k, replace=False) for _ in range(N)]) for _ in range(B)]).astype(np.int32)
    want = reference_for(ops, val, idx, V, refs)
    v = torch.from_numpy(val).cuda().requires_grad_(True)
    Vd, ix = torch.from_numpy(V).cuda(), torch.from_numpy(idx).cuda()
    E = nn_ops.dirichlet_term(v, ix, Vd, op)
    assert E.requires_grad and E.dtype == torch.float32
    wts = torch.tensor([0.5, -2.0, 3.0], device="cuda")
    g, = torch.autograd.grad((E * wts).sum(), v)
    for b, ref in enumerate(want):
        sc = abs(float(wts[b]))
        gerr = np.abs(host(g)[b].astype(np.float64) - float(wts[b]) * ref["g"])
        assert (gerr <= sc * D.grad_bound(ref) + 2.0 ** -23 * sc * np.abs(ref["g"])).all()   # one more fp32 product
    check_against_reference("node", (E, ops.dirichlet_term(v, ix, Vd, op, grad=True)[1]), want)
    with torch.no_grad():
        raw = ops.dirichlet_term(v, ix, Vd, op)
        assert torch.equal(T.bits(ml.dirichlet_term(v, ix, Vd, op, normalize=False)), T.bits(raw))
        assert torch.equal(T.bits(ml.dirichlet_term(v, ix.long(), Vd, op)), T.bits(raw / op.norm))
    with pytest.raises(ValueError, match="V is data"):
        nn_ops.dirichlet_term(v, ix, Vd.clone().requires_grad_(True), op)
    # the torch fallback on the same device agrees with the kernel (what the stand-alone benchmark compares)
    fb = ml._dirichlet_term_torch(v.detach(), ix, Vd, op)
    for b, ref in enumerate(want):
        assert abs(float(fb[b]) - ref["E"]) <= D.loss_bound(ref) + 2.0 ** -23 * abs(ref["E"])


def test_identity_map_has_energy_one(ops):
    """eval_geodesic.map_dirichlet_energy on a mesh matched to itself by the identity: 1 within 1e-6, vertex form and precise form."""
    sys.path.insert(0, os.path.join(ROOT, "dv-matcher_amd"))
    from eval_geodesic import map_dirichlet_energy
    verts, faces = D.grid_mesh(12, 11, noise=0.1, seed=5)
    N = len(verts)
    e_vertex = map_dirichlet_energy(verts, faces, verts, T=np.arange(N))
    # the precise form of the identity: every vertex at a corner of one of its own faces, with that corner's weight 1
    face, bary = np.zeros(N, np.int64), np.zeros((N, 3), np.float32)
    for f, tri in enumerate(faces):
        for c, v in enumerate(tri):
            face[v], bary[v] = f, np.eye(3, dtype=np.float32)[c]
    e_precise = map_dirichlet_energy(verts, faces, verts, face=face, bary=bary, faces_tgt=faces)
    print("identity map: vertex form %.9g, precise form %.9g" % (e_vertex, e_precise))
    assert abs(e_vertex - 1.0) <= 1e-6 and abs(e_precise - 1.0) <= 1e-6
    # a map that tears the mesh apart is far from 1
    assert map_dirichlet_energy(verts, faces, verts, T=np.random.default_rng(0).permutation(N)) > 5.0
    with pytest.raises(ValueError):
        map_dirichlet_energy(verts, faces, verts)
