"""-m gpu: the criterion on deformation graphs skinned by its distance matrices (GraphDeformLoss_Neural.graph_metric = "geodesic",
graph_ring_metric; ops.dg_build_geod) — routing, the native training node, the graph cache, and the defaults, which keep their bits.

The two-sheet shape: two parallel 16 x 16 grids a quarter of the in-plane spacing apart.  Euclidean skinning ties vertices to
nodes of the other sheet; with the in-sheet distance (the other sheet farther than the sheet's diameter) every influence node and
every ring entry stays on the vertex's own sheet."""
import random

import numpy as np
import pytest
import torch

import dg_geod_ref as R
from oracle import oracle as O

pytestmark = pytest.mark.gpu

KW = dict(k_deform=10, w_dist=0.02, w_map=0.005, k_dist=40, N_dist=60, partial=False, w_deform=0.5, w_img=0, w_rank=0,
          w_self_rec=0.5, w_cd=0.1, w_arap=0.01, save_name="t")
GRAPH_KEYS = ("nodes_idx", "one_ring", "infl_idx", "dists", "weights", "sigma")


def host(t):
    return t.detach().cpu().numpy()


def two_sheets(seed):
    """-> verts (512,3) float32, dist (512,512) float32, sheet (512,) of 0 / 1."""
    g = np.random.default_rng(seed)
    h = 1.0 / 16
    ij = np.stack(np.meshgrid(np.arange(16), np.arange(16), indexing="ij"), -1).reshape(-1, 2) * h
    xy = np.concatenate([ij, ij]) + g.uniform(-0.2 * h, 0.2 * h, (512, 2))        # jitter: no two distances tie
    z = np.concatenate([np.zeros(256), np.full(256, 0.25 * h)]) + g.uniform(-0.02 * h, 0.02 * h, 512)
    v = np.concatenate([xy, z[:, None]], 1).astype(np.float32)
    sheet = np.repeat([0, 1], 256)
    d = np.sqrt(((v[:, None, :].astype(np.float64) - v[None, :, :]) ** 2).sum(-1))
    far = d[sheet[:, None] == sheet[None, :]].max() + 1.0                          # the sheet's diameter + 1
    d = np.where(sheet[:, None] == sheet[None, :], d, far).astype(np.float32)
    return v, d, sheet


@pytest.fixture(scope="module")
def sheets():
    v, d, sheet = two_sheets(0)
    # on the CPU first: with the statement on the oracle's FPS nodes, this shape alone satisfies both halves
    ob = O.dg_build(v, 3)
    nodes = ob["nodes_idx"].astype(np.int64)
    infl, _, ring = R.skin(d, nodes, ring_k=9)
    assert R.tie_free(d, nodes, 9)
    assert (sheet[nodes[infl]] == sheet[:, None]).all() and (sheet[nodes[ring]] == sheet[nodes][:, None]).all()
    mixed = (sheet[nodes[ob["infl_idx"]]] != sheet[:, None]).any(1)
    assert mixed.sum() >= 1, "the Euclidean graph must mix the sheets, or this fixture shows nothing"
    return v, d, sheet, int(mixed.sum())


@pytest.fixture(scope="module")
def deformer(golden):
    import models.model as mm
    w = golden("deformer_scape_r_weights")
    d = mm.Deformer(10)
    d.load_state_dict({k.replace("__", "."): torch.from_numpy(v) for k, v in w.items()})
    return d.cuda().eval()


def crit_of(metric="euclidean", ring="euclidean", **kw):
    import models.loss as ml
    c = ml.GraphDeformLoss_Neural(**dict(KW, **kw))
    c.graph_metric, c.graph_ring_metric = metric, ring
    return c


def test_two_sheets_stay_apart_under_the_geodesic_graph(sheets):
    from dvm import ops
    v, d, sheet, n_mixed = sheets
    vt, dt = torch.from_numpy(v).cuda()[None], torch.from_numpy(d).cuda()[None]
    start = torch.tensor([3], dtype=torch.int32).cuda()
    plain = ops.dg_build(vt, start)
    nodes = host(plain["nodes_idx"])[0].astype(np.int64)
    assert (sheet[nodes[host(plain["infl_idx"])[0]]] != sheet[:, None]).any(1).sum() == n_mixed >= 1
    for ring_metric in ("euclidean", "geodesic"):
        g = ops.dg_build_geod(vt, dt, start, ring_metric)
        assert np.array_equal(host(g["nodes_idx"])[0], nodes)
        assert (sheet[nodes[host(g["infl_idx"])[0]]] == sheet[:, None]).all()
        ring_own = (sheet[nodes[host(g["one_ring"])[0]]] == sheet[nodes][:, None]).all()
        assert ring_own == (ring_metric == "geodesic")      # the Euclidean ring crosses the gap, the geodesic one never does


def _pairs(seed, B, N):
    g = torch.Generator().manual_seed(seed)
    v1, v2 = torch.rand(B, N, 3, generator=g), torch.rand(B, N, 3, generator=g)
    f1 = 0.3 * torch.relu(torch.randn(B, N, 128, generator=g))
    f2 = 0.3 * torch.relu(torch.randn(B, N, 128, generator=g))
    # the library's own matmul-form distances (what dg_build's kernels compute), so that a graph skinned by them is dg_build's
    d1 = torch.from_numpy(np.stack([O.cdist(x.numpy(), x.numpy()) for x in v1]))
    d2 = torch.from_numpy(np.stack([O.cdist(x.numpy(), x.numpy()) for x in v2]))
    starts = (torch.randint(0, N, (B,), generator=g), torch.randint(0, N, (B,), generator=g))
    anchors = (list(range(0, 120, 2)), list(range(1, 121, 2)))
    return [t.cuda() for t in (v1, v2, f1, f2, d1, d2)], starts, anchors


def test_cdist_routes_to_the_default_graph(deformer):
    (v1, v2, f1, f2, d1, d2), starts, anchors = _pairs(31, 2, 300)
    plain, geod = crit_of(), crit_of("geodesic", "geodesic")
    ga, gb = plain.geometry(v1, v2, starts), geod.geometry(v1, v2, starts, None, (d1, d2))
    for side in (0, 1):
        for key in ("nodes_idx", "one_ring", "infl_idx"):
            assert torch.equal(ga[side][key], gb[side][key]), key
    with torch.no_grad():
        a = plain(f1, f2, d1, d2, v1, v2, 50.0, deformer, fps_starts=starts, anchors=anchors)
        b = geod(f1, f2, d1, d2, v1, v2, 50.0, deformer, fps_starts=starts, anchors=anchors)
    print("default", [float(x) for x in a], "geodesic graph on cdist", [float(x) for x in b])
    assert [float(x) for x in a] == [float(x) for x in b]
    with pytest.raises(ValueError):
        geod(f1, f2, None, d2, v1, v2, 50.0, deformer, fps_starts=starts, anchors=anchors)
    with pytest.raises(ValueError):
        geod.geometry(v1, v2, starts)


def test_two_sheet_matrix_changes_the_loss_and_the_warp_graph(sheets, deformer):
    from dvm import ops
    v, d, sheet, _ = sheets
    g = torch.Generator().manual_seed(5)
    v1 = torch.from_numpy(v)[None].cuda()
    v2 = (torch.from_numpy(v)[None] + 0.01 * torch.randn(1, 512, 3, generator=g)).cuda()
    f1 = (0.3 * torch.relu(torch.randn(1, 512, 128, generator=g))).cuda()
    f2 = (0.3 * torch.relu(torch.randn(1, 512, 128, generator=g))).cuda()
    dd = torch.from_numpy(d)[None].cuda()
    starts = (torch.tensor([3]), torch.tensor([3]))
    anchors = (list(range(0, 120, 2)), list(range(1, 121, 2)))
    plain, geod = crit_of(), crit_of("geodesic", "geodesic")
    g1, g2, _, _ = geod.geometry(v1, v2, starts, None, (dd, dd))
    want = ops.dg_build_geod(v1, dd, torch.tensor([3], dtype=torch.int32).cuda(), "geodesic")
    for key in GRAPH_KEYS:
        assert torch.equal(g1[key], want[key]), key
    nodes = host(g1["nodes_idx"])[0].astype(np.int64)
    assert (sheet[nodes[host(g1["infl_idx"])[0]]] == sheet[:, None]).all()
    assert (sheet[nodes[host(g1["one_ring"])[0]]] == sheet[nodes][:, None]).all()
    with torch.no_grad():
        a = plain(f1, f2, dd, dd, v1, v2, 50.0, deformer, fps_starts=starts, anchors=anchors)
        b = geod(f1, f2, dd, dd, v1, v2, 50.0, deformer, fps_starts=starts, anchors=anchors)
    assert float(a[0]) != float(b[0]) and float(a[2]) != float(b[2])       # the loss and its deformation part


def _rel(a, b):
    return float((a - b).norm() / (b.norm() + 1e-30))


def test_native_training_node_under_the_geodesic_graph(sheets):
    """native_train True / False agree under the geodesic graph at the bars tests/test_gpu_criterion_native.py sets for the default."""
    import models.model as mm
    v, d, _, _ = sheets
    g = torch.Generator().manual_seed(9)
    B, N = 2, 512
    v1 = torch.from_numpy(v)[None].repeat(B, 1, 1).cuda()
    v2 = (v1.cpu() + 0.02 * torch.randn(B, N, 3, generator=g)).cuda()
    dd = torch.from_numpy(d)[None].repeat(B, 1, 1).cuda()
    featj = (0.3 * torch.relu(torch.randn(2 * B, N, 128, generator=g))).cuda().requires_grad_(True)
    torch.manual_seed(10)
    dfm = mm.Deformer(10).cuda().train()
    crit = crit_of("geodesic", "geodesic", k_dist=50)
    starts = (torch.tensor([3, 100]), torch.tensor([7, 400]))
    anchors = (random.Random(1).sample(range(N), crit.N_dist), random.Random(2).sample(range(N), crit.N_dist))

    def step(native):
        crit.native_train = native
        dfm.zero_grad(set_to_none=True)
        featj.grad = None
        random.seed(5)
        out = crit(featj[:B], featj[B:], dd, dd, v1, v2, 60.0, dfm, fps_starts=starts, anchors=anchors)
        crit.data_parallel_loss(0.5).backward()
        return [float(o.detach()) if torch.is_tensor(o) else float(o) for o in out], featj.grad.clone(), {k: p.grad.clone() for k, p in dfm.named_parameters()}
    ln, gfn, gdn = step(True)
    la, gfa, gda = step(False)
    for x, y in zip(ln, la):
        assert abs(x - y) <= 2e-5 * max(abs(y), 1e-3), (ln, la)
    assert torch.isfinite(gfn).all()
    assert _rel(gfn, gfa) <= 2e-3, _rel(gfn, gfa)
    for k in gda:
        assert _rel(gdn[k], gda[k]) <= 2e-3, (k, _rel(gdn[k], gda[k]))
    crit.graph_metric = crit.graph_ring_metric = "euclidean"
    assert step(True)[0] != ln                                             # and the graph is what differs


def test_graph_cache_keeps_the_kinds_apart(sheets, deformer):
    v, d, _, _ = sheets
    g = torch.Generator().manual_seed(13)
    shapes = torch.stack([torch.from_numpy(v), torch.from_numpy(v) + 0.01 * torch.randn(512, 3, generator=g)]).cuda()
    feats = (0.3 * torch.relu(torch.randn(2, 512, 128, generator=g))).cuda()
    dd = torch.from_numpy(d)[None].repeat(2, 1, 1).cuda()
    starts = (torch.tensor([3]), torch.tensor([9]))
    anchors = (list(range(0, 120, 2)), list(range(1, 121, 2)))
    cached = crit_of(graph_cache={})

    def run(c, metric, ids=None):
        c.graph_metric = c.graph_ring_metric = metric
        with torch.no_grad():
            out = c(feats[:1], feats[1:], dd[:1], dd[1:], shapes[:1], shapes[1:], 50.0, deformer, fps_starts=starts, anchors=anchors,
                    shape_ids=ids)
        return [float(x) for x in out]
    fresh = {m: run(crit_of(), m) for m in ("euclidean", "geodesic")}
    assert fresh["euclidean"] != fresh["geodesic"]
    ids = (["a"], ["b"])
    for metric in ("euclidean", "geodesic", "euclidean", "geodesic"):     # fill, then hit: never the other kind's entry
        assert run(cached, metric, ids) == fresh[metric], metric
    assert len(cached.graph_cache) == 4
    assert sorted({k[3:] for k in cached.graph_cache}) == [("euclidean", "euclidean"), ("geodesic", "geodesic")]


def test_defaults_keep_their_bits(sheets, deformer):
    from dvm import ops
    from lib.deformation_graph_point import DeformationGraph_geod
    v, d, _, _ = sheets
    vt, dt = torch.from_numpy(v).cuda(), torch.from_numpy(d).cuda()
    start = torch.tensor([3], dtype=torch.int32).cuda()
    want = ops.dg_build(vt[None], start)
    dg = DeformationGraph_geod()
    dg.construct_graph_euclidean(vt, d, start=3)                           # `geod` given but not asked for: the default
    for key in GRAPH_KEYS:
        assert torch.equal(dg._g[key], want[key]), key
    c = crit_of()
    assert (c.graph_metric, c.graph_ring_metric) == ("euclidean", "euclidean")
    g1, g2, _, _ = c.geometry(vt[None], vt[None], (torch.tensor([3]), torch.tensor([3])))
    for key in GRAPH_KEYS:
        assert torch.equal(g1[key], want[key]) and torch.equal(g2[key], want[key]), key
    # and the opt-in of the graph class: a host array or a device tensor, both ring metrics
    for geod_arg, ring_metric in ((d, "euclidean"), (dt, "geodesic")):
        dg.construct_graph_euclidean(vt, geod_arg, start=3, use_geod=True, ring_metric=ring_metric)
        gw = ops.dg_build_geod(vt[None], dt[None], start, ring_metric)
        for key in GRAPH_KEYS:
            assert torch.equal(dg._g[key], gw[key]), key
    with pytest.raises(ValueError):
        dg.construct_graph_euclidean(vt, None, start=3, use_geod=True)
    with pytest.raises(ValueError):
        dg.construct_graph_euclidean(vt, d[:100], start=3, use_geod=True)
