"""The numpy statement of the geodesic skinning rule (tests/dg_geod_ref.py) against the reference's own graphs: the three mesh
fixtures (construct_graph on real edge geodesics, Nn != N/2) and the four point-cloud fixtures (construct_graph_euclidean fed
torch.cdist computed on the CPU, rings from KDTree with k = 9).  No GPU."""
import numpy as np
import pytest
import torch

import dg_geod_ref as R

MESH = ("meshgraph_a", "meshgraph_b", "meshgraph_c")
DG = ("dg_rand_256", "dg_rand_2048", "dg_scape_512", "dg_scape_1024")


@pytest.mark.parametrize("name", MESH)
def test_statement_reproduces_mesh_fixtures(golden, name):
    g = golden(name)
    assert R.tie_free(g["geod"], g["nodes_idx"], 3), "a tie among the first four entries would hide a tie-rule difference"
    infl, dists, _ = R.skin(g["geod"], g["nodes_idx"])
    assert np.array_equal(infl, g["infl_idx"])
    assert np.array_equal(dists, g["dists"])
    w = R.weights(dists, g["sigma"])
    err = np.abs(w - g["weights"]).max()
    print("%s: V=%d Nn=%d, float64 weights vs fixture %.3g" % (name, len(g["geod"]), len(g["nodes_idx"]), err))
    assert err < 1e-7   # the fixture's weights are fp32 roundings of the same formula (measured: 3.9e-8)


@pytest.mark.parametrize("name", DG)
def test_statement_reproduces_point_cloud_fixtures(golden, name):
    g = golden(name)
    v = torch.from_numpy(g["verts"])
    cd = torch.cdist(v, v, p=2.0).numpy()
    assert R.tie_free(cd, g["nodes_idx"], 9), "a tie among the first ten entries would hide a tie-rule difference"
    infl, dists, ring = R.skin(cd, g["nodes_idx"], ring_k=9)
    assert np.array_equal(infl, g["infl_idx"])
    assert np.array_equal(ring, g["one_ring"])
    # the selected entries are this host's cdist, bit for bit; they are the fixture's bits where the host's matrix product sums
    # as the generator's did (printed), and within the rounding of the matmul form everywhere
    assert np.array_equal(dists, cd[g["nodes_idx"].astype(np.int64)[infl], np.arange(len(cd))[:, None]])
    print("%s: this host's cdist gives the fixture's dists bit for bit: %s" % (name, np.array_equal(dists, g["dists"])))
    assert R.same_up_to_cdist_rounding(dists, g["dists"])


def test_statement_rules():
    """NaN ranks as +inf, -0 == +0, ties to the lower node position, node rows read along v."""
    d = np.array([[0.0, 1.0, 2.0, 3.0],
                  [1.0, -0.0, np.nan, 3.0],
                  [5.0, 0.0, 0.0, 3.0],
                  [7.0, 7.0, np.inf, 3.0]], dtype=np.float32)
    nodes = np.array([0, 1, 2, 3])
    o = R.order(d, nodes)
    assert o[:, 0].tolist() == [0, 1, 2, 3]          # column 0: 0, 1, 5, 7
    assert o[:, 1].tolist() == [1, 2, 0, 3]          # column 1: 1, -0, 0, 7: -0 == 0 goes to the lower position
    assert o[:, 2].tolist() == [2, 0, 1, 3]          # column 2: 2, NaN, 0, inf: NaN == inf, lower position first
    assert o[:, 3].tolist() == [0, 1, 2, 3]          # all equal
    infl, dists, ring = R.skin(d, np.array([2, 3, 1]), ring_k=2)
    # vertex 0 meets nodes (rows 2, 3, 1) at 5, 7, 1
    assert infl[0].tolist() == [2, 0, 1] and dists[0].tolist() == [1.0, 5.0, 7.0]
    d2 = R.skin(d, nodes)[1][2]                       # vertex 2: 0 (row 2), 2 (row 0), then the NaN of row 1 in front of the inf
    assert d2[:2].tolist() == [0.0, 2.0] and np.isnan(d2[2])   # entries are copied unchanged
    assert ring.shape == (3, 2)
    w = R.weights(np.array([[0.0, np.inf, np.nan], [np.inf, np.inf, np.inf], [1.0, 1.0, 1.0]]), 1.0)
    assert w[0].tolist() == [1.0, 0.0, 0.0] and w[1].tolist() == [1.0, 0.0, 0.0]
    assert np.allclose(w[2], 1.0 / 3.0) and not np.isnan(w).any()
    assert R.weights(np.zeros((2, 3)), 0.0).tolist() == [[1.0, 0.0, 0.0]] * 2   # sigma = 0: 0/0
