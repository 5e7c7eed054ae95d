"""CPU half of the bit-for-bit loss-scalar checks (tests/exact_inputs.py; the device half is tests/test_gpu_loss_scalars_exact.py).

(1) On every planted case the GPU tests use, the CPU oracle's losses[2..5] EQUAL the rational reference: the planted inputs are
    exact in fp32 through the whole chain (soft correspondence -> verts12 -> Deformer -> rot6d -> ARAP / Chamfer / map term), and the
    reference models the definitions.
(2) The reference bites: single-row mutations of each term — one point dropped, one (point, slot) dropped, a neighbour slot or a ring
    entry read one off, another node's T, one row counted twice — all change the float32 value.  Mutations are drawn (seeded, fixed)
    among those that change the exact sum at all: slot 0 of the map term and of the ring is the point / node itself and contributes
    exactly 0, as does a Chamfer row whose point coincides with a target."""
import numpy as np
import pytest

import exact_inputs as X
from oracle import oracle as O


def _oracle_losses(p, swap=False):
    a, b = ("2", "1") if swap else ("1", "2")
    return O.pair_direction(X.deformer_weights(), p["feat" + a], p["feat" + b], p["verts" + a], p["verts" + b], X.ALPHA, p["start" + a])


def _check_oracle(p, ref, swap=False):
    o = _oracle_losses(p, swap)
    assert np.array_equal(o["T12"], ref["T12"])
    assert np.array_equal(o["verts12"], ref["verts12"].astype(np.float32))
    for t in (2, 3, 4, 5):
        assert o["losses"][t] == ref["losses"][t], (t, o["losses"][t], ref["losses"][t])
    assert all(ref["losses"][t] > 0 for t in (2, 3, 4, 5))


@pytest.mark.parametrize("shape", X.PAIR_SHAPES, ids=lambda s: "%dx%d" % s)
def test_oracle_equals_rational_reference_one_way(shape):
    for b in range(3):
        p, r12, _ = X.planted_case(*shape, X.PAIR_SEED + b)
        _check_oracle(p, r12)


@pytest.mark.parametrize("shape", X.MIRRORED_SHAPES + X.MIRRORED_NOMAP_SHAPES + [(n, n) for n in X.SWAPPED_SIZES], ids=lambda s: "%dx%d" % s)
def test_oracle_equals_rational_reference_mirrored(shape):
    for b in range(3):
        p, r12, r21 = X.planted_case(*shape, X.PAIR_SEED + b, True)
        _check_oracle(p, r12)
        _check_oracle(p, r21, swap=True)


def test_oracle_decoder_returns_the_planted_rows():
    """def9 = [verts1[node], -1, 1, 0, -1, -1, 0] and R = the z rotation, exactly, from the oracle's Deformer and rot6d."""
    p, r, _ = X.planted_case(300, 170, X.PAIR_SEED)
    pval, pidx, _, _ = O.softcorr(p["feat1"], p["feat2"], X.ALPHA)
    n = (r["pval"] != 0).sum(1)
    for i in range(p["N"]):
        assert np.array_equal(pidx[i, :n[i]], r["pidx"][i, :n[i]]) and np.array_equal(pval[i], r["pval"][i].astype(np.float32))
    def9 = O.deformer(X.deformer_weights(), p["feat1"], p["feat2"], p["verts1"], r["verts12"], r["idx11"], r["idx22"], pval, pidx,
                      r["graph"]["nodes_idx"])
    assert np.array_equal(def9, r["def9"].astype(np.float32))
    R, T = O.rot6d(def9)
    assert np.array_equal(R, r["R"]) and np.array_equal(T, r["T"])


# ----------------------------------------------------------------------------------------------------------------- mutations
MUTATION_CASES = [(300, 170), (1025, 1024)]
N_MUT = 30      # per kind: 120 - 150 mutations per term and case


def _draw(rng, ok, *highs):
    """a seeded index tuple in the given ranges for which ok(*idx) holds"""
    for _ in range(10000):
        idx = tuple(int(rng.integers(lo, hi)) for lo, hi in highs)
        if ok(*idx):
            return idx
    raise AssertionError("no valid mutation")


@pytest.mark.parametrize("shape", MUTATION_CASES, ids=lambda s: "%dx%d" % s)
def test_map_term_mutations_change_the_float(shape):
    p, r, _ = X.planted_case(*shape, X.PAIR_SEED)
    rows, N, k = r["rows"]["map"], r["N"], X.K_XYZ
    total, base = rows.sum(), r["losses"][5]
    v12, v2 = r["verts12"], p["verts2"].astype(np.float64)
    rng = np.random.default_rng(11)
    vals = []
    for _ in range(N_MUT):
        i, = _draw(rng, lambda i: rows[i].sum() > 0, (0, N))
        vals.append(("drop point", total - rows[i].sum()))
        i, = _draw(rng, lambda i: rows[i].sum() > 0, (0, N))
        vals.append(("point twice", total + rows[i].sum()))
        i, s = _draw(rng, lambda i, s: rows[i, s] > 0, (0, N), (1, k))
        vals.append(("drop (point, slot)", total - rows[i, s]))
        # the targets' neighbour slot read one off: s +- 1 instead of s
        i, s, up = _draw(rng, lambda i, s, up: 0 <= s + 2 * up - 1 < k, (0, N), (0, k), (0, 2))
        s2 = s + 2 * up - 1
        acc = (r["pval"][i][:, None] * v2[r["idx22"][r["pidx"][i], s2]]).sum(0)
        e = v12[r["idx11"][i, s]] - acc
        vals.append(("neighbour slot s+-1", total - rows[i, s] + (e * e).sum()))
        # the sources' neighbour slot read one off
        i, s, up = _draw(rng, lambda i, s, up: 0 <= s + 2 * up - 1 < k, (0, N), (0, k), (0, 2))
        s2 = s + 2 * up - 1
        acc = (r["pval"][i][:, None] * v2[r["idx22"][r["pidx"][i], s]]).sum(0)
        e = v12[r["idx11"][i, s2]] - acc
        vals.append(("source slot s+-1", total - rows[i, s] + (e * e).sum()))
    assert len(vals) >= 100
    for kind, v in vals:
        assert X.f32(v) != base, kind


@pytest.mark.parametrize("shape", MUTATION_CASES, ids=lambda s: "%dx%d" % s)
def test_arap_mutations_change_the_float(shape):
    p, r, _ = X.planted_case(*shape, X.PAIR_SEED)
    rows, Nn, ring = r["rows"]["arap"], r["Nn"], r["graph"]["one_ring"]
    total, base = rows.sum(), r["losses"][2]
    rng = np.random.default_rng(12)
    vals = []
    for _ in range(N_MUT):
        a, = _draw(rng, lambda a: True, (0, Nn))
        vals.append(("drop node", total - rows[a].sum()))
        a, = _draw(rng, lambda a: True, (0, Nn))
        vals.append(("node twice", total + rows[a].sum()))
        a, q = _draw(rng, lambda a, q: rows[a, q] > 0, (0, Nn), (1, 9))
        vals.append(("drop (node, ring slot)", total - rows[a, q]))
        a, q, up = _draw(rng, lambda a, q, up: 0 <= a + 2 * up - 1 < Nn and ring[a + 2 * up - 1, q] != ring[a, q], (0, Nn), (0, 9), (0, 2))
        ring2 = ring.copy()
        ring2[a, q] = ring[a + 2 * up - 1, q]
        vals.append(("ring entry of node a+-1", X.arap_rows(r["g"], r["R"], r["T"], ring2).sum()))
        a, c = _draw(rng, lambda a, c: a != c, (0, Nn), (0, Nn))
        T2 = r["T"].copy()
        T2[a] = r["T"][c]
        vals.append(("T of another node", X.arap_rows(r["g"], r["R"], T2, ring).sum()))
    assert len(vals) >= 100
    for kind, v in vals:
        assert X.f32(v / Nn) != base, kind


@pytest.mark.parametrize("term", [3, 4])
@pytest.mark.parametrize("shape", MUTATION_CASES, ids=lambda s: "%dx%d" % s)
def test_chamfer_mean_mutations_change_the_float(shape, term):
    p, r, _ = X.planted_case(*shape, X.PAIR_SEED)
    d = r["rows"]["d1" if term == 3 else "d2"]
    total, base, n = d.sum(), r["losses"][term], d.size
    rng = np.random.default_rng(13 + term)
    vals = []
    for _ in range(2 * N_MUT):
        i, = _draw(rng, lambda i: d[i] > 0, (0, n))
        vals.append(("drop point", total - d[i]))
        i, = _draw(rng, lambda i: d[i] > 0, (0, n))
        vals.append(("point twice", total + d[i]))
        i, j = _draw(rng, lambda i, j: d[i] != d[j], (0, n), (0, n))
        vals.append(("another row's distance", total - d[i] + d[j]))
    assert len(vals) >= 100
    for kind, v in vals:
        assert X.f32(v / n) != base, kind


def test_direct_entry_references_bite():
    """the richer plantings of ops.map_term and ops.dg_warp_arap[_graph]: dropping any single row changes the float32 value"""
    m = X.map_term_direct(300, 311, 10, 10, 1)
    tot = m["rows"].sum()
    assert (m["rows"] > 0).mean() > 0.99
    for i in range(0, 300, 3):
        assert X.f32(tot - m["rows"][i].sum()) != m["value"]
    w = X.warp_direct(677, 600, 18, 1)
    tot, ts = w["arap_rows"].sum(), w["sr_rows"].sum()
    for a in range(0, 600, 6):
        assert X.f32((tot - w["arap_rows"][a].sum()) / 600) != w["arap"]
        assert w["sr_rows"][a].sum() > 0 and X.f32((ts - w["sr_rows"][a].sum()) / (600 * 18 * 9.0)) != w["sr"]
