"""CPU half of the per-anchor dist-term checks (tests/dist_term_exact.py; the device half is tests/test_gpu_dist_term_anchors.py).

For every case the GPU test runs:
(1) the builder's own assertions hold (planted_case raises otherwise): every score the kNN forms and the three sums of every anchor
    are integers below 2^24;
(2) the planted neighbour lists EQUAL the CPU oracle's knn_neg, boundary ties included;
(3) the rational term agrees with oracle/torch_ref.py::dist_loss_term in float64 to 1e-12 per batch element.  torch.topk does not
    promise an order among equal scores, so the float64 form of the reference is evaluated on torch's own selection, which must be
    the planted one up to members of a tie (the same x, row for row);
(4) the reference bites: for EVERY slot j < k of every anchor, a dropped slot, y taken from slot j - 1 or j + 1, slot j + 1 read
    twice, x_j formed without one of its 4-channel groups and y read transposed each change the float32 output of at least one of the
    case's batch elements.  No pair escapes; the exemptions are the ones arithmetic forces (listed in dist_term_exact.py)."""
import numpy as np
import pytest
import torch

import dist_term_exact as D
from oracle import oracle as O
from oracle import torch_ref as TR


@pytest.mark.parametrize("spec", D.ALL_CASES, ids=D.case_id)
def test_planted_lists_equal_the_oracle_knn(spec):
    c = D.planted_case(*spec)
    assert np.array_equal(c["out"].astype(np.float64).astype(np.float32), c["out"]) and np.isfinite(c["out"]).all()
    for b in range(c["B"]):
        idx = O.knn_neg(c["feat"][b][c["anchors"]], c["feat"][b], c["k"])
        assert np.array_equal(idx, c["lists"][b])


@pytest.mark.parametrize("spec", D.ALL_CASES, ids=D.case_id)
def test_rational_term_agrees_with_torch_float64(spec):
    c = D.planted_case(*spec)
    feat, dist = torch.from_numpy(c["feat"]).double(), torch.from_numpy(c["dist"]).double()
    anchors = torch.from_numpy(c["anchors"]).long()
    ref = TR.dist_loss_term(feat, dist, anchors, c["k"]).numpy()
    sel = TR.knn_scores(feat[:, anchors], feat).topk(c["k"], dim=-1)[1].numpy()     # the selection dist_loss_term made
    for b, el in enumerate(c["elements"]):
        rank = np.empty((c["nA"], c["N"]), np.int64)
        rank[:] = -1
        rank[np.arange(c["nA"])[:, None], el["rows"]] = np.arange(c["S"])[None]
        r = np.take_along_axis(rank, sel[b], 1)
        assert (r >= 0).all()
        x, y = np.take_along_axis(el["xs"], r, 1), np.take_along_axis(el["ys"], r, 1)
        assert np.array_equal(np.sort(x, 1), el["xs"][:, :c["k"]])               # the planted list up to members of a tie
        t64 = D.term_f64(*D.sums(x, y))
        assert abs(t64.sum() - ref[b]) <= 1e-12, (b, t64.sum(), ref[b])
        untied = np.array([np.array_equal(np.sort(sel[b, n]), np.sort(c["lists"][b, n])) for n in range(c["nA"])])
        # float32 against float64 on the planted lists: three roundings of values near 1
        assert np.abs(D.term_f64(*D.sums(el["xs"][:, :c["k"]], el["ys"][:, :c["k"]])) - c["terms"][b]).max() <= 4 * 2.0 ** -24
        assert np.abs(t64 - c["terms"][b])[untied].max(initial=0.0) <= 4 * 2.0 ** -24


@pytest.mark.parametrize("spec", D.ALL_CASES, ids=D.case_id)
def test_every_slot_mutation_moves_the_output(spec):
    c = D.planted_case(*spec)
    escapes = D.mutation_escapes(c)
    assert not escapes, (len(escapes), escapes[:10])


def test_exemptions_are_forced_by_arithmetic():
    """k = 1 and the degenerate kinds give exactly 1; at k = 2 the cosine does not depend on x_1 > 0."""
    assert np.array_equal(D.planted_case(*D.SLOT_CASES[0])["terms"], np.ones((2, 1)))
    c = D.planted_case(*D.DEGENERATE_CASES[0])
    kinds = np.array(c["kinds"])
    assert (c["terms"][:, (kinds == "dup") | (kinds == "yzero")] == 1.0).all()
    assert ((c["terms"][:, kinds == "yneg"] > 0) & (c["terms"][:, kinds == "yneg"] < 1)).all()
    for b, el in enumerate(c["elements"]):
        for n in np.flatnonzero(kinds == "tie"):      # two rows tied across the k-th place, different y, the lower row number in the list
            k = c["k"]
            assert el["xs"][n, k - 1] == el["xs"][n, k] and el["ys"][n, k - 1] != el["ys"][n, k] and el["rows"][n, k - 1] < el["rows"][n, k]
    y0, y1 = 7.0, 24.0
    t = [D.term_f32(x1 * y1, x1 * x1, y0 * y0 + y1 * y1)[0] for x1 in (1.0, 3.0, 40.0)]
    assert t[0] == t[1] == t[2]


def test_case_list_covers_what_the_kernel_branches_on():
    ks = {s[1] for s in D.SLOT_CASES}
    assert {1, 2, 3, 63, 64, 65, 127, 128, 129, 511, 512} <= ks and any(k % 2 for k in ks)
    assert {s[2] for s in D.WG_CASES} >= {1, 2, 3, 4, 5, 7, 8, 9, 1028}
    assert all(s[1] == s[3] for s in D.FULL_CASES)
    assert {36, 64} <= set(D.GENERIC_CS) and 128 not in D.GENERIC_CS
    a = D.planted_case(*D.WG_CASES[7])["anchors"]
    assert (np.diff(a) < 0).any() and (np.diff(a) > 0).any()             # shuffled, non-monotone
    assert {4, 16, 64} <= set(D.offset_shapes(128)) and D.offset_shapes(36) == [1, 4, 16]
