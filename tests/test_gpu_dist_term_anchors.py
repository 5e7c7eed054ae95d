"""-m gpu: the dist-loss term (csrc/dvm_dist_loss.hip, dvm_dist_loss_fwd_f32) per ANCHOR, bit for bit on planted inputs
(tests/dist_term_exact.py; CPU half: tests/test_dist_term_exact_cpu.py) — the pin of its neighbour selection, of every neighbour slot
and of the workgroup slots.

On the planting every kNN score, every x_j and the sums sxy / sxx / syy are integers below 2^24, so the output has ONE bit pattern:
fl32(sum_n (1 - |fl(sxy) / fl(fl(sqrt sxx) fl(sqrt syy))|)).  Every exact case first asserts that the device's idx equals the planted
lists, then np.array_equal on the output — no tolerance — and that want_idx=False (neighbours kept in scratch) returns the same bits.
The CPU half shows that a dropped slot, a y from the slot before or after, a slot read twice, an x_j short of one 4-channel group
or a transposed y, applied to ANY slot j < k of any anchor, moves the output of at least one of the two batch elements.

What each family reaches:
  slots (C = 128, nA = 1)   dist_rows128: k = 1 (only the anchor: x = 0, the 1e-8 floor, term exactly 1), 2, 3, then k at and around
                            every chunk edge the case list names — slot u = j / 64 for u = 0 .. 7, lane jj or jj + 1 of a pair, an
                            odd k's dead half in the last pair, index loads clamped to k - 1 past k
  k = N (65, 129)           one cluster, no spare row: every row selected, the clamp live on every lane past k
  workgroup slots           nA = 1 .. 9 at k = 33: waves 0 .. 3 of a workgroup under the n < nA guard, (r0 + r1) + (r2 + r3), one and
                            several partials; nA = 1028 at k = 3: 257 partials, reduce_partials_kernel strides, clusters marked in two
                            channels (nA > C); anchors in shuffled order, every anchor another planting
  generic (C = 8, 36, 64, 132, nA = 5)   dist_rows_generic, one lane per neighbour: k = 1, 63, 64, 65, 200, 512; the kNN's scalar
                            (8, 36, 132) and matrix-core (64) score kernels
  degenerate anchors        all rows duplicates of the anchor (x = 0 -> 1), y = 0 (-> 1), y < 0 (|cos|), a tie across the k-th place
                            whose members differ in y (the lower row number is used), on both routes
  realistic (not exact)     N = 300 / 1100, k = 25 / 500: features a noisy linear image of the points, terms 1e-4 .. 1e-2, where
                            1 - |cos| cancels.  One anchor per call against the float64 term on the device's own idx; the bound is
                            4 x the worst error of the float32 torch evaluation of the same anchors (floor 2^-22): torch sums
                            pairwise, the kernel lane-then-tree — the same order of error, not the same value.  Measured:
                            profiles/notes_dist_term.md."""
import numpy as np
import pytest
import torch

import dist_term_exact as D
from oracle import torch_ref as TR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from dvm import ops as _ops
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _ops


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def _check_exact(ops, spec):
    c = D.planted_case(*spec)
    feat, dist, anchors = dev(c["feat"]), dev(c["dist"]), dev(c["anchors"])
    out, idx = ops.dist_loss(feat, dist, anchors, c["k"], want_idx=True)
    out, idx = host(out), host(idx)
    assert np.array_equal(idx, c["lists"]), "the device selected other neighbours than the planted ones"
    print(D.case_id(spec), "device", out, "reference", c["out"], "ulps", D.ulp_distance(out, c["out"]))
    assert np.array_equal(out, c["out"]), (out, c["out"], D.ulp_distance(out, c["out"]))
    scratch = host(ops.dist_loss(feat, dist, anchors, c["k"]))       # want_idx=False: the neighbours stay in scratch
    assert np.array_equal(scratch, out), (scratch, out)
    return c


@pytest.mark.parametrize("spec", D.SLOT_CASES, ids=D.case_id)
def test_every_slot_c128(ops, spec):
    c = _check_exact(ops, spec)
    if c["k"] == 1:
        assert np.array_equal(c["out"], np.ones(2, np.float32))       # x all zero: the floored norm, a term of exactly 1


@pytest.mark.parametrize("spec", D.FULL_CASES, ids=D.case_id)
def test_k_equals_n(ops, spec):
    c = _check_exact(ops, spec)
    assert c["k"] == c["N"]


@pytest.mark.parametrize("spec", D.WG_CASES, ids=D.case_id)
def test_workgroup_slots_and_reduction(ops, spec):
    _check_exact(ops, spec)


@pytest.mark.parametrize("spec", D.GENERIC_CASES, ids=D.case_id)
def test_generic_route(ops, spec):
    _check_exact(ops, spec)


@pytest.mark.parametrize("spec", D.DEGENERATE_CASES, ids=D.case_id)
def test_degenerate_anchors(ops, spec):
    c = _check_exact(ops, spec)
    kinds = np.array(c["kinds"])
    assert (c["terms"][:, (kinds == "dup") | (kinds == "yzero")] == 1.0).all()
    # each kind alone, one anchor per call: the term itself, exactly
    feat, dist = dev(c["feat"]), dev(c["dist"])
    for n in range(c["nA"]):
        out, idx = ops.dist_loss(feat, dist, dev(c["anchors"][n:n + 1]), c["k"], want_idx=True)
        assert np.array_equal(host(idx)[:, 0], c["lists"][:, n]), (n, kinds[n])
        assert np.array_equal(host(out), c["terms"][:, n].astype(np.float32)), (n, kinds[n], host(out), c["terms"][:, n])


# ------------------------------------------------------------------------------------------------- realistic inputs, per anchor
@pytest.mark.parametrize("N,k", D.REAL_CASES, ids=lambda v: str(v))
def test_realistic_terms_per_anchor_float64(ops, N, k):
    c = D.realistic_case(N, k)
    feat_h, dist_h = torch.from_numpy(c["feat"])[None], torch.from_numpy(c["dist"])[None]
    feat, dist = dev(c["feat"][None]), dev(c["dist"][None])
    err_cpu, err_dev, single = [], [], []
    for a in c["anchors"]:
        at = torch.tensor([int(a)])
        sel = TR.knn_scores(feat_h[:, at], feat_h).topk(k, dim=-1)[1][0].numpy()          # the selection dist_loss_term makes
        t32 = float(TR.dist_loss_term(feat_h, dist_h, at, k)[0])
        err_cpu.append(abs(t32 - D.terms_f64_on_lists(c["feat"], c["dist"], [a], sel)[0]))
        out, idx = ops.dist_loss(feat, dist, dev(np.array([a], np.int32)), k, want_idx=True)
        idx = host(idx)[0]
        assert idx.shape == (1, k) and len(set(idx[0].tolist())) == k and idx[0, 0] == a
        ref = D.terms_f64_on_lists(c["feat"], c["dist"], [a], idx)[0]
        assert 1e-5 < ref < 2e-2
        single.append(float(host(out)[0]))
        err_dev.append(abs(single[-1] - ref))
    bound = max(4.0 * max(err_cpu), 2.0 ** -22)
    print("N=%d k=%d: float32 torch on the CPU, worst |err| %.3e; kernel, worst |err| %.3e; bound %.3e" % (N, k, max(err_cpu), max(err_dev), bound))
    assert max(err_dev) <= bound, (max(err_dev), bound)
    # the same 16 anchors in one call: four workgroups of four waves, one sum
    total = float(host(ops.dist_loss(feat, dist, dev(c["anchors"]), k))[0])
    s = float(np.sum(np.array(single, np.float64)))
    assert abs(total - s) <= (len(single) + 1) * 2.0 ** -24 * max(1.0, s), (total, s)
