"""-m gpu: the feature-space kNN (dvm_knn_neg_f32, csrc/dvm_knn.hip) on planted rows at every selection branch.

The selection kernels branch on the DATA of a row: how many keys pass the lane-minima threshold (one-slot / two-slot sort, exact
search), whether the threshold is tight, where a tie at the k-th key is cut, how many radix passes have something to decide.
tests/knn_select_cases.py plants rows whose scores are exact integers, so the expected (B, N, k) index tensor follows from the
construction alone, and models each kernel's decision; tests/test_knn_select_cases_cpu.py proves on the CPU that every case below
reaches the branch it is named after and that the construction equals the oracle.  Here every comparison is np.array_equal on the
whole index tensor, the oracle a second witness on the same inputs."""
import numpy as np
import pytest
import torch

import knn_select_cases as K
from oracle import oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from dvm import ops as _ops
    assert torch.cuda.is_available()
    return _ops


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def knn(ops, a, b, k):
    idx = ops.knn_neg(dev(a), dev(b), k)
    torch.cuda.synchronize()
    assert idx.dtype == torch.int32 and tuple(idx.shape) == (a.shape[0], a.shape[1], k)
    return idx.cpu().numpy()


def first_difference(got, want):
    bad = np.argwhere(got != want)
    return None if not len(bad) else (tuple(bad[0]), int(got[tuple(bad[0])]), int(want[tuple(bad[0])]), len(bad))


@pytest.mark.parametrize("i", range(len(K.TABLE)), ids=K.case_id)
def test_planted_rows(ops, i):
    c = K.table_case(i)
    got = knn(ops, c["a"], c["b"], c["k"])
    assert np.array_equal(got, c["want"]), (c["kernel"], K.score_route(c["C"]), first_difference(got, c["want"]))
    for e in range(c["B"]):   # the oracle on the same features (the queries of an entry are one row repeated)
        assert np.array_equal(O.knn_neg(c["a"][e][:1], c["b"][e], c["k"]), got[e][:1])


@pytest.mark.parametrize("M", [200, 2048, 4995])
def test_mixed_workgroup(ops, M):
    """Consecutive rows of one call on different tails (N = 1, seven batch entries: the four waves of a workgroup share cand[4][128]
    and nothing else).  Every row equals the same row run alone, and the construction."""
    k = 40
    rows = [rt for _, rt in K.mixed_rows(M, k)]
    a, b = K.build_call(rows, 64, 1, M)
    want = np.stack([K.expected(r, t, k)[None] for r, t in rows])
    got = knn(ops, a, b, k)
    assert np.array_equal(got, want), first_difference(got, want)
    for e in range(len(rows)):
        alone = knn(ops, a[e:e + 1], b[e:e + 1], k)
        assert np.array_equal(alone, got[e:e + 1]), e
    order = [3, 0, 5, 2, 6, 1, 4]                                     # the same rows in other waves
    got = knn(ops, a[order], b[order], k)
    assert np.array_equal(got, want[order]), first_difference(got, want[order])


SCALE_SHAPES = [(2, 130, 300, 40), (1, 5, 2049, 40), (1, 5, 600, 129)]     # (B, N, M, k): wave, stream and block selection


@pytest.mark.parametrize("C", [64, 128, 36])
def test_power_of_two_scaling(ops, C):
    """Scaling a and b by 2^s scales every product, partial sum and score by 4^s exactly (nothing leaves the normal range at
    s = -30 or +40 for unit-normal features): the order of the scores, ties included, and so the indices cannot move.  A kernel
    that compared against an absolute constant, or lost low bits in a reordered sum, would."""
    rng = np.random.default_rng([21, C])
    for (B, N, M, k) in SCALE_SHAPES:
        a = rng.standard_normal((B, N, C)).astype(np.float32)
        b = rng.standard_normal((B, M, C)).astype(np.float32)
        b[:, 5] = b[:, 3]
        base = knn(ops, a, b, k)
        for e in range(B):
            assert np.array_equal(base[e], O.knn_neg(a[e], b[e], k)), (M, k, e)
        for s in (-30, 40):
            f = np.float32(2.0 ** s)
            sa, sb = a * f, b * f
            assert np.array_equal(sa / f, a) and np.array_equal(sb / f, b)
            assert np.abs(sb).min() > 2.0 ** -60 and np.abs(sb).max() < 2.0 ** 50
            got = knn(ops, sa, sb, k)
            assert np.array_equal(got, base), (M, k, s, first_difference(got, base))


@pytest.mark.parametrize("C", [64, 128])
def test_self_call_equals_the_call_with_a_copy(ops, C):
    """ops.knn_neg(x, x, k) takes the shared-norm path (a == bq: one set of norms); a separate copy of x computes both."""
    rng = np.random.default_rng([22, C])
    for (B, N, k) in [(2, 130, 40), (1, 70, 64), (1, 130, 129)]:
        x = rng.standard_normal((B, N, C)).astype(np.float32)
        x[:, 9] = x[:, 2]                                             # a duplicated point: tied in every row, and twice at score 0
        xd = dev(x)
        same = ops.knn_neg(xd, xd, k)
        copy = ops.knn_neg(xd, xd.clone(), k)
        torch.cuda.synchronize()
        same, copy = same.cpu().numpy(), copy.cpu().numpy()
        assert np.array_equal(same, copy), (N, k, first_difference(same, copy))
        for e in range(B):
            assert np.array_equal(same[e], O.knn_neg(x[e], x[e], k)), (N, k, e)


NONFINITE_SHAPES = [(130, 300, 40), (5, 2049, 40), (5, 600, 129)]           # (N, M, k): wave, stream and block selection


def in_range_and_distinct(idx, M):
    assert idx.min() >= 0 and idx.max() < M, (int(idx.min()), int(idx.max()))
    srt = np.sort(idx, -1)
    assert (srt[..., 1:] != srt[..., :-1]).all()


@pytest.mark.parametrize("C", [64, 128, 36])
def test_non_finite_features_keep_indices_in_range(ops, C):
    """The kernel documents NaN-free input, but a diverged step can hand it anything and the lists feed unchecked gathers: every index
    stays in [0, M) and a list never repeats a column.  A NaN in one query row leaves every other row of the call the oracle's."""
    rng = np.random.default_rng([23, C])
    for (N, M, k) in NONFINITE_SHAPES:
        a = rng.standard_normal((2, N, C)).astype(np.float32)
        b = rng.standard_normal((2, M, C)).astype(np.float32)
        row = N // 2
        a[1, row, C // 3] = np.nan                                     # one query row, in the middle of the call
        got = knn(ops, a, b, k)
        in_range_and_distinct(got, M)
        for e in range(2):
            keep = np.array([i for i in range(N) if (e, i) != (1, row)])
            assert np.array_equal(got[e][keep], O.knn_neg(a[e][keep], b[e], k)), (N, M, k, e)
        a[1, row, C // 3] = 0.5
        b[0, M - 2, 1] = np.inf                                        # one key: a NaN or -inf score in its column of every row
        b[1, 7, C - 1] = -np.inf
        in_range_and_distinct(knn(ops, a, b, k), M)
