"""CPU half of the planted kNN selection checks (tests/knn_select_cases.py; the device half is tests/test_gpu_knn_select.py).

For every case the GPU test runs:
(1) the planting's own assertions hold (plant() raises otherwise): every integer the scores are formed from stays below 2^24 and the
    score is -(r^2 + t) exactly;
(2) the construction's expected list EQUALS the CPU oracle's knn_neg on the planted features, tie order included;
(3) the branch models (wave_branch / select_branch on the exact scores) report the branch the family is named after, for every batch
    entry of the case;
and the case table covers every family on every selection kernel, every (kernel, tail) pair, both kinds of tie cut, every shape and
every score route the device test is meant to reach: the table cannot shrink unnoticed."""
import numpy as np
import pytest

import knn_select_cases as K
from oracle import oracle as O

ALL = range(len(K.TABLE))


@pytest.mark.parametrize("i", ALL, ids=K.case_id)
def test_expected_list_equals_the_oracle(i):
    c = K.table_case(i)
    assert c["want"].shape == (c["B"], c["N"], c["k"]) and c["a"].dtype == np.float32 and c["b"].dtype == np.float32
    for e in range(c["B"]):
        assert np.array_equal(O.knn_neg(c["a"][e][:1], c["b"][e], c["k"]), c["want"][e][:1])
        assert len(set(c["want"][e][0])) == c["k"]
    for e in range(1, c["B"]):   # a planting per entry
        assert not np.array_equal(c["a"][e], c["a"][0]) or not np.array_equal(c["b"][e], c["b"][0])


def test_planting_bound_is_checked_and_binds():
    """plant() accepts the largest rank with every sign and channel, and refuses a rank whose norm leaves the exact range"""
    for C in (36, 64, 128):
        for seed in range(8):
            rng = np.random.default_rng([3, C, seed])
            r = np.concatenate([[0, 1, K.RMAX, K.RMAX], rng.integers(0, K.RMAX + 1, 60)])
            t = np.concatenate([[0, C - 2, C - 2, 0], rng.integers(0, C - 1, 60)])
            u, b = K.plant(rng, C, r, t)
            ub, bb = u.astype(np.int64), b.astype(np.int64)
            assert np.array_equal(ub, u) and np.array_equal(bb, b) and np.abs(bb).max() <= K.RMAX + 1
            assert max((bb * bb).sum(1).max(), np.abs(bb).sum(1).max()) < K.LIMIT
            assert np.array_equal(K.scores(r, t), -((ub - bb) ** 2).sum(1).astype(np.float32))
    assert (K.RMAX + 1) ** 2 + 4 * 126 + 128 < K.LIMIT
    with pytest.raises(AssertionError):
        K.plant(np.random.default_rng(0), 128, np.array([4200]))


def test_desc_key_orders_like_the_float_scores():
    rng = np.random.default_rng(5)
    s = np.concatenate([rng.standard_normal(500) * 10.0 ** rng.integers(-20, 20, 500), [0.0, -0.0, np.inf, -np.inf, 1.0, 1.0]])
    s = rng.permutation(s.astype(np.float32))
    key = K.desc_key(s)
    assert key.dtype == np.uint32
    order = np.argsort(key, kind="stable")
    assert np.array_equal(s[order], np.sort(s)[::-1])
    assert key[s == np.inf][0] == key.min() and key[s == -np.inf][0] == key.max() < K.PAD
    same = np.flatnonzero(s == 1.0)
    assert key[same[0]] == key[same[1]]
    # the planted scores: integers, exact, ordered by rank
    r = rng.integers(0, K.RMAX + 1, 300)
    assert np.array_equal(np.argsort(K.desc_key(K.scores(r)), kind="stable"), np.argsort(r, kind="stable"))


def _tail_of(C):
    return "one-slot" if C <= 64 else "two-slot" if C <= 128 else "exact-search"


def _models(c):
    model = K.wave_branch if c["k"] <= 64 else K.select_branch
    return [model(K.scores(r, t), c["k"]) for r, t in c["rows"]]


@pytest.mark.parametrize("i", ALL, ids=K.case_id)
def test_families_are_what_they_claim(i):
    c = K.table_case(i)
    fam, M, k, arg = c["family"], c["M"], c["k"], c["arg"]
    for (r, t), want, m in zip(c["rows"], c["want"][:, 0], _models(c)):
        if k <= 64:
            assert m["tail"] == _tail_of(m["C"])
            slots = -(-M // 64)
            if fam == "spread":
                assert m["exact"] and m["C"] == k and m["max_lane"] == 1
            elif fam == "pairs":
                assert m["exact"] and m["C"] == k and m["max_lane"] == 2
            elif fam == "triple":
                assert not m["exact"] and m["C"] == k + arg + 1 and m["max_lane"] == 3 and m["tied"] == 1
                assert want[0] == np.flatnonzero(r < K.FAR).max()                # the best key is the last candidate in column order
            elif fam == "stacked":
                assert m["tail"] == "exact-search" and not m["exact"] and m["tied"] == 1 and m["max_lane"] == min(k, slots)
            elif fam == "tie_edge":
                assert m["exact"] and m["C"] == k - 1 + arg and m["tied"] == arg
                tied = np.flatnonzero(r == k - 1)
                if arg >= 2:
                    assert tied.max() >= 64 * (slots - 1)                        # one in the last slot
                    assert k == 1 or tied.min() < want[:k - 1].max()             # one in a column below a winner
                if arg >= 64:
                    assert len(set(tied // 64)) >= min(slots, 4)                 # scattered over the slots
            elif fam == "all_equal":
                assert m["exact"] and m["C"] == M and m["tied"] == M and np.array_equal(want, np.arange(k))
            elif fam == "ends":
                assert m["exact"] and m["C"] == k and m["max_lane"] <= 2 and want[0] == M - 1
                assert k == 1 or (want[-1] == 0 and np.array_equal(want[:-1], M - 1 - np.arange(k - 1)))
            elif fam == "chunk_edges":
                e = K.chunk_edge_columns(c["B"], c["N"], M)
                kchunk, nz = K.key_chunk(c["B"], c["N"], M)
                assert set(want[:min(k, len(e))]) <= set(e) and (len(e) > k or set(e) <= set(want))
                assert M - 1 in e and 64 * ((M - 1) // 64) in e and all(q * kchunk in e and q * kchunk - 1 in e for q in range(1, nz))
            else:
                raise AssertionError(fam)
        else:
            if fam == "low_byte":
                assert m["multi_bin_passes"] == (4 if arg else 1) and m["tied"] >= 2
                assert m["cut"] != "none" or not arg
                d = r * r + t
                assert not arg or (d[want[-1]] >> 8 == (K.LOW_P ** 2) >> 8 and (1 << 23) <= d[want[-1]] < (1 << 24))
            elif fam == "tie_cut":
                assert m["cut"] == arg and m["tied"] == 13 and m["remaining"] == 7
            elif fam == "all_equal":
                ept = K.ept_of(M)
                assert m["tied"] == M and m["remaining"] == k and m["multi_bin_passes"] == 0 and np.array_equal(want, np.arange(k))
                assert m["cut"] == ("none" if M == k else "inside" if (k - 1) // ept == k // ept else "between")
            elif fam == "ends":
                assert m["cut"] == "none" and m["tied"] == 1 and m["multi_bin_passes"] >= 1 and want[0] == M - 1 and want[-1] == 0
            else:
                raise AssertionError(fam)


def test_models_on_rows_worked_by_hand():
    """the models themselves, on rows small enough to follow"""
    s = np.float32(0) - np.arange(200, dtype=np.float32)          # column j scores -j: the winners are columns 0 .. k - 1
    m = K.wave_branch(s, 40)                                       # one per lane
    assert m == dict(C=40, exact=True, tail="one-slot", max_lane=1, tied=1)
    s2 = s.copy()
    s2[[0, 64, 128]] = [5.0, 4.0, 3.0]                             # lane 0 holds the three best: its third is no lane minimum
    m = K.wave_branch(s2, 3)
    assert not m["exact"] and m["max_lane"] == 3 and m["C"] == 4 and m["tail"] == "one-slot"   # Tc = column 1's key
    assert K.wave_branch(np.zeros(129, np.float32), 2) == dict(C=129, exact=True, tail="exact-search", max_lane=1, tied=129)
    assert K.wave_branch(np.zeros(128, np.float32), 2)["tail"] == "two-slot"
    # block kernel: 300 columns (8 per thread), all equal: the cut after column k - 1
    z = np.zeros(300, np.float32)
    assert K.select_branch(z, 72)["cut"] == "between" and K.select_branch(z, 73)["cut"] == "inside"
    assert K.select_branch(z, 300) == dict(multi_bin_passes=0, tied=300, remaining=300, cut="none", kp2=512)
    v = np.float32(0) - np.array([1.0, 2.0, 2.0 ** 20, 2.0 ** 20 + 1.0] * 75, np.float32)
    m = K.select_branch(v, 200)                                    # 75 each of 1 and 2, then 50 of the 75 keys 2^20
    # 0x3f800000, 0x40000000, 0x49800000, 0x49800008: the top byte and, among the 0x4980 00xx, the low byte decide
    assert m["tied"] == 75 and m["remaining"] == 50 and m["multi_bin_passes"] == 2 and m["kp2"] == 256


def test_launch_rules_match_the_host_code():
    """kernel_of / key_chunk restate launch_knn_neg: read the thresholds back from the source"""
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "dv-matcher_amd", "csrc", "dvm_knn.hip")).read()
    host = src[src.index("int launch_knn_neg"):]
    for needle in ("KS_KT = 64, KS_QB = 128", "while (B * qtiles * nz < 1024 && nz * 2 <= ktiles) nz *= 2;",
                   "const int kchunk = ((ktiles + nz - 1) / nz) * KS_KT;", "nz = (M + kchunk - 1) / kchunk;",
                   "if (k <= 64 && M <= 8192)", "if (M <= 2048)", "int ept = (M + 255) / 256;", "if (C == 128)", "else if (C == 64)"):
        assert needle in src, needle
    assert re.search(r"topk_wave_kernel<32>", host) and "if (C <= 128)" in src and "const bool small = base <= 64;" in src
    assert K.key_chunk(1, 1, 4995) == (128, 40) and K.key_chunk(8, 2048, 2048) == (256, 8) and K.key_chunk(3, 130, 40) == (64, 1)
    assert [K.kernel_of(M, 64) for M in (2048, 2049)] == ["wave", "stream"]
    assert [K.kernel_of(M, 65) for M in (65, 2048, 2049, 4096, 4097, 8192)] == ["select8"] * 2 + ["select16"] * 2 + ["select32"] * 2


def test_table_covers_every_kernel_branch_and_shape():
    seen, tails, cuts = set(), set(), set()
    for i in ALL:
        c = K.table_case(i)
        seen.add((c["family"], c["kernel"]))
        for m in _models(c):
            if c["k"] <= 64:
                tails.add((c["kernel"], m["tail"], m["exact"], m["tied"] > 1))
            else:
                cuts.add((c["kernel"], m["cut"], m["multi_bin_passes"] == 4, m["kp2"]))
    # every family on every kernel of its range
    assert {(f, kn) for f in K.WAVE_FAMILIES for kn in ("wave", "stream")} | \
        {(f, "select%d" % e) for f in K.BLOCK_FAMILIES for e in (8, 16, 32)} == seen
    for kn in ("wave", "stream"):
        for tail in ("one-slot", "two-slot", "exact-search"):
            assert any(t[:2] == (kn, tail) for t in tails), (kn, tail)
            assert (kn, tail, False, False) in tails, (kn, tail)          # reached by a loose threshold, no tie involved
        for tail in ("one-slot", "two-slot", "exact-search"):
            assert (kn, tail, True, True) in tails, (kn, tail)            # reached by ties at an exact threshold
    # the candidate counts on both sides of each tail's limit, with k = 40
    for kn, M, k in (("wave", 2047, 64), ("wave", 2048, 63), ("stream", 4995, 64), ("stream", 8192, 40)):   # ... under a loose threshold
        cs = {K.wave_branch(K.scores(*K.table_case(i)["rows"][0]), k)["C"] for i in ALL if K.TABLE[i][:3] == ("triple", M, k)}
        assert cs & {64, 65, 128, 129}, (kn, M, k, cs)
    loose = {K.wave_branch(K.scores(*K.table_case(i)["rows"][0]), K.TABLE[i][2])["C"] for i in ALL if K.TABLE[i][0] == "triple"}
    assert {64, 65, 128, 129} <= loose
    for M in (200, 4995):
        assert {K.wave_branch(K.scores(*K.table_case(i)["rows"][0]), 40)["C"] for i in ALL
                if K.TABLE[i][:3] == ("tie_edge", M, 40)} == {64, 65, 128, 129}
    for e in (8, 16, 32):
        kn = "select%d" % e
        assert {c[1] for c in cuts if c[0] == kn} == {"none", "inside", "between"}
        assert any(c[0] == kn and c[2] for c in cuts)
    assert {c[3] for c in cuts} == {128, 256, 512}
    wave = [row for row in K.TABLE if row[2] <= 64]
    block = [row for row in K.TABLE if row[2] > 64]
    assert {row[1] for row in wave} == set(K.WAVE_MS + K.STREAM_MS) and {row[2] for row in wave} == set(K.WAVE_KS)
    assert {(40, 40), (64, 64)} <= {row[1:3] for row in wave}                                     # k = M
    assert {row[2] for row in block} == set(K.BLOCK_KS)
    assert {row[1] for row in block} >= {300, 2048, 2049, 4096, 4097, 8192} and any(row[1] == row[2] for row in block)
    for kn in ("wave", "stream", "select8", "select16", "select32"):
        mine = [row for row in K.TABLE if K.kernel_of(row[1], row[2]) == kn]
        assert {K.score_route(row[4]) for row in mine} == {"mfma", "dma", "scalar"}, kn
        assert {row[5] for row in mine} == {1, 5, 130} and {row[6] for row in mine} == {1, 2, 3}, kn
    # a winner in the last partial key tile and on a ragged chunk edge
    assert any(row[0] == "chunk_edges" and row[1] % 64 and K.key_chunk(row[6], row[5], row[1])[0] > 64 for row in K.TABLE)


@pytest.mark.parametrize("M", [200, 2048, 4995])
def test_mixed_workgroup_rows_take_the_tails_they_name(M):
    rows = K.mixed_rows(M, 40)
    names = [n for n, _ in rows]
    assert set(names) == {"one-slot", "two-slot", "exact-search", "all_equal"} and all(a != b for a, b in zip(names, names[1:]))
    for name, (r, t) in rows:
        m = K.wave_branch(K.scores(r, t), 40)
        assert m["tail"] == ("exact-search" if name == "all_equal" else name), (name, m)
        assert (m["tied"] == M) == (name == "all_equal")
    a, b = K.build_call([rt for _, rt in rows], 64, 1, M)
    for e, (_, (r, t)) in enumerate(rows):
        assert np.array_equal(O.knn_neg(a[e], b[e], 40)[0], K.expected(r, t, 40))
