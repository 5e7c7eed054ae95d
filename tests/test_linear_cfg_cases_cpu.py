"""No GPU: the case table of tests/test_gpu_linear_cfgs.py (tests/linear_cfg_cases.py) is sufficient, as a condition computed from
the route predicates alone — every tile configuration of the forward GEMM meets every K-block count, both operand-load and
epilogue forms, ragged and exact tile edges, both tile orders, DMA staging and its register-staged twin — and the Python
restatement of the K-blocking is the oracle's."""
import ctypes

import pytest

import linear_cfg_cases as LC


def test_gemm_kblocks_is_the_oracles():
    from oracle import oracle as O
    lib = O.lib()
    starts = (ctypes.c_int * 34)()
    for K in range(1, 3001):
        n = lib.dvo_gemm_kblocks(K, starts, 33)
        assert LC.gemm_kblocks(K) == list(starts[:n + 1]), K


def test_predicates_on_the_values_the_table_is_built_from():
    """The reasons the dimension lists give for their values, as facts."""
    kb = LC.gemm_kblocks
    assert kb(6) == [0, 6] and LC.kvec(6) == 0
    assert kb(100) == [0, 100] and LC.kvec(100) == 1 and 100 % LC.GK and not LC.dma_ok(100)
    assert kb(384) == [0, 384] and LC.dma_ok(384)
    assert kb(400) == [0, 200, 400] and LC.kvec(400) == 1 and not LC.dma_ok(400)
    assert kb(768) == [0, 384, 768] and LC.dma_ok(768)
    assert kb(772) == [0, 384, 578, 772] and LC.kvec(772) == 0          # (772 > 768: one block of 384, then two halves)
    assert kb(1152) == [0, 384, 768, 1152] and LC.dma_ok(1152)
    assert kb(1156) == [0, 384, 768, 962, 1156] and LC.kvec(1156) == 0   # four blocks: the running total over more than three
    assert [LC.yvec(c) for c in LC.PM_CO] == [0, 1, 0, 1, 1, 1]
    assert not LC.dma_ok(384, prefix=True) and not LC.dma_ok(384, aligned=False) and LC.kvec(384, aligned=False) == 0
    assert LC.TWIN == {4: 1, 5: 1, 6: 2, 7: 3}
    for c, t in LC.TWIN.items():                      # the twin is no larger than the DMA tile in either direction
        assert LC.PM_TILE[t][0] <= LC.PM_TILE[c][0] and LC.PM_TILE[t][1] == LC.PM_TILE[c][1]
    for c in LC.PM_CFGS:                              # 256 x 512: a tile count divisible by 8 at every tile size
        ti, tj = LC.tiles(0, c, 256, 512)
        assert ti * tj % 8 == 0


def test_table_is_drawn_from_the_dimension_lists():
    for M, K, Co in LC.PM_CASES:
        assert M in LC.PM_M and K in LC.PM_K and Co in LC.PM_CO
    for N, K, Co in LC.CM_CASES:
        assert N in LC.CM_N and K in LC.CM_K and Co in LC.CM_CO
    for vals, col in ((LC.PM_M, 0), (LC.PM_K, 1), (LC.PM_CO, 2)):
        assert {t[col] for t in LC.PM_CASES} == set(vals)
    for vals, col in ((LC.CM_N, 0), (LC.CM_K, 1), (LC.CM_CO, 2)):
        assert {t[col] for t in LC.CM_CASES} == set(vals)
    assert len(set(LC.PM_CASES)) == len(LC.PM_CASES) <= 20 and len(set(LC.CM_CASES)) == len(LC.CM_CASES) <= 10
    assert LC.PREFIX_CASES[:3] == [(2, 300, 512, 256, 128), (1, 77, 8, 56, 16), (3, 64, 384, 128, 40)]
    for B, N, Cg, Cx, Co in LC.PREFIX_CASES:          # what dvm_linear_prefix_f32 accepts
        assert Cg % 4 == 0 and Cg >= 4 and LC.kvec(Cg + Cx)
    assert {Cg % LC.GK != 0 for _, _, Cg, _, _ in LC.PREFIX_CASES} == {True, False}
    assert any(Cg > 384 and Cg % 384 for _, _, Cg, _, _ in LC.PREFIX_CASES)
    for M, K, Co in LC.GUARD_CASES + [LC.OFFGRID_CASE]:
        assert (M, K, Co) in LC.PM_CASES
    assert {K for _, K, _ in LC.GUARD_CASES} == {1152, 1156} and all(Co % 4 == 0 for _, _, Co in LC.GUARD_CASES)
    assert LC.GUARD_OFFSETS == {67: 0, 64: 1} and LC.OFFGRID_CASE[1] == 384


def _features(rows, cols, bm, bn, e):
    ti, tj = e[6], e[7]
    return {"nkb": e[3], "kvec": e[4], "yvec": e[5], "row_exact": rows % bm == 0, "col_exact": cols % bn == 0,
            "remap": ti * tj % 8 == 0}


WANT = {"nkb": {1, 2, 3}, "kvec": {0, 1}, "yvec": {0, 1}, "row_exact": {False, True}, "col_exact": {False, True},
        "remap": {False, True}}


def _seen(runs):
    """the values met per feature; K-block counts beyond 3 (K = 1156 has 4) are more than is asked and dropped here"""
    return {k: {f[k] for f in runs} & WANT[k] for k in WANT}


@pytest.mark.parametrize("c", LC.PM_CFGS)
def test_point_major_table_covers_configuration(c):
    """What the child process with DVM_LINEAR_CFG=c will launch for the point-major table: the entries that land on table index c
    itself must meet every condition.  For 4..7 those are the DMA launches, where kvec is 1 by dma_ok's definition; kvec = 0 is
    then asserted of the twin's launches, and both kinds of launch must occur."""
    own, other = [], []
    for M, K, Co in LC.PM_CASES:
        e = LC.expect(c, 0, M, K, Co)
        bm, bn = LC.PM_TILE[e[1]]
        assert (e[6], e[7]) == ((M + bm - 1) // bm, (Co + bn - 1) // bn)
        (own if e[1] == c else other).append(_features(M, Co, bm, bn, e))
        assert e[2] == int(c >= 4 and e[1] == c)
    seen = _seen(own)
    if c < 4:
        assert not other and seen == WANT, (c, seen)
    else:
        assert own and other, c                       # a shape where DMA is allowed, and one where the twin must take over
        assert seen["kvec"] == {1}
        assert {k: v for k, v in seen.items() if k != "kvec"} == {k: v for k, v in WANT.items() if k != "kvec"}, (c, seen)
        assert {f["kvec"] for f in other} == {0, 1} and {f["nkb"] for f in other} >= {1, 2, 3}, c
        assert all(LC.launched(c, 0, K, Co) == (LC.TWIN[c], 0) for M, K, Co in LC.PM_CASES if not LC.dma_ok(K))


@pytest.mark.parametrize("c", LC.CM_CFGS)
def test_channel_major_table_covers_configuration(c):
    runs = []
    for N, K, Co in LC.CM_CASES:
        e = LC.expect(c, 1, None, K, Co, N=N)
        assert e[:3] == [1, c, 0]
        bm, bn = LC.CM_TILE[c]
        runs.append(_features(Co, N, bm, bn, e))
    assert _seen(runs) == WANT, (c, _seen(runs))


def test_the_eight_children_name_all_twelve_instantiations():
    """(channel_major, index, dma) over everything child c launches, c = 0..7: tables, prefix, scaled residual, guards, operands
    off the 16-byte grid.  tests/test_gpu_linear_cfgs.py asserts that each child observed exactly its set."""
    union = set()
    for c in LC.PM_CFGS:
        s = LC.expected_triples(c)
        union |= s
        if c < 4:
            assert s == {(0, c, 0), (1, c, 0)}
        else:
            assert s == {(0, c, 1), (0, LC.TWIN[c], 0), (1, 0, 0), (1, 1, 0)}
    assert union == LC.INSTANTIATIONS and len(union) == 12
