"""CPU checks of tests/wgrad_ref.py: the exact families are exact at every shape the device test uses, the decoders name a dropped or a
doubled row, the float families' bound holds for two float32 summation orders and still detects a missing row, and the row split
restated from dvm_gemm.hip::wgrad_chunks gives the hand-computed cases."""
import numpy as np
import pytest

import wgrad_ref as WR


def test_row_split_hand_computed():
    # one tile: 1 -> 64 chunks (16401 // 128 = 128 < 256 stops the doubling), 257 rows each -> 288, recount: 57 chunks, the last one
    # holds 16401 - 56 * 288 = 273 rows = 8 steps of 32 and one of 17
    assert WR.row_split(16401, 64, 64) == (288, 57)
    assert WR.chunk_ranges(16401, 64, 64)[-1] == (16128, 16401)
    # 5 tiles: 1000 // 2 = 500 >= 256 -> 2 chunks, 1000 // 4 = 250 stops; 500 -> 512 rows, 2 chunks (512 + 488)
    assert WR.row_split(1000, 9, 262) == (512, 2)
    # 6 tiles: 513 // 2 = 256 -> 2 chunks of 257 -> 288 rows: 288 + 225
    assert WR.row_split(513, 65, 129) == (288, 2)
    assert WR.row_split(512, 64, 64) == (256, 2)
    assert WR.row_split(511, 512, 262) == (512, 1)
    assert WR.row_split(1, 7, 20) == (32, 1)
    # 8209 // 64 = 128 stops at 32 chunks of 257 -> 288 rows; 29 chunks, the last one 145 rows = 4 steps of 32 and one of 17
    assert WR.row_split(8209, 64, 64) == (288, 29)
    # many tiles: 18 * 8 = 144 tiles, 8 chunks reach 1024 workgroups
    assert WR.row_split(16384, 1152, 512) == (2048, 8)


@pytest.mark.parametrize("R,Co,K", WR.exact_cases())
def test_exact_families_stay_below_2_24(R, Co, K):
    for name in WR.EXACT_FAMILIES:
        gy, x = WR.exact_family(name, R, Co, K)
        assert gy.dtype == np.float32 and x.dtype == np.float32 and gy.shape == (R, Co) and x.shape == (R, K)
        assert np.array_equal(gy, np.rint(gy)) and np.array_equal(x, np.rint(x))
        # + the pattern `out=` is pre-filled with (|.| <= 100)
        assert WR.magnitude(gy, x).max() + 100 < 2 ** 24, (name, R, Co, K)
        ref = WR.exact_product(gy, x)
        if Co * K <= 65 * 129 or name != "ints":
            # numpy's own float32 product (BLAS: blocked, vectorised, another order) gives the same bits, and int64 matmul agrees
            assert np.array_equal(gy.T @ x, ref.astype(np.float32)), (name, R, Co, K)
            assert np.array_equal(gy.astype(np.int64).T @ x.astype(np.int64), ref), (name, R, Co, K)
    planted = WR.planted_rows(R, Co, K)
    rg = WR.chunk_ranges(R, Co, K)
    assert len(planted) <= 12 and 0 in planted and R - 1 in planted and rg[-1][0] in planted and rg[0][1] - 1 in planted
    assert rg[-1][0] + (rg[-1][1] - rg[-1][0] - 1) // 32 * 32 in planted
    assert rg[0][0] == 0 and rg[-1][1] == R and all(a[1] == b[0] for a, b in zip(rg, rg[1:]))


@pytest.mark.parametrize("R,Co,K", [(16401, 64, 64), (513, 9, 262), (1000, 65, 129), (33, 7, 20), (1, 130, 6)])
def test_bitmask_decoder_names_the_row(R, Co, K):
    planted = WR.planted_rows(R, Co, K)
    gy, x = WR.rows_bitmask(R, Co, K)
    good = WR.exact_product(gy, x)
    assert WR.decode_bitmask(good, planted, Co) == []
    for i, r in enumerate(planted):
        row = np.outer(gy[r], x[r]).astype(np.int64)
        for times, mutated in ((0, good - row), (2, good + row)):
            msg = WR.decode_bitmask(mutated, planted, Co)
            assert len(msg) == 1 and msg[0].startswith("planted row %d (number %d," % (r, i)) and "counted %d times" % times in msg[0], msg
        # a row lost in ONE column only (a store guard off by one)
        part = good.copy()
        part[:, K - 1] -= row[:, K - 1]
        msg = WR.decode_bitmask(part, planted, Co)
        assert len(msg) == 1 and "planted row %d " % r in msg[0] and "columns k %d..%d" % (K - 1, K - 1) in msg[0], msg
    assert "no count pattern" in WR.decode_bitmask(good + 0.5, planted, Co)[0]
    text = WR.explain("rows_bitmask", (good - np.outer(gy[R - 1], x[R - 1])).astype(np.float32), good, R, Co, K)
    assert "planted row %d " % (R - 1) in text and "counted 0 times" in text, text


def test_outer_decoder_names_the_element():
    R, Co, K = 33, 9, 262
    gy, x = WR.outer_index(R, Co, K)
    good = WR.exact_product(gy, x)
    assert np.array_equal(good, np.outer(np.arange(1, 10), np.arange(1, 263))) and WR.decode_outer(good) == []
    shifted = good.copy()
    shifted[:, 1:] = good[:, :-1]          # every column one to the right
    msg = WR.decode_outer(shifted)
    assert "dW[0,1] = 1.0, expected 2 (the value of dW[0,0])" in msg[1], msg
    lost = good.copy()
    lost[8, 261] = 0
    msg = WR.decode_outer(lost)
    assert msg[0].startswith("1 elements wrong, rows co 8..8, columns k 261..261") and "dW[8,261] = 0.0, expected 2358" in msg[1], msg
    assert "dW[8,261]" in WR.explain("outer_index", lost.astype(np.float32), good, R, Co, K)


@pytest.mark.parametrize("R", WR.FLOAT_R)
@pytest.mark.parametrize("name", WR.FLOAT_FAMILIES)
def test_float_bound_holds_for_two_orders_and_sees_a_missing_row(name, R):
    Co, K = 65, 129
    gy, x = WR.float_family(name, R, Co, K)
    assert gy.dtype == np.float32 and x.dtype == np.float32
    ref, b = WR.ref64(gy, x), WR.bound(gy, x)
    for what, got in (("numpy float32 product", gy.T @ x), ("sequential float32 chain", WR.chain32(gy, x))):
        ratio, nonzero = WR.worst_ratio(got, gy, x)
        print("%s R=%d %s: worst err / bound %.3f" % (name, R, what, ratio))
        assert ratio <= 1.0 and nonzero == 0, (name, R, what, ratio, nonzero)
    if name == "sparse":
        assert 0.005 < np.count_nonzero(gy) / gy.size < 0.05
        assert R > 33 or (b == 0).any()     # whole columns of gy are zero at the smallest size: those outputs must be exactly 0
    if name == "cancel":
        assert np.abs(ref).max() < 0.05 * WR.magnitude(gy, x).max()
    # a result that misses one row lies outside the bound somewhere.  The row: the one with the largest entry of gy (in `decades` a
    # row scaled by 1e-3 is legitimately below the rounding of the rows scaled by 1e3)
    r = int(np.abs(gy).max(1).argmax())
    missing = ref - np.outer(gy[r].astype(np.float64), x[r].astype(np.float64))
    assert (np.abs(missing - ref) > b).any(), (name, R, r)
    if name != "decades":       # and the last row, which a wrong `rend` loses
        missing = ref - np.outer(gy[R - 1].astype(np.float64), x[R - 1].astype(np.float64))
        assert (np.abs(missing - ref) > b).any(), (name, R)
