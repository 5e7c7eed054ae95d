"""Helpers for the per-element tests of the weight-gradient GEMM (csrc/dvm_gemm.hip::linear_wgrad_kernel, dW = gy^T x over the rows):
the library's row split restated, input families whose answer is ONE bit pattern on every route, float families with a derived
bound, and decoders that turn a wrong element into the row or element at fault.  Used by tests/test_gpu_wgrad_elements.py (device)
and tests/test_wgrad_ref_cpu.py (the same checks on numpy products and on planted mutations).  numpy only.

Exact families.  Every product and every partial sum is an integer below 2^24, so fp32 adds them without rounding in ANY order:
atomics, per-chunk partials, the matrix instruction's chain and numpy's BLAS all give the same bits.
    ints          entries in {-2..2}; 4 R < 2^24 (asserted from the data).
    rows_bitmask  all rows zero except <= 12 planted ones; planted row number i has gy[r, i % Co] = 1 and x[r, :] = 4^i, so
                  dW[co, k] written in base 4 has digit i = how often planted row i was summed (1 expected).  The rows sit on the
                  edges of the split (planted_rows).
    outer_index   only row R - 1 is non-zero: gy = co + 1, x = k + 1, dW[co, k] = (co + 1)(k + 1): a transposed or shifted ragged
                  tile shows up under the name of its element.

Float families (R in FLOAT_R).  bound() = R 2^-24 (|gy|^T |x|): the any-order summation bound — a sum of R exactly formed products
(the kernel's fma chain rounds once per step; partial sums are bounded by the sum of magnitudes) errs by at most (R - 1) u times the
sum of magnitudes, and the chunk adds and atomics are part of the same R - 1 additions.  Derived, never measured; where it is 0 the
output must be exactly 0."""
import numpy as np

U = 2.0 ** -24
WG_ROWS = 32          # rows per staged step of the kernel
ARENA_ALIGN = 256     # dvm_common.h::align_up

SHAPES = [(64, 64), (9, 262), (512, 262), (65, 129), (68, 196), (7, 20), (130, 6), (192, 64)]   # (Co, K)
R_ALL = [1, 31, 32, 33, 511, 512, 513, 1000]
R_ONE_TILE = [8209, 16401]
FLOAT_R = [33, 300, 1000]
EXACT_FAMILIES = ("ints", "rows_bitmask", "outer_index")
FLOAT_FAMILIES = ("randn", "decades", "cancel", "sparse")


def one_tile(Co, K):
    return Co <= 64 and K <= 64


def exact_cases():
    """every (R, Co, K) the exact families run at"""
    return [(R, Co, K) for Co, K in SHAPES for R in R_ALL + (R_ONE_TILE if one_tile(Co, K) else [])]


def row_split(R, Co, K):
    """(rchunk, chunks) of dvm_gemm.hip::wgrad_chunks: double the chunk count while there are fewer than 1024 workgroups and the
    halves keep at least 256 rows, round the rows per chunk up to the 32-row step, recount."""
    tiles = ((Co + 63) // 64) * ((K + 63) // 64)
    chunks = 1
    while tiles * chunks < 1024 and R // (2 * chunks) >= 256:
        chunks *= 2
    rchunk = (R + chunks - 1) // chunks
    rchunk = (rchunk + WG_ROWS - 1) // WG_ROWS * WG_ROWS
    return rchunk, (R + rchunk - 1) // rchunk


def chunk_ranges(R, Co, K):
    rchunk, chunks = row_split(R, Co, K)
    return [(c * rchunk, min((c + 1) * rchunk, R)) for c in range(chunks)]


def planted_rows(R, Co, K):
    """<= 12 distinct rows on the edges of the split: row 0, row R - 1, first and last row of the first, a middle and the last chunk,
    rows 31 and 32 of the first and of the last chunk, the first row of the last chunk's last 32-row step."""
    rg = chunk_ranges(R, Co, K)
    last = rg[-1]
    cand = [0, R - 1]
    for b, e in (rg[0], rg[len(rg) // 2], last):
        cand += [b, e - 1]
    cand += [rg[0][0] + 31, rg[0][0] + 32, last[0] + 31, last[0] + 32, last[0] + (last[1] - last[0] - 1) // WG_ROWS * WG_ROWS]
    rows = []
    for r in cand:
        if 0 <= r < R and r not in rows:
            rows.append(r)
    return rows[:12]


# ------------------------------------------------------------------------------------------------------------------ exact families
def ints(R, Co, K, seed=0):
    g = np.random.default_rng([seed, R, Co, K, 1])
    gy = g.integers(-2, 3, (R, Co)).astype(np.float32)
    x = g.integers(-2, 3, (R, K)).astype(np.float32)
    return gy, x


def rows_bitmask(R, Co, K, planted=None):
    planted = planted_rows(R, Co, K) if planted is None else list(planted)
    assert len(planted) <= 12 and len(set(planted)) == len(planted)
    gy, x = np.zeros((R, Co), np.float32), np.zeros((R, K), np.float32)
    for i, r in enumerate(planted):
        gy[r, i % Co] = 1.0
        x[r, :] = 4.0 ** i
    return gy, x


def outer_index(R, Co, K):
    gy, x = np.zeros((R, Co), np.float32), np.zeros((R, K), np.float32)
    gy[R - 1] = np.arange(1, Co + 1)
    x[R - 1] = np.arange(1, K + 1)
    return gy, x


def exact_family(name, R, Co, K):
    gy, x = {"ints": ints, "rows_bitmask": rows_bitmask, "outer_index": outer_index}[name](R, Co, K)
    assert magnitude(gy, x).max() < 2 ** 24, (name, R, Co, K)
    return gy, x


def magnitude(gy, x):
    """|gy|^T |x| in float64"""
    return np.abs(gy).astype(np.float64).T @ np.abs(x).astype(np.float64)


def exact_product(gy, x):
    """The product as int64.  Formed in float64: entries are integers and every partial sum stays below 2^24 (asserted), far inside
    float64's 2^53, so the float64 BLAS product IS the integer product (tests/test_wgrad_ref_cpu.py checks it against int64 matmul)."""
    assert magnitude(gy, x).max() < 2 ** 24
    p = gy.astype(np.float64).T @ x.astype(np.float64)
    q = p.astype(np.int64)
    assert np.array_equal(q, p)
    return q


# ------------------------------------------------------------------------------------------------------------------ decoders
def decode_bitmask(got, planted, Co):
    """got (Co,K) from a rows_bitmask input -> list of complaints naming the planted row: (row, times counted, columns k affected)."""
    got = np.asarray(got, np.float64)
    out = []
    whole = (got == np.rint(got)) & (got >= 0) & (got < 2 ** 30)
    if not whole.all():
        co, k = np.argwhere(~whole)[0]
        out.append("dW[%d,%d] = %r is no count pattern" % (co, k, float(got[co, k])))
    v = np.where(whole, got, 0).astype(np.int64)
    for i, r in enumerate(planted):
        digit = (v >> (2 * i)) & 3          # (a row counted 4 times or more carries into the next digit and is named there)
        want = np.zeros(got.shape, np.int64)
        want[i % Co, :] = 1
        bad = np.argwhere(digit != want)
        if bad.size:
            co, k = bad[0]
            out.append("planted row %d (number %d, 4^%d on dW row %d) counted %d times at dW[%d,%d]; %d elements wrong, columns k %d..%d"
                       % (r, i, i, i % Co, int(digit[co, k]), co, k, len(bad), bad[:, 1].min(), bad[:, 1].max()))
    return out


def decode_outer(got):
    """got (Co,K) from an outer_index input -> complaints naming the element, and whose value it holds instead."""
    got = np.asarray(got, np.float64)
    Co, K = got.shape
    want = np.outer(np.arange(1, Co + 1), np.arange(1, K + 1)).astype(np.float64)
    bad = np.argwhere(got != want)
    out = []
    for co, k in bad[:4]:
        src = np.argwhere(want == got[co, k])
        out.append("dW[%d,%d] = %r, expected %d%s" % (co, k, float(got[co, k]), int(want[co, k]),
                                                      "" if not src.size else " (the value of dW[%d,%d])" % tuple(src[0])))
    if len(bad):
        out.insert(0, "%d elements wrong, rows co %d..%d, columns k %d..%d" % (len(bad), bad[:, 0].min(), bad[:, 0].max(), bad[:, 1].min(),
                                                                                bad[:, 1].max()))
    return out


def explain(name, got, want, R, Co, K):
    """failure message of an exact-family comparison (got, want: (Co,K) arrays; want already holds any pre-filled pattern)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    bad = np.argwhere(got != want)
    head = "%s R=%d Co=%d K=%d: %d elements differ, first dW[%d,%d] = %r, expected %r" % (
        name, R, Co, K, len(bad), bad[0][0], bad[0][1], float(got[tuple(bad[0])]), float(want[tuple(bad[0])]))
    base = want - exact_product(*exact_family(name, R, Co, K))        # the pattern `out=` was pre-filled with (0 otherwise)
    if name == "rows_bitmask":
        return head + "; " + "; ".join(decode_bitmask(got - base, planted_rows(R, Co, K), Co))
    if name == "outer_index":
        return head + "; " + "; ".join(decode_outer(got - base))
    return head


# ------------------------------------------------------------------------------------------------------------------ float families
def float_family(name, R, Co, K, seed=0):
    g = np.random.default_rng([seed, R, Co, K, 2 + FLOAT_FAMILIES.index(name)])
    gy, x = g.standard_normal((R, Co)), g.standard_normal((R, K))
    if name == "decades":           # rows spread over seven decades
        gy = gy * (10.0 ** ((np.arange(R) % 7) - 3.0))[:, None]
    elif name == "cancel":          # second half = the negated first half, x perturbed by 1e-3: sums fall far below their terms
        h = R // 2
        o = R - 2 * h               # (odd R: row 0 has no partner; it must not dominate the sums)
        gy[o + h:] = -gy[o:o + h]
        x[o + h:] = x[o:o + h] + 1e-3 * g.standard_normal((h, K))
        gy[:o] *= 1e-3
    elif name == "sparse":          # 2 % non-zeros in gy: the shape of the dist term's W
        gy = gy * (g.random((R, Co)) < 0.02)
        gy[R - 1, Co - 1] = 1.5     # never vacuous at the smallest sizes
    return gy.astype(np.float32), x.astype(np.float32)


def ref64(gy, x):
    return gy.astype(np.float64).T @ x.astype(np.float64)


def bound(gy, x):
    return gy.shape[0] * U * magnitude(gy, x)


def worst_ratio(got, gy, x):
    """-> (largest err / bound over the elements with bound > 0, number of elements with bound == 0 that are not exactly 0)"""
    err, b = np.abs(np.asarray(got, np.float64) - ref64(gy, x)), bound(gy, x)
    assert np.isfinite(np.asarray(got)).all()
    pos = b > 0
    return (float((err[pos] / b[pos]).max()) if pos.any() else 0.0), int(np.count_nonzero(np.asarray(got)[~pos]))


def chain32(gy, x):
    """the row-ordered float32 chain acc += gy[r]^T x[r] (one rounded product, one rounded add per step)"""
    acc = np.zeros((gy.shape[1], x.shape[1]), np.float32)
    for r in range(gy.shape[0]):
        acc = acc + np.outer(gy[r], x[r])
    assert acc.dtype == np.float32
    return acc
