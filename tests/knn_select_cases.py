"""Planted rows for the feature-space kNN (csrc/dvm_knn.hip, K3): exact scores, the expected list by construction, and numpy
models of the branch each selection kernel takes on a row.

Planting.  A row is given by integer ranks r_j >= 0 (and, for the k > 64 families, a count t_j of unit entries).  The query is
a = u with u in {+-1}^C, key j is  b_j = u +- r_j e_{c_j} +- (t_j unit entries in t_j other channels),  with the channel c_j,
every sign and u drawn per batch entry.  Every feature, every partial sum of |b_j|^2 and of a.b_j and every step of
s = (-|a|^2 - (-2 a.b_j)) - |b_j|^2 is an integer below 2^24 (asserted in plant()), so s_j = -(r_j^2 + t_j) exactly in any
summation order, on the matrix cores as in the oracle's fma chain.  The expected list is argsort(r^2 + t, stable)[:k]: best score
first, ties in column order.  It depends neither on the oracle nor on the kernel.

Branch models.  wave_branch() and select_branch() replay, on the exact scores, the decisions topk_wave_kernel<32> /
topk_wave_stream_kernel (k <= 64) and topk_select_kernel<EPT> (k > 64) take from the data of a row.  The families below are
named after the branch they are built to reach; tests/test_knn_select_cases_cpu.py checks every claim with the models, and
that the case table covers every (kernel, branch) pair."""
import functools

import numpy as np

LIMIT = 1 << 24
RMAX = 4000          # largest rank used: (RMAX + 1)^2 + 4 * 126 + 128 < 2^24
FAR = 600            # far keys: ranks in [FAR, RMAX], drawn with repeats; every named rank of a family stays below FAR
LANES = 64
SEED = 9100
PAD = np.uint32(0xffffffff)

WAVE_KS = (1, 2, 40, 63, 64)
BLOCK_KS = (65, 128, 129, 500, 512)
WAVE_MS = (40, 64, 65, 200, 2047, 2048)
STREAM_MS = (2049, 4995, 8192)


# ------------------------------------------------------------------------------------------------------------ launch rules
def kernel_of(M, k):
    """the selection kernel launch_knn_neg picks"""
    if k <= 64:
        return "wave" if M <= 2048 else "stream"
    return "select%d" % ept_of(M)


def ept_of(M):
    ept = (M + 255) // 256
    return 8 if ept <= 8 else 16 if ept <= 16 else 32


def score_route(C):
    return {128: "dma", 64: "mfma"}.get(C, "scalar")


def key_chunk(B, N, M):
    """(kchunk, nz) of the score kernels' grid.z key split: the arithmetic of launch_knn_neg"""
    qtiles, ktiles = (N + 127) // 128, (M + 63) // 64
    nz = 1
    while B * qtiles * nz < 1024 and nz * 2 <= ktiles:
        nz *= 2
    kchunk = ((ktiles + nz - 1) // nz) * 64
    return kchunk, (M + kchunk - 1) // kchunk


# ----------------------------------------------------------------------------------------------------------------- planting
def plant(rng, C, r, t=None):
    """-> (u (C,) float32, b (M, C) float32) with score(u, b_j) = -(r_j^2 + t_j) exactly; raises if a bound is missed"""
    r = np.asarray(r, np.int64)
    M = len(r)
    t = np.zeros(M, np.int64) if t is None else np.asarray(t, np.int64)
    assert r.min() >= 0 and r.max() <= RMAX and t.min() >= 0 and t.max() <= C - 2
    u = rng.choice([-1, 1], C).astype(np.int64)
    b = np.tile(u, (M, 1))
    c = rng.integers(0, C, M)
    b[np.arange(M), c] += rng.choice([-1, 1], M) * r
    if t.any():
        draw = rng.random((M, C))
        draw[np.arange(M), c] = 2.0                                   # never the rank's own channel
        unit = np.argsort(np.argsort(draw, 1), 1) < t[:, None]        # t_j channels of row j
        b += unit * rng.choice([-1, 1], (M, C))
    # what the device and the oracle form, in integers: both norms, every partial sum of the dot chain in any order, the steps of s
    na, nb, dot = C, (b * b).sum(1), b @ u
    assert max(nb.max(), np.abs(b).sum(1).max(), np.abs(2 * dot).max(), np.abs(2 * dot - na).max()) < LIMIT
    assert np.array_equal(na + nb - 2 * dot, r * r + t)
    return u.astype(np.float32), b.astype(np.float32)


def scores(r, t=None):
    """the exact float32 score row"""
    r = np.asarray(r, np.int64)
    d = r * r + (0 if t is None else np.asarray(t, np.int64))
    assert d.max() < LIMIT
    return np.float32(0) - d.astype(np.float32)                        # (rank 0 scores +0, as the kernel's C - C)


def expected(r, t, k):
    r = np.asarray(r, np.int64)
    d = r * r + (0 if t is None else np.asarray(t, np.int64))
    return np.argsort(d, kind="stable")[:k].astype(np.int32)


# ------------------------------------------------------------------------------------------------------------ branch models
def desc_key(s):
    """desc_key of dvm_knn.hip: float bits -> uint32, ascending key == descending score"""
    u = np.ascontiguousarray(s, np.float32).view(np.uint32)
    u = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))
    return ~u


def wave_branch(s, k):
    """topk_wave_kernel<32> / topk_wave_stream_kernel on the score row s -> dict
         C          keys <= Tc, Tc the k-th smallest of the 128 lane minima (two smallest keys of columns = lane mod 64)
         exact      Tc is the row's true k-th key
         tail       "one-slot" (C <= 64) | "two-slot" (C <= 128) | "exact-search" (wave_select_ties; the stream kernel has by then
                    dropped the candidates at positions >= 128 and starts over)
         max_lane   the most winners one lane holds
         tied       keys equal to the true k-th key"""
    key = desc_key(s)
    M = len(key)
    E = -(-M // LANES)
    pad = np.full(E * LANES, PAD, np.uint32)
    pad[:M] = key
    g = np.sort(pad.reshape(E, LANES), 0)
    minima = np.concatenate([g[0], g[1] if E > 1 else np.full(LANES, PAD, np.uint32)])
    Tc = np.sort(minima)[k - 1]
    kth = np.sort(key)[k - 1]
    C = int((key <= Tc).sum())
    win = np.argsort(key, kind="stable")[:k]
    return dict(C=C, exact=bool(Tc == kth), tail="one-slot" if C <= 64 else "two-slot" if C <= 128 else "exact-search",
                max_lane=int(np.bincount(win % LANES, minlength=LANES).max()), tied=int((key == kth).sum()))


def select_branch(s, k):
    """topk_select_kernel<EPT> on the score row s -> dict
         multi_bin_passes   radix passes (of 4) in which the keys still matching the prefix occupy more than one bin
         tied, remaining    keys equal to the k-th key, and how many of them the list takes
         cut                "none" (all of them taken) | "inside" (the last tie taken and the first one left sit in one thread's
                            EPT consecutive columns) | "between" (in two threads)
         kp2                the padded length of the sort"""
    key = desc_key(s)
    ept = ept_of(len(key))
    prefix, mask, remaining, multi = 0, 0, k, 0
    for shift in (24, 16, 8, 0):
        live = key[(key & np.uint32(mask)) == np.uint32(prefix)]
        hist = np.bincount((live >> np.uint32(shift)) & np.uint32(255), minlength=256)
        multi += int((hist > 0).sum() > 1)
        cum = np.cumsum(hist)
        b = int(np.searchsorted(cum, remaining))                      # the one bin with excl < remaining <= excl + count
        prefix |= b << shift
        mask |= 255 << shift
        remaining -= int(cum[b] - hist[b])
    assert prefix == int(np.sort(key)[k - 1])
    eq = np.flatnonzero(key == np.uint32(prefix))
    cut = "none" if len(eq) == remaining else "inside" if eq[remaining - 1] // ept == eq[remaining] // ept else "between"
    kp2 = 1
    while kp2 < k:
        kp2 *= 2
    return dict(multi_bin_passes=multi, tied=len(eq), remaining=remaining, cut=cut, kp2=kp2)


# --------------------------------------------------------------------------------------------------------- families, k <= 64
def _far(rng, M):
    return rng.integers(FAR, RMAX + 1, M)


def _slots(lane, M):
    return (M - lane + LANES - 1) // LANES


def _one_per_lane(rng, M, n, avoid=()):
    """n columns in n different lanes (not in `avoid`), a random slot each"""
    lanes = np.setdiff1d(np.arange(min(M, LANES)), avoid)
    assert n <= len(lanes)
    lanes = rng.permutation(lanes)[:n]
    return np.array([rng.integers(_slots(l, M)) * LANES + l for l in lanes], np.int64)


def spread(rng, M, k):
    """one winner per lane: Tc exact, C = k"""
    r = _far(rng, M)
    r[_one_per_lane(rng, M, k)] = rng.permutation(k)
    return r


def pairs(rng, M, k):
    """two winners per lane (the lane's two minima): Tc exact, C = k"""
    two = [l for l in range(min(M, LANES)) if _slots(l, M) >= 2]
    assert k >= 2 and (k + 1) // 2 <= len(two)
    cols = []
    for l in rng.permutation(two)[:(k + 1) // 2]:
        cols += [s * LANES + l for s in rng.permutation(_slots(l, M))[:2]]
    r = _far(rng, M)
    r[np.array(cols[:k])] = rng.permutation(k)
    return r


def triple(rng, M, k, extra):
    """One lane holds three winners and, behind them, `extra` keys of the next ranks; the next rank after those sits in another
    lane.  The lane minima miss the lane's third winner: Tc is that last key, loose, and C = k + extra + 1.  The best key is the
    candidate in the highest column: the one a compaction in column order reaches last (the stream kernel keeps 128)."""
    deep = [l for l in range(min(M, LANES)) if _slots(l, M) >= 3 + extra]
    assert k >= 3 and deep
    L = int(rng.choice(deep))
    own = np.sort(rng.permutation(_slots(L, M))[:3 + extra])[::-1] * LANES + L       # the lane's highest slot taken is a winner
    cols = np.concatenate([own[:3], _one_per_lane(rng, M, k - 3, avoid=[L])])
    r = _far(rng, M)
    r[cols] = rng.permutation(k)
    r[own[3:]] = k + rng.permutation(extra)
    hi = cols.max()
    r[cols[r[cols] == 0]], r[hi] = r[hi], 0
    free = np.flatnonzero((r >= FAR) & (np.arange(M) % LANES != L) & (np.arange(M) < hi))
    r[rng.choice(free)] = k + extra
    return r


def stacked(rng, M, k):
    """All k winners in one lane (in as few lanes as hold them when k exceeds the lane's slots), and behind them 129 - k or more
    keys of the next ranks filling whole lanes: the minima see two keys of each such lane, Tc lands among the far keys, C > 128
    with no tie anywhere near the threshold: the exact search with a single key at T."""
    lanes = sorted(rng.permutation(min(M, LANES)), key=lambda l: -_slots(l, M))       # full lanes first, random among equals
    r = _far(rng, M)
    left, dense, li = k, 0, 0
    win = []
    while left:
        l = lanes[li]
        li += 1
        take = rng.permutation(_slots(l, M))[:left] * LANES + l
        win += list(take)
        left -= len(take)
    r[np.array(win)] = rng.permutation(k)
    fill = []
    while len(fill) < 129 - k:
        l = lanes[li]
        li += 1
        fill += [s * LANES + l for s in range(_slots(l, M))]
    assert 2 * li < k, "the k-th lane minimum has to be a far key"
    r[np.array(fill)] = k + rng.permutation(len(fill))
    assert k + len(fill) < FAR
    return r


def tie_edge(rng, M, k, t):
    """k - 1 distinct winners, one per lane, and t keys tied at the next rank: Tc is exact and C = k - 1 + t.  The tied keys are
    scattered over all slots, the lowest and the highest free column among them (below some winner, and in the last slot)."""
    r = _far(rng, M)
    r[_one_per_lane(rng, M, k - 1)] = rng.permutation(k - 1)
    free = np.flatnonzero(r >= FAR)
    assert t <= len(free)
    tied = rng.permutation(free[1:-1])[:max(t - 2, 0)]
    tied = np.concatenate([tied, free[[0, -1]]]) if t >= 2 else rng.permutation(free)[:t]
    r[tied] = k - 1
    return r


def all_equal(rng, M, k):
    """every key the same score: columns 0 .. k - 1"""
    return np.full(M, 3, np.int64)


def ends(rng, M, k):
    """the best key in the last column, the next in the columns before it, the k-th in column 0"""
    r = _far(rng, M)
    r[M - 1 - np.arange(k - 1)] = np.arange(k - 1)
    r[M - 1 if k == 1 else 0] = k - 1
    return r


def chunk_edge_columns(B, N, M):
    """the last and the first column of neighbouring grid.z key chunks, and the first and last column of the last key tile"""
    kchunk, nz = key_chunk(B, N, M)
    e = {q * kchunk - 1 for q in range(1, nz)} | {q * kchunk for q in range(1, nz)} | {64 * ((M - 1) // 64), M - 1}
    return np.array(sorted(e), np.int64)


def chunk_edges(rng, M, k, B, N):
    """the best keys on the chunk edges (all of them, or the best k when there are more edges than that), other winners anywhere"""
    e = chunk_edge_columns(B, N, M)
    r = _far(rng, M)
    r[e] = rng.permutation(len(e))
    if len(e) < k:
        r[rng.permutation(np.flatnonzero(r >= FAR))[:k - len(e)]] = len(e) + rng.permutation(k - len(e))
    assert len(e) < FAR
    return r


# ---------------------------------------------------------------------------------------------------------- families, k > 64
LOW_P = 2897         # 2897^2 = 2^23 + 4001: d = p^2 + t, t <= 94, shares the three top bytes of its float (and of its key)


def low_byte(rng, M, k, C, others=True):
    """-> (r, t).  The bulk of the row scores -(2897^2 + t), t = 0 .. T - 1, every value repeated: one key bin in the three upper
    radix passes, T bins in the last one, the k-th key tied.  With `others`: five nearer keys (another top byte), six keys of
    rank 4000 (another second byte) and six of rank 2898 (another third byte), so that every pass has to pick among occupied
    bins; the k-th key is still one of the bulk."""
    T = min(C - 1, 95)
    r, t = np.full(M, LOW_P, np.int64), np.zeros(M, np.int64)
    cols = rng.permutation(M)
    n = 17 if others else 0
    if others:
        assert M >= k + 12 and k > 5
        r[cols[:5]], r[cols[5:11]], r[cols[11:17]] = np.arange(5), 4000, 2898
    t[cols[n:]] = rng.permutation(M - n) % T
    return r, t


def tie_cut(rng, M, k, where):
    """-> (r, None).  k - 7 distinct winners, then 13 keys tied at the threshold rank of which the list takes 7: the seventh and
    the eighth are neighbouring columns, `where` = "inside" one thread's run of EPT columns or "between" two threads."""
    ept = ept_of(M)
    j1 = (M // ept // 2) * ept + (ept // 2 - 1 if where == "inside" else ept - 1)
    assert k > 7 and j1 + 1 < M and j1 >= 6 and M - j1 - 2 >= 5 and M >= k + 6
    tied = np.concatenate([rng.permutation(j1)[:6], [j1, j1 + 1], j1 + 2 + rng.permutation(M - j1 - 2)[:5]])
    r = _far(rng, M)
    r[tied] = k - 7
    r[rng.permutation(np.flatnonzero(r >= FAR))[:k - 7]] = rng.permutation(k - 7)
    assert k - 7 < FAR
    return r, None


WAVE_FAMILIES = dict(spread=spread, pairs=pairs, triple=triple, stacked=stacked, tie_edge=tie_edge, all_equal=all_equal, ends=ends,
                     chunk_edges=chunk_edges)
BLOCK_FAMILIES = dict(low_byte=low_byte, tie_cut=tie_cut, all_equal=all_equal, ends=ends)


# -------------------------------------------------------------------------------------------------------------- case table
# (family, M, k, family argument or None).  Which branch each row reaches is asserted in tests/test_knn_select_cases_cpu.py.
WAVE_TABLE = [
    ("spread", 40, 40, None), ("spread", 64, 64, None), ("spread", 64, 1, None), ("spread", 65, 1, None), ("spread", 200, 40, None),
    ("spread", 2047, 63, None), ("spread", 2048, 64, None), ("spread", 2049, 2, None), ("spread", 4995, 40, None),
    ("spread", 8192, 64, None),
    ("pairs", 65, 2, None), ("pairs", 200, 40, None), ("pairs", 2047, 63, None), ("pairs", 2048, 64, None), ("pairs", 2049, 40, None),
    ("pairs", 4995, 64, None), ("pairs", 8192, 2, None),
    ("triple", 200, 40, 1), ("triple", 2048, 40, 5), ("triple", 2048, 63, 5), ("triple", 2047, 64, 0), ("triple", 2049, 40, 30),
    ("triple", 4995, 63, 0), ("triple", 4995, 64, 3), ("triple", 8192, 40, 90),
    ("stacked", 2048, 40, None), ("stacked", 2047, 63, None), ("stacked", 2048, 64, None), ("stacked", 2049, 63, None),
    ("stacked", 4995, 40, None), ("stacked", 4995, 64, None), ("stacked", 8192, 64, None),
    ("tie_edge", 200, 40, 25), ("tie_edge", 200, 40, 26), ("tie_edge", 200, 40, 89), ("tie_edge", 200, 40, 90),
    ("tie_edge", 2048, 64, 1), ("tie_edge", 2048, 64, 2), ("tie_edge", 2048, 64, 65), ("tie_edge", 2048, 64, 66),
    ("tie_edge", 2047, 1, 64), ("tie_edge", 2047, 1, 129), ("tie_edge", 2048, 63, 2), ("tie_edge", 2048, 2, 127),
    ("tie_edge", 4995, 40, 25), ("tie_edge", 4995, 40, 26), ("tie_edge", 4995, 40, 89), ("tie_edge", 4995, 40, 90),
    ("tie_edge", 2049, 64, 66), ("tie_edge", 2049, 2, 63), ("tie_edge", 8192, 1, 128), ("tie_edge", 8192, 63, 3),
    ("all_equal", 40, 40, None), ("all_equal", 64, 64, None), ("all_equal", 64, 1, None), ("all_equal", 65, 64, None),
    ("all_equal", 200, 40, None), ("all_equal", 2047, 2, None), ("all_equal", 2048, 63, None), ("all_equal", 2049, 1, None),
    ("all_equal", 4995, 40, None), ("all_equal", 8192, 64, None),
    ("ends", 40, 40, None), ("ends", 64, 64, None), ("ends", 65, 64, None), ("ends", 200, 40, None), ("ends", 2047, 63, None),
    ("ends", 2048, 1, None), ("ends", 2048, 64, None), ("ends", 2049, 64, None), ("ends", 4995, 40, None), ("ends", 8192, 2, None),
    ("chunk_edges", 65, 2, None), ("chunk_edges", 200, 40, None), ("chunk_edges", 2047, 64, None), ("chunk_edges", 2048, 40, None),
    ("chunk_edges", 2049, 40, None), ("chunk_edges", 4995, 63, None), ("chunk_edges", 8192, 64, None),
]
BLOCK_TABLE = [
    ("low_byte", 129, 129, False), ("low_byte", 300, 65, True), ("low_byte", 2048, 512, True), ("low_byte", 2049, 129, True),
    ("low_byte", 4096, 500, True), ("low_byte", 4097, 128, True), ("low_byte", 8192, 512, True),
    ("tie_cut", 300, 128, "inside"), ("tie_cut", 300, 129, "between"), ("tie_cut", 2048, 500, "inside"),
    ("tie_cut", 2048, 65, "between"), ("tie_cut", 2049, 65, "inside"), ("tie_cut", 4096, 512, "between"),
    ("tie_cut", 4096, 128, "inside"), ("tie_cut", 4097, 129, "between"), ("tie_cut", 8192, 500, "inside"),
    ("tie_cut", 8192, 65, "between"),
    ("all_equal", 65, 65, None), ("all_equal", 512, 512, None), ("all_equal", 300, 129, None), ("all_equal", 2048, 128, None),
    ("all_equal", 2049, 500, None), ("all_equal", 4096, 65, None), ("all_equal", 4097, 512, None), ("all_equal", 8192, 129, None),
    ("ends", 128, 128, None), ("ends", 500, 500, None), ("ends", 300, 65, None), ("ends", 2048, 512, None), ("ends", 2049, 128, None),
    ("ends", 4096, 129, None), ("ends", 4097, 500, None), ("ends", 8192, 65, None),
]
# both sides of the stream kernel's 128 kept candidates and of the one-slot sort's 64, under a loose threshold (no tie to absorb a
# dropped candidate)
EXTRA_TABLE = [("triple", 8192, 40, 87), ("triple", 8192, 40, 88), ("triple", 2048, 63, 0), ("triple", 4995, 64, 0)]
# (C, N, B) of the call, rotated over the table: every score route, N = 1 / 5 / 130 (rows per workgroup not a multiple of 4, a ragged
# query tile), 1 to 3 batch entries with a planting each
CALLS = [(64, 1, 3), (128, 5, 2), (36, 130, 1), (64, 130, 2), (128, 1, 3), (36, 5, 3), (128, 130, 1), (64, 5, 2), (36, 1, 2)]
TABLE = [row + CALLS[i % len(CALLS)] for i, row in enumerate(WAVE_TABLE + BLOCK_TABLE + EXTRA_TABLE)]


def case_id(i):
    fam, M, k, arg, C, N, B = TABLE[i]
    return "%s%s-M%d-k%d-C%d-N%d-B%d" % (fam, "" if arg is None else "[%s]" % arg, M, k, C, N, B)


def family_ranks(rng, fam, M, k, arg, C, N, B):
    """-> (r, t) of one batch entry"""
    if k > 64:
        if fam == "low_byte":
            return low_byte(rng, M, k, C, arg)
        if fam == "tie_cut":
            return tie_cut(rng, M, k, arg)
        return BLOCK_FAMILIES[fam](rng, M, k), None
    if fam == "chunk_edges":
        return chunk_edges(rng, M, k, B, N), None
    if fam in ("triple", "tie_edge"):
        return WAVE_FAMILIES[fam](rng, M, k, arg), None
    return WAVE_FAMILIES[fam](rng, M, k), None


def build_call(rows, C, N, seed):
    """rows: one (r, t) per batch entry -> (a (B,N,C), b (B,M,C)) float32, a planting of its own per entry"""
    a, b = [], []
    for i, (r, t) in enumerate(rows):
        u, keys = plant(np.random.default_rng([SEED, seed, i, 1]), C, r, t)
        a.append(np.tile(u, (N, 1)))
        b.append(keys)
    return np.stack(a), np.stack(b)


@functools.lru_cache(maxsize=4)
def table_case(i):
    """-> dict(a (B,N,C) f32, b (B,M,C) f32, want (B,N,k) int32, rows [(r, t)] per batch entry, ...).  Shared, never modified."""
    fam, M, k, arg, C, N, B = TABLE[i]
    rows = [family_ranks(np.random.default_rng([SEED, i, e]), fam, M, k, arg, C, N, B) for e in range(B)]
    a, b = build_call(rows, C, N, i)
    want = np.stack([np.tile(expected(r, t, k), (N, 1)) for r, t in rows])
    return dict(family=fam, M=M, k=k, arg=arg, C=C, N=N, B=B, rows=rows, a=a, b=b, want=want, kernel=kernel_of(M, k))


# ---------------------------------------------------------------------------------------------- one workgroup, four tails
def mixed_rows(M, k):
    """Seven one-row batch entries of one call (N = 1: rows 0-3 share a workgroup, rows 4-6 the next one), consecutive rows on
    different tails -> [(name, (r, t))]"""
    assert k == 40 and M >= 200
    plan = [("one-slot", tie_edge, 25), ("two-slot", tie_edge, 89), ("exact-search", stacked if M >= 2047 else tie_edge, 90),
            ("all_equal", all_equal, None), ("exact-search", tie_edge, 90), ("two-slot", tie_edge, 26), ("one-slot", spread, None)]
    out = []
    for i, (name, fam, arg) in enumerate(plan):
        rng = np.random.default_rng([SEED, 77, M, i])
        args = (rng, M, k) if arg is None or fam is stacked else (rng, M, k, arg)
        out.append((name, (fam(*args), None)))
    return out
