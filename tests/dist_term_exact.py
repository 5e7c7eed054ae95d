"""Planted inputs on which the dist-loss term (csrc/dvm_dist_loss.hip, K10) is exact per anchor, and its rational reference.

ops.dist_loss returns, per batch element, the sum over the anchors of 1 - |cos(x, y)| with x_j = |feat[idx_j] - feat[a]| and
y_j = dist[idx_j, a] over the anchor's k nearest rows in feature space.  On the planting below the kNN's scores, every x_j and the
three sums  sxy = sum x y, sxx = sum x^2, syy = sum y^2  are integers below 2^24: neither the summation order, the lane layout nor FMA
contraction can move a bit of them, and what is left of the kernel — sqrt_rn, one product, one quotient, all correctly rounded — is
evaluated here in numpy float32.  A dropped, doubled or mispaired neighbour slot, a y read transposed, a term credited to the wrong
workgroup slot then moves the float32 output (tests/test_dist_term_exact_cpu.py proves that for every slot of every case).

Planting of one batch element (numpy only, every draw seeded):
  cloud     nA clusters, one per anchor, of S >= k rows each, scattered over the N = nA * S row numbers by a permutation; the anchors'
            row numbers are shared by the batch (ops.dist_loss takes one anchor list) and listed in shuffled order.
  anchor    integers in [-3, 3] in every channel (a walk that forgets to subtract the anchor row is wrong in every lane), plus the
            cluster's marker 256 in channel g mod C and, when nA > C, a second one in channel (g mod C + 1 + g div C) mod C: two
            clusters differ by 256 in at least two channels, every cross-cluster distance exceeds every in-cluster one.
  rows      anchor row + an offset of squared norm m^2, m an integer in [1, 40]: +-m in one channel, +-m/2 in four channels of four
            different lanes of the C = 128 walk, +-m/4 in sixteen, +-m/8 in sixty-four (the shapes that fit C).  The shape and its
            first channel rotate with the row's rank in its cluster, so the selected rows of one anchor carry a non-zero difference in
            every channel (asserted for k >= 63).  x = m exactly.  Ranks are by (m, row number): the device's tie rule.
  dist      dist[v, a] = y_v, an integer in [1, 100] drawn independently of m (consecutive ranks never share a y), dist[a, a]
            included; every other entry is 101 + (31 i + 17 j) mod 97: not symmetric, never a planted value.
  kinds     per anchor: "plain"; "dup" (every row of the cluster equals the anchor row: x = 0, term exactly 1); "yzero" (y = 0, term
            exactly 1); "yneg" (y < 0: |cos| is taken); "tie" (ranks k - 1 and k share m and differ in y: the lower row number wins).
"""
import functools

import numpy as np

from exact_inputs import f32, ulp_distance   # noqa: F401  (re-exported for the tests)

STEP = 8                 # features are multiples of 1 / STEP; scores are counted in units of 1 / STEP^2
MARK = 256
M_MAX, Y_MAX = 40, 100
LIMIT = 1 << 24
TERM_GRID = float(1 << 32)   # every term is a multiple of 2^-32 (asserted): sums of up to 2^20 of them are exact in float64
SEED = 7300


# ------------------------------------------------------------------------------------------------------------------ planting
def _channels(C, n, base):
    stride = C // n
    if n == 1:
        return [base % C]
    if n == 4:
        return [(base + q * stride + q) % C for q in range(4)]
    if n == 16:
        return [(base + q * stride + q // 4) % C for q in range(16)]
    return [(base + q * stride + (q // 32 if stride > 1 else 0)) % C for q in range(64)]


def offset_shapes(C):
    """channel counts n of the offset shapes that fit C: n distinct channels of magnitude m / sqrt(n)"""
    return [n for n in (1, 4, 16, 64) if n <= C and len(set(_channels(C, n, 0))) == n]


def offset_channels(C, n, base):
    """the n distinct channels of a shape: spread over the row with stride C // n, the component within a 4-channel group advancing
    every fourth (n = 4: every) step"""
    ch = _channels(C, n, base)
    assert len(set(ch)) == n, (C, n, base)
    return np.array(ch)


def _plant_element(rng, C, k, nA, S, anchors, kinds):
    N = nA * S
    shapes = offset_shapes(C)
    rest = rng.permutation(np.setdiff1d(np.arange(N), anchors)).reshape(nA, S - 1) if S > 1 else np.empty((nA, 0), np.int64)
    feat = np.zeros((N, C), np.float64)
    ii, jj = np.arange(N, dtype=np.int64)[:, None], np.arange(N, dtype=np.int64)[None]
    dist = (101 + (31 * ii + 17 * jj) % 97).astype(np.float64)
    rows, xs, ys, yt = (np.zeros((nA, S), np.int64) for _ in range(4))
    gsq = np.zeros((nA, S, C // 4), np.int64)                      # squared offset per 4-channel group, in units of 1 / STEP^2
    for g in range(nA):
        kind = kinds[g]
        a = int(anchors[g])
        base = rng.integers(-3, 4, C).astype(np.float64)
        base[g % C] += MARK
        if nA > C:
            base[(g % C + 1 + g // C) % C] += MARK
        member = np.concatenate([[a], rest[g]])
        m = np.concatenate([[0], rng.integers(1, M_MAX + 1, S - 1)])
        if kind == "dup":
            m[:] = 0
        if kind == "tie":
            assert 2 <= k < S
            ms = np.sort(m[1:])
            ms[k - 1] = ms[k - 2]
            m[1:] = rng.permutation(ms)
        order = np.lexsort((member, m))                            # rank: (m, row number); the anchor first unless it has duplicates
        member, m = member[order], m[order]
        y = np.empty(S, np.int64)
        y[0] = rng.integers(1, Y_MAX + 1)
        step = rng.integers(1, Y_MAX, S)
        for r in range(1, S):
            y[r] = (y[r - 1] - 1 + step[r]) % Y_MAX + 1            # never the previous rank's value
        if kind == "yzero":
            y[:] = 0
        if kind == "yneg":
            y = -y
        for r in range(S):
            row = base.copy()
            if m[r]:
                n = shapes[r % len(shapes)]
                ch = offset_channels(C, n, r // len(shapes) + 3 * g)
                mag = m[r] / np.sqrt(n)                            # m, m/2, m/4, m/8
                row[ch] += mag * rng.choice([-1.0, 1.0], n)
                np.add.at(gsq[g, r], ch // 4, int(mag * mag * STEP * STEP))
            feat[member[r]] = row
        dist[member, a] = y
        rows[g], xs[g], ys[g] = member, m, y
        yt[g] = dist[a, member]                                    # what a transposed read would take (dist[a, a] is its own transpose)
    return dict(feat=feat, dist=dist, rows=rows, xs=xs, ys=ys, yt=yt, gsq=gsq)


def _assert_exact(el, C, k, anchors):
    """what makes selection and sums exact in float32, in integers (float64 matrix products of integers far below 2^53)"""
    F = el["feat"] * STEP
    assert np.array_equal(F, np.rint(F)) and np.array_equal(el["feat"].astype(np.float32), el["feat"])
    A = F[anchors]
    nb, na = (F * F).sum(1), (A * A).sum(1)
    dot, mag = A @ F.T, np.abs(A) @ np.abs(F).T                    # a.b and the bound of every partial sum of its chain
    assert nb.max() < LIMIT and mag.max() < LIMIT and np.abs(2 * dot - na[:, None]).max() < LIMIT
    d2 = na[:, None] + nb[None] - 2 * dot
    nA, S = el["rows"].shape
    own = np.zeros(d2.shape, bool)
    own[np.arange(nA)[:, None], el["rows"]] = True
    assert np.array_equal(d2[own].reshape(nA, S), (el["xs"] ** 2)[np.arange(nA)[:, None], np.argsort(el["rows"], 1)] * STEP * STEP)
    if (~own).any():
        assert d2[~own].min() > d2[own].max()
    x, y = el["xs"][:, :k], el["ys"][:, :k]
    assert np.array_equal(el["gsq"].sum(-1), el["xs"] ** 2 * STEP * STEP)
    for s in ((x * y).sum(1), (x * x).sum(1), (y * y).sum(1)):
        assert np.abs(s).max() < LIMIT
    if k >= 63:   # every channel carries a non-zero difference for some selected row of every anchor with offsets
        diff = el["feat"][el["rows"][:, :k]] - el["feat"][anchors][:, None]
        live = el["xs"][:, 1:k].any(1)
        assert (diff != 0).any(1)[live].all()
    D = el["dist"]
    assert np.array_equal(D, np.rint(D)) and np.abs(D).max() < 256 and not np.array_equal(D, D.T)


def term_f32(sxy, sxx, syy):
    """The kernel's arithmetic from the three sums, vectorised: c = fl(sxy) / fl(max(fl(sqrt sxx), 1e-8f) * max(fl(sqrt syy), 1e-8f)) in
    float32 (numpy's float32 sqrt, product and quotient are correctly rounded, like the kernel's), the term 1 - |c| in float64."""
    sxy, sxx, syy = (np.atleast_1d(np.asarray(v, np.float64)).astype(np.float32) for v in (sxy, sxx, syy))
    floor = np.float32(1e-8)
    c = sxy / (np.maximum(np.sqrt(sxx), floor) * np.maximum(np.sqrt(syy), floor))
    assert c.dtype == np.float32
    return 1.0 - np.abs(c.astype(np.float64))


def term_f64(sxy, sxx, syy):
    """the same definition in float64 (the floor never binds on a non-degenerate anchor)"""
    sxy, sxx, syy = (np.atleast_1d(np.asarray(v, np.float64)) for v in (sxy, sxx, syy))
    return 1.0 - np.abs(sxy / (np.maximum(np.sqrt(sxx), 1e-8) * np.maximum(np.sqrt(syy), 1e-8)))


def sums(x, y):
    """(sxy, sxx, syy) over the last axis, integers"""
    x, y = np.asarray(x, np.int64), np.asarray(y, np.int64)
    return (x * y).sum(-1), (x * x).sum(-1), (y * y).sum(-1)


def exact_total(terms):
    """sum of terms that are multiples of 2^-32 below 2^20 altogether: integer arithmetic, exact"""
    t = np.asarray(terms, np.float64) * TERM_GRID
    assert np.array_equal(t, np.rint(t)) and t.size < (1 << 20)
    return int(np.rint(t).astype(np.int64).sum()) / TERM_GRID


@functools.lru_cache(maxsize=2)
def planted_case(C, k, nA, S, kinds=None, seed=SEED, B=2):
    """-> dict(feat (B,N,C) f32, dist (B,N,N) f32, anchors (nA,) int32, lists (B,nA,k) int32, terms (B,nA) float64, out (B,) float32,
    elements: per batch element the rank-ordered tables rows / xs / ys / yt (nA,S) and gsq (nA,S,C/4)).  Shared, never modified."""
    assert C % 4 == 0 and 1 <= k <= S and k <= 512
    kinds = tuple(kinds) if kinds else ("plain",) * nA
    assert len(kinds) == nA
    N = nA * S
    anchors = np.random.default_rng([seed, C, k, nA, S]).permutation(N)[:nA]
    els = [_plant_element(np.random.default_rng([seed, C, k, nA, S, b]), C, k, nA, S, anchors, kinds) for b in range(B)]
    terms = []
    for el in els:
        _assert_exact(el, C, k, anchors)
        t = term_f32(*sums(el["xs"][:, :k], el["ys"][:, :k]))
        c = 1.0 - t
        assert ((c == 0) | (c >= 2.0 ** -8)).all()                  # |c| has at most 32 fractional bits: TERM_GRID
        terms.append(t)
    d = dict(C=C, k=k, nA=nA, S=S, N=N, B=B, kinds=kinds, anchors=anchors.astype(np.int32), elements=els, terms=np.stack(terms),
             feat=np.stack([el["feat"] for el in els]).astype(np.float32), dist=np.stack([el["dist"] for el in els]).astype(np.float32),
             lists=np.stack([el["rows"][:, :k] for el in els]).astype(np.int32))
    d["out"] = np.array([f32(exact_total(t)) for t in terms], np.float32)
    return d


# --------------------------------------------------------------------------------------------------------------------- cases
# (C, k, nA, S, kinds); tests/test_gpu_dist_term_anchors.py says which part of the kernel each family reaches
SLOT_KS = (1, 2, 3, 31, 32, 33, 63, 64, 65, 127, 128, 129, 511, 512)
SLOT_CASES = [(128, k, 1, k + 8, None) for k in SLOT_KS]
FULL_CASES = [(128, k, 1, k, None) for k in (65, 129)]                                  # k = N: every row selected
WG_CASES = [(128, 33, nA, 41, None) for nA in (1, 2, 3, 4, 5, 7, 8, 9)] + [(128, 3, 1028, 4, None)]
GENERIC_CS = (8, 36, 64, 132)
GENERIC_CASES = [(C, k, 5, k + 8, None) for C in GENERIC_CS for k in (1, 63, 64, 65, 200, 512)]
DEGENERATE_KINDS = ("dup", "yzero", "yneg", "tie", "plain", "tie", "yneg")
DEGENERATE_CASES = [(128, 33, 7, 41, DEGENERATE_KINDS), (128, 130, 7, 138, DEGENERATE_KINDS), (36, 65, 7, 73, DEGENERATE_KINDS)]
ALL_CASES = SLOT_CASES + FULL_CASES + WG_CASES + GENERIC_CASES + DEGENERATE_CASES


def case_id(c):
    C, k, nA, S, kinds = c
    return "C%d-k%d-nA%d-S%d%s" % (C, k, nA, S, "-kinds" if kinds else "")


# ----------------------------------------------------------------------------------------------------------------- mutations
MUTATIONS = ("drop", "y_next", "y_prev", "twice", "group", "transposed")
# Slot / mutation pairs that CANNOT move the output — arithmetic, not luck:
#   k = 1                       x_0 = 0 (the anchor itself): sxy = 0 and the term is 1 whatever the slot holds;
#   kinds "dup" and "yzero"     sxy = 0 by construction: the term is 1 whatever slot moves;
#   k = 2, "group" on slot 1    with x_0 = 0 the cosine is y_1 / sqrt(y_0^2 + y_1^2) for ANY x_1 > 0 (x_1 -> 0 is not exempt);
#   "group" on a slot with x = 0     the anchor's own slot has no non-zero group to leave out;
#   "transposed" on slot 0      dist[a, a] is its own transpose;
#   "y_next" / "twice" on slot k - 1 when k = S, "y_prev" on slot 0: there is no such slot.


def mutation_escapes(case):
    """For every (anchor, slot j < k, mutation): does the float32 output of EVERY batch element stay put?  -> list of escapes
    (anchor, slot, mutation), exemptions (see above) left out.  "group" counts as noticed in a batch element only if leaving out
    each of the slot's non-zero 4-channel groups, one at a time, moves the output."""
    k, nA, S, B = case["k"], case["nA"], case["S"], case["B"]
    if k == 1:
        return []
    j = np.arange(k)
    noticed = {m: np.zeros((nA, k), bool) for m in MUTATIONS}
    applies = {m: np.ones((nA, k), bool) for m in MUTATIONS}
    for b, el in enumerate(case["elements"]):
        total = exact_total(case["terms"][b])
        for n in range(nA):
            if case["kinds"][n] in ("dup", "yzero"):
                for m in MUTATIONS:
                    applies[m][n] = False
                continue
            x, y, yt = (el[t][n].astype(np.float64) for t in ("xs", "ys", "yt"))
            xk, yk = x[:k], y[:k]
            sxy, sxx, syy = (float(s) for s in sums(xk, yk))
            rest = total - case["terms"][b, n]

            def moved(nxy, nxx, nyy):
                return (rest + term_f32(nxy, nxx, nyy)).astype(np.float32) != case["out"][b]

            def swap(x2, y2):   # slot j holds (x2, y2) instead of (x_j, y_j)
                return moved(sxy - xk * yk + x2 * y2, sxx - xk * xk + x2 * x2, syy - yk * yk + y2 * y2)

            noticed["drop"][n] |= moved(sxy - xk * yk, sxx - xk * xk, syy - yk * yk)
            nxt = j + 1 < S
            jn = np.minimum(j + 1, S - 1)
            applies["y_next"][n] &= nxt
            applies["twice"][n] &= nxt
            noticed["y_next"][n] |= swap(xk, y[jn]) & nxt
            noticed["twice"][n] |= swap(x[jn], y[jn]) & nxt
            applies["y_prev"][n] &= j >= 1
            noticed["y_prev"][n] |= swap(xk, y[np.maximum(j - 1, 0)]) & (j >= 1)
            applies["transposed"][n] &= j >= 1
            noticed["transposed"][n] |= swap(xk, yt[:k]) & (j >= 1)
            q = el["gsq"][n, :k].astype(np.float64) / (STEP * STEP)            # (k, C/4)
            x2 = np.sqrt(np.maximum(xk[:, None] ** 2 - q, 0.0))                  # x_j without the group
            mv = moved(sxy + (x2 - xk[:, None]) * yk[:, None], sxx - q, syy)
            live = q > 0
            if k == 2:
                live &= ~((j[:, None] == 1) & (x2 > 0))
            applies["group"][n] &= live.any(1)
            noticed["group"][n] |= (mv | ~live).all(1) & live.any(1)
    return [(n, s, m) for m in MUTATIONS for n, s in zip(*np.nonzero(applies[m] & ~noticed[m]))]


# ------------------------------------------------------------------------------------- realistic inputs (not exact): cos -> 1
# Features are a noisy linear image of 3-D points — an orthonormal 3 x 128 frame scaled by 2, plus noise — so x ~ s y and the
# terms are 1e-4 .. 1e-2: 1 - |cos| cancels, which integers cannot show.  dist = the points' pairwise distances.
REAL_CASES = [(300, 25), (1100, 25), (1100, 500)]      # (N, k), C = 128
REAL_ANCHORS = 16
REAL_NOISE = 0.01


@functools.lru_cache(maxsize=None)
def realistic_case(N, k, seed=SEED):
    rng = np.random.default_rng([seed, N, k, 128])
    pts = rng.random((N, 3))
    frame = np.linalg.qr(rng.standard_normal((128, 3)))[0].T                     # (3, 128), orthonormal rows
    feat = (2.0 * pts @ frame + REAL_NOISE * rng.standard_normal((N, 128))).astype(np.float32)
    diff = pts[:, None] - pts[None]
    dist = np.sqrt((diff * diff).sum(-1)).astype(np.float32)
    anchors = rng.permutation(N)[:REAL_ANCHORS].astype(np.int32)
    return dict(N=N, k=k, feat=feat, dist=dist, anchors=anchors)


def terms_f64_on_lists(feat, dist, anchors, idx):
    """float64 terms (nA,) of one batch element on GIVEN neighbour lists idx (nA, k): the definition, nothing rounded to float32"""
    feat, dist = np.asarray(feat, np.float64), np.asarray(dist, np.float64)
    anchors, idx = np.asarray(anchors, np.int64), np.asarray(idx, np.int64)
    d = feat[idx] - feat[anchors][:, None]
    x = np.sqrt((d * d).sum(-1))
    y = dist[idx, anchors[:, None]]
    c = (x * y).sum(1) / (np.maximum(np.sqrt((x * x).sum(1)), 1e-8) * np.maximum(np.sqrt((y * y).sum(1)), 1e-8))
    return 1.0 - np.abs(c)
