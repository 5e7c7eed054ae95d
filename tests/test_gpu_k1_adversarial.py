"""-m gpu: the K1 coarse screen (csrc/dvm_softcorr_coarse.hip) on query rows whose nearest columns are PLANTED at chosen lanes of
its tiling, inside otherwise random features.  The screen keeps, per half-lane and 32-column sub-tile, the two smallest keys in a
12-entry list and the third in a 16-bit record that covers `rgrp` sub-tiles (2 at M = 2048, 8 at M = 8192); sub-tiles whose
record lies at or below the row bound are re-done, the two half-lanes merge into 16 entries, and pass B certifies every row
against the largest entry written or flags it for the exact-rows kernel.  Each family below targets one link of that chain.

Planting.  Column j of the key side sits at sub-tile s = j // 32, half-lane h, register r with j = 32 s + 4 h + (r & 3) + 8 (r >> 2)
(make_keys).  A planted row q and its planted keys q + o have coordinates on a 1/256 grid below 8 in magnitude: at the common
scale (max |x s| in [2^11, 2^12)) every scaled coordinate is an fp16 number, so the coarse screen's one-plane product is exact
and its keys differ from the exact squared distances only by the 2^-14 truncation of the list entries.  The planted
arrangement is then the one the screen sees, also where the exact gaps are far below pass B's band delta.  Planted rows and
columns avoid the probe's samples (rows r N / 4, columns t M / min(M, 256)), and few rows are planted per entry, so that the
probe keeps the background's route and the gate (1/128 of a direction's rows flagged) does not replace the coarse lists.

Every case compares with the C oracle (columns and row maxima bit-exact, sums rtol 2e-5, values rtol 5e-5) and with a float64
dense softmax over all columns (values 1e-4 absolute; the k-th column's distance equal to the float64 k-th smallest within
4 fp32 ulps of the distance, which is how far two columns may swap on a near-tie), and the hard maps bit for bit with the oracle.
The route-forced reruns and the witnesses run in child processes (the route policy and DVM_DEBUG are read once per process).
(reference: models/loss.py:110-114 soft map, 91-95 hard map)"""
import ctypes
import os
import re
import subprocess
import sys
import zlib

import numpy as np
import pytest
import torch

from oracle import oracle as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = 128
HC_ERR = 1.12e-3                  # dvm_softcorr_f16.h: |d2_coarse - d2_exact| <= HC_ERR (|q|^2 + max |k|^2)
AM_BAND = 2 * (HC_ERR + 2e-5)     # the hard map's band around a row's best coarse value, in the same units
ROUTE = os.environ.get("DVM_K1_ROUTE")   # set in the route-forced child reruns


@pytest.fixture(scope="module")
def ops():
    from dvm import ops as _ops
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _ops


def lane_col(s, h, r):
    return 32 * s + 4 * h + (r & 3) + 8 * (r >> 2)


def rgrp_of(M):
    nsub = (M + 63) // 64 * 2                   # 64-key LDS tiles of two sub-tiles
    return (nsub + 31) // 32


def probe_rows(N):
    return {r * N // 4 for r in range(4)}


def probe_cols(M):
    C = min(M, 256)
    return {t * M // C for t in range(C)}


class Planter:
    """Plants rows of one batch entry: picks free registers of chosen (sub-tile, half-lane) slots and writes q + o there."""

    def __init__(self, f1, f2, b, rng):
        self.f1, self.f2, self.b, self.rng = f1, f2, b, rng
        N, M = f1.shape[1], f2.shape[1]
        self.N, self.M = N, M
        self.nsub = (M + 31) // 32
        self.rgrp = rgrp_of(M)
        self.probe = probe_cols(M)
        self.used = set()
        self.used_rows = set(probe_rows(N))
        self.cols = []                          # every planted column

    def row(self):
        free = [i for i in range(self.N) if i not in self.used_rows]
        i = int(self.rng.choice(free))
        self.used_rows.add(i)
        q = np.clip(np.round(self.rng.standard_normal(D) * 16) / 16, -2.5, 2.5).astype(np.float32)
        self.f1[self.b, i] = q
        return i, q

    def col(self, s, h, strict=True):
        """a free register of (s, h), off the probe's columns where one is left; strict=False: any free column nearby"""
        regs = [int(r) for r in self.rng.permutation(16)]
        cand = [lane_col(s, h, r) for r in regs]
        if not strict:
            cand += [lane_col((s + u) % self.nsub, (h + u) & 1, r) for u in range(1, self.nsub) for r in regs]
        cand = [j for j in cand if j < self.M and j not in self.used]
        pick = [j for j in cand if j not in self.probe] or cand
        if not pick:
            raise AssertionError("no free register at sub-tile %d half %d" % (s, h))
        self.used.add(pick[0])
        self.cols.append(pick[0])
        return pick[0]

    def free(self, s, h):
        return sum(1 for r in range(16) if lane_col(s, h, r) < self.M and lane_col(s, h, r) not in self.used)

    def subs(self, n, exclude=(), lo=0, hi=None, need=2):
        """n distinct sub-tiles with `need` free registers in both half-lanes (a ragged last one only if it holds 24 columns)"""
        hi = self.nsub if hi is None else hi
        pool = [s for s in range(lo, hi) if s not in exclude and self.M - 32 * s >= 24 and min(self.free(s, 0), self.free(s, 1)) >= need]
        return [int(s) for s in self.rng.choice(pool, size=n, replace=False)]

    def key(self, q, s, h, o):
        """o: {axis: offset} on the 1/256 grid; the key q + o lies at squared distance sum(o^2) from q."""
        j = self.col(s, h)
        k = q.copy()
        for ax, v in o.items():
            k[ax] = q[ax] - v if q[ax] >= 0 else q[ax] + v
        assert np.all(np.abs(k) < 8) and np.all(k * 256 == np.round(k * 256))
        self.f2[self.b, j] = k
        return j


def grid_up(x):
    return np.ceil(x * 256) / 256


class Ctx:
    def __init__(self, alpha, delta):
        self.cutw = 20.0 / alpha
        self.delta = delta
        self.base = 5.0
        # "high" keys: beyond the softmax cut of a row whose minimum is `base`, by 4 delta, and beyond the hard map's band
        band = AM_BAND / HC_ERR * delta
        self.high = grid_up(max(np.sqrt((self.base + self.cutw) ** 2 + 4 * delta), np.sqrt(self.base ** 2 + 2 * band)))

    def packed(self, t):                 # t-th of a packed run: exact gaps 2 base / 256 ~ 0.04 in d^2, far above the key truncation
        return self.base + t / 256

    def hi(self, t):
        return self.high + t / 256


def ax_for(rng):
    perm = rng.permutation(D)
    it = iter(perm)
    return lambda: int(next(it))


# near-tie squared-distance excesses (in units of 2^-16): 16 distinct sums of two squares, all within 4.5e-4 of each other
TIE = [0, 1, 2, 4, 5, 8, 9, 10, 13, 16, 17, 18, 20, 25, 26, 29]
TIE_M = {t: next((a, b) for a in range(6) for b in range(a, 6) if a * a + b * b == t) for t in TIE}


def stale_layout(P, q, c, dist_of):
    """The stale-bound arrangement (fixed in the coarse screen): half-lane B holds the 3 smallest, half-lane A 5 in one
    sub-tile (keys 1-5) and singles 6-13 in the packed run, then B's 13.5-13.8 and A's 14, 15 beyond the cut.  After the
    sweep A's list is {1, 2, 6, ..., 15}: the bound is A's 12th (15); the re-done sub-tile adds 3-5 and pushes 13-15 out of
    A's list while B's 13.5 stays written.  dist_of(slot) -> offset dict of the packed slot 0..15."""
    hA = int(P.rng.integers(2))
    hB = 1 - hA
    st = P.subs(1, need=5)[0]
    sa = [st] + sorted(P.subs(10, exclude=(st,)))
    singles, ahigh = sa[1:9], sa[9:]
    sb = P.subs(7)
    cols = {}
    for t in range(3):
        cols[t] = P.key(q, sb[t], hB, dist_of(t))
    for t in range(3, 8):
        cols[t] = P.key(q, st, hA, dist_of(t))
    for t, s in zip(range(8, 16), singles):
        cols[t] = P.key(q, s, hA, dist_of(t))
    nax = ax_for(P.rng)
    for u in range(4):
        P.key(q, sb[3 + u], hB, {nax(): c.hi(u)})
    for u, s in enumerate(ahigh):
        P.key(q, s, hA, {nax(): c.hi(4 + u)})
    return cols


def fam_stale(P, q, c):
    nax = ax_for(P.rng)
    stale_layout(P, q, c, lambda t: {nax(): c.packed(t)})


def fam_stale_tie(P, q, c):
    """Near-tie variant for the hard map: the 16 packed slots lie within 4.5e-4 of each other in d^2 (far below delta; a
    list entry keeps 2^-14 of the accumulator, ~1.6e-3 here, so they mostly share one 19-bit key and order by sub-tile),
    and the exact minimum sits at A's single in the highest sub-tile: the entry the stale bound drops."""
    ties = [t for t in TIE[1:]]
    P.rng.shuffle(ties)
    order = ties[:15]
    excess = {t: order[t] if t < 15 else 0 for t in range(16)}

    def off(t):   # (own axes per key: the keys are near-ties for q, not near-copies of each other)
        m1, m2 = TIE_M[excess[t]]
        a1, a2, a3 = (int(x) for x in P.rng.permutation(D)[:3])
        return {a1: c.base, a2: m1 / 256, a3: m2 / 256}
    stale_layout(P, q, c, off)


def fam_stack(n):
    def f(P, q, c):
        """n of the row's nearest columns in ONE half-lane of one sub-tile, the rest of its 12 nearest as singles."""
        h = int(P.rng.integers(2))
        nax = ax_for(P.rng)
        s0 = P.subs(1, need=n)[0]
        for t in range(n):
            P.key(q, s0, h, {nax(): c.packed(t)})
        for t, s in zip(range(n, 12), P.subs(max(0, 12 - n), exclude=(s0,))):
            P.key(q, s, int(P.rng.integers(2)), {nax(): c.packed(t)})
        for u, s in enumerate(P.subs(6, exclude=(s0,))):
            P.key(q, s, u & 1, {nax(): c.hi(u)})
    return f


def fam_group(P, q, c):
    """3 near columns in each of up to 4 sub-tiles of ONE record group (one 16-bit record holds their smallest third key)."""
    h = int(P.rng.integers(2))
    nax = ax_for(P.rng)
    rg = P.rgrp
    if rg == 1:
        s0 = P.subs(1, hi=P.nsub - 1)[0]
        tiles = [s0, s0 + 1]
    else:
        g = int(P.rng.integers((P.nsub - 1) // rg))
        tiles = [g * rg + u for u in range(min(rg, 4))]
    t = 0
    for s in tiles:
        for _ in range(3):
            P.key(q, s, h, {nax(): c.packed(t)})
            t += 1
    for u, s in enumerate(P.subs(6, exclude=tiles)):
        P.key(q, s, u & 1, {nax(): c.hi(u)})


def fam_cross(P, q, c):
    """3 near columns in the last sub-tile of one record group and 3 in the first of the next."""
    h = int(P.rng.integers(2))
    nax = ax_for(P.rng)
    rg = P.rgrp
    g = 1 + int(P.rng.integers(max(1, (P.nsub - 1) // rg - 1)))
    tiles = [g * rg - 1, g * rg]
    t = 0
    for s in tiles:
        for _ in range(3):
            P.key(q, s, h, {nax(): c.packed(t)})
            t += 1
    for u, s in enumerate(P.subs(6, exclude=tiles)):
        P.key(q, s, u & 1, {nax(): c.hi(u)})


def fam_dup(n):
    def f(P, q, c):
        """n exact copies of the row's nearest column over both half-lanes, several sub-tiles and record groups; ties go to
        the lowest column."""
        nax = ax_for(P.rng)
        ns = min(P.nsub, max(4, (n + 1) // 2))
        tiles = P.subs(ns)
        a = nax()
        j0 = P.key(q, tiles[0], 0, {a: c.packed(0)})
        for u in range(1, n):
            j = P.col(tiles[u % ns], (u // ns + u) & 1, strict=False)
            P.f2[P.b, j] = P.f2[P.b, j0]
        for t, s in zip(range(1, 5), P.subs(4)):
            P.key(q, s, t & 1, {nax(): c.packed(t)})
        for u, s in enumerate(P.subs(6)):
            P.key(q, s, u & 1, {nax(): c.hi(u)})
    return f


def fam_keyres(P, q, c):
    """Ranks 8-17 closer than 2^-14 relative: their list entries agree in the 19 key bits (order by sub-tile, half, register)."""
    nax = ax_for(P.rng)
    for t, s in enumerate(P.subs(8)):
        P.key(q, s, t & 1, {nax(): c.base - 0.25 + t / 256})
    ties = TIE[:10]
    for t, s in zip(P.rng.permutation(ties), P.subs(10)):
        m1, m2 = TIE_M[int(t)]
        a1, a2, a3 = (int(x) for x in P.rng.permutation(D)[:3])
        P.key(q, s, int(P.rng.integers(2)), {a1: c.base, a2: m1 / 256, a3: m2 / 256})
    for u, s in enumerate(P.subs(6)):
        P.key(q, s, u & 1, {nax(): c.hi(u)})


def fam_overflow(P, q, c):
    """List overflow inside the cut: the row's top-10 clear of the rest by more than delta, but 22 more columns well inside the
    softmax cut: the list of 16 cannot hold every term the row owes, so pass B must flag it on the cut condition alone."""
    nax = ax_for(P.rng)
    for t, s in enumerate(P.subs(10)):
        P.key(q, s, t & 1, {nax(): c.packed(t)})
    far = grid_up(c.base + 0.5 * c.cutw)
    for t, s in enumerate(P.subs(22)):
        P.key(q, s, t & 1, {nax(): far + t / 256})


def offset_d2(target, axes):
    """two grid offsets whose squares add up to `target` within 2e-3"""
    x = np.floor(np.sqrt(target) * 256) / 256
    y = np.round(np.sqrt(max(target - x * x, 0.0)) * 256) / 256
    assert abs(x * x + y * y - target) < 2e-3, target
    return {axes[0]: x, axes[1]: y}


CUT_EPS = 0.06   # d^2 margin of the cut-edge rows: above the entry truncation (~2e-3 here) and what later planted keys add to delta


def fam_cut(side):
    def f(P, q, c):
        """The cut edge: 15 packed columns inside the softmax cut, then the 16th written entry at d_cut^2 + delta + side CUT_EPS,
        the rest several delta beyond.  Pass B certifies the row only if d_cut^2 < tmax - delta (tmax: the 16th entry): it
        does by CUT_EPS for side = +1 and fails by CUT_EPS for side = -1 — whatever the 16 listed entries hold."""
        nax = ax_for(P.rng)
        for t, s in enumerate(P.subs(15)):
            P.key(q, s, t & 1, {nax(): c.packed(t)})
        # pass B's own terms: delta = HC_ERR (|q|^2 + max |k|^2 of the entry), d_cut = d_min 1.000001 + 20 / alpha
        delta = HC_ERR * (float((q.astype(np.float64) ** 2).sum()) + float((P.f2[P.b].astype(np.float64) ** 2).sum(1).max()))
        dcut = c.base * 1.000001 + c.cutw
        edge = dcut * dcut * 1.000001 + delta + side * CUT_EPS
        P.key(q, P.subs(1)[0], 1, offset_d2(edge, (nax(), nax())))
        for u, s in enumerate(P.subs(6)):
            P.key(q, s, u & 1, {nax(): c.hi(u)})
    return f


FAMILIES = {
    "stale": fam_stale, "stale_tie": fam_stale_tie,
    "stack3": fam_stack(3), "stack4": fam_stack(4), "stack5": fam_stack(5), "stack16": fam_stack(16),
    "group": fam_group, "cross": fam_cross,
    "dup9": fam_dup(9), "dup10": fam_dup(10), "dup11": fam_dup(11), "dup12": fam_dup(12), "dup13": fam_dup(13),
    "dup16": fam_dup(16), "dup17": fam_dup(17), "dup40": fam_dup(40),
    "keyres": fam_keyres, "overflow": fam_overflow, "cut_in": fam_cut(+1), "cut_out": fam_cut(-1),
}


def make_case(family, B, N, M, alpha, seed, rows_per_entry=None):
    """Random N(0, 1) background with `rows_per_entry` planted rows of `family` per entry (None: one per 256 rows)."""
    rng = np.random.default_rng(seed)
    f1 = rng.standard_normal((B, N, D)).astype(np.float32)
    f2 = rng.standard_normal((B, M, D)).astype(np.float32)
    nrow = min(16, max(1, N // 256)) if rows_per_entry is None else rows_per_entry
    planted = []
    for b in range(B):
        P = Planter(f1, f2, b, rng)
        delta = HC_ERR * (2.5 ** 2 * D + float((f2[b].astype(np.float64) ** 2).sum(1).max()))   # (|q|^2 <= 6.25 D)
        c = Ctx(alpha, delta)
        rows = []
        for _ in range(nrow):
            i, q = P.row()
            FAMILIES[family](P, q, c)
            rows.append(i)
        planted.append(sorted(rows))
    return f1, f2, planted


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def check_rows(b, rows, f1, f2, alpha, val, idx, smax, ssum, topk=10, planted=()):
    """The kernel's rows `rows` of entry b against the C oracle and against a float64 dense softmax over all columns.  The
    float64 bar is 1e-4 absolute on the planted rows, whose distances are exact in fp32; on random rows the fp32 chain itself
    (the reference's arithmetic) is off by a few ulps of the norms, and alpha times that is added to the bar."""
    rows = np.asarray(sorted(set(rows)))
    oval, oidx, osmax, osum = O.softcorr(f1[b][rows], f2[b], alpha, topk=topk)
    kv, ki, km, ks = val[b][rows], idx[b][rows], smax[b][rows], ssum[b][rows]
    bad = np.nonzero((ki != oidx).any(1))[0]
    assert bad.size == 0, "top-k columns differ from the oracle at rows %s" % rows[bad][:8]
    np.testing.assert_array_equal(km, osmax)
    np.testing.assert_allclose(ks, osum, rtol=2e-5, err_msg="row sums (oracle)")
    np.testing.assert_allclose(kv, oval, rtol=5e-5, atol=1e-30, err_msg="values (oracle)")
    # float64 dense reference: every column of the row
    q = torch.from_numpy(f1[b][rows]).cuda().double()
    k = torch.from_numpy(f2[b]).cuda().double()
    d2 = torch.cat([((q[i:i + 64, None, :] - k[None]) ** 2).sum(-1) for i in range(0, len(rows), 64)])
    d = d2.sqrt()
    logit = -alpha * d
    p = torch.softmax(logit, dim=1)
    dsorted = torch.sort(d, dim=1).values[:, :topk]
    kid = torch.from_numpy(ki.astype(np.int64)).cuda()
    dk = torch.gather(d, 1, kid)
    tol = 4 * 2.0 ** -23 * dsorted + 1e-30
    assert bool(((dk - dsorted).abs() <= tol).all()), "k-th column's float64 distance is not the k-th smallest"
    pk = host(torch.gather(p, 1, kid))
    norms = host((q * q).sum(1) + (k * k).sum(1).max())
    ed = 8 * 2.0 ** -24 * norms / np.maximum(host(d.min(1).values), 1e-30)       # fp32 chain: a few ulps of the norms, in d
    bar = np.where(np.isin(rows, np.asarray(list(planted), dtype=np.int64)), 1e-4, 1e-4 + alpha * ed)
    assert np.all(np.abs(kv - pk) <= bar[:, None]), ("values (float64 dense softmax)", float(np.abs(kv - pk).max()))
    # (no float64 bar on the sums: every term carries alpha times the fp32 rounding of its distance, ~2e-4 relative at
    # alpha 100 on the background rows; the sums are held to the oracle's fp32 chain above)


def last_routes(ops):
    from dvm import _lib
    c = (ctypes.c_int * 5)()
    ops.check(_lib.load().dvm_k1_last_routes(c), "dvm_k1_last_routes")
    return list(c)


def sample_rows(N, planted, seed, extra=48):
    rng = np.random.default_rng(seed)
    return sorted(set(planted) | set(int(x) for x in rng.choice(N, size=min(N, extra), replace=False)))


SHAPES = [(256, 1024), (255, 1025), (257, 2048), (2048, 4095), (2048, 8192), (8192, 2048)]
FAST_SHAPES = [(256, 1024), (257, 2048), (2048, 8192)]


def shape_id(s):
    return "%dx%d" % s


def cases():
    out = []
    for fam in FAMILIES:
        shapes = SHAPES if fam in ("stale", "stale_tie", "stack3", "stack16", "group", "cross", "dup17", "overflow", "cut_in", "cut_out") else FAST_SHAPES
        for s in shapes:
            for alpha in (32.0, 100.0):
                out.append(pytest.param(fam, s, alpha, id="%s-%s-a%d" % (fam, shape_id(s), alpha)))
    return out


@pytest.mark.parametrize("family,shape,alpha", cases())
def test_planted_softcorr(ops, family, shape, alpha):
    """variant 3 (the routed 16-bit path) on planted rows + a seeded sample of background rows."""
    N, M = shape
    B = 2
    seed = zlib.crc32(("%s %d %d %g" % (family, N, M, alpha)).encode())
    f1, f2, planted = make_case(family, B, N, M, alpha, seed)
    val, idx, smax, ssum = ops.softcorr(dev(f1), dev(f2), alpha, topk=10, variant=3)
    r = last_routes(ops)
    val, idx, smax, ssum = host(val), host(idx), host(smax), host(ssum)
    for b in range(B):
        check_rows(b, sample_rows(N, planted[b], seed + b), f1, f2, alpha, val, idx, smax, ssum, planted=planted[b])
    # the route the planted entries took: whatever is forced, else the probe's choice on the background; behind the coarse
    # screen the gate stays silent (few planted rows), so the lists checked above are the coarse screen's own
    assert r[4] == B and sum(r[:3]) == B, r
    if ROUTE == "3":
        assert r[2] == B, r
    elif ROUTE in ("1", "0"):
        assert r[int(ROUTE)] == B, r
    if r[2] == B and alpha >= 100 and not family.startswith("dup"):
        # (at alpha 32 random rows alone can flag more than 1/128 of a direction at M = 8192, and the gate then re-sweeps it;
        # a cluster of copied columns lies within the cut of ~1 in 1000 random rows, which then cannot be certified either)
        assert r[3] == 0, ("the gate re-swept planted entries", r)


def test_planted_mixed_batch_equals_single_entries(ops):
    """One launch of a clean (background-only) entry, planted entries of several families and a gate-flooding entry: every
    entry's integer outputs equal its B = 1 run bit for bit; floats bit for bit where the route is the same, else at the
    oracle's bars.  The flooding entry sends the direction away from the coarse lists: the probe routes it elsewhere, or the
    gate re-sweeps it."""
    N, M, alpha = 1024, 2048, 100.0
    fams = ["stale", "stack5", "dup13", "keyres", "cross"]
    parts = [make_case("stale", 1, N, M, alpha, 899, rows_per_entry=0)]
    parts += [make_case(f, 1, N, M, alpha, 900 + u) for u, f in enumerate(fams)]
    f1 = np.concatenate([p[0] for p in parts])
    f2 = np.concatenate([p[1] for p in parts])
    rng = np.random.default_rng(7)
    fl1 = rng.standard_normal((1, N, D)).astype(np.float32)
    fl2 = np.repeat(fl1[:, :64], M // 64, axis=1) + 1e-3 * rng.standard_normal((1, M, D)).astype(np.float32)   # clusters
    f1, f2 = np.concatenate([f1, fl1]), np.concatenate([f2, fl2])
    outs = [host(t) for t in ops.softcorr(dev(f1), dev(f2), alpha, topk=10, variant=3)]
    rb = last_routes(ops)
    B = f1.shape[0]
    assert rb[4] == B and (rb[2] < B or rb[3] == B), ("the clustered entry floods the direction: the gate must re-sweep it", rb)
    if ROUTE == "3":
        assert rb[2] == B and rb[3] == B, rb
    for b in range(f1.shape[0]):
        one = [host(t) for t in ops.softcorr(dev(f1[b:b + 1]), dev(f2[b:b + 1]), alpha, topk=10, variant=3)]
        r1 = last_routes(ops)
        assert np.array_equal(one[1][0], outs[1][b]), "entry %d: columns differ from its B = 1 run" % b
        np.testing.assert_array_equal(one[2][0], outs[2][b])
        if b < len(parts) and r1[2] == 1:
            assert r1[3] == 0, ("entry %d alone: the gate re-swept it" % b, r1)
        same = r1 == [x // f1.shape[0] for x in rb] or ROUTE in ("0", "1")
        if same:
            np.testing.assert_array_equal(one[0][0], outs[0][b])
            np.testing.assert_array_equal(one[3][0], outs[3][b])
        else:
            np.testing.assert_allclose(outs[3][b], one[3][0], rtol=2e-5)
            np.testing.assert_allclose(outs[0][b], one[0][0], rtol=5e-5, atol=1e-30)
        pl = parts[b][2][0] if b < len(parts) else []   # (entry 0: clean, no planted rows)
        check_rows(b, sample_rows(N, pl, 40 + b, extra=24), f1, f2, alpha, *outs, planted=pl)


@pytest.mark.parametrize("family", ["stale", "stale_tie", "stack5", "group", "cross", "dup13", "dup40", "keyres"])
@pytest.mark.parametrize("shape", [(256, 1024), (2048, 2048), (1024, 8192)], ids=shape_id)
def test_planted_hard_map(ops, family, shape):
    """argmin_exact (screened and not) and argmin_pair on the same families: indices and distances bit for bit with the
    oracle.  The hard map always takes the coarse screen first; its gate fires at 1/16 of a direction's rows."""
    N, M = shape
    B = 2
    seed = zlib.crc32(("am %s %d %d" % (family, N, M)).encode())
    f1, f2, planted = make_case(family, B, N, M, 100.0, seed, rows_per_entry=max(4, N // 128))
    T, dm = ops.argmin_exact(dev(f1), dev(f2), want_dist=True)
    Tf, dmf = ops.argmin_exact(dev(f1), dev(f2), want_dist=True, screen=False)
    T12, T21 = ops.argmin_pair(dev(f1), dev(f2))
    T, dm, Tf, dmf, T12, T21 = (host(x) for x in (T, dm, Tf, dmf, T12, T21))
    for b in range(B):
        rows = sample_rows(N, planted[b], seed + b)
        oT, odm = O.argmin_exact(f1[b][rows], f2[b])
        bad = np.nonzero(T[b][rows] != oT)[0]
        assert bad.size == 0, "screened hard map differs from the oracle at rows %s" % np.asarray(rows)[bad][:8]
        np.testing.assert_array_equal(dm[b][rows], odm)
        np.testing.assert_array_equal(Tf[b][rows], oT)
        np.testing.assert_array_equal(dmf[b][rows], odm)
        np.testing.assert_array_equal(T12[b][rows], oT)
        cols = sample_rows(M, [], seed + 7 + b, extra=64)
        oT21, _ = O.argmin_exact(f2[b][cols], f1[b])
        np.testing.assert_array_equal(T21[b][cols], oT21)


@pytest.mark.parametrize("where", ["f1_last", "f2_last", "f1_first", "f2_first"])
@pytest.mark.parametrize("shape", [(300, 170), (150, 5), (65, 33)], ids=shape_id)
def test_hard_map_absmax_at_the_edge_rows(ops, shape, where):
    """The hard map's scale comes from the absmax slots of the row-norm kernel (8 rows per half-wave, 64 per workgroup).  One
    element of 300.0 in the last channel of the last row of the last batch entry (or of row 0 of entry 0), in either tensor, among
    unit normal features: with that maximum missed the scale would take it past fp16's range (300 x 2^9).  Every row of both
    maps, and the distances, bit for bit against the oracle and against screen=False."""
    N, M = shape
    B = 2
    rng = np.random.default_rng(zlib.crc32(("edge %d %d %s" % (N, M, where)).encode()))
    f1 = rng.standard_normal((B, N, D)).astype(np.float32)
    f2 = rng.standard_normal((B, M, D)).astype(np.float32)
    t = f1 if where.startswith("f1") else f2
    if where.endswith("last"):
        t[B - 1, -1, D - 1] = 300.0
    else:
        t[0, 0, D - 1] = 300.0
    T, dm = ops.argmin_exact(dev(f1), dev(f2), want_dist=True)
    Tf, dmf = ops.argmin_exact(dev(f1), dev(f2), want_dist=True, screen=False)
    T12, T21 = ops.argmin_pair(dev(f1), dev(f2))
    T, dm, Tf, dmf, T12, T21 = (host(x) for x in (T, dm, Tf, dmf, T12, T21))
    for b in range(B):
        oT, odm = O.argmin_exact(f1[b], f2[b])
        np.testing.assert_array_equal(T[b], oT)
        np.testing.assert_array_equal(dm[b], odm)
        np.testing.assert_array_equal(Tf[b], oT)
        np.testing.assert_array_equal(dmf[b], odm)
        np.testing.assert_array_equal(T12[b], oT)
        np.testing.assert_array_equal(T21[b], O.argmin_exact(f2[b], f1[b])[0])


def test_coarse_limit_8193_takes_another_form(ops):
    """M or N = 8193 is beyond the coarse screen's 8-bit sub-tile field: even with route 3 forced the launch must be served by
    another form, say so in dvm_k1_last_routes, and still give the oracle's results."""
    for N, M in ((512, 8193), (8193, 512)):
        f1, f2, planted = make_case("stack5", 1, N, M, 100.0, N + 3 * M, rows_per_entry=4)
        val, idx, smax, ssum = (host(t) for t in ops.softcorr(dev(f1), dev(f2), 100.0, topk=10, variant=3))
        r = last_routes(ops)
        assert r[4] == 1 and r[2] == 0, ("the coarse screen cannot serve %d x %d" % (N, M), r)
        check_rows(0, sample_rows(N, planted[0], 11, extra=32), f1, f2, 100.0, val, idx, smax, ssum, planted=planted[0])
        T = host(ops.argmin_exact(dev(f1), dev(f2)))
        rows = sample_rows(N, planted[0], 12, extra=32)
        np.testing.assert_array_equal(T[0][rows], O.argmin_exact(f1[0][rows], f2[0])[0])


def test_pair_forward_planted_both_directions(ops, golden):
    """ops.pair_forward at 2048 x 2048 with planted rows in both directions against O.pair_direction (the bars of
    test_pair_forward_contract_size_low_alpha_vs_oracle)."""
    w = golden("deformer_scape_r_weights")
    wl = ops.deformer_weight_list(w, "cuda")
    B, N, alpha = 2, 2048, 100.0
    rng = np.random.default_rng(4242)
    f1 = rng.standard_normal((B, N, D)).astype(np.float32)
    f2 = rng.standard_normal((B, N, D)).astype(np.float32)
    for b in range(B):
        fwd = Planter(f1, f2, b, rng)                     # rows of f1, keys in f2
        rev = Planter(f2, f1, b, rng)                     # rows of f2, keys in f1

        def exchange():   # an f2 row is a forward key or a reverse query row, an f1 row a forward query row or a reverse key
            rev.used |= fwd.used_rows
            rev.used_rows |= fwd.used
            fwd.used |= rev.used_rows
            fwd.used_rows |= rev.used
        rows_f, rows_r = [], []
        for _ in range(8):
            c = Ctx(alpha, HC_ERR * (2.5 ** 2 * D + 200.0))
            exchange()
            i, q = fwd.row()
            FAMILIES["stale"](fwd, q, c)
            rows_f.append(i)
            exchange()
            i, q = rev.row()
            FAMILIES["stack5"](rev, q, c)
            rows_r.append(i)
        # no planted row or key of one direction overwrites one of the other
        assert not set(rows_f) & set(rev.cols) and not set(rows_r) & set(fwd.cols), b
    g = torch.Generator().manual_seed(5)
    v1, v2 = torch.rand(B, N, 3, generator=g).numpy(), torch.rand(B, N, 3, generator=g).numpy()
    s1, s2 = np.array([3, 2000], np.int32), np.array([0, 1024], np.int32)
    o12, o21 = ops.pair_forward(wl, dev(f1), dev(f2), dev(v1), dev(v2), alpha, dev(s1), dev(s2))
    torch.cuda.synchronize()
    for b in range(B):
        for out, (fa, fb, va, vb, st) in ((o12, (f1, f2, v1, v2, s1)), (o21, (f2, f1, v2, v1, s2))):
            o = O.pair_direction(w, fa[b], fb[b], va[b], vb[b], alpha, int(st[b]))
            assert np.array_equal(host(out["T12"])[b], o["T12"]), "arg-max map differs from the oracle"
            np.testing.assert_allclose(host(out["verts12"])[b], o["verts12"], rtol=0, atol=1e-5)
            np.testing.assert_allclose(host(out["warped"])[b], o["warped"], rtol=0, atol=1e-4)
            np.testing.assert_allclose(host(out["losses"])[b], o["losses"], rtol=1e-3)


def test_cut_shell_every_other_column_just_beyond_the_cut(ops):
    """One row whose other columns lie just beyond its softmax cut at M = 8192 (all but the other rows' private keys): the terms
    a certified list leaves out total ~M e^-20 (5e-6 of the sum here), next to the 2e-5 sum bar.  The row against the float64
    sum over ALL columns.  It sits at the origin with its nearest column (d_min = 0); the shell keys at (1.03 ... 1.05) 20 / alpha
    in random directions; every other row 3 cut-widths out with 11 private keys between one and 1.4 cut-widths away (its top-10
    and cut lie in its list, far from the shell)."""
    alpha, N, M = 100.0, 256, 8192
    c = 20.0 / alpha
    rng = np.random.default_rng(8192)

    def unit(n):
        v = rng.standard_normal((n, D))
        return v / np.linalg.norm(v, axis=1, keepdims=True)
    f1 = (3 * c * unit(N)).astype(np.float32)
    i0, j0 = 5, 3                                          # (off the probe's rows and columns)
    f1[i0] = 0.0
    f2 = (c * (1.03 + 0.02 * rng.random((M, 1))) * unit(M)).astype(np.float32)
    f2[j0] = 0.0
    cols = iter(j for j in range(M) if j != j0 and j % 32 != 0)
    priv = []
    for i in range(N):
        if i != i0:
            for t in range(11):
                j = next(cols)
                f2[j] = f1[i] + (c * (1 + 0.04 * t) * unit(1)[0]).astype(np.float32)
                priv.append(j)
    f1, f2 = f1[None], f2[None]
    val, idx, smax, ssum = (host(t) for t in ops.softcorr(dev(f1), dev(f2), alpha, topk=10, variant=3))
    r = last_routes(ops)
    if ROUTE == "3":
        assert r[2] == 1 and r[3] == 0, ("the coarse screen serves the shell and certifies its rows", r)
    # float64 over every column: the shell's share of the sum is what a certified list leaves out
    d = np.sqrt(((f2[0].astype(np.float64) - f1[0, i0].astype(np.float64)) ** 2).sum(1))
    terms = np.exp(-alpha * (d - d.min()))
    shell = terms[sorted(set(range(M)) - set(priv) - {j0})]
    assert 3e-6 < shell.sum() / terms.sum() < 2e-5, shell.sum() / terms.sum()     # the row indeed sits next to the bar
    assert float(smax[0, i0]) == 0.0
    np.testing.assert_allclose(ssum[0, i0], terms.sum(), rtol=2e-5, err_msg="the shell row's sum (float64, every column)")
    check_rows(0, sample_rows(N, [i0], 9, extra=32), f1, f2, alpha, val, idx, smax, ssum, planted=[i0])


@pytest.mark.parametrize("shape", [(1024, 2048), (2048, 8192)], ids=shape_id)
def test_norm_outliers(ops, shape):
    """(a) One key at 100 x the norm of the others in one entry: pass B's delta = HC_ERR (|q|^2 + max |k|^2) widens 10^4 x, no
    row of that entry can be certified, and the gate must send the direction through the lean form (count[3] = B behind the
    coarse screen).  (b) Query rows at 1e-3 and 1e3 x scale in one entry: the common scale follows the large rows (2^-1 here),
    the small rows' own norms vanish next to the 4.5 floor of the accumulator.  Both against the oracle and float64."""
    N, M = shape
    B, alpha = 2, 100.0
    f1, f2, planted = make_case("stack5", B, N, M, alpha, 77 + M)
    f2[1, 7] *= 100.0                                     # (column 7: off the probe's columns)
    val, idx, smax, ssum = (host(t) for t in ops.softcorr(dev(f1), dev(f2), alpha, topk=10, variant=3))
    r = last_routes(ops)
    assert r[4] == B and (r[2] < B or r[3] == B), ("an unflaggable entry behind the coarse screen: the gate must fire", r)
    if ROUTE == "3":
        assert r[2] == B and r[3] == B, r
    for b in range(B):
        check_rows(b, sample_rows(N, planted[b] + [i for i in range(8, 16)], 5 + b), f1, f2, alpha, val, idx, smax, ssum,
                   planted=planted[b])
    g1 = f1.copy()
    free = [i for i in range(N) if i not in planted[0] and i not in probe_rows(N)][:16]
    small, big = free[:8], free[8:12]
    g1[0, small] *= 1e-3
    g1[0, big] *= 1e3
    val, idx, smax, ssum = (host(t) for t in ops.softcorr(dev(g1), dev(f2), alpha, topk=10, variant=3))
    for b in range(B):
        rows = sample_rows(N, planted[b] + (small + big if b == 0 else []), 15 + b)
        check_rows(b, rows, g1, f2, alpha, val, idx, smax, ssum, planted=planted[b])


# ---------------------------------------------------------------- child processes: forced routes and witnesses
def _child(args, env_extra, timeout):
    env = dict(os.environ)
    env.pop("DVM_K1_ROUTE", None), env.pop("DVM_K1_ROUTE_P", None), env.pop("DVM_DEBUG", None)
    env.update(env_extra)
    return subprocess.run([sys.executable] + args, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)


@pytest.mark.skipif(ROUTE is not None, reason="(inside a route-forced rerun)")
@pytest.mark.parametrize("route", ["3", "1", "0"], ids=["coarse", "lean", "full"])
def test_child_planted_with_the_route_forced(route):
    r = _child(["-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider",
                "-k", "not child_ and not pair_forward and not hard_map"], {"DVM_K1_ROUTE": route}, 600)
    tail = (r.stdout or "")[-2500:] + (r.stderr or "")[-800:]
    assert r.returncode == 0, tail
    assert " passed" in r.stdout and "failed" not in r.stdout, tail


WITNESS = r"""
import os, sys
sys.path.insert(0, %(root)r); sys.path.insert(0, os.path.join(%(root)r, 'dv-matcher_amd')); sys.path.insert(0, os.path.join(%(root)r, 'tests'))
import numpy as np, torch
from dvm import ops
import test_gpu_k1_adversarial as T
N = M = 2048
def run(tag, f1, f2, alpha):
    print('@@' + tag, file=sys.stderr, flush=True)
    ops.softcorr(T.dev(f1), T.dev(f2), alpha, topk=10, variant=3)
    torch.cuda.synchronize()
    print('routes %%s' %% T.last_routes(ops), file=sys.stderr, flush=True)
    print('@@end', file=sys.stderr, flush=True)
for alpha in (100.0,):
    f1, f2, _ = T.make_case('stale', 2, N, M, alpha, 1, rows_per_entry=0)
    run('background %%g' %% alpha, f1, f2, alpha)
    for fam in %(fams)r:
        f1, f2, _ = T.make_case(fam, 2, N, M, alpha, 1, rows_per_entry=T.WITNESS_ROWS.get(fam, 8))
        run('%%s %%g' %% (fam, alpha), f1, f2, alpha)
# the re-done records: EVERY query row of an entry lane-stacked (64 distinct planted rows, each repeated 32 times, 3 near keys in
# one half-lane of a sub-tile of its own record group)
rng = np.random.default_rng(3)
f1 = rng.standard_normal((1, N, 128)).astype(np.float32)
f2 = rng.standard_normal((1, M, 128)).astype(np.float32)
P = T.Planter(f1, f2, 0, rng)
P.used = set()
c = T.Ctx(100.0, 0.4)
for u in range(64):
    q = np.clip(np.round(rng.standard_normal(128) * 16) / 16, -2.5, 2.5).astype(np.float32)
    f1[0, u::64] = q
    s = (u %% 32) * P.rgrp + (u // 32)
    nax = T.ax_for(rng)
    for t in range(3):
        P.key(q, s, u & 1, {nax(): c.packed(t)})
run('allstacked', f1, f2, 100.0)
run('allbackground', rng.standard_normal((1, N, 128)).astype(np.float32), rng.standard_normal((1, M, 128)).astype(np.float32), 100.0)
"""
WITNESS_FAMS = ["stale", "stale_tie", "stack3", "stack5", "stack16", "group", "cross", "dup10", "dup17", "dup40", "keyres", "overflow",
                "cut_in", "cut_out"]
# planted rows per entry (2 entries): 8, but 2 for the big copy clusters — a cluster of 17 or 40 copies also lies within the cut
# of a few random rows, and the direction must stay under the gate's 1/128 (32 of 4096 rows) for the count to be the coarse screen's
WITNESS_ROWS = {"dup17": 2, "dup40": 2}


def _witness_blocks(stderr):
    out, tag = {}, None
    for ln in stderr.splitlines():
        if ln.startswith("@@"):
            tag = None if ln == "@@end" else ln[2:]
            if tag:
                out[tag] = []
        elif tag:
            out[tag].append(ln)
    return out


@pytest.mark.skipif(ROUTE is not None, reason="(inside a route-forced rerun)")
def test_child_witnesses_flagged_rows_and_redone_records():
    """DVM_DEBUG = 10 (flagged rows + the stamped coarse form), route 3 forced.  Flagged rows rise where a family is meant to be
    flagged and stay at the background's count where it tests the coarse lists themselves; a launch whose every row is
    lane-stacked re-does far more records per wave than a background-only launch."""
    code = WITNESS % {"root": ROOT, "fams": WITNESS_FAMS}
    r = _child(["-c", code], {"DVM_K1_ROUTE": "3", "DVM_DEBUG": "10"}, 300)
    assert r.returncode == 0, r.stderr[-3000:]
    blocks = _witness_blocks(r.stderr)
    flagged, redo, routes = {}, {}, {}
    for tag, lines in blocks.items():
        for ln in lines:
            if ln.startswith("routes "):
                routes[tag] = eval(ln[7:])
            m = re.search(r"K1 pass B: (\d+) \+ (\d+) of (\d+) rows", ln)
            if m:
                flagged[tag] = int(m.group(1)) + int(m.group(2))
            m = re.search(r"([0-9.]+) re-done records per wave", ln)
            if m:
                redo[tag] = float(m.group(1))
    print("flagged rows:", flagged)
    print("re-done records per wave:", redo)
    sys.stderr.write("witness flagged %s\nwitness redo %s\n" % (flagged, redo))
    for tag in routes:   # every launch on the coarse screen, none re-swept by the gate: the counts are the coarse screen's
        if tag.startswith("all"):
            continue
        assert routes[tag][2] == routes[tag][4] and routes[tag][3] == 0, (tag, routes[tag])
    for alpha in ("100",):   # (at alpha 32 the background alone comes near the gate's 1/128 once planted rows add to it)
        bg = flagged["background " + alpha]
        assert bg <= 4, (alpha, flagged)
        # families whose row cannot be certified from a list of 16 (or sits just outside the certification threshold): every
        # planted row flagged
        for fam in ("stale", "stack16", "dup17", "dup40", "keyres", "overflow", "cut_out"):
            assert flagged["%s %s" % (fam, alpha)] >= bg + 2 * WITNESS_ROWS.get(fam, 8), (fam, alpha, flagged)
        # families whose lists certify the row (cut_in: just inside the threshold): no more than the background
        for fam in ("stack3", "stack5", "group", "cross", "cut_in"):
            assert flagged["%s %s" % (fam, alpha)] <= bg + 2, (fam, alpha, flagged)
    assert redo["allbackground"] < 4, redo
    assert redo["allstacked"] > redo["allbackground"] + 20, redo
