"""The Deformer's decoder MLP (262 -> 512 -> 256 -> 128 -> 9, ELU; csrc/dvm_mlp_f16.hip, dvm_mlp_bf16.hip) judged ROW BY ROW at
the edges of the fp16 planes' range.  The two-plane kernel multiplies fp32 operands as fixed-scale fp16 planes (activations x 32,
weights x 256; three of the four partial products); its range guard is the output (an overflow anywhere surfaces as NaN, the flag
comes up, the bf16x3 kernel recomputes the whole launch).  The parity suite compares whole launches at 2e-5 of the launch's
largest output; here every row is held to a bar of its own scale.

Reference  the MLP in float64 numpy (x @ W.T + b, expm1 ELU) on the float32 inputs and weights.
Yardstick  the same MLP in float32 numpy with exp(x) - 1 (what the reference project computes):
           noise(F) = max over the rows of family F and the nine outputs of |fp32 - fp64|.
Bar        a row drawn from family F satisfies max_o |gpu - fp64| <= 3 noise(F), wherever in the launch it sits and whatever its
           neighbours are (DESIGN.md section 2's "3 x the same formulation's fp32-vs-fp64 noise", per family instead of per launch).
           The bar is never derived from what the GPU returns.

Families (rows x 262 float32, one seed each, homogeneous in scale so that noise(F) is one stable number) are listed at family();
the synthetic weight sets at weights().  A launch of n rows of a family takes the family's rows cyclically, so every row of
every launch is a member of the family its bar was computed on.  The first test of the module runs without a GPU: it checks the
inputs themselves (finite where they claim to be, the brink rows where they claim to be, the small families' bars below what a
flushed fp16 subnormal would cost).  Each GPU test prints `MLPROWS <case> <kernel> noise err ratio` before it asserts
(profiles/notes_mlp_rows.md is made from those lines).
(reference: models/model.py:433-452 MLP, 464-478 Deformer)"""
import functools
import os
import zlib

import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
LIM = 65504.0 / 32.0              # the largest activation whose scaled value is an fp16 number (dvm_mlp_f16.h: MH_SA = 32)
W_LIMIT = 60000.0 / 256.0         # the packing kernels' weight guard (MH_LIMIT / MH_SW)
WKEY, BKEY = "deformation_decoder_layer__linear__%d__weight", "deformation_decoder_layer__linear__%d__bias"
LAYERS = (0, 2, 4, 6)
BIG = 2 * 256 * 64 + 77           # more 64-row blocks than compute units x blocks per workgroup


# ------------------------------------------------------------------------------------------------------------------ references
def mats(w):
    return ([np.asarray(w[WKEY % i], np.float32) for i in LAYERS], [np.asarray(w[BKEY % i], np.float32) for i in LAYERS])


def chain64(w, x, hidden=False):
    """the decoder on float64 rows; hidden=True: also the largest |activation| per row over the input and the three hidden layers"""
    W, b = mats(w)
    with np.errstate(all="ignore"):
        hm = np.abs(x).max(1)
        for i in range(4):
            x = x @ W[i].astype(np.float64).T + b[i].astype(np.float64)
            if i < 3:
                x = np.where(x > 0, x, np.expm1(np.minimum(x, 0)))
                hm = np.maximum(hm, np.abs(x).max(1))
    return (x, hm) if hidden else x


def mlp64(w, z, hidden=False):
    """the reference: float64 on the float32 rows and weights"""
    return chain64(w, np.asarray(z, np.float32).astype(np.float64), hidden)


def mlp32(w, z):
    """the yardstick: float32 throughout, ELU as exp(x) - 1"""
    W, b = mats(w)
    with np.errstate(all="ignore"):
        x = np.asarray(z, np.float32)
        for i in range(4):
            x = (x @ W[i].T + b[i]).astype(np.float32)
            if i < 3:
                x = np.where(x > 0, x, np.exp(np.minimum(x, np.float32(0))) - np.float32(1)).astype(np.float32)
    return x


# ------------------------------------------------------------------------------------------------------------------ weight sets
@functools.lru_cache(maxsize=None)
def weights(name="trained"):
    """trained    the committed decoder (tests/golden/deformer_scape_r_weights.npz)
    tiny_w     every |w| ~ 1e-5 (biases as trained): 256 w ~ 2.6e-3, so every m plane of the weights is an fp16 subnormal
    sparse_w   the trained matrices with 90 % of the entries exact zeros, a quarter of those -0.0
    wide_w     |w| = 10^U(-6, 0) per element with random signs: six decades inside one contraction
    w_flag_l1  trained, one weight of layer 1 set to 250 > 60000 / 256: the packing kernel's guard (pack_weights_f16_body)
    w_flag_l3  the same in layer 3, which the persistent kernel packs on its own path (pack_w3x_body)
    conv_b0    trained with the pooling convolution's bias set to zero (so that pooled rows of small features stay small)"""
    w = dict(np.load(os.path.join(GOLDEN, "deformer_scape_r_weights.npz")))
    g = np.random.default_rng(zlib.crc32(name.encode()))
    if name == "tiny_w":
        for i in LAYERS:
            w[WKEY % i] = (1e-5 * g.standard_normal(w[WKEY % i].shape)).astype(np.float32)
    elif name == "sparse_w":
        for i in LAYERS:
            W = w[WKEY % i].copy()
            u = g.random(W.shape)
            W[u < 0.9] = 0.0
            W[u < 0.225] = -0.0
            w[WKEY % i] = W
    elif name == "wide_w":
        for i in LAYERS:
            s = w[WKEY % i].shape
            w[WKEY % i] = (np.sign(g.standard_normal(s)) * 10.0 ** g.uniform(-6.0, 0.0, s)).astype(np.float32)
    elif name == "w_flag_l1":
        W = w[WKEY % 2].copy()
        W[7, 300] = 250.0
        w[WKEY % 2] = W
    elif name == "w_flag_l3":
        W = w[WKEY % 6].copy()
        W[4, 77] = 250.0
        w[WKEY % 6] = W
    elif name == "conv_b0":
        w["conv_layer__bias"] = np.zeros_like(w["conv_layer__bias"])
    else:
        assert name == "trained", name
    return w


WEIGHT_SETS_IN_RANGE = ["tiny_w", "sparse_w", "wide_w"]


# ------------------------------------------------------------------------------------------------------------------ families
def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _path_like(g, n):
    return np.concatenate([g.random((n, 3)), 0.3 * np.maximum(g.standard_normal((n, 128)), 0), g.random((n, 3)),
                           0.3 * np.maximum(g.standard_normal((n, 128)), 0)], 1).astype(np.float32)


def _brink(name, frac):
    """randn rows, each scaled by bisection in float64 so that its largest |activation| (input and hidden layers, trained weights)
    is frac x 65504 / 32"""
    g = _rng(name)
    base = g.standard_normal((128, 262)).astype(np.float32)
    lo, hi = np.zeros(128), np.full(128, 1e5)
    w = weights()
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        hm = mlp64(w, base * mid.astype(np.float32)[:, None], hidden=True)[1]
        below = hm < frac * LIM
        lo, hi = np.where(below, mid, lo), np.where(below, hi, mid)
    return (base * lo.astype(np.float32)[:, None]).astype(np.float32)


@functools.lru_cache(maxsize=None)
def family(name):
    """unit           randn: the scale every other Deformer test uses
    path_like      [rand(3) | 0.3 relu(randn(128)) | rand(3) | 0.3 relu(randn(128))]: what the pair path feeds the decoder; half the
                   feature columns are exact zeros, a quarter of those carry the sign bit (-0.0)
    small_1e-4     1e-4 randn: 32 z ~ 3e-3, the m plane (~1.5e-6) lies wholly in fp16's subnormals
    small_1e-6     1e-6 randn: the h plane is subnormal too
    tiny_1e-10     1e-10 randn: 32 z is below half of fp16's smallest subnormal, both planes round to zero, the output is the bias path
    mixed_decades  randn x 10^k, k uniform in -7 .. 1 per element: normal, subnormal and vanishing planes inside one contraction
    one_hot_1      row i holds 1.0 in column i and zeros elsewhere, i = 0 .. 261: pins mh_zcol_of_plane_col and the packed layer-0
    one_hot_1e-3   weights column by column (the six coordinate columns sit at plane columns 256 .. 261); the same with 1e-3
    brink_in       randn rows scaled so that the largest |activation| is 0.97 x 65504 / 32: just inside the two-plane kernel's range
    brink_out      the same at 1.03: just outside, the row must come back from the fallback
    blown          randn x 4000: far outside (the parity suite's fallback input)
    blown_coords   path_like rows whose three source coordinates are 3000 rand: the fused pair test's situation"""
    g = _rng(name)
    if name == "unit":
        z = g.standard_normal((256, 262))
    elif name == "path_like":
        z = _path_like(g, 256)
        z[(z == 0) & (g.random(z.shape) < 0.25)] = -0.0
    elif name in ("small_1e-4", "small_1e-6", "tiny_1e-10"):
        z = float(name.split("_")[1]) * g.standard_normal((256, 262))
    elif name == "mixed_decades":
        z = g.standard_normal((256, 262)) * 10.0 ** g.integers(-7, 2, (256, 262))
    elif name in ("one_hot_1", "one_hot_1e-3"):
        z = float(name[8:]) * np.eye(262)
    elif name == "brink_in":
        z = _brink(name, 0.97)
    elif name == "brink_out":
        z = _brink(name, 1.03)
    elif name == "blown":
        z = 4000.0 * g.standard_normal((128, 262))
    elif name == "blown_coords":
        z = _path_like(g, 128)
        z[:, :3] = 3000.0 * g.random((128, 3))
    else:
        raise KeyError(name)
    z = np.ascontiguousarray(z, np.float32)
    z.setflags(write=False)
    return z


IN_RANGE = ["unit", "path_like", "small_1e-4", "small_1e-6", "tiny_1e-10", "mixed_decades", "one_hot_1", "one_hot_1e-3", "brink_in"]
OUT_OF_RANGE = ["brink_out", "blown", "blown_coords"]
FAMILIES = IN_RANGE + OUT_OF_RANGE
SMALL = ["small_1e-4", "small_1e-6", "tiny_1e-10"]


def non_finite_rows():
    """three randn rows holding one NaN, one +inf, one -inf: data the kernels are specified for, asserted on only through their
    neighbours"""
    z = _rng("non_finite").standard_normal((3, 262)).astype(np.float32)
    z[0, 17], z[1, 140], z[2, 259] = np.nan, np.inf, -np.inf
    return z


@functools.lru_cache(maxsize=None)
def ref64(name, wname="trained"):
    return mlp64(weights(wname), family(name))


@functools.lru_cache(maxsize=None)
def noise(name, wname="trained"):
    return float(np.abs(mlp32(weights(wname), family(name)).astype(np.float64) - ref64(name, wname)).max())


def bar(name, wname="trained"):
    return 3.0 * noise(name, wname)


def take(name, n):
    """-> (row indices into the family, the n rows)"""
    idx = np.arange(n) % len(family(name))
    return idx, family(name)[idx]


# ------------------------------------------------------------------------------------------------------------------ the inputs (no GPU)
def test_families_are_what_they_claim():
    """Runs without a GPU.  Every family is finite, at least 128 rows, its noise positive; the in-range families' float64 hidden
    maxima stay below 0.9 x 65504 / 32 (brink_in: within 1e-3 of 0.97); brink_out within 1e-3 of 1.03, the blown families beyond
    the range; tiny_1e-10 below half an fp16 subnormal after scaling; the small families' bars below 1e-5, so that they can see
    the ~5e-5 a flush of fp16 subnormals would cost; the synthetic weight sets meant for the two-plane kernel keep the hidden
    maxima below 0.9 of the range on the rows they are run with, the w_flag sets exceed the packing guard in one weight."""
    w = weights()
    for name in FAMILIES:
        z = family(name)
        hm = mlp64(w, z, hidden=True)[1]
        print("family %-14s rows %3d  hidden max / limit %.4f .. %.4f  out max %.3g  noise %.3e  bar %.3e" % (
            name, len(z), hm.min() / LIM, hm.max() / LIM, np.abs(ref64(name)).max(), noise(name), bar(name)))
        assert z.dtype == np.float32 and z.shape[1] == 262 and len(z) >= 128 and np.isfinite(z).all(), name
        assert np.isfinite(ref64(name)).all() and noise(name) > 0, name
        if name == "brink_in":
            assert np.abs(hm / LIM - 0.97).max() < 1e-3
        elif name == "brink_out":
            assert np.abs(hm / LIM - 1.03).max() < 1e-3
        elif name in IN_RANGE:
            assert hm.max() < 0.9 * LIM, (name, hm.max())
        else:
            assert hm.max() > 1.001 * LIM, (name, hm.max())
    assert np.abs(family("tiny_1e-10")).max() * 32 < 2.0 ** -25
    assert ((family("path_like") == 0) & np.signbit(family("path_like"))).sum() > 1000
    for name in SMALL:
        assert bar(name) < 1e-5, (name, bar(name))
    nf = non_finite_rows()
    assert np.isnan(nf[0]).sum() == 1 and (nf[1] == np.inf).sum() == 1 and (nf[2] == -np.inf).sum() == 1
    for wname in WEIGHT_SETS_IN_RANGE:
        for name in ("unit", "small_1e-4"):
            hm = mlp64(weights(wname), family(name), hidden=True)[1]
            print("weights %-9s rows %-10s hidden max / limit %.4f  noise %.3e" % (wname, name, hm.max() / LIM, noise(name, wname)))
            assert hm.max() < 0.9 * LIM and noise(name, wname) > 0, (wname, name)
    assert all(np.abs(mats(weights("tiny_w"))[0][i]).max() * 256 < 2.0 ** -3 for i in range(4))   # the m planes: below 2^-14
    assert (mats(weights("sparse_w"))[0][0] == 0).mean() > 0.85 and np.signbit(mats(weights("sparse_w"))[0][0]).any()
    for wname, layer in (("w_flag_l1", 1), ("w_flag_l3", 3)):
        W = mats(weights(wname))[0][layer]
        assert (np.abs(W) > W_LIMIT).sum() == 1 and np.abs(W).max() * 256 < 65504      # flagged by the guard, still an fp16 number
        for name in ("unit", "small_1e-4"):
            assert noise(name, wname) > 0


# ------------------------------------------------------------------------------------------------------------------ GPU side
@pytest.fixture(scope="module")
def ops():
    from dvm import ops as _ops
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _ops


def run(ops, z, wname="trained"):
    wl = ops.deformer_weight_list(weights(wname), "cuda")
    return ops.deformer_mlp(wl, torch.from_numpy(np.ascontiguousarray(z)).cuda()).cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def judge(case, kernel, got, ref, bars, yard):
    """per-row max error against per-row bars; prints the figures, then asserts.  yard: the noise the ratio is quoted against"""
    with np.errstate(invalid="ignore"):
        err = np.abs(got.astype(np.float64) - ref).max(1)
    bars = np.broadcast_to(np.asarray(bars, np.float64), err.shape)
    worst = int(np.argmax(np.where(np.isnan(err), np.inf, err) / bars))
    print("MLPROWS %-34s %-9s noise %.3e  err %.3e  ratio %.3f  (rows %d, not finite %d)" % (
        case, kernel, yard, np.nanmax(err), np.nanmax(err) / yard, len(err), int((~np.isfinite(got)).any(1).sum())))
    assert np.isfinite(got).all(), "%s: %d rows not finite" % (case, int((~np.isfinite(got)).any(1).sum()))
    assert (err <= bars).all(), "%s: row %d off by %.3e, bar %.3e (%d of %d rows beyond their bar)" % (
        case, worst, err[worst], bars[worst], int((err > bars).sum()), len(err))


ALONE = [(f, n) for f in FAMILIES for n in (64, 200)] + [(f, BIG) for f in ("unit", "small_1e-4", "path_like")]


@gpu
@pytest.mark.parametrize("name,n", ALONE, ids=["%s-%d" % c for c in ALONE])
def test_family_alone(ops, name, n):
    """One family per launch at a block, three blocks and a bit, and (three families) more blocks than the chip walks at once.
    In-range families come from the two-plane kernel, the others from the fallback: the bar is the same.  Rows repeat cyclically
    in the long launches: a repeated row must also repeat bit for bit (same arithmetic in every block and workgroup)."""
    idx, z = take(name, n)
    got = run(ops, z)
    judge("%s/%d" % (name, n), "two-plane" if name in IN_RANGE else "fallback", got, ref64(name)[idx], bar(name), noise(name))
    assert np.array_equal(bits(got), bits(got[:len(family(name))][idx]))


@gpu
@pytest.mark.parametrize("name", FAMILIES)
def test_bf16x3_kernel_on_family(ops, name):
    """The bf16x3 kernel on chosen rows: one blown sentinel row appended raises the flag, the fallback then recomputes the whole
    launch, so the family's rows are that kernel's output.  Same bar.  (The sentinel coming back finite and within its own bar
    is the evidence that the fallback ran.)"""
    idx, z = take(name, 200)
    got = run(ops, np.concatenate([z, family("blown")[:1]]))
    judge("%s+sentinel" % name, "bf16x3", got[:200], ref64(name)[idx], bar(name), noise(name))
    judge("sentinel", "bf16x3", got[200:], ref64("blown")[:1], bar("blown"), noise("blown"))


def _stack(names):
    z = np.concatenate([family(f) for f in names])
    fam = np.concatenate([np.full(len(family(f)), i) for i, f in enumerate(names)])
    ref = np.concatenate([ref64(f) for f in names])
    bars = np.array([bar(f) for f in names])[fam]
    return z, fam, ref, bars


@gpu
def test_interleaved_in_range_rows_are_position_independent(ops):
    """A seeded shuffle of every in-range family in one launch (length not a multiple of 64; no fallback): each row within its own
    family's bar, and bit-identical to the same row in a launch of its family alone and at positions 0, 31, 32, 63, 64 and last
    of another launch.  The summation order is fixed and a row's output depends on no other row: a brink_in neighbour at 2e3, a
    zero row, or the next block's LDS-DMA landing early would show here, and no tolerance is involved."""
    z, fam, ref, bars = _stack(IN_RANGE)
    n = len(z)
    assert n % 64 != 0
    perm = _rng("interleave").permutation(n)
    got = run(ops, z[perm])
    judge("interleaved in-range", "two-plane", got, ref[perm], bars[perm], max(noise(f) for f in IN_RANGE))
    alone = np.concatenate([run(ops, family(f)) for f in IN_RANGE])
    same = (bits(got) == bits(alone[perm])).all(1)
    assert same.all(), "rows differ from their family-alone launch: %s" % sorted({IN_RANGE[i] for i in fam[perm][~same]})
    other = z[_rng("interleave2").permutation(n)]
    base = run(ops, other)
    pos = np.array([0, 31, 32, 63, 64, n - 1])
    keep = np.ones(n, bool)
    keep[pos] = False
    for i, f in enumerate(IN_RANGE):
        r = int(np.flatnonzero(fam == i)[5])
        o = other.copy()
        o[pos] = z[r]
        out = run(ops, o)
        assert (bits(out[pos]) == bits(alone[r])[None]).all(), "a %s row depends on its position" % f
        assert np.array_equal(bits(out[keep]), bits(base[keep])), "a %s row changes its neighbours" % f


@gpu
def test_interleaved_with_fallback_rows(ops):
    """The same shuffle with brink_out, blown, blown_coords and the three non-finite rows mixed in: the flag comes up and the
    bf16x3 kernel recomputes the launch.  Every finite row within its family's bar (none turns non-finite), two runs bit-identical
    on the finite rows.  What the poisoned rows return is not asserted."""
    names = IN_RANGE + OUT_OF_RANGE
    z, fam, ref, bars = _stack(names)
    nf = non_finite_rows()
    z = np.concatenate([z, nf])
    n = len(z)
    assert n % 64 != 0
    perm = _rng("interleave_fb").permutation(n)
    fin = perm < n - len(nf)
    got = run(ops, z[perm])
    judge("interleaved with fallback", "bf16x3", got[fin], ref[perm[fin]], bars[perm[fin]], max(noise(f) for f in names))
    again = run(ops, z[perm])
    assert np.array_equal(bits(got[fin]), bits(again[fin]))


@gpu
def test_fallback_launch_leaves_nothing_behind(ops):
    """One cached workspace: an in-range launch, a fallback launch of the same size, the first launch again.  First and third are
    bit-identical (the flag is cleared per launch, the gated packings and fp32 rows leave nothing the next launch reads), and the
    fallback launch's ordinary rows meet the unit bar."""
    idx, z = take("unit", 200)
    zb = z.copy()
    zb[:50] = family("blown")[:50]
    first = run(ops, z)
    mid = run(ops, zb)
    third = run(ops, z)
    judge("state: in-range launch", "two-plane", first, ref64("unit")[idx], bar("unit"), noise("unit"))
    judge("state: ordinary rows of fallback", "bf16x3", mid[50:], ref64("unit")[idx][50:], bar("unit"), noise("unit"))
    judge("state: blown rows of fallback", "bf16x3", mid[:50], ref64("blown")[:50], bar("blown"), noise("blown"))
    assert np.array_equal(bits(first), bits(third))
    assert not np.array_equal(bits(first[50:]), bits(mid[50:]))     # (the two kernels differ in the last bits: a stuck flag would show above)


@gpu
@pytest.mark.parametrize("name", ["unit", "small_1e-4"])
@pytest.mark.parametrize("wname", WEIGHT_SETS_IN_RANGE)
def test_synthetic_weights(ops, wname, name):
    """Seeded weight sets of the decoder's shapes on the two-plane kernel and (sentinel row) on bf16x3, at the bar computed with
    those weights.  The float64 hidden maxima stay below 0.9 of the range, so the two-plane kernel is the one that answers."""
    w = weights(wname)
    idx, z = take(name, 200)
    ref, hm = mlp64(w, z, hidden=True)
    assert hm.max() < 0.9 * LIM
    judge("%s %s" % (wname, name), "two-plane", run(ops, z, wname), ref, bar(name, wname), noise(name, wname))
    got = run(ops, np.concatenate([z, family("blown")[:1]]), wname)
    judge("%s %s+sentinel" % (wname, name), "bf16x3", got[:200], ref, bar(name, wname), noise(name, wname))


@gpu
@pytest.mark.parametrize("name", ["unit", "small_1e-4"])
@pytest.mark.parametrize("wname", ["w_flag_l1", "w_flag_l3"])
def test_weight_flag_takes_the_fallback(ops, wname, name):
    """One weight of 250 (256 x 250 = 64000 is still an fp16 number, so the two-plane result would be finite): the packing kernel's
    guard must raise the flag.  The rows then are the bf16x3 kernel's — bit-identical to the same rows of a launch that a blown
    sentinel sends there — and within the bar of those weights.  The trained set afterwards, in the same workspace, gives the
    bits it gave before."""
    idx, z = take(name, 200)
    before = run(ops, z)
    got = run(ops, z, wname)
    judge("%s %s" % (wname, name), "bf16x3", got, mlp64(weights(wname), z), bar(name, wname), noise(name, wname))
    forced = run(ops, np.concatenate([z, family("blown")[:1]]), wname)[:200]
    assert np.array_equal(bits(got), bits(forced)), "the weight guard did not send the launch to the fallback"
    assert np.array_equal(bits(run(ops, z)), bits(before))


# ------------------------------------------------------------------------------------------------------------------ the fused producers
def deformer_ref(w, a, dt):
    """The four lines at the top of csrc/dvm_deformer.hip in numpy at precision dt: pool (1x1 conv over the k neighbours), transfer
    (sparse Pi @ g2 over the top-k slots as they stand: a repeated column adds twice, a zero-weight slot adds nothing), row, MLP."""
    cw = np.asarray(w["conv_layer__weight"], np.float32).reshape(-1).astype(dt)
    cb = dt(np.asarray(w["conv_layer__bias"], np.float32).reshape(-1)[0])
    outs = []
    for b in range(a["feat1"].shape[0]):
        f1, f2 = a["feat1"][b].astype(dt), a["feat2"][b].astype(dt)
        g1, g2 = np.zeros_like(f1), np.zeros_like(f2)
        for s in range(len(cw)):
            g1 = (g1 + cw[s] * f1[a["idx11"][b][:, s]]).astype(dt)
            g2 = (g2 + cw[s] * f2[a["idx22"][b][:, s]]).astype(dt)
        g1, g2 = (g1 + cb).astype(dt), (g2 + cb).astype(dt)
        gx = np.zeros_like(f1)
        for t in range(a["pi_val"].shape[2]):
            gx = (gx + a["pi_val"][b][:, t, None].astype(dt) * g2[a["pi_idx"][b][:, t]]).astype(dt)
        v = a["fps1"][b]
        outs.append(np.concatenate([a["verts1"][b][v].astype(dt), g1[v], a["verts12"][b][v].astype(dt), gx[v]], 1))
    z = np.concatenate(outs)
    return mlp32(w, z) if dt is np.float32 else chain64(w, z)


def deformer_inputs(case):
    """small      features 1e-4 randn, coordinates 1e-4 rand, conv bias 0: pooled rows as small as small_1e-4 (m planes subnormal)
    path_like  0.3 relu(randn) features, unit-box coordinates
    coords3000 path_like with coordinates x 3000: the plane rows overflow, the fp32 rows and bf16x3 answer
    repeat     path_like whose top-k rows hold repeated columns (a third of the rows: one column twice; a third: one column in all
               ten slots)
    Neighbour lists, graph nodes and the sparse map are seeded random index arrays (any indices in range are valid input)."""
    g = _rng("deformer_" + case)
    B, N, M, Nn = 2, 300, 200, 150
    if case == "small":
        f1, f2 = 1e-4 * g.standard_normal((B, N, 128)), 1e-4 * g.standard_normal((B, M, 128))
        v1, v12 = 1e-4 * g.random((B, N, 3)), 1e-4 * g.random((B, N, 3))
    else:
        f1, f2 = 0.3 * np.maximum(g.standard_normal((B, N, 128)), 0), 0.3 * np.maximum(g.standard_normal((B, M, 128)), 0)
        v1, v12 = g.random((B, N, 3)), g.random((B, N, 3))
    if case == "coords3000":
        v1, v12 = 3000.0 * v1, 3000.0 * v12
    pi_idx = np.argsort(g.random((B, N, M)), axis=2)[:, :, :10]
    pi_val = g.random((B, N, 10)) ** 4
    pi_val /= pi_val.sum(2, keepdims=True) * g.uniform(1.0, 1.5, (B, N, 1))
    if case == "repeat":
        pi_idx[:, 0::3, 7] = pi_idx[:, 0::3, 2]
        pi_idx[:, 1::3, :] = pi_idx[:, 1::3, :1]
    a = dict(feat1=f1, feat2=f2, verts1=v1, verts12=v12, pi_val=pi_val)
    a = {k: np.ascontiguousarray(v, np.float32) for k, v in a.items()}
    a.update(idx11=g.integers(0, N, (B, N, 10)).astype(np.int32), idx22=g.integers(0, M, (B, M, 10)).astype(np.int32),
             pi_idx=np.ascontiguousarray(pi_idx, np.int32),
             fps1=np.stack([g.permutation(N)[:Nn] for _ in range(B)]).astype(np.int32))
    return a


def run_deformer(ops, wname, a, variant):
    wl = ops.deformer_weight_list(weights(wname), "cuda")
    d = {k: torch.from_numpy(v).cuda() for k, v in a.items()}
    out = ops.deformer(wl, d["feat1"], d["feat2"], d["verts1"], d["verts12"], d["idx11"], d["idx22"], d["pi_val"], d["pi_idx"], d["fps1"],
                       variant=variant)
    return out.cpu().numpy().reshape(-1, 9)


@gpu
@pytest.mark.parametrize("variant", [0, 1, 2, 3])
@pytest.mark.parametrize("case", ["small", "path_like", "coords3000", "repeat"])
def test_deformer_rows_against_float64(ops, case, variant):
    """ops.deformer (pool, transfer, row assembly, split_rows_kernel, MLP; variant 1 the scalar chain, 2 fp32 MFMA, 3 bf16x3)
    against the float64 restatement of the whole entry, every row within 3 x the float32 twin's error over the launch's rows."""
    wname = "conv_b0" if case == "small" else "trained"
    a = deformer_inputs(case)
    ref = deformer_ref(weights(wname), a, np.float64)
    yard = float(np.abs(deformer_ref(weights(wname), a, np.float32).astype(np.float64) - ref).max())
    assert yard > 0 and (case != "small" or 3 * yard < 1e-5)
    judge("deformer %s" % case, "variant %d" % variant, run_deformer(ops, wname, a, variant), ref, 3 * yard, yard)


@gpu
def test_deformer_short_topk_rows(ops):
    """M < 10: ops.softcorr leaves three of the ten slots unused; whatever it writes there (weights of zero on valid columns) goes
    through the transfer unchanged.  Variant 0 and the scalar chain against the float64 restatement."""
    g = _rng("deformer_M7")
    B, N, M, Nn = 2, 300, 7, 150
    f1, f2 = 0.3 * np.maximum(g.standard_normal((B, N, 128)), 0), 0.3 * np.maximum(g.standard_normal((B, M, 128)), 0)
    a = dict(feat1=f1, feat2=f2, verts1=g.random((B, N, 3)), verts12=g.random((B, N, 3)))
    a = {k: np.ascontiguousarray(v, np.float32) for k, v in a.items()}
    val, idx, _, _ = ops.softcorr(torch.from_numpy(a["feat1"]).cuda(), torch.from_numpy(a["feat2"]).cuda(), 20.0)
    a.update(pi_val=val.cpu().numpy(), pi_idx=idx.cpu().numpy(), idx11=g.integers(0, N, (B, N, 10)).astype(np.int32),
             idx22=g.integers(0, M, (B, M, 10)).astype(np.int32), fps1=np.stack([g.permutation(N)[:Nn] for _ in range(B)]).astype(np.int32))
    assert a["pi_idx"].min() >= 0 and a["pi_idx"].max() < M and np.isfinite(a["pi_val"]).all()
    assert ((a["pi_val"] == 0).sum(2) >= 3).all()
    ref = deformer_ref(weights(), a, np.float64)
    yard = float(np.abs(deformer_ref(weights(), a, np.float32).astype(np.float64) - ref).max())
    assert yard > 0
    for variant in (0, 1):
        judge("deformer M=7", "variant %d" % variant, run_deformer(ops, "trained", a, variant), ref, 3 * yard, yard)


@gpu
def test_pair_entries_under_the_gate_against_oracle(ops):
    """Coordinates x 3000 through ops.pair_direction and ops.pair_forward: the plane rows (assemble_pooled_kernel<10, true>)
    overflow, the rows are re-assembled as floats under the gate and the bf16x3 kernel answers.  Against the C oracle: the hard
    map bit for bit, verts12 and warped at the parity suite's bars (1e-5, 1e-4) scaled by the clouds' largest |coordinate| — a
    bar carried over from tests/test_gpu_parity.py::test_pair_direction_vs_oracle, not measured from a float64 warp."""
    from oracle import oracle as O
    B, N, M = 2, 330, 330
    g = torch.Generator().manual_seed(77)
    f1 = 0.3 * torch.relu(torch.randn(B, N, 128, generator=g))
    f2 = 0.3 * torch.relu(torch.randn(B, M, 128, generator=g))
    v1, v2 = 3000.0 * torch.rand(B, N, 3, generator=g), 3000.0 * torch.rand(B, M, 3, generator=g)
    s1 = torch.randint(0, N, (B,), generator=g).int()
    s2 = torch.randint(0, M, (B,), generator=g).int()
    w = weights()
    wl = ops.deformer_weight_list(w, "cuda")
    d = [t.cuda() for t in (f1, f2, v1, v2)]
    o12, o21 = ops.pair_forward(wl, *d, 33.0, s1.cuda(), s2.cuda())
    r12 = ops.pair_direction(wl, d[0], d[1], d[2], d[3], 33.0, s1.cuda())
    scale = float(max(v1.abs().max(), v2.abs().max()))
    for b in range(B):
        o = O.pair_direction(w, f1[b].numpy(), f2[b].numpy(), v1[b].numpy(), v2[b].numpy(), 33.0, int(s1[b]))
        p = O.pair_direction(w, f2[b].numpy(), f1[b].numpy(), v2[b].numpy(), v1[b].numpy(), 33.0, int(s2[b]))
        for tag, got, want in (("pair_direction 12", r12, o), ("pair_forward 12", o12, o), ("pair_forward 21", o21, p)):
            e12 = np.abs(got["verts12"][b].cpu().numpy() - want["verts12"]).max()
            ew = np.abs(got["warped"][b].cpu().numpy() - want["warped"]).max()
            print("MLPROWS %-34s %-9s verts12 err %.3e (bar %.3e)  warped err %.3e (bar %.3e)" % (
                "%s b=%d coords x 3000" % (tag, b), "bf16x3", e12, 1e-5 * scale, ew, 1e-4 * scale))
            assert np.array_equal(got["T12"][b].cpu().numpy(), want["T12"]), tag
            assert e12 < 1e-5 * scale and ew < 1e-4 * scale, tag
