"""CPU half of the per-element checks of the visual-injection kernels (device half: tests/test_gpu_visual_elements.py; references, bars,
families, restatements and the comparisons themselves: tests/visual_ref.py).  It proves without a GPU that the device tests can fail, and
only for a reason:

(1) the float64 references agree with torch's own CPU operators: F.interpolate(bicubic), F.pad(reflect), F.unfold,
    JBULearnedRange.combined_kernel_torch in float64 on an identity range_proj, oracle/torch_ref.py::i2p in float64; the render is compared
    with oracle/torch_ref.py::proj2img itself, and its float64 restatement reproduces the oracle's code on every decided pixel;
(2) the fp32 restatements pass every comparison of the device half at HALF the bar (bit equality where the device half asks for it); the
    one exception is the adaptive convolution at d = 1, where the bar d d u |in k| is the rounding of the single product itself;
(3) every planted mutation of a restatement fails the comparison the device half makes, on at least one of its cases;
(4) the stated caps hold on the reference alone: undecided pixels <= 2 % of the non-empty pixels of each rendered image; the lattice family
    has >= 100 points whose fp32 quotient is within an ulp below an integer and >= 100 at or within an ulp above one; the cancellation
    family's pairs render as background inside a coloured silhouette and its pairs off by 2^-20 do not; the planted JBU pixels are there.

Two render defects one would list first change no value, on any input, and are pinned as such instead (test_render_neutral_mutations):
 * "shift without clamp" -- the pre-shift pixel index lies in [-1, 224] by construction of the offsets (the cell index is in [0, 221], the
   footprint adds -2 .. 2, then + 1 and a centring offset that is 0 on the long axis), so after the shift the clamp is unreachable; for the
   same reason the clamp alone would equal the shift.  What differs is a splat that neither shifts nor clamps but guards its store: `no_shift`.
 * "5 x 5 offsets transposed" -- the footprint is the full square, the same set of 25 pixels either way.  What differs is the image
   transposed (`pixel_transposed`: row and column swapped in the pixel index)."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import visual_ref as V
from oracle import torch_ref


def _caught(run, cases):
    """the mutation is caught if the comparison fails on at least one case"""
    for c in cases:
        try:
            run(*c)
        except AssertionError:
            return True
    return False


# ======================================================================================================================= render
@pytest.mark.parametrize("family", V.RENDER_FAMILIES)
def test_render_restatement_and_cap(family):
    ora = V.render_oracle(family)
    assert ora["pts"].shape[0] == 3 and ora["pts"].shape[1] <= 2048
    V.render_check(family, V.proj2img_np)
    for b, cl in enumerate(ora["cls"]):
        print("RATIO render %s[%d] undecided share %.5f of %d non-empty" % (family, b, cl["share"], int(cl["nonempty"].sum())))
        assert cl["share"] <= V.CAP_UNDECIDED, (family, b, cl["share"])
        assert np.array_equal(cl["nonempty"], ora["codes"][b] != 256)
        agree = cl["code64"] == ora["codes"][b]
        assert agree[cl["decided"]].all() and np.abs(cl["code64"] - ora["codes"][b]).max() <= 1
        if family != "zero":
            assert cl["nonempty"].sum() >= 200
        else:
            assert not cl["nonempty"].any()


def test_render_families_hit_their_targets():
    # collisions: at most 144 cells
    for p in V.render_family("collisions"):
        assert len({tuple(i) for i in V.render_params(p)["idx"].tolist()}) <= 144 and np.all(p[:, 2] * 64 == np.rint(p[:, 2] * 64))
    # cancellation: pairs are background inside a coloured footprint's reach; pairs off by 2^-20 are coloured
    ora = V.render_oracle("cancellation")
    for b in range(3):
        pair, off = V.cancellation_pixels(b)
        c = ora["codes"][b]
        for dr in range(-2, 3):
            for dc in range(-2, 3):
                assert (c[pair[:, 0] + dr, pair[:, 1] + dc] == 256).all() and (c[off[:, 0] + dr, off[:, 1] + dc] != 256).all()
        assert (ora["cls"][b]["contrib"][pair[:, 0], pair[:, 1]] == 2).all()
    # borders / flat: pre-shift indices -1 and 224 both occur, on either axis over the family; three aspect ratios; ry = 0
    seen = set()
    for fam in ("borders", "flat"):
        for b, p in enumerate(V.render_family(fam)):
            q = V.render_params(p)
            px, py = V.render_pixels(q)[3]
            seen |= {("x", int(px.min())), ("x", int(px.max())), ("y", int(py.min())), ("y", int(py.max()))}
            assert px.min() >= -1 and px.max() <= 224 and py.min() >= -1 and py.max() <= 224
            r = p[:, :2].max(0) - p[:, :2].min(0)
            assert (r[0] > r[1], r[1] > r[0], r[0] == r[1])[b] or fam == "flat"
            if fam == "flat":
                assert r.min() == 0
    assert {("x", -1), ("x", 224), ("y", -1), ("y", 224)} <= seen
    # lattice: quotients within an ulp of an integer, on both sides
    below = above = 0
    for p in V.render_family("lattice"):
        q = V.render_params(p)
        for a in range(2):
            lo, hi = V.lattice_near_integer(p[:, a], q["mn"][a], q["grid"])
            below, above = below + lo, above + hi
        assert np.all(p[:, 2] * 256 == np.rint(p[:, 2] * 256))
    assert below >= 100 and above >= 100, (below, above)
    # exponent: below its cap with max|z| = 2^13, at its cap with max|z| = 2^-20
    ex = V.render_family("exponent")
    assert [V.render_params(p)["e"] for p in ex] == [32, 40, 32] and [float(np.abs(p[:, 2]).max()) for p in ex] == [2.0 ** 13, 2.0 ** -20, 2.0 ** 13]
    assert not V.render_family("zero")[:, :, 2].any()


@pytest.mark.parametrize("mut", V.RENDER_MUTATIONS)
def test_render_mutation_is_caught(mut):
    assert _caught(lambda fam: V.render_check(fam, lambda p: V.proj2img_np(p, mut)), [(f,) for f in V.RENDER_FAMILIES])


@pytest.mark.parametrize("mut", V.RENDER_NEUTRAL)
def test_render_neutral_mutations(mut):
    """see the module docstring: these two change no value; `shift_no_clamp` also asserts that no index leaves the image unclamped"""
    for fam in V.RENDER_FAMILIES:
        pts = V.render_family(fam)
        for a, b in zip(V.proj2img_np(pts), V.proj2img_np(pts, mut)):
            assert np.array_equal(a, b)


# ============================================================================================================== back-projection
def _i2p_np(mut=None):
    return lambda pts, f, mn, grid, off, normalize: V.i2p_np(pts, f, mn, grid, off, normalize, mut)


def test_i2p_points_cover_every_pixel_class():
    pts, mn, grid, off, pix = V.i2p_points()
    assert pts.shape[1] <= 1024
    for b in range(2):
        have = {tuple(p) for p in pix[b].tolist()}
        assert {(r, c) for r in V._EDGE for c in V._EDGE} <= have
        assert sum(1 for r, c in have if 3 <= r <= 220 and 3 <= c <= 220) >= 200


@pytest.mark.parametrize("size", [s for s in V.I2P_SIZES])
def test_i2p_reference_is_torch_float64(size):
    pts, mn, grid, off, pix = V.i2p_points()
    f = V.i2p_features(size, 5, "real")
    want = torch_ref.i2p(torch.from_numpy(pts).double(), torch.from_numpy(f).double(), torch.from_numpy(mn).double().view(2, 1, 2),
                         torch.from_numpy(grid).double().view(2, 1, 1), (torch.from_numpy(off[:, :1]).double(), torch.from_numpy(off[:, 1:]).double()))
    ref, bar = V.i2p_reference(f, pix)
    scale = np.abs(f).max()
    assert np.abs(ref - want.numpy()).max() <= 1e-12 * scale
    refn, _ = V.i2p_reference(f, pix, True)
    assert np.abs(refn - F.normalize(want, dim=-1).numpy()).max() <= 1e-12


@pytest.mark.parametrize("size", V.I2P_SIZES)
def test_i2p_restatement_within_half_bar(size):
    for C in V.i2p_channels(size):
        print("RATIO i2p %s C=%d emulation %.3f" % (size, C, V.i2p_check(size, C, _i2p_np(), 0.5)))


def test_i2p_exact_weights():
    """at 448 the sample offsets are 1/2, at 112 they are 1/4 and 3/4: fp32 forms the weights exactly, as multiples of 1/256"""
    for t in (0.25, 0.5, 0.75):
        c32, c64 = V._cubic32(np.float32(t)), V._cubic64(t)[0]
        assert np.array_equal(c32.astype(np.float64), c64) and np.all(c64 * 256 == np.rint(c64 * 256))


@pytest.mark.parametrize("mut", V.I2P_MUTATIONS)
def test_i2p_mutation_is_caught(mut):
    assert _caught(lambda size, C: V.i2p_check(size, C, _i2p_np(mut)), [(s, C) for s in ((37, 70), (32, 32), (448, 448), (224, 224)) for C in (65, 130)])


# ========================================================================================================================= resize
def _resize_cases():
    out = []
    for (Hi, Wi) in V.RESIZE_X2_SIZES:
        for pad in V.RESIZE_X2_PADS:
            if pad < 2 * Hi and pad < 2 * Wi:
                out.append(((Hi, Wi), (2 * Hi, 2 * Wi), pad, "int"))
                out.append(((Hi, Wi), (2 * Hi, 2 * Wi), pad, "real"))
    for src, dst in V.RESIZE_GENERAL:
        out += [(src, dst, pad, "real") for pad in V.RESIZE_GENERAL_PADS]
    return out


def test_resize_reference_is_torch_float64():
    for src, dst, pad, kind in _resize_cases():
        x = V.resize_input(src[0], src[1], kind)
        want = F.interpolate(torch.from_numpy(x).double(), size=dst, mode="bicubic", align_corners=False)
        if pad:
            want = F.pad(want, [pad] * 4, mode="reflect")
        ref, _ = V.resize_reference(x, dst, pad)
        assert ref.shape == tuple(want.shape) and np.abs(ref - want.numpy()).max() <= 1e-12 * np.abs(x).max(), (src, dst, pad)


def test_resize_restatement_within_half_bar():
    worst = 0.0
    for c in _resize_cases():
        worst = max(worst, V.resize_check(*c, V.resize_np, 0.5))
    print("RATIO resize emulation %.3f" % worst)


@pytest.mark.parametrize("mut", V.RESIZE_MUTATIONS)
def test_resize_mutation_is_caught(mut):
    assert _caught(lambda *c: V.resize_check(*c, lambda x, size, pad: V.resize_np(x, size, pad, mut)), _resize_cases())


# ============================================================================================================ adaptive convolution
def _aconv_cases():
    out = [(B, C, H, W, 7) for (H, W) in V.ACONV7_SHAPES for C in V.aconv7_channels((H, W)) for B in (1, 3)]
    return out + [(2, C, H, W, d) for (H, W) in V.ACONV_GENERIC_SHAPES for d in V.ACONV_GENERIC_D for C in V.ACONV_GENERIC_CHANNELS]


def test_aconv_reference_is_unfold_float64():
    for (B, C, H, W, d) in [(3, 5, 17, 33, 7), (2, 9, 5, 130, 15), (1, 1, 1, 1, 7), (2, 5, 3, 63, 1)]:
        x, k = V.aconv_inputs(B, C, H, W, d, "real")
        win = F.unfold(torch.from_numpy(x).double(), d).view(B, C, d * d, H, W)
        want = (win * torch.from_numpy(k).double().reshape(B, 1, H, W, d * d).permute(0, 1, 4, 2, 3)).sum(2)
        ref, bar = V.aconv_reference(x, k)
        assert np.abs(ref - want.numpy()).max() <= 1e-13 * (np.abs(x).max() * np.abs(k).max() * d * d)


def test_aconv7_split_table_has_the_partial_chunks():
    """the shapes reach a channel slice that is no multiple of the 4-channel chunk, a split, and an odd height"""
    tab = {(B, C, H, W): V.aconv7_split(B, C, H, W) for (B, C, H, W, d) in _aconv_cases() if d == 7}
    assert tab[(1, 384, 32, 32)] == (64, 6) and tab[(3, 384, 32, 32)] == (64, 6)
    assert any(cs > 1 and cper % 4 for cs, cper in tab.values()) and any(H % 2 for (_, _, H, _) in tab)


def test_aconv_restatement_within_half_bar():
    worst = [0.0, 0.0]
    for c in _aconv_cases():
        for tm in (False, True):
            r = V.aconv_check(*c, tm, V.aconv_np, 0.5 if c[4] > 1 else 1.0)
            worst[c[4] > 1] = max(worst[c[4] > 1], r)
    print("RATIO adaptive_conv emulation d=1 %.3f, d>1 %.3f" % tuple(worst))


@pytest.mark.parametrize("mut", V.ACONV_MUTATIONS)
def test_aconv_mutation_is_caught(mut):
    cases = [(1, 22, 17, 33, 7, False), (3, 5, 2, 31, 7, False), (1, 384, 32, 32, 7, True)]
    assert _caught(lambda *c: V.aconv_check(*c, lambda x, k, tm: V.aconv_np(x, k, tm, mut)), cases)


# ===================================================================================================================== JBU kernel
def _jbu_cases():
    out = [(s, rt, sg, "peaked") for s in V.JBU_SHAPES for rt in V.JBU_TEMPS for sg in V.JBU_SIGMAS]
    return out + [(s, 0.7, 0.8, "random") for s in V.JBU_SHAPES]


@functools.lru_cache(maxsize=None)
def _jbu_module():
    from models.image_backbone import JBULearnedRange
    jbu = JBULearnedRange(3, 16, 32, radius=3).double().eval()
    jbu.range_proj = torch.nn.Identity()
    return jbu


def test_jbu_reference_is_combined_kernel_torch_float64():
    jbu = _jbu_module()
    for (shape, rt, sg, kind) in _jbu_cases():
        p = V.jbu_proj(shape[0], shape[1], kind)
        torch.set_default_dtype(torch.float64)                        # the module's linspace of tap coordinates takes the default dtype
        try:
            want = _jbu_torch(jbu, p, rt, sg)
        finally:
            torch.set_default_dtype(torch.float32)
        ref, bar = V.jbu_reference(p, rt, sg, kind == "peaked")
        assert ref.shape == want.shape and np.all(np.abs(ref - want) <= 1e-7 * np.abs(want) + 1e-300), (shape, rt, sg, kind)


def _jbu_torch(jbu, p, rt, sg):
    with torch.no_grad():
        # the module holds temp and sigma in float64: hand it the fp32 values the kernel works with (exp(log t) = t (1 +- 2e-16), times
        # logits up to 4e7 at the upper clamp: hence 1e-7 and not 1e-12)
        jbu.range_temp.fill_(float(np.log(np.float64(V.jbu_temp(rt)))))
        jbu.sigma_spatial.fill_(float(np.float32(sg)))
        return jbu.combined_kernel_torch(torch.from_numpy(p).double()).numpy()


def test_jbu_plants_are_there():
    """at temp 1 and sigma 1 the two larger maps hold pixels whose whole kernel sits on the centre tap, on each corner tap, and split evenly
    between two taps; at sigma 0.05 a pair next to the centre falls under the 1e-7 floor with a non-zero value, a corner peak far below the fp32 range;
    every logit gap of a planted pixel exceeds 104"""
    for shape in ((8, 33), (9, 41)):
        ref, _ = V.jbu_reference(V.jbu_proj(shape[0], shape[1], "peaked"), 0.0, 1.0, True)
        ref = ref.transpose(0, 2, 3, 1).reshape(-1, 49)
        one = ref[(ref.max(1) > 1 - 1e-12)].argmax(1)
        assert {24, 0, 6, 42, 48} <= set(one.tolist()), set(one.tolist())
        two = np.sort(np.argsort(ref[np.abs(np.sort(ref, 1)[:, -2:] - 0.5).max(1) < 0.2], 1)[:, -2:], 1)
        assert {(23, 25), (17, 31)} <= {tuple(t) for t in two.tolist()}, two
        low, _ = V.jbu_reference(V.jbu_proj(shape[0], shape[1], "peaked"), 0.0, 0.05, True)
        low = low.transpose(0, 2, 3, 1).reshape(-1, 49)
        assert np.any((low.sum(1) > 1e-4) & (low.sum(1) < 1e-2)) and np.any(low.sum(1) < 1e-100)
        r = (np.float32(-1) + np.float32(2) * np.arange(7, dtype=np.float32) / np.float32(6)) ** 2
        with np.errstate(under="ignore"):
            g = np.exp(-(r[:, None] + r[None, :]) * (np.float32(1) / (np.float32(2) * np.float32(0.02) * np.float32(0.02)))).astype(np.float32)
        assert g[3, 3] == 1 and np.count_nonzero(g) == 1               # sigma 0.02: every off-centre spatial weight underflows in fp32
        p = V.jbu_proj(shape[0], shape[1], "peaked").astype(np.float64)
        l = np.sort((p[:, :, None, None] * V._jbu_windows(p)).sum(1).reshape(2, 49, -1), 1)
        assert ((l[:, -1] - l[:, 0] > 104).sum()) >= len(V.JBU_PLANTS)


def test_jbu_restatement_within_half_bar():
    worst = {}
    for c in _jbu_cases():
        worst[c[3]] = max(worst.get(c[3], 0.0), V.jbu_check(*c, V.jbu_np, 0.5))
    print("RATIO jbu emulation %r" % worst)


@pytest.mark.parametrize("mut", V.JBU_MUTATIONS)
def test_jbu_mutation_is_caught(mut):
    assert _caught(lambda *c: V.jbu_check(*c, lambda p, rt, sg: V.jbu_np(p, rt, sg, mut)), _jbu_cases())
