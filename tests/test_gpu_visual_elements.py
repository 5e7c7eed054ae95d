"""-m gpu: the visual-injection kernels of csrc/dvm_proj.hip judged per pixel / per element at their tile edges (references, bars with
their derivations, input families and the comparisons themselves: tests/visual_ref.py; the same comparisons on fp32 restatements and
on planted mutations of them, and the caps on the references alone: tests/test_visual_ref_cpu.py; measured ratios:
profiles/notes_visual_tests.md).

render     ops.proj2img, B = 3 clouds per family against oracle/torch_ref.py::proj2img: parameters and empty-pixel mask bit for bit, the
           colour code exact on every decided pixel, one bin elsewhere; bit-equal under a permutation of the points
i2p        ops.i2p at every pixel class (36 border combinations, 260 interior pixels, two parameter sets) x 8 feature sizes x C in
           {1, 63, 64, 65, 130 (, 384)}: per-element bar; bit equality at the dyadic sizes and on the identity route; normalize with all-zero
           rows; the out= / col form
resize     ops.bicubic_resize_pad: x2 at pads {0, 1, 2, 3, 5} bit-equal on integers, per-element bar on real inputs and general scales
aconv      ops.adaptive_conv, d = 7 route and generic route, both kernel layouts: bit-equal on integers, bar d d u sum|in k| on real inputs
jbu        ops.jbu_kernel on peaked exact logits at both temperature clamps and temp 1, sigma in {1, 0.8, 0.05, 0.02}, and on random guidance"""
import numpy as np
import pytest
import torch

import visual_ref as V

pytestmark = pytest.mark.gpu


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _render(pts):
    from dvm import ops
    img, mn, grid, off = ops.proj2img(_t(pts))
    assert img.shape == (pts.shape[0], 3, 224, 224)
    return V.codes(img), mn.cpu().numpy(), grid.cpu().numpy(), off.cpu().numpy()


def _i2p(pts, f, mn, grid, off, normalize):
    from dvm import ops
    return ops.i2p(_t(pts), _t(f), _t(mn), _t(grid), _t(off), normalize=normalize).cpu().numpy()


def _resize(x, size, pad):
    from dvm import ops
    return ops.bicubic_resize_pad(_t(x), size, pad).cpu().numpy()


def _aconv(x, k, tap_major):
    from dvm import ops
    kt = _t(k)
    if tap_major:
        B, H, W, d, _ = k.shape
        kt = kt.reshape(B, H, W, d * d).permute(0, 3, 1, 2).contiguous()
    return ops.adaptive_conv(_t(x), kt, tap_major=tap_major).cpu().numpy()


def _jbu(p, range_temp, sigma):
    from dvm import ops
    return ops.jbu_kernel(_t(p), torch.tensor(range_temp, dtype=torch.float32).cuda(), torch.tensor(sigma, dtype=torch.float32).cuda()).cpu().numpy()


@pytest.mark.parametrize("family", V.RENDER_FAMILIES)
def test_render_per_pixel(family):
    V.render_check(family, _render)
    got = _render(V.render_oracle(family)["pts"])[0]
    for b, cl in enumerate(V.render_oracle(family)["cls"]):
        und = cl["nonempty"] & ~cl["decided"]
        print("RATIO gpu render %s[%d]: %d undecided pixels, %d of them one bin off the oracle" % (
            family, b, int(und.sum()), int((got[b] != V.render_oracle(family)["codes"][b])[und].sum())))


@pytest.mark.parametrize("size", V.I2P_SIZES)
def test_i2p_per_element(size):
    for C in V.i2p_channels(size):
        print("RATIO gpu i2p %s C=%d %.3f" % (size, C, V.i2p_check(size, C, _i2p)))


def test_i2p_out_col_form():
    """columns [col, col + C) of a (B,N,ldo) tensor; every other column keeps its sentinel bit for bit"""
    from dvm import ops
    pts, mn, grid, off, pix = V.i2p_points()
    B, N = pts.shape[:2]
    for size, C, ldo in (((37, 70), 65, 200), ((32, 32), 130, 137), ((224, 224), 64, 71)):
        f = V.i2p_features(size, C, "real")
        for normalize in (False, True):
            want = _i2p(pts, f, mn, grid, off, normalize)
            for col in (0, 7, ldo - C):
                sentinel = torch.full((B, N, ldo), -1234.5, dtype=torch.float32).cuda()
                out = ops.i2p(_t(pts), _t(f), _t(mn), _t(grid), _t(off), normalize=normalize, out=sentinel, col=col)
                assert out is sentinel
                out = out.cpu().numpy()
                assert np.array_equal(out[:, :, col:col + C], want), (size, C, ldo, col, normalize)
                keep = np.ones(ldo, bool)
                keep[col:col + C] = False
                assert np.all(out[:, :, keep] == np.float32(-1234.5)), (size, C, ldo, col, normalize)


@pytest.mark.parametrize("src", V.RESIZE_X2_SIZES)
def test_resize_x2_per_element(src):
    worst = 0.0
    for pad in V.RESIZE_X2_PADS:
        if pad < 2 * src[0] and pad < 2 * src[1]:
            for kind in ("int", "real"):
                worst = max(worst, V.resize_check(src, (2 * src[0], 2 * src[1]), pad, kind, _resize))
    print("RATIO gpu resize x2 %s %.3f" % (src, worst))


@pytest.mark.parametrize("src,dst", V.RESIZE_GENERAL)
def test_resize_general_per_element(src, dst):
    for pad in V.RESIZE_GENERAL_PADS:
        print("RATIO gpu resize %s -> %s pad %d %.3f" % (src, dst, pad, V.resize_check(src, dst, pad, "real", _resize)))


@pytest.mark.parametrize("shape", V.ACONV7_SHAPES)
def test_aconv7_per_element(shape):
    worst = 0.0
    for C in V.aconv7_channels(shape):
        for B in (1, 3):
            for tm in (False, True):
                worst = max(worst, V.aconv_check(B, C, shape[0], shape[1], 7, tm, _aconv))
    print("RATIO gpu adaptive_conv7 %s %.3f" % (shape, worst))


@pytest.mark.parametrize("shape", V.ACONV_GENERIC_SHAPES)
def test_aconv_generic_per_element(shape):
    for d in V.ACONV_GENERIC_D:
        worst = 0.0
        for C in V.ACONV_GENERIC_CHANNELS:
            for tm in (False, True):
                worst = max(worst, V.aconv_check(2, C, shape[0], shape[1], d, tm, _aconv))
        print("RATIO gpu adaptive_conv %s d=%d %.3f" % (shape, d, worst))


@pytest.mark.parametrize("shape", V.JBU_SHAPES)
def test_jbu_per_element(shape):
    for rt in V.JBU_TEMPS:
        for sg in V.JBU_SIGMAS:
            print("RATIO gpu jbu %s temp %g sigma %g peaked %.3f" % (shape, rt, sg, V.jbu_check(shape, rt, sg, "peaked", _jbu)))
    print("RATIO gpu jbu %s random %.3f" % (shape, V.jbu_check(shape, 0.7, 0.8, "random", _jbu)))
