"""References, per-element bars, hard input families and fp32 restatements for the visual-injection kernels of csrc/dvm_proj.hip:
dvm_proj2img_f32 (depth render), dvm_i2p_f32 (bicubic back-projection), dvm_bicubic_resize_pad_f32, dvm_jbu_kernel_f32 and
dvm_adaptive_conv_f32 (d = 7 route and generic route).  Used by tests/test_gpu_visual_elements.py (device) and
tests/test_visual_ref_cpu.py (the same checks on the restatements and on planted mutations of them).  u = 2^-24 throughout.

Every restatement is numpy fp32 in the kernel's own operation order with one rounding per operation (an fma is evaluated in float64 and
rounded once) and takes mut=<name>: one deliberate defect.  The device may contract a * b + c where the source writes it in two
operations; that removes roundings, so the bars (which count one per operation) hold either way.

RENDER.  Compared with oracle/torch_ref.py::proj2img: pc_min / grid_size / offsets and the empty-pixel mask bit for bit; the colour code
of a non-empty pixel exactly where the pixel is DECIDED, within one bin elsewhere.  Classification (render_classify) from a float64
restatement: the cells in fp32 (the same arithmetic on every side), float64 depth sums s, sg = 1 / (1 + exp(-s)),
v = (sg - 0.485f) / 0.229f, d = (v - vmin) / (vmax - vmin), x = 256 d.  A pixel is decided when x is farther than its guard g from every
integer 1 .. 255 (0 and 256 are no bin boundaries: v >= vmin and v <= vmax hold on every side, so x in [0, g) gives code 0 and
x in (256 - g, 256] gives 255; this contains the image's minimum and maximum, where d is exactly 0 or 1).  The guard bounds the error of
ONE side's fp32 x against the float64 x, so both sides land in the float64 bin:
    e_sg = u (|s| w + 2 w + 2 sg) + s_err w,  w = sg (1 - sg)     the cast of s to fp32 moves sg by u |s| w; expf within 1 ulp = 2 u
                                                                   relative on e^-s moves sg by 2 u w; 1 + e and the reciprocal: u sg each
    e_v  = (e_sg + u |sg - 0.485|) / 0.229 + u |v|                the subtraction's and the division's rounding
    g    = 256 ((e_v(p) + e_v(min) + d (e_v(max) + e_v(min))) / R + 3 u),  R = vmax - vmin
                                                                   numerator and denominator errors, then the roundings of v - vmin,
                                                                   of R and of the quotient (u d each, d <= 1); the factor 256 is exact
s_err is the order error of the pixel's sum: 0 when every partial sum is exact (all depths multiples of a quantum q, the pixel's sum of
magnitudes below 2^24 q, q >= the fixed-point resolution), else (n - 1) u sum|z| for the oracle's sequential fp32 sum plus n 2^-(e+1) for
the splat's fixed-point rounding.  With e_v <= (5.78 + 4.73 |v|) u and two to four such terms in g, the simpler form
g = 256 (c u max|v| + s_err) / R (the first draft of this guard) corresponds to c = 15 .. 29 on a saturated image (max|v| = 2.25; it was written with c = 16).  That form is
NOT kept: e_sg is absolute (1.5 u at sg = 0.5), so c u max|v| understates it on a faint image (max|v| = 0.066 when every sum is tiny) --
the missing term -- and 0 / 256 are treated as no boundaries, which a "minimum or maximum" rule only covers at d = 0, 1 exactly.
Cap (a condition on the families, checked on the oracle alone): undecided <= 2 % of the non-empty pixels of each image.

BACK-PROJECTION and RESIZE.  Reference: float64 bicubic (A = -0.75, align_corners False, source index clamped).  Per-element bar
    K1 u sum|cy_a cx_b f_ab| + sum (dcy_a |cx_b| + |cy_a| dcx_b) |f_ab|,    dc = |c'(t)| dt + K2 u,   dt = u (3 |src| + 1)
K1 = 8: a product with cx and at most three adds (or four fma) to the row value, the same again with cy.  K2 = 32: the outer cubic in
Horner form at x = 2 rounds A x (1.5 u), - 5 A (2.25 u), * x (4.5 u), + 8 A (1.5 u), * x (3 u), carried through the later factors x <= 2:
6 + 9 + 9 + 3 + 3 = 30 u, plus x = t + 1 or 2 - t (2 u); the error is absolute, not relative to |c| (c has zeros).  dt: the source
coordinate scale * (i + 0.5) - 0.5 is formed in fp32 -- rounding of the scale, of the product, of the subtraction -- while the reference
has it exact; this term was missing in the first draft of the bar and dominates at non-dyadic scales.  Where scale and offsets are dyadic
(448, 112, 224; every x2 resize) the weights are multiples of 1/256, integer features make every product and partial sum exact, and the
output must equal the reference bit for bit.  normalize: bar / |row| + |out| (rho + u), rho = sum|v| bar / |row|^2 + (C / 2 + 4) u (the
norm's own error: C squares and adds, the wave reduction, the root); an all-zero row gives exactly 0.

ADAPTIVE CONVOLUTION.  Reference: float64 unfold contraction; bar d d u sum|in k| (a chain of d d fma); integer inputs: bit-equal.

JBU KERNEL.  Reference: the definition in float64 with the fp32 values of temp and sigma.  out_t = (e_t / se) G_t / max(tot, 1e-7),
e_t = exp(l_t - max l), G_t = exp(arg_t), arg_t = -(x^2 + y^2) / (2 sigma^2).  Relative bar per element (first order, times 1.01):
    rho_e = 2 u + u |l_t - mx| + dl_t + dl_mx      expf 1 ulp; the subtraction; the logits' own errors dl = NL temp u sum|q_c k_c|,
                                                   NL = 1 (the product temp * dot) on exact integer dots, 35 (32 fma, expf of
                                                   range_temp, the product) on real ones
    rho_se = 49 u + sum p_s rho_e,s                the 49-term sum, p = softmax
    rho_G = 2 u + 8 u |arg|                        the linspace coordinate, its square, the sum, 2 sigma^2 and its reciprocal, the product
    rho_v = rho_e + rho_se + rho_G + 2 u           the division by se and the product with G
    rho   = rho_v + 49 u + sum (v_s / tot) rho_v,s + 2 u        tot, its reciprocal, the last product
plus the absolute term 2^-126 (3 / max(tot, 1e-7) + 1) for values below the fp32 underflow of either exponential or of a product.
"""
import functools

import numpy as np

U = 2.0 ** -24
IMG = 224
F32 = np.float32
K1_CUBIC, K2_CUBIC = 8, 32
CAP_UNDECIDED = 0.02
TINY = 2.0 ** -126

RENDER_MUTATIONS = ("no_shift", "pixel_transposed", "bg_no_contributor", "no_255_clip", "recip_div")
RENDER_NEUTRAL = ("shift_no_clamp", "offsets_transposed")       # value-identical by construction: see test_visual_ref_cpu.py
I2P_MUTATIONS = ("swap_cxy", "t_flip", "wrap", "vec_at_border", "skip_ch64")
RESIZE_MUTATIONS = ("edge_repeat", "k_off_by_one", "wlo_whi_swapped")
ACONV_MUTATIONS = ("live1_from_k0", "drop_last_chunk", "tap_transposed")
JBU_MUTATIONS = ("edge_repeat", "spatial_before_norm", "no_floor", "taps_transposed")


# ----------------------------------------------------------------------------------------------------------------------- checks
def check_equal(name, got, exact):
    """bit for bit (NaN never passes): got fp32, exact float64 whose rounding to fp32 is the expected value"""
    got, ref = np.asarray(got), np.asarray(exact).astype(F32)
    assert got.shape == ref.shape and got.dtype == F32, (name, got.shape, ref.shape, got.dtype)
    bad = np.flatnonzero(~(got.ravel() == ref.ravel()))
    assert bad.size == 0, "%s: %d of %d elements differ; first at %s: got %r, exact %r" % (
        name, bad.size, ref.size, np.unravel_index(bad[0], ref.shape), float(got.ravel()[bad[0]]), float(ref.ravel()[bad[0]]))


def check_bound(name, got, ref, bound, frac=1.0):
    """per element |got - ref| <= frac * bound (NaN never passes); returns the largest err / bound"""
    got, ref, bound = np.asarray(got, np.float64), np.asarray(ref), np.broadcast_to(np.asarray(bound), np.shape(ref))
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    err = np.abs(got - ref)
    bad = np.flatnonzero(~(err.ravel() <= frac * bound.ravel()))
    if bad.size:
        w = bad[np.argmax(np.nan_to_num(err.ravel()[bad] / np.maximum(bound.ravel()[bad], 1e-300), nan=np.inf))]
        raise AssertionError("%s: %d of %d elements outside %.2g x their bound; worst at %s: got %r, ref %r, |err| %.3e, bound %.3e" % (
            name, bad.size, ref.size, frac, np.unravel_index(w, ref.shape), float(got.ravel()[w]), float(ref.ravel()[w]),
            float(err.ravel()[w]), float(bound.ravel()[w])))
    nz = bound.ravel() > 0
    return float((err.ravel()[nz] / bound.ravel()[nz]).max()) if nz.any() else 0.0


def _fma(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F32)


# ======================================================================================================================= render
_OFFS = np.array([[i, j] for i in range(-2, 3) for j in range(-2, 3)])       # o -> (o / 5 - 2, o % 5 - 2)
MEAN0, STD0 = np.float64(F32(0.485)), np.float64(F32(0.229))


def codes(img):
    """(B,3,224,224) colours -> colour-table index per pixel, 256 for the -1 background (tests/test_proj.py::_codes, and an image without
    a single coloured pixel passes through)."""
    import torch
    from oracle import torch_ref
    lut = torch_ref.piyg_lut().to(img.device)
    flat = img.permute(0, 2, 3, 1).reshape(-1, 3)
    code = torch.full((flat.shape[0],), 256, dtype=torch.int64, device=img.device)
    live = flat[:, 0] != -1
    if bool(live.any()):
        d = (flat[live][:, None, :] - lut[None]).abs().sum(-1)
        assert float(d.min(1)[0].max()) == 0.0                    # every colour IS a table entry
        code[live] = d.argmin(1)
    return code.view(img.shape[0], 224, 224).cpu().numpy()


def render_params(p, mut=None):
    """proj_range_kernel for one cloud p (N,3) fp32 -> dict(mn (2,), grid, off (2,), e, idx (N,2) fp32 cell indices)"""
    p = np.asarray(p, F32)
    N = p.shape[0]
    mn, mx = p[:, :2].min(0), p[:, :2].max(0)
    az = np.abs(p[:, 2]).max()
    rng = mx - mn
    grid = F32(max(rng[0], rng[1])) / F32(IMG - 3)
    with np.errstate(divide="ignore", invalid="ignore"):
        imax = np.floor((mx - mn) / grid)
        c = np.floor(((imax + F32(3)) + F32(-1)) / F32(2))
        off = F32(IMG // 2) - c.astype(np.int32).astype(F32) - F32(1)
        d = p[:, :2] - mn
        idx = np.floor(d * (F32(1) / grid) if mut == "recip_div" else d / grid)
    bound = float(az) * 25.0 * N
    e = min(61 - (int(np.floor(np.log2(bound))) + 1), 40) if bound > 0 else 40
    return dict(mn=mn, grid=grid, off=off, e=e, idx=idx)


def render_pixels(q, mut=None):
    """proj_splat_kernel's pixel of every (point, offset): -> r, c (N,25) int64 and keep (N,25) bool; raw (pre-shift) px, py"""
    offs = _OFFS.astype(F32)
    ax, ay = (1, 0) if mut == "offsets_transposed" else (0, 1)       # transposed: x steps with o % 5, y with o / 5 -- the same 25 pixels
    px = (q["idx"][:, None, 0] + offs[None, :, ax]) + F32(1) + q["off"][0]
    py = (q["idx"][:, None, 1] + offs[None, :, ay]) + F32(1) + q["off"][1]
    raw = (px.copy(), py.copy())
    keep = np.ones(px.shape, bool)
    if mut == "no_shift":                                            # no shift, the store guarded instead: the term is lost
        keep = (px >= 0) & (px <= IMG - 1) & (py >= 0) & (py <= IMG - 1)
    else:
        px = px + ((px < 0).astype(F32) - (px > IMG - 1).astype(F32))
        py = py + ((py < 0).astype(F32) - (py > IMG - 1).astype(F32))
    r, c = px.astype(np.int64), py.astype(np.int64)
    if mut == "shift_no_clamp":
        assert r.min() >= 0 and r.max() <= IMG - 1 and c.min() >= 0 and c.max() <= IMG - 1
    r, c = np.clip(r, 0, IMG - 1), np.clip(c, 0, IMG - 1)
    if mut == "pixel_transposed":
        r, c = c, r
    return r, c, keep, raw


def _depth_value32(s):
    with np.errstate(over="ignore"):
        sg = F32(1) / (F32(1) + np.exp(-s).astype(F32))
    return (sg - F32(0.485)) / F32(0.229)


def proj2img_np(pts, mut=None):
    """the four kernels of dvm_proj2img_f32 -> codes (B,224,224) int64 (256 = background), pc_min (B,2), grid (B,), offsets (B,2)"""
    pts = np.asarray(pts, F32)
    out, mns, grids, offs = [], [], [], []
    for p in pts:
        q = render_params(p, mut)
        r, c, keep, _ = render_pixels(q, mut)
        term = np.rint(np.ldexp(p[:, 2].astype(np.float64), q["e"])).astype(np.int64)
        acc, cnt = np.zeros(IMG * IMG, np.int64), np.zeros(IMG * IMG, np.int64)
        np.add.at(acc, (r * IMG + c)[keep], np.broadcast_to(term[:, None], r.shape)[keep])
        np.add.at(cnt, (r * IMG + c)[keep], 1)
        s = np.ldexp(acc.astype(np.float64), -q["e"]).astype(F32)
        v = _depth_value32(s)
        with np.errstate(invalid="ignore", divide="ignore"):
            d = (v - v.min()) / (v.max() - v.min())
            x = d * F32(256)
            k = np.where(x >= 256, 255 if mut != "no_255_clip" else 256, np.where(x < 0, 0, np.nan_to_num(x).astype(np.int64)))
        live = (cnt > 0) if mut == "bg_no_contributor" else (s != 0)
        out.append(np.where(live, k, 256).reshape(IMG, IMG))
        mns.append(q["mn"]), grids.append(q["grid"]), offs.append(q["off"])
    return np.stack(out), np.stack(mns), np.array(grids, F32), np.stack(offs)


def _quantum_exact(z, e, mags):
    """every partial sum exact in fp32 and in the fixed point: depths multiples of q = 2^-k, k <= e, and sum|z| < 2^24 q per pixel"""
    z = np.asarray(z, np.float64)
    for k in range(-20, e + 1):
        if np.all(np.ldexp(z, k) == np.rint(np.ldexp(z, k))):
            return float(mags.max()) < 2.0 ** (24 - k)
    return False


def _ev(s, serr):
    with np.errstate(over="ignore"):
        sg = 1.0 / (1.0 + np.exp(-s))
    w = sg * (1.0 - sg)
    v = (sg - MEAN0) / STD0
    return (U * (np.abs(s) * w + 2 * w + 2 * sg) + serr * w + U * np.abs(sg - MEAN0)) / STD0 + U * np.abs(v), v


def render_classify(pts):
    """float64 restatement per image -> list of dict(code64, nonempty, decided (224,224), share = undecided / non-empty, contrib)"""
    out = []
    for p in np.asarray(pts, F32):
        q = render_params(p)
        r, c, _, _ = render_pixels(q)
        flat = (r * IMG + c).ravel()
        z = np.broadcast_to(p[:, None, 2].astype(np.float64), r.shape).ravel()
        s, mags, n = np.zeros(IMG * IMG), np.zeros(IMG * IMG), np.zeros(IMG * IMG)
        np.add.at(s, flat, z), np.add.at(mags, flat, np.abs(z)), np.add.at(n, flat, 1)
        serr = np.zeros_like(s) if _quantum_exact(p[:, 2], q["e"], mags) else np.maximum(n - 1, 0) * U * mags + n * 2.0 ** -(q["e"] + 1)
        ev, v = _ev(s, serr)
        lo, hi = v.argmin(), v.argmax()
        R = v[hi] - v[lo]
        with np.errstate(invalid="ignore", divide="ignore"):
            d = (v - v[lo]) / R
            g = 256 * ((ev + ev[lo] + d * (ev[hi] + ev[lo])) / R + 3 * U)
            x = 256 * d
        near = np.clip(np.rint(x), 1, 255)
        decided = np.abs(x - near) > g
        nonempty = s != 0
        code = np.where(nonempty, np.clip(np.nan_to_num(np.floor(x)), 0, 255).astype(np.int64), 256)
        out.append(dict(code64=code.reshape(IMG, IMG), nonempty=nonempty.reshape(IMG, IMG), decided=decided.reshape(IMG, IMG),
                        share=float((nonempty & ~decided).sum()) / max(int(nonempty.sum()), 1), contrib=n.reshape(IMG, IMG)))
    return out


@functools.lru_cache(maxsize=None)
def render_oracle(family):
    """-> dict(pts, codes, pc_min (B,2), grid (B,), offsets (B,2) from oracle/torch_ref.py::proj2img, cls = render_classify)"""
    import torch
    from oracle import torch_ref
    pts = render_family(family)
    img, pc_min, grid, offs = torch_ref.proj2img(torch.from_numpy(pts))
    return dict(pts=pts, codes=codes(img), pc_min=pc_min.view(-1, 2).numpy(), grid=grid.view(-1).numpy(),
                offsets=torch.cat(offs, 1).float().numpy(), cls=render_classify(pts))


def check_render(name, got, ora):
    """got = (codes, pc_min, grid, offsets) of the implementation under test; ora = render_oracle(family)"""
    code, mn, grid, off = (np.asarray(a) for a in got)
    for k, a in (("pc_min", mn), ("grid", grid), ("offsets", off)):
        assert np.array_equal(np.asarray(a, F32).reshape(ora[k].shape), ora[k]), "%s: %s differs: %r vs %r" % (name, k, a, ora[k])
    for b, cl in enumerate(ora["cls"]):
        want = ora["codes"][b]
        assert np.array_equal(code[b] == 256, want == 256), "%s[%d]: the empty-pixel mask differs at %d pixels" % (
            name, b, int(((code[b] == 256) != (want == 256)).sum()))
        diff = np.abs(code[b] - want)
        bad = cl["nonempty"] & cl["decided"] & (diff != 0) & (want != 256)
        assert not bad.any(), "%s[%d]: %d decided pixels differ, first at %s: got %d, oracle %d" % (
            name, b, int(bad.sum()), tuple(np.argwhere(bad)[0]), code[b][bad][0], want[bad][0])
        assert diff[want != 256].max(initial=0) <= 1, "%s[%d]: an undecided pixel is %d bins off" % (name, b, diff[want != 256].max())


# ---- families: B = 3 clouds each.  Dyadic geometry: x = min + (k + f) g with g a power of two, so the cell of every point is certain
RENDER_FAMILIES = ("collisions", "cancellation", "borders", "flat", "lattice", "exponent", "zero", "random")
_G0 = 2.0 ** -8


def _dyadic_cloud(kx, ky, z, fx=None, fy=None, mn=(-0.25, 0.375)):
    """cells (kx, ky) in [0, 221] -> points; the caller pins cell 0 and cell 221 (offset 0) on the long axis"""
    fx = np.zeros(len(kx)) if fx is None else fx
    fy = np.zeros(len(ky)) if fy is None else fy
    return np.stack([mn[0] + (np.asarray(kx) + fx) * _G0, mn[1] + (np.asarray(ky) + fy) * _G0, np.asarray(z, np.float64)], 1).astype(F32)


def _aspect(b, kx, ky):
    """entry 0: rx > ry, entry 1: ry > rx (axes swapped), entry 2: rx == ry (the caller's ky spans 0 .. 221 there)"""
    return (ky, kx) if b == 1 else (kx, ky)


def _pins(b, ymax):
    """four corner cells: long axis 0 and 221 (offset 0), short axis 0 and ymax (221 for entry 2)"""
    ym = 221 if b == 2 else ymax
    return np.array([0, 0, 221, 221]), np.array([0, ym, 0, ym])


def lattice_xy(rng, n, lo, g, kmax, hi=None):
    """coordinates lo + k g formed in fp32, k random in [0, kmax], k = 0 and k = kmax pinned (the long axis passes its maximum hi, which
    stands in for k = 221, and nothing exceeds it): the fp32 quotient (x - lo) / g falls within an ulp of the integer k"""
    lo, g = F32(lo), F32(g)
    k = rng.integers(0, kmax + 1, n)
    k[0], k[1] = 0, kmax
    x = (lo + (k.astype(F32) * g).astype(F32)).astype(F32)
    if hi is not None:
        x = np.minimum(x, F32(hi))
        x[1] = F32(hi)
    return x


def lattice_near_integer(x, lo, g):
    """-> (below, at_or_above): points whose fp32 quotient is the float just below an integer / an integer or the float just above"""
    q = ((np.asarray(x, F32) - F32(lo)) / F32(g)).astype(F32)
    k = np.rint(q)
    below = (q < k) & (np.nextafter(q, F32(np.inf)) >= k)
    above = (q >= k) & (np.nextafter(q, F32(-np.inf)) <= k)
    return int(below.sum()), int(above.sum())


@functools.lru_cache(maxsize=None)
def render_family(family):
    out = []
    for b in range(3):
        rng = np.random.default_rng([4242, RENDER_FAMILIES.index(family), b])
        if family == "collisions":                                   # 2000 points in 132 + 4 cells, footprints of neighbours overlap
            cx, cy = np.meshgrid(40 + 3 * np.arange(12), 30 + 3 * np.arange(11), indexing="ij")
            pick = rng.integers(0, cx.size, 1996)
            px, py = _pins(b, 150)
            kx, ky = _aspect(b, np.concatenate([px, cx.ravel()[pick]]), np.concatenate([py, cy.ravel()[pick] + (60 if b == 2 else 0)]))
            f = rng.integers(0, 8, (2, 2000)) / 8.0
            f[:, :4] = 0
            out.append(_dyadic_cloud(kx, ky, rng.integers(-64, 65, 2000) / 64.0, f[0], f[1]))
        elif family == "cancellation":                               # isolated cells (spacing 6): 36 exact pairs, 36 pairs off by 2^-20, 36 singles
            cx, cy = np.meshgrid(10 + 6 * np.arange(12), 10 + 6 * np.arange(9), indexing="ij")
            cx, cy = cx.ravel(), cy.ravel()
            sgn = rng.choice([-1.0, 1.0], 108)                        # negatives stop at -3/4: the image is not symmetric about s = 0,
            z = np.where(sgn < 0, rng.integers(1, 49, 108), rng.integers(1, 65, 108)) / 64.0 * sgn     # so s = 2^-20 sits inside a bin
            px, py = _pins(b, 150)
            kx = np.concatenate([px, cx, cx[:72]])
            ky = np.concatenate([py, cy + (70 if b == 2 else 0), cy[:72] + (70 if b == 2 else 0)])
            zz = np.concatenate([[1.0, -0.75, 0.5, -0.5], z, -z[:36], -z[36:72] + 2.0 ** -20])
            kx, ky = _aspect(b, kx, ky)
            out.append(_dyadic_cloud(kx, ky, zz))
        elif family == "borders":                                    # minimum / maximum of both axes, all four corners, the edges between
            px, py = _pins(b, 150)
            ym = 221 if b == 2 else 150
            ex = np.concatenate([rng.integers(0, 222, 24), np.repeat([0, 221], 12), [0, 1, 2, 219, 220, 221] * 2])
            ey = np.concatenate([np.repeat([0, ym], 12), rng.integers(0, ym + 1, 24), [0] * 6 + [ym] * 6])
            kx, ky = _aspect(b, np.concatenate([px, ex]), np.concatenate([py, ey]))
            out.append(_dyadic_cloud(kx, ky, rng.integers(-64, 65, kx.size) / 64.0))
        elif family == "flat":                                       # one axis constant: entry 0, 2 every y equal (ry = 0), entry 1 every x equal
            kx = np.concatenate([[0, 221], rng.integers(0, 222, 62)])
            ky = np.zeros(64, np.int64)
            kx, ky = _aspect(b, kx, ky)
            out.append(_dyadic_cloud(kx, ky, rng.integers(-64, 65, 64) / 64.0 * (1 if b < 2 else 4)))
        elif family in ("lattice", "zero"):
            lo, hi, lo2, kmax = [(-0.37, 0.61, 0.113, 170), (1.7, 2.3, -5.1, 90), (-0.731, 0.269, 10.0, 220)][b]
            g = F32(F32(hi) - F32(lo)) / F32(IMG - 3)                  # the render's own grid for the long axis' extent
            x, y = lattice_xy(rng, 1500, lo, g, 221, hi), lattice_xy(rng, 1500, lo2, g, kmax)
            if b == 1:
                x, y = y, x
            z = rng.integers(-256, 257, 1500) / 256.0 if family == "lattice" else np.zeros(1500)
            out.append(np.stack([x, y, z.astype(F32)], 1).astype(F32))
        elif family == "exponent":
            px, py = _pins(b, 150)
            if b != 1:                                               # max|z| = 2^13: the exponent is 32 < 40, terms up to 2^45
                kx, ky = _aspect(b, np.concatenate([px, rng.integers(1, 221, 1996)]), np.concatenate([py, rng.integers(1, 150, 1996)]))
                z = rng.integers(-1024, 1025, 2000) * 8.0
                z[:4] = [8192.0, -8192.0, 8.0, -8.0]
                out.append(_dyadic_cloud(kx, ky, z))
            else:                                                    # max|z| = 2^-20: exponent at its cap 40; stacks in isolated cells give
                n = [900, 900, 39, 39, 95, 2, 2, 2, 2]               # sums +-900, +-39, 95, +-2 (+-4 in the doubled border rows) units: 256 d mid-bin
                sg = [1, -1, 1, -1, 1, 1, -1, 1, -1]
                cxs = [60, 100, 30, 140, 180, 0, 0, 221, 221]
                cys = [40, 90, 120, 20, 70, 0, 150, 0, 150]
                kx, ky = _aspect(b, np.repeat(cxs, n), np.repeat(cys, n))
                out.append(_dyadic_cloud(kx, ky, np.repeat(sg, n) * 2.0 ** -20))
        elif family == "random":                                     # Gaussian, depths not dyadic: exercises s_err
            sc = [(0.2, 0.5, 0.15), (0.6, 0.3, 0.4), (1.0, 1.0, 0.05)][b]
            out.append((rng.standard_normal((2048, 3)) * np.array(sc)).astype(F32))
        else:
            raise KeyError(family)
    n = min(len(p) for p in out)
    return np.stack([p[:n] for p in out])


def cancellation_pixels(b):
    """-> (pair cells, off-by-2^-20 cells) of entry b of the cancellation family as pixel centres (r, c) (N,2)"""
    cx, cy = np.meshgrid(10 + 6 * np.arange(12), 10 + 6 * np.arange(9), indexing="ij")
    cx, cy = cx.ravel(), cy.ravel() + (70 if b == 2 else 0)
    kx, ky = _aspect(b, cx, cy)
    q = render_params(render_family("cancellation")[b])
    pix = np.stack([kx + 1 + q["off"][0], ky + 1 + q["off"][1]], 1).astype(np.int64)
    return pix[:36], pix[36:72]


# ======================================================================================================= bicubic pieces (i2p, resize)
def _cubic32(t):
    """cubic_coeffs / cubic_w in fp32, one rounding per operation: t (...,) -> (..., 4)"""
    t = np.asarray(t, F32)
    A = F32(-0.75)
    o = lambda x: ((A * x - F32(5) * A) * x + F32(8) * A) * x - F32(4) * A          # noqa: E731
    i = lambda x: ((A + F32(2)) * x - (A + F32(3))) * x * x + F32(1)                # noqa: E731
    return np.stack([o(t + F32(1)), i(t), i(F32(1) - t), o(F32(2) - t)], -1).astype(F32)


def _cubic64(t):
    """-> coefficients (..., 4) and their derivatives in t"""
    t = np.asarray(t, np.float64)
    A = -0.75
    o = lambda x: ((A * x - 5 * A) * x + 8 * A) * x - 4 * A                         # noqa: E731
    i = lambda x: ((A + 2) * x - (A + 3)) * x * x + 1                               # noqa: E731
    do = lambda x: (3 * A * x - 10 * A) * x + 8 * A                                 # noqa: E731
    di = lambda x: (3 * (A + 2) * x - 2 * (A + 3)) * x                              # noqa: E731
    return (np.stack([o(t + 1), i(t), i(1 - t), o(2 - t)], -1), np.stack([do(t + 1), di(t), -di(1 - t), -do(2 - t)], -1))


def _axis64(n_src, n_dst, i):
    """destination indices i -> (taps (len,4) clamped, coefficients, dc bound) of the float64 definition"""
    src = n_src / n_dst * (np.asarray(i, np.float64) + 0.5) - 0.5
    i0 = np.floor(src)
    c, dc = _cubic64(src - i0)
    taps = np.clip(i0[:, None].astype(np.int64) - 1 + np.arange(4), 0, n_src - 1)
    dcb = np.abs(dc) * (U * (3 * np.abs(src) + 1))[:, None] + K2_CUBIC * U
    return taps, c, dcb


def _bicubic64(f, Ho, Wo, hs, ws, pairwise):
    """f (..., Hi, Wi) float64 sampled at destination (hs, ws): pairwise -> (..., len) at (hs[n], ws[n]); else the grid (..., len h, len w).
    -> value, bar"""
    Hi, Wi = f.shape[-2:]
    ty, cy, dy = _axis64(Hi, Ho, hs)
    tx, cx, dx = _axis64(Wi, Wo, ws)
    if pairwise:
        g = f[..., ty[:, :, None], tx[:, None, :]]                                   # (..., N, 4, 4)
        e = "...nab,na,nb->...n"
    else:
        g = f[..., ty[:, None, :, None], tx[None, :, None, :]]                       # (..., h, w, 4, 4)
        e = "...hwab,ha,wb->...hw"
    val = np.einsum(e, g, cy, cx)
    ag = np.abs(g)
    bar = (K1_CUBIC * U * np.einsum(e, ag, np.abs(cy), np.abs(cx)) + np.einsum(e, ag, dy, np.abs(cx))
           + np.einsum(e, ag, np.abs(cy), dx))
    return val, bar


# ============================================================================================================== back-projection
I2P_SIZES = ((224, 224), (256, 256), (32, 32), (37, 70), (448, 448), (112, 112), (3, 5), (1, 1))
I2P_CHANNELS = (1, 63, 64, 65, 130)
I2P_EXACT_SIZES = ((448, 448), (112, 112), (224, 224))
_EDGE = (0, 1, 2, 221, 222, 223)


def i2p_channels(size):
    return I2P_CHANNELS + ((384,) if size == (32, 32) else ())


@functools.lru_cache(maxsize=None)
def i2p_points():
    """B = 2 clouds with their own (pc_min, grid, offsets): all 36 combinations of rows / columns {0,1,2,221,222,223}, 260 interior pixels,
    mid-cell points (x = min + (k + 1/2) g in fp32).  -> pts (2,296,3), pc_min (2,2), grid (2,), offsets (2,2), pixel (2,296,2)"""
    pts, pix = [], []
    par = [((0.0, 0.0), 1.0, (-1.0, -1.0)), ((-0.4, 2.25), 0.00371, (-3.0, 4.0))]
    for b, (mn, g, off) in enumerate(par):
        rng = np.random.default_rng([777, b])
        r = np.concatenate([np.repeat(_EDGE, 6), rng.integers(3, 221, 260)])
        c = np.concatenate([np.tile(_EDGE, 6), rng.integers(3, 221, 260)])
        order = rng.permutation(r.size)
        r, c = r[order], c[order]
        k = np.stack([r - 1 - off[0], c - 1 - off[1]], 1)
        xy = (np.asarray(mn, F32) + ((k + 0.5).astype(F32) * F32(g)).astype(F32)).astype(F32)
        got = np.floor((xy - np.asarray(mn, F32)) / F32(g)) + F32(1) + np.asarray(off, F32)
        assert np.array_equal(got, np.stack([r, c], 1))
        pts.append(np.concatenate([xy, rng.standard_normal((r.size, 1)).astype(F32)], 1))
        pix.append(np.stack([r, c], 1))
    return (np.stack(pts), np.array([p[0] for p in par], F32), np.array([p[1] for p in par], F32), np.array([p[2] for p in par], F32),
            np.stack(pix))


def i2p_features(size, C, kind, seed=0):
    """(2, C, H, W) fp32: `real` normal with per-channel scales 1e-3 .. 1e3; `int` integers in [-64, 64]; `zero_rows` as real, but zero
    around the first 40 points of each cloud (all 16 taps; on maps below 32 x 32 the whole of entry 1 instead)"""
    rng = np.random.default_rng([778, size[0], size[1], C, seed])
    if kind == "int":
        return rng.integers(-64, 65, (2, C) + size, dtype=np.int8).astype(F32)
    f = rng.standard_normal((2, C) + size, dtype=F32) * (10.0 ** rng.uniform(-3, 3, (1, C, 1, 1))).astype(F32)
    if kind == "zero_rows" and size[0] * size[1] < 1024:              # small maps share their taps among all points: entry 1 is zero instead
        f[1] = 0
    elif kind == "zero_rows":
        pix = i2p_points()[4]
        for b in range(2):
            ty, _, _ = _axis64(size[0], IMG, pix[b, :40, 0])
            tx, _, _ = _axis64(size[1], IMG, pix[b, :40, 1])
            f[b][:, ty[:, :, None], tx[:, None, :]] = 0
    return f.astype(F32)


def i2p_reference(f, pix, normalize=False):
    """float64 definition at the points' pixels -> (value (B,N,C), bar (B,N,C))"""
    f = np.asarray(f, np.float64)
    H, W = f.shape[2:]
    vals, bars = [], []
    for b in range(f.shape[0]):
        if (H, W) == (IMG, IMG):
            v = f[b][:, pix[b][:, 0], pix[b][:, 1]]
            br = np.zeros_like(v)
        else:
            v, br = _bicubic64(f[b], IMG, IMG, pix[b][:, 0], pix[b][:, 1], True)
        vals.append(v.T), bars.append(br.T)
    v, br = np.stack(vals), np.stack(bars)
    if not normalize:
        return v, br
    nrm = np.sqrt((v * v).sum(-1, keepdims=True))
    C = v.shape[-1]
    with np.errstate(invalid="ignore", divide="ignore"):
        out = np.where(nrm > 0, v / np.maximum(nrm, 1e-12), 0.0)
        rho = (np.abs(v) * br).sum(-1, keepdims=True) / nrm ** 2 + (C / 2 + 4) * U
        # a row whose exact value is 0: all 16 taps zero (bar 0) -> exactly 0; else (taps that meet exact zeros of the weights) the
        # direction of the fp32 residue is not defined and nothing is asked
        bn = np.where(nrm > 0, br / nrm + np.abs(out) * (rho + U), np.where(i2p_tap_magnitude(f, pix)[..., None] == 0, 0.0, np.inf))
    return out, bn


def i2p_tap_magnitude(f, pix):
    """sum over channels and the 16 taps of |f| -> (B,N): 0 where a point samples nothing but zeros"""
    f = np.abs(np.asarray(f, np.float64)).sum(1)
    H, W = f.shape[1:]
    out = []
    for b in range(f.shape[0]):
        ty, _, _ = _axis64(H, IMG, pix[b][:, 0])
        tx, _, _ = _axis64(W, IMG, pix[b][:, 1])
        out.append(f[b][pix[b][:, 0], pix[b][:, 1]] if (H, W) == (IMG, IMG) else f[b][ty[:, :, None], tx[:, None, :]].sum((1, 2)))
    return np.stack(out)


def i2p_np(pts, f, pc_min, grid, offsets, normalize=False, mut=None):
    """i2p_kernel -> (B,N,C) fp32"""
    pts, f = np.asarray(pts, F32), np.asarray(f, F32)
    B, C, H, W = f.shape
    out = np.zeros((B, pts.shape[1], C), F32)
    for b in range(B):
        g = F32(grid[b])
        rc = (np.floor((pts[b][:, :2] - np.asarray(pc_min[b], F32)) / g) + F32(1)) + np.asarray(offsets[b], F32)
        rc = np.clip(rc.astype(np.int64), 0, IMG - 1)
        N = rc.shape[0]
        if H == IMG and W == IMG:
            cy = cx = np.tile(np.array([0, 1, 0, 0], F32), (N, 1))
            ys, xs = np.repeat(rc[:, :1], 4, 1), np.repeat(rc[:, 1:], 4, 1)
        else:
            sh, sw = F32(H) / F32(IMG), F32(W) / F32(IMG)
            fy, fx = sh * (rc[:, 0].astype(F32) + F32(0.5)) - F32(0.5), sw * (rc[:, 1].astype(F32) + F32(0.5)) - F32(0.5)
            y0, x0 = np.floor(fy), np.floor(fx)
            ty, tx = fy - y0, fx - x0
            cy, cx = _cubic32(ty), _cubic32(tx)
            if mut == "t_flip":
                cy[:, 2], cx[:, 2] = _cubic32(F32(1) - ty)[:, 2], _cubic32(F32(1) - tx)[:, 2]
            if mut == "swap_cxy":
                cy, cx = cx, cy
            ys, xs = y0[:, None].astype(np.int64) - 1 + np.arange(4), x0[:, None].astype(np.int64) - 1 + np.arange(4)
            if mut == "wrap":
                ys, xs = ys % H, xs % W
            else:
                ys, xs = np.clip(ys, 0, H - 1), np.clip(xs, 0, W - 1)
        flat = f[b].reshape(C, -1)
        xcol = xs[:, None, :]
        if mut == "vec_at_border":                                   # one 16-byte load from the first (clamped) tap, whatever follows it
            xcol = xs[:, None, :1] + np.arange(4)
        idx = np.minimum(ys[:, :, None] * W + xcol, H * W - 1)       # (N,4,4)
        t = flat[:, idx]                                             # (C,N,4,4)
        rows = ((t[..., 0] * cx[:, None, 0] + t[..., 1] * cx[:, None, 1]) + t[..., 2] * cx[:, None, 2]) + t[..., 3] * cx[:, None, 3]
        v = ((rows[..., 0] * cy[:, 0] + rows[..., 1] * cy[:, 1]) + rows[..., 2] * cy[:, 2]) + rows[..., 3] * cy[:, 3]      # (C,N)
        v = v.T.astype(F32)
        if mut == "skip_ch64":
            v[:, 64:] = 0
        if normalize:
            ss = np.zeros((N, 64), F32)
            for c0 in range(0, C, 64):
                w = min(64, C - c0)
                ss[:, :w] = ss[:, :w] + v[:, c0:c0 + w] * v[:, c0:c0 + w]
            s = 32
            while s:
                ss = ss + ss[:, np.arange(64) ^ s]
                s >>= 1
            v = v / np.maximum(np.sqrt(ss[:, :1]), F32(1e-12))
        out[b] = v
    return out


# ========================================================================================================================= resize
RESIZE_X2_SIZES = ((1, 1), (2, 3), (3, 2), (7, 5), (16, 16), (33, 17))
RESIZE_X2_PADS = (0, 1, 2, 3, 5)
RESIZE_GENERAL = (((7, 5), (224, 224)), ((9, 13), (18, 27)), ((16, 16), (8, 8)))
RESIZE_GENERAL_PADS = (0, 3)


def _reflect(i, n, repeat=False):
    i = np.asarray(i)
    return np.clip(i, 0, n - 1) if repeat else np.where(i < 0, -i, np.where(i >= n, 2 * n - 2 - i, i))


def resize_input(Hi, Wi, kind, BC=(2, 3)):
    rng = np.random.default_rng([779, Hi, Wi])
    if kind == "int":
        return rng.integers(-64, 65, BC + (Hi, Wi)).astype(F32)
    return (rng.standard_normal(BC + (Hi, Wi)) * 10.0 ** rng.uniform(-2, 2, BC + (1, 1))).astype(F32)


def resize_reference(x, size, pad):
    """float64 definition, then reflect pad -> (value, bar) (B,C,Ho+2pad,Wo+2pad)"""
    Ho, Wo = size
    hs, ws = _reflect(np.arange(-pad, Ho + pad), Ho), _reflect(np.arange(-pad, Wo + pad), Wo)
    return _bicubic64(np.asarray(x, np.float64), Ho, Wo, hs, ws, False)


def _bicubic_at32(x, Ho, Wo, hs, ws, sh, sw):
    """bicubic_at on the grid hs x ws (fma chains) -> (..., len h, len w) fp32"""
    Hi, Wi = x.shape[-2:]
    fy, fx = sh * (hs.astype(F32) + F32(0.5)) - F32(0.5), sw * (ws.astype(F32) + F32(0.5)) - F32(0.5)
    iy, ix = np.floor(fy), np.floor(fx)
    wy, wx = _cubic32(fy - iy), _cubic32(fx - ix)
    ty = np.clip(iy[:, None].astype(np.int64) - 1 + np.arange(4), 0, Hi - 1)
    tx = np.clip(ix[:, None].astype(np.int64) - 1 + np.arange(4), 0, Wi - 1)
    return _chain32(x, ty, tx, wy, wx)


def _chain32(x, ty, tx, wy, wx):
    acc = np.zeros(x.shape[:-2] + (ty.shape[0], tx.shape[0]), F32)
    for a in range(4):
        row = np.zeros_like(acc)
        for b in range(4):
            row = _fma(wx[None, :, b], x[..., ty[:, a][:, None], tx[:, b][None, :]], row)
        acc = _fma(wy[:, a][:, None], row, acc)
    return acc


def resize_np(x, size, pad, mut=None):
    """bicubic_pad_kernel, or bicubic_pad_x2_kernel where the launcher takes it -> (B,C,Ho+2pad,Wo+2pad) fp32"""
    x = np.asarray(x, F32)
    Hi, Wi = x.shape[-2:]
    Ho, Wo = size
    rep = mut == "edge_repeat"
    hp, wp = np.arange(Ho + 2 * pad), np.arange(Wo + 2 * pad)
    out = _bicubic_at32(x, Ho, Wo, _reflect(hp - pad, Ho, rep), _reflect(wp - pad, Wo, rep), F32(Hi) / F32(Ho), F32(Wi) / F32(Wo))
    if not (Ho == 2 * Hi and Wo == 2 * Wi and pad % 2 == 1):
        return out
    # 2 x 2 blocks: interior ones use the two constant weight sets on rows / columns k - 1 .. k + 2
    def axis(n_pad, n_out, n_in, swap):
        q = np.arange(n_pad)
        a0 = 2 * (q // 2) - pad                                       # the block's first unpadded coordinate (odd)
        inner = (a0 >= 0) & (a0 + 1 < n_out) & (2 * (q // 2) + 1 < n_pad)
        k = ((a0 - 1) >> 1) + (1 if mut == "k_off_by_one" else 0)
        t = np.where((q % 2 == 0) != swap, F32(0.25), F32(0.75))
        return inner, np.clip(k[:, None] - 1 + np.arange(4), 0, n_in - 1), _cubic32(t)
    iy, ty, wy = axis(Ho + 2 * pad, Ho, Hi, False)
    ix, tx, wx = axis(Wo + 2 * pad, Wo, Wi, mut == "wlo_whi_swapped")
    blk = _chain32(x, ty, tx, wy, wx)
    return np.where(iy[:, None] & ix[None, :], blk, out)


# ============================================================================================================ adaptive convolution
ACONV7_SHAPES = ((1, 1), (2, 31), (15, 32), (17, 33), (32, 32), (33, 65))
ACONV7_CHANNELS = (1, 3, 4, 5, 9, 22)
ACONV_GENERIC_SHAPES = ((3, 63), (2, 64), (5, 130))
ACONV_GENERIC_D = (1, 3, 5, 9, 15)
ACONV_GENERIC_CHANNELS = (1, 5, 9)
AT_CC, AT_TH, JT_W = 4, 16, 32


def aconv7_channels(shape):
    return ACONV7_CHANNELS + ((384,) if shape == (32, 32) else ())


def aconv7_split(B, C, H, W):
    """the launcher's channel split of the d = 7 route -> (csplit, cper)"""
    tiles = -(-W // JT_W) * -(-H // AT_TH) * B
    cs = 1
    while tiles * cs < 1024 and cs * 2 * AT_CC <= C:
        cs *= 2
    return cs, -(-C // cs)


def aconv_inputs(B, C, H, W, d, kind):
    """-> x (B,C,H+d-1,W+d-1), k (B,H,W,d,d) fp32; `int`: integers in [-8, 8]"""
    rng = np.random.default_rng([780, B, C, H, W, d])
    if kind == "int":
        return rng.integers(-8, 9, (B, C, H + d - 1, W + d - 1)).astype(F32), rng.integers(-8, 9, (B, H, W, d, d)).astype(F32)
    x = rng.standard_normal((B, C, H + d - 1, W + d - 1)) * 10.0 ** rng.uniform(-2, 2, (1, C, 1, 1))
    return x.astype(F32), rng.standard_normal((B, H, W, d, d)).astype(F32)


def _windows(x, d):
    return np.lib.stride_tricks.sliding_window_view(x, (d, d), axis=(-2, -1))     # (B,C,H,W,d,d)


def aconv_reference(x, k):
    """float64 unfold contraction -> (value, bar = d d u sum|in k|) (B,C,H,W)"""
    d = k.shape[-1]
    win, k64 = _windows(np.asarray(x, np.float64), d), np.asarray(k, np.float64)[:, None]
    val, mag = np.zeros(win.shape[:4]), np.zeros(win.shape[:4])
    for i in range(d):
        for j in range(d):
            t = win[..., i, j] * k64[..., i, j]
            val += t
            mag += np.abs(t)
    return val, d * d * U * mag


def aconv_np(x, k, tap_major=False, mut=None):
    """adaptive_conv7_kernel (d = 7) / adaptive_conv_kernel.  k is given pixel-major (B,H,W,d,d); tap_major says which layout the kernel
    under test reads (the values are the same) -> (B,C,H,W) fp32"""
    x, k = np.asarray(x, F32), np.asarray(k, F32)
    B, H, W, d, _ = k.shape
    C = x.shape[1]
    if mut == "tap_transposed" and not tap_major:
        k = k.transpose(0, 1, 2, 4, 3)
    if mut == "live1_from_k0" and d == 7:                             # the second pixel of a thread (odd row of its tile) takes the first's weights
        k = k.copy()
        k[:, 1::2] = k[:, 0:2 * (H // 2):2]
    win = _windows(x, d)
    acc = np.zeros((B, C, H, W), F32)
    for i in range(d):
        for j in range(d):
            acc = _fma(win[..., i, j], k[:, None, :, :, i, j], acc)
    if mut == "drop_last_chunk" and d == 7:
        cs, cper = aconv7_split(B, C, H, W)
        for s in range(cs):
            beg, end = s * cper, min(C, (s + 1) * cper)
            if end > beg:
                acc[:, beg + AT_CC * ((end - beg - 1) // AT_CC):end] = 0
    return acc


# ===================================================================================================================== JBU kernel
JBU_SHAPES = ((4, 4), (5, 8), (8, 33), (9, 41))
JBU_TEMPS = (10.0, -10.0, 0.0)          # range_temp: exp clamps to 1e4, to 1e-4, is exactly 1
JBU_SIGMAS = (1.0, 0.8, 0.05, 0.02)
# planted taps (i, j) of the 7 x 7 window: the centre, the four corners, ties of two taps next to the centre / of a corner and an edge tap
JBU_PLANTS = (((3, 3),), ((0, 0),), ((6, 6),), ((0, 6),), ((6, 0),), ((3, 2), (3, 4)), ((2, 3), (4, 3)), ((0, 0), (3, 6)), ((1, 5),))


def jbu_temp(range_temp):
    return np.clip(np.exp(F32(range_temp)).astype(F32), F32(1e-4), F32(1e4))


def jbu_proj(H, W, kind):
    """(2,32,H,W) fp32.  `peaked`: integers; background in [-1, 1]; plant n uses channel n: the query pixel holds 8 there, its target
    pixels 64 (and share one background vector, so ties are exact): the target's logit exceeds every other by > 350 at temp 1.
    `random`: uniform in [-1, 1)"""
    rng = np.random.default_rng([781, H, W])
    if kind == "random":
        return (rng.random((2, 32, H, W)) * 2 - 1).astype(F32)
    p = rng.integers(-1, 2, (2, 32, H, W)).astype(F32)
    for n, taps in enumerate(JBU_PLANTS):
        for b in ((0, 1) if H < 8 else (n % 2,)):
            if H < 8:                                                  # small maps: anywhere, the window reflects at both rims
                h, w = rng.integers(0, H), rng.integers(0, W)
            else:                                                      # whole windows inside the map, plants of one entry >= 6 columns apart
                h, w = H // 2, 3 + (n // 2) * ((W - 7) // 4)
            tgt = [(int(_reflect(h + i - 3, H)), int(_reflect(w + j - 3, W))) for i, j in taps]
            for th, tw in tgt[1:]:
                p[b, :, th, tw] = p[b, :, tgt[0][0], tgt[0][1]]
            p[b, n, h, w] = 64 if (h, w) in tgt else 8
            for th, tw in tgt:
                p[b, n, th, tw] = 64
    return p


def _jbu_windows(p, repeat=False):
    """(B,32,H,W) -> keys (B,32,7,7,H,W) under reflect padding"""
    H, W = p.shape[2:]
    hh = _reflect(np.arange(H)[None, :] + np.arange(-3, 4)[:, None], H, repeat)      # (7,H)
    ww = _reflect(np.arange(W)[None, :] + np.arange(-3, 4)[:, None], W, repeat)
    return p[:, :, hh[:, None, :, None], ww[None, :, None, :]]


def jbu_reference(proj, range_temp, sigma, exact_dots):
    """-> value (B,49,H,W) float64, bar (B,49,H,W)"""
    p = np.asarray(proj, np.float64)
    B, _, H, W = p.shape
    temp, sig = np.float64(jbu_temp(range_temp)), np.float64(F32(sigma))
    key = _jbu_windows(p)
    q = p[:, :, None, None]
    l = temp * (q * key).sum(1)                                        # (B,7,7,H,W)
    dl = (1 if exact_dots else 35) * temp * U * (np.abs(q) * np.abs(key)).sum(1)
    mx = l.max((1, 2), keepdims=True)
    dmx = dl.max((1, 2), keepdims=True)
    e = np.exp(l - mx)
    se = e.sum((1, 2), keepdims=True)
    pr = e / se
    r = np.linspace(-1, 1, 7)
    arg = -(r[:, None] ** 2 + r[None, :] ** 2) / (2 * sig * sig)
    G = np.exp(arg)[None, :, :, None, None]
    v = pr * G
    tot = v.sum((1, 2), keepdims=True)
    out = v / np.maximum(tot, 1e-7)
    rho_e = 2 * U + U * np.abs(l - mx) + dl + dmx
    rho_se = 49 * U + (pr * rho_e).sum((1, 2), keepdims=True)
    rho_v = rho_e + rho_se + (2 * U + 8 * U * np.abs(arg))[None, :, :, None, None] + 2 * U
    with np.errstate(invalid="ignore", divide="ignore"):
        rho_tot = 49 * U + np.where(tot > 0, (v * rho_v).sum((1, 2), keepdims=True) / tot, 0.0)
    bar = 1.01 * (rho_v + rho_tot + 2 * U) * out + TINY * (3 / np.maximum(tot, 1e-7) + 1)
    return out.reshape(B, 49, H, W), bar.reshape(B, 49, H, W)


def jbu_np(proj, range_temp, sigma, mut=None):
    """jbu_kernel_kernel<32, 7> -> (B,49,H,W) fp32"""
    p = np.asarray(proj, F32)
    B, _, H, W = p.shape
    temp, sig = jbu_temp(range_temp), F32(sigma)
    inv2s2 = F32(1) / (F32(2) * sig * sig)
    key = _jbu_windows(p, mut == "edge_repeat")
    dot = np.zeros((B, 7, 7, H, W), F32)
    for c in range(32):
        dot = _fma(p[:, c, None, None], key[:, c], dot)
    l = temp * dot
    mx = l.max((1, 2), keepdims=True)
    with np.errstate(under="ignore", over="ignore", invalid="ignore", divide="ignore"):
        e = np.exp(l - mx).astype(F32)
        se = np.zeros((B, 1, 1, H, W), F32)
        for t in range(49):
            se = se + e[:, t // 7, t % 7][:, None, None]
        r = (F32(-1) + F32(2) * np.arange(7, dtype=F32) / F32(6)).astype(F32)
        G = np.exp(-(r[None, :] * r[None, :] + r[:, None] * r[:, None]) * inv2s2).astype(F32)[None, :, :, None, None]
        v = (e * G if mut == "spatial_before_norm" else (e / se) * G).astype(F32)
        tot = np.zeros((B, 1, 1, H, W), F32)
        for t in range(49):
            tot = tot + v[:, t // 7, t % 7][:, None, None]
        inv = F32(1) / (tot if mut == "no_floor" else np.maximum(tot, F32(1e-7)))
        out = (v * inv).astype(F32)
    if mut == "taps_transposed":
        out = out.transpose(0, 2, 1, 3, 4)
    return out.reshape(B, 49, H, W)


# ================================================================================== the comparisons, on any implementation of the operators
# Each takes the implementation as numpy-in / numpy-out callables (the device binding in tests/test_gpu_visual_elements.py, the
# restatements above -- plain or mutated -- in tests/test_visual_ref_cpu.py), and returns the largest err / bar it saw (0 for exact checks).
# frac: the share of the bar that is allowed (the restatements must stay within 1/2).
def render_check(family, impl):
    """impl(pts (B,N,3)) -> (codes (B,224,224), pc_min, grid, offsets)"""
    ora = render_oracle(family)
    got = impl(ora["pts"])
    check_render(family, got, ora)
    perm = np.random.default_rng(5).permutation(ora["pts"].shape[1])
    again = impl(np.ascontiguousarray(ora["pts"][:, perm]))
    for a, b, k in zip(got, again, ("codes", "pc_min", "grid", "offsets")):
        assert np.array_equal(np.asarray(a), np.asarray(b)), "%s: %s changes when the points are permuted" % (family, k)
    return 0.0


def i2p_check(size, C, impl, frac=1.0):
    """impl(pts, f, pc_min, grid, offsets, normalize) -> (B,N,C) fp32"""
    pts, mn, grid, off, pix = i2p_points()
    worst = 0.0
    f = i2p_features(size, C, "real")
    ref, bar = i2p_reference(f, pix)
    got = impl(pts, f, mn, grid, off, False)
    name = "i2p %s C=%d" % (size, C)
    if size == (IMG, IMG):
        check_equal(name + " identity", got, ref)
    else:
        worst = max(worst, check_bound(name, got, ref, bar, frac))
    if size in I2P_EXACT_SIZES:
        fi = i2p_features(size, C, "int")
        check_equal(name + " int", impl(pts, fi, mn, grid, off, False), i2p_reference(fi, pix)[0])
    fz = i2p_features(size, C, "zero_rows")
    ref, bar = i2p_reference(fz, pix, True)
    got = impl(pts, fz, mn, grid, off, True)
    zero = i2p_tap_magnitude(fz, pix) == 0
    assert zero.sum() >= 80 and (~zero).sum() >= 200
    check_equal(name + " zero rows", got[zero], np.zeros_like(ref[zero]))
    worst = max(worst, check_bound(name + " normalize", got, ref, bar, frac))
    return worst


def resize_check(src, dst, pad, kind, impl, frac=1.0):
    """impl(x (B,C,Hi,Wi), size, pad) -> (B,C,Ho+2pad,Wo+2pad) fp32; kind `int`: bit-equal, `real`: the bar"""
    x = resize_input(src[0], src[1], kind)
    ref, bar = resize_reference(x, dst, pad)
    got = impl(x, dst, pad)
    name = "resize %s -> %s pad %d %s" % (src, dst, pad, kind)
    if kind == "int":
        check_equal(name, got, ref)
        return 0.0
    return check_bound(name, got, ref, bar, frac)


def aconv_check(B, C, H, W, d, tap_major, impl, frac=1.0):
    """impl(x, k (B,H,W,d,d), tap_major) -> (B,C,H,W) fp32 (the implementation lays k out tap-major itself when asked to)"""
    name = "adaptive_conv B=%d C=%d %dx%d d=%d %s" % (B, C, H, W, d, "tap-major" if tap_major else "pixel-major")
    x, k = aconv_inputs(B, C, H, W, d, "int")
    check_equal(name + " int", impl(x, k, tap_major), aconv_reference(x, k)[0])
    x, k = aconv_inputs(B, C, H, W, d, "real")
    ref, bar = aconv_reference(x, k)
    return check_bound(name, impl(x, k, tap_major), ref, bar, frac)


def jbu_check(shape, range_temp, sigma, kind, impl, frac=1.0):
    """impl(proj (B,32,H,W), range_temp, sigma) -> (B,49,H,W) fp32"""
    p = jbu_proj(shape[0], shape[1], kind)
    ref, bar = jbu_reference(p, range_temp, sigma, kind == "peaked")
    return check_bound("jbu %s temp %g sigma %g %s" % (shape, range_temp, sigma, kind), impl(p, range_temp, sigma), ref, bar, frac)
