"""The fused training BatchNorm (csrc/dvm_bn.hip) restated for its tests: the launch-route mirrors and case lists, the per-channel
input families, the fp64 reference of forward and backward with the per-element bounds, and a float32 emulation of the kernels'
operation sequence that only checks the reference on the CPU (tests/test_bn_ref_cpu.py).  tests/test_gpu_bn_elements.py holds the
kernels to the same reference.  No test lives here.

Layout: every array is [groups][rows][C] ("point-major"); a channel-major (B, C, N) tensor is one group of B * N rows in the order
e = b * N + n (to_rows / from_rows).  u = 2^-24 is the fp32 unit roundoff, n the number of values per channel and group.

Bounds (worst cases by derivation, no margin on top):
  save_mean            |got - mu| <= u |mu| + n 2^-53 mean|z|                    (one fp32 rounding + the fp64 sum in any order)
  save_invstd          relative 2u + rho, rho = delta / (2 (var + eps)), delta = n 2^-52 (mu^2 + var): the fp64 sum(z^2)/n - mean^2
                       form is off by at most delta in the variance, whatever the order of the sums
  y                    2^-23 (|s||mu| + 4 |s||z - mu| + |t| + |beta|) + rho |s||z - mu|, s = gamma invstd, t = (z - mu) s + beta:
                       the fp32 mean, gamma * invstd in fp32, the subtraction, the multiply-add in either contraction; the
                       activation is 1-Lipschitz for slope <= 1, so nothing near its kink is left out
  save_var_unbiased    2u var_unb + delta n / (n - 1): delta is an ABSOLUTE error of the variance; as a relative one it is
                       delta / var, which 2 rho = delta / (var + eps) understates once var is not far above eps (three rows of
                       the 1000 +- 0.05 channel left a relative 2u + 2 rho by a factor of 2 in the emulation)
  running statistics   per update 4u (|run| + m |batch|) + m (the batch value's own bound), carried from group to group
  dx                   2^-22 |k0| (|dz| + A1 + 3 |xhat| A2), A1 = mean|dz|, A2 = mean|dz xhat|, k0 = gamma invstd
  dbeta, dgamma        2^-23 n A1;  2^-22 n A2 + u |S2|;  groups: the kernel adds the groups' fp32 values in group order in fp32, the
                       reference in fp64: the groups' bounds plus u times the sum of their magnitudes (with the unused half of
                       the groups' bounds this is the worst case of up to 3 groups' additions; beyond that it covers the
                       additions' expected sqrt(groups) growth, not their (groups - 1) u worst case: test_bn_ref_cpu.py runs the
                       emulation at 64 groups);  accumulate: the fp64 sum with the prefilled value, + u |prefilled + value|
The backward takes y, save_mean and save_invstd as INPUTS, so the forward's rounding and the kink never enter its bounds."""
from collections import namedtuple

import numpy as np

U = 2.0 ** -24
EPS = 1e-5
MOMENTUM = 0.1
SLOPES = (1.0, 0.2, 0.0)
F32, F64 = np.float32, np.float64


# ------------------------------------------------------------------------------------------------------------------- route mirrors
def pm_group_for(C):
    return 128 if C % 128 == 0 else 64 if C % 64 == 0 else C


def pm_chunk_for(R, C):
    CG = pm_group_for(C)
    groups, rpp = C // CG, 256 // (CG >> 2)
    chunk = 4 * rpp
    while ((R + chunk - 1) // chunk) * groups > 256:
        chunk *= 2
    return chunk


def pm_splits_for(R, C):
    chunk = pm_chunk_for(R, C)
    return (R + chunk - 1) // chunk


def splits_for(B, C, N):
    total, S = B * N, 1
    while C * S < 1024 and total // (S * 2) >= 1024 and S < 64:
        S *= 2
    return S


PmRoute = namedtuple("PmRoute", "cg rpp idle splits splits_class doubled last_rows rem4")
CmRoute = namedtuple("CmRoute", "S vector last_short below_block")


def pm_route(R, C):
    """The route of bn_pm_reduce_kernel / the finalize kernels for R rows (per group) of C channels.  cg: '128', '64' or 'row' (the
    whole row, C % 64 != 0); rpp: thread rows per workgroup; idle: threads beyond rpp * (CG / 4); splits_class: '1', '2-32' (every
    partial on its own lane of pm_sum_partials) or '>32' (lanes loop); doubled: pm_chunk_for left 4 * rpp; last_rows: rows of the
    last chunk; rem4: passes of thread row 0 that the 4-rows-in-flight loop leaves to the remainder loop in the last chunk."""
    CG = pm_group_for(C)
    rpp = 256 // (CG >> 2)
    chunk, S = pm_chunk_for(R, C), pm_splits_for(R, C)
    last = R - (S - 1) * chunk
    return PmRoute("row" if CG == C and C % 64 else str(CG), rpp, rpp * (CG >> 2) < 256, S, "1" if S == 1 else "2-32" if S <= 32 else ">32",
                   chunk > 4 * rpp, last, ((last + rpp - 1) // rpp) % 4)


def cm_route(B, C, N):
    """The route of the channel-major kernels: S splits per channel; the float4 path (N % 4 == 0) or the scalar one; a last split
    shorter than the others; fewer elements per channel than one elementwise workgroup covers (1024)."""
    total, S = B * N, splits_for(B, C, N)
    chunk = (total + S - 1) // S
    return CmRoute(S, N % 4 == 0, total - (S - 1) * chunk < chunk, total < 1024)


CM_CASES = [(1, 1, 1), (2, 3, 5), (3, 5, 341), (2, 8, 1024), (1, 2, 2049), (1, 1, 65539), (1, 1024, 4), (2, 16, 300),
            (2, 4, 8192)]   # the last one: S = 16, the value between 2 and 64 that the others leave out
PM_CASES = [(R, C) for C, Rs in ((4, (1, 255, 257, 1023, 1025, 262147)), (12, (1, 84, 86, 341, 598)), (20, (50, 52, 205)),
                                 (64, (37, 65, 16385)), (128, (7, 9, 33, 8193)), (192, (100, 5505)), (260, (1, 2, 3, 4, 13, 3073)),
                                 (516, (1, 5, 1025)), (1000, (9,)), (1024, (33, 1025))) for R in Rs]
GROUP_CASES = [(37, 64, 2), (5, 12, 3), (13, 260, 2), (3, 8, 64)]   # (rows per group, C, groups)
SYNC_CASES = [(37, 64, 2), (5, 12, 1)]


# ------------------------------------------------------------------------------------------------------------------ input families
FAMILIES = ("normal", "offset", "hard_offset", "const", "tiny", "huge", "lastrow", "ramp", "pm1")
DY_FAMILIES = ("normal", "alt", "big")
CONST = 3.25


def family_of(c, g=0, start=0):
    """Channel c of group g: the families cycle over the channels, every group shifted by 4 (coprime to 9: neighbouring groups never
    share a channel's family, so another group's statistics are wrong by O(1))."""
    return FAMILIES[(c + 4 * g + start) % len(FAMILIES)]


def channel(fam, n, rng):
    r = np.arange(n)
    if fam == "normal":
        v = 3.0 * rng.standard_normal() + rng.uniform(0.5, 2.5) * rng.standard_normal(n)
    elif fam == "offset":
        v = 100.0 + 0.1 * rng.standard_normal(n)
    elif fam == "hard_offset":
        v = 1000.0 + 0.05 * rng.standard_normal(n)
    elif fam == "const":
        v = np.full(n, CONST)
    elif fam == "tiny":
        v = 1e-4 * rng.standard_normal(n)
    elif fam == "huge":
        v = 1e4 * rng.standard_normal(n)
    elif fam == "lastrow":
        v = np.zeros(n)
        v[-1] = 1.0
    elif fam == "ramp":
        v = r.astype(F64)
    elif fam == "pm1":
        v = 1.0 - 2.0 * (r & 1)
    else:
        raise ValueError(fam)
    return v.astype(F32)


def dy_channel(fam, n, rng):
    if fam == "normal":
        v = rng.standard_normal(n)
    elif fam == "alt":
        v = 1.0 - 2.0 * (np.arange(n) & 1)
    else:
        v = 1e3 * rng.standard_normal(n)
    return v.astype(F32)


def make_case(G, n, C, seed=0, with_res=False, dy_shift=0):
    """-> dict(x, res (or None), z = fl32(x + res), fams [G][C], gamma, beta, dy, dy_fams [C]).  gamma holds a 0 (c % 7 == 1) and
    negative values (c % 7 == 2), beta a 0 (c % 5 == 3), wherever C reaches that far."""
    rng = np.random.default_rng([seed, G, n, C, int(with_res)])
    start = (7 * n + C + seed) % len(FAMILIES)
    fams = [[family_of(c, g, start) for c in range(C)] for g in range(G)]
    x = np.empty((G, n, C), F32)
    dy = np.empty((G, n, C), F32)
    dy_fams = [DY_FAMILIES[(c + c // 9 + dy_shift) % 3] for c in range(C)]
    for g in range(G):
        for c in range(C):
            x[g, :, c] = channel(fams[g][c], n, rng)
            dy[g, :, c] = dy_channel(dy_fams[c], n, rng)
    res = rng.standard_normal((G, n, C)).astype(F32) if with_res else None
    z = x if res is None else x + res            # float32 + float32: rounded once, as the kernels form it
    idx = np.arange(C)
    gamma = rng.uniform(0.5, 1.5, C)
    gamma[idx % 7 == 1] = 0.0
    gamma[idx % 7 == 2] *= -1.0
    beta = rng.standard_normal(C)
    beta[idx % 5 == 3] = 0.0
    return dict(x=x, res=res, z=z, fams=fams, gamma=gamma.astype(F32), beta=beta.astype(F32), dy=dy, dy_fams=dy_fams)


def backward_inputs(z, gamma, beta, slope, stats_of=None):
    """The backward's y, save_mean and save_invstd as the TEST supplies them: the fp64 forward rounded to float32 (not a kernel's
    output), then +0.0, -0.0 and the smallest normal float planted into y (rows 0, 1, 2 of every group, rotating over the
    channels): both zeros must take the slope branch, the smallest normal the slope-1 branch."""
    f = forward_ref(z, gamma, beta, slope, stats_of=stats_of)
    y = f["y"].astype(F32)
    G, n, C = y.shape
    plants = (F32(0.0), F32(-0.0), np.finfo(F32).tiny)
    for g in range(G):
        for c in range(C):
            for k, v in enumerate(plants):
                if k < n:
                    y[g, (k + c) % n if n >= 3 else k, c] = v
    return y, f["mean"].astype(F32), f["invstd"].astype(F32)


def to_rows(t):
    """(B, C, N) -> [1][B * N][C]"""
    B, C, N = t.shape
    return np.ascontiguousarray(t.transpose(0, 2, 1).reshape(1, B * N, C))


def from_rows(r, B, N):
    """[1][B * N][C] -> (B, C, N)"""
    return np.ascontiguousarray(r.reshape(B, N, -1).transpose(0, 2, 1))


# -------------------------------------------------------------------------------------------------------------- the fp64 reference
def _f32c(v):
    return float(F32(v))


def forward_ref(z, gamma, beta, slope, eps=EPS, stats_of=None):
    """z [G][n][C] float32 (x + res already rounded).  stats_of: the rows whose statistics normalise z (the cross-rank form: both
    ranks' rows of every group); default z itself.  -> the fp64 values and their bounds, [G][C] or [G][n][C]."""
    zs = (z if stats_of is None else stats_of).astype(F64)
    n = zs.shape[1]
    mu = zs.sum(1) / n
    var = ((zs - mu[:, None]) ** 2).sum(1) / n
    mabs = np.abs(zs).sum(1) / n
    e = _f32c(eps)
    inv = 1.0 / np.sqrt(var + e)
    delta = n * 2.0 ** -52 * (mu * mu + var)
    rho = 0.5 * delta / (var + e)
    g, b, sl = np.asarray(gamma, F64), np.asarray(beta, F64), _f32c(slope)
    s = g * inv
    d = z.astype(F64) - mu[:, None]
    t = d * s[:, None] + b
    y = np.where(t > 0, t, sl * t)
    sd = np.abs(s)[:, None] * np.abs(d)
    unb = var * n / (n - 1) if n > 1 else var
    return dict(n=n, mean=mu, var=var, invstd=inv, rho=rho, y=y, unb=unb,
                mean_bound=U * np.abs(mu) + n * 2.0 ** -53 * mabs,
                invstd_bound=(2 * U + rho) * inv,
                y_bound=2.0 ** -23 * (np.abs(s * mu)[:, None] + 4 * sd + np.abs(t) + np.abs(b)) + rho[:, None] * sd,
                unb_bound=2 * U * unb + delta * (n / (n - 1.0) if n > 1 else 1.0))


def running_ref(run0, batch, batch_bound, momentum=MOMENTUM, fp32_constants=True):
    """(1 - m) run + m batch with the fp32 constants m and fl32(1 - m) (fp32_constants=False: 1 - m in fp64, torch's own form),
    group after group.  run0 [C], batch / batch_bound [G][C] -> (run, bound)."""
    m = _f32c(momentum)
    om = float(F32(1.0) - F32(momentum)) if fp32_constants else 1.0 - m
    run, err = np.asarray(run0, F64).copy(), np.zeros(len(run0))
    for g in range(batch.shape[0]):
        err = om * err + 4 * U * (np.abs(run) + m * np.abs(batch[g])) + m * batch_bound[g]
        run = om * run + m * batch[g]
    return run, err


def ordered_f32_sum(vals, prefilled=None):
    """The emulation's parameter gradients: the fp32 sum in group order of the groups' values rounded to fp32 (vals [G][C]), then
    once into `prefilled`."""
    acc = np.zeros(vals.shape[1], F32)
    for g in range(vals.shape[0]):
        acc = acc + vals[g].astype(F32)
    return acc if prefilled is None else np.asarray(prefilled, F32) + acc


def backward_ref(z, y, dy, mean, invstd, gamma, slope, other=None, prefilled=None):
    """z, y, dy [G][n][C]; mean, invstd [G][C] exactly as the kernel is handed them.  other = (z, y, dy) of the other rank's rows
    (cross-rank form): the means of dz and dz xhat are taken over both ranks' rows, dgamma / dbeta stay the local sums.
    prefilled = (dgamma, dbeta) the accumulate = 1 call adds into."""
    sl = _f32c(slope)
    mf, inv, g = np.asarray(mean, F64)[:, None], np.asarray(invstd, F64)[:, None], np.asarray(gamma, F64)

    def terms(z_, y_, dy_):
        dz = dy_.astype(F64) * np.where(y_ > 0, 1.0, sl)
        xh = (z_.astype(F64) - mf) * inv
        return dz, xh, dz.sum(1), (dz * xh).sum(1), np.abs(dz).sum(1), np.abs(dz * xh).sum(1)

    dz, xh, S1, S2, T1, T2 = terms(z, y, dy)
    n = z.shape[1]
    N, G1, G2, A1, A2 = n, S1, S2, T1, T2
    if other is not None:
        _, _, o1, o2, p1, p2 = terms(*other)
        N, G1, G2, A1, A2 = n + other[0].shape[1], S1 + o1, S2 + o2, T1 + p1, T2 + p2
    A1, A2 = A1 / N, A2 / N
    k0 = (g * inv[:, 0])[:, None]
    dx = k0 * ((dz - (G1 / N)[:, None]) - xh * (G2 / N)[:, None])
    dx_bound = 2.0 ** -22 * np.abs(k0) * (np.abs(dz) + A1[:, None] + 3 * np.abs(xh) * A2[:, None])
    many = U if z.shape[0] > 1 else 0.0
    dbeta_bound = (2.0 ** -23 * T1).sum(0) + many * np.abs(S1).sum(0)
    dgamma_bound = (2.0 ** -22 * T2 + U * np.abs(S2)).sum(0) + many * np.abs(S2).sum(0)
    dgamma, dbeta = S2.sum(0), S1.sum(0)           # fp64 and unrounded: the kernel's fp32 roundings are what the bounds count
    if prefilled is not None:
        dgamma, dbeta = dgamma + np.asarray(prefilled[0], F64), dbeta + np.asarray(prefilled[1], F64)
        dgamma_bound, dbeta_bound = dgamma_bound + U * np.abs(dgamma), dbeta_bound + U * np.abs(dbeta)
    return dict(dx=dx, dx_bound=dx_bound, dgamma=dgamma, dgamma_bound=dgamma_bound, dbeta=dbeta, dbeta_bound=dbeta_bound,
                S1=S1, S2=S2)


def rank_totals(z, bwd=None):
    """What one rank hands the collective: [G][C][2] totals + [G] row counts, float64 (forward: sum z, sum z^2; backward, with
    bwd = (y, dy, mean, invstd, slope): sum dz, sum dz xhat)."""
    G, n, C = z.shape
    zd = z.astype(F64)
    if bwd is None:
        a, q = zd.sum(1), (zd * zd).sum(1)
    else:
        y, dy, mean, invstd, slope = bwd
        dz = dy.astype(F64) * np.where(y > 0, 1.0, _f32c(slope))
        a, q = dz.sum(1), (dz * (zd - np.asarray(mean, F64)[:, None]) * np.asarray(invstd, F64)[:, None]).sum(1)
    return np.concatenate([np.stack([a, q], -1).reshape(-1), np.full(G, float(n))])


def worst(got, want, bound):
    """-> (ratio, index, got, want, bound) of the element with the largest error / bound (a NaN or a nonzero error on a zero bound
    counts as infinite)."""
    got, want, bound = np.asarray(got, F64), np.asarray(want, F64), np.broadcast_to(np.asarray(bound, F64), np.shape(want))
    err = np.abs(got - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0, 0.0, np.where(np.isnan(err), np.inf, err / bound))
    ratio = np.where(np.isnan(ratio), np.inf, ratio)
    i = np.unravel_index(int(np.argmax(ratio)), ratio.shape) if ratio.size else ()
    return (float(ratio[i]), i, float(got[i]), float(want[i]), float(bound[i])) if ratio.size else (0.0, (), 0.0, 0.0, 0.0)


# ------------------------------------------------------------------------------------------------------------- float32 emulation
PLANTS = ("drop_last_row", "biased_running", "other_group_stats", "ge_zero", "s1_for_s2")


def _madd(a, b, c, fma):
    """a * b + c on float32 arrays: two roundings, or one (the product of two floats is exact in fp64)."""
    return (a.astype(F64) * b.astype(F64) + c.astype(F64)).astype(F32) if fma else a * b + c


def emulate_forward(z, gamma, beta, slope, fma=False, eps=EPS, momentum=MOMENTUM, running=None, plant=None):
    """bn_stats_kernel + bn_apply_kernel (and the point-major pair) as documented: fp64 sums, fp32 mean / invstd / gamma * invstd,
    t = (z - mean) * sc + beta, y = t > 0 ? t : t * slope; running = (1 - m) running + m batch group after group."""
    n = z.shape[1]
    zs = z.astype(F64)
    if plant == "drop_last_row":
        zs = zs[:, :-1]
    mean = zs.sum(1) / n
    var = np.maximum((zs * zs).sum(1) / n - mean * mean, 0.0)
    inv, mf = (1.0 / np.sqrt(var + float(F32(eps)))).astype(F32), mean.astype(F32)
    unb = ((var * n / (n - 1)) if n > 1 and plant != "biased_running" else var).astype(F32)
    out = dict(mean=mf, invstd=inv, unb=unb)
    if running is not None:
        rm, rv = (np.asarray(r, F32).copy() for r in running)
        om, m = F32(1.0) - F32(momentum), F32(momentum)
        for g in range(z.shape[0]):
            rm, rv = _madd(np.full_like(rm, om), rm, m * mf[g], fma), _madd(np.full_like(rv, om), rv, m * unb[g], fma)
        out.update(running_mean=rm, running_var=rv)
    if plant == "other_group_stats":
        mf, inv = np.roll(mf, 1, 0), np.roll(inv, 1, 0)
    sc = np.asarray(gamma, F32) * inv
    bt = np.broadcast_to(np.asarray(beta, F32), z.shape)
    t = _madd(z - mf[:, None], np.broadcast_to(sc[:, None], z.shape), bt, fma)
    out["y"] = np.where(t > 0, t, t * F32(slope))
    return out


def emulate_backward(z, y, dy, mean, invstd, gamma, slope, fma=False, plant=None, prefilled=None):
    """bn_bwd_reduce_kernel + bn_bwd_apply_kernel (and the point-major pair): dz = dy * (y > 0 ? 1 : slope),
    xhat = (z - mean) * invstd in fp32, fp64 sums, dx = k0 * ((dz - m1) - xhat * m2)."""
    n = z.shape[1]
    mf, inv = np.asarray(mean, F32)[:, None], np.asarray(invstd, F32)[:, None]
    dz = dy * np.where((y >= 0) if plant == "ge_zero" else (y > 0), F32(1.0), F32(slope))
    xh = (z - mf) * inv
    rows = slice(0, -1) if plant == "drop_last_row" else slice(None)
    ta, tq = dz[:, rows].astype(F64).sum(1), (dz[:, rows].astype(F64) * xh[:, rows].astype(F64)).sum(1)
    pg, pb = (None, None) if prefilled is None else prefilled
    m1, m2 = (ta / n).astype(F32), ((ta if plant == "s1_for_s2" else tq) / n).astype(F32)
    k0 = (np.asarray(gamma, F32) * inv[:, 0])[:, None]
    a = dz - m1[:, None]
    inner = (a.astype(F64) - xh.astype(F64) * m2[:, None].astype(F64)).astype(F32) if fma else a - xh * m2[:, None]
    return dict(dx=k0 * inner, dgamma=ordered_f32_sum(tq, pg), dbeta=ordered_f32_sum(ta, pb))
