"""-m gpu: the fused training BatchNorm (csrc/dvm_bn.hip) per ELEMENT and per CHANNEL on every reduction route — channel-major
forward / backward, point-major forward / backward, the grouped form and the cross-rank `_sync` form — against the fp64 reference
and the derived bounds of tests/bn_ref.py (checked on the CPU by tests/test_bn_ref_cpu.py).  Every channel of a case carries
another input family (large offsets, a constant, variance far below eps, one outlier in the last row, ...), so a channel is held
to its OWN noise floor; the backward is handed y / save_mean / save_invstd of the test's making (both zeros and the smallest normal
planted into y), so nothing near the activation's kink is masked.  A failure names the case, its route, the output, the channel's
family, the worst element and its error / bound ratio.

The cross-rank form runs in ONE process: the collective is a ctypes callback that adds the "other rank's" totals (computed by the
reference) to the statistics buffer on the stream the library names.  No process group exists at any point (`import torch` itself
loads the torch.distributed module, so its absence from sys.modules cannot be the test; that it is never initialised is).

Largest measured error / bound on an MI355X (printed per test, `-s`): y 0.47, dx 0.74, save_invstd 0.49, save_var_unbiased 0.50,
running statistics 0.45, dgamma 0.45, dbeta 0.67; save_mean 0.999 and the accumulate = 1 gradients 0.98 — single correctly rounded
operations, whose half-ulp error reaches the u |value| term of their bound and cannot pass it."""
import ctypes

import numpy as np
import pytest
import torch

import bn_ref as BR

pytestmark = pytest.mark.gpu

EPS, MOM = BR.EPS, BR.MOMENTUM
SENTINEL = 12345.0
_NO_PROCESS_GROUP_AT_COLLECTION = not torch.distributed.is_initialized()
RATIOS = {}


@pytest.fixture(scope="module")
def ops():
    from dvm import ops as _ops
    assert torch.cuda.is_available()
    return _ops


def _cuda(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _act32(beta, slope):
    b = np.float32(beta)
    return b if b > 0 else b * np.float32(slope)


class _Report:
    """Collects every complaint of one case, so one failure shows all of them."""

    def __init__(self, group, case, route):
        self.group, self.case, self.route, self.lines = group, case, route, []

    def check(self, name, got, want, bound, fams=None, slope=None):
        ratio, i, g, w, b = BR.worst(got, want, bound)
        RATIOS[(self.group, name)] = max(RATIOS.get((self.group, name), 0.0), ratio)
        if not ratio <= 1.0:
            fam = "" if fams is None or not i else " family %s" % (fams[i[0]][i[-1]] if len(i) > 1 else "/".join(sorted({f[i[-1]] for f in fams})))
            self.lines.append("%s slope=%s: %s%s worst at %s: got %.9g want %.9g, error / bound = %.3g (bound %.3g)"
                              % (self.case, slope, name, fam, tuple(int(k) for k in i), g, w, ratio, b))
        return ratio

    def require(self, ok, text):
        if not ok:
            self.lines.append("%s: %s" % (self.case, text))

    def finish(self):
        print("RATIO %s up to %s, largest error / bound: %s" % (self.group, self.case, ", ".join(
            "%s %.3f" % (k[1], v) for k, v in sorted(RATIOS.items()) if k[0] == self.group)))
        assert not self.lines, "route %s\n%s" % (self.route, "\n".join(self.lines))


class _Pm:
    """[G][n][C] arrays <-> the point-major entry points (groups = 1 through the grouped wrappers as well)."""

    def __init__(self, ops, G, n, C):
        self.ops, self.G, self.n, self.C = ops, G, n, C

    def up(self, a):
        return None if a is None else _cuda(a.reshape(self.G * self.n, self.C))

    def down(self, t):
        return t.cpu().numpy().reshape(self.G, self.n, self.C)

    def fwd(self, x, res, gamma, beta, slope, rm, rv):
        return self.ops.bn_act_train_fwd_pm_groups(x, res, gamma, beta, EPS, slope, MOM, self.G, want_var=True, running_mean=rm, running_var=rv)

    def bwd(self, dy, y, x, res, gamma, mean, invstd, slope, grads=None):
        return self.ops.bn_act_train_bwd_pm_groups(dy, y, x, res, gamma, mean, invstd, slope, self.G, grads=grads)


class _Cm:
    """[1][B * N][C] arrays <-> the channel-major (B, C, N) entry points."""

    def __init__(self, ops, B, C, N):
        self.ops, self.B, self.N, self.C, self.G, self.n = ops, B, N, C, 1, B * N

    def up(self, a):
        return None if a is None else _cuda(BR.from_rows(a, self.B, self.N))

    def down(self, t):
        return BR.to_rows(t.cpu().numpy())

    def fwd(self, x, res, gamma, beta, slope, rm, rv):
        y, mean, invstd = self.ops.bn_act_train_fwd(x, res, gamma, beta, EPS, slope, MOM, rm, rv)
        return y, mean.view(1, -1), invstd.view(1, -1), None

    def bwd(self, dy, y, x, res, gamma, mean, invstd, slope, grads=None):
        assert grads is None
        return self.ops.bn_act_train_bwd(dy, y, x, res, gamma, mean.view(-1), invstd.view(-1), slope)


def _run_case(rep, lay, case, slope, seed):
    """Forward and backward of one case at one slope through layout `lay`, every output against the reference."""
    G, n, C = lay.G, lay.n, lay.C
    z, gamma, beta, fams = case["z"], case["gamma"], case["beta"], case["fams"]
    rng = np.random.default_rng([seed, G, n, C])
    run0 = rng.standard_normal(C).astype(np.float32), rng.uniform(0.5, 2.0, C).astype(np.float32)
    xd, rd, gd, bd, dyd = lay.up(case["x"]), lay.up(case["res"]), _cuda(gamma), _cuda(beta), lay.up(case["dy"])

    # ------------------------------------------------------------------------------------------------------------------ forward
    f = BR.forward_ref(z, gamma, beta, slope)
    rm, rv = _cuda(run0[0]), _cuda(run0[1])
    y, mean, invstd, var = lay.fwd(xd, rd, gd, bd, slope, rm, rv)
    yh = lay.down(y)
    rep.check("y", yh, f["y"], f["y_bound"], fams, slope)
    rep.check("save_mean", mean.cpu().numpy(), f["mean"], f["mean_bound"], fams, slope)
    rep.check("save_invstd", invstd.cpu().numpy(), f["invstd"], f["invstd_bound"], fams, slope)
    if var is not None:
        rep.check("save_var_unbiased", var.cpu().numpy(), f["unb"], f["unb_bound"], fams, slope)
    want, bound = BR.running_ref(run0[0], f["mean"], f["mean_bound"])
    rep.check("running_mean", rm.cpu().numpy(), want, bound, fams, slope)
    want, bound = BR.running_ref(run0[1], f["unb"], f["unb_bound"])
    rep.check("running_var", rv.cpu().numpy(), want, bound, fams, slope)
    rep.require(bool(torch.isfinite(rv).all()), "running_var is not finite")
    if G > 1:       # the rows on either side of every group boundary, by name
        for g in range(G):
            for row, which in ((0, "first"), (n - 1, "last")):
                r = BR.worst(yh[g, row], f["y"][g, row], f["y_bound"][g, row])
                rep.require(r[0] <= 1.0, "slope=%s: y of the %s row of group %d, channel %d (%s): got %.9g want %.9g, error / bound = %.3g"
                            % (slope, which, g, r[1][0] if r[1] else 0, fams[g][r[1][0]] if r[1] else "-", r[2], r[3], r[0]))

    # the same call again: the same bits (a fixed summation order); running_* = None: the same outputs, no statistics touched
    rm2, rv2 = _cuda(run0[0]), _cuda(run0[1])
    again = lay.fwd(xd, rd, gd, bd, slope, rm2, rv2)
    for name, a, b in zip(("y", "save_mean", "save_invstd", "save_var_unbiased", "running_mean", "running_var"),
                          (y, mean, invstd, var, rm, rv), again + (rm2, rv2)):
        rep.require(a is None or _same_bits(a, b), "slope=%s: %s differs between two identical calls" % (slope, name))
    keep_m, keep_v = _cuda(run0[0]), _cuda(run0[1])
    plain = lay.fwd(xd, rd, gd, bd, slope, None, None)
    for name, a, b in zip(("y", "save_mean", "save_invstd", "save_var_unbiased"), (y, mean, invstd, var), plain):
        rep.require(a is None or _same_bits(a, b), "slope=%s: %s differs without running statistics" % (slope, name))
    rep.require(_same_bits(keep_m, _cuda(run0[0])) and _same_bits(keep_v, _cuda(run0[1])), "statistics buffers changed by a call that was given none")
    if isinstance(lay, _Pm) and G == 1:     # dvm_bn_act_train_fwd_pm_f32 is the groups = 1 call of _var_f32
        rm3, rv3 = _cuda(run0[0]), _cuda(run0[1])
        y3, m3, i3 = lay.ops.bn_act_train_fwd_pm(xd, rd, gd, bd, EPS, slope, MOM, rm3, rv3)
        rep.require(_same_bits(y3, y) and _same_bits(m3.view(1, -1), mean) and _same_bits(i3.view(1, -1), invstd) and _same_bits(rm3, rm)
                    and _same_bits(rv3, rv), "slope=%s: dvm_bn_act_train_fwd_pm_f32 differs from the groups = 1 call" % slope)

    # exact: a constant channel
    if case["res"] is None:
        mh, ih, vh, rvh = mean.cpu().numpy(), invstd.cpu().numpy(), None if var is None else var.cpu().numpy(), rv.cpu().numpy()
        inv0 = np.float32(1.0 / np.sqrt(np.float64(np.float32(EPS))))
        for g in range(G):
            for c in range(C):
                if fams[g][c] != "const":
                    continue
                ok = np.array_equal(yh[g, :, c].view(np.int32), np.full(n, _act32(beta[c], slope), np.float32).view(np.int32))
                rep.require(ok, "slope=%s: const channel %d of group %d: y is not act(beta) = %r bit for bit (first %r)"
                            % (slope, c, g, _act32(beta[c], slope), yh[g, 0, c]))
                rep.require(mh[g, c] == np.float32(BR.CONST) and ih[g, c] == inv0 and (vh is None or vh[g, c] == 0.0),
                            "slope=%s: const channel %d of group %d: mean %r invstd %r (want %r) unbiased variance %r"
                            % (slope, c, g, mh[g, c], ih[g, c], inv0, None if vh is None else vh[g, c]))
                if G == 1:
                    want_rv = np.float32(np.float32(1.0) - np.float32(MOM)) * run0[1][c]
                    rep.require(rvh[c] == want_rv, "slope=%s: const channel %d: running_var %r, want fl32(fl32(1 - m) old) = %r" % (slope, c, rvh[c], want_rv))

    # ----------------------------------------------------------------------------------------------------------------- backward
    yb, mf, inv = BR.backward_inputs(z, gamma, beta, slope)
    ybd, mfd, invd = lay.up(yb), _cuda(mf), _cuda(inv)
    b = BR.backward_ref(z, yb, case["dy"], mf, inv, gamma, slope)
    dx, dgamma, dbeta = lay.bwd(dyd, ybd, xd, rd, gd, mfd, invd, slope)
    rep.check("dx", lay.down(dx), b["dx"], b["dx_bound"], fams, slope)
    rep.check("dgamma", dgamma.cpu().numpy(), b["dgamma"], b["dgamma_bound"], fams, slope)
    rep.check("dbeta", dbeta.cpu().numpy(), b["dbeta"], b["dbeta_bound"], fams, slope)
    dx2, dg2, db2 = lay.bwd(dyd, ybd, xd, rd, gd, mfd, invd, slope)
    rep.require(_same_bits(dx, dx2) and _same_bits(dgamma, dg2) and _same_bits(dbeta, db2), "slope=%s: the backward differs between two identical calls" % slope)
    if isinstance(lay, _Pm):        # accumulate = 1 into prefilled buffers
        pre = rng.standard_normal(C).astype(np.float32), (100 * rng.standard_normal(C)).astype(np.float32)
        grads = _cuda(pre[0]), _cuda(pre[1])
        b = BR.backward_ref(z, yb, case["dy"], mf, inv, gamma, slope, prefilled=pre)
        dx3, dg3, db3 = lay.bwd(dyd, ybd, xd, rd, gd, mfd, invd, slope, grads=grads)
        rep.require(dg3.data_ptr() == grads[0].data_ptr() and _same_bits(dx3, dx), "slope=%s: accumulate = 1 changed dx or did not use the buffers" % slope)
        rep.check("dgamma (accumulate)", dg3.cpu().numpy(), b["dgamma"], b["dgamma_bound"], fams, slope)
        rep.check("dbeta (accumulate)", db3.cpu().numpy(), b["dbeta"], b["dbeta_bound"], fams, slope)
        if G == 1:
            dx4, dg4, db4 = lay.ops.bn_act_train_bwd_pm(dyd, ybd, xd, rd, gd, mfd.view(-1), invd.view(-1), slope)
            rep.require(_same_bits(dx4, dx) and _same_bits(dg4, dgamma) and _same_bits(db4, dbeta),
                        "slope=%s: dvm_bn_act_train_bwd_pm_f32 differs from the groups = 1 call" % slope)


# --------------------------------------------------------------------------------------------------------------------------- tests
def test_no_process_group():
    assert _NO_PROCESS_GROUP_AT_COLLECTION and not torch.distributed.is_initialized()


@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("B,C,N", BR.CM_CASES)
def test_channel_major_per_element(ops, B, C, N, with_res):
    rep = _Report("channel-major", "(B=%d, C=%d, N=%d)%s" % (B, C, N, " + res" if with_res else ""), BR.cm_route(B, C, N))
    for k, slope in enumerate(BR.SLOPES):
        _run_case(rep, _Cm(ops, B, C, N), BR.make_case(1, B * N, C, seed=1, with_res=with_res, dy_shift=k), slope, seed=k)
    rep.finish()


@pytest.mark.parametrize("R,C", BR.PM_CASES)
def test_point_major_per_element(ops, R, C):
    """slope 0.2 runs with a residual, slopes 1 and 0 without (the exact checks of the constant channel need z = x)"""
    rep = _Report("point-major", "(R=%d, C=%d)" % (R, C), BR.pm_route(R, C))
    for k, slope in enumerate(BR.SLOPES):
        _run_case(rep, _Pm(ops, 1, R, C), BR.make_case(1, R, C, seed=2, with_res=slope == 0.2, dy_shift=k), slope, seed=k)
    rep.finish()


@pytest.mark.parametrize("R,C,G", BR.GROUP_CASES)
def test_groups_per_element(ops, R, C, G):
    rep = _Report("groups", "(R=%d per group, C=%d, groups=%d)" % (R, C, G), BR.pm_route(R, C))
    for k, slope in enumerate(BR.SLOPES):
        _run_case(rep, _Pm(ops, G, R, C), BR.make_case(G, R, C, seed=3, with_res=slope == 0.2, dy_shift=k), slope, seed=k)
    rep.finish()


@pytest.mark.parametrize("G", [0, 65])
def test_bad_group_count_raises_and_writes_nothing(ops, G):
    from dvm._lib import DvmError
    R, C = 5, 12
    rows = R * max(G, 1)
    g = torch.Generator().manual_seed(G)
    x, dy = torch.randn(rows, C, generator=g).cuda(), torch.randn(rows, C, generator=g).cuda()
    gamma, beta = torch.ones(C).cuda(), torch.zeros(C).cuda()
    stats = torch.ones(max(G, 1), C).cuda()
    outs = [torch.full((rows, C), SENTINEL).cuda(), torch.full((C,), SENTINEL).cuda(), torch.full((C,), SENTINEL).cuda()]
    with pytest.raises(DvmError, match="group count"):
        ops.bn_act_train_fwd_pm_groups(x, None, gamma, beta, EPS, 0.2, MOM, G, want_var=True, running_mean=outs[1], running_var=outs[2], y=outs[0])
    with pytest.raises(DvmError, match="group count"):
        ops.bn_act_train_bwd_pm_groups(dy, x, x, None, gamma, stats, stats, 0.2, G, grads=(outs[1], outs[2]), dx=outs[0])
    torch.cuda.synchronize()
    assert all(bool((o == SENTINEL).all()) for o in outs), "a refused call wrote to its outputs"


@pytest.mark.parametrize("slope", BR.SLOPES)
def test_one_row_and_one_element_agree(ops, slope):
    """R = 1 point-major and B * N = 1 channel-major are the same four floats: the same y = act(beta), a finite running variance"""
    C = 4
    x = _cuda(np.array([[3.0, -7.5, 1e4, 0.0]], np.float32))
    gamma, beta = _cuda(np.array([1.5, 0.0, -2.0, 0.7], np.float32)), _cuda(np.array([0.25, -1.0, 0.0, -3.0], np.float32))
    rv0 = np.array([0.5, 1.0, 2.0, 4.0], np.float32)
    rm_p, rv_p, rm_c, rv_c = torch.zeros(C).cuda(), _cuda(rv0), torch.zeros(C).cuda(), _cuda(rv0)
    yp, mp, ip = ops.bn_act_train_fwd_pm(x, None, gamma, beta, EPS, slope, MOM, rm_p, rv_p)
    yc, mc, ic = ops.bn_act_train_fwd(x.view(1, C, 1), None, gamma, beta, EPS, slope, MOM, rm_c, rv_c)
    want = torch.from_numpy(np.array([_act32(b, slope) for b in beta.cpu().numpy()], np.float32)).cuda()
    assert _same_bits(yp.view(-1), want) and _same_bits(yc.view(-1), want), (yp, yc, want)
    assert _same_bits(mp, mc) and _same_bits(ip, ic) and _same_bits(mp, x.view(-1))
    assert bool(torch.isfinite(rv_p).all()) and _same_bits(rv_p, rv_c) and _same_bits(rm_p, rm_c)
    assert np.array_equal(rv_p.cpu().numpy(), np.float32(np.float32(1.0) - np.float32(MOM)) * rv0)


# ------------------------------------------------------------------------------------------------ the cross-rank form, in one process
class _OtherRank:
    """A dvm_collective whose all-reduce adds `addend` (the other rank's totals and row counts, float64 on the device) to the
    buffer it is handed, on the stream it is handed.  It checks the pointer, the count, the type and the operation; no exception
    crosses the C boundary: `error` keeps it and the callback answers -1."""

    def __init__(self, buf, addend, count, fail=False):
        from dvm import dist as D
        self.buf, self.addend, self.count, self.fail, self.calls, self.error = buf, addend, count, fail, [], None
        self._fn = D._ALLREDUCE_FN(self._allreduce)
        self.struct = D._CollectiveStruct(self._fn, None)
        self._ptr = ctypes.pointer(self.struct)

    def ptr(self):
        return ctypes.cast(self._ptr, ctypes.c_void_p)

    def _allreduce(self, user, buf, count, dtype, op, stream):
        try:
            self.calls.append(int(count))
            if self.fail:
                return -1
            if int(buf) != self.buf.data_ptr() or int(count) != self.count or dtype != 1 or op != 0:
                raise RuntimeError("collective called with buf=%r count=%r dtype=%r op=%r" % (buf, count, dtype, op))
            st = torch.cuda.ExternalStream(int(stream)) if stream else torch.cuda.default_stream()
            with torch.cuda.stream(st):
                self.buf[:self.count] += self.addend
            return 0
        except Exception as e:  # noqa: BLE001
            self.error = e
            return -1


def _sync_buf(C, G):
    from dvm import _lib
    return torch.zeros(_lib.load().dvm_bn_pm_sync_bytes(C, G) // 8, dtype=torch.float64, device="cuda")


@pytest.mark.parametrize("R,C,G", BR.SYNC_CASES)
def test_sync_form_in_one_process(ops, R, C, G):
    from dvm._lib import DvmError
    assert not torch.distributed.is_initialized()
    rep = _Report("sync", "(R=%d per group, C=%d, groups=%d)" % (R, C, G), BR.pm_route(R, C))
    count, R1 = G * C * 2 + G, R + 3
    lay = _Pm(ops, G, R, C)
    for k, slope in enumerate(BR.SLOPES):
        mine = BR.make_case(G, R, C, seed=30, with_res=slope == 0.2, dy_shift=k)
        other = BR.make_case(G, R1, C, seed=9, with_res=slope == 0.2, dy_shift=k)     # (seeds: the same family per channel on both ranks)
        assert mine["fams"] == other["fams"]
        z, gamma, beta, fams = mine["z"], mine["gamma"], mine["beta"], mine["fams"]
        other["gamma"], other["beta"] = gamma, beta
        zall = np.concatenate([z, other["z"]], 1)
        rng = np.random.default_rng([k, R, C, G])
        run0 = rng.standard_normal(C).astype(np.float32), rng.uniform(0.5, 2.0, C).astype(np.float32)
        xd, rd, gd, bd, dyd = lay.up(mine["x"]), lay.up(mine["res"]), _cuda(gamma), _cuda(beta), lay.up(mine["dy"])
        buf = _sync_buf(C, G)
        zero = torch.zeros(count, dtype=torch.float64, device="cuda")

        def fwd(coll):
            rm, rv = _cuda(run0[0]), _cuda(run0[1])
            out = ops.bn_act_train_fwd_pm_sync(xd, rd, gd, bd, EPS, slope, MOM, G, None if coll is None else coll.ptr(), buf, want_var=True,
                                               running_mean=rm, running_var=rv)
            assert coll is None or coll.error is None, coll.error
            return out + (rm, rv)

        # a zero addend: the plain call, bit for bit
        coll0 = _OtherRank(buf, zero, count)
        plain, synced = fwd(None), fwd(coll0)
        rep.require(all(_same_bits(a, b) for a, b in zip(plain, synced)), "slope=%s: the forward with a zero addend differs from the plain call" % slope)
        rep.require(coll0.calls == [count], "slope=%s: the forward's collective saw the counts %r, want [%d]" % (slope, coll0.calls, count))
        # the other rank's totals: the reference on both ranks' rows
        coll = _OtherRank(buf, _cuda(BR.rank_totals(other["z"])), count)
        y, mean, invstd, var, rm, rv = fwd(coll)
        f = BR.forward_ref(z, gamma, beta, slope, stats_of=zall)
        assert f["n"] == R + R1
        rep.check("y", lay.down(y), f["y"], f["y_bound"], fams, slope)
        rep.check("save_mean", mean.cpu().numpy(), f["mean"], f["mean_bound"], fams, slope)
        rep.check("save_invstd", invstd.cpu().numpy(), f["invstd"], f["invstd_bound"], fams, slope)
        rep.check("save_var_unbiased (global row count)", var.cpu().numpy(), f["unb"], f["unb_bound"], fams, slope)
        want, bound = BR.running_ref(run0[0], f["mean"], f["mean_bound"])
        rep.check("running_mean", rm.cpu().numpy(), want, bound, fams, slope)
        want, bound = BR.running_ref(run0[1], f["unb"], f["unb_bound"])
        rep.check("running_var", rv.cpu().numpy(), want, bound, fams, slope)
        # a collective that fails: the call raises
        bad = _OtherRank(buf, zero, count, fail=True)
        with pytest.raises(DvmError, match="all-reduce failed"):
            fwd(bad)
        torch.cuda.synchronize()
        rep.require(bad.calls == [count], "slope=%s: the failing collective saw the counts %r" % (slope, bad.calls))

        # backward: y / mean / invstd of the test's making, from the statistics of both ranks' rows
        yb, mf, inv = BR.backward_inputs(z, gamma, beta, slope, stats_of=zall)
        y1 = BR.forward_ref(other["z"], gamma, beta, slope, stats_of=zall)["y"].astype(np.float32)
        ybd, mfd, invd = lay.up(yb), _cuda(mf), _cuda(inv)

        def bwd(coll):
            out = ops.bn_act_train_bwd_pm_sync(dyd, ybd, xd, rd, gd, mfd, invd, slope, G, None if coll is None else coll.ptr(), buf)
            assert coll is None or coll.error is None, coll.error
            return out

        coll0 = _OtherRank(buf, zero, count)
        plain, synced = bwd(None), bwd(coll0)
        rep.require(all(_same_bits(a, b) for a, b in zip(plain, synced)), "slope=%s: the backward with a zero addend differs from the plain call" % slope)
        rep.require(coll0.calls == [count], "slope=%s: the backward's collective saw the counts %r, want [%d]" % (slope, coll0.calls, count))
        coll = _OtherRank(buf, _cuda(BR.rank_totals(other["z"], bwd=(y1, other["dy"], mf, inv, slope))), count)
        dx, dgamma, dbeta = bwd(coll)
        b = BR.backward_ref(z, yb, mine["dy"], mf, inv, gamma, slope, other=(other["z"], y1, other["dy"]))
        rep.check("dx", lay.down(dx), b["dx"], b["dx_bound"], fams, slope)
        rep.check("dgamma (local sums)", dgamma.cpu().numpy(), b["dgamma"], b["dgamma_bound"], fams, slope)
        rep.check("dbeta (local sums)", dbeta.cpu().numpy(), b["dbeta"], b["dbeta_bound"], fams, slope)
        bad = _OtherRank(buf, zero, count, fail=True)
        with pytest.raises(DvmError, match="all-reduce failed"):
            bwd(bad)
        torch.cuda.synchronize()
    assert not torch.distributed.is_initialized()
    rep.finish()
