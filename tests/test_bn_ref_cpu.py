"""The reference that tests/test_gpu_bn_elements.py holds the fused training BatchNorm to (tests/bn_ref.py), checked where no GPU
is needed: against torch's batch_norm + leaky_relu under fp64 autograd, against a float32 emulation of the kernels' operation
sequence (every bound must hold, and must FAIL under a planted error), and for the launch routes its case lists reach."""
import numpy as np
import pytest
import torch

import bn_ref as BR

NS = (1, 2, 7, 37, 1000, 4096, 40000)
C9 = len(BR.FAMILIES)


def _torch_reference(z, gamma, beta, slope, dy, run):
    """One group: z, dy [n][C] float64 -> y, dz/dx, dgamma, dbeta, running statistics by torch in fp64."""
    zt = torch.from_numpy(z).requires_grad_(True)
    g = torch.from_numpy(gamma.astype(np.float64)).requires_grad_(True)
    b = torch.from_numpy(beta.astype(np.float64)).requires_grad_(True)
    t = torch.nn.functional.batch_norm(zt, run[0], run[1], g, b, True, float(np.float32(BR.MOMENTUM)), float(np.float32(BR.EPS)))
    y = torch.nn.functional.leaky_relu(t, float(np.float32(slope)))
    y.backward(torch.from_numpy(dy))
    return y.detach().numpy(), zt.grad.numpy(), g.grad.numpy(), b.grad.numpy()


def _rel(a, b, axis=None):
    """max |a - b| over the channel's own scale (axis 0 = rows), floored at 1"""
    scale = np.maximum(np.abs(b).max(axis=axis, keepdims=axis is not None), 1.0)
    return float((np.abs(a - b) / scale).max())


@pytest.mark.parametrize("groups", [1, 3])
@pytest.mark.parametrize("slope", BR.SLOPES)
def test_reference_equals_torch_fp64(groups, slope):
    """y, dx, dgamma, dbeta and the running statistics, to 1e-12 of each channel's scale; 3 groups = 3 torch calls that share the
    running statistics and whose parameter gradients add up."""
    n, C = 38, 18       # (an even count: no row of the ramp or the +-1 channel IS its mean, where beta = 0 would put t on the kink)
    case = BR.make_case(groups, n, C, seed=5)
    z, gamma, beta = case["z"], case["gamma"], case["beta"].copy()
    for c in range(C):      # a constant channel with beta = 0 has t = 0 exactly: which slope torch's own rounding of the mean picks there
        if beta[c] == 0 and any(case["fams"][g][c] == "const" for g in range(groups)):      # is not this reference's business
            beta[c] = 0.5
    assert (beta == 0).any()
    f = BR.forward_ref(z, gamma, beta, slope)
    b = BR.backward_ref(z, f["y"], case["dy"], f["mean"], f["invstd"], gamma, slope)   # fp64 y / mean / invstd: nothing rounded
    run0 = np.linspace(-1, 1, C), np.linspace(0.5, 2, C)
    run = tuple(torch.from_numpy(r.copy()) for r in run0)
    dg, db = np.zeros(C), np.zeros(C)
    for g in range(groups):
        y, dx, dgam, dbet = _torch_reference(z[g].astype(np.float64), gamma, beta, slope, case["dy"][g].astype(np.float64), run)
        assert _rel(f["y"][g], y, 0) <= 1e-12, ("y", g, _rel(f["y"][g], y, 0))
        assert _rel(b["dx"][g], dx, 0) <= 1e-12, ("dx", g, _rel(b["dx"][g], dx, 0))
        dg, db = dg + dgam, db + dbet
    # (the parameter gradients of the reference are rounded to fp32 group by group: compare its fp64 sums)
    assert _rel(b["S2"].sum(0), dg, None) <= 1e-12 and _rel(b["S1"].sum(0), db, None) <= 1e-12
    rm, _ = BR.running_ref(run0[0], f["mean"], np.zeros_like(f["mean"]), fp32_constants=False)
    rv, _ = BR.running_ref(run0[1], f["unb"], np.zeros_like(f["unb"]), fp32_constants=False)
    assert _rel(rm, run[0].numpy()) <= 1e-12 and _rel(rv, run[1].numpy()) <= 1e-12


def _emulation_ratios(n, slope, fma, plant=None, groups=2):
    """-> {(output, family): largest error / bound} of the emulation against the reference, every family in every group"""
    C = C9
    case = BR.make_case(groups, n, C, seed=11, with_res=False, dy_shift=n % 3)
    z, gamma, beta, dy = case["z"], case["gamma"], case["beta"], case["dy"]
    rng = np.random.default_rng(n)
    run0 = rng.standard_normal(C).astype(np.float32), rng.uniform(0.5, 2.0, C).astype(np.float32)
    f = BR.forward_ref(z, gamma, beta, slope)
    e = BR.emulate_forward(z, gamma, beta, slope, fma=fma, running=run0, plant=plant)
    out = {}

    def put(name, got, want, bound):
        for g in range(groups):
            for c in range(C):
                key = (name, case["fams"][g][c]) if np.ndim(want) > 1 else (name, "ch%d" % c)
                r = BR.worst(np.asarray(got)[g][..., c] if np.ndim(want) > 1 else np.asarray(got)[c],
                             np.asarray(want)[g][..., c] if np.ndim(want) > 1 else np.asarray(want)[c],
                             np.asarray(bound)[g][..., c] if np.ndim(want) > 1 else np.asarray(bound)[c])[0]
                out[key] = max(out.get(key, 0.0), r)

    put("mean", e["mean"], f["mean"], f["mean_bound"])
    put("invstd", e["invstd"], f["invstd"], f["invstd_bound"])
    put("unb", e["unb"], f["unb"], f["unb_bound"])
    put("y", e["y"], f["y"], f["y_bound"])
    for name, r0, batch, bb in (("running_mean", run0[0], f["mean"], f["mean_bound"]), ("running_var", run0[1], f["unb"], f["unb_bound"])):
        want, bound = BR.running_ref(r0, batch, bb)
        put(name, e[name], want, bound)
    y, mf, inv = BR.backward_inputs(z, gamma, beta, slope)
    pre = rng.standard_normal(C).astype(np.float32), (100 * rng.standard_normal(C)).astype(np.float32)
    for prefilled in (None, pre):
        b = BR.backward_ref(z, y, dy, mf, inv, gamma, slope, prefilled=prefilled)
        eb = BR.emulate_backward(z, y, dy, mf, inv, gamma, slope, fma=fma, plant=plant, prefilled=prefilled)
        put("dx", eb["dx"], b["dx"], b["dx_bound"])
        put("dgamma", eb["dgamma"], b["dgamma"], b["dgamma_bound"])
        put("dbeta", eb["dbeta"], b["dbeta"], b["dbeta_bound"])
    # the const channel: y = act(beta) bit for bit
    for g in range(groups):
        for c in range(C):
            if case["fams"][g][c] == "const" and plant is None:
                bt = beta[c]
                assert np.array_equal(e["y"][g, :, c], np.full(n, bt if bt > 0 else bt * np.float32(slope), np.float32))
    return out


def test_emulation_stays_inside_every_bound():
    worst = {}
    for n, groups in [(n, 2) for n in NS] + [(3, 64)]:
        for slope in BR.SLOPES:
            for fma in (False, True):
                for key, r in _emulation_ratios(n, slope, fma, groups=groups).items():
                    if r > worst.get(key, (0.0,))[0]:
                        worst[key] = (r, n, slope, fma)
    fwd = max(v[0] for k, v in worst.items() if k[0] in ("mean", "invstd", "unb", "y", "running_mean", "running_var"))
    bwd = max(v[0] for k, v in worst.items() if k[0] in ("dx", "dgamma", "dbeta"))
    table = "\n".join("%-12s %-12s ratio %.3f at n=%d slope=%g fma=%s" % (k + v) for k, v in sorted(worst.items()))
    print("largest error / bound: forward %.3f, backward %.3f\n%s" % (fwd, bwd, table))
    assert max(fwd, bwd) <= 1.0, "the emulation leaves a bound (largest ratio per output and family):\n" + table


@pytest.mark.parametrize("plant,outputs", [
    ("drop_last_row", ("mean", "y", "dbeta", "dx")),
    ("biased_running", ("running_var", "unb")),
    ("other_group_stats", ("y",)),
    ("ge_zero", ("dx", "dbeta")),
    ("s1_for_s2", ("dx",)),
])
def test_bounds_fail_under_a_planted_error(plant, outputs):
    """each planted error leaves the bound of at least one element of every named output by a factor of 100 or more"""
    got = {}
    for n in (2, 7, 37):
        for slope in (0.2, 0.0):
            for key, r in _emulation_ratios(n, slope, False, plant=plant).items():
                got[key[0]] = max(got.get(key[0], 0.0), r)
    assert all(got[o] >= 100.0 for o in outputs), (plant, {o: got[o] for o in outputs})


def test_case_lists_reach_every_route():
    pm = [BR.pm_route(R, C) for R, C in BR.PM_CASES]
    sets = {f: sorted(set(getattr(r, f) for r in pm), key=str) for f in BR.PmRoute._fields}
    print("point-major routes:", sets)
    assert sets["cg"] == ["128", "64", "row"]
    assert sets["rpp"] == [1, 16, 256, 3, 51, 8, 85]              # (sorted as strings) C = 516 / 1000, 64 / 192, 4, 260, 20, 128 / 1024, 12
    assert sets["idle"] == [False, True] and sets["doubled"] == [False, True]
    assert sets["splits_class"] == ["1", "2-32", ">32"]
    assert sets["rem4"] == [0, 1, 2, 3]
    assert 1 in sets["last_rows"] and any(r.last_rows == 4 * r.rpp - 1 for r in pm)    # a one-row last chunk, one short of a row
    # the whole-row branch at every lane count the issue names, the staging arrays to their last element (C = 4: 256 rows x 4)
    assert {(r.rpp, r.idle) for r, (R, C) in zip(pm, BR.PM_CASES) if r.cg == "row"} == {(256, False), (85, True), (51, True), (3, True), (1, True)}
    assert all(any(r.doubled and r.cg == c for r in pm) for c in ("128", "64", "row"))
    for R, C, G in BR.GROUP_CASES + BR.SYNC_CASES:
        assert 1 <= G <= 64 and C % 4 == 0
    cm = [BR.cm_route(*c) for c in BR.CM_CASES]
    csets = {f: sorted(set(getattr(r, f) for r in cm)) for f in BR.CmRoute._fields}
    print("channel-major routes:", csets)
    assert csets["S"] == [1, 2, 16, 64]
    assert csets["vector"] == [False, True] and csets["last_short"] == [False, True] and csets["below_block"] == [False, True]
    assert BR.cm_route(1, 1, 1).below_block and BR.cm_route(1, 1, 65539) == BR.CmRoute(64, False, True, False)


def test_every_family_is_drawn():
    """every case with C >= 9 holds every family; with groups, no two neighbouring groups give a channel the same family"""
    for R, C in BR.PM_CASES:
        if C >= C9:
            assert {BR.family_of(c, 0, (7 * R + C) % C9) for c in range(C)} == set(BR.FAMILIES)
    for g in range(63):
        assert all(BR.family_of(c, g) != BR.family_of(c, g + 1) for c in range(C9))
