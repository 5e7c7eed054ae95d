"""CPU half of the per-element checks of the geometric loss backward (device half: tests/test_gpu_geom_backward_rows.py; plantings:
tests/exact_inputs.py; references, bounds, families and restatements: tests/geom_backward_ref.py).  It proves without a GPU that the
device tests can fail, and only for a reason:

(1) the plantings are exact: every addend is a multiple of 2^-4 and every element's summed magnitudes stay below 2^20, so every
    partial sum in every order has at most 24 bits (exact_inputs.exact_sums); the rot6d plantings keep every intermediate of the
    backward exact;
(2) fp32 numpy restatements of the kernels' definitions — one rounding per operation, scatter sums accumulated in a shuffled order —
    pass every check of the device half: bit equality on the plantings, the derived bound 2 u (n + c) A on the real-valued families,
    the bar ROT6D_C u s per rot6d row (and ROT6D_C is reproduced from its recipe);
(3) the bounds are not vacuous: at N >= 64, for every family but `rigid` and `self`, at least 90 % of a case's output elements
    (d_R and d_T, resp. d_a and d_b, together) have a bound <= 1e-3 |ref|;
(4) each planted mutation of the restatements fails at least one check, reported by name."""
import functools
import math

import numpy as np
import pytest

import exact_inputs as X
import geom_backward_ref as G
from oracle import oracle as O


def _oracle_dg_build(xyz, start):
    return O.dg_build(xyz, start)


def _oracle_nn(a, b):
    return O.chamfer(a, b)[2:]


@functools.lru_cache(maxsize=None)
def _warp_family(family, N):
    return G.warp_family(family, N, _oracle_dg_build)


@functools.lru_cache(maxsize=None)
def _chamfer_family(family, N, M):
    return G.chamfer_family(family, N, M, _oracle_nn)


@functools.lru_cache(maxsize=None)
def _criterion_case(N, M, hi, swapped=False):
    _, cases = X.planted_batch(N, M, X.PAIR_SEED, both=swapped, hi=hi)
    refs = [c[1] for c in cases] + ([c[2] for c in cases] if swapped else [])
    ga = [(N // 2) / 8.0 * (1, -1)[p % 2] for p in range(len(refs))]
    return refs, ga, X.criterion_bwd_reference(refs, ga)


# ---------------------------------------------------------------------------------------------- the checks, on any implementation
def check_warp_exact(N, hub, mut=None):
    cases = X.warp_bwd_batch(N, hub)
    dR, dT = G.warp_arap_bwd_batch_np(cases, mut=mut)
    for b, c in enumerate(cases):
        G.check_equal("d_T entry %d" % b, dT[b], c["d_T"])
        G.check_equal("d_R entry %d" % b, dR[b], c["d_R"])


def check_chamfer_exact(shape, variant, mut=None):
    cases = X.chamfer_bwd_batch(*shape, variant)
    da, db = G.chamfer_bwd_batch_np(cases, mut=mut)
    for b, c in enumerate(cases):
        G.check_equal("d_a entry %d" % b, da[b], c["d_a"])
        G.check_equal("d_b entry %d" % b, db[b], c["d_b"])


def check_rot6d_exact(mut=None):
    r = X.rot6d_bwd_direct(X.BWD_SEED)
    G.check_equal("rot6d_bwd", G.rot6d_bwd_np(r["d6"], r["gR"], mut=mut), r["grad"])


def check_criterion_exact(case, swapped=False, mut=None):
    refs, ga, cr = _criterion_case(*case, swapped)
    db3, dW3 = G.criterion_bwd_np(refs, ga, mut=mut)
    G.check_equal("d b3", db3, cr["db3"])
    G.check_equal("d W3[:, :3]", dW3, cr["dW3"])


def check_warp_bound(family, N, mut=None):
    cases, ref = _warp_family(family, N)
    dR, dT = G.warp_arap_bwd_batch_np(cases, mut=mut)
    G.check_bound("d_T", dT, ref["d_T"], ref["bound_T"])
    G.check_bound("d_R", dR, ref["d_R"], ref["bound_R"])


def check_chamfer_bound(family, N, M, mut=None):
    cases, ref = _chamfer_family(family, N, M)
    da, db = G.chamfer_bwd_batch_np(cases, mut=mut)
    G.check_bound("d_a", da, ref["d_a"], ref["bound_a"])
    G.check_bound("d_b", db, ref["d_b"], ref["bound_b"])


def check_rot6d_bound(family, mut=None):
    d6, gR, ref, bar = G.rot6d_case(family)
    G.check_bound("rot6d_bwd", G.rot6d_bwd_np(d6, gR, mut=mut), ref, bar)


# ------------------------------------------------------------------------------------------------------------ (1) exact plantings
@pytest.mark.parametrize("hub", [False, True], ids=["plain", "hub"])
@pytest.mark.parametrize("N", X.BWD_SIZES)
def test_warp_planting_is_exact_and_restatement_equals_it(N, hub):
    cases = X.warp_bwd_batch(N, hub)
    for c in cases:
        assert X.exact_sums(c["addends"], (c["mag_R"], c["mag_T"]))
    assert [float(c["ga"]) * 8 / (N // 2) for c in cases] == [1.0, -1.0, 0.0]
    if hub:
        assert (np.bincount(cases[0]["infl_idx"].ravel(), minlength=N // 2)[0] >= 2 * N)
    check_warp_exact(N, hub)
    if N >= 64:
        assert all(np.count_nonzero(c["d_T"]) > 0.8 * c["d_T"].size for c in cases[:2])      # (entry 2: g_arap = 0, warp alone)


def test_rot6d_planting_is_exact_and_restatement_equals_it():
    r = X.rot6d_bwd_direct(X.BWD_SEED)
    a1, a2 = r["d6"][:, :3].astype(np.float64), r["d6"][:, 3:].astype(np.float64)
    orient = {(int(np.flatnonzero(x)[0]), float(np.sign(x[np.flatnonzero(x)[0]])), int(np.argmax(np.abs(y - (x @ y) / (x @ x) * x))),
               float(np.sign((y - (x @ y) / (x @ x) * x)[np.argmax(np.abs(y - (x @ y) / (x @ x) * x))]))) for x, y in zip(a1, a2)}
    assert len(orient) == 24
    trace = []
    out64 = G.rot6d_bwd_np(r["d6"], r["gR"], np.float64, trace=trace)
    for t in trace:       # every intermediate of the backward is representable in fp32, with bits to spare for another association
        assert np.array_equal(t.astype(np.float32).astype(np.float64), t) and np.array_equal(t * 2.0 ** 12, np.rint(t * 2.0 ** 12)) and (np.abs(t) < 2.0 ** 10).all()
    assert np.array_equal(out64, r["grad"])       # the analytic restatement == float64 autograd of the definition, exactly
    check_rot6d_exact()


@pytest.mark.parametrize("variant", X.CHAMFER_VARIANTS)
@pytest.mark.parametrize("shape", X.CHAMFER_BWD_SHAPES, ids=lambda s: "%dx%d" % s)
def test_chamfer_planting_is_exact_and_restatement_equals_it(shape, variant):
    for c in X.chamfer_bwd_batch(*shape, variant):
        assert X.exact_sums(c["addends"], (c["mag_a"], c["mag_b"]))
        if variant == "nn":       # true arg-mins
            D = ((c["a"].astype(np.float64)[:, None] - c["b"].astype(np.float64)[None]) ** 2).sum(-1)
            assert np.array_equal(D[np.arange(shape[0]), c["i1"]], D.min(1)) and np.array_equal(D[c["i2"], np.arange(shape[1])], D.min(0))
    check_chamfer_exact(shape, variant)


@pytest.mark.parametrize("case", X.CRIT_BWD_CASES + [X.CRIT_BWD_SWAPPED], ids=lambda c: "x".join(map(str, c)))
def test_criterion_planting_is_exact_and_restatement_equals_it(case):
    swapped = len(case) == 2
    case = (case[0], case[0], case[1]) if swapped else case
    refs, ga, cr = _criterion_case(*case, swapped)
    assert X.exact_sums(cr["addends"], (cr["mag_b3"], cr["mag_W3"]))
    assert np.abs(cr["db3"]).max() > 0 and (np.abs(cr["dW3"]).max(1) > 0).sum() >= 6
    check_criterion_exact(case, swapped)


def test_criterion_planting_at_full_coordinate_range_would_not_be_exact():
    """why hi shrank: at the forward plantings' range [0, 255] the weight gradient's sums leave 24 bits"""
    refs, ga, cr = _criterion_case(300, 170, 255)
    assert not X.exact_sums(cr["addends"], (cr["mag_b3"], cr["mag_W3"]))


# ----------------------------------------------------------------------------------------------- (2), (3) real-valued families
@pytest.mark.parametrize("N", G.WARP_SIZES)
@pytest.mark.parametrize("family", G.WARP_FAMILIES)
def test_warp_restatement_within_bound_and_bound_not_vacuous(family, N):
    check_warp_bound(family, N)
    cases, ref = _warp_family(family, N)
    if family not in G.VACUITY_EXEMPT:
        frac = G.nonvacuous_fraction(np.concatenate([ref["d_R"].ravel(), ref["d_T"].ravel()]), np.concatenate([ref["bound_R"].ravel(), ref["bound_T"].ravel()]))
        assert frac >= 0.9, frac
    if family == "rigid":     # the residual is rounding noise: the ARAP part of the reference is ~1e-7 of its envelope
        z = [dict(c, gw=np.zeros_like(c["gw"])) for c in cases]
        r = G.warp_arap_reference(z)
        assert np.abs(r["d_T"]).max() < 1e-5 * (r["bound_T"] / G.U).max()
    if family == "hub":
        assert np.bincount(cases[0]["infl_idx"].ravel())[0] >= 2 * N


@pytest.mark.parametrize("shape", X.CHAMFER_BWD_SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("family", G.CHAMFER_FAMILIES)
def test_chamfer_restatement_within_bound_and_bound_not_vacuous(family, shape):
    N, M = (shape[0], shape[0]) if family == "self" else shape
    check_chamfer_bound(family, N, M)
    cases, ref = _chamfer_family(family, N, M)
    if family == "self":
        assert not ref["d_a"].any() and not ref["bound_a"].any() and not ref["bound_b"].any()
    elif N >= 64:
        frac = G.nonvacuous_fraction(np.concatenate([ref["d_a"].ravel(), ref["d_b"].ravel()]), np.concatenate([ref["bound_a"].ravel(), ref["bound_b"].ravel()]))
        assert frac >= 0.9, frac


@pytest.mark.parametrize("family", G.ROT6D_FAMILIES)
def test_rot6d_restatement_within_bar(family):
    check_rot6d_bound(family)
    d6, gR, ref, bar = G.rot6d_case(family)
    n = np.linalg.norm(d6.astype(np.float64).reshape(-1, 2, 3), axis=2)
    assert n.min() > 1e-6        # nowhere near the 1e-12 clamp


def test_rot6d_constant_follows_its_recipe():
    worst, family = G.measure_rot6d_c()
    assert math.ceil(4 * worst) == G.ROT6D_C, (worst, family)


# ------------------------------------------------------------------------------------------------------------------- (4) mutations
def _failed_checks(mut):
    checks = []
    for N in (3, 64, 257):
        for hub in (False, True):
            checks.append(("exact:warp N=%d %s" % (N, "hub" if hub else "plain"), functools.partial(check_warp_exact, N, hub)))
    for shape in [(255, 1), (256, 257), (300, 170)]:
        for v in X.CHAMFER_VARIANTS:
            checks.append(("exact:chamfer %dx%d %s" % (shape + (v,)), functools.partial(check_chamfer_exact, shape, v)))
    checks.append(("exact:rot6d", check_rot6d_exact))
    checks.append(("exact:criterion 64x65", functools.partial(check_criterion_exact, X.CRIT_BWD_CASES[0])))
    for fam in G.WARP_FAMILIES:
        for N in (64, 257):
            checks.append(("bound:warp %s N=%d" % (fam, N), functools.partial(check_warp_bound, fam, N)))
    for fam in G.CHAMFER_FAMILIES:
        for shape in [(256, 257), (300, 170)]:
            N, M = (shape[0], shape[0]) if fam == "self" else shape
            checks.append(("bound:chamfer %s %dx%d" % (fam, N, M), functools.partial(check_chamfer_bound, fam, N, M)))
    for fam in G.ROT6D_FAMILIES:
        checks.append(("bound:rot6d %s" % fam, functools.partial(check_rot6d_bound, fam)))
    failed = []
    for name, fn in checks:
        try:
            fn(mut=mut)
        except AssertionError:
            failed.append(name)
    return failed, len(checks)


def test_unmutated_restatements_pass_the_mutation_suite():
    failed, n = _failed_checks(None)
    assert not failed and n >= 40, failed


# which kernel a mutation lives in: it must be caught by the exact plantings AND by the real-valued bound of that kernel
MUTATION_KERNEL = {"ring8": "warp", "skip_slot2": "warp", "neighbour_R": "warp", "scatter_sign": "warp", "wrong_T": "warp", "hub_drop": "warp",
                   "hub_double": "warp", "ga_entry0": "warp", "skip_last_vertex": "warp", "no_doth": "chamfer", "recompute_idx": "chamfer",
                   "cross_swapped": "rot6d", "no_identity": "criterion"}


@pytest.mark.parametrize("mut", G.MUTATIONS)
def test_mutation_fails_a_check(mut):
    failed, _ = _failed_checks(mut)
    print("%s fails %d checks: %s" % (mut, len(failed), "; ".join(failed)))
    kernel = MUTATION_KERNEL[mut]
    assert any(f.startswith("exact:" + kernel) for f in failed), (mut, failed)
    if kernel != "criterion":          # (the def9 form is reachable through the criterion only: exact plantings alone)
        assert any(f.startswith("bound:" + kernel) for f in failed), (mut, failed)
    assert all(kernel in f or (kernel == "warp" and "criterion" in f) or (kernel == "rot6d" and "criterion" in f) for f in failed), (mut, failed)
