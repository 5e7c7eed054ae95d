"""-m gpu: the HIP path (through the C ABI) against the CPU oracle and the golden vectors.

Bars: integer outputs bit-exact (arg-min / arg-max maps, top-k columns, kNN, FPS, graph
indices); floats within 1e-4 (absolute, the tolerance BASELINE.json's north_star states),
most of them far tighter.
"""
import glob
import zlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import oracle as O

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def names(prefix):
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, prefix + "*.npz")))


@pytest.fixture(scope="module")
def ops():
    from dvm import ops as _ops
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _ops


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def host(t):
    return t.detach().cpu().numpy()


def check_softcorr(ops, f1, f2, alpha, variant, topk=10):
    val, idx, smax, ssum = ops.softcorr(dev(f1)[None], dev(f2)[None], alpha, topk=topk, variant=variant)
    oval, oidx, osmax, osum = O.softcorr(f1, f2, alpha, topk=topk)
    assert np.array_equal(host(idx)[0], oidx), "top-k columns differ from the oracle"
    np.testing.assert_array_equal(host(smax)[0], osmax)
    np.testing.assert_allclose(host(ssum)[0], osum, rtol=2e-5)
    np.testing.assert_allclose(host(val)[0], oval, rtol=5e-5, atol=1e-30)
    return host(val)[0], host(idx)[0]


@pytest.mark.parametrize("variant", [1, 2, 3])
@pytest.mark.parametrize("name", names("softcorr_"))
def test_softcorr_vs_oracle_and_golden(ops, golden, name, variant):
    g = golden(name)
    f1, f2 = g["feat1"][0], g["feat2"][0]
    val, idx = check_softcorr(ops, f1, f2, float(g["alpha"]), variant)
    # against the reference itself
    rv, ri = g["topk_val"][0], g["topk_idx"][0]
    pad = np.pad(rv, ((0, 0), (1, 1)), constant_values=-1.0)
    uniq = (rv != pad[:, :-2]) & (rv != pad[:, 2:]) & (rv > 0)
    assert np.array_equal(idx[uniq], ri[uniq])
    assert np.array_equal(idx[:, 0], ri[:, 0])  # the arg-max correspondence
    np.testing.assert_allclose(val, rv, rtol=0, atol=1e-4)
    v12 = ops.apply(dev(val)[None], dev(idx)[None], dev(g["verts2"]))
    np.testing.assert_allclose(host(v12)[0], g["verts12"][0], rtol=0, atol=1e-5)
    np.testing.assert_array_equal(host(v12)[0], O.apply(val, idx, g["verts2"][0]))


@pytest.mark.parametrize("shape", [(1, 5, 3, 128), (1, 130, 77, 128), (2, 64, 2049, 128), (1, 257, 64, 64), (1, 100, 100, 36)])
def test_softcorr_ragged_shapes(ops, shape):
    """ragged / tiny / non-128 feature sizes, both kernels where applicable."""
    B, N, M, d = shape
    g = torch.Generator().manual_seed(N * 1000 + M)
    f1 = torch.randn(B, N, d, generator=g).numpy()
    f2 = torch.randn(B, M, d, generator=g).numpy()
    for b in range(B):
        for variant in ([1, 2, 3] if d == 128 else [1]):
            check_softcorr(ops, f1[b], f2[b], 25.0, variant)


def test_softcorr_writes_every_output_slot(ops):
    """Fewer columns than topk (M = 5 < 10): the unused positions of every row are defined outputs (value 0, column 0, like
    the oracle's).  The output tensors are handed out by the caching allocator uninitialised, so blocks of exactly their
    sizes are poisoned and released first — a position the kernels leave unwritten then shows as garbage (found when the
    M = 5 case ran first in a process: all empty candidate slots shared one rank and wrote one position)."""
    g = np.random.default_rng(77)
    N, M = 150, 5
    f1, f2 = g.standard_normal((N, 128)).astype(np.float32), g.standard_normal((M, 128)).astype(np.float32)
    for variant in (3, 2, 1):
        junk = [torch.full((1, N, 10), float("nan"), device="cuda"), torch.full((1, N, 10), 0x7f7f7f7f, dtype=torch.int32, device="cuda"),
                torch.full((1, N), float("nan"), device="cuda"), torch.full((1, N), float("nan"), device="cuda")]
        torch.cuda.synchronize()
        del junk
        check_softcorr(ops, f1, f2, 40.0, variant)


@pytest.mark.parametrize("alpha", [33.0, 100.0, 150.0])
def test_softcorr_routed_sweeps_vs_oracle(ops, alpha):
    """Pass A is chosen per launch by the probe (dvm_softcorr_passb.hip::k1_probe_kernel): on the "trained-like" feature set
    (0.3 relu(N(0,1)): tight distance spread) the alphas below take the full and the lean first form; random features at alpha
    100 take the coarse screen (test_pair_forward_full_size_vs_oracle, the bench).  Whatever the route, the result is the
    oracle's: columns exact, values to 5e-5.
    (Which route runs is checked by test_softcorr_probe_routes below; here the results are compared.)"""
    rng = np.random.default_rng(int(alpha))
    f1 = (0.3 * np.maximum(rng.standard_normal((2048, 128)), 0)).astype(np.float32)
    f2 = (0.3 * np.maximum(rng.standard_normal((2048, 128)), 0)).astype(np.float32)
    check_softcorr(ops, f1, f2, alpha, 3)


def test_softcorr_probe_routes():
    """The probe's choice on the two synthetic feature sets of SURVEY 8d, read from the DVM_DEBUG=1 report of a child
    process (the policy is read once per process): random features -> lean first form at alpha 33 (seven columns of a row within
    the cut: more than the coarse screen's list certifies for every row), the coarse screen at 100 and 150; trained-like features
    -> full first form at alpha 33, lean first form at 100 and 150."""
    code = (
        "import os, sys, torch\n"
        "sys.path.insert(0, os.path.join(%r, 'dv-matcher_amd'))\n"
        "from dvm import ops\n"
        "g = torch.Generator().manual_seed(3)\n"
        "for kind in ('randn', 'trained'):\n"
        "    f1, f2 = torch.randn(8, 2048, 128, generator=g).cuda(), torch.randn(8, 2048, 128, generator=g).cuda()\n"
        "    if kind == 'trained': f1, f2 = 0.3 * torch.relu(f1), 0.3 * torch.relu(f2)\n"
        "    for alpha in (33.0, 100.0, 150.0):\n"
        "        ops.softcorr(f1, f2, alpha, topk=10, variant=3)\n"
        "torch.cuda.synchronize()\n" % ROOT)
    env = dict(os.environ, DVM_DEBUG="1")
    env.pop("DVM_K1_ROUTE", None), env.pop("DVM_K1_ROUTE_P", None)
    res = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [ln for ln in res.stderr.splitlines() if ln.startswith("K1 routes:")]
    assert len(lines) == 6, res.stderr[-2000:]
    want = ["0 full, 8 lean, 0 coarse"] + ["0 full, 0 lean, 8 coarse"] * 2 + ["8 full, 0 lean, 0 coarse"] + ["0 full, 8 lean, 0 coarse"] * 2
    for ln, w in zip(lines, want):
        assert w in ln, (ln, w)


@pytest.mark.parametrize("mode", ["sq", "spike", "ragged", "zero"])
def test_pair_forward_fused_preparation_equals_two_pass(ops, golden, mode):
    """The pair path makes the row norms, the absmax and the fp16 planes of the features in ONE pass (rownorm_split_kernel,
    dvm_softcorr_prep.hip) with a provisional scale from a 1/64 sample of the rows, and re-makes the planes only when the true
    absmax has another exponent.  The one-direction entry prepares in two passes (norms + absmax, then the planes): every output of
    the fused call must be that path's, bit for bit — on random features (the sample is right), with one large value in a row the
    sample does not see (the planes are re-made), at a shape whose row counts are no multiples of anything, and for all-zero
    features.  (The planes themselves against a host computation: tools/check_planes.py.)"""
    B, N, M = {"sq": (3, 2048, 2048), "spike": (3, 2048, 2048), "ragged": (2, 1021, 777), "zero": (1, 256, 256)}[mode]
    wl = ops.deformer_weight_list(golden("deformer_scape_r_weights"), "cuda")
    g = torch.Generator().manual_seed(21)
    f1, f2 = torch.randn(B, N, 128, generator=g), torch.randn(B, M, 128, generator=g)
    if mode == "spike":
        f2[1, 33, 7] = 300.0
    if mode == "zero":
        f1, f2 = f1 * 0, f2 * 0
    v1, v2 = torch.rand(B, N, 3, generator=g), torch.rand(B, M, 3, generator=g)
    s = torch.zeros(B, dtype=torch.int32).cuda()
    d = [t.cuda() for t in (f1, f2, v1, v2)]
    o12, o21 = ops.pair_forward(wl, *d, 100.0, s, s)
    r12 = ops.pair_direction(wl, d[0], d[1], d[2], d[3], 100.0, s)
    r21 = ops.pair_direction(wl, d[1], d[0], d[3], d[2], 100.0, s)
    for k in r12:
        assert torch.equal(o12[k], r12[k]) or (torch.isnan(o12[k]) == torch.isnan(r12[k])).all() and torch.equal(torch.nan_to_num(o12[k]), torch.nan_to_num(r12[k])), ("12", k)
        assert torch.equal(o21[k], r21[k]) or (torch.isnan(o21[k]) == torch.isnan(r21[k])).all() and torch.equal(torch.nan_to_num(o21[k]), torch.nan_to_num(r21[k])), ("21", k)


def test_softcorr_duplicate_rows(ops):
    """exact ties (duplicated target features): lowest column first, like the oracle."""
    g = torch.Generator().manual_seed(5)
    f1 = torch.randn(96, 128, generator=g).numpy()
    f2 = torch.randn(70, 128, generator=g).numpy()
    f2 = np.concatenate([f2, f2[:40]], 0)
    for variant in (1, 2, 3):
        check_softcorr(ops, f1, f2, 40.0, variant)


def test_softcorr_large_alpha_and_topk16(ops):
    g = torch.Generator().manual_seed(6)
    f1 = torch.randn(200, 128, generator=g).numpy()
    f2 = torch.randn(300, 128, generator=g).numpy()
    for variant in (1, 2, 3):
        check_softcorr(ops, f1, f2, 101.0, variant)
        if variant != 3:  # the bf16 variant keeps 12 candidates: topk <= 10
            check_softcorr(ops, f1, f2, 10.0, variant, topk=16)
        check_softcorr(ops, f1, f2, 10.0, variant, topk=1)


@pytest.mark.parametrize("name", names("softcorr_"))
def test_argmin_exact(ops, golden, name):
    g = golden(name)
    f1, f2 = g["feat1"][0], g["feat2"][0]
    T, dm = ops.argmin_exact(dev(f1)[None], dev(f2)[None], want_dist=True)
    oT, odm = O.argmin_exact(f1, f2)
    assert np.array_equal(host(T)[0], oT)
    assert np.array_equal(host(dm)[0], odm)
    assert np.array_equal(host(T)[0], g["T12"][0, :, 0])  # the reference's knnsearch_t


@pytest.mark.parametrize("case", ["random", "duplicates", "near_ties", "tiny_M", "ragged", "clustered", "many_equal"])
def test_argmin_screened_equals_full_scan(ops, case):
    """The matrix-core screened hard map is the same function as the all-columns exact-difference scan and the oracle:
    bit-exact indices (ties -> lowest column) and distances, also when whole groups of columns tie."""
    g = torch.Generator().manual_seed(zlib.crc32(case.encode()))
    B, N, M = 2, 300, 257
    f1, f2 = torch.randn(B, N, 128, generator=g), torch.randn(B, M, 128, generator=g)
    if case == "duplicates":
        f2[:, 100:130] = f2[:, 5:6]                       # 31 identical columns: more than the candidate list holds
        f1[:, :40] = f2[:, 5:6] + 1e-3 * torch.randn(B, 40, 128, generator=g)
    elif case == "near_ties":
        f2[:, 1::2] = f2[:, 0::2][:, :M // 2] + 3e-6 * torch.randn(B, M // 2, 128, generator=g)   # pairs of columns ~1 ulp apart
        f1[:, :150] = f2[:, :150] + 1e-2 * torch.randn(B, 150, 128, generator=g)
    elif case == "tiny_M":
        M = 7
        f2 = f2[:, :M].contiguous()
    elif case == "ragged":
        N, M = 131, 1030
        f1, f2 = torch.randn(B, N, 128, generator=g), torch.randn(B, M, 128, generator=g)
    elif case == "clustered":
        f2 = 0.01 * f2 + 3.0                               # all columns nearly the same point, far from the origin
        f1 = 0.01 * f1 + 3.0
    elif case == "many_equal":
        f2[:] = f2[:, :1]                                  # every column identical: the answer is column 0 everywhere
    T, dm = ops.argmin_exact(dev(f1), dev(f2), want_dist=True)
    Tf, dmf = ops.argmin_exact(dev(f1), dev(f2), want_dist=True, screen=False)
    assert torch.equal(T, Tf) and torch.equal(dm, dmf)
    for b in range(B):
        oT, odm = O.argmin_exact(f1[b].numpy(), f2[b].numpy())
        assert np.array_equal(host(T[b]), oT) and np.array_equal(host(dm[b]), odm)
    T12, T21 = ops.argmin_pair(dev(f1), dev(f2))
    assert torch.equal(T12, T) and torch.equal(T21, ops.argmin_exact(dev(f2), dev(f1), screen=False))
    if case == "many_equal":
        assert int(T.max()) == 0


def test_argmin_full_size_screened(ops):
    """N = M = 4995 (test.py's shape): screened == all-columns scan on every row."""
    g = torch.Generator().manual_seed(77)
    f1, f2 = torch.randn(1, 4995, 128, generator=g), torch.randn(1, 4995, 128, generator=g)
    f1[0, :500] = f2[0, 1000:1500] + 0.05 * torch.randn(500, 128, generator=g)     # planted matches
    T = ops.argmin_exact(dev(f1), dev(f2))
    assert torch.equal(T, ops.argmin_exact(dev(f1), dev(f2), screen=False))
    assert np.array_equal(host(T[0, :500]), np.arange(1000, 1500))


@pytest.mark.parametrize("name", names("knn_"))
def test_knn_cdist(ops, golden, name):
    g = golden(name)
    v = g["verts"][0]
    idx = host(ops.knn_cdist(dev(v)[None], dev(v)[None], 10))[0]
    assert np.array_equal(idx, O.knn_cdist(v, v, 10))
    ref = g["knn_grad_idx"][0]
    assert (idx != ref).any(1).mean() < 0.01  # exact fp32 ties only (see test_oracle_vs_golden)


def test_knn_cdist_general_C(ops):
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 150, 7, generator=g).numpy()
    y = torch.randn(2, 90, 7, generator=g).numpy()
    idx = host(ops.knn_cdist(dev(x), dev(y), 5))
    for b in range(2):
        assert np.array_equal(idx[b], O.knn_cdist(x[b], y[b], 5))


@pytest.mark.parametrize("name", names("dg_"))
def test_graph_build_and_warp(ops, golden, name):
    g = golden(name)
    v = g["verts"]
    N = v.shape[0]
    start = np.array([int(g["fps_start"])], np.int32)
    nodes = host(ops.fps(dev(v)[None], N // 2, dev(start)))[0]
    assert np.array_equal(nodes, g["nodes_idx"])
    b = ops.dg_build(dev(v)[None], dev(start))
    ob = O.dg_build(v, int(start[0]))
    for key in ("nodes_idx", "one_ring", "infl_idx"):
        assert np.array_equal(host(b[key])[0], ob[key]), key
        assert np.array_equal(host(b[key])[0], g[key]), key  # and the reference itself
    assert np.array_equal(host(b["dists"])[0], ob["dists"])
    np.testing.assert_allclose(host(b["sigma"])[0], ob["sigma"], rtol=1e-13)
    np.testing.assert_allclose(host(b["weights"])[0], ob["weights"], rtol=0, atol=2e-7)
    np.testing.assert_allclose(host(b["weights"])[0], g["weights"], rtol=0, atol=3e-7)
    def9 = np.concatenate([g["T"][0], g["d6"][0]], -1)
    iden = np.array([1, 0, 0, 0, 1, 0], np.float32)
    R = ops.rot6d(dev(g["d6"] + iden))
    np.testing.assert_allclose(host(R)[0], g["R"][0], rtol=0, atol=1e-6)
    warped, arap, sr = ops.dg_warp_arap(dev(v)[None], b, R, dev(g["T"]))
    np.testing.assert_allclose(host(warped)[0], g["warped"][0], rtol=0, atol=1e-5)
    np.testing.assert_allclose(float(arap[0]), float(g["arap"]), rtol=1e-5)
    np.testing.assert_allclose(float(sr[0]), float(g["sr"]), rtol=1e-5)


def test_fps_batched_and_large(ops):
    g = torch.Generator().manual_seed(9)
    for N in (300, 2048, 4995):
        v = torch.rand(3, N, 3, generator=g).numpy()
        start = np.array([0, N // 2, N - 1], np.int32)
        out = host(ops.fps(dev(v), N // 2, dev(start)))
        for b in range(3):
            assert np.array_equal(out[b], O.fps(v[b], N // 2, int(start[b])))


@pytest.mark.parametrize("variant", [0, 1, 2, 3])
@pytest.mark.parametrize("name", ["deformer_256x256", "deformer_300x200"])
def test_deformer_and_chamfer(ops, golden, name, variant):
    g = golden(name)
    w = golden("deformer_scape_r_weights")
    wl = ops.deformer_weight_list(w, "cuda")
    f1, f2, v1, v2 = dev(g["feat1"]), dev(g["feat2"]), dev(g["verts1"]), dev(g["verts2"])
    val, idx, _, _ = ops.softcorr(f1, f2, float(g["alpha"]))
    v12 = ops.apply(val, idx, v2)
    np.testing.assert_allclose(host(v12), g["verts12"], rtol=0, atol=1e-5)
    idx11, idx22 = ops.knn_cdist(v1, v1, 10), ops.knn_cdist(v2, v2, 10)
    out = host(ops.deformer(wl, f1, f2, v1, v12, idx11, idx22, val, idx, dev(g["fps1"]), variant=variant))
    np.testing.assert_allclose(out, g["deformations"], rtol=0, atol=1e-4)
    for b in range(out.shape[0]):
        o = O.deformer(w, g["feat1"][b], g["feat2"][b], g["verts1"][b], host(v12)[b], host(idx11)[b], host(idx22)[b],
                       host(val)[b], host(idx)[b], g["fps1"][b])
        np.testing.assert_allclose(out[b], o, rtol=0, atol=5e-6)
    d1, d2, i1, i2 = ops.chamfer(dev(g["verts12"]), v2)
    for b in range(out.shape[0]):
        od1, od2, oi1, oi2 = O.chamfer(g["verts12"][b], g["verts2"][b])
        assert np.array_equal(host(d1)[b], od1) and np.array_equal(host(d2)[b], od2)
        assert np.array_equal(host(i1)[b], oi1) and np.array_equal(host(i2)[b], oi2)


def _pair_inputs(B, N, M, seed):
    g = torch.Generator().manual_seed(seed)
    f1 = 0.3 * torch.relu(torch.randn(B, N, 128, generator=g))
    f2 = 0.3 * torch.relu(torch.randn(B, M, 128, generator=g))
    v1 = torch.rand(B, N, 3, generator=g)
    v2 = torch.rand(B, M, 3, generator=g)
    start = torch.randint(0, N, (B,), generator=g).int()
    return f1, f2, v1, v2, start


@pytest.mark.parametrize("shape", [(2, 256, 256), (2, 300, 170), (1, 1024, 1024), (1, 2200, 4995), (1, 4995, 2200)])
def test_pair_direction_vs_oracle(ops, golden, shape):
    B, N, M = shape
    w = golden("deformer_scape_r_weights")
    wl = ops.deformer_weight_list(w, "cuda")
    f1, f2, v1, v2, start = _pair_inputs(B, N, M, 77 + N)
    out = ops.pair_direction(wl, f1.cuda(), f2.cuda(), v1.cuda(), v2.cuda(), 40.0, start.cuda())
    torch.cuda.synchronize()
    for b in range(B):
        o = O.pair_direction(w, f1[b].numpy(), f2[b].numpy(), v1[b].numpy(), v2[b].numpy(), 40.0, int(start[b]))
        assert np.array_equal(host(out["T12"])[b], o["T12"])
        np.testing.assert_allclose(host(out["verts12"])[b], o["verts12"], rtol=0, atol=5e-6)
        np.testing.assert_allclose(host(out["warped"])[b], o["warped"], rtol=0, atol=1e-4)
        L = host(out["losses"])[b]
        np.testing.assert_allclose(L, o["losses"], rtol=1e-3, atol=1e-7)
        np.testing.assert_allclose(L[[3, 4, 5]], o["losses"][[3, 4, 5]], rtol=1e-4)


def test_pair_direction_full_size_properties(ops, golden):
    """BASELINE config 2 size (N = M = 2048): properties that do not need the oracle at full size,
    plus the oracle on one pair."""
    B, N, M = 4, 2048, 2048
    w = golden("deformer_scape_r_weights")
    wl = ops.deformer_weight_list(w, "cuda")
    f1, f2, v1, v2, start = _pair_inputs(B, N, M, 1234)
    d = [t.cuda() for t in (f1, f2, v1, v2)]
    out = ops.pair_direction(wl, *d, 100.0, start.cuda())
    # (1) determinism: same launch twice -> identical bits
    out2 = ops.pair_direction(wl, *d, 100.0, start.cuda(), out=None)
    for k in out:
        assert torch.equal(out[k], out2[k]), k
    # (2) batch independence: pair b alone gives the same bits as inside the batch
    solo = ops.pair_direction(wl, *[t[2:3] for t in d], 100.0, start[2:3].cuda())
    for k in out:
        assert torch.equal(out[k][2:3], solo[k]), k
    # (3) verts12 is a convex-ish combination of target points: inside their bounding box (Pi rows sum <= 1)
    assert float(out["verts12"].max()) <= float(d[3].max()) + 1e-6 and float(out["verts12"].min()) >= -1e-6
    # (4) the arg-max map agrees with brute-force torch on the device up to fp32 ties
    T = torch.cdist(d[0], d[1]).argmin(-1)
    assert (T.int() != out["T12"]).float().mean() < 1e-3
    # (5) one pair against the oracle
    o = O.pair_direction(w, f1[0].numpy(), f2[0].numpy(), v1[0].numpy(), v2[0].numpy(), 100.0, int(start[0]))
    assert np.array_equal(host(out["T12"])[0], o["T12"])
    np.testing.assert_allclose(host(out["warped"])[0], o["warped"], rtol=0, atol=1e-4)
    np.testing.assert_allclose(host(out["losses"])[0], o["losses"], rtol=1e-3)


@pytest.mark.parametrize("shape", [(3, 512, 512), (2, 300, 170), (2, 330, 330)])
def test_pair_forward_equals_two_directions(ops, golden, shape):
    """The fused two-direction entry shares work between the directions; every output must be
    bit-identical to running the one-direction entry twice."""
    B, N, M = shape
    w = golden("deformer_scape_r_weights")
    wl = ops.deformer_weight_list(w, "cuda")
    f1, f2, v1, v2, s1 = _pair_inputs(B, N, M, 5 + N)
    s2 = torch.arange(B, dtype=torch.int32) % M
    d = [t.cuda() for t in (f1, f2, v1, v2)]
    o12, o21 = ops.pair_forward(wl, *d, 33.0, s1.cuda(), s2.cuda())
    r12 = ops.pair_direction(wl, d[0], d[1], d[2], d[3], 33.0, s1.cuda())
    r21 = ops.pair_direction(wl, d[1], d[0], d[3], d[2], 33.0, s2.cuda())
    for k in r12:
        assert torch.equal(o12[k], r12[k]), ("12", k)
        assert torch.equal(o21[k], r21[k]), ("21", k)


@pytest.mark.parametrize("shape", [(3, 512, 512), (2, 300, 170), (2, 330, 330), (2, 2048, 2048), (1, 4995, 2200)])
@pytest.mark.parametrize("with_map", [True, False])
def test_pair_pipeline_equals_pair_forward(ops, golden, shape, with_map):
    """The two-call form (dvm_pair_geometry_f32 on its own stream for batch t + 1 while dvm_pair_fwd_cached_f32 consumes batch t's)
    over a stream of FIVE different batches through TWO rotating workspaces: every output of every batch bit-identical to the
    one-call dvm_pair_fwd_f32 — a prefetch is never a cache hit (each batch has its own coordinates and FPS starts), and a
    workspace is rewritten while the other is being consumed."""
    B, N, M = shape
    w = golden("deformer_scape_r_weights")
    wl = ops.deformer_weight_list(w, "cuda")
    batches = []
    for t in range(5):
        f1, f2, v1, v2, s1 = _pair_inputs(B, N, M, 900 + 7 * t + N)
        s2 = (torch.arange(B, dtype=torch.int32) * (t + 3)) % M
        batches.append([x.cuda() for x in (f1, f2, v1, v2, s1, s2)])
    ref = []
    for f1, f2, v1, v2, s1, s2 in batches:
        o12, o21 = ops.pair_forward(wl, f1, f2, v1, v2, 50.0, s1, s2, with_map=with_map)
        ref.append(({k: v.clone() for k, v in o12.items()}, {k: v.clone() for k, v in o21.items()}))
        if not with_map:   # no map term: losses[:,5] is an exact 0, read from nothing
            for o in (o12, o21):
                assert torch.equal(o["losses"][:, 5].view(torch.int32), torch.zeros(B, dtype=torch.int32, device="cuda")), o["losses"]
    torch.cuda.synchronize()
    loaded = torch.cuda.Event()
    loaded.record()
    for order in ("step", "geometry first", "features first", "no ready event"):
        pipe = ops.PairPipeline(wl, B, N, M, with_map=with_map)
        ready = None if order == "no ready event" else loaded
        if order in ("geometry first", "features first"):
            pipe.schedule = order
        tk = pipe.prefetch(*batches[0][2:], ready=ready)
        got = []
        for t in range(5):
            outs, tk = pipe.step(tk, batches[t][0], batches[t][1], 50.0, next_coords=batches[t + 1][2:] if t + 1 < 5 else None, ready=ready)
            got.append(outs)
        assert tk is None
        torch.cuda.synchronize()
        for t in range(5):
            for side in (0, 1):
                for k in ref[t][side]:
                    assert torch.equal(got[t][side][k], ref[t][side][k]), (order, t, side, k)


def test_pair_geometry_call_without_helper_streams(ops, golden):
    """dvm_pair_geometry_f32 + dvm_pair_fwd_cached_f32(reuse_geometry = 1) straight through the C ABI on a stream that has NO
    dvm_pair_init context (everything on the caller's stream), and with the helper-stream overlap switched off: same bits as the
    one-call form; a workspace that is too small is refused before any launch."""
    import ctypes
    from dvm import _lib
    lib = _lib.load()
    B, N, M = 2, 384, 384
    w = golden("deformer_scape_r_weights")
    wl = ops.deformer_weight_list(w, "cuda")
    f1, f2, v1, v2, s1 = _pair_inputs(B, N, M, 4711)
    f1, f2, v1, v2, s1 = (x.cuda() for x in (f1, f2, v1, v2, s1))
    s2 = torch.tensor([3, 300], dtype=torch.int32).cuda()
    ref12, ref21 = ops.pair_forward(wl, f1, f2, v1, v2, 70.0, s1, s2)
    torch.cuda.synchronize()
    nb = lib.dvm_pair_workspace_bytes(B, N, M)
    P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    assert lib.dvm_pair_geometry_f32(P(v1), P(v2), B, N, M, P(s1), P(s2), 1, None, 0, None) == -3      # DVM_ENOSPACE
    for overlap in (1, 0):
        prev = lib.dvm_pair_set_overlap(overlap)
        try:
            st = torch.cuda.Stream()          # (never passed to dvm_pair_init)
            ws = torch.zeros(nb, dtype=torch.uint8, device="cuda")
            out = [dict(warped=torch.empty(B, n, 3, device="cuda"), verts12=torch.empty(B, n, 3, device="cuda"),
                        T12=torch.empty(B, n, dtype=torch.int32, device="cuda"), losses=torch.empty(B, 6, device="cuda")) for n in (N, M)]
            st.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(st):
                raw = ctypes.c_void_p(st.cuda_stream)
                ops.check(lib.dvm_pair_geometry_f32(P(v1), P(v2), B, N, M, P(s1), P(s2), 1, P(ws), nb, raw), "dvm_pair_geometry_f32")
                ops.check(lib.dvm_pair_fwd_cached_f32(P(f1), P(f2), P(v1), P(v2), B, N, M, ops.neg_alpha_f32(70.0), P(s1), P(s2), *[P(x) for x in wl], 1,
                                                      P(out[0]["warped"]), P(out[0]["verts12"]), P(out[0]["T12"]), P(out[0]["losses"]),
                                                      P(out[1]["warped"]), P(out[1]["verts12"]), P(out[1]["T12"]), P(out[1]["losses"]), P(ws), nb, 1, raw),
                          "dvm_pair_fwd_cached_f32")
            st.synchronize()
        finally:
            lib.dvm_pair_set_overlap(prev)
        for o, r in zip(out, (ref12, ref21)):
            for k in r:
                assert torch.equal(o[k], r[k]), (overlap, k)


def test_pair_pipeline_rejects_other_shapes(ops, golden):
    from dvm._lib import DvmError
    wl = ops.deformer_weight_list(golden("deformer_scape_r_weights"), "cuda")
    pipe = ops.PairPipeline(wl, 2, 256, 256)
    f1, f2, v1, v2, s1 = _pair_inputs(2, 256, 200, 3)
    with pytest.raises(DvmError):
        pipe.prefetch(v1.cuda(), v2.cuda(), s1.cuda(), s1.cuda())
    # a ticket whose workspace a later prefetch has rewritten (two workspaces rotate) is refused, not silently consumed
    f1, f2, v1, v2, s1 = (x.cuda() for x in _pair_inputs(2, 256, 256, 4))
    stale = pipe.prefetch(v1, v2, s1, s1)
    pipe.prefetch(v1, v2, s1, s1)
    live = pipe.prefetch(v1, v2, s1, s1)
    with pytest.raises(DvmError):
        pipe.forward(stale, f1, f2, 50.0)
    pipe.forward(live, f1, f2, 50.0)
    pipe.close()
    with pytest.raises(DvmError):
        pipe.prefetch(v1, v2, s1, s1)


def test_pair_forward_full_size_vs_oracle(ops, golden):
    """The very call bench.py times — ops.pair_forward at N = M = 2048, d = 128, randn features, alpha = 100, helper-stream
    overlap ON — against the oracle for EVERY pair and both directions: arg-max maps bit-exact, coordinates <= 1e-4,
    losses rtol 1e-3 (B = 4: the oracle needs ~1 s per pair and direction on the box's host cores)."""
    w = golden("deformer_scape_r_weights")
    wl = ops.deformer_weight_list(w, "cuda")
    B, N = 4, 2048
    g = torch.Generator().manual_seed(2048)
    f1, f2 = torch.randn(B, N, 128, generator=g), torch.randn(B, N, 128, generator=g)
    v1, v2 = torch.rand(B, N, 3, generator=g), torch.rand(B, N, 3, generator=g)
    s1, s2 = torch.tensor([0, 5, 77, 2047], dtype=torch.int32), torch.zeros(B, dtype=torch.int32)
    from dvm import _lib
    assert _lib.load().dvm_pair_set_overlap(1) in (0, 1)
    o12, o21 = ops.pair_forward(wl, f1.cuda(), f2.cuda(), v1.cuda(), v2.cuda(), 100.0, s1.cuda(), s2.cuda())
    torch.cuda.synchronize()
    for b in range(B):
        for out, (fa, fb, va, vb, st) in ((o12, (f1, f2, v1, v2, s1)), (o21, (f2, f1, v2, v1, s2))):
            o = O.pair_direction(w, fa[b].numpy(), fb[b].numpy(), va[b].numpy(), vb[b].numpy(), 100.0, int(st[b]))
            assert np.array_equal(host(out["T12"])[b], o["T12"]), "arg-max map differs from the oracle"
            np.testing.assert_allclose(host(out["verts12"])[b], o["verts12"], rtol=0, atol=1e-5)
            np.testing.assert_allclose(host(out["warped"])[b], o["warped"], rtol=0, atol=1e-4)
            np.testing.assert_allclose(host(out["losses"])[b], o["losses"], rtol=1e-3)


def test_errors_are_loud(ops):
    from dvm._lib import DvmError
    f = torch.randn(1, 8, 128)
    with pytest.raises(DvmError):
        ops.softcorr(f, f, 10.0)  # CPU tensors: no fallback
    with pytest.raises(DvmError):
        ops.softcorr(f.cuda(), f.cuda(), 10.0, topk=17)
    with pytest.raises(DvmError):
        ops.softcorr(torch.randn(1, 8, 130).cuda(), torch.randn(1, 8, 130).cuda(), 10.0)
    with pytest.raises(DvmError):
        ops.softcorr(f.cuda(), f.cuda(), -10.0)


@pytest.mark.parametrize("case", ["wide_range", "zeros", "tiny_M", "single_row", "huge_scale", "tiny_scale", "clustered"])
def test_softcorr_fp16_split_edge_cases(ops, case):
    """Variant 3 (fp16x2-split sweep + exact re-evaluation): inputs chosen to stress the split's scaling, the
    certification and the exact-recompute fallback; outputs must still equal the oracle's (columns bit-exact)."""
    import zlib
    g = np.random.default_rng(zlib.crc32(case.encode()))
    N, M, d = 150, 210, 128
    f1 = g.standard_normal((N, d)).astype(np.float32)
    f2 = g.standard_normal((M, d)).astype(np.float32)
    alpha = 40.0
    if case == "wide_range":       # one coordinate 1e4 times the others, some 1e-6
        f1[:, 3] *= 1e4; f2[:, 3] *= 1e4; f1[:, 7] *= 1e-6; f2[:, 9] *= 1e-6
        alpha = 0.01
    elif case == "zeros":          # every distance ties: nothing can be certified, all rows take the exact kernel
        f1[:], f2[:] = 0.0, 0.0
    elif case == "tiny_M":
        f2 = f2[:5]
    elif case == "single_row":
        f1, f2 = f1[:1], f2[:13]
    elif case == "huge_scale":
        f1 *= 3e5; f2 *= 3e5; alpha = 1e-5
    elif case == "tiny_scale":
        f1 *= 1e-12; f2 *= 1e-12; alpha = 1e13
    elif case == "clustered":      # many near-duplicates: dense ties around the 10th neighbour
        f2 = np.repeat(f2[:21], 10, axis=0) + (1e-7 * g.standard_normal((210, d))).astype(np.float32)
    check_softcorr(ops, f1, f2, alpha, 3)


def test_deformer_mlp_fp16_range_fallback(ops, golden):
    """Variant 0's fp16x2 MLP raises its flag when an activation leaves fp16's range; the gated bf16x3 launch must
    then deliver the result (compared with the fp32-MFMA variant on inputs scaled far outside the range)."""
    w = golden("deformer_scape_r_weights")
    wl = ops.deformer_weight_list(dict(w), "cuda")
    g = torch.Generator().manual_seed(3)
    z = torch.randn(2, 100, 262, generator=g).cuda()
    z[0, :50] *= 4000.0          # |z * 32| > 60000
    ref = ops.deformer_mlp(wl, z * 1.0)  # variant 0 path (with fallback)
    # reference: fp64 MLP on the host
    W = [w["deformation_decoder_layer__linear__%d__weight" % i].astype(np.float64) for i in (0, 2, 4, 6)]
    bb = [w["deformation_decoder_layer__linear__%d__bias" % i].astype(np.float64) for i in (0, 2, 4, 6)]
    x = host(z).astype(np.float64)
    for i in range(4):
        x = x @ W[i].T + bb[i]
        if i < 3:
            x = np.where(x > 0, x, np.expm1(x))
    # outputs of the blown-up rows are O(1e4) sums of O(1e5) terms: fp32-level agreement is relative to that scale
    np.testing.assert_allclose(host(ref), x, rtol=2e-5, atol=2e-5 * np.abs(x).max())
    # the 150 ordinary rows, which the fallback recomputes as well, at THEIR scale: each within 3 x the error of the fp32 chain
    # (numpy, exp(x) - 1) against float64 on these rows (tests/test_gpu_deformer_mlp_adversarial.py: the per-family bar)
    plain = np.ones((2, 100), bool)
    plain[0, :50] = False
    y = host(z)[plain]
    for i in range(4):
        y = (y @ W[i].astype(np.float32).T + bb[i].astype(np.float32)).astype(np.float32)
        if i < 3:
            y = np.where(y > 0, y, np.exp(np.minimum(y, np.float32(0))) - np.float32(1)).astype(np.float32)
    noise = np.abs(y - x[plain]).max()
    assert noise > 0
    assert np.abs(host(ref)[plain] - x[plain]).max() <= 3 * noise, (np.abs(host(ref)[plain] - x[plain]).max(), noise)


@pytest.mark.parametrize("rows", [1, 63, 64, 65, 200, 2 * 256 * 64 + 77])
def test_deformer_mlp_persistent_form_row_counts(ops, golden, rows):
    """Variant 0's persistent kernel walks 64-row blocks, the next block's fp16 planes arriving by LDS-DMA while the current one
    is computed: row counts below / at / above a block, and more blocks than the chip has compute units (every workgroup walks
    three), against the fp64 MLP on the host.  (reference models/model.py:433-452)"""
    w = golden("deformer_scape_r_weights")
    wl = ops.deformer_weight_list(dict(w), "cuda")
    g = torch.Generator().manual_seed(rows)
    z = torch.randn(1, rows, 262, generator=g)
    z[..., :3] = torch.rand(1, rows, 3, generator=g)
    got = host(ops.deformer_mlp(wl, z.cuda()))
    W = [w["deformation_decoder_layer__linear__%d__weight" % i].astype(np.float64) for i in (0, 2, 4, 6)]
    bb = [w["deformation_decoder_layer__linear__%d__bias" % i].astype(np.float64) for i in (0, 2, 4, 6)]
    x = z.numpy().astype(np.float64)
    for i in range(4):
        x = x @ W[i].T + bb[i]
        if i < 3:
            x = np.where(x > 0, x, np.expm1(x))
    assert got.shape == x.shape and np.isfinite(got).all()
    np.testing.assert_allclose(got, x, rtol=2e-5, atol=2e-5 * np.abs(x).max())
    again = host(ops.deformer_mlp(wl, z.cuda()))
    assert np.array_equal(got, again)                      # fixed summation order: bit-reproducible


def test_pair_forward_range_fallback_equals_two_directions(ops, golden):
    """Coordinates far outside fp16's range (|32 v| > 65504): the persistent MLP kernel's outputs are NaN for those nodes, its flag
    comes up, and the GATED launches behind it — the fp32 rows, then the bf16x3 kernel — deliver the result.  The fused entry
    assembles its rows in the plane form and re-assembles them as floats under the gate; the one-direction entry keeps the float
    rows: both must agree bit for bit, and be finite."""
    B, N, M = 2, 330, 330
    w = golden("deformer_scape_r_weights")
    wl = ops.deformer_weight_list(w, "cuda")
    f1, f2, v1, v2, s1 = _pair_inputs(B, N, M, 77)
    v1, v2 = v1 * 3000.0, v2 * 3000.0
    s2 = torch.arange(B, dtype=torch.int32) % M
    d = [t.cuda() for t in (f1, f2, v1, v2)]
    o12, o21 = ops.pair_forward(wl, *d, 33.0, s1.cuda(), s2.cuda())
    r12 = ops.pair_direction(wl, d[0], d[1], d[2], d[3], 33.0, s1.cuda())
    r21 = ops.pair_direction(wl, d[1], d[0], d[3], d[2], 33.0, s2.cuda())
    for k in r12:
        assert torch.equal(o12[k], r12[k]), ("12", k)
        assert torch.equal(o21[k], r21[k]), ("21", k)
    assert torch.isfinite(o12["warped"]).all() and torch.isfinite(o21["warped"]).all()


@pytest.mark.parametrize("rows,K", [(1, 128), (7, 128), (4096 + 3, 128), (2 * 2048, 128), (513, 64), (300, 262), (64, 3)])
def test_rownorm2_bit_exact(ops, rows, K):
    """|x|^2 per row in ATen's summation order (the norms cdist's matmul form adds to the products): the K = 128 kernel's
    DPP / permlane reduction tree and the generic kernel against the oracle's restatement, bit for bit, at row counts that
    leave the last wave partly filled."""
    g = torch.Generator().manual_seed(rows * 131 + K)
    x = torch.randn(rows, K, generator=g) * torch.rand(rows, 1, generator=g) * 3
    got = ops.rownorm2(x.cuda()).cpu().numpy()
    assert np.array_equal(got, O.rownorm2(x.numpy())), (rows, K)


@pytest.mark.parametrize("kind", ["collapsed_target", "far_queries", "duplicates", "holes"])
def test_chamfer_grid_scan_path_equals_brute_force(ops, kind):
    """The uniform-grid Chamfer at a batch large enough to take it (B * (N + M) > 65536), on the configurations where most
    lanes of a wave fail the radius-1 certification and the kernel scans the whole target instead of walking the grid — a
    target collapsed to a tiny cluster (what a flat soft-max row makes of the correspondence image), queries far outside
    the target's box, duplicated target points (ties -> lowest index) — against a brute-force arg-min in torch."""
    g = torch.Generator().manual_seed(5)
    B, N, M = 20, 2048, 2048
    a = torch.rand(B, N, 3, generator=g)
    b = torch.rand(B, M, 3, generator=g)
    if kind == "collapsed_target":
        b = 0.5 + 1e-3 * torch.rand(B, M, 3, generator=g)
    elif kind == "far_queries":
        a = a + torch.tensor([3.0, -2.0, 5.0])
    elif kind == "holes":
        # the WALK path (round 6: the radius-3 cube searched by the whole wave): a few queries per wave whose radius-1 cube holds no
        # certifiable neighbour — the target has empty balls of ~1.5 cells radius — with the displaced points stacked onto others
        # (exact ties on the rim: lowest index wins)
        centres = torch.rand(B, 12, 3, generator=g)
        inside = (torch.cdist(b, centres) < 0.12).any(-1)                     # (B, M)
        donors = torch.randint(0, M, (B, M), generator=g)
        b = torch.where(inside.unsqueeze(-1), torch.gather(b, 1, donors.unsqueeze(-1).expand(-1, -1, 3)), b)
        inside2 = (torch.cdist(b, centres) < 0.12).any(-1)                    # (a donor may itself lie in a ball: push those out)
        b = torch.where(inside2.unsqueeze(-1), b[:, :1].expand(-1, M, -1), b)
    else:
        b[:, M // 2:] = b[:, :M // 2]
    d1, d2, i1, i2 = ops.chamfer(a.cuda(), b.cuda(), want_idx=True)
    for q, t, d, ix in ((a, b, d1, i1), (b, a, d2, i2)):
        diff = q[:, :, None, :].cuda() - t[:, None, :, :].cuda()
        D = (diff[..., 0] * diff[..., 0] + diff[..., 1] * diff[..., 1]) + diff[..., 2] * diff[..., 2]   # the kernel's formula
        ref_d, ref_i = D.min(dim=2)
        assert torch.equal(d, ref_d), kind
        # torch.min returns one of the minima; the kernel's index must be a minimiser, and the lowest one
        got = torch.gather(D, 2, ix.long().unsqueeze(-1)).squeeze(-1)
        assert torch.equal(got, ref_d), kind
        lowest = (D == ref_d.unsqueeze(-1)).float().argmax(dim=2)
        assert torch.equal(ix.long(), lowest), kind


# ---------------------------------------------------------------------------------------------------------------------
# Contract sizes across the alpha schedule (VERDICT r3 'weak 1'): the schedule starts at alpha = 10
# (config/scape_r.yaml:40, train.py:75), where the FIRST sweep form runs in full and every column owes a softmax term.
def _feature_set(kind, rows, seed):
    rng = np.random.default_rng(seed)
    f = rng.standard_normal((rows, 128)).astype(np.float32)
    return (0.3 * np.maximum(f, 0)).astype(np.float32) if kind == "trained" else f


@pytest.mark.parametrize("kind", ["randn", "trained"])
@pytest.mark.parametrize("alpha", [10.0, 33.0])
def test_softcorr_contract_size_low_alpha_vs_oracle(ops, alpha, kind):
    """2048 x 2048, d = 128 at alpha 10 / 33 on both synthetic feature sets of SURVEY 8d: top-10 columns bit-exact, row
    maxima bit-exact, softmax sums 2e-5, values 5e-5 relative — the flat-row regime (at alpha 10 the trained-like rows
    spread their mass over hundreds of columns: every term of the sum comes from the fp16-split sweep)."""
    f1, f2 = _feature_set(kind, 2048, 1000 + int(alpha)), _feature_set(kind, 2048, 2000 + int(alpha))
    val, idx = check_softcorr(ops, f1, f2, alpha, 3)
    assert (idx >= 0).all() and (idx < 2048).all()
    if kind == "trained" and alpha == 10.0:
        assert float(val[:, 0].max()) < 0.5            # flat rows indeed: no row is near one-hot


@pytest.mark.parametrize("kind", ["randn", "trained"])
@pytest.mark.parametrize("alpha", [10.0, 33.0])
def test_pair_forward_contract_size_low_alpha_vs_oracle(ops, golden, alpha, kind):
    """ops.pair_forward (what bench.py times) at N = M = 2048 for the low end of the alpha schedule, both feature sets,
    both directions, against the oracle: arg-max maps bit-exact, coordinates <= 1e-4, losses rtol 1e-3."""
    w = golden("deformer_scape_r_weights")
    wl = ops.deformer_weight_list(w, "cuda")
    B, N = 2, 2048
    f1 = np.stack([_feature_set(kind, N, 31 + b + int(alpha)) for b in range(B)])
    f2 = np.stack([_feature_set(kind, N, 61 + b + int(alpha)) for b in range(B)])
    g = torch.Generator().manual_seed(5 + int(alpha))
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


def test_softcorr_non_finite_features_keep_columns_in_range(ops):
    """the coarse screen (as the second-form sweep it replaced) is built with -fno-honor-nans ("no NaN is ever formed" holds for finite features).
    A diverged training step can hand it NaN / Inf rows; whatever the values then are, every column index written must
    stay inside [0, M): the columns feed unchecked gathers (Pi @ V, the Deformer rows, the map term).  The finite rows of
    the same launch that do not see a non-finite key are still the oracle's."""
    rng = np.random.default_rng(4)
    N = M = 2048
    f1 = rng.standard_normal((2, N, 128)).astype(np.float32)
    f2 = rng.standard_normal((2, M, 128)).astype(np.float32)
    f1[0, 7] = np.nan
    f1[0, 300, 5] = np.inf
    f1[0, 301, 9] = -np.inf
    f2[1, 11] = np.nan                                 # a non-finite KEY: every row of pair 1 sees it
    f2[1, 900, 3] = np.inf
    for alpha in (10.0, 100.0):                        # first form in full / the routed coarse screen
        for variant in (0, 3):
            junk = [torch.full((2, N, 10), 0x7f7f7f7f, dtype=torch.int32, device="cuda")]
            torch.cuda.synchronize()
            del junk
            val, idx, _, _ = ops.softcorr(dev(f1), dev(f2), alpha, variant=variant)
            torch.cuda.synchronize()
            assert int(idx.min()) >= 0 and int(idx.max()) < M, (alpha, variant, int(idx.min()), int(idx.max()))
            v12 = ops.apply(val, idx, dev(rng.random((2, M, 3)).astype(np.float32)))   # the gather itself must not fault
            torch.cuda.synchronize()
            assert v12.shape == (2, N, 3)
        clean = [r for r in range(0, N, 97) if r not in (7, 300, 301)]
        _, oidx, _, _ = O.softcorr(f1[0][clean], f2[0], alpha)
        assert np.array_equal(host(idx)[0][clean], oidx)


def test_partial_criterion_contract_size_vs_oracle(ops, golden):
    """GraphDeformLoss_Neural_Partial's 5-tuple at config 4's real shape, 4995 x 2200 (models/dataset_partial.py:253), B = 1,
    config/scape_partial.yaml's weights and anchor counts — against the same terms assembled from the oracle
    (oracle.pair_direction for both directions, torch_ref.dist_loss_term in float64), rtol 2e-4 (models/loss.py:986-1073)."""
    import random
    import models.loss as ml
    import models.model as mm
    from oracle import torch_ref as TR
    w = golden("deformer_scape_r_weights")
    d = mm.Deformer(10)
    d.load_state_dict({k.replace("__", "."): torch.from_numpy(v) for k, v in w.items()})
    d = d.cuda().eval()
    N, M, alpha = 4995, 2200, 40.0
    g = torch.Generator().manual_seed(4995)
    f1 = 0.3 * torch.relu(torch.randn(1, N, 128, generator=g))
    f2 = 0.3 * torch.relu(torch.randn(1, M, 128, generator=g))
    v1, v2 = torch.rand(1, N, 3, generator=g), torch.rand(1, M, 3, generator=g)
    dist1, dist2 = torch.cdist(v1, v1), torch.cdist(v2, v2)
    kw = dict(k_deform=10, w_dist=0.02, w_map=0.005, k_dist=300, N_dist=500, partial=True, w_deform=1000, w_img=0, w_rank=0,
              w_self_rec=1000, w_cd=0.1, w_arap=0.01)
    crit = ml.GraphDeformLoss_Neural_Partial(save_name="t", **kw)
    rnd = random.Random(9)
    anchors = (rnd.sample(range(N), 500), rnd.sample(range(M), 500))
    starts = (torch.tensor([17]), torch.tensor([2100]))
    with torch.no_grad():
        out = crit(f1.cuda(), f2.cuda(), dist1.cuda(), dist2.cuda(), v1.cuda(), v2.cuda(), alpha, d, fps_starts=starts, anchors=anchors)
    got = [float(o) for o in out]
    # the oracle's terms
    o12 = O.pair_direction(w, f1[0].numpy(), f2[0].numpy(), v1[0].numpy(), v2[0].numpy(), alpha, 17, with_map=False)
    o21 = O.pair_direction(w, f2[0].numpy(), f1[0].numpy(), v2[0].numpy(), v1[0].numpy(), alpha, 2100, with_map=False)
    # one-sided Chamfer: the side of the smaller cloud (models/loss.py:875-880) = losses[1] / [4] when the deformed cloud is
    # the larger one (12: 4995 -> 2200), losses[0] / [3] when it is the smaller (21)
    cw12, cs12 = float(o12["losses"][1]), float(o12["losses"][4])
    cw21, cs21 = float(o21["losses"][0]), float(o21["losses"][3])
    deform = ((cw12 * 0.1 + float(o12["losses"][2]) * 0.01) + (cw21 * 0.1 + float(o21["losses"][2]) * 0.01)) * 1000 / 2
    self_rec = (cs12 + cs21) * 1000 / 2
    dl = 0.02 * (float(TR.dist_loss_term(f1.double(), dist1.double(), torch.tensor(anchors[0]), 300).sum()) +
                 float(TR.dist_loss_term(f2.double(), dist2.double(), torch.tensor(anchors[1]), 300).sum()))
    want = [dl + deform + self_rec, dl, deform, 0.0, self_rec]
    np.testing.assert_allclose(got, want, rtol=2e-4, atol=1e-12)


def test_pair_forward_graph_cache_is_bit_identical(ops, golden):
    """SURVEY 8f-2 / 8d, the opt-in per-shape graph cache: a hit (dvm_pair_fwd_cached_f32 with reuse_geometry = 1 on the
    workspace of an earlier call with the same coordinates and FPS starts) gives the bits of the uncached call for NEW
    features; another key, other starts or other sizes miss and rebuild; N == M and N != M layouts."""
    w = golden("deformer_scape_r_weights")
    wl = ops.deformer_weight_list(w, "cuda")
    for B, N, M in ((3, 512, 512), (2, 330, 170)):
        f1, f2, v1, v2, start = _pair_inputs(B, N, M, 9 + N)
        g = torch.Generator().manual_seed(N)
        f1b, f2b = torch.randn(B, N, 128, generator=g), torch.randn(B, M, 128, generator=g)
        d = [t.cuda() for t in (v1, v2)]
        s1, s2 = start.cuda(), (start % M).int().cuda()
        cache = ops.GeometryCache()
        first = ops.pair_forward(wl, f1.cuda(), f2.cuda(), *d, 60.0, s1, s2, cache=cache, key=("a", N))
        plain1 = ops.pair_forward(wl, f1.cuda(), f2.cuda(), *d, 60.0, s1, s2)
        hit = ops.pair_forward(wl, f1b.cuda(), f2b.cuda(), *d, 60.0, s1, s2, cache=cache, key=("a", N))      # new features, cached geometry
        plain2 = ops.pair_forward(wl, f1b.cuda(), f2b.cuda(), *d, 60.0, s1, s2)
        assert (cache.hits, cache.misses) == (1, 1)
        for got, want in ((first, plain1), (hit, plain2)):
            for a, b in zip(got, want):
                for k in a:
                    assert torch.equal(a[k], b[k]), (B, N, M, k)
        # other starts under another key: a miss, and the result is that of the uncached call with those starts
        s1b = ((start + 5) % N).int().cuda()
        other = ops.pair_forward(wl, f1.cuda(), f2.cuda(), *d, 60.0, s1b, s2, cache=cache, key=("b", N))
        plain3 = ops.pair_forward(wl, f1.cuda(), f2.cuda(), *d, 60.0, s1b, s2)
        assert cache.misses == 2
        for a, b in zip(other, plain3):
            for k in a:
                assert torch.equal(a[k], b[k]), k
        assert not torch.equal(other[0]["warped"], first[0]["warped"])
