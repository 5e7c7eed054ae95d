"""-m gpu: results must not depend on what the scratch held.  Every workspace the library receives comes from ops.workspace() or
ops.scratch() (torch.empty: whatever the caching allocator hands back).  Here both are replaced by a poisoning allocator: each call
gets a fresh buffer of EXACTLY the queried size, filled with one byte and framed by two 1 MiB guard bands of the same byte.

  clean   fill 0x00, run twice: the entry is run-to-run reproducible (bitwise)
  poison  fill 0xFF (NaN as fp16 / fp32 / fp64, -1 as int32: a stray index lands in the guard band, not before the buffer),
          outputs pre-filled with NaN / 0x7f7f7f7f: the result equals the clean one bit for bit
  guards  both bands still hold their fill byte after the run: nothing wrote past what *_workspace_bytes() reported

and each case also checks its clean result against the C oracle (or the path the existing parity test compares it with).  The last
tests run the existing GPU parity / backward / backbone / training suites in a child process with the same poisoning allocator
installed, so every oracle and fp64 assertion they make holds against poisoned scratch too."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import oracle as O
from oracle import torch_ref as TR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
MiB = 1 << 20


class PoisonedScratch:
    """Replacement for ops.workspace / ops.scratch: a fresh buffer per call, `nbytes` exactly, at offset 1 MiB of an allocation of
    nbytes + 2 MiB filled with `fill` (torch's blocks are 512-byte aligned, so the view keeps the arena's 256-byte alignment).  The
    buffers live until release(), so anything read back after the call (dvm_k1_last_routes) still sees its own memory."""

    def __init__(self, fill):
        self.fill, self.bufs = fill, []

    def scratch(self, nbytes, device):
        n = int(nbytes)
        full = torch.full((n + 2 * MiB,), self.fill, dtype=torch.uint8, device=device)
        self.bufs.append((full, n))
        return full[MiB:MiB + n]

    def workspace(self, nbytes, device, tag="ws"):
        return self.scratch(nbytes, device)

    def install(self, ops, monkeypatch=None):
        if monkeypatch is None:
            ops.workspace, ops.scratch = self.workspace, self.scratch
        else:
            monkeypatch.setattr(ops, "workspace", self.workspace)
            monkeypatch.setattr(ops, "scratch", self.scratch)

    def check_guards(self):
        torch.cuda.synchronize()
        bad = [(i, n) for i, (full, n) in enumerate(self.bufs)
               if not (bool((full[:MiB] == self.fill).all()) and bool((full[MiB + n:] == self.fill).all()))]
        assert not bad, "writes past the queried workspace size (buffer #, bytes): %s" % bad

    def release(self):
        torch.cuda.synchronize()
        self.bufs = []


@pytest.fixture(scope="module")
def ops():
    from dvm import ops as _ops
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _ops


@pytest.fixture(scope="module")
def lib(ops):
    from dvm import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def weights():
    w = dict(np.load(os.path.join(GOLDEN, "deformer_scape_r_weights.npz")))
    return w


def rel(a, ref):
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    return float((a - ref).norm() / (ref.norm() + 1e-300))


def _flat(x, name="out"):
    if isinstance(x, torch.Tensor):
        return [(name, x)]
    if isinstance(x, dict):
        return [p for k in sorted(x) for p in _flat(x[k], "%s.%s" % (name, k))]
    if isinstance(x, (list, tuple)):
        return [p for i, v in enumerate(x) for p in _flat(v, "%s[%d]" % (name, i))]
    if x is None:
        return []
    if isinstance(x, (float, int)):
        return [(name, torch.tensor(x, dtype=torch.float64))]
    raise TypeError(type(x))


_BITS = {torch.float32: torch.int32, torch.float64: torch.int64, torch.float16: torch.int16, torch.bfloat16: torch.int16}


def _bits(t):
    t = t.detach().contiguous().cpu()
    return t.view(_BITS[t.dtype]) if t.dtype in _BITS else t


def _junk(like):
    """Blocks of the outputs' sizes, NaN / 0x7f7f7f7f, released before the poisoned run: the caching allocator hands them back as
    the outputs (tests/test_gpu_parity.py::test_softcorr_writes_every_output_slot)."""
    js = [torch.full(t.shape, float("nan"), dtype=t.dtype, device="cuda") if t.is_floating_point()
          else torch.full(t.shape, 0x7f7f7f7f if t.dtype == torch.int32 else -1, dtype=t.dtype, device="cuda") for _, t in like]
    torch.cuda.synchronize()
    del js


def _out_like(shapes, poison):
    """`out=` tensors: zeros in the clean runs, NaN / 0x7f7f7f7f in the poisoned one."""
    res = []
    for shape, dt in shapes:
        if dt == torch.int32:
            res.append(torch.full(shape, 0x7f7f7f7f if poison else 0, dtype=dt, device="cuda"))
        else:
            res.append(torch.full(shape, float("nan") if poison else 0.0, dtype=dt, device="cuda"))
    return res


def hygiene(ops, monkeypatch, fn, tol=None):
    """fn(poison: bool) -> outputs (tensors, nested in dicts / tuples).  Runs clean twice and poisoned once; asserts bitwise equality
    and intact guard bands; -> the clean outputs (on the host, flattened to [(name, tensor)]).  tol {name: relative tolerance}: the
    outputs that are not run-to-run reproducible by design (fp32 atomics: no fixed summation order) are compared at that
    tolerance instead, and must be finite."""
    tol = tol or {}
    runs = []
    for poison in (False, False, True):
        P = PoisonedScratch(0xFF if poison else 0x00)
        P.install(ops, monkeypatch)
        if poison:
            _junk(runs[0])
        try:
            outs = [(k, v.detach().cpu().clone()) for k, v in _flat(fn(poison))]
            torch.cuda.synchronize()
            P.check_guards()
        finally:
            P.release()
        runs.append(outs)
    clean, again, pois = runs
    assert [k for k, _ in clean] == [k for k, _ in pois]
    for (k, a), (_, b) in zip(clean, again):
        if k in tol:
            assert rel(b, a) <= tol[k], "clean runs differ beyond %g: %s (%g)" % (tol[k], k, rel(b, a))
        else:
            assert torch.equal(_bits(a), _bits(b)), "clean runs differ: %s" % k
    for (k, a), (_, b) in zip(clean, pois):
        if k in tol:
            assert bool(torch.isfinite(b).all()) and rel(b, a) <= tol[k], "poisoned scratch changes %s (%g)" % (k, rel(b, a))
        else:
            assert torch.equal(_bits(a), _bits(b)), "poisoned scratch changes %s (NaN: %d of %d)" % (
                k, int(torch.isnan(b).sum()) if b.is_floating_point() else -1, b.numel())
    return dict(clean)


@pytest.fixture
def overlap(lib):
    """dvm_pair_set_overlap(value) for the test, restored after it."""
    prev = []

    def set_(on):
        prev.append(lib.dvm_pair_set_overlap(int(on)))
    yield set_
    if prev:
        lib.dvm_pair_set_overlap(prev[0])


@pytest.fixture
def deterministic(ops):
    prev = ops.set_deterministic(True)
    yield
    ops.set_deterministic(prev)


def _pair_inputs(B, N, M, seed):
    g = torch.Generator().manual_seed(seed)
    f1 = 0.3 * torch.relu(torch.randn(B, N, 128, generator=g))
    f2 = 0.3 * torch.relu(torch.randn(B, M, 128, generator=g))
    v1, v2 = torch.rand(B, N, 3, generator=g), torch.rand(B, M, 3, generator=g)
    s1 = torch.randint(0, N, (B,), generator=g).int()
    s2 = torch.randint(0, M, (B,), generator=g).int()
    return f1, f2, v1, v2, s1, s2


def _check_direction_vs_oracle(w, out, f1, f2, v1, v2, alpha, start, with_map, pre):
    """The tolerances of tests/test_gpu_parity.py::test_pair_direction_vs_oracle."""
    for b in range(f1.shape[0]):
        o = O.pair_direction(w, f1[b].numpy(), f2[b].numpy(), v1[b].numpy(), v2[b].numpy(), alpha, int(start[b]), with_map=with_map)
        assert np.array_equal(out[pre + ".T12"][b].numpy(), o["T12"])
        np.testing.assert_allclose(out[pre + ".verts12"][b].numpy(), o["verts12"], rtol=0, atol=5e-6)
        np.testing.assert_allclose(out[pre + ".warped"][b].numpy(), o["warped"], rtol=0, atol=1e-4)
        L = out[pre + ".losses"][b].numpy()
        np.testing.assert_allclose(L, o["losses"], rtol=1e-3, atol=1e-7)
        np.testing.assert_allclose(L[[3, 4, 5]], o["losses"][[3, 4, 5]], rtol=1e-4)
        if not with_map:
            assert (L[5] == 0.0) and not np.signbit(L[5]), L


def _pair_out_shapes(B, N, M):
    def one(n):
        return [((B, n, 3), torch.float32), ((B, n, 3), torch.float32), ((B, n), torch.int32), ((B, 6), torch.float32)]
    return one(N) + one(M)


def _pair_out_dicts(ts):
    keys = ("warped", "verts12", "T12", "losses")
    return dict(zip(keys, ts[:4])), dict(zip(keys, ts[4:]))


# ------------------------------------------------------------------------------------------------------------------ pair path
@pytest.mark.parametrize("ovl", [1, 0], ids=["overlap", "one_stream"])
@pytest.mark.parametrize("with_map", [True, False], ids=["map", "nomap"])
@pytest.mark.parametrize("shape", [(2, 300, 170), (3, 512, 512), (1, 4995, 2200)], ids=["ragged", "square512", "contract"])
def test_pair_forward_poisoned_scratch(ops, monkeypatch, overlap, weights, shape, with_map, ovl):
    """dvm_pair_fwd_f32 with `out=`.  With with_map=False and one stream, losses[:,5] used to be mean(w.cd[0]) * 0 read BEFORE the
    warped-cloud Chamfer wrote w.cd[0] (and, with overlap, on another stream at the same time): NaN from poisoned scratch."""
    B, N, M = shape
    overlap(ovl)
    wl = ops.deformer_weight_list(weights, "cuda")
    f1, f2, v1, v2, s1, s2 = _pair_inputs(B, N, M, 31 + N + M)
    d = [t.cuda() for t in (f1, f2, v1, v2, s1, s2)]

    def run(poison):
        out = _pair_out_dicts(_out_like(_pair_out_shapes(B, N, M), poison))
        return ops.pair_forward(wl, *d[:4], 40.0, d[4], d[5], with_map=with_map, out=out)
    got = hygiene(ops, monkeypatch, run)
    if not with_map:
        for side in ("out[0]", "out[1]"):
            assert torch.equal(_bits(got[side + ".losses"][:, 5]), torch.zeros(B, dtype=torch.int32)), got[side + ".losses"]
    if ovl == 1:   # (one-stream clean == overlapped clean is the fused path's own contract: the parity suite runs both)
        _check_direction_vs_oracle(weights, got, f1, f2, v1, v2, 40.0, s1, with_map, "out[0]")
        _check_direction_vs_oracle(weights, got, f2, f1, v2, v1, 40.0, s2, with_map, "out[1]")


@pytest.mark.parametrize("with_map", [True, False], ids=["map", "nomap"])
@pytest.mark.parametrize("shape", [(2, 300, 170), (1, 2200, 4995)], ids=["ragged", "contract"])
def test_pair_direction_poisoned_scratch(ops, monkeypatch, weights, shape, with_map):
    B, N, M = shape
    wl = ops.deformer_weight_list(weights, "cuda")
    f1, f2, v1, v2, s1, _ = _pair_inputs(B, N, M, 77 + N)
    d = [t.cuda() for t in (f1, f2, v1, v2, s1)]

    def run(poison):
        out = dict(zip(("warped", "verts12", "T12", "losses"), _out_like(_pair_out_shapes(B, N, M)[:4], poison)))
        return ops.pair_direction(wl, *d[:4], 40.0, d[4], with_map=with_map, out=out)
    got = hygiene(ops, monkeypatch, run)
    _check_direction_vs_oracle(weights, got, f1, f2, v1, v2, 40.0, s1, with_map, "out")


@pytest.mark.parametrize("with_map", [True, False], ids=["map", "nomap"])
def test_pair_pipeline_poisoned_workspaces(ops, monkeypatch, weights, with_map):
    """Three batches through both rotating workspaces (ops.scratch), each bit-identical to the clean one-call pair_forward."""
    B, N, M = 2, 300, 170
    wl = ops.deformer_weight_list(weights, "cuda")
    batches = [[t.cuda() for t in _pair_inputs(B, N, M, 500 + t)] for t in range(3)]
    P = PoisonedScratch(0x00)
    P.install(ops, monkeypatch)
    ref = [ops.pair_forward(wl, *b[:4], 50.0, b[4], b[5], with_map=with_map) for b in batches]
    torch.cuda.synchronize()

    def run(poison):
        pipe = ops.PairPipeline(wl, B, N, M, with_map=with_map)
        loaded = torch.cuda.Event()
        loaded.record()
        tk = pipe.prefetch(*batches[0][2:], ready=loaded)
        got = []
        for t in range(3):
            out = _pair_out_dicts(_out_like(_pair_out_shapes(B, N, M), poison))
            outs, tk = pipe.step(tk, batches[t][0], batches[t][1], 50.0, next_coords=batches[t + 1][2:] if t + 1 < 3 else None,
                                 ready=loaded, out=out)
            got.append(outs)
        pipe.close()
        return got
    got = hygiene(ops, monkeypatch, run)
    for t in range(3):
        for side in (0, 1):
            for k, v in ref[t][side].items():
                assert torch.equal(got["out[%d][%d].%s" % (t, side, k)], v.cpu()), (t, side, k)
    P.release()


def test_pair_forward_geometry_cache_miss_poisoned(ops, monkeypatch, weights):
    """The cache entry (ops.scratch) is poisoned on the miss; the hit that follows reuses it.  Both equal the plain call."""
    B, N, M = 2, 330, 170
    wl = ops.deformer_weight_list(weights, "cuda")
    f1, f2, v1, v2, s1, s2 = [t.cuda() for t in _pair_inputs(B, N, M, 9)]
    f1b, f2b = f1.flip(1).contiguous(), f2.flip(1).contiguous()

    def run(poison):
        cache = ops.GeometryCache()
        miss = ops.pair_forward(wl, f1, f2, v1, v2, 60.0, s1, s2, cache=cache, key="k")
        hit = ops.pair_forward(wl, f1b, f2b, v1, v2, 60.0, s1, s2, cache=cache, key="k")
        assert (cache.hits, cache.misses) == (1, 1)
        return miss, hit
    got = hygiene(ops, monkeypatch, run)
    P = PoisonedScratch(0x00)
    P.install(ops, monkeypatch)
    for i, (a, b) in enumerate(((f1, f2), (f1b, f2b))):
        plain = ops.pair_forward(wl, a, b, v1, v2, 60.0, s1, s2)
        for side in (0, 1):
            for k, v in plain[side].items():
                assert torch.equal(got["out[%d][%d].%s" % (i, side, k)], v.cpu()), (i, side, k)
    P.release()


def test_pair_pipeline_prefetch_waits_for_its_conversions(ops, weights):
    """float64 / non-contiguous coordinates and int64 starts are converted on the current stream inside prefetch(); the geometry
    stream must wait for those copies, not only for `ready`.  `ready` is recorded, then the current stream is held up, then prefetch
    runs: a geometry call that waits only for `ready` reads the copies before they land.  Blocks of the copies' sizes are zeroed and
    released first, so such a read sees finite in-range zeros (non-zero starts: a stale 0 shows as a different graph)."""
    B, N, M = 2, 300, 170
    wl = ops.deformer_weight_list(weights, "cuda")
    f1, f2, v1, v2, _, _ = [t.cuda() for t in _pair_inputs(B, N, M, 4242)]
    s1 = torch.tensor([17, 250], dtype=torch.int32, device="cuda")
    s2 = torch.tensor([99, 3], dtype=torch.int32, device="cuda")
    ref = ops.pair_forward(wl, f1, f2, v1, v2, 50.0, s1, s2)
    ref = [{k: v.clone() for k, v in r.items()} for r in ref]
    v1_64 = v1.double()
    v2_nc = torch.empty(B, 3, M, device="cuda").transpose(1, 2)   # non-contiguous view
    v2_nc.copy_(v2)
    s1_64, s2_64 = s1.long(), s2.long()
    torch.cuda.synchronize()
    pipe = ops.PairPipeline(wl, B, N, M)
    z = [torch.zeros(B, N, 3, device="cuda"), torch.zeros(B, M, 3, device="cuda"), torch.zeros(B, dtype=torch.int32, device="cuda"),
         torch.zeros(B, dtype=torch.int32, device="cuda")]
    torch.cuda.synchronize()
    del z
    ready = torch.cuda.Event()
    ready.record()
    torch.cuda._sleep(40_000_000)     # ~20 ms of spinning on the current stream after `ready`
    tk = pipe.prefetch(v1_64, v2_nc, s1_64, s2_64, ready=ready)
    o12, o21 = pipe.forward(tk, f1, f2, 50.0)
    torch.cuda.synchronize()
    pipe.close()
    for side, o in ((0, o12), (1, o21)):
        for k in ref[side]:
            assert torch.equal(o[k], ref[side][k]), (side, k)


def test_pair_pipeline_refuses_another_pipelines_ticket(ops, weights):
    B, N, M = 2, 300, 170
    wl = ops.deformer_weight_list(weights, "cuda")
    f1, f2, v1, v2, s1, s2 = [t.cuda() for t in _pair_inputs(B, N, M, 7)]
    a, b = ops.PairPipeline(wl, B, N, M), ops.PairPipeline(wl, B, N, M)
    tk = a.prefetch(v1, v2, s1, s2)
    with pytest.raises(ops.DvmError, match="another pipeline"):
        b.forward(tk, f1, f2, 50.0)
    got = a.forward(tk, f1, f2, 50.0)
    ref = ops.pair_forward(wl, f1, f2, v1, v2, 50.0, s1, s2)
    for side in (0, 1):
        for k in ref[side]:
            assert torch.equal(got[side][k], ref[side][k]), (side, k)
    a.close(), b.close()


# ------------------------------------------------------------------------------------------------------------------ K1 / argmin
def _features(kind, B, rows, seed):
    g = torch.Generator().manual_seed(seed)
    f = torch.randn(B, rows, 128, generator=g)
    return 0.3 * torch.relu(f) if kind == "trained" else f


def _check_softcorr(got, f1, f2, alpha, topk):
    """The bars of tests/test_gpu_parity.py::check_softcorr."""
    for b in range(f1.shape[0]):
        oval, oidx, osmax, osum = O.softcorr(f1[b].numpy(), f2[b].numpy(), alpha, topk=topk)
        assert np.array_equal(got["out[1]"][b].numpy(), oidx), "top-k columns differ from the oracle"
        np.testing.assert_array_equal(got["out[2]"][b].numpy(), osmax)
        np.testing.assert_allclose(got["out[3]"][b].numpy(), osum, rtol=2e-5)
        np.testing.assert_allclose(got["out[0]"][b].numpy(), oval, rtol=5e-5, atol=1e-30)


@pytest.mark.parametrize("variant", [1, 2, 3])
@pytest.mark.parametrize("kind,alpha", [("randn", 100.0), ("trained", 33.0), ("trained", 10.0)], ids=["coarse", "full33", "full10"])
@pytest.mark.parametrize("shape", [(2, 300, 170), (1, 150, 5), (1, 2048, 2048)], ids=["ragged", "M<topk", "contract"])
def test_softcorr_poisoned_scratch(ops, monkeypatch, shape, kind, alpha, variant):
    B, N, M = shape
    f1, f2 = _features(kind, B, N, N + 1), _features(kind, B, M, M + 2)
    d1, d2 = f1.cuda(), f2.cuda()
    got = hygiene(ops, monkeypatch, lambda poison: ops.softcorr(d1, d2, alpha, topk=10, variant=variant))
    _check_softcorr(got, f1, f2, alpha, 10)


@pytest.mark.parametrize("variant", [1, 2])
@pytest.mark.parametrize("shape,alpha", [((2, 300, 170, 128), 10.0), ((1, 130, 333, 128), 100.0), ((1, 2048, 2048, 128), 37.5)],
                         ids=["ragged", "ragged100", "contract"])
def test_softcorr_bwd_poisoned_scratch(ops, monkeypatch, shape, alpha, variant):
    """Against TR.softcorr_bwd (fp64 autograd) at the bars of tests/test_gpu_backward.py::test_softcorr_bwd_vs_fp64_autograd."""
    B, N, M, d = shape
    g = torch.Generator().manual_seed(N * 1000 + M)
    scale = 0.25 if alpha >= 30 else 1.0
    f1, f2 = (torch.randn(B, N, d, generator=g) * scale).cuda(), (torch.randn(B, M, d, generator=g) * scale).cuda()
    gval = torch.randn(B, N, 10, generator=g).cuda()
    val, idx, smax, ssum = ops.softcorr(f1, f2, alpha)
    tol = 1e-4 if alpha <= 40 else 1e-3
    # (both gradients are accumulated with fp32 atomics: run to run they agree to rounding, at the parity test's bar)
    got = hygiene(ops, monkeypatch, lambda poison: ops.softcorr_bwd(f1, f2, alpha, val, idx, smax, ssum, gval, variant=variant),
                  tol={"out[0]": tol, "out[1]": tol})
    _, rf1, rf2 = TR.softcorr_bwd(f1.cpu(), f2.cpu(), ops.neg_alpha_f32(alpha), idx.cpu(), gval.cpu())
    assert rel(got["out[0]"], rf1) < tol and rel(got["out[1]"], rf2) < tol, (rel(got["out[0]"], rf1), rel(got["out[1]"], rf2))


@pytest.mark.parametrize("shape", [(2, 300, 170), (1, 150, 5), (1, 2048, 2048)], ids=["ragged", "M<topk", "contract"])
def test_argmin_poisoned_scratch(ops, monkeypatch, shape):
    B, N, M = shape
    f1, f2 = _features("randn", B, N, 11), _features("randn", B, M, 12)
    d1, d2 = f1.cuda(), f2.cuda()
    got = hygiene(ops, monkeypatch, lambda poison: (ops.argmin_exact(d1, d2, want_dist=True), ops.argmin_pair(d1, d2)))
    full = ops.argmin_exact(d1, d2, screen=False).cpu()
    for b in range(B):
        assert np.array_equal(got["out[0][0]"][b].numpy(), O.argmin_exact(f1[b].numpy(), f2[b].numpy())[0])
        assert np.array_equal(got["out[1][1]"][b].numpy(), O.argmin_exact(f2[b].numpy(), f1[b].numpy())[0])
    assert torch.equal(got["out[0][0]"], full) and torch.equal(got["out[1][0]"], full)


# ------------------------------------------------------------------------------------------------------------------ geometry
@pytest.mark.parametrize("N", [300, 2048, 4995])
def test_fps_dg_build_poisoned_scratch(ops, monkeypatch, N):
    g = torch.Generator().manual_seed(N)
    v = torch.rand(2, N, 3, generator=g)
    start = torch.tensor([N // 3, N - 1], dtype=torch.int32)
    dv, ds = v.cuda(), start.cuda()
    got = hygiene(ops, monkeypatch, lambda poison: (ops.fps(dv, N // 2, ds), ops.dg_build(dv, ds)))
    for b in range(2):
        assert np.array_equal(got["out[0]"][b].numpy(), O.fps(v[b].numpy(), N // 2, int(start[b])))
        if N <= 2048:
            ob = O.dg_build(v[b].numpy(), int(start[b]))
            for key in ("nodes_idx", "one_ring", "infl_idx", "dists"):
                assert np.array_equal(got["out[1].%s" % key][b].numpy(), ob[key]), key
            np.testing.assert_allclose(got["out[1].weights"][b].numpy(), ob["weights"], rtol=0, atol=2e-7)


@pytest.mark.parametrize("shape", [(2, 300, 170), (1, 2048, 2048), (2, 40000, 300)], ids=["ragged", "contract", "grid40000"])
def test_chamfer_fwd_bwd_poisoned_scratch(ops, monkeypatch, shape):
    B, N, M = shape
    g = torch.Generator().manual_seed(N + M)
    a, b = torch.rand(B, N, 3, generator=g), torch.rand(B, M, 3, generator=g)
    g1, g2 = torch.randn(B, N, generator=g), torch.randn(B, M, generator=g)
    da, db, dg1, dg2 = a.cuda(), b.cuda(), g1.cuda(), g2.cuda()

    def run(poison):
        d1, d2, i1, i2 = ops.chamfer(da, db)
        return (d1, d2, i1, i2), ops.chamfer_bwd(da, db, i1, i2, dg1, dg2)
    # (the backward scatters into both clouds' gradients with fp32 atomics: compared at 1e-5, the bar of test_chamfer_bwd_vs_autograd)
    got = hygiene(ops, monkeypatch, run, tol={"out[1][0]": 1e-5, "out[1][1]": 1e-5})
    for bb in range(B):
        od1, od2, oi1, oi2 = O.chamfer(a[bb].numpy(), b[bb].numpy())
        assert np.array_equal(got["out[0][0]"][bb].numpy(), od1) and np.array_equal(got["out[0][1]"][bb].numpy(), od2)
        assert np.array_equal(got["out[0][2]"][bb].numpy(), oi1) and np.array_equal(got["out[0][3]"][bb].numpy(), oi2)


@pytest.mark.parametrize("shape,C,k", [((2, 300, 170), 3, 10), ((1, 1024, 1024), 3, 10), ((2, 150, 90), 7, 5)], ids=["ragged", "contract", "C7"])
def test_knn_cdist_poisoned_scratch(ops, monkeypatch, shape, C, k):
    B, N, M = shape
    g = torch.Generator().manual_seed(N * C)
    x, y = torch.randn(B, N, C, generator=g), torch.randn(B, M, C, generator=g)
    dx, dy = x.cuda(), y.cuda()
    got = hygiene(ops, monkeypatch, lambda poison: ops.knn_cdist(dx, dy, k))
    for b in range(B):
        assert np.array_equal(got["out"][b].numpy(), O.knn_cdist(x[b].numpy(), y[b].numpy(), k))


@pytest.mark.parametrize("shape,C,k", [((2, 300, 300), 64, 20), ((1, 1100, 1100), 128, 500), ((2, 515, 515), 128, 40)],
                         ids=["ragged", "k500", "contract"])
def test_knn_neg_poisoned_scratch(ops, monkeypatch, shape, C, k):
    B, N, M = shape
    g = torch.Generator().manual_seed(N + k)
    x = torch.randn(B, N, C, generator=g)
    dx = x.cuda()
    got = hygiene(ops, monkeypatch, lambda poison: ops.knn_neg(dx, dx, k))
    for b in range(B):
        ref = O.knn_neg(x[b].numpy(), x[b].numpy(), k)
        assert np.array_equal(got["out"][b].numpy(), ref)


# ------------------------------------------------------------------------------------------------------------------ Deformer
@pytest.mark.parametrize("variant", [0, 1, 2, 3])
@pytest.mark.parametrize("name", ["deformer_256x256", "deformer_300x200"])
def test_deformer_and_map_term_poisoned_scratch(ops, monkeypatch, weights, name, variant):
    g = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
    wl = ops.deformer_weight_list(weights, "cuda")
    f1, f2, v1, v2 = (torch.from_numpy(g[k]).cuda() for k in ("feat1", "feat2", "verts1", "verts2"))
    fps1 = torch.from_numpy(g["fps1"]).cuda()
    val, idx, _, _ = ops.softcorr(f1, f2, float(g["alpha"]))
    v12 = ops.apply(val, idx, v2)
    idx11, idx22 = ops.knn_cdist(v1, v1, 10), ops.knn_cdist(v2, v2, 10)
    got = hygiene(ops, monkeypatch, lambda poison: (ops.deformer(wl, f1, f2, v1, v12, idx11, idx22, val, idx, fps1, variant=variant),
                                                    ops.map_term(v12, v2, idx11, idx22, val, idx)))
    h = lambda t: t.cpu().numpy()  # noqa: E731
    for b in range(f1.shape[0]):
        o = O.deformer(weights, g["feat1"][b], g["feat2"][b], g["verts1"][b], h(v12)[b], h(idx11)[b], h(idx22)[b], h(val)[b], h(idx)[b],
                       g["fps1"][b])
        np.testing.assert_allclose(got["out[0]"][b].numpy(), o, rtol=0, atol=5e-6)
        om = O.map_term(h(v12)[b], g["verts2"][b], h(idx11)[b], h(idx22)[b], h(val)[b], h(idx)[b])
        np.testing.assert_allclose(float(got["out[1]"][b]), float(om), rtol=1e-4)


def _mlp64(weights, z):
    W = [weights["deformation_decoder_layer__linear__%d__weight" % i].astype(np.float64) for i in (0, 2, 4, 6)]
    bb = [weights["deformation_decoder_layer__linear__%d__bias" % i].astype(np.float64) for i in (0, 2, 4, 6)]
    x = z.astype(np.float64)
    for i in range(4):
        x = x @ W[i].T + bb[i]
        if i < 3:
            with np.errstate(over="ignore"):   # (np.where evaluates expm1 on the positive entries too)
                x = np.where(x > 0, x, np.expm1(x))
    return x


@pytest.mark.parametrize("rows", [1, 65, 2 * 256 * 64 + 77, "fallback"])
def test_deformer_mlp_poisoned_scratch(ops, monkeypatch, weights, rows):
    """The persistent fp16 form at row counts below / above a block and beyond one wave of workgroups, and the fp16 range fallback
    (its flag lives in the workspace) — against the fp64 MLP at the bars of the parity suite."""
    wl = ops.deformer_weight_list(weights, "cuda")
    g = torch.Generator().manual_seed(3)
    if rows == "fallback":
        z = torch.randn(2, 100, 262, generator=g)
        z[0, :50] *= 4000.0
    else:
        z = torch.randn(1, rows, 262, generator=g)
        z[..., :3] = torch.rand(1, rows, 3, generator=g)
    dz = z.cuda()
    got = hygiene(ops, monkeypatch, lambda poison: ops.deformer_mlp(wl, dz))
    x = _mlp64(weights, z.numpy())
    np.testing.assert_allclose(got["out"].numpy(), x, rtol=2e-5, atol=2e-5 * np.abs(x).max())
    if rows == "fallback":   # the 150 ordinary rows at their own scale (tests/test_gpu_deformer_mlp_adversarial.py: the per-family bar)
        plain = np.ones((2, 100), bool)
        plain[0, :50] = False
        noise = np.abs(_mlp32(weights, z.numpy()[plain]) - x[plain]).max()
        assert noise > 0 and np.abs(got["out"].numpy()[plain] - x[plain]).max() <= 3 * noise


def _mlp32(weights, z):
    """the fp32 chain (numpy, exp(x) - 1): its error against _mlp64 is the yardstick of the per-row bars"""
    x = z.astype(np.float32)
    for n, i in enumerate((0, 2, 4, 6)):
        x = (x @ weights["deformation_decoder_layer__linear__%d__weight" % i].T
             + weights["deformation_decoder_layer__linear__%d__bias" % i]).astype(np.float32)
        if n < 3:
            x = np.where(x > 0, x, np.exp(np.minimum(x, np.float32(0))) - np.float32(1)).astype(np.float32)
    return x


def test_deformer_mlp_weight_flag_poisoned_scratch(ops, monkeypatch, weights):
    """One weight of layer 1 beyond 60000 / 256: the range flag is raised by the PACKING kernel (no activation overflows on the
    small rows), on poisoned scratch; the gated bf16x3 launch answers.  Every row within 3 x the fp32 chain's error against
    float64 with these weights."""
    w = dict(weights)
    w["deformation_decoder_layer__linear__2__weight"] = w["deformation_decoder_layer__linear__2__weight"].copy()
    w["deformation_decoder_layer__linear__2__weight"][7, 300] = 250.0
    wl = ops.deformer_weight_list(w, "cuda")
    g = torch.Generator().manual_seed(4)
    z = torch.randn(200, 262, generator=g)
    z[100:] *= 1e-4
    dz = z.cuda()
    got = hygiene(ops, monkeypatch, lambda poison: ops.deformer_mlp(wl, dz))
    x = _mlp64(w, z.numpy())
    for part in (slice(0, 100), slice(100, 200)):
        noise = np.abs(_mlp32(w, z.numpy()[part]) - x[part]).max()
        assert noise > 0 and np.abs(got["out"].numpy()[part] - x[part]).max() <= 3 * noise, (part, noise)


# ------------------------------------------------------------------------------------------------------------------ backbone
def test_pos_encoding_and_bn_poisoned_scratch(ops, monkeypatch, deterministic):
    """pos_encoding (its range reduction in scratch) and the fused training BatchNorm, channel-major and point-major, fwd + bwd.
    Reference: torch's batch_norm in fp64 (the layer these kernels replace)."""
    g = torch.Generator().manual_seed(8)
    x = torch.rand(2, 3, 301, generator=g).cuda()
    xb = torch.randn(3, 128, 257, generator=g).cuda()
    res = torch.randn(3, 128, 257, generator=g).cuda()
    gamma, beta = (0.5 + torch.rand(128, generator=g)).cuda(), torch.randn(128, generator=g).cuda()
    dy = torch.randn(3, 128, 257, generator=g).cuda()
    xp, dyp = xb.transpose(1, 2).contiguous(), dy.transpose(1, 2).contiguous()

    def run(poison):
        pe = ops.pos_encoding(x)
        y, m, s = ops.bn_act_train_fwd(xb, res, gamma, beta, 1e-5, 0.2, 0.1)
        bwd = ops.bn_act_train_bwd(dy, y, xb, res, gamma, m, s, 0.2)
        yp, mp, sp = ops.bn_act_train_fwd_pm(xp, None, gamma, beta, 1e-5, 0.2, 0.1)
        bwdp = ops.bn_act_train_bwd_pm(dyp, yp, xp, None, gamma, mp, sp, 0.2)
        return pe, (y, m, s), bwd, (yp, mp, sp), bwdp
    got = hygiene(ops, monkeypatch, run)
    for name, xin, r in (("cm", xb, res), ("pm", xb, None)):
        a = (xin.double() + (r.double() if r is not None else 0)).detach().requires_grad_(True)
        ga, be = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
        t = torch.nn.functional.batch_norm(a, None, None, ga, be, training=True, eps=1e-5)
        yref = torch.where(t > 0, t, t * 0.2)
        (yref * dy.double()).sum().backward()
        if name == "cm":
            y, dx, dgam, dbet = got["out[1][0]"], got["out[2][0]"], got["out[2][1]"], got["out[2][2]"]
        else:
            y, dx, dgam, dbet = got["out[3][0]"].transpose(1, 2), got["out[4][0]"].transpose(1, 2), got["out[4][1]"], got["out[4][2]"]
        assert rel(y, yref) < 2e-6, name      # the bars of tests/test_gpu_backward.py::test_fused_batchnorm_vs_torch
        assert rel(dx, a.grad) < 2e-5 and rel(dgam, ga.grad) < 2e-5 and rel(dbet, be.grad) < 2e-5, name


@pytest.mark.parametrize("C,K,N", [(64, 40, 300), (128, 7, 257), (128, 1, 5)])
def test_n2p_core_poisoned_scratch(ops, monkeypatch, deterministic, C, K, N):
    """Against the fp64 formulation of tests/test_gpu_backward.py::test_n2p_core_fwd_bwd_vs_fp64_autograd (models/model.py:339-350)."""
    B, H = 2, 4
    g = torch.Generator().manual_seed(C + K + N)
    qkv = torch.randn(B, N, 3 * C, generator=g)
    idx = torch.randint(0, N, (B, N, K), generator=g, dtype=torch.int32)
    gout = torch.randn(B, N, C, generator=g)
    dq, di, dg = qkv.cuda(), idx.cuda(), gout.cuda()

    def run(poison):
        out, attn = ops.n2p_core_fwd(dq, di, H)
        return out, attn, ops.n2p_core_bwd(dq, di, attn, dg, H)
    got = hygiene(ops, monkeypatch, run)
    x = qkv.double().requires_grad_(True)
    q, kp, vp = x[..., :C], x[..., C:2 * C], x[..., 2 * C:]
    gi = idx.long().reshape(B, N * K, 1).expand(-1, -1, C)
    kd = (torch.gather(kp, 1, gi).view(B, N, K, C) - kp[:, :, None]).view(B, N, K, H, C // H)
    vd = (torch.gather(vp, 1, gi).view(B, N, K, C) - vp[:, :, None]).view(B, N, K, H, C // H)
    e = (q.view(B, N, 1, H, C // H) * kd).sum(-1) / (C // H) ** 0.5
    a = torch.softmax(e, dim=2)
    ref = (a.unsqueeze(-1) * vd).sum(2).reshape(B, N, C)
    (ref * gout.double()).sum().backward()
    assert rel(got["out[0]"], ref) < 1e-5 and rel(got["out[1]"], a) < 1e-5
    assert rel(got["out[2]"], x.grad) < 1e-5


@pytest.mark.parametrize("B,N", [(2, 300), (3, 77), (1, 1000), (1, 1100)])
def test_sa_attention_poisoned_scratch(ops, monkeypatch, deterministic, B, N):
    """Eval and training forms and the backward, against tests/test_gpu_backward.py::test_sa_core_fwd_bwd_vs_fp64_autograd's
    fp64 formulation (models/model.py:113-121)."""
    g = torch.Generator().manual_seed(N)
    p = torch.randn(B, N, 16, generator=g) * 0.7
    v = torch.randn(B, N, 64, generator=g)
    gx = torch.randn(B, N, 64, generator=g)
    dp_, dv_, dgx = p.cuda(), v.cuda(), gx.cuda()

    def run(poison):
        xr = ops.sa_attention_pm(dp_, dv_)
        xt, st, ci = ops.sa_attention_train_fwd(dp_, dv_)
        return xr, (xt, st, ci), ops.sa_attention_bwd(dp_, dv_, xt, st, ci, dgx)
    got = hygiene(ops, monkeypatch, run)
    p64, v64 = p.double().requires_grad_(True), v.double().requires_grad_(True)
    att = torch.softmax(torch.bmm(p64, p64.transpose(1, 2)), dim=-1)
    att = att / (1e-9 + att.sum(dim=1, keepdim=True))
    ref = torch.bmm(att.transpose(1, 2), v64)
    (ref * gx.double()).sum().backward()
    assert rel(got["out[0]"], ref) < 1e-5 and rel(got["out[1][0]"], ref) < 1e-5
    assert rel(got["out[2][1]"], v64.grad) < 1e-4 and rel(got["out[2][0]"], p64.grad) < 1e-4


@pytest.mark.parametrize("C", [3, 128, 200])
def test_apply_bwd_poisoned_scratch(ops, monkeypatch, deterministic, C):
    """The gather form (workspace: reversed lists), against tests/test_gpu_backward.py::test_sparse_apply_bwd_vs_fp64_autograd."""
    B, N, M, k = 2, 190, 75, 10
    g = torch.Generator().manual_seed(C)
    val = torch.rand(B, N, k, generator=g)
    idx = torch.randint(0, M, (B, N, k), generator=g, dtype=torch.int32)
    idx[1, :40] = 5
    V, gout = torch.randn(B, M, C, generator=g), torch.randn(B, N, C, generator=g)
    d = [t.cuda() for t in (val, idx, V, gout)]
    # (d_V: the reversed lists are filled through an atomic cursor, so each column's in-edges are summed in a run-dependent order:
    # compared at 1e-5, the bar of test_sparse_apply_bwd_vs_fp64_autograd)
    got = hygiene(ops, monkeypatch, lambda poison: ops.apply_bwd(*d, atomics=False), tol={"out[1]": 1e-5})
    v64, V64 = val.double().requires_grad_(True), V.double().requires_grad_(True)
    rows = torch.gather(V64, 1, idx.long().reshape(B, N * k, 1).expand(-1, -1, C)).view(B, N, k, C)
    ((v64.unsqueeze(-1) * rows).sum(2) * gout.double()).sum().backward()
    assert rel(got["out[0]"], v64.grad) < 1e-5 and rel(got["out[1]"], V64.grad) < 1e-5


@pytest.mark.parametrize("N,nA,k", [(300, 40, 25), (1100, 50, 500)])
def test_dist_loss_poisoned_scratch(ops, monkeypatch, deterministic, N, nA, k):
    """Forward against the reference's formulation (models/loss.py:1351-1396, as tests/test_gpu_backward.py evaluates it in fp64)
    on the kernel's own neighbour sets (their selection and every neighbour slot are pinned per anchor, bit for bit, by
    tests/test_gpu_dist_term_anchors.py; tests/test_gpu_backbone.py::test_dist_loss_vs_torch, which the child run below repeats on
    poisoned scratch, checks the batch sum on random data); the backward weights poisoned == clean."""
    B, C = 2, 128
    g = torch.Generator().manual_seed(N + k)
    feat = torch.randn(B, N, C, generator=g)
    v = torch.rand(B, N, 3, generator=g)
    dist = torch.cdist(v, v)
    anchors = torch.randperm(N, generator=g)[:nA]
    gout = torch.randn(B, generator=g)
    df, dd, da, dgo = feat.cuda(), dist.cuda(), anchors.cuda(), gout.cuda()

    def run(poison):
        out, idx = ops.dist_loss(df, dd, da, k, want_idx=True)
        return out, idx, ops.dist_loss_bwd_weights(df, dd, da, idx, dgo)
    got = hygiene(ops, monkeypatch, run)
    idx = got["out[1]"].long()
    f64 = feat.double()
    f1 = f64[:, anchors]
    f2 = torch.gather(f64, 1, idx.reshape(B, nA * k, 1).expand(-1, -1, C)).view(B, nA, k, C)
    d2 = ((f2 - f1[:, :, None, :]) ** 2).sum(-1)
    x = torch.where(d2 > 0, torch.sqrt(d2.clamp_min(1e-300)), torch.zeros_like(d2))
    y = torch.stack([dist[b].double()[idx[b], anchors[:, None]] for b in range(B)])
    ref = (1 - torch.abs(torch.nn.functional.cosine_similarity(x, y, dim=2))).sum(1)
    assert rel(got["out[0]"], ref) < 1e-5


# ------------------------------------------------------------------------------------------------------------------ training nodes
def _sibling(name):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    try:
        return __import__(name)
    finally:
        sys.path.pop(0)


@pytest.mark.parametrize("B,N", [(2, 256), (1, 64)])
def test_native_criterion_poisoned_arena(ops, monkeypatch, deterministic, B, N):
    """The full criterion's native node (its arena: ops.scratch) fwd + bwd, deterministic, against the per-op autograd path at the
    bars of tests/test_gpu_criterion_native.py."""
    import copy
    cn = _sibling("test_gpu_criterion_native")
    crit, d, featj, v1, v2, starts, anchors = cn._setup(B, N, 5 + N)

    def run(poison):
        c2, d2 = copy.deepcopy(crit), copy.deepcopy(d)
        losses, gfeat, gd, s, m = cn._step(c2, d2, featj, v1, v2, starts, anchors, True)
        return torch.tensor(losses, dtype=torch.float64), gfeat, gd
    # (the gradients go through the soft correspondence's backward, whose fp32 atomics the deterministic switch does not order:
    # compared at 2e-3, the bar of test_native_criterion_equals_autograd_path; the losses bitwise)
    tol = {k: 2e-3 for k in ["out[1]"] + ["out[2].%s" % n for n, _ in d.named_parameters()]}
    got = hygiene(ops, monkeypatch, run, tol=tol)
    la, ga, gda, _, _ = cn._step(copy.deepcopy(crit), copy.deepcopy(d), featj, v1, v2, starts, anchors, False)
    for x, y in zip(got["out[0]"].tolist(), la):
        assert abs(x - y) <= 2e-5 * max(abs(y), 1e-3), (got["out[0]"], la)
    assert cn._rel(got["out[1]"], ga.cpu()) <= 2e-3
    for k in gda:
        assert cn._rel(got["out[2].%s" % k], gda[k].cpu()) <= 2e-3, k


@pytest.mark.parametrize("partial", [True, False], ids=["partial", "full"])
def test_directional_criterion_poisoned_arena(ops, monkeypatch, deterministic, partial):
    """N != M: each direction its own native node (dvm_criterion_dir_train_*), at (301, 212)."""
    import copy
    import models.loss as ml
    import models.model as mm
    B, N, M = 2, 301, 212
    g = torch.Generator().manual_seed(N * 7 + M)
    v1, v2 = (torch.rand(B, N, 3, generator=g) - 0.5).cuda(), (torch.rand(B, M, 3, generator=g) - 0.5).cuda()
    f1 = (0.3 * torch.relu(torch.randn(B, N, 128, generator=g))).cuda().requires_grad_(True)
    f2 = (0.3 * torch.relu(torch.randn(B, M, 128, generator=g))).cuda().requires_grad_(True)
    torch.manual_seed(11)
    d = mm.Deformer(10).cuda().train()
    cls = ml.GraphDeformLoss_Neural_Partial if partial else ml.GraphDeformLoss_Neural
    crit = cls(k_deform=10, w_dist=0.02, w_map=0.005, k_dist=40, N_dist=30, partial=partial, w_deform=0.5, w_img=0, w_rank=0, w_self_rec=0.5,
               w_cd=0.1, w_arap=0.01, save_name="t")
    starts = (torch.randint(0, N, (B,), generator=g), torch.randint(0, M, (B,), generator=g))
    anchors = (random.Random(1).sample(range(N), 30), random.Random(2).sample(range(M), 30))

    def step(native):
        c2, d2 = copy.deepcopy(crit), copy.deepcopy(d)
        c2.native_train = native
        f1.grad = f2.grad = None
        random.seed(5)
        out = c2(f1, f2, torch.cdist(v1, v1), torch.cdist(v2, v2), v1, v2, 45.0, d2, fps_starts=starts, anchors=anchors)
        out[0].backward()
        return (torch.tensor([float(o) for o in out], dtype=torch.float64), f1.grad.clone(), f2.grad.clone(),
                {k: p.grad.clone() for k, p in d2.named_parameters()})
    # (gradients through fp32 atomics the deterministic switch does not order: at 2e-3, the bar of
    # test_directional_node_equals_autograd_path; the losses bitwise)
    tol = {k: 2e-3 for k in ["out[1]", "out[2]"] + ["out[3].%s" % n for n, _ in d.named_parameters()]}
    got = hygiene(ops, monkeypatch, lambda poison: step(True), tol=tol)
    la, g1a, g2a, gda = step(False)
    for x, y in zip(got["out[0]"].tolist(), la.tolist()):
        assert abs(x - y) <= 2e-5 * max(abs(y), 1e-3), (got["out[0]"], la)
    rel = lambda a, b: float((a - b).norm() / (b.norm() + 1e-30))  # noqa: E731
    assert rel(got["out[1]"], g1a.cpu()) <= 2e-3 and rel(got["out[2]"], g2a.cpu()) <= 2e-3
    for k in gda:
        assert rel(got["out[3].%s" % k], gda[k].cpu()) <= 2e-3, k


def test_native_uni3fc_training_poisoned_arena(ops, monkeypatch, deterministic):
    """LG-Net's native training node fwd + bwd at (2, 300): features, running statistics and gradients under a poisoned arena equal
    the clean ones bitwise; the clean step matches the autograd path as in tests/test_gpu_train_native.py."""
    import copy
    tn = _sibling("test_gpu_train_native")
    B, N, k = 2, 300, 20
    a, b = tn._nets(k, seed=N, gain=0.5)
    x, dino = tn._inputs(B, N, 7 + N)
    g = torch.Generator().manual_seed(3)
    gf, gt = torch.randn(B, N, 128, generator=g).cuda(), torch.randn(B, N, 64, generator=g).cuda()
    nets = []

    def run(poison):
        n = copy.deepcopy(a)
        feat, tmp = tn._run(n, x, dino, True, True, gf, gt)
        nets.append(n)
        return feat, tmp, {k_: p.grad for k_, p in n.named_parameters() if p.grad is not None}, dict(n.named_buffers())
    got = hygiene(ops, monkeypatch, run)
    fb, tb = tn._run(b, x, dino, False, True, gf, gt)
    assert torch.equal(got["out[0]"], fb.cpu()) and torch.equal(got["out[1]"], tb.cpu())
    tn._compare(nets[0], b, 2e-4)


# ------------------------------------------------------------------------------------------------------------------ child runs
SUITES = ["test_gpu_parity.py", "test_gpu_backward.py", "test_gpu_backbone.py", "test_gpu_criterion_native.py", "test_gpu_train_native.py"]

_CHILD = r'''
import os, sys
root = sys.argv[1]
sys.path[:0] = [root, os.path.join(root, "dv-matcher_amd"), os.path.join(root, "tests")]
import pytest
from dvm import ops
from test_gpu_scratch_hygiene import PoisonedScratch

class Poison:
    """The poisoning allocator for every test of the run: guards checked and buffers released at each test's teardown."""
    def __init__(self):
        self.p = PoisonedScratch(0xFF)
        self.p.install(ops)
        self.bad = []
    @pytest.hookimpl(hookwrapper=True)
    def pytest_runtest_teardown(self, item):
        yield
        try:
            self.p.check_guards()
        except AssertionError as e:
            self.bad.append("%s: %s" % (item.nodeid, e))
        self.p.release()

plug = Poison()
rc = pytest.main(sys.argv[2:], plugins=[plug])
for b in plug.bad:
    print("GUARD", b)
print("POISONED_SCRATCH_CALLS", "ok" if not plug.bad else "guard bands overwritten")
sys.exit(int(rc) or (3 if plug.bad else 0))
'''


@pytest.mark.parametrize("route", [None, "1"], ids=["probe", "lean"])
def test_gpu_suites_on_poisoned_scratch(route):
    """The parity / backward / backbone / criterion / training suites with every workspace and arena poisoned (0xFF, exact sizes,
    guard bands checked after each test) in a child process.  Their own child-process tests (drivers, forced routes) are skipped:
    the allocator hook would not reach those grandchildren.  route "1": the K1 slice again with the lean first form forced, which
    the probe otherwise picks only near its thresholds."""
    env = dict(os.environ)
    env.pop("DVM_K1_ROUTE", None)
    if route is None:
        files, sel = SUITES, "not driver and not probe_routes"
    else:
        env["DVM_K1_ROUTE"] = route
        files, sel = ["test_gpu_parity.py"], "(softcorr or argmin or pair_forward or pair_direction) and not probe_routes"
    args = [os.path.join(ROOT, "tests", f) for f in files] + ["-m", "gpu", "-q", "-k", sel, "-p", "no:cacheprovider", "-x"]
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT] + args, cwd=ROOT, env=env, capture_output=True, text=True, timeout=1800)
    tail = (r.stdout or "")[-3000:] + (r.stderr or "")[-1000:]
    assert r.returncode == 0, tail
    assert " passed" in r.stdout and "failed" not in r.stdout and "POISONED_SCRATCH_CALLS ok" in r.stdout, tail
