"""The CPU half of tests/test_gpu_attention_rows.py: the SA training forward (both passes, key chunks with their merges), the SA
backward (both passes, the inner-loop split) and the two N2P forwards restated in plain fp32 torch in the kernels' order of
operations (max-shifted exponentials, chunked statistics with merge, u_i = v_i . dv_i - sum_j Ah_ij t_j, the online softmax of the
inference kernel), exp in place of the fast exponential.  Two things are shown with the drivers and bars of tests/attention_ref.py,
the ones the GPU half runs the kernels through:

(a) the unmutated restatement meets every exact planting and every bar on every family and shape of the GPU half (the SA forward
    shapes with N >= 2045 take randn alone here), i.e. a correct fp32 implementation fits the bars;
(b) each planted mutation fails at least one check.  Leaving `- kp_i` out of the logits shifts every logit of a (point, head) by the
    same -q_h . kp_i / sqrt(D), which a softmax does not see: no bar can catch it.  What it changes is where fp32 rounds, so it is
    caught by the `offset` planting of attention_ref.n2p_exact_case alone (kp carries +-2^23, the exact differences sum to 0).

The float64 closed form that attention_ref.sa_ref64 uses for dv / dp is checked here once against float64 autograd of
models/model.py:113-121, and the route mirrors (sa_fwd_route, sa_bwd_route) against the routes the shape lists claim.
"""
import pytest
import torch

import attention_ref as R
from attention_ref import N2P_BN, N2P_CK, SA_BWD_SHAPES, SA_DET_N, SA_FLAT_N, SA_FWD_SHAPES, SA_TAIL_N
from test_gpu_backward_adversarial import n2p_inputs as n2p_base_inputs


@pytest.fixture(scope="module", autouse=True)
def _ratios():
    yield
    print("\nlargest err / bar of the fp32 restatement\n" + R.report("sa") + "\n" + R.report("n2p"))


# ----------------------------------------------------------------------------------------- the fp32 restatements
def sim_sa_forward(p, v, mut=None):
    """dvm_sa_attention_train_fwd_f32 on batched CPU float32: pass 1 per key chunk + merge, pass 2 per key chunk + merge."""
    B, N, _ = p.shape
    _, kchunk, Z = R.sa_fwd_route(B, N)
    chunks = [(z * kchunk, min(N, (z + 1) * kchunk)) for z in range(Z)]
    xr, stats, cinv = torch.empty(B, N, 64), torch.empty(B, N, 2), torch.empty(B, N)
    for b in range(B):
        E = p[b] @ p[b].T
        ms, ls = [], []
        for a, e in chunks:                                                   # pass 1: (m, l) per chunk
            Ez = E[:, a:e]
            if mut == "skip_last_col" and e == N:
                Ez = torch.cat([Ez[:, :-1], torch.full((N, 1), float("-inf"))], 1)
            m = Ez.max(1)[0]
            l = torch.exp(Ez - m[:, None]).sum(1)
            if mut == "pad_col" and e == N:                                   # a padding column (p = 0, E = 0) counted
                m2 = torch.maximum(m, torch.zeros_like(m))
                l, m = l * torch.exp(m - m2) + torch.exp(-m2), m2
            ms.append(m)
            ls.append(l)
        gm = torch.stack(ms).max(0)[0]
        gl = sum(l * torch.exp(m - gm) for m, l in zip(ms, ls))
        st = torch.stack([gm, 1.0 / gl], 1)
        stats[b] = st
        if mut == "next_row_stats":
            st = torch.roll(st, -1, 0)
        cs, acc = [], []
        for a, e in chunks:                                                   # pass 2: keys i of the chunk, all columns j
            w = torch.exp(E[a:e] - st[a:e, :1]) * st[a:e, 1:]
            if mut == "skip_last_row" and e == N:
                w[-1] = 0.0
            cs.append(w.sum(0))
            acc.append(w)
        if mut == "lost_chunk" and Z > 1:
            cs[-1] = torch.zeros_like(cs[-1])
            acc[-1] = torch.zeros_like(acc[-1])
        csum = sum(cs)
        inv = 1.0 / (csum if mut == "no_eps" else torch.tensor(1e-9, dtype=torch.float32) + csum)
        if mut == "ci_for_cj":
            x = sum((w * inv[a:e, None]).T @ v[b, a:e] for (a, e), w in zip(chunks, acc))
        else:
            x = sum(w.T @ v[b, a:e] for (a, e), w in zip(chunks, acc)) * inv[:, None]
        if mut == "swap_v":
            x = x[:, [0, 1, 2, 5, 4, 3] + list(range(6, 64))]
        xr[b], cinv[b] = x, inv
    return xr, stats, cinv


def sim_sa_backward(p, v, xr, stats, cinv, G, mut=None, deterministic=False):
    """dvm_sa_attention_bwd_f32: pass R (u, dv) and pass D (dp), the inner loop cut into the launch's splits."""
    B, N, _ = p.shape
    split, per, ntiles = R.sa_bwd_route(B, N, deterministic)
    dp, dv = torch.zeros_like(p), torch.zeros_like(v)
    for b in range(B):
        E = p[b] @ p[b].T
        m, il, ci = stats[b, :, :1], stats[b, :, 1:], cinv[b]
        t = (G[b] * xr[b]).sum(1)
        u = torch.zeros(N)
        cols = [(sp * per * 32, min(min((sp + 1) * per, ntiles) * 32, N)) for sp in range(split)]
        cols = [(a, e) for a, e in cols if a < e]
        for k, (a, e) in enumerate(cols):
            ah = torch.exp(E[:, a:e] - m) * il * ci[None, a:e]
            part = ah @ G[b, a:e]
            if mut == "lost_split" and k == 0 and len(cols) > 1:
                continue
            ul = torch.zeros(N) if mut == "u_without_Aht" else -(ah * t[None, a:e]).sum(1)
            u += ul + (v[b] * part).sum(1)
            dv[b] += part
        for a, e in cols:
            Aij = torch.exp(E[:, a:e] - m) * il
            Aji = torch.exp(E[:, a:e] - m[a:e].T) * il[a:e].T
            X, Y = v[b] @ G[b, a:e].T, G[b] @ v[b, a:e].T
            dEij = Aij * ((X - t[None, a:e]) * ci[None, a:e] - u[:, None])
            dEji = Aji * ((Y - t[:, None]) * ci[:, None] - u[None, a:e])
            dp[b] += (dEij if mut == "no_dEji" else dEij + dEji) @ p[b, a:e]
    if mut == "swap_dp":                                                      # two channels of the pcol permutation exchanged
        dp = dp[:, :, [0, 1, 2, 5, 4, 3] + list(range(6, 16))]
    return dp, dv


def _n2p_parts(q, kp, vp, idx):
    B, N, C = q.shape
    Kn = idx.shape[-1]
    gi = idx.long().reshape(B, N * Kn, 1).expand(-1, -1, C)
    return torch.gather(kp, 1, gi).view(B, N, Kn, C), torch.gather(vp, 1, gi).view(B, N, Kn, C)


def _n2p_logits(q, kp, kj, mut):
    B, N, Kn, C = kj.shape
    D = C // 4
    kd = kj if mut == "no_kp_i" else kj - kp[:, :, None]
    e = (q.view(B, N, 1, 4, D) * kd.view(B, N, Kn, 4, D)).sum(-1) / (float(D) if mut == "div_D" else torch.tensor(float(D)).sqrt())
    return torch.roll(e, -1, 3) if mut == "next_head" else e


def _n2p_tail(out, mut):
    """The tail wave (row clamped to N - 1) writing what it computed, at its own unclamped row: rows 0.. of the next cloud."""
    if mut == "tail_writes":
        B, N = out.shape[:2]
        for b in range(B - 1):
            out[b + 1, :min(N, (4 - N % 4) % 4)] = out[b, N - 1]
    return out


def sim_n2p_core(qkv, idx, mut=None):
    """n2p_core_fwd_kernel: logits, max, exponentials, one division, weights, out."""
    C = qkv.shape[-1] // 3
    q, kp, vp = qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:]
    kj, vj = _n2p_parts(q, kp, vp, idx)
    B, N, Kn, _ = kj.shape
    e = _n2p_logits(q, kp, kj, mut)
    w = torch.exp(e - e.max(2, keepdim=True)[0])
    if mut == "skip_last_slot":
        w[:, :, -1] = 0.0
    a = w * (1.0 / w.sum(2, keepdim=True))
    vd = vj if mut == "no_vp_i" else vj - vp[:, :, None]
    out = (a.unsqueeze(-1) * vd.view(B, N, Kn, 4, C // 4)).sum(2).reshape(B, N, C)
    return _n2p_tail(out, mut), _n2p_tail(a, mut)


def sim_n2p_pm(q, kp, vp, idx, mut=None):
    """n2p_attention_kernel: the online softmax, one neighbour per step."""
    kj, vj = _n2p_parts(q, kp, vp, idx)
    B, N, Kn, C = kj.shape
    e = _n2p_logits(q, kp, kj, mut)
    m = torch.full((B, N, 4), float("-inf"))
    l = torch.zeros(B, N, 4)
    acc = torch.zeros(B, N, 4, C // 4)
    for j in range(Kn - 1 if mut == "skip_last_slot" else Kn):
        mn = torch.maximum(m, e[:, :, j])
        sc, w = torch.exp(m - mn), torch.exp(e[:, :, j] - mn)
        l = l * sc + w
        vd = vj[:, :, j] if mut == "no_vp_i" else vj[:, :, j] - vp
        acc = w.unsqueeze(-1) * vd.view(B, N, 4, C // 4) + acc * sc.unsqueeze(-1)
        m = mn
    return _n2p_tail((acc * (1.0 / l).unsqueeze(-1)).reshape(B, N, C), mut)


# ----------------------------------------------------------------------------------------- the references themselves
def test_closed_form_matches_float64_autograd():
    """attention_ref.sa_ref64 uses the closed form of csrc/dvm_sa_bwd.hip's header; here it is held against float64 autograd of
    models/model.py:113-121 once (hub25 has column sums near 1e-9)."""
    for family in ("randn", "hub25", "dup_pairs"):
        p, v, G = R.sa_inputs(family, 1, 90, seed=3)
        ref = R.sa_ref64(p[0], v[0], G[0])
        xr, dv, dp = R.sa_autograd64(p[0], v[0], G[0])
        for name, x in (("xr", xr), ("dv", dv), ("dp", dp)):
            assert float((ref[name] - x).norm() / x.norm()) < 1e-11, (family, name)


def test_route_mirrors_select_the_listed_routes():
    for (B, N), (S, Z) in SA_FWD_SHAPES.items():
        assert R.sa_fwd_route(B, N)[0::2] == (S, Z), (B, N, R.sa_fwd_route(B, N))
    assert R.sa_fwd_route(1, 2100)[1] == 640
    assert R.sa_fwd_route(1, 1024)[2] == 2 and R.sa_fwd_route(1, 2048)[2] == 4      # the flat planting's chunked shapes
    for (B, N), split in SA_BWD_SHAPES.items():
        assert R.sa_bwd_route(B, N)[0] == split, (B, N, R.sa_bwd_route(B, N))
    split, per, ntiles = R.sa_bwd_route(1, 1030)
    assert (split - 1) * per > ntiles                                       # the last split is empty, its t0 past ntiles
    for N in SA_DET_N + SA_TAIL_N:
        assert R.sa_bwd_route(3, N, deterministic=True)[0] == 1
    assert all(R.sa_fwd_route(3, N)[2] == 1 for N in SA_TAIL_N)


# ----------------------------------------------------------------------------------------- (a) the restatement meets everything
@pytest.mark.parametrize("N", SA_FLAT_N)
def test_sa_flat_exact(N):
    R.sa_flat_case(sim_sa_forward, sim_sa_backward, 1, N)


@pytest.mark.parametrize("BN", list(SA_FWD_SHAPES), ids=str)
def test_sa_forward_shapes(BN):
    B, N = BN
    for family in (["randn"] if N >= 2045 else R.SA_FAMILIES):
        R.sa_run_case(sim_sa_forward, None, family, B, N, seed=N + B, backward=False)


@pytest.mark.parametrize("BN", list(SA_BWD_SHAPES), ids=str)
def test_sa_backward_shapes(BN):
    B, N = BN
    for family in (["randn", "hub25"] if B * N >= 2048 else R.SA_FAMILIES):
        R.sa_run_case(sim_sa_forward, sim_sa_backward, family, B, N, seed=N + B)


@pytest.mark.parametrize("N", SA_DET_N)
def test_sa_backward_unsplit(N):
    det = lambda *a: sim_sa_backward(*a, deterministic=True)    # noqa: E731
    for family in ("randn", "hub25"):
        R.sa_run_case(sim_sa_forward, det, family, 1, N, seed=N)


@pytest.mark.parametrize("N", SA_TAIL_N)
def test_sa_tails(N):
    for family in R.SA_FAMILIES:
        R.sa_run_case(sim_sa_forward, sim_sa_backward, family, 3, N, seed=N)


@pytest.mark.parametrize("C,Kn", N2P_CK)
@pytest.mark.parametrize("B,N", N2P_BN)
def test_n2p_families(B, N, C, Kn):
    for family in R.N2P_FAMILIES:
        R.n2p_run_case(n2p_base_inputs, sim_n2p_core, sim_n2p_pm, family, B, N, C, Kn, seed=B * N + Kn + C)


@pytest.mark.parametrize("C", [64, 128])
@pytest.mark.parametrize("B,N", N2P_BN)
@pytest.mark.parametrize("kind", ["k1", "q0", "same", "offset"])
def test_n2p_exact(kind, B, N, C):
    R.n2p_exact_case(sim_n2p_core, sim_n2p_pm, kind, B, N, C, seed=N + C)


# ----------------------------------------------------------------------------------------- (b) every mutation is caught
SA_MUTATIONS = ["no_eps", "ci_for_cj", "no_dEji", "skip_last_row", "skip_last_col", "swap_v", "next_row_stats", "lost_chunk",
                "lost_split", "u_without_Aht", "pad_col", "swap_dp"]
N2P_MUTATIONS = ["next_head", "skip_last_slot", "no_vp_i", "no_kp_i", "div_D", "tail_writes"]


def _failures(cases):
    failed = []
    for name, run in cases:
        try:
            run()
        except AssertionError:
            failed.append(name)
    return failed


def _sa_cases(fwd, bwd):
    cases = [("flat %d" % N, lambda N=N: R.sa_flat_case(fwd, bwd, 1, N)) for N in (2, 128, 1024)]
    for family, B, N in (("randn", 3, 77), ("hub25", 3, 77), ("hub100", 3, 77), ("dup_all", 3, 33), ("randn", 1, 256), ("randn", 1, 1023)):
        cases.append(("%s (%d,%d)" % (family, B, N), lambda f=family, B=B, N=N: R.sa_run_case(fwd, bwd, f, B, N, seed=N + B, record=False)))
    return cases


def test_sa_unmutated_passes_the_mutation_cases():
    assert _failures(_sa_cases(sim_sa_forward, sim_sa_backward)) == []


@pytest.mark.parametrize("mut", SA_MUTATIONS)
def test_sa_mutation_is_caught(mut):
    fwd = lambda p, v: sim_sa_forward(p, v, mut=mut)            # noqa: E731
    bwd = lambda *a: sim_sa_backward(*a, mut=mut)               # noqa: E731
    failed = _failures(_sa_cases(fwd, bwd))
    print(mut, "fails", failed)
    assert failed, "mutation %s passes every check" % mut


def _n2p_cases(core, pm):
    cases = []
    for kind, C in (("k1", 64), ("q0", 64), ("same", 64), ("offset", 64), ("offset", 128)):
        cases.append(("exact %s C %d" % (kind, C), lambda k=kind, C=C: R.n2p_exact_case(core, pm, k, 2, 5, C, seed=1)))
    for family, B, N, C, Kn in (("random", 2, 5, 64, 3), ("random", 3, 1030, 64, 40), ("peaked", 2, 5, 128, 64), ("tie", 3, 1030, 128, 3)):
        cases.append(("%s C %d K %d (%d,%d)" % (family, C, Kn, B, N), lambda f=family, B=B, N=N, C=C, Kn=Kn: R.n2p_run_case(
            n2p_base_inputs, core, pm, f, B, N, C, Kn, seed=N + Kn, record=False)))
    return cases


@pytest.mark.parametrize("mut", N2P_MUTATIONS)
def test_n2p_mutation_is_caught(mut):
    core = lambda qkv, idx: sim_n2p_core(qkv, idx, mut=mut)     # noqa: E731
    pm = lambda *a: sim_n2p_pm(*a, mut=mut)                     # noqa: E731
    failed = _failures(_n2p_cases(core, pm))
    print(mut, "fails", failed)
    assert failed, "mutation %s passes every check" % mut
    if mut != "tail_writes":                                                # the inference kernel's tail waves return before any write
        failed = _failures(_n2p_cases(sim_n2p_core, pm))
        assert failed, "mutation %s of the inference form alone passes every check" % mut
    failed = _failures(_n2p_cases(core, sim_n2p_pm))
    assert failed, "mutation %s of the training forward alone passes every check" % mut
