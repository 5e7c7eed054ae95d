"""Float64 references, input families and per-row bars of the two attention cores of LG-Net: the SA core (csrc/dvm_sa.hip training
forward, csrc/dvm_sa_bwd.hip) and the N2P core's forwards (n2p_core_fwd_kernel in csrc/dvm_n2p_bwd.hip, n2p_attention_kernel in
csrc/dvm_n2p.hip).  No GPU code here: every function runs on whatever device its tensors live on, so tests/test_attention_rows_cpu.py
uses it on the CPU and tests/test_gpu_attention_rows.py on the card.

Bar of every row of every output (the form of K1's backward in tests/test_gpu_backward_adversarial.py, same K = 64):

    err_row <= max(3 err32_row, K 2^-24 s_row) + ftz_row  [+ 3 fwd_row on the backward run fed the forward's own statistics]

err_row is the 2-norm over the row's channels of got - ref64 (a scalar output is its own row), err32_row the same for the reference's
own fp32 formulation (the torch fp32 ops of models/model.py on the CPU, autograd for the gradients: sa_fp32_formulation,
n2p_fp32_formulation), s_row and ftz_row the 2-norms of the per-channel terms derived below.

SA (one cloud; p (N,16), v (N,64), G = dL/dxr (N,64)).  Reference: E = p p^T, A = softmax_rows(E), c_j = 1e-9 + sum_i A_ij,
Ah = A / c, xr_j = sum_i Ah_ij v_i, stats_i = (m_i = max_j E_ij, 1 / sum_j exp(E_ij - m_i)), cinv_j = 1 / c_j; dv, dp by the closed
form of csrc/dvm_sa_bwd.hip's header (dv_i = sum_j Ah_ij G_j, t_j = G_j . xr_j, dA_ij = (v_i . G_j - t_j) cinv_j, u_i = sum_j A_ij dA_ij,
dE_ij = A_ij (dA_ij - u_i), dp_i = sum_j (dE_ij + dE_ji) p_j); tests/test_attention_rows_cpu.py checks that closed form once against
float64 autograd of models/model.py:113-121.  With fwd = (xr, stats, cinv) of a forward the same closed form is fed those (A =
exp(E - m) il on exact E): "ref(forward's statistics)", whose distance from ref prices the forward alone.

  Derivation of s.  A logit is a sum of 16 products, so fp32 leaves it off by about 2^-24 aE_ij, aE_ij = sum_k |p_ik p_jk|; the fast
  exponential multiplies its argument by log2(e) in fp32, so its relative error grows with |E_ij - m_i|.  Hence the relative error of
  exp(E_ij - m_i) is e_ij = aE_ij + |E_ij - m_i| (in units of 2^-24), and through the row's normalisation a weight moves by
  A_ij (1 + sens_ij),  sens_ij = e_ij + sum_j' A_ij' e_ij'.
    stats_i:  m_i moves by max_j aE_ij (a max is 1-Lipschitz); 1/l_i by il_i (1 + max_j aE_ij + sum_j A_ij e_ij): a shifted m rescales l.
    cinv_j:   c_j moves by sum_i A_ij (1 + sens_ij), so cinv_j by cinv_j (1 + rc_j), rc_j = sum_i Ah_ij (1 + sens_ij).
    xr_j:     each addend Ah_ij v_i moves by Ah_ij (1 + sens_ij) |v_i| and the division by c_j moves the sum by rc_j |xr_j|:
              s = sum_i Ah_ij (1 + sens_ij) (|v_i| + |xr_j|).
    dv_i:     s = sum_j Ah_ij (1 + sens_ij + rc_j) |G_j|  (the division differs from column to column, so rc_j stays inside the sum).
    dp_i:     dAh_ij - t_j is formed from aX_ij = sum_c |G_jc v_ic| and aT_j = sum_c |G_jc xr_jc| before they cancel (v + 100 makes
              them cancel), times cinv_j; u_i sums them over the row: uabs_i = sum_j A_ij (1 + sens_ij) (aX_ij + aT_j) cinv_j.
              |dE|abs_ij = A_ij (1 + sens_ij) ((aX_ij + aT_j) cinv_j + uabs_i),  s = sum_j (|dE|abs_ij + |dE|abs_ji) |p_j|.
  Derivation of ftz.  The device flushes a weight below 2^-126 to 0, float64 keeps it: T = 2^-126 per weight times what multiplies it.
    stats_i:  m: 0;  1/l_i: il_i N T.                           cinv_j:  cinv_j^2 N T.
    xr_j:     T cinv_j (sum_i |v_i| + N |xr_j|)  (the lost addends, and the lost part of c_j; cinv_j is up to 1e9).
    dv_i:     T sum_j cinv_j |G_j|.
    dp_i:     uftz_i = T sum_j (aX_ij + aT_j) cinv_j;  |dE|ftz_ij = T ((aX_ij + aT_j) cinv_j + uabs_i) + A_ij uftz_i;  summed like s.

N2P (one cloud; qkv (N,3C), idx (N,K), 4 heads of D = C/4): e_hj = q_h . (kp_j - kp_i)_h / sqrt(D), a = softmax_j, out_h = sum_j a_hj
(vp_j - vp_i)_h (n2p_ref64: the block n2p_check of tests/test_gpu_backward_adversarial.py differentiates).  ae_hj = sum |q| (|kp_j| +
|kp_i|) / sqrt(D) are a logit's absolute terms, e_hj = ae_hj + |e_hj - m_h|, and a weight moves by aa_hj = a_hj (1 + e_hj + sum_j' a e).
    attn:  s = aa (the relative form), ftz = T per weight.
    out:   s = sum_j aa_hj (|vp_j| + |vp_i|),  ftz = T (sum_j (|vp_j| + |vp_i|) + K)  (the online form also flushes its running sum once
           per step, below T each time).

Largest err / bar per family and output.  "fp32": the fp32 restatement of the kernels' order of operations in
tests/test_attention_rows_cpu.py (exp in place of the fast exponential) over every shape of that file; "gpu": the kernels on the MI355X
over every shape of tests/test_gpu_attention_rows.py.  dv / dp: the backward on float64-exact xr / stats / cinv (plain bar);
dv(fwd) / dp(fwd): on the forward's own (bar + the forward term); (pm): the inference kernel's form.
  sa               xr fp32|gpu        m fp32|gpu       il fp32|gpu     cinv fp32|gpu
  randn          0.0055|0.0067       0.065|0.065       0.025|0.029       0.0097|0.01
  relu           0.0041|0.0038       0.051|0.051        0.02|0.021     0.0075|0.0074
  peaked         0.0049|0.0047       0.056|0.056       0.013|0.013         0.03|0.03
  hub10           0.002|0.0019     0.0093|0.0093     0.0032|0.0045     0.0067|0.0079
  hub25            0.011|0.014     0.0099|0.0099   4.5e-05|8.9e-05      0.007|0.0086
  hub100       1.8e-05|1.8e-05         0.01|0.01               0|0   3.8e-05|3.8e-05
  dup_pairs      0.0063|0.0053       0.065|0.065       0.016|0.017      0.0093|0.012
  dup_all      0.00084|0.00065       0.046|0.046     0.0014|0.0014       0.0076|0.01
  gzero          0.0055|0.0058       0.065|0.065       0.019|0.018       0.0097|0.01
  voffset         0.0038|0.003       0.065|0.065       0.019|0.018       0.0097|0.01
  vscale1e3      0.0055|0.0058       0.065|0.065       0.019|0.018       0.0097|0.01
  vscale1e-3      0.0053|0.006       0.065|0.065       0.019|0.018       0.0097|0.01
  sa          dv(fwd) fp32|gpu  dp(fwd) fp32|gpu       dv fp32|gpu       dp fp32|gpu
  randn           0.006|0.0082   0.00012|0.00012       0.017|0.017   0.00011|0.00013
  relu            0.0029|0.003   0.00024|0.00025       0.011|0.011    0.00012|0.0005
  peaked         0.0017|0.0018   5.6e-06|7.3e-06       0.019|0.019   1.7e-05|1.7e-05
  hub10          0.0011|0.0011   8.7e-06|8.6e-06     0.0013|0.0012   1.2e-05|1.1e-05
  hub25          0.0013|0.0015     3.9e-06|4e-06     0.0015|0.0016   4.5e-06|4.6e-06
  hub100       2.1e-05|2.1e-05   2.6e-07|2.7e-07   2.1e-05|2.1e-05   2.6e-07|2.9e-07
  dup_pairs       0.005|0.0044   0.00015|0.00013       0.011|0.011   0.00016|0.00012
  dup_all      0.00053|0.00045   2.8e-05|2.8e-05     0.0044|0.0053   3.1e-05|3.8e-05
  gzero            0.017|0.015   0.00017|0.00017       0.014|0.014   0.00016|0.00016
  voffset         0.006|0.0061   9.3e-05|9.1e-05       0.014|0.014   9.5e-05|9.2e-05
  vscale1e3       0.006|0.0061   7.4e-05|9.5e-05       0.014|0.014   7.8e-05|8.3e-05
  vscale1e-3      0.006|0.0061    8.8e-05|0.0001       0.014|0.014   7.2e-05|0.00012
  n2p             out fp32|gpu     attn fp32|gpu
  random         0.0027|0.0019     0.0098|0.0063
  random(pm)     0.0045|0.0044               -|-
  hub            0.0026|0.0019     0.0097|0.0062
  hub(pm)        0.0043|0.0041               -|-
  self            0.002|0.0017     0.0097|0.0059
  self(pm)       0.0043|0.0044               -|-
  same           0.0042|0.0053     0.0011|0.0011
  same(pm)         0.015|0.015               -|-
  peaked         0.0024|0.0024     0.0055|0.0042
  peaked(pm)      0.0024|0.002               -|-
  wide           0.0027|0.0018      0.006|0.0033
  wide(pm)        0.0027|0.002               -|-
  tie            0.0024|0.0024      0.0094|0.006
  tie(pm)         0.005|0.0055               -|-
The dp bar is by far the widest: s sums |G_j . v_i|, |t_j| and |u_i| before they cancel and weighs them with 1 + sens (20 to 30 on
randn), so on randn it is about 15 % of |dp_i| for the median row where xr / dv / cinv sit near 1e-4 of the row: a dp row that is
wrong (a lost half of the symmetric term, a lost split, two exchanged channels) fails, a dp row off by a few per cent does not.
"""
import torch

EPS = 2.0 ** -24
K = 64.0            # tests/test_gpu_backward_adversarial.py's constant; this file introduces no other
TINY = 2.0 ** -126
SA_P, SA_C, SA_KB = 16, 64, 128

RATIOS = {}         # (core, family, output) -> largest err / bar seen in this process (reports only; nothing asserts on it)


# --------------------------------------------------------------------------------------------- launch routes (mirrors of the launch code)
def sa_fwd_route(B, N):
    """(S, kchunk, Z) of launch_sa_forward: S = sa_splits(B, N), Z key chunks of kchunk keys."""
    groups = B * ((N + 31) // 32)
    S = 1
    if groups < 400:
        while groups * S < 1024 and S < 8 and (N + 2 * S - 1) // (2 * S) >= 4 * SA_KB:
            S *= 2
    kchunk = ((N + S - 1) // S + SA_KB - 1) // SA_KB * SA_KB
    return S, kchunk, (N + kchunk - 1) // kchunk


def sa_bwd_route(B, N, deterministic=False):
    """(split, tiles per split, ntiles) of dvm_sa_attention_bwd_f32."""
    ot, ntiles = (N + 127) // 128, (N + 31) // 32
    split = 1
    if not deterministic:
        while B * ot * split < 512 and split < 16 and ntiles // (2 * split) >= 4:
            split *= 2
    return split, (ntiles + split - 1) // split, ntiles


# The smallest shapes that select each route; both halves run them and tests/test_attention_rows_cpu.py holds the labels against the
# mirrors above.  SA forward (B, N) -> (S, Z):
SA_FWD_SHAPES = {
    (3, 77): (1, 1),      # one chunk, the last column group partial
    (2, 300): (1, 1),     # one chunk, three staged 128-key blocks
    (1, 1023): (2, 2),    # two chunks of 512: both merge kernels
    (2, 1023): (2, 2),    # S = 2 with B > 1: chunk-major partials of two clouds
    (1, 2045): (4, 4),    # four chunks of 512
    (1, 2100): (4, 4),    # four chunks, kchunk = 640 (525 rounded up to the staged block)
    (1, 4089): (8, 8),    # eight chunks of 512
    (1, 4100): (8, 7),    # kchunk = 640: Z = 7 chunks in a workspace sized for S = 8
    (8, 2048): (1, 1),    # 512 column groups (>= 400): no split at the training shape
}
# SA backward (B, N) -> split of the inner loop (non-deterministic mode)
SA_BWD_SHAPES = {
    (1, 224): 1,          # 7 inner tiles: the largest N that is not split
    (1, 255): 2,          # 8 inner tiles (the ragged last one) already split in two
    (1, 256): 2,
    (1, 512): 4,
    (1, 1024): 8,
    (1, 1030): 8,         # 33 tiles, 5 per split: the last split is empty (t0 = 35 > 33)
    (1, 2048): 16,
    (8, 2048): 4,         # the training shape
}
SA_DET_N = [256, 1030, 2048]                  # under set_deterministic(True): split = 1, two calls bit for bit
SA_TAIL_N = [1, 2, 31, 32, 33, 127, 129]      # with B = 3: the last cloud's last row is a tail row
SA_FLAT_N = [1, 2, 32, 128, 256, 1024, 2048]  # the exact planting at B = 1; 1024 and 2048 go through Z = 2 and Z = 4
N2P_CK = [(C, Kn) for C in (64, 128) for Kn in (1, 3, 40, 64)]   # K = 3: below the 4 slots per step at C = 64, odd for the 2 at C = 128
N2P_BN = [(1, 1), (2, 5), (3, 1030)]          # N % 4 != 0 with several clouds: the clamped tail waves


# --------------------------------------------------------------------------------------------- rows
def _rownorm(x):
    return x.abs() if x.dim() == 1 else x.norm(dim=-1)


def check_rows(got, ref, ref32, s, ftz, what, key=None, extra=None):
    """Every row of `got` against the bar; returns the largest err / bar.  key = (core, family, output) files it under RATIOS."""
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), "%s: non-finite values" % what
    ref = ref.to(got.device)
    err = _rownorm(got.double() - ref)
    err32 = _rownorm(ref32.double().to(got.device) - ref)
    bar = torch.maximum(3.0 * err32, K * EPS * _rownorm(s.to(got.device))) + _rownorm(ftz.to(got.device))
    if extra is not None:
        bar = bar + 3.0 * extra.to(got.device)
    ratio = (err / torch.where(bar > 0, bar, torch.full_like(bar, 1e-300))).reshape(-1)
    k = int(ratio.argmax())
    if key is not None and key[1] is not None:
        RATIOS[key] = max(RATIOS.get(key, 0.0), float(ratio[k]))
    assert bool((err <= bar).all()), "%s row %d of %d: err %.3e bar %.3e (3 err32 %.3e); %d rows over" % (
        what, k, ratio.numel(), err.reshape(-1)[k], bar.reshape(-1)[k], 3 * err32.reshape(-1)[k], int((err > bar).sum()))
    return float(ratio[k])


def report(core):
    """The RATIOS of one core as text: one line per family, outputs in columns."""
    fams, outs = [], []
    for (c, f, o) in RATIOS:
        if c == core:
            fams += [f] if f not in fams else []
            outs += [o] if o not in outs else []
    lines = ["%-12s" % core + " ".join("%10s" % o for o in outs)]
    for f in fams:
        lines.append("%-12s" % f + " ".join("%10s" % ("%.2g" % RATIOS[(core, f, o)] if (core, f, o) in RATIOS else "-") for o in outs))
    return "\n".join(lines)


# --------------------------------------------------------------------------------------------- SA
def sa_ref64(p, v, G=None, fwd=None):
    """One cloud in float64 on the tensors' device -> dict: xr, stats, cinv [, dv, dp], their s_* and f_* (ftz) terms per channel.
    fwd = (xr, stats, cinv): the backward's closed form fed those instead of the exact ones (dv, dp only; no terms)."""
    p, v = p.double(), v.double()
    N = p.shape[0]
    E = p @ p.T
    m = E.max(1)[0]
    X = torch.exp(E - m[:, None])
    il = 1.0 / X.sum(1)
    A = X * il[:, None]
    del X
    cinv = 1.0 / (1e-9 + A.sum(0))
    xr = (A * cinv[None]).T @ v
    R = {"xr": xr, "stats": torch.stack([m, il], 1), "cinv": cinv}
    if fwd is not None:
        G = G.double()
        xr_b, st_b, cinv_b = (x.double() for x in fwd)
        A_b = torch.exp(E - st_b[:, :1]) * st_b[:, 1:]
        R["dv"] = (A_b * cinv_b[None]) @ G
        dA = (v @ G.T - (G * xr_b).sum(1)[None]) * cinv_b[None]
        dE = A_b * (dA - (A_b * dA).sum(1, keepdim=True))
        R["dp"] = (dE + dE.T) @ p
        return R
    ap, av = p.abs(), v.abs()
    aE = ap @ ap.T
    e = aE + (E - m[:, None]).abs()
    ae_row = (A * e).sum(1)
    sens1 = 1.0 + e + ae_row[:, None]                     # 1 + sens_ij
    del e
    W = A * cinv[None] * sens1                            # Ah_ij (1 + sens_ij)
    rc = W.sum(0)
    maxaE = aE.max(1)[0]
    del aE
    R["s_xr"] = W.T @ av + rc[:, None] * xr.abs()
    R["s_stats"] = torch.stack([maxaE, il * (1.0 + maxaE + ae_row)], 1)
    R["s_cinv"] = cinv * (1.0 + rc)
    R["f_xr"] = TINY * cinv[:, None] * (av.sum(0)[None] + N * xr.abs())
    R["f_stats"] = torch.stack([torch.zeros_like(il), il * N * TINY], 1)
    R["f_cinv"] = cinv * cinv * N * TINY
    if G is None:
        return R
    G = G.double()
    aG = G.abs()
    R["dv"] = (A * cinv[None]) @ G
    dA = (v @ G.T - (G * xr).sum(1)[None]) * cinv[None]
    dE = A * (dA - (A * dA).sum(1, keepdim=True))
    del dA
    R["dp"] = (dE + dE.T) @ p
    del dE
    R["s_dv"] = (W + A * cinv[None] * rc[None]) @ aG
    R["f_dv"] = (TINY * (cinv[:, None] * aG).sum(0))[None].expand(N, -1)
    del W
    aXT = (av @ aG.T + (aG * xr.abs()).sum(1)[None]) * cinv[None]      # (aX_ij + aT_j) cinv_j
    A1 = A * sens1
    del sens1
    uabs = (A1 * aXT).sum(1)
    dEabs = A1 * (aXT + uabs[:, None])
    del A1
    R["s_dp"] = (dEabs + dEabs.T) @ ap
    del dEabs
    dEf = TINY * (aXT + uabs[:, None]) + A * (TINY * aXT.sum(1))[:, None]
    R["f_dp"] = (dEf + dEf.T) @ ap
    return R


def sa_autograd64(p, v, G):
    """models/model.py:113-121 point-major in float64 under autograd, one cloud -> xr, dv, dp."""
    p64, v64 = p.double().clone().requires_grad_(True), v.double().clone().requires_grad_(True)
    att = torch.softmax(p64 @ p64.T, dim=-1)
    att = att / (1e-9 + att.sum(dim=0, keepdim=True))
    xr = att.T @ v64
    (xr * G.double()).sum().backward()
    return xr.detach(), v64.grad, p64.grad


def sa_fp32_formulation(p, v, G=None):
    """The reference's own formulation in fp32 on the CPU (models/model.py:113-121, autograd for the gradients), one cloud ->
    dict xr, stats, cinv [, dv, dp].  It measures the reference, never a kernel."""
    p32, v32 = p.detach().float().cpu().clone().requires_grad_(True), v.detach().float().cpu().clone().requires_grad_(True)
    energy = p32 @ p32.T
    att = torch.softmax(energy, dim=-1)
    col = 1e-9 + att.sum(dim=0, keepdim=True)
    xr = (att / col).T @ v32
    with torch.no_grad():
        m = energy.max(1)[0]
        R = {"xr": xr.detach(), "stats": torch.stack([m, 1.0 / torch.exp(energy - m[:, None]).sum(1)], 1), "cinv": (1.0 / col)[0]}
    if G is not None:
        (xr * G.detach().float().cpu()).sum().backward()
        R["dv"], R["dp"] = v32.grad, p32.grad
    return R


SA_FAMILIES = ["randn", "relu", "peaked", "hub10", "hub25", "hub100", "dup_pairs", "dup_all", "gzero", "voffset", "vscale1e3",
               "vscale1e-3"]


def sa_inputs(family, B, N, seed):
    """-> p (B,N,16), v (B,N,64), G (B,N,64) on the CPU in float32."""
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(B, N, SA_P, generator=g) * 0.7
    v = torch.randn(B, N, SA_C, generator=g)
    G = torch.randn(B, N, SA_C, generator=g)
    if family == "relu":
        p, v = torch.relu(p), torch.relu(v)
    elif family == "peaked":                      # rows one-hot on the diagonal, off-diagonal weights underflow
        p = p * 3.0
    elif family.startswith("hub"):                # every row attends to column h with a logit gap of about delta
        delta = float(family[3:])
        s = delta ** 0.5
        p = torch.cat([torch.full((B, N, 1), s), 0.1 * torch.randn(B, N, SA_P - 1, generator=g)], 2)
        p[:, N // 3] = 0.0
        p[:, N // 3, 0] = s + (delta + 0.5) / s   # E_ih - E_ij = delta + 0.5 - r_i . r_j, |r|^2 ~ 0.15
    elif family == "dup_pairs":                   # pairs of identical points
        p[:, 1::2], v[:, 1::2] = p[:, 0:N - 1:2].clone(), v[:, 0:N - 1:2].clone()
    elif family == "dup_all":                     # all points identical and non-zero
        p = p[:, :1].expand(B, N, SA_P).contiguous()
    elif family == "gzero":
        G[:, ::3] = 0.0
    elif family == "voffset":                     # G_j . v_i - t_j cancels
        v = v + 100.0
    elif family == "vscale1e3":
        v = v * 1e3
    elif family == "vscale1e-3":
        v = v * 1e-3
    else:
        assert family == "randn", family
    return p.contiguous(), v.contiguous(), G.contiguous()


def sa_flat_inputs(B, N, seed):
    """The exact planting: p = 0, v and G small integers -> (p, v, G, xr, stats, cinv, dv) with the exact fp32 answers (dp = 0)."""
    g = torch.Generator().manual_seed(seed)
    v = torch.randint(-2, 3, (B, N, SA_C), generator=g).float()
    G = torch.randint(-2, 3, (B, N, SA_C), generator=g).float()
    xr = (v.double().sum(1, keepdim=True) / N).float().expand(B, N, SA_C)
    dv = (G.double().sum(1, keepdim=True) / N).float().expand(B, N, SA_C)
    stats = torch.tensor([0.0, 1.0 / N]).expand(B, N, 2)
    return torch.zeros(B, N, SA_P), v, G, xr, stats, torch.ones(B, N), dv


def sa_check_forward(got, R, R32, family, what):
    """got = (xr, stats, cinv) of one cloud (N, ...) on any device; every row of the three (the two columns of stats apart) against
    its bar.  R = sa_ref64(p, v[, G]), R32 = sa_fp32_formulation(p, v[, G])."""
    for name, x in zip(("xr", "stats", "cinv"), got):
        if name == "stats":
            for c, nm in ((0, "m"), (1, "il")):
                check_rows(x[:, c], R["stats"][:, c], R32["stats"][:, c], R["s_stats"][:, c], R["f_stats"][:, c], "%s %s" % (what, nm),
                           ("sa", family, nm))
        else:
            check_rows(x, R[name], R32[name], R["s_" + name], R["f_" + name], "%s %s" % (what, name), ("sa", family, name))


def sa_check_backward(dv, dp, R, R32, family, what, fwd_ref=None):
    """dv, dp of one cloud against the bars of R (from sa_ref64 with G).  fwd_ref = sa_ref64(..., fwd=...) of the forward whose
    statistics the backward was fed: adds 3 |ref(forward's statistics) - ref| per row."""
    for name, x in (("dv", dv), ("dp", dp)):
        extra = None if fwd_ref is None else (fwd_ref[name] - R[name]).norm(dim=1)
        check_rows(x, R[name], R32[name], R["s_" + name], R["f_" + name], "%s %s" % (what, name),
                   ("sa", family, name + ("" if fwd_ref is None else "(fwd)")), extra)


# --------------------------------------------------------------------------------------------- N2P
def n2p_ref64(x, idx, H=4):
    """One cloud: x (1,N,3C) float64 (may require grad), idx (1,N,K) -> dict q, kp, vp, kj, vj (1,N,K,C), qh (1,N,1,H,D),
    e, a (1,N,K,H), out (1,N,C): models/model.py:339-350 on projected rows."""
    _, N, C3 = x.shape
    C, Kn = C3 // 3, idx.shape[-1]
    Dh = C // H
    gi = idx.long().reshape(1, N * Kn, 1).expand(-1, -1, C)
    q, kp, vp = x[..., :C], x[..., C:2 * C], x[..., 2 * C:]
    kj = torch.gather(kp, 1, gi).view(1, N, Kn, C)
    vj = torch.gather(vp, 1, gi).view(1, N, Kn, C)
    kd = (kj - kp[:, :, None]).view(1, N, Kn, H, Dh)
    vd = (vj - vp[:, :, None]).view(1, N, Kn, H, Dh)
    qh = q.view(1, N, 1, H, Dh)
    e = (qh * kd).sum(-1) / Dh ** 0.5
    a = torch.softmax(e, dim=2)
    out = (a.unsqueeze(-1) * vd).sum(2).reshape(1, N, C)
    return {"q": q, "kp": kp, "vp": vp, "kj": kj, "vj": vj, "qh": qh, "e": e, "a": a, "out": out, "gi": gi}


def n2p_terms(r, H=4):
    """s and ftz of attn (N, K H) and out (N, C) from n2p_ref64's dict (no grad)."""
    with torch.no_grad():
        _, N, Kn, C = r["kj"].shape
        Dh = C // H
        a, e = r["a"], r["e"]
        ae = (r["qh"].abs() * (r["kj"].abs() + r["kp"].abs()[:, :, None]).view(1, N, Kn, H, Dh)).sum(-1) / Dh ** 0.5
        ee = ae + (e - e.max(2, keepdim=True)[0]).abs()
        aa = a * (1.0 + ee + (a * ee).sum(2, keepdim=True))
        av = (r["vj"].abs() + r["vp"].abs()[:, :, None]).view(1, N, Kn, H, Dh)
        s_out = (aa.unsqueeze(-1) * av).sum(2).reshape(N, C)
        f_out = TINY * (av.sum(2).reshape(N, C) + Kn)
        return {"s_attn": aa.reshape(N, Kn * H), "f_attn": torch.full_like(aa, TINY).reshape(N, Kn * H), "s_out": s_out, "f_out": f_out}


def n2p_fp32_formulation(qkv, idx, H=4):
    """models/model.py:339-350 in fp32 on the CPU, one cloud: qkv (N,3C), idx (N,K) -> attn (N, K H), out (N, C)."""
    with torch.no_grad():
        r = n2p_ref64(qkv.detach().float().cpu()[None], idx.cpu()[None], H)
        return r["a"].reshape(qkv.shape[0], -1), r["out"][0]


N2P_FAMILIES = ["random", "hub", "self", "same", "peaked", "wide", "tie"]


def n2p_family_inputs(base_inputs, B, N, C, Kn, family, seed):
    """`base_inputs` is n2p_inputs of tests/test_gpu_backward_adversarial.py (random / hub / self / same); this adds peaked (q x 8),
    wide (q x 30: weights underflow to exactly 0) and tie (two listed neighbours with identical rows).  -> qkv, idx; every index
    is a valid row."""
    if family in ("random", "hub", "self", "same"):
        qkv, idx, _ = base_inputs(B, N, C, Kn, family, seed)
        if family == "hub":                  # n2p_inputs lists point 5; keep it a valid row in the small clouds
            idx[:, :, 0] = min(5, N - 1)
    else:
        qkv, idx, _ = base_inputs(B, N, C, Kn, "random", seed)
        if family == "peaked":
            qkv[..., :C] *= 8.0
        elif family == "wide":
            qkv[..., :C] *= 30.0
        else:
            assert family == "tie", family
            j1, j2 = N // 3, N - 1
            qkv[:, j2] = qkv[:, j1]
            idx[:, :, 0], idx[:, :, -1] = j1, j2
    assert int(idx.min()) >= 0 and int(idx.max()) < N
    return qkv.contiguous(), idx.contiguous()


def n2p_check_forward(out, attn, qkv, idx, family, what, H=4):
    """out (N,C) and, when given, attn (N,K,H) of one cloud against float64 on out's device, every row."""
    with torch.no_grad():
        r = n2p_ref64(qkv.double().to(out.device)[None], idx.to(out.device)[None], H)
        t = n2p_terms(r, H)
        a32, o32 = n2p_fp32_formulation(qkv, idx, H)
        check_rows(out, r["out"][0], o32, t["s_out"], t["f_out"], what + " out", ("n2p", family, "out"))
        if attn is not None:
            N = out.shape[0]
            check_rows(attn.reshape(N, -1), r["a"].reshape(N, -1), a32, t["s_attn"], t["f_attn"], what + " attn", ("n2p", family, "attn"))


# --------------------------------------------------------------------------------------------- cases: the same driver for the fp32 restatement and the kernels
def sa_run_case(fwd, bwd, family, B, N, seed, device="cpu", backward=True, record=True):
    """fwd(p, v) -> xr, stats, cinv and bwd(p, v, xr, stats, cinv, G) -> dp, dv on batched float32 tensors on `device`.  Every row of
    xr / stats / cinv; then every row of dv / dp twice: on the forward's own xr / stats / cinv (bar + 3 |ref(forward's statistics)
    - ref|) and on the float64-exact ones rounded to fp32 (the exact-forward rerun, plain bar)."""
    p, v, G = sa_inputs(family, B, N, seed)
    fam = family if record else None
    pd, vd, Gd = p.to(device), v.to(device), G.to(device)
    xr, st, ci = fwd(pd, vd)
    if backward:
        dp, dv = bwd(pd, vd, xr, st, ci, Gd)
    exact = []
    for e in range(B):
        what = "%s (%d,%d) cloud %d" % (family, B, N, e)
        R = sa_ref64(pd[e], vd[e], Gd[e] if backward else None)
        R32 = sa_fp32_formulation(p[e], v[e], G[e] if backward else None)
        sa_check_forward((xr[e], st[e], ci[e]), R, R32, fam, what)
        if backward:
            Rf = sa_ref64(pd[e], vd[e], Gd[e], fwd=(xr[e], st[e], ci[e]))
            sa_check_backward(dv[e], dp[e], R, R32, fam, what + " own forward", fwd_ref=Rf)
            exact.append((R, R32))
    if backward:
        ex = [torch.stack([R[k].float() for R, _ in exact]).contiguous() for k in ("xr", "stats", "cinv")]
        dp, dv = bwd(pd, vd, ex[0], ex[1], ex[2], Gd)
        for e, (R, R32) in enumerate(exact):
            sa_check_backward(dv[e], dp[e], R, R32, fam, "%s (%d,%d) cloud %d exact forward" % (family, B, N, e))


def sa_flat_case(fwd, bwd, B, N, device="cpu"):
    """p = 0: every output bit for bit (dp: exactly 0)."""
    p, v, G, xr_x, st_x, ci_x, dv_x = (t.to(device) for t in sa_flat_inputs(B, N, seed=N + B))
    xr, st, ci = fwd(p, v)
    assert torch.equal(xr, xr_x), "flat (%d,%d): xr is not the mean of v bit for bit; %d elements differ" % (B, N, int((xr != xr_x).sum()))
    assert torch.equal(st, st_x), "flat (%d,%d): stats != (0, 1/N); %d differ" % (B, N, int((st != st_x).sum()))
    assert torch.equal(ci, ci_x), "flat (%d,%d): cinv != 1; %d differ" % (B, N, int((ci != ci_x).sum()))
    dp, dv = bwd(p, v, xr, st, ci, G)
    assert torch.equal(dv, dv_x), "flat (%d,%d): dv != sum(G) / N bit for bit; %d elements differ" % (B, N, int((dv != dv_x).sum()))
    assert bool((dp == 0).all()), "flat (%d,%d): dp != 0 at %d elements" % (B, N, int((dp != 0).sum()))


def n2p_run_case(base_inputs, core, pm, family, B, N, C, Kn, seed, device="cpu", record=True):
    """core(qkv, idx) -> out, attn (the training forward) and pm(q, kp, vp, idx) -> out (the inference kernel's form), batched."""
    qkv, idx = n2p_family_inputs(base_inputs, B, N, C, Kn, family, seed)
    fam = family if record else None
    qd, ix = qkv.to(device), idx.to(device)
    out, attn = core(qd, ix)
    out2 = pm(qd[..., :C].contiguous(), qd[..., C:2 * C].contiguous(), qd[..., 2 * C:].contiguous(), ix)
    for e in range(B):
        what = "%s C %d K %d (%d,%d) cloud %d" % (family, C, Kn, B, N, e)
        n2p_check_forward(out[e], attn[e], qkv[e], idx[e], fam, what + " core")
        n2p_check_forward(out2[e], None, qkv[e], idx[e], None if fam is None else fam + "(pm)", what + " pm")


def n2p_exact_case(core, pm, kind, B, N, C, seed, device="cpu"):
    """kind 'k1': K = 1, any finite inputs: attn == 1, out == vp_j - vp_i.  'q0' (q = 0) and 'same' (all slots equal), K = 64,
    integer vp: attn == 1/64, out the exact mean.  'offset': every head of kp holds (2^23 + a, c, -2^23 + b, ...) with a + b + c = 16 in
    every row (a integer, b and c half-integers) and q = 1 on those three channels, 0 elsewhere: the differences kp_j - kp_i are exact
    and sum to 0, so every logit is 0 and attn == 1/64 -- but only if the difference is taken BEFORE the product, as the reference
    does: q . kp_j alone rounds at 2^23 (the one check that sees `- kp_i` left out, which a softmax otherwise hides as a common
    shift).  Bit for bit in both forwards."""
    g = torch.Generator().manual_seed(seed)
    Kn = 1 if kind == "k1" else 64
    qkv = torch.randn(B, N, 3 * C, generator=g)
    idx = torch.randint(0, N, (B, N, Kn), generator=g, dtype=torch.int32)
    if kind != "k1":
        qkv[..., 2 * C:] = torch.randint(-4, 5, (B, N, C), generator=g).float()
        if kind == "q0":
            qkv[..., :C] = 0.0
        elif kind == "same":
            idx[:] = idx[:, :, :1]
        else:
            assert kind == "offset", kind
            D = C // 4
            a = torch.randint(0, 8, (B, N, 4), generator=g).float()
            c = torch.randint(0, 4, (B, N, 4), generator=g).float() + 0.5
            q, kp = torch.zeros(B, N, 4, D), torch.randint(-4, 5, (B, N, 4, D), generator=g).float()
            q[..., :3] = 1.0
            kp[..., 0], kp[..., 1], kp[..., 2] = 2.0 ** 23 + a, c, -2.0 ** 23 + (16.0 - a - c)
            qkv[..., :C], qkv[..., C:2 * C] = q.reshape(B, N, C), kp.reshape(B, N, C)
    vp = qkv[..., 2 * C:]
    vj = torch.gather(vp.double(), 1, idx.long().reshape(B, N * Kn, 1).expand(-1, -1, C)).view(B, N, Kn, C)
    want = (vj - vp.double()[:, :, None]).mean(2).float() if kind != "k1" else vj[:, :, 0].float() - vp
    qd, ix = qkv.to(device), idx.to(device)
    out, attn = core(qd, ix)
    out2 = pm(qd[..., :C].contiguous(), qd[..., C:2 * C].contiguous(), qd[..., 2 * C:].contiguous(), ix)
    what = "%s C %d (%d,%d)" % (kind, C, B, N)
    assert bool((attn == 1.0 / Kn).all()), "%s: attn != 1/%d at %d entries" % (what, Kn, int((attn != 1.0 / Kn).sum()))
    assert torch.equal(out, want.to(device)), "%s core: out differs at %d elements" % (what, int((out != want.to(device)).sum()))
    assert torch.equal(out2, want.to(device)), "%s pm: out differs at %d elements" % (what, int((out2 != want.to(device)).sum()))
