"""The case table of the forward GEMM's tile-configuration tests (csrc/dvm_gemm.hip::linear_mfma_kernel), shared by
tests/test_linear_cfg_cases_cpu.py (is the table sufficient?) and tests/test_gpu_linear_cfgs.py (does every configuration give the
oracle's bits?), with a restatement in Python of the route predicates of launch_linear_impl / launch_cfg / pick_cfg: what a call
will launch is computed here and compared with what dvm_linear_last_launch reports.  numpy only: importable without a GPU."""
import numpy as np

GK = 32                                         # k-step of the kernel
GEMM_MAX_KB = 24

# table index -> workgroup tile (rows of the output, columns of the output)
PM_TILE = {0: (128, 32), 1: (64, 64), 2: (64, 128), 3: (128, 128), 4: (64, 64), 5: (128, 64), 6: (64, 128), 7: (128, 128)}
CM_TILE = {0: (32, 128), 1: (64, 64), 2: (128, 64), 3: (128, 128)}            # rows = output channels, columns = points
TWIN = {4: 1, 5: 1, 6: 2, 7: 3}                 # register-staged entry that runs where LDS-DMA staging does not apply
PM_CFGS, CM_CFGS = tuple(range(8)), tuple(range(4))
# the twelve kernel instantiations as (channel_major, table index, LDS-DMA staging)
INSTANTIATIONS = frozenset([(0, c, 0) for c in range(4)] + [(0, c, 1) for c in range(4, 8)] + [(1, c, 0) for c in range(4)])


def gemm_kblocks(K):
    """K-block edges [0, .., K] of dvm_gemm.hip::gemm_kblocks (== oracle's dvo_gemm_kblocks while K <= 384 * 22)."""
    starts, k = [0], 0
    while K - k > 768 and len(starts) - 1 < GEMM_MAX_KB - 2:
        k += 384
        starts.append(k)
    if K - k > 384 and len(starts) - 1 < GEMM_MAX_KB - 1:
        k += (K - k + 1) // 2
        starts.append(k)
    starts.append(K)
    return starts


def kvec(K, aligned=True):
    """16-byte operand loads along K: every block edge a multiple of 4, operand bases on the 16-byte grid"""
    return int(aligned and all(s % 4 == 0 for s in gemm_kblocks(K)))


def dma_ok(K, prefix=False, aligned=True):
    """LDS-DMA staging applies (point-major only): vector loads, no row prefix, every block edge a multiple of the k-step"""
    return bool(kvec(K, aligned) and not prefix and all(s % GK == 0 for s in gemm_kblocks(K)))


def yvec(ldy, aligned=True):
    """16-byte accesses in the epilogue: output rows of a multiple of 4 floats (point-major Co, channel-major N), bases aligned"""
    return int(aligned and ldy % 4 == 0)


def default_cfg(channel_major, K, Co):
    """pick_cfg without DVM_LINEAR_CFG"""
    if Co <= 32:
        return 0
    if channel_major:
        return 1
    return 6 if K >= 768 else 4


def launched(c, channel_major, K, Co, prefix=False, aligned=True):
    """(table index, LDS-DMA staging) under DVM_LINEAR_CFG=c (None: unset)"""
    n = 4 if channel_major else 8
    cfg = c if c is not None and 0 <= c < n else default_cfg(channel_major, K, Co)
    if channel_major:
        return cfg, 0
    if cfg >= 4 and not dma_ok(K, prefix, aligned):
        return TWIN[cfg], 0
    return cfg, int(cfg >= 4)


def tiles(channel_major, idx, rows, cols):
    """(row tiles, column tiles) of table entry idx: point-major rows = B * N, cols = Co; channel-major rows = Co, cols = N"""
    bm, bn = (CM_TILE if channel_major else PM_TILE)[idx]
    return (rows + bm - 1) // bm, (cols + bn - 1) // bn


def expect(c, channel_major, rows_pm, K, Co, N=None, prefix=False, aligned=True, y_aligned=True):
    """The eight ints dvm_linear_last_launch must report for a call under DVM_LINEAR_CFG=c.  Point-major: rows_pm = B * N;
    channel-major: N points per batch element."""
    idx, dma = launched(c, channel_major, K, Co, prefix, aligned)
    if channel_major:
        ti, tj = tiles(1, idx, Co, N)
        yv = yvec(N, y_aligned)
    else:
        ti, tj = tiles(0, idx, rows_pm, Co)
        yv = yvec(Co, y_aligned)
    return [int(channel_major), idx, dma, len(gemm_kblocks(K)) - 1, kvec(K, aligned), yv, ti, tj]


# ----------------------------------------------------------------------------------------------------------------- the table
# Each dimension list is the smallest that reaches an edge of a 128 x 128 tile and of the K rules.
PM_M = (1, 127, 129, 256, 300)        # 1: every staged row clamped; 127 / 129 either side of a 128-row tile; 256 with Co = 512: a tile
#                                       count divisible by 8 at every tile size (the XCD remap); 300: two full tiles and a ragged one
PM_K = (6, 100, 384, 400, 768, 772, 1152, 1156)
#   6 < a k-step, no multiple of 4 | 100 ragged last k-step, kvec 1 | 384 one DMA block | 400 = 200 + 200: kvec 1, DMA refused |
#   768 two DMA blocks | 772 = 384 + 194 + 194: kvec 0 | 1152 three DMA blocks | 1156 = 384 + 384 + 194 + 194: kvec 0, four blocks
PM_CO = (7, 64, 130, 132, 384, 512)   # 7, 130: yvec 0; 132: a multiple of 4, ragged past 128 (vector stores in a partial tile)

PM_CASES = [  # (M, K, Co)
    (1, 6, 7), (127, 6, 384), (127, 100, 64), (300, 100, 130),
    (129, 384, 130), (256, 384, 512), (1, 384, 132),
    (300, 400, 132), (256, 400, 512),
    (127, 768, 7), (256, 768, 512), (129, 772, 64),
    (300, 1152, 384), (1, 1152, 130), (256, 1152, 512),
    (129, 1156, 132), (256, 1156, 512), (300, 1156, 7)]
PM_EPILOGUES = ("none", "full")        # full: bias + residual + BatchNorm affine + LeakyReLU(0.2)

CM_B = 2
# N = 256, Co = 512 and K = 1152 are not among the edge values (1, 77, 127, 129, 260 | 16, 64, 130, 192 | 64, 400, 768, 1156): they are
# what an exact last row / column tile and a tile count divisible by 8 need at 128 x 128, and what three K-blocks need (1156 has
# four); test_linear_cfg_cases_cpu.py asserts these conditions
CM_N = (1, 77, 127, 129, 260, 256)    # the first four: no multiples of 4 (qvec 0, yvec 0)
CM_K = (64, 400, 768, 1156, 1152)
CM_CO = (16, 64, 130, 192, 512)
CM_CASES = [  # (N, K, Co), B = CM_B; epilogue: bias + BatchNorm affine
    (1, 64, 16), (77, 400, 64), (127, 768, 130), (129, 1156, 192), (260, 64, 130), (260, 1156, 64), (129, 400, 16),
    (77, 768, 192), (256, 64, 512), (127, 1152, 64)]

PREFIX_CASES = [(2, 300, 512, 256, 128), (1, 77, 8, 56, 16), (3, 64, 384, 128, 40), (2, 129, 40, 216, 132)]   # (B, N, Cg, Cx, Co)
SCALED_PM = (3, 129, 100, 132)         # (B, N, K, Co)
SCALED_CM = (2, 77, 400, 130)
SCALE = 0.1

GUARD_CASES = [(129, 1156, 132), (300, 1152, 384)]   # Y-parked block totals (the twin runs) / register totals (DMA runs)
GUARD_OFFSETS = {67: 0, 64: 1}         # floats in front of `out` -> the yvec the read-back must report
GUARD_PAD = 67
SENTINEL = 12345.0
OFFGRID_CASE = (129, 384, 130)         # x and w as views 1 float into their buffers


def expected_triples(c):
    """(channel_major, index, dma) of everything the child process with DVM_LINEAR_CFG=c launches"""
    s = set()
    for M, K, Co in PM_CASES + GUARD_CASES:
        s.add(tuple(expect(c, 0, M, K, Co)[:3]))
    for N, K, Co in CM_CASES + [SCALED_CM[1:]]:
        s.add(tuple(expect(c, 1, None, K, Co, N=N)[:3]))
    for B, N, Cg, Cx, Co in PREFIX_CASES:
        e = expect(c, 0, B * N, Cg + Cx, Co, prefix=True)
        assert e[2] == 0                              # every prefix call is a non-DMA launch
        s.add(tuple(e[:3]))
    B, N, K, Co = SCALED_PM
    s.add(tuple(expect(c, 0, B * N, K, Co)[:3]))
    M, K, Co = OFFGRID_CASE
    e = expect(c, 0, M, K, Co, aligned=False)
    assert e[2] == 0 and e[4] == 0 and expect(c, 0, M, K, Co)[2] == int(c >= 4)
    s.add(tuple(e[:3]))
    return s


# ----------------------------------------------------------------------------------------------------------------- the inputs
def _rng(*key):
    return np.random.default_rng(list(key))


def pm_inputs(M, K, Co, epilogue):
    g = _rng(1, M, K, Co, PM_EPILOGUES.index(epilogue))
    d = {"x": (2 * g.standard_normal((M, K))).astype(np.float32), "w": (g.standard_normal((Co, K)) / K ** 0.5).astype(np.float32),
         "bias": None, "res": None, "alpha": None, "beta": None, "slope": 1.0}
    if epilogue == "full":
        d.update(bias=(0.1 * g.standard_normal(Co)).astype(np.float32), res=g.standard_normal((M, Co)).astype(np.float32),
                 alpha=(1 + 0.2 * g.standard_normal(Co)).astype(np.float32), beta=(0.3 * g.standard_normal(Co)).astype(np.float32),
                 slope=0.2)
    return d


def cm_inputs(N, K, Co):
    g = _rng(2, N, K, Co)
    return {"x": g.standard_normal((CM_B, K, N)).astype(np.float32), "w": (g.standard_normal((Co, K)) / K ** 0.5).astype(np.float32),
            "bias": (0.1 * g.standard_normal(Co)).astype(np.float32), "alpha": (1 + 0.2 * g.standard_normal(Co)).astype(np.float32),
            "beta": (0.3 * g.standard_normal(Co)).astype(np.float32)}


def prefix_inputs(B, N, Cg, Cx, Co):
    g = _rng(3, B, N, Cg, Cx, Co)
    return {"g": g.standard_normal((B, Cg)).astype(np.float32), "x": g.standard_normal((B, N, Cx)).astype(np.float32),
            "w": (g.standard_normal((Co, Cg + Cx)) / 20).astype(np.float32),
            "alpha": (1 + 0.1 * g.standard_normal(Co)).astype(np.float32), "beta": (0.1 * g.standard_normal(Co)).astype(np.float32)}


def scaled_inputs(channel_major, B, N, K, Co):
    g = _rng(4, int(channel_major), B, N, K, Co)
    return {"x": g.standard_normal((B, K, N) if channel_major else (B, N, K)).astype(np.float32),
            "w": g.standard_normal((Co, K)).astype(np.float32), "bias": g.standard_normal(Co).astype(np.float32),
            "r": g.standard_normal((B, Co, N) if channel_major else (B, N, Co)).astype(np.float32)}


# ----------------------------------------------------------------------------------------------------------------- the references
def references(linear):
    """name -> expected output, every one made by `linear` = oracle.linear (point-major x (M,K), w (Co,K) -> (M,Co)) on explicit
    operands: channel-major per batch element on the transposed slice, the prefix on the concatenation it stands for, the scaled
    residual as plain * s + r in float32 (one multiply, one add)."""
    out = {}
    for M, K, Co in PM_CASES:
        for ep in PM_EPILOGUES:
            d = pm_inputs(M, K, Co, ep)
            out["pm_%d_%d_%d_%s" % (M, K, Co, ep)] = linear(d["x"], d["w"], d["bias"], d["res"], d["alpha"], d["beta"], d["slope"])
    for N, K, Co in CM_CASES:
        d = cm_inputs(N, K, Co)
        out["cm_%d_%d_%d" % (N, K, Co)] = np.stack([linear(np.ascontiguousarray(d["x"][b].T), d["w"], d["bias"], None, d["alpha"],
                                                           d["beta"], 1.0).T for b in range(CM_B)])
    for B, N, Cg, Cx, Co in PREFIX_CASES:
        d = prefix_inputs(B, N, Cg, Cx, Co)
        cat = np.concatenate([np.broadcast_to(d["g"][:, None, :], (B, N, Cg)), d["x"]], -1).reshape(B * N, Cg + Cx)
        out["prefix_%d_%d_%d_%d_%d" % (B, N, Cg, Cx, Co)] = linear(cat, d["w"], None, None, d["alpha"], d["beta"], 0.2).reshape(B, N, Co)
    for cm, (B, N, K, Co) in ((0, SCALED_PM), (1, SCALED_CM)):
        d = scaled_inputs(cm, B, N, K, Co)
        if cm:
            plain = np.stack([linear(np.ascontiguousarray(d["x"][b].T), d["w"], d["bias"]).T for b in range(B)])
        else:
            plain = linear(d["x"].reshape(B * N, K), d["w"], d["bias"]).reshape(B, N, Co)
        want = plain * np.float32(SCALE) + d["r"]
        assert plain.dtype == np.float32 and want.dtype == np.float32
        out["scaled_%d" % cm] = want
    return out
