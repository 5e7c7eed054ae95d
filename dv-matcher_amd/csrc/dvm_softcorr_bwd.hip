// dvm_softcorr_bwd.hip — backward twin of the soft-correspondence kernel (SURVEY §8b "backward twins";
// reference: autograd through models/loss.py:110-114 `softmax(-alpha * cdist)` followed by the top-k
// keep of models/loss.py:1339-1347).
//
// Forward (dvm_softcorr.hip):  D_ij = |f1_i - f2_j|,  S = neg_alpha * D,  P_ij = exp(S_ij - smax_i) / l_i,
// outputs val_t = P_{i, idx_t} for the row's top-k.  With g_t = dL/dval_t, gp_t = g_t * val_t, G_i = sum_t gp_t:
//     dL/dS_ij = [j = idx_t] gp_t  -  P_ij * G_i
//     W_ij     = neg_alpha * dL/dS_ij / D_ij              (0 where D_ij = 0, like cdist's backward)
//     df1_i    = sum_j W_ij (f1_i - f2_j)   ,   df2_j = sum_i W_ij (f2_j - f1_i)
// The row's top-k columns belong to the prep kernel, BOTH terms: W = neg_alpha * (gp_t - val_t * G) / D with the
// exact-difference D and the forward's own val_t as P.  On a one-hot row the two terms cancel exactly; split over
// two kernels they would each take their own D (and the dense one a P recomputed from it), and for a column much
// closer than sqrt(eps) |f| the 1/D of the two differ by O(1): a gradient of order alpha * g where it is ~0.  The
// prep kernel marks those columns in a bit matrix [B][N][ceil(M/32)] and the dense passes skip them.  (The
// columns of a row's top-k are distinct, as the forward writes them; its padding slots at M < topk carry val 0.)
// Every other column takes the dense term (-P*G), recomputed tile by tile from row_smax / row_sum, flash-attention
// style, once row-major (df1) and once column-major (df2).  Per 32x32 tile: 64 fp32 MFMAs (32x32x2) rebuild the
// distances by the norm expansion, ~15 VALU per entry turn them into W in the accumulator layout, and 64 more MFMAs
// apply W to the staged rows — W's C-layout registers are fed straight back as the A operand (the contraction index
// is permuted consistently on the B side), so W never touches LDS.  Where the expansion cancels
// (v < TAU (|f_o|^2 + |f_i|^2): a cluster of columns near one query, more than its top-k) the entry's D is
// redone from the exact difference in a wave-uniform branch that ordinary features never take.
// The geometry, the tile, the redo, the skip mask, the apply chain and the output loop are the phase-B pieces of
// dvm_dist_tile.h.
#include <algorithm>

#include "dvm_dist_tile.h"

namespace dvm {
namespace {

using namespace dtile;

constexpr int BW_TILE_FLOATS = ROWS_FLOATS + 3 * KT + BW_MASK;  // rows + {norm, c2, coef} + mask
constexpr size_t BW_LDS_BYTES = ((size_t)2 * BW_TILE_FLOATS + BW_OB) * sizeof(float);


// "outer" rows live in registers (32 per wave), "inner" rows stream through LDS.  The softmax row statistics
// (c2 = smax*log2e, coef = -neg_alpha*G/l) belong to f1's rows: they sit on the outer side in the df1 pass
// and on the inner side in the df2 pass; the other side's pointers are null (c2 = 0, coef = 1).
struct SBGroup {
    const float *fo, *fi, *no, *ni;
    const float *c2o, *coefo, *c2i, *coefi;
    float *dout;
    int No, Ni, tiles_o;
};
struct SBArgs {
    SBGroup g[2];
    const uint32_t *topk_bits;  // [B][N][wpr]: bit j of row i set for the row's top-k columns (the prep kernel owns them)
    int wpr;                    // (M + 31) / 32
    int blocks0;  // B * g[0].tiles_o * split
    int split;    // the inner loop is cut into `split` pieces (small batches: fill the chip); outputs are atomics
    float a2;     // neg_alpha * log2(e)
};

// (its own prologue and loop, not a frame and a loop shared with skb_apply_mfma_kernel: both kernels sit at 256 VGPRs with spills,
// and any change in their text moved the spill counts up)
__global__ __launch_bounds__(BW_THREADS, 2) void softcorr_bwd_mfma_kernel(const SBArgs args) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float *const rsum = smem + 2 * BW_TILE_FLOATS;  // [BW_OB]

    int lid = xcd_remap(blockIdx.x, gridDim.x);
    const int grp = lid >= args.blocks0 ? 1 : 0;
    lid -= grp ? args.blocks0 : 0;
    const SBGroup &G = args.g[grp];
    const int No = G.No, Ni = G.Ni;
    const int sp = lid % args.split;
    lid /= args.split;
    const int ot = lid % G.tiles_o, b = lid / G.tiles_o;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r32 = lane & 31, h = lane >> 5;
    const float a2 = args.a2;

    const float *ibase = G.fi + (size_t)b * Ni * D;
    const float *inb = G.ni + (size_t)b * Ni;
    const float *ic2 = G.c2i ? G.c2i + (size_t)b * Ni : nullptr;
    const float *icf = G.coefi ? G.coefi + (size_t)b * Ni : nullptr;

    const int orow = ot * BW_OB + wave * 32 + r32;
    const int orc = orow < No ? orow : No - 1;
    const float *op = G.fo + ((size_t)b * No + orc) * D;
    float q[D / 2];  // B operand of the distance GEMM
    load_query_frag(op, h, q);
    const float nrm_o = G.no[(size_t)b * No + orc];
    const float c2_o = G.c2o ? G.c2o[(size_t)b * No + orc] : 0.f;
    const float coef_o = orow < No ? (G.coefo ? G.coefo[(size_t)b * No + orc] : 1.f) : 0.f;

    const int ntiles = (Ni + KT - 1) / KT;
    const int per = (ntiles + args.split - 1) / args.split;
    const int t0 = sp * per, t1 = min(ntiles, t0 + per);
    if (t0 >= t1) return;  // uniform over the workgroup

    f32x4 pre[BW_LD_PER_THREAD];
    float pres = 0.f;
    uint32_t prem = 0;
    const uint32_t *bits = args.topk_bits;
    const int wpr = args.wpr;
    auto issue_loads = [&](int t) {
        const int j0 = t * KT;
        issue_tile<BW_THREADS>(ibase, j0, Ni, tid, pre);
        if (tid < 3 * KT) {  // threads 0..63: norm, 64..127: c2, 128..191: coef
            const int which = tid >> 6, j = j0 + (tid & 63);
            const bool ok = j < Ni;
            if (which == 0) pres = ok ? inb[j] : 0.f;
            else if (which == 1) pres = (ok && ic2) ? ic2[j] : 0.f;
            else pres = ok ? (icf ? icf[j] : 1.f) : 0.f;
        }
        prem = skip_mask_load<BW_WAVES>(grp, bits, wpr, b, ot, j0, No, Ni, tid);
    };
    auto commit_loads = [&](int buf) {
        float *kt = smem + buf * BW_TILE_FLOATS;
        commit_tile<BW_THREADS>(kt, tid, pre);
        if (tid < 3 * KT) kt[ROWS_FLOATS + tid] = pres;
        ((uint32_t *)kt)[ROWS_FLOATS + 3 * KT + tid] = prem;
    };

    f32x16 acc2[4];  // [position block cb] : out[outer row (C layout)][position 4*r32 + cb]
#pragma unroll
    for (int cb = 0; cb < 4; ++cb)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc2[cb][r] = 0.f;
    float rl = 0.f;  // this lane's share of sum_t W[t][o]

    issue_loads(t0);
    commit_loads(0);
    __syncthreads();

    for (int t = t0; t < t1; ++t) {
        const int buf = (t - t0) & 1;
        const float *kt = smem + buf * BW_TILE_FLOATS;
        if (t + 1 < t1) issue_loads(t + 1);
#pragma unroll 1
        for (int sub = 0; sub < 2; ++sub) {
            f32x16 acc;
            outer_inner_sqdist(kt, kt + ROWS_FLOATS, sub, r32, h, q, op, nrm_o, acc);
            // this lane's 16 inner rows: lane_key(r, h)
            const float *sc = kt + ROWS_FLOATS + sub * 32 + 4 * h;
            const uint32_t *msk = (const uint32_t *)(kt + ROWS_FLOATS + 3 * KT);
            const unsigned skip = skip_mask_lane<BW_WAVES>(grp, msk, wave, r32, sub, h);
            float w[16];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x4 cc = *(const f32x4 *)(sc + KT + 8 * g);
                const f32x4 cf = *(const f32x4 *)(sc + 2 * KT + 8 * g);
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int r = 4 * g + u;
                    const float v = fmaxf(acc[r], 0.f);
                    const float dist = sqrt_rn(v);
                    const float e = __builtin_amdgcn_exp2f(fmaf(dist, a2, -(c2_o + cc[u])));
                    const float wv = (coef_o * cf[u]) * e * __builtin_amdgcn_rcpf(dist);
                    // padding rows of the last tile carry coef 0 but zero features: their "distance" |f_o| can be far
                    // below the row minimum, e overflows to +inf and 0 * inf would poison the whole output row
                    w[r] = (v > 0.f && cf[u] != 0.f && !((skip >> r) & 1u)) ? wv : 0.f;
                    rl += w[r];
                }
            }
            apply_chain(kt, sub, r32, h, w, acc2);
        }
        if (t + 1 < t1) commit_loads(buf ^ 1);
        __syncthreads();
    }

    // atomics: the split pieces and the prep kernel's top-k entries add to the same rows
    store_outer_rows<true>(rsum, rl, G.fo, G.dout, b, ot * BW_OB + wave * 32, No, wave, r32, h, acc2);
}

// Any d (multiple of 4, <= 512): one wave per outer row, lanes own channels lane + 64u.  Reference-quality
// fallback and the cross-check for the MFMA kernel (variant 1).
struct SBScalarArgs {
    SBGroup g[2];
    const uint32_t *topk_bits;  // as in SBArgs
    int wpr;
    long rows0;      // B * g[0].No
    long rows_total;  // rows0 + B * g[1].No
    int d;
    float a2;
};

__global__ __launch_bounds__(256) void softcorr_bwd_scalar_kernel(const SBScalarArgs args) {
    const int lane = threadIdx.x & 63;
    long gw = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (gw >= args.rows_total) return;
    const int grp = gw >= args.rows0 ? 1 : 0;
    gw -= grp ? args.rows0 : 0;
    const SBGroup &G = args.g[grp];
    const int No = G.No, Ni = G.Ni, d = args.d;
    const int b = (int)(gw / No), row = (int)(gw % No);
    const float *fo = G.fo + ((size_t)b * No + row) * d;
    float ov[8], av[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int c = lane + 64 * u;
        ov[u] = c < d ? fo[c] : 0.f;
        av[u] = 0.f;
    }
    const float nrm_o = G.no[(size_t)b * No + row];
    const float c2_o = G.c2o ? G.c2o[(size_t)b * No + row] : 0.f;
    const float coef_o = G.coefo ? G.coefo[(size_t)b * No + row] : 1.f;
    float rsum = 0.f;
    for (int j = 0; j < Ni; ++j) {
        const float *fi = G.fi + ((size_t)b * Ni + j) * d;
        float xv[8];
        const float part = wave_row_load_dot(fi, d, lane, ov, xv);
        // the row's top-k columns are the prep kernel's (grp 0: outer = f1 row, grp 1: inner j = f1 row)
        const uint32_t *bw = args.topk_bits + (grp == 0 ? ((size_t)b * No + row) * args.wpr + (j >> 5)
                                                         : ((size_t)b * Ni + j) * args.wpr + (row >> 5));
        if ((*bw >> (grp == 0 ? (j & 31) : (row & 31))) & 1u) continue;  // uniform over the wave
        const float v = wave_row_sqdist(part, ov, xv, nrm_o, G.ni[(size_t)b * Ni + j]);
        const float dist = sqrt_rn(v);
        const float c2 = c2_o + (G.c2i ? G.c2i[(size_t)b * Ni + j] : 0.f);
        const float cf = coef_o * (G.coefi ? G.coefi[(size_t)b * Ni + j] : 1.f);
        const float w = v > 0.f ? cf * exp2f(fmaf(dist, args.a2, -c2)) / dist : 0.f;
        rsum += w;
#pragma unroll
        for (int u = 0; u < 8; ++u) av[u] = fmaf(w, xv[u], av[u]);
    }
    float *dst = G.dout + ((size_t)b * No + row) * d;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int c = lane + 64 * u;
        if (c < d) unsafeAtomicAdd(dst + c, rsum * ov[u] - av[u]);
    }
}

// Per f1 row: G = sum_t g_t*val_t, the row's dense-term coefficients, the top-k bits, and both terms of the top-k
// entries (gathered rows of f2; scatter-add into df2).  One wave per row, lanes own channels lane + 64u.
__global__ __launch_bounds__(256) void softcorr_bwd_prep_kernel(const float *__restrict__ f1, const float *__restrict__ f2,
                                                                const float *__restrict__ pi_val,
                                                                const int32_t *__restrict__ pi_idx,
                                                                const float *__restrict__ gval,
                                                                const float *__restrict__ row_smax,
                                                                const float *__restrict__ row_sum, int B, int N, int M, int d,
                                                                int topk, float neg_alpha, float *__restrict__ coef,
                                                                float *__restrict__ c2, uint32_t *__restrict__ topk_bits,
                                                                float *__restrict__ df1, float *__restrict__ df2) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= (long)B * N) return;
    const int b = (int)(row / N);
    const float *a = f1 + (size_t)row * d;
    float av[8], own[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int c = lane + 64 * u;
        av[u] = c < d ? a[c] : 0.f;
        own[u] = 0.f;
    }
    float G = 0.f;
    for (int t = 0; t < topk; ++t) G += gval[(size_t)row * topk + t] * pi_val[(size_t)row * topk + t];
    const int wpr = (M + 31) >> 5;
    for (int t = 0; t < topk; ++t) {
        const int j = pi_idx[(size_t)row * topk + t];
        if (j < 0 || j >= M) continue;  // uniform over the wave
        if (lane == 0) atomicOr(topk_bits + (size_t)row * wpr + (j >> 5), 1u << (j & 31));
        // both terms of the entry, on the forward's P: [j = idx_t] gp_t - val_t G = 0 where the row is one-hot
        const float val = pi_val[(size_t)row * topk + t];
        const float ds = fmaf(-val, G, gval[(size_t)row * topk + t] * val);
        if (ds == 0.f) continue;
        const float gp = ds;
        const float *x = f2 + ((size_t)b * M + j) * d;
        float dx[8], part = 0.f;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int c = lane + 64 * u;
            dx[u] = c < d ? av[u] - x[c] : 0.f;
            part = fmaf(dx[u], dx[u], part);
        }
        const float D = sqrt_rn(wave_sum(part));
        if (!(D > 0.f)) continue;
        const float w = neg_alpha * gp / D;
        float *dst = df2 + ((size_t)b * M + j) * d;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int c = lane + 64 * u;
            own[u] = fmaf(w, dx[u], own[u]);
            if (c < d) unsafeAtomicAdd(dst + c, -w * dx[u]);
        }
    }
    if (lane == 0) {
        coef[row] = -neg_alpha * G / row_sum[row];
        c2[row] = row_smax[row] * LOG2E;
    }
    float *dst = df1 + (size_t)row * d;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int c = lane + 64 * u;
        if (c < d) unsafeAtomicAdd(dst + c, own[u]);
    }
}

}  // namespace
}  // namespace dvm

using namespace dvm;

struct SoftcorrBwdWs {
    float *n1, *coef, *c2, *n2;
    uint32_t *bits;   // [B][N][wpr]: one bit per column
    int wpr;
};
static size_t carve_softcorr_bwd(Arena &ar, int B, int N, int M, SoftcorrBwdWs &w) {
    w.n1 = ar.take<float>((size_t)B * N);
    w.coef = ar.take<float>((size_t)B * N);
    w.c2 = ar.take<float>((size_t)B * N);
    w.n2 = ar.take<float>((size_t)B * M);
    w.wpr = (M + 31) / 32;
    w.bits = ar.take<uint32_t>((size_t)B * N * w.wpr);
    return ar.off;
}

DVM_EXPORT size_t dvm_softcorr_bwd_workspace_bytes(int B, int N, int M, int d) {
    (void)d;
    return null_carve<SoftcorrBwdWs>(carve_softcorr_bwd, B, N, M);
}

DVM_EXPORT int dvm_softcorr_bwd_f32(const float *f1, const float *f2, int B, int N, int M, int d, float neg_alpha, int topk,
                                    const float *pi_val, const int32_t *pi_idx, const float *row_smax, const float *row_sum,
                                    const float *g_val, float *d_f1, float *d_f2, int variant, void *ws, size_t ws_bytes,
                                    void *stream) {
    const int rc = softcorr_family_check("dvm_softcorr_bwd_f32", f1 && f2 && pi_val && pi_idx && row_smax && row_sum && g_val && d_f1 && d_f2, B,
                                         N, M, d, topk, neg_alpha, variant, 2);
    if (rc != DVM_OK) return rc;
    DVM_REQUIRE(variant != 2 || d == D, "dvm_softcorr_bwd_f32: MFMA variant needs d == 128");
    SoftcorrBwdWs w;
    if (!carve_ws(ws, ws_bytes, "dvm_softcorr_bwd_f32", w, carve_softcorr_bwd, B, N, M)) return DVM_ENOSPACE;
    float *const n1 = w.n1, *const coef = w.coef, *const c2 = w.c2, *const n2 = w.n2;
    uint32_t *const bits = w.bits;
    const int wpr = w.wpr;
    hipStream_t s = (hipStream_t)stream;
    (void)hipMemsetAsync(d_f1, 0, (size_t)B * N * d * sizeof(float), s);
    (void)hipMemsetAsync(d_f2, 0, (size_t)B * M * d * sizeof(float), s);
    (void)hipMemsetAsync(bits, 0, (size_t)B * N * wpr * sizeof(uint32_t), s);
    launch_rownorm2(f1, B * N, d, n1, s);
    launch_rownorm2(f2, B * M, d, n2, s);
    hipLaunchKernelGGL(softcorr_bwd_prep_kernel, dim3((unsigned)(((size_t)B * N + 3) / 4)), dim3(256), 0, s, f1, f2, pi_val, pi_idx,
                       g_val, row_smax, row_sum, B, N, M, d, topk, neg_alpha, coef, c2, bits, d_f1, d_f2);
    const float a2 = neg_alpha * LOG2E;
    const bool mfma = (variant == 2) || (variant == 0 && d == D);
    if (mfma) {
        SBArgs a;
        a.g[0] = SBGroup{f1, f2, n1, n2, c2, coef, nullptr, nullptr, d_f1, N, M, (N + BW_OB - 1) / BW_OB};
        a.g[1] = SBGroup{f2, f1, n2, n1, nullptr, nullptr, c2, coef, d_f2, M, N, (M + BW_OB - 1) / BW_OB};
        int split = 1;
        const int base = B * (a.g[0].tiles_o + a.g[1].tiles_o);
        const int min_tiles = (std::min(N, M) + KT - 1) / KT;
        while (base * split < 512 && split < 8 && min_tiles / (2 * split) >= 4) split *= 2;
        a.split = split;
        a.topk_bits = bits;
        a.wpr = wpr;
        a.blocks0 = B * a.g[0].tiles_o * split;
        a.a2 = a2;
        ensure_dyn_lds((const void *)softcorr_bwd_mfma_kernel, (int)BW_LDS_BYTES);
        hipLaunchKernelGGL(softcorr_bwd_mfma_kernel, dim3(base * split), dim3(BW_THREADS), BW_LDS_BYTES, s, a);
    } else {
        SBScalarArgs a;
        a.g[0] = SBGroup{f1, f2, n1, n2, c2, coef, nullptr, nullptr, d_f1, N, M, 0};
        a.g[1] = SBGroup{f2, f1, n2, n1, nullptr, nullptr, c2, coef, d_f2, M, N, 0};
        a.rows0 = (long)B * N;
        a.rows_total = (long)B * N + (long)B * M;
        a.topk_bits = bits;
        a.wpr = wpr;
        a.d = d;
        a.a2 = a2;
        const size_t rows = (size_t)B * N + (size_t)B * M;
        hipLaunchKernelGGL(softcorr_bwd_scalar_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, a);
    }
    DVM_CHECK_LAUNCH("softcorr_bwd");
    return DVM_OK;
}
