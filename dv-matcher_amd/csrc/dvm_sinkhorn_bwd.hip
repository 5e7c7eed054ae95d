// dvm_sinkhorn_bwd.hip — backward twin of the Sinkhorn-normalised soft correspondence (dvm_sinkhorn.hip): the exact
// gradient of the unrolled, fixed-n_iter operator with respect to f1 and f2.  NOT in the reference.
//
// Forward, T = n_iter, c = log(N/M), v^0 = 0 (history kept by dvm_sinkhorn_fwd_hist_f32):
//     u^t_i = -LSE_j(S_ij + v^(t-1)_j)     v^t_j = c - LSE_i(S_ij + u^t_i)     t = 1..T
//     u^f_i = -LSE_j(S_ij + v^T_j)         P_ij = exp(S_ij + u^f_i + v^T_j)    val_t = P_{i, idx_t}
// Backward, g_t = dL/dval_t, gp_t = g_t val_t, G_i = sum_t gp_t:
//     Sbar_ij = [j = idx_t] gp_t - G_i P_ij  -  sum_t ( vbar^t_j Q^t_ij + ubar^t_i R^t_ij )
//     Q^t_ij = exp(S_ij + u^t_i + v^t_j - c)     R^t_ij = exp(S_ij + u^t_i + v^(t-1)_j)
//     vbar^T_j = sum_i ([j = idx_t] gp_t - G_i P_ij)     ubar^t_i = -sum_j vbar^t_j Q^t_ij     vbar^(t-1)_j = -sum_i ubar^t_i R^t_ij
//     W_ij = neg_alpha Sbar_ij / D_ij (0 where D_ij = 0)     df1_i = sum_j W_ij (f1_i - f2_j)     df2_j = sum_i W_ij (f2_j - f1_i)
// Every exponent is that of a probability, so each term takes its own exp2 (the factored form P exp(du) exp(dv) leaves
// fp32's range: |v^t - v^T| reaches 300).  No N x M array is written: the potentials' history is (T+1)(N+M) floats.
//
//   prep        one wave per f1 row: G, the top-k bit matrix [B][N][ceil(M/32)] (as dvm_softcorr_bwd.hip), and per top-k
//               slot the final-step term E = gp_t - val_t G on the forward's own val_t, with its weight neg_alpha E / D on
//               the exact-difference D — both terms on one D, so that a one-hot row cancels.  Writes the slots' share of df1.
//   colgather   the column side of those slots WITHOUT atomics: one wave per 8 columns walks the bit matrix's word column
//               in ascending row order, finds the slot in the row's pi_idx and adds the slot's E into vbar^T_j and its
//               weight into df2_j — a gather in ascending edge order, the same bits on every run.
//   phase A     2T sweeps of the forward's shape (256 query rows per workgroup, keys streamed through the double-buffered
//               LDS tile, squared distances on the fp32 matrix cores, the exact sqrt: the forward's S_ij bit for bit).  A
//               query accumulates -sum_key coef_key exp(S + pot_query + pot_key) in fp64; the first sweep (vbar^T) skips
//               the top-k entries' final-step term through the bit matrix and adds to what colgather left.
//   pack        the 2(T+1) per-row and per-column scalars of phase B (potentials scaled by log2 e, coefficients) as planes.
//   phase B     the phase-B pieces of dvm_dist_tile.h (shared with softcorr_bwd_mfma_kernel), one launch per pass (df1
//               row-major, df2 column-major): outer rows in registers, inner rows and their scalar planes through LDS,
//               distances by 64 fp32 MFMAs per 32x32 tile with the TAU exact-difference redo, the entry's weight the
//               sum of 2T + 1 exp2 terms, W fed back as
//               the A operand of the second product.  The inner loop is never split: an output row is owned by one
//               workgroup and added to the slots' share with a plain read-modify-write.
// No float atomics and no host synchronisation anywhere, n_iter = 0 included (it runs prep, colgather, pack and phase B
// with one term; dvm_softcorr_bwd_f32's atomics are not used).  variant 1 runs scalar forms of phase A and B (any
// d % 4 == 0, d <= 512; untuned): the cross-check of the matrix-core kernels and the path for d != 128.
// Every kernel here forms its distances with dvm_dist_tile.h, which also owns the workgroup geometries and the sweep loops
// (two_role_sweep, scalar_sweep): what is here are the argument structs, the planes and the epilogues.
//
// dvm_sinkhorn_ub_bwd_f32 is the same structure for the unbalanced operator (the formulas are in include/dvm.h).  Its history
// holds the normalisers m^t, n^t; skb_ub_pots_kernel re-makes the potentials u^t, v^t from them by the forward's expression.
// prep takes H_i = tau_row G_i - (1 - tau_row) g_lmass_i for G_i and R^f = val exp(-row_lmass) for P; a phase A sweep scales
// what it stores (nbar^t = tau_col vbar^t, mbar^t = tau_row ubar^t are what the next sweep and phase B read); Q^t pairs
// (u^t, n^t) and R^t pairs (m^t, v^(t-1)), so phase B reads R^t's potentials from a third group of planes; and
// skb_ub_logw_kernel adds the adjoints over t, in ascending t, into d_log_a / d_log_b.
#include <float.h>
#include <math.h>

#include <algorithm>

#include "dvm_dist_tile.h"

namespace dvm {
namespace {

using namespace dtile;

constexpr int SKB_MAX_ITER = 32;

// ------------------------------------------------------------------------------------------------ prep / colgather / pack
__global__ __launch_bounds__(256) void skb_prep_kernel(const float *__restrict__ f1, const float *__restrict__ f2,
                                                       const float *__restrict__ pi_val, const int32_t *__restrict__ pi_idx,
                                                       const float *__restrict__ gval, int B, int N, int M, int d, int topk,
                                                       float neg_alpha, float *__restrict__ Gout, float *__restrict__ esp,
                                                       float *__restrict__ wsp, uint32_t *__restrict__ topk_bits,
                                                       float *__restrict__ df1, const float *__restrict__ row_lmass,
                                                       const float *__restrict__ g_lmass, float tau_row, float *__restrict__ Graw) {
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
    // unbalanced (row_lmass given): the final step's coefficient is H, its probability R^f = val / mass.  exp(-row_lmass) is
    // applied as two equal factors: it alone leaves fp32's range where the mass is below 2^-126 and val is still nonzero.
    const float Graw_i = G;
    float unmass = 1.f;
    if (row_lmass) {
        G = tau_row * G - (1.f - tau_row) * (g_lmass ? g_lmass[row] : 0.f);
        unmass = expf(-0.5f * fmaxf(row_lmass[row], -170.f));   // (below e^-170 every val is 0)
    }
    const int wpr = (M + 31) >> 5;
    for (int t = 0; t < topk; ++t) {
        const int j = pi_idx[(size_t)row * topk + t];
        float E = 0.f, w = 0.f;
        if (j >= 0 && j < M) {   // uniform over the wave
            if (lane == 0) atomicOr(topk_bits + (size_t)row * wpr + (j >> 5), 1u << (j & 31));
            const float val = pi_val[(size_t)row * topk + t];
            E = fmaf(row_lmass ? -((val * unmass) * unmass) : -val, G, gval[(size_t)row * topk + t] * val);
            if (E != 0.f) {
                const float *x = f2 + ((size_t)b * M + j) * d;
                float dx[8], part = 0.f;
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int c = lane + 64 * u;
                    dx[u] = c < d ? av[u] - x[c] : 0.f;
                    part = fmaf(dx[u], dx[u], part);
                }
                const float D = sqrt_rn(wave_sum(part));
                if (D > 0.f) {
                    w = neg_alpha * E / D;
#pragma unroll
                    for (int u = 0; u < 8; ++u) own[u] = fmaf(w, dx[u], own[u]);
                }
            }
        }
        if (lane == 0) {
            esp[(size_t)row * topk + t] = E;
            wsp[(size_t)row * topk + t] = w;
        }
    }
    if (lane == 0) Gout[row] = G;
    if (lane == 0 && Graw) Graw[row] = Graw_i;
    float *dst = df1 + (size_t)row * d;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int c = lane + 64 * u;
        if (c < d) dst[c] = own[u];
    }
}

// one workgroup per (entry, 32-column word), each of its 4 waves owning 8 of the columns: acc [32][d] and the 32 column sums
// live in LDS; every wave walks all rows (a column's hits stay in ascending row order whatever the wave count)
__global__ __launch_bounds__(256) void skb_colgather_kernel(const float *__restrict__ f1, const float *__restrict__ f2,
                                                           const int32_t *__restrict__ pi_idx, const float *__restrict__ esp,
                                                           const float *__restrict__ wsp, const uint32_t *__restrict__ topk_bits,
                                                           int N, int M, int d, int topk, float *__restrict__ df2,
                                                           float *__restrict__ vbarT, long vbar_bs) {
    extern __shared__ __attribute__((aligned(16))) float smem[];   // [32][d] + [32]
    const int lane = threadIdx.x & 63;
    const uint32_t mine = 0xffu << (8 * (threadIdx.x >> 6));   // this wave's columns of the word
    const int wpr = (M + 31) >> 5;
    const int wc = blockIdx.x, b = blockIdx.y;
    float *vacc = smem + 32 * d;
    for (int e = threadIdx.x; e < 32 * d + 32; e += 256) smem[e] = 0.f;
    __syncthreads();
    for (int i0 = 0; i0 < N; i0 += 64) {
        const int i = i0 + lane;
        const uint32_t word = i < N ? (topk_bits[((size_t)b * N + i) * wpr + wc] & mine) : 0u;
        unsigned long long m = __ballot(word != 0u);
        while (m) {
            const int l = __ffsll((long long)m) - 1;
            m &= m - 1;
            uint32_t w = (uint32_t)__shfl((int)word, l, 64);
            const int ii = i0 + l;
            const size_t srow = ((size_t)b * N + ii) * topk;
            const int myidx = lane < topk ? pi_idx[srow + lane] : -1;
            const float *x1 = f1 + ((size_t)b * N + ii) * d;
            while (w) {
                const int c = __ffs((int)w) - 1;
                w &= w - 1;
                const int j = wc * 32 + c;
                unsigned long long mm = __ballot(myidx == j);   // the slot(s) of column j in row ii (padding slots repeat column 0 with E = 0)
                float wv = 0.f, ev = 0.f;
                while (mm) {
                    const int t = __ffsll((long long)mm) - 1;
                    mm &= mm - 1;
                    wv += wsp[srow + t];
                    ev += esp[srow + t];
                }
                if (lane == 0) vacc[c] += ev;
                if (wv != 0.f) {
                    const float *x2 = f2 + ((size_t)b * M + j) * d;
                    for (int ch = lane; ch < d; ch += 64) smem[c * d + ch] = fmaf(wv, x2[ch] - x1[ch], smem[c * d + ch]);
                }
            }
        }
    }
    __syncthreads();
    for (int c = 0; c < 32; ++c) {
        const int j = wc * 32 + c;
        if (j >= M) break;
        for (int ch = threadIdx.x; ch < d; ch += 256) df2[((size_t)b * M + j) * d + ch] = smem[c * d + ch];
    }
    if (vbarT && threadIdx.x < 32 && wc * 32 + threadIdx.x < M) vbarT[(size_t)b * vbar_bs + wc * 32 + threadIdx.x] = vacc[threadIdx.x];
}

// planes of phase B, K2 = 2 (T + 1) per side: [0..T] potentials * log2(e), [T+1..2T+1] coefficients
//   rows:    pot[0] = u^f, pot[t] = u^t;   coef[0] = G, coef[t] = ubar^t
//   columns: pot[t] = v^t (t = 0..T);      coef[0] unused, coef[t] = vbar^t * M/N  (the -c of Q^t)
__global__ void skb_pack_kernel(const float *__restrict__ u_hist, const float *__restrict__ v_hist, const float *__restrict__ G,
                                const float *__restrict__ ubar, const float *__restrict__ vbar, int N, int M, int T, float m_over_n,
                                float *__restrict__ tabR, float *__restrict__ tabC) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int t = blockIdx.y, b = blockIdx.z;
    const int K2 = 2 * (T + 1);
    if (i < N) {
        const float *uh = u_hist + (size_t)b * (T + 1) * N;
        tabR[((size_t)b * K2 + t) * N + i] = uh[(size_t)(t == 0 ? T : t - 1) * N + i] * LOG2E;
        tabR[((size_t)b * K2 + T + 1 + t) * N + i] = t == 0 ? G[(size_t)b * N + i] : ubar[((size_t)b * T + t - 1) * N + i];
    }
    if (i < M) {
        tabC[((size_t)b * K2 + t) * M + i] = v_hist[((size_t)b * (T + 1) + t) * M + i] * LOG2E;
        tabC[((size_t)b * K2 + T + 1 + t) * M + i] = t == 0 ? 0.f : vbar[((size_t)b * T + t - 1) * M + i] * m_over_n;
    }
}

// unbalanced: the potentials of every iterate from the normalisers, by the forward's expression tau * (log weight + normaliser)
//   upot [B][T][N]: u^1..u^T      vpot [B][T+1][M]: v^0 = 0, v^1..v^T      (log_a NULL = 0, log_b NULL = log_ratio)
__global__ void skb_ub_pots_kernel(const float *__restrict__ rn_hist, const float *__restrict__ cn_hist, const float *__restrict__ log_a,
                                   const float *__restrict__ log_b, float tau_row, float tau_col, float log_ratio, int N, int M, int T,
                                   float *__restrict__ upot, float *__restrict__ vpot) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int t = blockIdx.y, b = blockIdx.z;
    if (i < N && t < T) {
        const float w = log_a ? log_a[(size_t)b * N + i] : 0.f;
        upot[((size_t)b * T + t) * N + i] = tau_row * (w + rn_hist[((size_t)b * (T + 1) + t) * N + i]);
    }
    if (i < M) {
        const float w = log_b ? log_b[(size_t)b * M + i] : log_ratio;
        vpot[((size_t)b * (T + 1) + t) * M + i] = t == 0 ? 0.f : tau_col * (w + cn_hist[((size_t)b * (T + 1) + t) * M + i]);
    }
}

// unbalanced planes of phase B, K2 = 3 (T + 1) per side: [0..T] Q^t's potentials, [T+1..2T+1] coefficients, [2T+2..3T+2] R^t's
//   rows:    potQ[0] = m^f, potQ[t] = u^t;   coef[0] = H, coef[t] = mbar^t;   potR[0] = m^f, potR[t] = m^t
//   columns: potQ[t] = n^t;                  coef[0] unused, coef[t] = nbar^t;   potR[t] = v^t (t = 0..T: R^t reads v^(t-1), the final step v^T)
__global__ void skb_ub_pack_kernel(const float *__restrict__ rn_hist, const float *__restrict__ cn_hist, const float *__restrict__ upot,
                                   const float *__restrict__ vpot, const float *__restrict__ H, const float *__restrict__ mbar,
                                   const float *__restrict__ nbar, int N, int M, int T, float *__restrict__ tabR, float *__restrict__ tabC) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int t = blockIdx.y, b = blockIdx.z;
    const int K2 = 3 * (T + 1);
    if (i < N) {
        const float m = rn_hist[((size_t)b * (T + 1) + (t == 0 ? T : t - 1)) * N + i] * LOG2E;
        tabR[((size_t)b * K2 + t) * N + i] = t == 0 ? m : upot[((size_t)b * T + t - 1) * N + i] * LOG2E;
        tabR[((size_t)b * K2 + T + 1 + t) * N + i] = t == 0 ? H[(size_t)b * N + i] : mbar[((size_t)b * T + t - 1) * N + i];
        tabR[((size_t)b * K2 + 2 * T + 2 + t) * N + i] = m;
    }
    if (i < M) {
        tabC[((size_t)b * K2 + t) * M + i] = cn_hist[((size_t)b * (T + 1) + t) * M + i] * LOG2E;
        tabC[((size_t)b * K2 + T + 1 + t) * M + i] = t == 0 ? 0.f : nbar[((size_t)b * T + t - 1) * M + i];
        tabC[((size_t)b * K2 + 2 * T + 2 + t) * M + i] = vpot[((size_t)b * (T + 1) + t) * M + i] * LOG2E;
    }
}

// d_log_a_i = tau_row (G_i + g_lmass_i) + sum_t mbar^t_i      d_log_b_j = sum_t nbar^t_j      (t ascending; either may be NULL)
__global__ void skb_ub_logw_kernel(const float *__restrict__ G, const float *__restrict__ g_lmass, const float *__restrict__ mbar,
                                   const float *__restrict__ nbar, float tau_row, int N, int M, int T, float *__restrict__ d_log_a,
                                   float *__restrict__ d_log_b) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int b = blockIdx.y;
    if (d_log_a && i < N) {
        float acc = tau_row * (G[(size_t)b * N + i] + (g_lmass ? g_lmass[(size_t)b * N + i] : 0.f));
        for (int t = 0; t < T; ++t) acc += mbar[((size_t)b * T + t) * N + i];
        d_log_a[(size_t)b * N + i] = acc;
    }
    if (d_log_b && i < M) {
        float acc = 0.f;
        for (int t = 0; t < T; ++t) acc += nbar[((size_t)b * T + t) * M + i];
        d_log_b[(size_t)b * M + i] = acc;
    }
}

// ------------------------------------------------------------------------------------------------ phase A
struct SAArgs {
    const float *q, *k;       // queries [B][N][d], keys [B][M][d]
    const float *nq, *nk;     // their |.|^2
    const float *potq, *potk, *coefk;   // the queries' potential, the keys' potential and coefficient (entry b at p + b * bs)
    long potq_bs, potk_bs, coefk_bs, out_bs;
    float add;                // added to the queries' potential (-c in the sweeps over Q^t)
    float scale;              // on what is stored: 1, or the tau that turns vbar into nbar / ubar into mbar (unbalanced)
    int N, M, d, tiles;
    float neg_alpha;
    float *out;               // out_q = [MASKED: out_q] - sum_k coef_k exp(S_qk + potk_k + (potq_q + add))
    const uint32_t *bits;     // MASKED (queries = columns, keys = f1 rows): the top-k bit matrix, entries with a set bit are skipped
    int wpr;
};

// scalar form: the scalar sweep of dvm_dist_tile.h (one thread per query row, keys through LDS in tiles of 32)
template <bool SWAP, bool MASKED>
__global__ __launch_bounds__(128) void skb_sweep_scalar_kernel(const SAArgs a) {
    // two sidecar planes: the keys' potentials and coefficients
    const int N = a.N, M = a.M;
    const ScalarFrame f = scalar_frame(a.q, a.nq, N, a.d);
    const int b = f.b, i = f.i, ic = f.ic;
    const float na = f.na;
    const float pq = a.potq[(size_t)b * a.potq_bs + ic] + a.add;
    const float neg_alpha = a.neg_alpha;
    double sum = 0.0;
    scalar_sweep(
        f, a.k, a.nk, M, a.d,
        [&](int j, bool in, float *side) {
            side[SC_KT] = in ? a.potk[(size_t)b * a.potk_bs + j] : 0.f;
            side[2 * SC_KT] = in ? a.coefk[(size_t)b * a.coefk_bs + j] : 0.f;
        },
        [&](int j0, const float (&acc)[SC_KT], const float *kn) {
            const float *kp = kn + SC_KT, *kc = kn + 2 * SC_KT;
            float ls = 0.f;
#pragma unroll
            for (int j = 0; j < SC_KT; ++j) {
                const float L = sqrt_rn(sqdist<SWAP>(acc[j], na, kn[j])) * neg_alpha + kp[j];
                float term = kc[j] * __builtin_amdgcn_exp2f((L + pq) * LOG2E);
                if (MASKED) {
                    const int key = j0 + j < M ? j0 + j : M - 1;
                    const uint32_t word = a.bits[((size_t)b * M + key) * a.wpr + (ic >> 5)];
                    term = ((word >> (ic & 31)) & 1u) ? 0.f : term;
                }
                ls += term;
            }
            sum += (double)ls;
        });
    if (i < N) {
        float *o = a.out + (size_t)b * a.out_bs + i;
        *o = (float)((MASKED ? (double)*o : 0.0) - sum) * a.scale;
    }
}

// matrix-core form (d == 128): tile, LDS layout, geometry and the two-role phase structure of dvm_dist_tile.h
constexpr int SA_TILE_FLOATS = ROWS_FLOATS + 3 * KT + KT * SW_WAVES;   // keys + {norm, potential, coefficient} + mask words [key][wave]
constexpr size_t SA_LDS_BYTES = (size_t)2 * SA_TILE_FLOATS * sizeof(float);

template <bool SWAP, bool MASKED>
__global__ __launch_bounds__(SW_THREADS, 2) void skb_sweep_mfma_kernel(const SAArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    // (its own prologue, not row_frame: with the frame the backward benchmarks came out slower than the two runs before it differ)
    const int lid = xcd_remap(blockIdx.x, gridDim.x);
    const int N = a.N, M = a.M;
    const int b = lid / a.tiles;
    const int qt = lid % a.tiles;
    const float neg_alpha = a.neg_alpha;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r32 = lane & 31, h = lane >> 5;

    const float *kbase = a.k + (size_t)b * M * D;
    const float *knb = a.nk + (size_t)b * M;
    const float *kpb = a.potk + (size_t)b * a.potk_bs;
    const float *kcb = a.coefk + (size_t)b * a.coefk_bs;
    const uint32_t *bits = a.bits;
    const int wpr = a.wpr;

    const int qrow = qt * SW_QB + wave * SW_QW + r32;
    const int qrc = qrow < N ? qrow : N - 1;
    float q[D / 2];
    load_query_frag(a.q + ((size_t)b * N + qrc) * D, h, q);
    const float na = a.nq[(size_t)b * N + qrc];
    const float pq = a.potq[(size_t)b * a.potq_bs + qrc] + a.add;
    double sum = 0.0;

    const int ntiles = (M + KT - 1) / KT;
    f32x4 pre[SW_LD_PER_THREAD];
    float pren = 0.f;   // threads 0..63: a key's norm; 64..127: its potential; 128..191: its coefficient
    uint32_t prem = 0;  // MASKED: the word of key tid / 8 for the 32 queries of wave tid % 8

    auto issue_loads = [&](int t) __attribute__((always_inline)) {
        const int j0 = t * KT;
        issue_tile<SW_THREADS>(kbase, j0, M, tid, pre);
        if (tid < KT)
            pren = (j0 + tid < M) ? knb[j0 + tid] : INFINITY;
        else if (tid < 2 * KT)
            pren = (j0 + tid - KT < M) ? kpb[j0 + tid - KT] : 0.f;
        else if (tid < 3 * KT)
            pren = (j0 + tid - 2 * KT < M) ? kcb[j0 + tid - 2 * KT] : 0.f;
        if (MASKED) prem = skip_mask_load<SW_WAVES>(1, bits, wpr, b, qt, j0, N, M, tid);   // queries = columns: the df2 layout
    };
    auto commit_loads = [&](int buf) __attribute__((always_inline)) {
        float *kt = smem + buf * SA_TILE_FLOATS;
        commit_tile<SW_THREADS>(kt, tid, pre);
        if (tid < 3 * KT) kt[ROWS_FLOATS + tid] = pren;
        if (MASKED) ((uint32_t *)kt)[ROWS_FLOATS + 3 * KT + tid] = prem;
    };

    f32x16 acc;
    float nbv[16], pv[16], cv[16];
    unsigned skip = 0;
    auto mfma_chain = [&](int buf, int sub) __attribute__((always_inline)) {
        const float *kt = smem + buf * SA_TILE_FLOATS;
        dist_chain(kt, sub, r32, h, q, acc);
        lane_scalars(kt + ROWS_FLOATS, sub, h, nbv);
        lane_scalars(kt + ROWS_FLOATS + KT, sub, h, pv);
        lane_scalars(kt + ROWS_FLOATS + 2 * KT, sub, h, cv);
        if (MASKED) skip = skip_mask_lane<SW_WAVES>(1, (const uint32_t *)(kt + ROWS_FLOATS + 3 * KT), wave, r32, sub, h);
    };
    auto epilogue = [&](int, int) __attribute__((always_inline)) {
        float ls = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float L = sqrt_rn(sqdist<SWAP>(acc[r], na, nbv[r])) * neg_alpha + pv[r];   // -inf for padding keys
            const float term = cv[r] * __builtin_amdgcn_exp2f((L + pq) * LOG2E);
            ls += (MASKED && ((skip >> r) & 1u)) ? 0.f : term;
        }
        sum += (double)ls;
    };

    const int role = __builtin_amdgcn_readfirstlane(wave >> 2);
    two_role_sweep<false>(ntiles, role, issue_loads, commit_loads, mfma_chain, epilogue);

    sum += __shfl_xor(sum, 32, 64);
    if (h == 0 && qrow < N) {
        float *o = a.out + (size_t)b * a.out_bs + qrow;
        *o = (float)((MASKED ? (double)*o : 0.0) - sum) * a.scale;
    }
}

template <bool SWAP, bool MASKED>
void launch_sweep_t(bool mfma, SAArgs a, int B, hipStream_t s) {
    if (mfma) {
        a.tiles = (a.N + SW_QB - 1) / SW_QB;
        ensure_dyn_lds((const void *)skb_sweep_mfma_kernel<SWAP, MASKED>, (int)SA_LDS_BYTES);
        hipLaunchKernelGGL((skb_sweep_mfma_kernel<SWAP, MASKED>), dim3((unsigned)(B * a.tiles)), dim3(SW_THREADS), SA_LDS_BYTES, s, a);
    } else {
        const size_t lds = scalar_sweep_lds_bytes(a.d, 2);
        ensure_dyn_lds((const void *)skb_sweep_scalar_kernel<SWAP, MASKED>, 66 * 1024);
        hipLaunchKernelGGL((skb_sweep_scalar_kernel<SWAP, MASKED>), dim3((a.N + 127) / 128, B), dim3(128), lds, s, a);
    }
}

// ------------------------------------------------------------------------------------------------ phase B
constexpr int BW_FIXED_FLOATS = ROWS_FLOATS + KT + BW_MASK;   // rows + norms + mask; the K2 planes [K2][KT] follow

// group 0: df1 (outer = f1 rows, inner = f2 rows); group 1: df2 (outer = f2 rows, inner = f1 rows)
struct PBGroup {
    const float *fo, *fi, *no, *ni;
    const float *tabo, *tabi;   // skb_pack_kernel's planes of the outer / inner side
    float *dout;
    int No, Ni, tiles_o;
};
struct PBArgs {
    PBGroup g[2];
    const uint32_t *topk_bits;
    int wpr, T, tile_floats;
    float a2, nalpha;   // neg_alpha * log2(e), -neg_alpha
};

// UB: the unbalanced operator's planes (skb_ub_pack_kernel): R^t takes its two potentials from the third group
// (its own prologue and loop, as softcorr_bwd_mfma_kernel and for the same reason: 256 VGPRs with spills)
template <int grp, bool UB>
__global__ __launch_bounds__(BW_THREADS, 2) void skb_apply_mfma_kernel(const PBArgs args) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int TF = args.tile_floats;
    float *const rsum = smem + 2 * TF;   // [BW_OB]

    const int lid = xcd_remap(blockIdx.x, gridDim.x);
    const PBGroup &G = args.g[grp];
    const int No = G.No, Ni = G.Ni, T = args.T, K2 = (UB ? 3 : 2) * (T + 1);
    const int PR = 2 * T + 2;   // UB: the first of R^t's planes
    const int ot = lid % G.tiles_o, b = lid / G.tiles_o;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r32 = lane & 31, h = lane >> 5;
    const float a2 = args.a2;

    const float *ibase = G.fi + (size_t)b * Ni * D;
    const float *inb = G.ni + (size_t)b * Ni;
    const float *itab = G.tabi + (size_t)b * K2 * Ni;

    const int orow = ot * BW_OB + wave * 32 + r32;
    const int orc = orow < No ? orow : No - 1;
    const float *op = G.fo + ((size_t)b * No + orc) * D;
    const float *to = G.tabo + (size_t)b * K2 * No + orc;   // plane kk at to[kk * No]
    float q[D / 2];
    load_query_frag(op, h, q);
    const float nrm_o = G.no[(size_t)b * No + orc];

    const int ntiles = (Ni + KT - 1) / KT;
    f32x4 pre[BW_LD_PER_THREAD];
    float pres = 0.f;
    uint32_t prem = 0;
    const uint32_t *bits = args.topk_bits;
    const int wpr = args.wpr;
    auto issue_loads = [&](int t) __attribute__((always_inline)) {
        const int j0 = t * KT;
        issue_tile<BW_THREADS>(ibase, j0, Ni, tid, pre);
        if (tid < KT) pres = (j0 + tid < Ni) ? inb[j0 + tid] : 0.f;
        prem = skip_mask_load<BW_WAVES>(grp, bits, wpr, b, ot, j0, No, Ni, tid);
    };
    // the planes go from L2 to LDS without a register stage (their count depends on T); padding rows: potential -inf
    // (every term exp2(-inf) = 0), coefficient 0
    auto commit_loads = [&](int buf, int t) __attribute__((always_inline)) {
        float *kt = smem + buf * TF;
        const int j0 = t * KT;
        commit_tile<BW_THREADS>(kt, tid, pre);
        if (tid < KT) kt[ROWS_FLOATS + tid] = pres;
        ((uint32_t *)kt)[ROWS_FLOATS + KT + tid] = prem;
        for (int e = tid; e < K2 * KT; e += BW_THREADS) {
            const int kk = e >> 6, j = j0 + (e & 63);
            kt[BW_FIXED_FLOATS + e] = j < Ni ? itab[(size_t)kk * Ni + j] : ((kk <= T || kk >= PR) ? -INFINITY : 0.f);
        }
    };

    f32x16 acc2[4];
#pragma unroll
    for (int cb = 0; cb < 4; ++cb)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc2[cb][r] = 0.f;
    float rl = 0.f;

    issue_loads(0);
    commit_loads(0, 0);
    __syncthreads();

    for (int t = 0; t < ntiles; ++t) {
        const int buf = t & 1;
        const float *kt = smem + buf * TF;
        if (t + 1 < ntiles) issue_loads(t + 1);
#pragma unroll 1
        for (int sub = 0; sub < 2; ++sub) {
            f32x16 acc;
            outer_inner_sqdist(kt, kt + ROWS_FLOATS, sub, r32, h, q, op, nrm_o, acc);
            const uint32_t *msk = (const uint32_t *)(kt + ROWS_FLOATS + KT);
            const float *tb = kt + BW_FIXED_FLOATS + sub * 32 + 4 * h;   // plane kk of this lane's 16 inner rows: tb[kk * 64 + 8 * g + u]
            // acc becomes the distance; w the sum of the entry's 2T + 1 terms
            float w[16];
            {   // the final row step's term, skipped on the row's top-k columns (prep / colgather own it there)
                const unsigned skip = skip_mask_lane<BW_WAVES>(grp, msk, wave, r32, sub, h);
                const int vT = UB ? PR + T : T;   // the columns' plane of v^T
                const float po = to[(size_t)(grp == 0 ? 0 : vT) * No];
                const float co = grp == 0 ? to[(size_t)(T + 1) * No] : 1.f;
                const float *pin = tb + (grp == 0 ? vT : 0) * KT;
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const f32x4 pi = *(const f32x4 *)(pin + 8 * g);
                    f32x4 ci = {1.f, 1.f, 1.f, 1.f};
                    if (grp == 1) ci = *(const f32x4 *)(tb + (T + 1) * KT + 8 * g);
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int r = 4 * g + u;
                        acc[r] = sqrt_rn(fmaxf(acc[r], 0.f));
                        const float e = __builtin_amdgcn_exp2f(fmaf(acc[r], a2, po + pi[u]));
                        w[r] = ((skip >> r) & 1u) ? 0.f : (co * ci[u]) * e;
                    }
                }
            }
#pragma unroll 1
            for (int tt = 1; tt <= T; ++tt) {
                const float po = to[(size_t)tt * No];
                // R^t: balanced, the row's u^t again and the column's v^(t-1); UB, the row's m^t and the column's v^(t-1)
                const float pox = UB ? to[(size_t)(PR + tt - grp) * No] : (grp == 0 ? po : to[(size_t)(tt - 1) * No]);
                const float co = to[(size_t)(T + 1 + tt) * No];
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const f32x4 pi = *(const f32x4 *)(tb + tt * KT + 8 * g);
                    f32x4 pix = pi;
                    if (UB)
                        pix = *(const f32x4 *)(tb + (PR + tt - 1 + grp) * KT + 8 * g);
                    else if (grp == 0)
                        pix = *(const f32x4 *)(tb + (tt - 1) * KT + 8 * g);
                    const f32x4 ci = *(const f32x4 *)(tb + (T + 1 + tt) * KT + 8 * g);
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int r = 4 * g + u;
                        const float e1 = __builtin_amdgcn_exp2f(fmaf(acc[r], a2, po + pi[u]));     // Q^t: u^t + v^t
                        const float e2 = __builtin_amdgcn_exp2f(fmaf(acc[r], a2, pox + pix[u]));   // R^t: u^t + v^(t-1)
                        // Q^t carries the column's coefficient, R^t the row's
                        w[r] = fmaf(grp == 0 ? ci[u] : co, e1, w[r]);
                        w[r] = fmaf(grp == 0 ? co : ci[u], e2, w[r]);
                    }
                }
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float wv = args.nalpha * w[r] * __builtin_amdgcn_rcpf(acc[r]);
                w[r] = acc[r] > 0.f ? wv : 0.f;
                rl += w[r];
            }
            apply_chain(kt, sub, r32, h, w, acc2);
        }
        if (t + 1 < ntiles) commit_loads(buf ^ 1, t + 1);
        __syncthreads();
    }

    // this workgroup owns the rows: a plain add on top of the top-k slots' share
    store_outer_rows<false>(rsum, rl, G.fo, G.dout, b, ot * BW_OB + wave * 32, No, wave, r32, h, acc2);
}

// scalar form: one wave per outer row, lanes own channels lane + 64u (the scalar phase B of dvm_dist_tile.h)
struct PBScalarArgs {
    const float *f1, *f2, *n1, *n2, *tabR, *tabC;
    float *df1, *df2;
    const uint32_t *topk_bits;
    int N, M, d, T, wpr;
    int ub;   // the unbalanced operator's planes (skb_ub_pack_kernel)
    long rows0, rows_total;
    float a2, nalpha;
};

__global__ __launch_bounds__(256) void skb_apply_scalar_kernel(const PBScalarArgs args) {
    const int lane = threadIdx.x & 63;
    long gw = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (gw >= args.rows_total) return;
    const int grp = gw >= args.rows0 ? 1 : 0;
    gw -= grp ? args.rows0 : 0;
    const int N = args.N, M = args.M, d = args.d, T = args.T, K2 = (args.ub ? 3 : 2) * (T + 1);
    const int PR = args.ub ? 2 * T + 2 : 0;   // the first of R^t's planes (balanced: R^t reads Q^t's)
    const int No = grp ? M : N, Ni = grp ? N : M;
    const int b = (int)(gw / No), row = (int)(gw % No);
    const float *fob = grp ? args.f2 : args.f1, *fib = grp ? args.f1 : args.f2;
    const float *nob = grp ? args.n2 : args.n1, *nib = grp ? args.n1 : args.n2;
    const float *tr = args.tabR + (size_t)b * K2 * N, *tc = args.tabC + (size_t)b * K2 * M;
    const float *fo = fob + ((size_t)b * No + row) * d;
    float ov[8], av[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int c = lane + 64 * u;
        ov[u] = c < d ? fo[c] : 0.f;
        av[u] = 0.f;
    }
    const float nrm_o = nob[(size_t)b * No + row];
    float rsum = 0.f;
    for (int j = 0; j < Ni; ++j) {
        const float *fi = fib + ((size_t)b * Ni + j) * d;
        float xv[8];
        const float part = wave_row_load_dot(fi, d, lane, ov, xv);
        const int ri = grp ? j : row, ci = grp ? row : j;   // the entry's f1 row and f2 row (column)
        const bool topk = (args.topk_bits[((size_t)b * N + ri) * args.wpr + (ci >> 5)] >> (ci & 31)) & 1u;
        const float v = wave_row_sqdist(part, ov, xv, nrm_o, nib[(size_t)b * Ni + j]);
        if (!(v > 0.f)) continue;
        const float D = sqrt_rn(v);
        float sum = topk ? 0.f : tr[(size_t)(T + 1) * N + ri] * exp2f(fmaf(D, args.a2, tr[ri] + tc[(size_t)(PR + T) * M + ci]));
        for (int t = 1; t <= T; ++t) {
            const float pr = tr[(size_t)t * N + ri];
            sum = fmaf(tc[(size_t)(T + 1 + t) * M + ci], exp2f(fmaf(D, args.a2, pr + tc[(size_t)t * M + ci])), sum);
            sum = fmaf(tr[(size_t)(T + 1 + t) * N + ri],
                       exp2f(fmaf(D, args.a2, tr[(size_t)(PR + t) * N + ri] + tc[(size_t)(PR + t - 1) * M + ci])), sum);
        }
        const float w = args.nalpha * sum / D;
        rsum += w;
#pragma unroll
        for (int u = 0; u < 8; ++u) av[u] = fmaf(w, xv[u], av[u]);
    }
    float *dst = (grp ? args.df2 : args.df1) + ((size_t)b * No + row) * d;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int c = lane + 64 * u;
        if (c < d) dst[c] += rsum * ov[u] - av[u];
    }
}

// ub (dvm_sinkhorn_ub_bwd_f32): ubar / vbar hold mbar / nbar, the planes are 3 (T + 1) per side, plus the unscaled G and the
// re-made potentials upot [B][T][N], vpot [B][T+1][M]
struct SkbWs {
    float *n1, *n2, *G, *esp, *wsp, *ubar, *vbar, *tabR, *tabC, *Graw, *upot, *vpot;
    uint32_t *bits;
};
size_t skb_carve(Arena &ar, int B, int N, int M, int n_iter, int topk, bool ub, SkbWs &w) {
    const size_t T = (size_t)n_iter, P = ub ? 3 : 2;
    w.n1 = ar.take<float>((size_t)B * N);
    w.n2 = ar.take<float>((size_t)B * M);
    w.G = ar.take<float>((size_t)B * N);
    w.esp = ar.take<float>((size_t)B * N * topk);
    w.wsp = ar.take<float>((size_t)B * N * topk);
    w.ubar = ar.take<float>((size_t)B * N * (T ? T : 1));
    w.vbar = ar.take<float>((size_t)B * M * (T ? T : 1));
    w.tabR = ar.take<float>((size_t)B * N * P * (T + 1));
    w.tabC = ar.take<float>((size_t)B * M * P * (T + 1));
    w.bits = ar.take<uint32_t>((size_t)B * N * ((M + 31) / 32));
    w.Graw = ub ? ar.take<float>((size_t)B * N) : nullptr;
    w.upot = ub ? ar.take<float>((size_t)B * N * (T ? T : 1)) : nullptr;
    w.vpot = ub ? ar.take<float>((size_t)B * M * (T + 1)) : nullptr;
    return ar.off;
}

}  // namespace
}  // namespace dvm

using namespace dvm;

DVM_EXPORT size_t dvm_sinkhorn_bwd_workspace_bytes(int B, int N, int M, int d, int n_iter) {
    (void)d;
    if (B < 1 || N < 1 || M < 1 || n_iter < 0 || n_iter > SKB_MAX_ITER) return 0;
    return null_carve<SkbWs>(skb_carve, B, N, M, n_iter, 16, false);   // (sized for the longest list)
}

// what the unbalanced entry adds to the run below
struct SkbUb {
    float tau_row, tau_col;
    const float *log_a, *log_b, *row_lmass, *g_lmass;
    float *d_log_a, *d_log_b;
};

// Both backward entries.  balanced (ub NULL): rhist / chist are u_hist / v_hist.  unbalanced: they are rn_hist / cn_hist, the
// potentials come from skb_ub_pots_kernel, and every sweep stores its result times the tau of the side it belongs to.
static int skb_run(const SkbWs &w, const float *f1, const float *f2, int B, int N, int M, int d, float neg_alpha, int T, int topk,
                   const float *pi_val, const int32_t *pi_idx, const float *rhist, const float *chist, const float *g_val, float *d_f1,
                   float *d_f2, bool mfma, const SkbUb *ub, hipStream_t s) {
    const int wpr = (M + 31) / 32;
    const long u_bs = (long)(T + 1) * N, v_bs = (long)(T + 1) * M;
    const float c = (float)log((double)N / (double)M);
    (void)hipMemsetAsync(w.bits, 0, (size_t)B * N * wpr * sizeof(uint32_t), s);
    launch_rownorm2(f1, B * N, d, w.n1, s);
    launch_rownorm2(f2, B * M, d, w.n2, s);
    if (ub)
        hipLaunchKernelGGL(skb_ub_pots_kernel, dim3((std::max(N, M) + 255) / 256, T + 1, B), dim3(256), 0, s, rhist, chist, ub->log_a, ub->log_b,
                           ub->tau_row, ub->tau_col, c, N, M, T, w.upot, w.vpot);
    hipLaunchKernelGGL(skb_prep_kernel, dim3((unsigned)(((size_t)B * N + 3) / 4)), dim3(256), 0, s, f1, f2, pi_val, pi_idx, g_val, B, N, M, d,
                       topk, neg_alpha, w.G, w.esp, w.wsp, w.bits, d_f1, ub ? ub->row_lmass : nullptr, ub ? ub->g_lmass : nullptr,
                       ub ? ub->tau_row : 1.f, w.Graw);
    {
        const size_t lds = (size_t)(32 * d + 32) * sizeof(float);
        ensure_dyn_lds((const void *)skb_colgather_kernel, 66 * 1024);
        hipLaunchKernelGGL(skb_colgather_kernel, dim3(wpr, B), dim3(256), lds, s, f1, f2, pi_idx, w.esp, w.wsp, w.bits, N, M, d, topk, d_f2,
                           T ? w.vbar + (size_t)(T - 1) * M : nullptr, (long)T * M);
    }
    if (T) {
        // the potentials of the queries / keys of each sweep: balanced, slices of the two histories (Q^t's -c on the row side);
        // unbalanced, Q^t = exp(S + u^t + n^t) and R^t = exp(S + m^t + v^(t-1)) pair a re-made potential with a normaliser
        const float *uQ = ub ? w.upot : rhist, *vR = ub ? w.vpot : chist;
        const long uQ_bs = ub ? (long)T * N : u_bs;
        SAArgs row{}, col{};
        row.q = f1, row.k = f2, row.nq = w.n1, row.nk = w.n2, row.N = N, row.M = M, row.d = d, row.neg_alpha = neg_alpha;
        col.q = f2, col.k = f1, col.nq = w.n2, col.nk = w.n1, col.N = M, col.M = N, col.d = d, col.neg_alpha = neg_alpha;
        row.potq_bs = uQ_bs, row.potk_bs = v_bs, row.coefk_bs = (long)T * M, row.out_bs = (long)T * N, row.add = ub ? 0.f : -c;
        col.potq_bs = v_bs, col.potk_bs = u_bs, col.out_bs = (long)T * M, col.add = 0.f;
        row.scale = ub ? ub->tau_row : 1.f, col.scale = ub ? ub->tau_col : 1.f;
        // vbar^T_j = [colgather: the top-k slots] - sum_i G_i P_ij over the other entries (unbalanced: H_i R^f_ij)
        col.potq = vR + (size_t)T * M, col.potk = rhist + (size_t)T * N, col.coefk = w.G, col.coefk_bs = N;
        col.out = w.vbar + (size_t)(T - 1) * M, col.bits = w.bits, col.wpr = wpr;
        launch_sweep_t<true, true>(mfma, col, B, s);
        col.bits = nullptr, col.coefk_bs = (long)T * N;
        for (int t = T; t >= 1; --t) {
            row.potq = uQ + (size_t)(t - 1) * N, row.potk = chist + (size_t)t * M, row.coefk = w.vbar + (size_t)(t - 1) * M;
            row.out = w.ubar + (size_t)(t - 1) * N;
            launch_sweep_t<false, false>(mfma, row, B, s);   // ubar^t = -sum_j vbar^t_j Q^t_ij
            if (t > 1) {
                col.potq = vR + (size_t)(t - 1) * M, col.potk = rhist + (size_t)(t - 1) * N, col.coefk = w.ubar + (size_t)(t - 1) * N;
                col.out = w.vbar + (size_t)(t - 2) * M;
                launch_sweep_t<true, false>(mfma, col, B, s);   // vbar^(t-1) = -sum_i ubar^t_i R^t_ij
            }
        }
    }
    const dim3 pgrid((std::max(N, M) + 255) / 256, T + 1, B);
    if (ub) {
        hipLaunchKernelGGL(skb_ub_pack_kernel, pgrid, dim3(256), 0, s, rhist, chist, w.upot, w.vpot, w.G, w.ubar, w.vbar, N, M, T, w.tabR, w.tabC);
        if (ub->d_log_a || ub->d_log_b)
            hipLaunchKernelGGL(skb_ub_logw_kernel, dim3((std::max(N, M) + 255) / 256, B), dim3(256), 0, s, w.Graw, ub->g_lmass, w.ubar, w.vbar,
                               ub->tau_row, N, M, T, ub->d_log_a, ub->d_log_b);
    } else {
        hipLaunchKernelGGL(skb_pack_kernel, pgrid, dim3(256), 0, s, rhist, chist, w.G, w.ubar, w.vbar, N, M, T, (float)((double)M / (double)N),
                           w.tabR, w.tabC);
    }
    const float a2 = neg_alpha * LOG2E;
    const int planes = (ub ? 3 : 2) * (T + 1);
    if (mfma) {
        PBArgs a;
        a.g[0] = PBGroup{f1, f2, w.n1, w.n2, w.tabR, w.tabC, d_f1, N, M, (N + BW_OB - 1) / BW_OB};
        a.g[1] = PBGroup{f2, f1, w.n2, w.n1, w.tabC, w.tabR, d_f2, M, N, (M + BW_OB - 1) / BW_OB};
        a.topk_bits = w.bits, a.wpr = wpr, a.T = T, a.a2 = a2, a.nalpha = -neg_alpha;
        a.tile_floats = BW_FIXED_FLOATS + planes * KT;
        const size_t lds = ((size_t)2 * a.tile_floats + BW_OB) * sizeof(float);
        const int lds_max = (int)(((size_t)2 * (BW_FIXED_FLOATS + (ub ? 3 : 2) * (SKB_MAX_ITER + 1) * KT) + BW_OB) * sizeof(float));
        if (ub) {
            ensure_dyn_lds((const void *)skb_apply_mfma_kernel<0, true>, lds_max);
            ensure_dyn_lds((const void *)skb_apply_mfma_kernel<1, true>, lds_max);
            hipLaunchKernelGGL((skb_apply_mfma_kernel<0, true>), dim3(B * a.g[0].tiles_o), dim3(BW_THREADS), lds, s, a);
            hipLaunchKernelGGL((skb_apply_mfma_kernel<1, true>), dim3(B * a.g[1].tiles_o), dim3(BW_THREADS), lds, s, a);
        } else {
            ensure_dyn_lds((const void *)skb_apply_mfma_kernel<0, false>, lds_max);
            ensure_dyn_lds((const void *)skb_apply_mfma_kernel<1, false>, lds_max);
            hipLaunchKernelGGL((skb_apply_mfma_kernel<0, false>), dim3(B * a.g[0].tiles_o), dim3(BW_THREADS), lds, s, a);
            hipLaunchKernelGGL((skb_apply_mfma_kernel<1, false>), dim3(B * a.g[1].tiles_o), dim3(BW_THREADS), lds, s, a);
        }
    } else {
        PBScalarArgs a;
        a.f1 = f1, a.f2 = f2, a.n1 = w.n1, a.n2 = w.n2, a.tabR = w.tabR, a.tabC = w.tabC, a.df1 = d_f1, a.df2 = d_f2;
        a.topk_bits = w.bits, a.N = N, a.M = M, a.d = d, a.T = T, a.wpr = wpr, a.ub = ub ? 1 : 0, a.a2 = a2, a.nalpha = -neg_alpha;
        a.rows0 = (long)B * N, a.rows_total = (long)B * N + (long)B * M;
        hipLaunchKernelGGL(skb_apply_scalar_kernel, dim3((unsigned)((a.rows_total + 3) / 4)), dim3(256), 0, s, a);
    }
    DVM_CHECK_LAUNCH("sinkhorn_bwd");
    return DVM_OK;
}

DVM_EXPORT int dvm_sinkhorn_bwd_f32(const float *f1, const float *f2, int B, int N, int M, int d, float neg_alpha, int n_iter, int topk,
                                    const float *pi_val, const int32_t *pi_idx, const float *u_hist, const float *v_hist,
                                    const float *g_val, float *d_f1, float *d_f2, int variant, void *ws, size_t ws_bytes, void *stream) {
    const int rc = softcorr_family_check("dvm_sinkhorn_bwd_f32", f1 && f2 && pi_val && pi_idx && u_hist && v_hist && g_val && d_f1 && d_f2, B, N,
                                         M, d, topk, neg_alpha, variant, 1, n_iter, SKB_MAX_ITER);
    if (rc != DVM_OK) return rc;
    SkbWs w;
    if (!carve_ws(ws, ws_bytes, "dvm_sinkhorn_bwd_f32", w, skb_carve, B, N, M, n_iter, topk, false)) return DVM_ENOSPACE;
    return skb_run(w, f1, f2, B, N, M, d, neg_alpha, n_iter, topk, pi_val, pi_idx, u_hist, v_hist, g_val, d_f1, d_f2, variant == 0 && d == D,
                   nullptr, (hipStream_t)stream);
}

DVM_EXPORT size_t dvm_sinkhorn_ub_bwd_workspace_bytes(int B, int N, int M, int d, int n_iter) {
    (void)d;
    if (B < 1 || N < 1 || M < 1 || n_iter < 0 || n_iter > SKB_MAX_ITER) return 0;
    return null_carve<SkbWs>(skb_carve, B, N, M, n_iter, 16, true);
}

DVM_EXPORT int dvm_sinkhorn_ub_bwd_f32(const float *f1, const float *f2, int B, int N, int M, int d, float neg_alpha, int n_iter, int topk,
                                       float tau_row, float tau_col, const float *log_a, const float *log_b, const float *pi_val,
                                       const int32_t *pi_idx, const float *row_lmass, const float *rn_hist, const float *cn_hist,
                                       const float *g_val, const float *g_lmass, float *d_f1, float *d_f2, float *d_log_a, float *d_log_b,
                                       int variant, void *ws, size_t ws_bytes, void *stream) {
    const int rc = softcorr_family_check("dvm_sinkhorn_ub_bwd_f32",
                                         f1 && f2 && pi_val && pi_idx && row_lmass && rn_hist && cn_hist && g_val && d_f1 && d_f2, B, N, M, d, topk,
                                         neg_alpha, variant, 1, n_iter, SKB_MAX_ITER, tau_row, tau_col);
    if (rc != DVM_OK) return rc;
    SkbWs w;
    if (!carve_ws(ws, ws_bytes, "dvm_sinkhorn_ub_bwd_f32", w, skb_carve, B, N, M, n_iter, topk, true)) return DVM_ENOSPACE;
    const SkbUb ub{tau_row, tau_col, log_a, log_b, row_lmass, g_lmass, d_log_a, d_log_b};
    return skb_run(w, f1, f2, B, N, M, d, neg_alpha, n_iter, topk, pi_val, pi_idx, rn_hist, cn_hist, g_val, d_f1, d_f2, variant == 0 && d == D,
                   &ub, (hipStream_t)stream);
}
