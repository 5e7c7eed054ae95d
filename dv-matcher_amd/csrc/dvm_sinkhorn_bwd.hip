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
//   phase B     softcorr_bwd_mfma_kernel's structure, one launch per pass (df1 row-major, df2 column-major): outer
//               rows in registers, inner rows and their scalar planes through LDS, distances by 64 fp32 MFMAs per 32x32
//               tile with the BW_TAU exact-difference redo, the entry's weight the sum of 2T + 1 exp2 terms, W fed back as
//               the A operand of the second product.  The inner loop is never split: an output row is owned by one
//               workgroup and added to the slots' share with a plain read-modify-write.
// No float atomics and no host synchronisation anywhere, n_iter = 0 included (it runs prep, colgather, pack and phase B
// with one term; dvm_softcorr_bwd_f32's atomics are not used).  variant 1 runs scalar forms of phase A and B (any
// d % 4 == 0, d <= 512; untuned): the cross-check of the matrix-core kernels and the path for d != 128.
#include <float.h>
#include <math.h>

#include <algorithm>

#include "dvm_common.h"

namespace dvm {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

void launch_rownorm2(const float *x, int rows, int K, float *out, hipStream_t s);   // dvm_softcorr.hip

namespace {

constexpr float LOG2E = 1.4426950408889634f;
constexpr int SKB_MAX_ITER = 32;

// ------------------------------------------------------------------------------------------------ prep / colgather / pack
__global__ __launch_bounds__(256) void skb_prep_kernel(const float *__restrict__ f1, const float *__restrict__ f2,
                                                       const float *__restrict__ pi_val, const int32_t *__restrict__ pi_idx,
                                                       const float *__restrict__ gval, int B, int N, int M, int d, int topk,
                                                       float neg_alpha, float *__restrict__ Gout, float *__restrict__ esp,
                                                       float *__restrict__ wsp, uint32_t *__restrict__ topk_bits,
                                                       float *__restrict__ df1) {
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
        float E = 0.f, w = 0.f;
        if (j >= 0 && j < M) {   // uniform over the wave
            if (lane == 0) atomicOr(topk_bits + (size_t)row * wpr + (j >> 5), 1u << (j & 31));
            const float val = pi_val[(size_t)row * topk + t];
            E = fmaf(-val, G, gval[(size_t)row * topk + t] * val);
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

// ------------------------------------------------------------------------------------------------ phase A
struct SAArgs {
    const float *q, *k;       // queries [B][N][d], keys [B][M][d]
    const float *nq, *nk;     // their |.|^2
    const float *potq, *potk, *coefk;   // the queries' potential, the keys' potential and coefficient (entry b at p + b * bs)
    long potq_bs, potk_bs, coefk_bs, out_bs;
    float add;                // added to the queries' potential (-c in the sweeps over Q^t)
    int N, M, d, tiles;
    float neg_alpha;
    float *out;               // out_q = [MASKED: out_q] - sum_k coef_k exp(S_qk + potk_k + (potq_q + add))
    const uint32_t *bits;     // MASKED (queries = columns, keys = f1 rows): the top-k bit matrix, entries with a set bit are skipped
    int wpr;
};

constexpr int SS_KT = 32;
constexpr int SS_DC = 32;

// scalar form: sinkhorn_scalar_kernel's distances (one thread per query row, keys through LDS in tiles of 32)
template <bool SWAP, bool MASKED>
__global__ __launch_bounds__(128) void skb_sweep_scalar_kernel(const SAArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];   // [SS_KT][d] keys + norms + potentials + coefficients
    const int N = a.N, M = a.M, d = a.d;
    float *kt = smem;
    float *kn = smem + SS_KT * d;
    float *kp = kn + SS_KT;
    float *kc = kp + SS_KT;
    const int b = blockIdx.y;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int ic = i < N ? i : N - 1;
    const float *q = a.q + ((size_t)b * N + ic) * d;
    const float na = a.nq[(size_t)b * N + ic];
    const float pq = a.potq[(size_t)b * a.potq_bs + ic] + a.add;
    const float *kbase = a.k + (size_t)b * M * d;
    const float neg_alpha = a.neg_alpha;
    double sum = 0.0;
    for (int j0 = 0; j0 < M; j0 += SS_KT) {
        __syncthreads();
        for (int e = threadIdx.x; e < SS_KT * d / 4; e += blockDim.x) {
            int r = e / (d / 4), c = e % (d / 4);
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (j0 + r < M) v = *(const f32x4 *)(kbase + (size_t)(j0 + r) * d + 4 * c);
            *(f32x4 *)(kt + r * d + 4 * c) = v;
        }
        if (threadIdx.x < SS_KT) {
            const int j = j0 + threadIdx.x;
            kn[threadIdx.x] = j < M ? a.nk[(size_t)b * M + j] : INFINITY;
            kp[threadIdx.x] = j < M ? a.potk[(size_t)b * a.potk_bs + j] : 0.f;
            kc[threadIdx.x] = j < M ? a.coefk[(size_t)b * a.coefk_bs + j] : 0.f;
        }
        __syncthreads();
        float acc[SS_KT];
#pragma unroll
        for (int j = 0; j < SS_KT; ++j) acc[j] = 0.f;
        for (int c0 = 0; c0 < d; c0 += SS_DC) {
            float qr[SS_DC];
            int cw = d - c0 < SS_DC ? d - c0 : SS_DC;
#pragma unroll
            for (int c = 0; c < SS_DC; c += 4) {
                f32x4 v = {0.f, 0.f, 0.f, 0.f};
                if (c < cw) v = *(const f32x4 *)(q + c0 + c);
                qr[c] = -2.f * v.x, qr[c + 1] = -2.f * v.y, qr[c + 2] = -2.f * v.z, qr[c + 3] = -2.f * v.w;
            }
#pragma unroll
            for (int j = 0; j < SS_KT; ++j) {
#pragma unroll
                for (int c = 0; c < SS_DC; c += 4) {
                    if (c < cw) {
                        f32x4 kv = *(const f32x4 *)(kt + j * d + c0 + c);
                        acc[j] = fmaf(qr[c], kv.x, acc[j]);
                        acc[j] = fmaf(qr[c + 1], kv.y, acc[j]);
                        acc[j] = fmaf(qr[c + 2], kv.z, acc[j]);
                        acc[j] = fmaf(qr[c + 3], kv.w, acc[j]);
                    }
                }
            }
        }
        float ls = 0.f;
#pragma unroll
        for (int j = 0; j < SS_KT; ++j) {
            float d2 = SWAP ? (acc[j] + kn[j]) + na : (acc[j] + na) + kn[j];
            d2 = d2 > 0.f ? d2 : 0.f;
            const float L = sqrt_rn(d2) * neg_alpha + kp[j];
            float term = kc[j] * __builtin_amdgcn_exp2f((L + pq) * LOG2E);
            if (MASKED) {
                const int key = j0 + j < M ? j0 + j : M - 1;
                const uint32_t word = a.bits[((size_t)b * M + key) * a.wpr + (ic >> 5)];
                term = ((word >> (ic & 31)) & 1u) ? 0.f : term;
            }
            ls += term;
        }
        sum += (double)ls;
    }
    if (i < N) {
        float *o = a.out + (size_t)b * a.out_bs + i;
        *o = (float)((MASKED ? (double)*o : 0.0) - sum);
    }
}

// matrix-core form (d == 128): tile shapes, LDS layout and the two-role phase structure of sinkhorn_mfma_kernel
constexpr int SK_D = 128;
constexpr int SK_KT = 64;
constexpr int SK_LDK = SK_D + 4;
constexpr int SK_QW = 32;
constexpr int SK_WAVES = 8;
constexpr int SK_QB = SK_QW * SK_WAVES;
constexpr int SK_THREADS = 64 * SK_WAVES;
constexpr int SK_LD_PER_THREAD = SK_KT * SK_D / 4 / SK_THREADS;
constexpr int SA_TILE_FLOATS = SK_KT * SK_LDK + 3 * SK_KT + SK_KT * SK_WAVES;   // keys + {norm, potential, coefficient} + mask words [key][wave]
constexpr size_t SA_LDS_BYTES = (size_t)2 * SA_TILE_FLOATS * sizeof(float);

template <bool SWAP, bool MASKED>
__global__ __launch_bounds__(SK_THREADS, 2) void skb_sweep_mfma_kernel(const SAArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int lid = xcd_remap(blockIdx.x, gridDim.x);
    const int N = a.N, M = a.M;
    const int b = lid / a.tiles;
    const int qt = lid % a.tiles;
    const float neg_alpha = a.neg_alpha;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r32 = lane & 31, h = lane >> 5;

    const float *kbase = a.k + (size_t)b * M * SK_D;
    const float *knb = a.nk + (size_t)b * M;
    const float *kpb = a.potk + (size_t)b * a.potk_bs;
    const float *kcb = a.coefk + (size_t)b * a.coefk_bs;
    const uint32_t *bits = a.bits;
    const int wpr = a.wpr;

    const int qrow = qt * SK_QB + wave * SK_QW + r32;
    const int qrc = qrow < N ? qrow : N - 1;
    const float *qp = a.q + ((size_t)b * N + qrc) * SK_D;
    float q[SK_D / 2];
#pragma unroll
    for (int c = 0; c < SK_D / 4; ++c) {
        f32x4 v = *(const f32x4 *)(qp + 4 * c);
        q[2 * c] = -2.f * (h ? v.y : v.x);
        q[2 * c + 1] = -2.f * (h ? v.w : v.z);
    }
    const float na = a.nq[(size_t)b * N + qrc];
    const float pq = a.potq[(size_t)b * a.potq_bs + qrc] + a.add;
    double sum = 0.0;

    const int ntiles = (M + SK_KT - 1) / SK_KT;
    f32x4 pre[SK_LD_PER_THREAD];
    float pren = 0.f;   // threads 0..63: a key's norm; 64..127: its potential; 128..191: its coefficient
    uint32_t prem = 0;  // MASKED: the word of key tid / 8 for the 32 queries of wave tid % 8

    auto issue_loads = [&](int t) __attribute__((always_inline)) {
        const int j0 = t * SK_KT;
#pragma unroll
        for (int e = 0; e < SK_LD_PER_THREAD; ++e) {
            int id = tid + e * SK_THREADS;
            int r = id >> 5, c = id & 31;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (j0 + r < M) v = *(const f32x4 *)(kbase + (size_t)(j0 + r) * SK_D + 4 * c);
            pre[e] = v;
        }
        if (tid < SK_KT)
            pren = (j0 + tid < M) ? knb[j0 + tid] : INFINITY;
        else if (tid < 2 * SK_KT)
            pren = (j0 + tid - SK_KT < M) ? kpb[j0 + tid - SK_KT] : 0.f;
        else if (tid < 3 * SK_KT)
            pren = (j0 + tid - 2 * SK_KT < M) ? kcb[j0 + tid - 2 * SK_KT] : 0.f;
        if (MASKED) {
            const int key = j0 + (tid >> 3), wc = qt * SK_WAVES + (tid & 7);
            prem = (key < M && wc < wpr) ? bits[((size_t)b * M + key) * wpr + wc] : 0u;
        }
    };
    auto commit_loads = [&](int buf) __attribute__((always_inline)) {
        float *kt = smem + buf * SA_TILE_FLOATS;
#pragma unroll
        for (int e = 0; e < SK_LD_PER_THREAD; ++e) {
            int id = tid + e * SK_THREADS;
            int r = id >> 5, c = id & 31;
            float2 ev = {pre[e].x, pre[e].z}, od = {pre[e].y, pre[e].w};
            *(float2 *)(kt + r * SK_LDK + 2 * c) = ev;
            *(float2 *)(kt + r * SK_LDK + 64 + 2 * c) = od;
        }
        if (tid < 3 * SK_KT) kt[SK_KT * SK_LDK + tid] = pren;
        if (MASKED) ((uint32_t *)kt)[SK_KT * SK_LDK + 3 * SK_KT + tid] = prem;
    };

    issue_loads(0);
    commit_loads(0);
    __syncthreads();

    const int role = __builtin_amdgcn_readfirstlane(wave >> 2);   // see sinkhorn_mfma_kernel

    // everything the epilogue needs leaves LDS here: role 1 runs a sub-tile's epilogue after the barrier that frees its buffer
    auto mfma_chain = [&](const float *kt, int sub, f32x16 &acc, float (&nbv)[16], float (&pv)[16], float (&cv)[16], unsigned &skip) __attribute__((always_inline)) {
        const float *arow = kt + (sub * 32 + r32) * SK_LDK + h * 64;
        acc = f32x16{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < 16; ++c) {
            f32x4 av = *(const f32x4 *)(arow + 4 * c);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, q[4 * c], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, q[4 * c + 1], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, q[4 * c + 2], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, q[4 * c + 3], acc, 0, 0, 0);
        }
        const float *kn = kt + SK_KT * SK_LDK + sub * 32 + 4 * h;   // local key = (r&3) + 8*(r>>2) + 4*h
        const uint32_t *msk = (const uint32_t *)(kt + SK_KT * SK_LDK + 3 * SK_KT);
        skip = 0;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            f32x4 nb = *(const f32x4 *)(kn + 8 * g);
            f32x4 pb = *(const f32x4 *)(kn + SK_KT + 8 * g);
            f32x4 cb = *(const f32x4 *)(kn + 2 * SK_KT + 8 * g);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                nbv[4 * g + u] = nb[u], pv[4 * g + u] = pb[u], cv[4 * g + u] = cb[u];
                if (MASKED) skip |= ((msk[(sub * 32 + 4 * h + 8 * g + u) * SK_WAVES + wave] >> r32) & 1u) << (4 * g + u);
            }
        }
    };
    auto epilogue = [&](const f32x16 &acc, const float (&nbv)[16], const float (&pv)[16], const float (&cv)[16], unsigned skip) __attribute__((always_inline)) {
        float ls = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            float d2 = SWAP ? (acc[r] + nbv[r]) + na : (acc[r] + na) + nbv[r];   // +inf for padding keys
            d2 = d2 > 0.f ? d2 : 0.f;
            const float L = sqrt_rn(d2) * neg_alpha + pv[r];
            const float term = cv[r] * __builtin_amdgcn_exp2f((L + pq) * LOG2E);
            ls += (MASKED && ((skip >> r) & 1u)) ? 0.f : term;
        }
        sum += (double)ls;
    };

    f32x16 acc;
    float nbv[16], pv[16], cv[16];
    unsigned skip = 0;
    for (int t = 0; t < ntiles; ++t) {
        const int buf = t & 1;
        if (t + 1 < ntiles) issue_loads(t + 1);
        const float *kt = smem + buf * SA_TILE_FLOATS;
        if (role == 1 && t > 0) epilogue(acc, nbv, pv, cv, skip);   // the previous tile's second sub-tile
        mfma_chain(kt, 0, acc, nbv, pv, cv, skip);
        epilogue(acc, nbv, pv, cv, skip);
        mfma_chain(kt, 1, acc, nbv, pv, cv, skip);
        if (role == 0) epilogue(acc, nbv, pv, cv, skip);
        if (t + 1 < ntiles) commit_loads(buf ^ 1);
        __syncthreads();
    }
    if (role == 1) epilogue(acc, nbv, pv, cv, skip);

    sum += __shfl_xor(sum, 32, 64);
    if (h == 0 && qrow < N) {
        float *o = a.out + (size_t)b * a.out_bs + qrow;
        *o = (float)((MASKED ? (double)*o : 0.0) - sum);
    }
}

template <bool SWAP, bool MASKED>
void launch_sweep_t(bool mfma, SAArgs a, int B, hipStream_t s) {
    if (mfma) {
        a.tiles = (a.N + SK_QB - 1) / SK_QB;
        ensure_dyn_lds((const void *)skb_sweep_mfma_kernel<SWAP, MASKED>, (int)SA_LDS_BYTES);
        hipLaunchKernelGGL((skb_sweep_mfma_kernel<SWAP, MASKED>), dim3((unsigned)(B * a.tiles)), dim3(SK_THREADS), SA_LDS_BYTES, s, a);
    } else {
        const size_t lds = (size_t)(SS_KT * a.d + 3 * SS_KT) * sizeof(float);
        ensure_dyn_lds((const void *)skb_sweep_scalar_kernel<SWAP, MASKED>, 66 * 1024);
        hipLaunchKernelGGL((skb_sweep_scalar_kernel<SWAP, MASKED>), dim3((a.N + 127) / 128, B), dim3(128), lds, s, a);
    }
}

// ------------------------------------------------------------------------------------------------ phase B
constexpr int BW_D = 128;
constexpr int BW_KT = 64;
constexpr int BW_LDK = BW_D + 4;
constexpr int BW_WAVES = 4;
constexpr int BW_OB = 32 * BW_WAVES;
constexpr int BW_THREADS = 64 * BW_WAVES;
constexpr int BW_LD_PER_THREAD = BW_KT * BW_D / 4 / BW_THREADS;
constexpr int BW_MASK = 256;
constexpr int BW_FIXED_FLOATS = BW_KT * BW_LDK + BW_KT + BW_MASK;   // rows + norms + mask; the K2 planes [K2][BW_KT] follow
constexpr float BW_TAU = 1.f / 64.f;

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

template <int grp>
__global__ __launch_bounds__(BW_THREADS, 2) void skb_apply_mfma_kernel(const PBArgs args) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int TF = args.tile_floats;
    float *const rsum = smem + 2 * TF;   // [BW_OB]

    const int lid = xcd_remap(blockIdx.x, gridDim.x);
    const PBGroup &G = args.g[grp];
    const int No = G.No, Ni = G.Ni, T = args.T, K2 = 2 * (T + 1);
    const int ot = lid % G.tiles_o, b = lid / G.tiles_o;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r32 = lane & 31, h = lane >> 5;
    const float a2 = args.a2;

    const float *ibase = G.fi + (size_t)b * Ni * BW_D;
    const float *inb = G.ni + (size_t)b * Ni;
    const float *itab = G.tabi + (size_t)b * K2 * Ni;

    const int orow = ot * BW_OB + wave * 32 + r32;
    const int orc = orow < No ? orow : No - 1;
    const float *op = G.fo + ((size_t)b * No + orc) * BW_D;
    const float *to = G.tabo + (size_t)b * K2 * No + orc;   // plane kk at to[kk * No]
    float q[BW_D / 2];
#pragma unroll
    for (int c = 0; c < BW_D / 4; ++c) {
        f32x4 v = *(const f32x4 *)(op + 4 * c);
        q[2 * c] = -2.f * (h ? v.y : v.x);
        q[2 * c + 1] = -2.f * (h ? v.w : v.z);
    }
    const float nrm_o = G.no[(size_t)b * No + orc];

    const int ntiles = (Ni + BW_KT - 1) / BW_KT;
    f32x4 pre[BW_LD_PER_THREAD];
    float pres = 0.f;
    uint32_t prem = 0;
    const uint32_t *bits = args.topk_bits;
    const int wpr = args.wpr;
    auto issue_loads = [&](int t) __attribute__((always_inline)) {
        const int j0 = t * BW_KT;
#pragma unroll
        for (int e = 0; e < BW_LD_PER_THREAD; ++e) {
            int id = tid + e * BW_THREADS;
            int r = id >> 5, c = id & 31;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (j0 + r < Ni) v = *(const f32x4 *)(ibase + (size_t)(j0 + r) * BW_D + 4 * c);
            pre[e] = v;
        }
        if (tid < BW_KT) pres = (j0 + tid < Ni) ? inb[j0 + tid] : 0.f;
        if (grp == 0) {   // as softcorr_bwd_mfma_kernel
            const int mrow = ot * BW_OB + (tid >> 1), wc = (j0 >> 5) + (tid & 1);
            prem = (mrow < No && wc < wpr) ? bits[((size_t)b * No + mrow) * wpr + wc] : 0u;
        } else {
            const int irow = j0 + (tid >> 2), wc = ot * (BW_OB / 32) + (tid & 3);
            prem = (irow < Ni && wc < wpr) ? bits[((size_t)b * Ni + irow) * wpr + wc] : 0u;
        }
    };
    // the planes go from L2 to LDS without a register stage (their count depends on T); padding rows: potential -inf
    // (every term exp2(-inf) = 0), coefficient 0
    auto commit_loads = [&](int buf, int t) __attribute__((always_inline)) {
        float *kt = smem + buf * TF;
        const int j0 = t * BW_KT;
#pragma unroll
        for (int e = 0; e < BW_LD_PER_THREAD; ++e) {
            int id = tid + e * BW_THREADS;
            int r = id >> 5, c = id & 31;
            float2 ev = {pre[e].x, pre[e].z}, od = {pre[e].y, pre[e].w};
            *(float2 *)(kt + r * BW_LDK + 2 * c) = ev;
            *(float2 *)(kt + r * BW_LDK + 64 + 2 * c) = od;
        }
        if (tid < BW_KT) kt[BW_KT * BW_LDK + tid] = pres;
        ((uint32_t *)kt)[BW_KT * BW_LDK + BW_KT + tid] = prem;
        for (int e = tid; e < K2 * BW_KT; e += BW_THREADS) {
            const int kk = e >> 6, j = j0 + (e & 63);
            kt[BW_FIXED_FLOATS + e] = j < Ni ? itab[(size_t)kk * Ni + j] : (kk <= T ? -INFINITY : 0.f);
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
            const float *arow = kt + (sub * 32 + r32) * BW_LDK + h * 64;
            f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int c = 0; c < 16; ++c) {
                f32x4 a = *(const f32x4 *)(arow + 4 * c);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, q[4 * c], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, q[4 * c + 1], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, q[4 * c + 2], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, q[4 * c + 3], acc, 0, 0, 0);
            }
            const float *sc = kt + BW_KT * BW_LDK + sub * 32 + 4 * h;   // this lane's 16 inner rows: (r&3) + 8*(r>>2) + 4*h
            const uint32_t *msk = (const uint32_t *)(kt + BW_KT * BW_LDK + BW_KT);
            const float *tb = kt + BW_FIXED_FLOATS + sub * 32 + 4 * h;   // plane kk of those rows: tb[kk * 64 + 8 * g + u]
            unsigned exact = 0;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x4 nb = *(const f32x4 *)(sc + 8 * g);
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int r = 4 * g + u;
                    acc[r] = (acc[r] + nrm_o) + nb[u];
                    exact |= (acc[r] < BW_TAU * (nrm_o + nb[u]) ? 1u : 0u) << r;
                }
            }
            if (__any(exact != 0)) {   // rare: redo v = |f_o - f_i|^2 from the difference where the expansion cancelled
#pragma unroll 1
                for (int r = 0; r < 16; ++r) {
                    if (!__any((exact >> r) & 1u)) continue;
                    const int er = sub * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                    const float *xr = kt + er * BW_LDK;
                    float v = 0.f;
#pragma unroll 4
                    for (int c = 0; c < BW_D / 4; ++c) {
                        const f32x4 o4 = *(const f32x4 *)(op + 4 * c);
                        const float2 ev = *(const float2 *)(xr + 2 * c), od = *(const float2 *)(xr + 64 + 2 * c);
                        const float d0 = ev.x - o4.x, d1 = od.x - o4.y, d2 = ev.y - o4.z, d3 = od.y - o4.w;
                        v = fmaf(d0, d0, v);
                        v = fmaf(d1, d1, v);
                        v = fmaf(d2, d2, v);
                        v = fmaf(d3, d3, v);
                    }
#pragma unroll
                    for (int rr = 0; rr < 16; ++rr)
                        if (rr == r && ((exact >> r) & 1u)) acc[rr] = v;
                }
            }
            // acc becomes D; w the sum of the entry's 2T + 1 terms
            float w[16];
            {   // the final row step's term, skipped on the row's top-k columns (prep / colgather own it there)
                const float po = to[(size_t)(grp == 0 ? 0 : T) * No];
                const float co = grp == 0 ? to[(size_t)(T + 1) * No] : 1.f;
                const float *pin = tb + (grp == 0 ? T : 0) * BW_KT;
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const f32x4 pi = *(const f32x4 *)(pin + 8 * g);
                    f32x4 ci = {1.f, 1.f, 1.f, 1.f};
                    if (grp == 1) ci = *(const f32x4 *)(tb + (T + 1) * BW_KT + 8 * g);
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int r = 4 * g + u;
                        const int il = (r & 3) + 8 * (r >> 2) + 4 * h;
                        const bool topk = grp == 0 ? ((msk[(wave * 32 + r32) * 2 + sub] >> il) & 1u)
                                                   : ((msk[(sub * 32 + il) * 4 + wave] >> r32) & 1u);
                        acc[r] = sqrt_rn(fmaxf(acc[r], 0.f));
                        const float e = __builtin_amdgcn_exp2f(fmaf(acc[r], a2, po + pi[u]));
                        w[r] = topk ? 0.f : (co * ci[u]) * e;
                    }
                }
            }
#pragma unroll 1
            for (int tt = 1; tt <= T; ++tt) {
                const float po = to[(size_t)tt * No];
                const float pox = grp == 0 ? po : to[(size_t)(tt - 1) * No];
                const float co = to[(size_t)(T + 1 + tt) * No];
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const f32x4 pi = *(const f32x4 *)(tb + tt * BW_KT + 8 * g);
                    f32x4 pix = pi;
                    if (grp == 0) pix = *(const f32x4 *)(tb + (tt - 1) * BW_KT + 8 * g);
                    const f32x4 ci = *(const f32x4 *)(tb + (T + 1 + tt) * BW_KT + 8 * g);
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
            // apply: out[o][pos] += sum_t W[t][o] * X[t][pos]; step r contracts t = (r&3)+8*(r>>2)+4*h
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int trow = sub * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                const f32x4 x = *(const f32x4 *)(kt + trow * BW_LDK + 4 * r32);
                acc2[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(w[r], x.x, acc2[0], 0, 0, 0);
                acc2[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(w[r], x.y, acc2[1], 0, 0, 0);
                acc2[2] = __builtin_amdgcn_mfma_f32_32x32x2f32(w[r], x.z, acc2[2], 0, 0, 0);
                acc2[3] = __builtin_amdgcn_mfma_f32_32x32x2f32(w[r], x.w, acc2[3], 0, 0, 0);
            }
        }
        if (t + 1 < ntiles) commit_loads(buf ^ 1, t + 1);
        __syncthreads();
    }

    // d_out[o] += (sum_t W[t][o]) * f_o - acc2[o]: this workgroup owns the rows, on top of the top-k slots' share
    const float rtot = rl + __shfl_xor(rl, 32, 64);
    if (h == 0) rsum[wave * 32 + r32] = rtot;
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int o = (r & 3) + 8 * (r >> 2) + 4 * h;
        const int row = ot * BW_OB + wave * 32 + o;
        if (row >= No) continue;
        const float rr = rsum[wave * 32 + o];
        const float *fo = G.fo + ((size_t)b * No + row) * BW_D;
        float *dst = G.dout + ((size_t)b * No + row) * BW_D;
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) {
            const int pos = 4 * r32 + cb;
            const int ch = pos < 64 ? 2 * pos : 2 * (pos - 64) + 1;
            dst[ch] += rr * fo[ch] - acc2[cb][r];
        }
    }
}

// scalar form: one wave per outer row, lanes own channels lane + 64u (softcorr_bwd_scalar_kernel's distances)
struct PBScalarArgs {
    const float *f1, *f2, *n1, *n2, *tabR, *tabC;
    float *df1, *df2;
    const uint32_t *topk_bits;
    int N, M, d, T, wpr;
    long rows0, rows_total;
    float a2, nalpha;
};

__global__ __launch_bounds__(256) void skb_apply_scalar_kernel(const PBScalarArgs args) {
    const int lane = threadIdx.x & 63;
    long gw = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (gw >= args.rows_total) return;
    const int grp = gw >= args.rows0 ? 1 : 0;
    gw -= grp ? args.rows0 : 0;
    const int N = args.N, M = args.M, d = args.d, T = args.T, K2 = 2 * (T + 1);
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
        float xv[8], part = 0.f;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int c = lane + 64 * u;
            xv[u] = c < d ? fi[c] : 0.f;
            part = fmaf(ov[u], xv[u], part);
        }
        const int ri = grp ? j : row, ci = grp ? row : j;   // the entry's f1 row and f2 row (column)
        const bool topk = (args.topk_bits[((size_t)b * N + ri) * args.wpr + (ci >> 5)] >> (ci & 31)) & 1u;
        const float dot = wave_sum(part);
        const float ni = nib[(size_t)b * Ni + j];
        float v = (-2.f * dot + nrm_o) + ni;
        if (v < BW_TAU * (nrm_o + ni)) {   // uniform: the expansion cancelled, redo v from the difference
            float p2 = 0.f;
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const float dd = ov[u] - xv[u];
                p2 = fmaf(dd, dd, p2);
            }
            v = wave_sum(p2);
        }
        v = fmaxf(v, 0.f);
        if (!(v > 0.f)) continue;
        const float D = sqrt_rn(v);
        float sum = topk ? 0.f : tr[(size_t)(T + 1) * N + ri] * exp2f(fmaf(D, args.a2, tr[ri] + tc[(size_t)T * M + ci]));
        for (int t = 1; t <= T; ++t) {
            const float pr = tr[(size_t)t * N + ri];
            sum = fmaf(tc[(size_t)(T + 1 + t) * M + ci], exp2f(fmaf(D, args.a2, pr + tc[(size_t)t * M + ci])), sum);
            sum = fmaf(tr[(size_t)(T + 1 + t) * N + ri], exp2f(fmaf(D, args.a2, pr + tc[(size_t)(t - 1) * M + ci])), sum);
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

struct SkbWs {
    float *n1, *n2, *G, *esp, *wsp, *ubar, *vbar, *tabR, *tabC;
    uint32_t *bits;
};
SkbWs skb_carve(Arena &ar, int B, int N, int M, int n_iter, int topk) {
    SkbWs w;
    const size_t T = (size_t)n_iter;
    w.n1 = ar.take<float>((size_t)B * N);
    w.n2 = ar.take<float>((size_t)B * M);
    w.G = ar.take<float>((size_t)B * N);
    w.esp = ar.take<float>((size_t)B * N * topk);
    w.wsp = ar.take<float>((size_t)B * N * topk);
    w.ubar = ar.take<float>((size_t)B * N * (T ? T : 1));
    w.vbar = ar.take<float>((size_t)B * M * (T ? T : 1));
    w.tabR = ar.take<float>((size_t)B * N * 2 * (T + 1));
    w.tabC = ar.take<float>((size_t)B * M * 2 * (T + 1));
    w.bits = ar.take<uint32_t>((size_t)B * N * ((M + 31) / 32));
    return w;
}

}  // namespace
}  // namespace dvm

using namespace dvm;

DVM_EXPORT size_t dvm_sinkhorn_bwd_workspace_bytes(int B, int N, int M, int d, int n_iter) {
    (void)d;
    if (B < 1 || N < 1 || M < 1 || n_iter < 0 || n_iter > SKB_MAX_ITER) return 0;
    Arena ar(nullptr, 0);
    (void)skb_carve(ar, B, N, M, n_iter, 16);
    return ar.off;
}

DVM_EXPORT int dvm_sinkhorn_bwd_f32(const float *f1, const float *f2, int B, int N, int M, int d, float neg_alpha, int n_iter, int topk,
                                    const float *pi_val, const int32_t *pi_idx, const float *u_hist, const float *v_hist,
                                    const float *g_val, float *d_f1, float *d_f2, int variant, void *ws, size_t ws_bytes, void *stream) {
    DVM_REQUIRE(f1 && f2 && pi_val && pi_idx && u_hist && v_hist && g_val && d_f1 && d_f2, "dvm_sinkhorn_bwd_f32: null pointer");
    DVM_REQUIRE(B >= 1 && N >= 1 && M >= 1, "dvm_sinkhorn_bwd_f32: empty input (B=%d N=%d M=%d)", B, N, M);
    DVM_REQUIRE(d >= 4 && d % 4 == 0 && d <= 512, "dvm_sinkhorn_bwd_f32: d=%d unsupported (need d%%4==0, 4<=d<=512)", d);
    DVM_REQUIRE(topk >= 1 && topk <= 16, "dvm_sinkhorn_bwd_f32: topk=%d unsupported (1..16)", topk);
    DVM_REQUIRE(n_iter >= 0 && n_iter <= SKB_MAX_ITER, "dvm_sinkhorn_bwd_f32: n_iter=%d unsupported (0..%d)", n_iter, SKB_MAX_ITER);
    DVM_REQUIRE(neg_alpha < 0.f, "dvm_sinkhorn_bwd_f32: neg_alpha must be negative (got %g)", (double)neg_alpha);
    DVM_REQUIRE(variant == 0 || variant == 1, "dvm_sinkhorn_bwd_f32: bad variant %d (0 = auto, 1 = scalar)", variant);
    Arena ar(ws, ws_bytes);
    const SkbWs w = skb_carve(ar, B, N, M, n_iter, topk);
    if (!ar.ok()) {
        set_error("dvm_sinkhorn_bwd_f32: workspace too small (%zu < %zu)", ws_bytes, ar.off);
        return DVM_ENOSPACE;
    }
    hipStream_t s = (hipStream_t)stream;
    const int T = n_iter, wpr = (M + 31) / 32;
    const bool mfma = variant == 0 && d == SK_D;
    const long u_bs = (long)(T + 1) * N, v_bs = (long)(T + 1) * M;
    (void)hipMemsetAsync(w.bits, 0, (size_t)B * N * wpr * sizeof(uint32_t), s);
    launch_rownorm2(f1, B * N, d, w.n1, s);
    launch_rownorm2(f2, B * M, d, w.n2, s);
    hipLaunchKernelGGL(skb_prep_kernel, dim3((unsigned)(((size_t)B * N + 3) / 4)), dim3(256), 0, s, f1, f2, pi_val, pi_idx, g_val, B, N, M, d,
                       topk, neg_alpha, w.G, w.esp, w.wsp, w.bits, d_f1);
    {
        const size_t lds = (size_t)(32 * d + 32) * sizeof(float);
        ensure_dyn_lds((const void *)skb_colgather_kernel, 66 * 1024);
        hipLaunchKernelGGL(skb_colgather_kernel, dim3(wpr, B), dim3(256), lds, s, f1, f2, pi_idx, w.esp, w.wsp, w.bits, N, M, d, topk, d_f2,
                           T ? w.vbar + (size_t)(T - 1) * M : nullptr, (long)T * M);
    }
    if (T) {
        const float c = (float)log((double)N / (double)M);
        SAArgs row{}, col{};
        row.q = f1, row.k = f2, row.nq = w.n1, row.nk = w.n2, row.N = N, row.M = M, row.d = d, row.neg_alpha = neg_alpha;
        col.q = f2, col.k = f1, col.nq = w.n2, col.nk = w.n1, col.N = M, col.M = N, col.d = d, col.neg_alpha = neg_alpha;
        row.potq_bs = u_bs, row.potk_bs = v_bs, row.coefk_bs = (long)T * M, row.out_bs = (long)T * N, row.add = -c;
        col.potq_bs = v_bs, col.potk_bs = u_bs, col.out_bs = (long)T * M, col.add = 0.f;
        // vbar^T_j = [colgather: the top-k slots] - sum_i G_i P_ij over the other entries
        col.potq = v_hist + (size_t)T * M, col.potk = u_hist + (size_t)T * N, col.coefk = w.G, col.coefk_bs = N;
        col.out = w.vbar + (size_t)(T - 1) * M, col.bits = w.bits, col.wpr = wpr;
        launch_sweep_t<true, true>(mfma, col, B, s);
        col.bits = nullptr, col.coefk_bs = (long)T * N;
        for (int t = T; t >= 1; --t) {
            row.potq = u_hist + (size_t)(t - 1) * N, row.potk = v_hist + (size_t)t * M, row.coefk = w.vbar + (size_t)(t - 1) * M;
            row.out = w.ubar + (size_t)(t - 1) * N;
            launch_sweep_t<false, false>(mfma, row, B, s);   // ubar^t = -sum_j vbar^t_j Q^t_ij
            if (t > 1) {
                col.potq = v_hist + (size_t)(t - 1) * M, col.potk = u_hist + (size_t)(t - 1) * N, col.coefk = w.ubar + (size_t)(t - 1) * N;
                col.out = w.vbar + (size_t)(t - 2) * M;
                launch_sweep_t<true, false>(mfma, col, B, s);   // vbar^(t-1) = -sum_i ubar^t_i R^t_ij
            }
        }
    }
    hipLaunchKernelGGL(skb_pack_kernel, dim3((std::max(N, M) + 255) / 256, T + 1, B), dim3(256), 0, s, u_hist, v_hist, w.G, w.ubar, w.vbar, N,
                       M, T, (float)((double)M / (double)N), w.tabR, w.tabC);
    const float a2 = neg_alpha * LOG2E;
    if (mfma) {
        PBArgs a;
        a.g[0] = PBGroup{f1, f2, w.n1, w.n2, w.tabR, w.tabC, d_f1, N, M, (N + BW_OB - 1) / BW_OB};
        a.g[1] = PBGroup{f2, f1, w.n2, w.n1, w.tabC, w.tabR, d_f2, M, N, (M + BW_OB - 1) / BW_OB};
        a.topk_bits = w.bits, a.wpr = wpr, a.T = T, a.a2 = a2, a.nalpha = -neg_alpha;
        a.tile_floats = BW_FIXED_FLOATS + 2 * (T + 1) * BW_KT;
        const size_t lds = ((size_t)2 * a.tile_floats + BW_OB) * sizeof(float);
        const int lds_max = (int)(((size_t)2 * (BW_FIXED_FLOATS + 2 * (SKB_MAX_ITER + 1) * BW_KT) + BW_OB) * sizeof(float));
        ensure_dyn_lds((const void *)skb_apply_mfma_kernel<0>, lds_max);
        ensure_dyn_lds((const void *)skb_apply_mfma_kernel<1>, lds_max);
        hipLaunchKernelGGL(skb_apply_mfma_kernel<0>, dim3(B * a.g[0].tiles_o), dim3(BW_THREADS), lds, s, a);
        hipLaunchKernelGGL(skb_apply_mfma_kernel<1>, dim3(B * a.g[1].tiles_o), dim3(BW_THREADS), lds, s, a);
    } else {
        PBScalarArgs a;
        a.f1 = f1, a.f2 = f2, a.n1 = w.n1, a.n2 = w.n2, a.tabR = w.tabR, a.tabC = w.tabC, a.df1 = d_f1, a.df2 = d_f2;
        a.topk_bits = w.bits, a.N = N, a.M = M, a.d = d, a.T = T, a.wpr = wpr, a.a2 = a2, a.nalpha = -neg_alpha;
        a.rows0 = (long)B * N, a.rows_total = (long)B * N + (long)B * M;
        hipLaunchKernelGGL(skb_apply_scalar_kernel, dim3((unsigned)((a.rows_total + 3) / 4)), dim3(256), 0, s, a);
    }
    DVM_CHECK_LAUNCH("sinkhorn_bwd");
    return DVM_OK;
}
