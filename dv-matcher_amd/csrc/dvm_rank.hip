// dvm_rank.hip — the rank term ||P P^T - I_N||_F of a sparse top-k correspondence P (pi_val / pi_idx [B,N,topk], M columns) and its
// gradient in pi_val (models/loss.py:1427-1433 of the reference, which forms the dense N x N product).
//
// Row form: with S = P P^T,   F^2 = sum_i [ (S_ii - 1)^2 + sum_{i' != i} S_ii'^2 ]  — every term non-negative, nothing cancels, and
// row i of S is non-zero only at rows i' that share a column with row i.  The entries of every column come from the reversed lists
// of launch_rev_csr (dvm_geom.hip).  One workgroup per row i:
//   1. row i of S in LDS (N fp32 words): for slot t = 0..topk-1 in turn, walk the list of column pi_idx[i,t] and add
//      pi_val[i,t] * val(e) into S[row(e)].  The rows of one column are distinct and a barrier separates the slots, so no two threads
//      touch one word: no LDS atomics, and S[i'] takes its (at most topk) terms in slot order whatever the order of the lists.
//   2. sum_i' (S_ii' - delta_ii')^2 in float64, thread x over i' = x, x + 256, .., then the fixed tree -> partial[b][i].
//   3. gradient (GRAD): dF^2 / d pi_val[i,t] = 4 sum_{e in column pi_idx[i,t]} (S - I)[i, row(e)] val(e), two more walks of the same
//      lists.  Their order is that of rev_fill_kernel's integer atomics, and a floating-point sum would carry it into the result's
//      last bits.  So the sum is formed in fixed point, which no order can change: a first walk takes the largest |term| m of every
//      slot's list (a maximum does not depend on the order either), a second one adds the terms as 64-bit integers in units of
//      2^(ilogb(m) + 1 - 50) — every term below 2^50, a list holds at most N <= 2^13 of them.  The quantisation, at most
//      N 2^-50 m, is far below one fp32 rounding of the result's own terms.  The same bits from run to run, alone or in a batch.
// rank_finish_kernel: loss = sqrt(F^2) and g_val *= 1 / (2 loss), 0 where loss == 0 (an exact permutation: torch.norm's subgradient).
// No float atomics anywhere; arrays: the lists (B (2 M + 1 + N topk) int32), B N doubles, B floats.
#include "dvm_common.h"

namespace dvm {

constexpr int RANK_MAX_N = 8192;    // the criterion's own gate; the row of S takes N fp32 words of LDS (32 KB at the limit)
constexpr int RANK_THREADS = 256;   // block_tree_sum's width

// fix_unit_exp of the largest |term| of slot t (the maximum over the workgroup's waves): every term of the slot is below 2^that
__device__ __forceinline__ int rank_unit_exp(const double (*gmax)[16], int t) {
    double m = gmax[0][t];
    for (int w = 1; w < RANK_THREADS / WAVE; ++w) m = fmax(m, gmax[w][t]);
    return fix_unit_exp(m);
}

template <int K, bool GRAD>
__global__ __launch_bounds__(RANK_THREADS) void rank_row_kernel(const float *__restrict__ pi_val, const int32_t *__restrict__ pi_idx,
                                                                const int32_t *__restrict__ offs, const int32_t *__restrict__ edges,
                                                                int N, int M, int topk, double *__restrict__ partial,
                                                                float *__restrict__ g_val) {
    extern __shared__ float rank_lds[];   // S [N]
    __shared__ int sbeg[16], send[16];
    __shared__ float sval[16];
    __shared__ double gmax[RANK_THREADS / WAVE][16];
    __shared__ long long qred[RANK_THREADS / WAVE][16];
    float *S = rank_lds;
    const int tid = threadIdx.x, i = blockIdx.x, b = blockIdx.y;
    const size_t E = (size_t)N * topk;
    const float *vb = pi_val + (size_t)b * E;
    const int32_t *ib = pi_idx + (size_t)b * E;
    const int32_t *ed = edges + (size_t)b * E;
    if (tid < 16) {
        int j = -1;
        if (tid < topk) j = ib[(size_t)i * topk + tid];
        const bool ok = j >= 0 && j < M;   // an index outside [0, M) is in no list: the slot contributes nothing
        sbeg[tid] = ok ? offs[(size_t)b * (M + 1) + j] : 0;
        send[tid] = ok ? offs[(size_t)b * (M + 1) + j + 1] : 0;
        sval[tid] = tid < topk ? vb[(size_t)i * topk + tid] : 0.f;
    }
    for (int r = tid; r < N; r += RANK_THREADS) S[r] = 0.f;
    __syncthreads();
    for (int t = 0; t < topk; ++t) {
        const float v = sval[t];
        const int end = send[t];
        for (int e = sbeg[t] + tid; e < end; e += RANK_THREADS) {
            const int en = ed[e];        // entry number = row * topk + slot, < N * topk by construction of the lists
            const float w = vb[en];
            // a value of 0 adds nothing; skipping it also keeps the repeated (0, 0) slots of a row with M < topk off one word
            if (w != 0.f) {
                const int r = en / topk;
                S[r] = fmaf(v, w, S[r]);
            }
        }
        __syncthreads();
    }
    double acc = 0.0;
    for (int r = tid; r < N; r += RANK_THREADS) {
        const double x = (double)S[r] - (r == i ? 1.0 : 0.0);
        acc += x * x;
    }
    acc = block_tree_sum(acc);
    if (tid == 0) partial[(size_t)b * N + i] = acc;
    if (!GRAD) return;
    const int lane = tid & (WAVE - 1), wave = tid / WAVE;
    double mx[K];
#pragma unroll
    for (int t = 0; t < K; ++t) {
        mx[t] = 0.0;
        if (t < topk) {
            const int end = send[t];
            for (int e = sbeg[t] + tid; e < end; e += RANK_THREADS) {
                const int en = ed[e], r = en / topk;
                mx[t] = fmax(mx[t], fabs(resid_term(S[r], r == i, vb[en])));
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) mx[t] = fmax(mx[t], __shfl_xor(mx[t], o, 64));
        if (lane == 0) gmax[wave][t] = mx[t];
    }
    __syncthreads();
    long long Q[K];
#pragma unroll
    for (int t = 0; t < K; ++t) {
        Q[t] = 0;
        if (t < topk) {
            const int ue = rank_unit_exp(gmax, t);
            const int end = send[t];
            for (int e = sbeg[t] + tid; e < end; e += RANK_THREADS) {
                const int en = ed[e], r = en / topk;
                Q[t] += fix_quant(resid_term(S[r], r == i, vb[en]), ue);
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) Q[t] += __shfl_xor(Q[t], o, 64);
        if (lane == 0) qred[wave][t] = Q[t];
    }
    __syncthreads();
    if (tid < topk) {
        long long q = 0;
        for (int w = 0; w < RANK_THREADS / WAVE; ++w) q += qred[w][tid];
        g_val[(size_t)b * E + (size_t)i * topk + tid] = (float)(4.0 * fix_value(q, rank_unit_exp(gmax, tid)));
    }
}

// f2 [B] = F^2 -> loss [B] = F; g_val [B][E] *= num / F, 0 where F == 0 (num = 1/2: g_val = dF^2 / d pi_val -> dF / d pi_val)
__global__ void rank_finish_kernel(const float *__restrict__ f2, size_t E, double num, float *__restrict__ loss, float *__restrict__ g_val) {
    const int b = blockIdx.y;
    const double F = sqrt((double)f2[b]);
    if (blockIdx.x == 0 && threadIdx.x == 0) loss[b] = (float)F;
    if (g_val == nullptr) return;
    const double sc = F > 0.0 ? num / F : 0.0;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < E; e += (size_t)gridDim.x * blockDim.x)
        g_val[(size_t)b * E + e] = (float)((double)g_val[(size_t)b * E + e] * sc);
}

void launch_frob_finish(const float *f2, int B, size_t E, double num, float *loss, float *g_val, hipStream_t s) {
    const unsigned fblocks = g_val ? (unsigned)((E + 1023) / 1024) : 1u;
    hipLaunchKernelGGL(rank_finish_kernel, dim3(fblocks, B), dim3(256), 0, s, f2, E, num, loss, g_val);
}

}  // namespace dvm

using namespace dvm;

struct RankWs {
    int32_t *offs, *cursor, *edges;   // the reversed lists of launch_rev_csr
    double *partial;                  // [B][N]: one per row
    float *f2;                        // [B]
};
static size_t carve_rank(Arena &ar, int B, int N, int M, int topk, RankWs &w) {
    w.offs = ar.take<int32_t>((size_t)B * (M + 1));
    w.cursor = ar.take<int32_t>((size_t)B * M);
    w.edges = ar.take<int32_t>((size_t)B * N * topk);
    w.partial = ar.take<double>((size_t)B * N);
    w.f2 = ar.take<float>((size_t)B);
    return ar.off;
}
static bool rank_shape_ok(int B, int N, int M, int topk) {
    return B >= 1 && B <= 65535 && N >= 1 && N <= RANK_MAX_N && M >= 1 && topk >= 1 && topk <= 16;
}

DVM_EXPORT int dvm_rank_term_max_n(void) { return RANK_MAX_N; }

DVM_EXPORT size_t dvm_rank_term_workspace_bytes(int B, int N, int M, int topk) {
    return rank_shape_ok(B, N, M, topk) ? null_carve<RankWs>(carve_rank, B, N, M, topk) : 0;
}

DVM_EXPORT int dvm_rank_term_f32(const float *pi_val, const int32_t *pi_idx, int B, int N, int M, int topk, float *loss, float *g_val,
                                 void *ws, size_t ws_bytes, void *stream) {
    DVM_REQUIRE(pi_val && pi_idx && loss, "dvm_rank_term_f32: null pointer");
    DVM_REQUIRE(B >= 1 && N >= 1 && M >= 1, "dvm_rank_term_f32: empty input (B=%d N=%d M=%d)", B, N, M);
    DVM_REQUIRE(B <= 65535, "dvm_rank_term_f32: B=%d unsupported (<= 65535)", B);
    DVM_REQUIRE(topk >= 1 && topk <= 16, "dvm_rank_term_f32: topk=%d unsupported (1..16)", topk);
    DVM_REQUIRE(N <= RANK_MAX_N, "dvm_rank_term_f32: N=%d unsupported (a row of P P^T must fit LDS: N <= %d)", N, RANK_MAX_N);
    RankWs w;
    if (!carve_ws(ws, ws_bytes, "dvm_rank_term_f32", w, carve_rank, B, N, M, topk)) return DVM_ENOSPACE;
    hipStream_t s = (hipStream_t)stream;
    const size_t E = (size_t)N * topk;
    launch_rev_csr(pi_idx, B, (long)E, M, w.offs, w.cursor, w.edges, s);
    const size_t lds = (size_t)N * sizeof(float);
    const dim3 grid(N, B), block(RANK_THREADS);
#define RANK_LAUNCH(K, GRAD) \
    hipLaunchKernelGGL((rank_row_kernel<K, GRAD>), grid, block, lds, s, pi_val, pi_idx, w.offs, w.edges, N, M, topk, w.partial, g_val)
    if (!g_val)
        RANK_LAUNCH(1, false);
    else if (topk <= 10)
        RANK_LAUNCH(10, true);
    else
        RANK_LAUNCH(16, true);
#undef RANK_LAUNCH
    launch_reduce_partials(w.partial, B, N, 1.f, w.f2, 1, 0, s);
    launch_frob_finish(w.f2, B, E, 0.5, loss, g_val, s);
    DVM_CHECK_LAUNCH("rank_term");
    return DVM_OK;
}
