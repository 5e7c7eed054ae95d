// dvm_rank.hip — the rank term ||P P^T - I_N||_F of a sparse top-k correspondence P (pi_val / pi_idx [B,N,topk], M columns) and its
// gradient in pi_val (models/loss.py:1427-1433 of the reference, which forms the dense N x N product).
//
// Row form: with S = P P^T,   F^2 = sum_i [ (S_ii - 1)^2 + sum_{i' != i} S_ii'^2 ]  — every term non-negative, nothing cancels, and
// row i of S is non-zero only at rows i' that share a column with row i.  The entries of every column come from the reversed lists
// of launch_rev_csr (dvm_revlist.hip).  One workgroup per row i:
//   1. row i of S in LDS (N fp32 words): for slot t = 0..topk-1 in turn, walk the list of column pi_idx[i,t] and add
//      pi_val[i,t] * val(e) into S[row(e)].  The rows of one column are distinct and a barrier separates the slots, so no two threads
//      touch one word: no LDS atomics, and S[i'] takes its (at most topk) terms in slot order whatever the order of the lists.
//   2. sum_i' (S_ii' - delta_ii')^2 in float64, thread x over i' = x, x + 256, .., then the fixed tree -> partial[b][i].
//   3. gradient (GRAD): dF^2 / d pi_val[i,t] = 4 sum_{e in column pi_idx[i,t]} (S - I)[i, row(e)] val(e), two more walks of the same
//      lists.  Their order is that of rev_fill_kernel's integer atomics, so the sum is formed in the order-free fixed point that
//      dvm_frob.h explains: a first walk takes the largest |term| of every slot's list, a second one adds the terms as integers.
// frob_finish (dvm_frob.hip): loss = sqrt(F^2) and g_val *= 1 / (2 loss), 0 where loss == 0 (an exact permutation).
// Arrays: the lists (B (2 M + 1 + N topk) int32), B N doubles, B floats.
#include "dvm_frob.h"

namespace dvm {

// fix_unit_exp of the largest |term| of slot t (the maximum over the workgroup's waves): every term of the slot is below 2^that
__device__ __forceinline__ int rank_unit_exp(const double (*gmax)[16], int t) {
    double m = gmax[0][t];
    for (int w = 1; w < FROB_THREADS / WAVE; ++w) m = fmax(m, gmax[w][t]);
    return fix_unit_exp(m);
}

template <int K, bool GRAD>
__global__ __launch_bounds__(FROB_THREADS) void rank_row_kernel(const float *__restrict__ pi_val, const int32_t *__restrict__ pi_idx,
                                                                const int32_t *__restrict__ offs, const int32_t *__restrict__ edges,
                                                                int N, int M, int topk, double *__restrict__ partial,
                                                                float *__restrict__ g_val) {
    extern __shared__ float rank_lds[];   // S [N]
    __shared__ int sbeg[16], send[16];
    __shared__ float sval[16];
    __shared__ double gmax[FROB_THREADS / WAVE][16];
    __shared__ long long qred[FROB_THREADS / WAVE][16];
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
    for (int r = tid; r < N; r += FROB_THREADS) S[r] = 0.f;
    __syncthreads();
    for (int t = 0; t < topk; ++t) {
        const float v = sval[t];
        const int end = send[t];
        for (int e = sbeg[t] + tid; e < end; e += FROB_THREADS) {
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
    const double acc = frob_row_sq_sum(S, N, i);
    if (tid == 0) partial[(size_t)b * N + i] = acc;
    if (!GRAD) return;
    const int lane = tid & (WAVE - 1), wave = tid / WAVE;
    double mx[K];
#pragma unroll
    for (int t = 0; t < K; ++t) {
        mx[t] = 0.0;
        if (t < topk) {
            const int end = send[t];
            for (int e = sbeg[t] + tid; e < end; e += FROB_THREADS) {
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
            for (int e = sbeg[t] + tid; e < end; e += FROB_THREADS) {
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
        for (int w = 0; w < FROB_THREADS / WAVE; ++w) q += qred[w][tid];
        g_val[(size_t)b * E + (size_t)i * topk + tid] = (float)(4.0 * fix_value(q, rank_unit_exp(gmax, tid)));
    }
}

}  // namespace dvm

using namespace dvm;

struct RankWs {
    RevLists rev;    // the reversed lists of pi_idx over the M columns
    FrobSums sums;
};
static size_t carve_rank(Arena &ar, int B, int N, int M, int topk, RankWs &w) {
    w.rev.take(ar, B, M, (size_t)N * topk);
    w.sums.take(ar, B, N);
    return ar.off;
}
// the criterion's own gate: the row of S takes N fp32 words of LDS (32 KB at the limit)
static const char *rank_limits(int B, int N, int M, int topk) {
    const char *who = "dvm_rank_term_f32";
    FROB_BATCH_LIMITS(who, B, N, M);
    FROB_TOPK_LIMIT(who, topk);
    FROB_LIMIT(N <= FROB_MAX_N, "%s: N=%d unsupported (a row of P P^T must fit LDS: N <= %d)", who, N, FROB_MAX_N);
    return nullptr;
}

DVM_EXPORT int dvm_rank_term_max_n(void) { return FROB_MAX_N; }

DVM_EXPORT size_t dvm_rank_term_workspace_bytes(int B, int N, int M, int topk) {
    return rank_limits(B, N, M, topk) ? 0 : null_carve<RankWs>(carve_rank, B, N, M, topk);
}

DVM_EXPORT int dvm_rank_term_f32(const float *pi_val, const int32_t *pi_idx, int B, int N, int M, int topk, float *loss, float *g_val,
                                 void *ws, size_t ws_bytes, void *stream) {
    DVM_REQUIRE(pi_val && pi_idx && loss, "dvm_rank_term_f32: null pointer");
    const char *why = rank_limits(B, N, M, topk);
    DVM_REQUIRE(!why, "%s", why);
    RankWs w;
    if (!carve_ws(ws, ws_bytes, "dvm_rank_term_f32", w, carve_rank, B, N, M, topk)) return DVM_ENOSPACE;
    hipStream_t s = (hipStream_t)stream;
    const size_t E = (size_t)N * topk;
    launch_rev_csr(pi_idx, B, (long)E, M, w.rev, s);
    const size_t lds = (size_t)N * sizeof(float);
    const dim3 grid(N, B), block(FROB_THREADS);
#define RANK_LAUNCH(K, GRAD) \
    hipLaunchKernelGGL((rank_row_kernel<K, GRAD>), grid, block, lds, s, pi_val, pi_idx, w.rev.offs, w.rev.edges, N, M, topk, w.sums.partial, g_val)
    if (!g_val)
        RANK_LAUNCH(1, false);
    else if (topk <= 10)
        RANK_LAUNCH(10, true);
    else
        RANK_LAUNCH(16, true);
#undef RANK_LAUNCH
    return frob_finish(w.sums, B, N, 0.5, loss, {{g_val, E}}, "rank_term", s);
}
