// dvm_cycle.hip — the cycle term ||P12 P21 - I_N||_F of the two sparse top-k correspondences of a pair, P12 (val12 / idx12
// [B,N,k12], M columns) and P21 (val21 / idx21 [B,M,k21], N columns), and its gradients in val12 and val21 (not in the reference,
// whose loss terms each look at one direction).
//
// With C = P12 P21 (N x N, at most k12 k21 non-zeros per row) and R = C - I:   F^2 = sum_i sum_c R[i,c]^2,
//   dF / d val12[i,t] = (1/F) sum_s R[i, idx21[j,s]] val21[j,s],  j = idx12[i,t]              (row i's own residuals)
//   dF / d val21[j,s] = (1/F) sum_{(i,t): idx12[i,t] = j} val12[i,t] R[i, idx21[j,s]]         (one residual of every row that picks j)
// cycle_row_kernel, one workgroup per row i, 256 threads = 16 slots t x 16 slots s, thread (t, s) owning the product
// val12[i,t] val21[j,s] at column c = idx21[j,s]:
//   1. row i of C in LDS (N fp32 words): slot t = 0..k12-1 in turn, a barrier between them, thread (t, s) adds its product into C[c].
//      The columns of one row of P21 are distinct, so no two threads touch one word: no LDS atomics, C[c] takes its (at most k12)
//      terms in slot order.
//   2. sum_c (C[c] - delta_ic)^2 in float64, thread x over c = x, x + 256, .., then the fixed tree -> partial[b][i].
//   3. gradient (GRAD): thread (t, s) reads C[c] back: the sample smp[b][i][t][s] (what the column kernel needs from this row) and
//      the term R[i,c] val21[j,s]; thread t < k12 adds its k21 terms in slot order in float64 -> g12[i,t], unscaled.
// cycle_col_kernel, one wave per column j of P12 = row j of P21, lanes = 4 list entries x 16 slots s: the list of j from
// launch_rev_csr (dvm_revlist.hip) is walked twice for the order-free sum that dvm_frob.h explains: the largest |term| per slot s,
// then the 64-bit integer sum -> g21[j,s], unscaled; 0 for a column nobody picks.
// frob_finish (dvm_frob.hip): loss = sqrt(F^2), g12 and g21 *= 1 / F, 0 where F == 0.
// The loss-only call runs steps 1 and 2 and the finish: no lists, no samples.  Arrays: the lists (B (2 M + 1 + N k12) int32),
// B N doubles, B floats, the samples (B N k12 k21 floats).
#include "dvm_frob.h"

namespace dvm {

static_assert(FROB_THREADS == 16 * 16, "cycle_row_kernel: one thread per (t, s) pair");

template <bool GRAD>
__global__ __launch_bounds__(FROB_THREADS) void cycle_row_kernel(const float *__restrict__ val12, const int32_t *__restrict__ idx12,
                                                                  const float *__restrict__ val21, const int32_t *__restrict__ idx21, int N,
                                                                  int M, int k12, int k21, double *__restrict__ partial,
                                                                  float *__restrict__ g12, float *__restrict__ smp) {
    extern __shared__ float cycle_lds[];   // C [N]
    __shared__ double gterm[FROB_THREADS];
    float *C = cycle_lds;
    const int tid = threadIdx.x, i = blockIdx.x, b = blockIdx.y;
    const int t = tid >> 4, s = tid & 15;
    const size_t row12 = ((size_t)b * N + i) * k12;
    // an index outside its range leaves c = -1: the pair contributes nothing and never becomes an address
    float v = 0.f, w = 0.f;
    int c = -1;
    if (t < k12 && s < k21) {
        const int j = idx12[row12 + t];
        if (j >= 0 && j < M) {
            const size_t e21 = ((size_t)b * M + j) * k21 + s;
            const int cc = idx21[e21];
            v = val12[row12 + t];
            w = val21[e21];
            if (cc >= 0 && cc < N) c = cc;
        }
    }
    for (int r = tid; r < N; r += FROB_THREADS) C[r] = 0.f;
    __syncthreads();
    for (int u = 0; u < k12; ++u) {
        // a value of 0 adds nothing; skipping it also keeps the repeated (0, 0) slots of a row with fewer columns than topk off one word
        if (t == u && c >= 0 && v != 0.f && w != 0.f) C[c] = fmaf(v, w, C[c]);
        __syncthreads();
    }
    const double acc = frob_row_sq_sum(C, N, i);
    if (tid == 0) partial[(size_t)b * N + i] = acc;
    if (!GRAD) return;
    const float cs = c >= 0 ? C[c] : 0.f;
    if (t < k12 && s < k21) smp[(row12 + t) * k21 + s] = cs;
    gterm[tid] = c >= 0 ? resid_term(cs, c == i, w) : 0.0;
    __syncthreads();
    if (tid < k12) {
        double g = 0.0;
        for (int q = 0; q < k21; ++q) g += gterm[tid * 16 + q];
        g12[row12 + tid] = (float)g;
    }
}

// g21[j,s] = sum over the list of column j (entries e = i * k12 + t with idx12[e] == j) of val12[e] (smp[e][s] - delta(i, idx21[j,s])), unscaled
__global__ __launch_bounds__(FROB_THREADS) void cycle_col_kernel(const float *__restrict__ val12, const int32_t *__restrict__ idx21,
                                                                  const int32_t *__restrict__ offs, const int32_t *__restrict__ edges,
                                                                  const float *__restrict__ smp, int N, int M, int k12, int k21,
                                                                  float *__restrict__ g21) {
    const int lane = threadIdx.x & (WAVE - 1), b = blockIdx.y;
    const long jl = (long)blockIdx.x * (FROB_THREADS / WAVE) + threadIdx.x / WAVE;
    if (jl >= M) return;   // whole waves leave; the kernel has no barrier
    const int j = (int)jl, s = lane & 15, sub = lane >> 4;
    const size_t E12 = (size_t)N * k12, row21 = ((size_t)b * M + j) * k21;
    const float *vb = val12 + (size_t)b * E12;
    const float *sb = smp + (size_t)b * E12 * k21;
    const int32_t *ed = edges + (size_t)b * E12;
    int c = -1;
    if (s < k21) {
        const int cc = idx21[row21 + s];
        if (cc >= 0 && cc < N) c = cc;
    }
    const int beg = offs[(size_t)b * (M + 1) + j], end = offs[(size_t)b * (M + 1) + j + 1];
    double mx = 0.0;
    if (c >= 0)
        for (int e = beg + sub; e < end; e += 4) {
            const int en = ed[e];   // entry number = row * k12 + slot, < N * k12 by construction of the lists
            mx = fmax(mx, fabs(resid_term(sb[(size_t)en * k21 + s], en / k12 == c, vb[en])));
        }
    mx = fmax(mx, __shfl_xor(mx, 16, 64));
    mx = fmax(mx, __shfl_xor(mx, 32, 64));
    const int ue = fix_unit_exp(mx);
    long long Q = 0;
    if (c >= 0)
        for (int e = beg + sub; e < end; e += 4) {
            const int en = ed[e];
            Q += fix_quant(resid_term(sb[(size_t)en * k21 + s], en / k12 == c, vb[en]), ue);
        }
    Q += __shfl_xor(Q, 16, 64);
    Q += __shfl_xor(Q, 32, 64);
    if (sub == 0 && s < k21) g21[row21 + s] = (float)fix_value(Q, ue);
}

}  // namespace dvm

using namespace dvm;

struct CycleWs {
    RevLists rev;    // the reversed lists of idx12 over the M columns
    FrobSums sums;
    float *smp;      // [B][N][k12][k21]: C[i, idx21[idx12[i,t], s]]
};
static size_t carve_cycle(Arena &ar, int B, int N, int M, int k12, int k21, CycleWs &w) {
    w.rev.take(ar, B, M, (size_t)N * k12);
    w.sums.take(ar, B, N);
    w.smp = ar.take<float>((size_t)B * N * k12 * k21);
    return ar.off;
}
// the row of C takes N fp32 words of LDS (32 KB at the limit), as the rank term's row
static const char *cycle_limits(int B, int N, int M, int k12, int k21) {
    const char *who = "dvm_cycle_term_f32";
    FROB_BATCH_LIMITS(who, B, N, M);
    FROB_TOPK_LIMIT(who, k12);
    FROB_TOPK_LIMIT(who, k21);
    FROB_LIMIT(N <= FROB_MAX_N, "%s: N=%d unsupported (a row of P12 P21 must fit LDS: N <= %d)", who, N, FROB_MAX_N);
    return nullptr;
}

DVM_EXPORT int dvm_cycle_term_max_n(void) { return FROB_MAX_N; }

DVM_EXPORT size_t dvm_cycle_term_workspace_bytes(int B, int N, int M, int k12, int k21) {
    return cycle_limits(B, N, M, k12, k21) ? 0 : null_carve<CycleWs>(carve_cycle, B, N, M, k12, k21);
}

DVM_EXPORT int dvm_cycle_term_f32(const float *val12, const int32_t *idx12, const float *val21, const int32_t *idx21, int B, int N, int M,
                                  int k12, int k21, float *loss, float *g12, float *g21, void *ws, size_t ws_bytes, void *stream) {
    DVM_REQUIRE(val12 && idx12 && val21 && idx21 && loss, "dvm_cycle_term_f32: null pointer");
    const char *why = cycle_limits(B, N, M, k12, k21);
    DVM_REQUIRE(!why, "%s", why);
    DVM_REQUIRE((g12 == nullptr) == (g21 == nullptr), "dvm_cycle_term_f32: g12 and g21 must both be NULL or both be given");
    CycleWs w;
    if (!carve_ws(ws, ws_bytes, "dvm_cycle_term_f32", w, carve_cycle, B, N, M, k12, k21)) return DVM_ENOSPACE;
    hipStream_t s = (hipStream_t)stream;
    const size_t lds = (size_t)N * sizeof(float);
    const dim3 grid(N, B), block(FROB_THREADS);
    if (!g12) {
        hipLaunchKernelGGL(cycle_row_kernel<false>, grid, block, lds, s, val12, idx12, val21, idx21, N, M, k12, k21, w.sums.partial, g12, w.smp);
    } else {
        launch_rev_csr(idx12, B, (long)N * k12, M, w.rev, s);
        hipLaunchKernelGGL(cycle_row_kernel<true>, grid, block, lds, s, val12, idx12, val21, idx21, N, M, k12, k21, w.sums.partial, g12, w.smp);
        const dim3 cgrid((unsigned)(((long)M + FROB_THREADS / WAVE - 1) / (FROB_THREADS / WAVE)), B);
        hipLaunchKernelGGL(cycle_col_kernel, cgrid, block, 0, s, val12, idx21, w.rev.offs, w.rev.edges, w.smp, N, M, k12, k21, g21);
    }
    return frob_finish(w.sums, B, N, 1.0, loss, {{g12, (size_t)N * k12}, {g21, (size_t)M * k21}}, "cycle_term", s);
}
