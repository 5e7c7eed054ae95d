// dvm_distortion.hip — the geodesic distortion term ||P D2 P^T - D1||_F of a sparse top-k correspondence P (pi_val / pi_idx
// [B,N,topk], M columns) between a source shape with distance matrix D1 [N,N] and a target shape with D2 [M,M], both symmetric, and
// its gradient in pi_val (not in the reference, which uses the two matrices only for its anchor-sampled cosine).
//
// With S = P D2 P^T (N x N), R = S - D1 and F = ||R||_F:   S[i,j] = sum_s val[j,s] u_i[idx[j,s]],   u_i = D2 P[i,:]^T,
//   dF / d val[i,t] = (2/F) sum_m D2[c,m] q_i[m],   c = idx[i,t],   q_i = P^T R[i,:]   (q_i[m] = sum_{(j,s): idx[j,s] = m} val[j,s] R[i,j])
// — S and R are symmetric, so the row-role and the column-role half of the derivative are equal: the factor 2, and no term from
// another row.  distortion_row_kernel, one workgroup of 256 threads per row i:
//   1. u_i in LDS (M fp32 words): u_i[m] = sum_t val[i,t] D2[idx[i,t], m], topk coalesced row reads of D2, an fmaf chain in slot
//      order.
//   2. the residual row: thread x takes j = x, x + 256, ..: S[i,j] = topk gathers from u_i, an fmaf chain in slot order;
//      r = (double)S - (double)D1[i,j] (the coalesced row of D1), kept in LDS as fp32 (GRAD), sum r^2 in float64 through the fixed
//      tree -> partial[b][i].
//   3. gradient (GRAD): q_i[m] in LDS.  Its terms val[j,s] r[j] arrive by column in no particular order, so they are added in
//      the order-free 64-bit fixed point that dvm_frob.h explains: a first sweep over P takes the largest |term| of every column (an LDS
//      integer maximum on the fp32 bit pattern), a second one adds the float64 terms as integers in units of 2^-50 of that
//      maximum's binade (an LDS 64-bit integer add).  Integer maximum and integer sum commute, so no order can reach the result,
//      and the reversed lists of the rank and cycle terms are not needed.  q_i takes u_i's place.  Then topk more coalesced row
//      reads of D2, each dotted with q_i in float64 (the butterfly of a wave, the four waves added in order) -> g[i,t], unscaled.
// frob_finish (dvm_frob.hip): loss = sqrt(F^2), g *= 2 / F, 0 where F == 0.
// The loss-only call runs steps 1 and 2 and the finish.  Arrays: B N doubles, B floats.
// A workgroup that owns a tile of 2 or 4 rows sharing every sweep over P was measured and is not kept: with gradients it is slower
// (profiles/notes_distortion.md).
#include "dvm_frob.h"

namespace dvm {

__device__ __forceinline__ int distortion_unit_exp(unsigned max_bits) { return fix_unit_exp((double)__uint_as_float(max_bits)); }

template <bool GRAD>
__global__ __launch_bounds__(FROB_THREADS) void distortion_row_kernel(const float *__restrict__ pi_val, const int32_t *__restrict__ pi_idx,
                                                                            const float *__restrict__ dist_src, const float *__restrict__ dist_tgt,
                                                                            int N, int M, int topk, double *__restrict__ partial,
                                                                            float *__restrict__ g_val) {
    extern __shared__ double distortion_lds[];
    __shared__ int scol[16], sok[16];
    __shared__ float sval[16];
    __shared__ double gred[FROB_THREADS / WAVE][16];
    float *u = (float *)distortion_lds;           // [M], steps 1 and 2
    long long *Q = (long long *)distortion_lds;   // [M], step 3: the fixed-point sums, then q as doubles in place
    float *res = (float *)(distortion_lds + M);   // [N] (GRAD)
    unsigned *mx = (unsigned *)(res + N);         // [M] (GRAD): bit pattern of the column's largest |term|
    const int tid = threadIdx.x, i = blockIdx.x, b = blockIdx.y;
    const int E = N * topk;
    const float *vb = pi_val + (size_t)b * E;
    const int32_t *ib = pi_idx + (size_t)b * E;
    const float *d1 = dist_src + ((size_t)b * N + i) * N;
    const float *d2 = dist_tgt + (size_t)b * M * M;
    if (tid < 16) {
        int c = -1;
        float v = 0.f;
        if (tid < topk) {
            c = ib[(size_t)i * topk + tid];
            v = vb[(size_t)i * topk + tid];
        }
        // an index outside [0, M) never becomes an address: its slot reads row 0 with value 0, which adds nothing to a finite chain
        const bool ok = c >= 0 && c < M;
        scol[tid] = ok ? c : 0;
        sok[tid] = ok;
        sval[tid] = ok ? v : 0.f;
    }
    __syncthreads();
    for (int m = tid; m < M; m += FROB_THREADS) {
        float a = 0.f;
        for (int t = 0; t < topk; ++t) a = fmaf(sval[t], d2[(size_t)scol[t] * M + m], a);
        u[m] = a;
    }
    __syncthreads();
    double acc = 0.0;
    for (int j = tid; j < N; j += FROB_THREADS) {
        float S = 0.f;
        for (int s = 0; s < topk; ++s) {
            const int c = ib[(size_t)j * topk + s];
            const float v = vb[(size_t)j * topk + s];
            const bool ok = c >= 0 && c < M;
            S = fmaf(ok ? v : 0.f, u[ok ? c : 0], S);
        }
        const double d = (double)S - (double)d1[j];
        acc += d * d;
        if (GRAD) res[j] = (float)d;
    }
    acc = block_tree_sum(acc);   // its last barrier: res is complete and u is dead
    if (tid == 0) partial[(size_t)b * N + i] = acc;
    if (!GRAD) return;
    for (int m = tid; m < M; m += FROB_THREADS) {
        Q[m] = 0;
        mx[m] = 0u;
    }
    __syncthreads();
    for (int e = tid; e < E; e += FROB_THREADS) {
        const float v = vb[e];
        const int c = ib[e];
        // rounding to fp32 is monotone and keeps powers of two: every float64 term stays below 2^(ilogb(the fp32 maximum) + 1)
        if (v != 0.f && c >= 0 && c < M) atomicMax(&mx[c], __float_as_uint(fabsf((float)((double)v * (double)res[e / topk]))));
    }
    __syncthreads();
    for (int e = tid; e < E; e += FROB_THREADS) {
        const float v = vb[e];
        const int c = ib[e];
        if (v != 0.f && c >= 0 && c < M) {
            const long long q = fix_quant((double)v * (double)res[e / topk], distortion_unit_exp(mx[c]));
            atomicAdd((unsigned long long *)&Q[c], (unsigned long long)q);
        }
    }
    __syncthreads();
    double *q = (double *)distortion_lds;
    for (int m = tid; m < M; m += FROB_THREADS) q[m] = fix_value(Q[m], distortion_unit_exp(mx[m]));
    __syncthreads();
    const int lane = tid & (WAVE - 1), wave = tid / WAVE;
    for (int t = 0; t < topk; ++t) {
        const float *row = d2 + (size_t)scol[t] * M;
        double a = 0.0;
        for (int m = tid; m < M; m += FROB_THREADS) a += (double)row[m] * q[m];
        a = wave_sum(a);
        if (lane == 0) gred[wave][t] = a;
    }
    __syncthreads();
    if (tid < topk) {
        const double g = ((gred[0][tid] + gred[1][tid]) + gred[2][tid]) + gred[3][tid];
        g_val[(size_t)b * E + (size_t)i * topk + tid] = sok[tid] ? (float)g : 0.f;
    }
}

}  // namespace dvm

using namespace dvm;

static size_t carve_distortion(Arena &ar, int B, int N, FrobSums &w) {
    w.take(ar, B, N);
    return ar.off;
}
// FROB_MAX_N bounds N and M: LDS is 12 M + 4 N bytes with gradients (128 KB at the limit), 4 M without
static const char *distortion_limits(int B, int N, int M, int topk) {
    const char *who = "dvm_distortion_term_f32";
    FROB_BATCH_LIMITS(who, B, N, M);
    FROB_TOPK_LIMIT(who, topk);
    FROB_LIMIT(N <= FROB_MAX_N, "%s: N=%d unsupported (a residual row must fit LDS: N <= %d)", who, N, FROB_MAX_N);
    FROB_LIMIT(M <= FROB_MAX_N, "%s: M=%d unsupported (a row of P D2 must fit LDS: M <= %d)", who, M, FROB_MAX_N);
    return nullptr;
}

template <bool GRAD>
static void launch_distortion_rows(const float *pi_val, const int32_t *pi_idx, const float *dist_src, const float *dist_tgt, int B, int N, int M,
                                   int topk, double *partial, float *g_val, hipStream_t s) {
    const size_t lds = GRAD ? 12 * (size_t)M + 4 * (size_t)N : 8 * (((size_t)M + 1) / 2);
    ensure_dyn_lds((const void *)distortion_row_kernel<GRAD>, (int)lds);   // with gradients above the 64 KB default from N = M = 4096 on
    hipLaunchKernelGGL(distortion_row_kernel<GRAD>, dim3(N, B), dim3(FROB_THREADS), lds, s, pi_val, pi_idx, dist_src, dist_tgt, N, M, topk,
                       partial, g_val);
}

DVM_EXPORT int dvm_distortion_term_max_n(void) { return FROB_MAX_N; }

DVM_EXPORT size_t dvm_distortion_term_workspace_bytes(int B, int N, int M, int topk) {
    return distortion_limits(B, N, M, topk) ? 0 : null_carve<FrobSums>(carve_distortion, B, N);
}

DVM_EXPORT int dvm_distortion_term_f32(const float *pi_val, const int32_t *pi_idx, const float *dist_src, const float *dist_tgt, int B, int N,
                                       int M, int topk, float *loss, float *g_val, void *ws, size_t ws_bytes, void *stream) {
    DVM_REQUIRE(pi_val && pi_idx && dist_src && dist_tgt && loss, "dvm_distortion_term_f32: null pointer");
    const char *why = distortion_limits(B, N, M, topk);
    DVM_REQUIRE(!why, "%s", why);
    FrobSums w;
    if (!carve_ws(ws, ws_bytes, "dvm_distortion_term_f32", w, carve_distortion, B, N)) return DVM_ENOSPACE;
    hipStream_t s = (hipStream_t)stream;
    if (!g_val)
        launch_distortion_rows<false>(pi_val, pi_idx, dist_src, dist_tgt, B, N, M, topk, w.partial, g_val, s);
    else
        launch_distortion_rows<true>(pi_val, pi_idx, dist_src, dist_tgt, B, N, M, topk, w.partial, g_val, s);
    return frob_finish(w, B, N, 2.0, loss, {{g_val, (size_t)N * topk}}, "distortion_term", s);
}
