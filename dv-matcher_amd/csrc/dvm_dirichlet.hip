// dvm_dirichlet.hip — the Dirichlet energy of a sparse top-k correspondence P (pi_val / pi_idx [B,N,topk], M columns) under a
// weighted neighbour matrix of the source shape in CSR (rowptr [B,N+1], col / w [B,Ecap]: dvm_laplacian.hip), and its gradient
// in pi_val (not in the reference): with Y = P V, V [B,M,C] the target's values (its coordinates),
//   E[b] = 1/2 sum over the entries (i, j, w) of w |y_i - y_j|^2,
//   dE / d pi_val[i,s] = r_i . V[pi_idx[i,s]],   r_i = 2 sum over the entries of row i of w (y_i - y_j)
// — the operator is structurally symmetric (every entry (i, j, w) has its mirror (j, i, w)), so the half of the derivative that
// comes from the rows naming i equals the half from row i itself: the factor 2, and no term from another row.  The loss is E
// itself: no square root, no frob_finish.
//
// Steps: (1) a copy of P in which a slot with an index outside [0, M) is (value 0, column 0): it adds nothing to a finite chain
// and never becomes an address; (2) Y by launch_apply on that copy — dvm_softcorr_apply_f32's launches, so its bits; (3)
// dirichlet_row_kernel; (4) launch_reduce_partials over the rows' float64 shares -> loss.
//
// dirichlet_row_kernel — the mapping.  A row has 0 to ~40 entries on real data, and C (<= 16, 3 for coordinates) channels, so a
// workgroup or even a wave per row would idle most of its lanes, and a thread per row would gather C strided words per entry.
// Here a row belongs to a group of TG = 4, 8 or 16 adjacent lanes (the smallest that holds C), one lane per channel: the lanes
// of a group read one contiguous row of Y per entry, a wave covers 16 / 8 / 4 rows, and every lane walks the row's entries IN
// CSR ORDER, adding w (y_i - y_j) and w (y_i - y_j)^2 of its channel in float64 — a plain sequential chain, the same whatever the
// launch.  The entries are taken four at a time (the four columns, weights and rows of Y are requested before the first is used)
// so that a hub row, up to N - 1 entries after symmetrisation, is a pipelined walk and not N dependent round trips; a split of
// long rows over more lanes would give them another summation order than short ones and is not made.  The channels' shares are
// added by the xor butterfly of the group (fixed partners), the row's energy goes to partial[b][i]; with GRAD the residual r_i[c]
// is still in the lane's register: topk products with V's rows, the same butterfly each -> g_val[i,s].  No LDS, no atomics.
// An entry with a column outside [0, N) adds nothing and is never an address; rowptr is clamped to [0, Ecap].
#include "dvm_frob.h"

namespace dvm {
namespace {

constexpr int DIR_THREADS = 256;
constexpr int DIR_MAX_N = 1 << 24;   // N C, M C and N topk stay far inside int32

// (val, idx) -> (sval, sidx): a slot with an index outside [0, M) becomes (0, column 0)
__global__ __launch_bounds__(DIR_THREADS) void dirichlet_sanitise_kernel(const float *__restrict__ val, const int32_t *__restrict__ idx, size_t n,
                                                                         int M, float *__restrict__ sval, int32_t *__restrict__ sidx) {
    const size_t e = (size_t)blockIdx.x * DIR_THREADS + threadIdx.x;
    if (e >= n) return;
    const int c = idx[e];
    const bool ok = (unsigned)c < (unsigned)M;
    sval[e] = ok ? val[e] : 0.f;
    sidx[e] = ok ? c : 0;
}

template <int TG>
__device__ __forceinline__ double group_sum(double v) {
#pragma unroll
    for (int o = TG / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

template <int TG, bool GRAD>
__global__ __launch_bounds__(DIR_THREADS) void dirichlet_row_kernel(const int32_t *__restrict__ pi_idx, const float *__restrict__ V,
                                                                    const float *__restrict__ Y, const int32_t *__restrict__ rowptr,
                                                                    const int32_t *__restrict__ col, const float *__restrict__ w, int N, int M,
                                                                    int topk, int C, int Ecap, double *__restrict__ partial,
                                                                    float *__restrict__ g_val) {
    const int b = blockIdx.y;
    const int i = blockIdx.x * (DIR_THREADS / TG) + (int)threadIdx.x / TG, c = (int)threadIdx.x % TG;
    // no lane leaves before the last butterfly: a row past N, or a channel past C, walks nothing and adds zeros
    const bool row = i < N, live = row && c < C;
    const float *Yb = Y + (size_t)b * N * C;
    const int32_t *cb = col + (size_t)b * Ecap;
    const float *wb = w + (size_t)b * Ecap;
    int beg = 0, end = 0;
    if (live) {
        beg = max(rowptr[(size_t)b * (N + 1) + i], 0);
        end = min(rowptr[(size_t)b * (N + 1) + i + 1], Ecap);
    }
    const float yi = live ? Yb[(size_t)i * C + c] : 0.f;
    double r = 0.0, e = 0.0;
    for (int p = beg; p < end; p += 4) {
        int j[4];
        float wv[4], yj[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int q = p + u < end ? p + u : p;   // (clamped, then selected: the loads stay unconditional)
            j[u] = cb[q];
            wv[u] = wb[q];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const bool ok = p + u < end && (unsigned)j[u] < (unsigned)N;
            yj[u] = Yb[(size_t)(ok ? j[u] : i) * C + c];
            wv[u] = ok ? wv[u] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const double d = (double)yi - (double)yj[u];
            const double t = (double)wv[u] * d;
            if (p + u < end && (unsigned)j[u] < (unsigned)N) {   // (an entry left out adds nothing, not even 0 x inf)
                r += t;
                e += t * d;
            }
        }
    }
    const double share = group_sum<TG>(e);
    if (row && c == 0) partial[(size_t)b * N + i] = 0.5 * share;
    if (!GRAD) return;
    for (int s = 0; s < topk; ++s) {
        const int m = row ? pi_idx[((size_t)b * N + i) * topk + s] : -1;
        const bool ok = (unsigned)m < (unsigned)M;
        const float v = ok && live ? V[((size_t)b * M + m) * C + c] : 0.f;
        const double g = group_sum<TG>(ok && live ? r * (double)v : 0.0);
        if (row && c == 0) g_val[((size_t)b * N + i) * topk + s] = ok ? (float)(2.0 * g) : 0.f;
    }
}

}  // namespace
}  // namespace dvm

using namespace dvm;

struct DirichletWs {
    float *Y, *sval;     // [B][N][C]; the copy of P: [B][N][topk]
    int32_t *sidx;
    double *partial;     // [B][N]
};
static size_t carve_dirichlet(Arena &ar, int B, int N, int topk, int C, DirichletWs &w) {
    w.Y = ar.take<float>((size_t)B * N * C);
    w.sval = ar.take<float>((size_t)B * N * topk);
    w.sidx = ar.take<int32_t>((size_t)B * N * topk);
    w.partial = ar.take<double>((size_t)B * N);
    return ar.off;
}
static const char *dirichlet_limits(int B, int N, int M, int topk, int C, int Ecap) {
    const char *who = "dvm_dirichlet_term_f32";
    FROB_BATCH_LIMITS(who, B, N, M);
    FROB_TOPK_LIMIT(who, topk);
    FROB_LIMIT(C >= 1 && C <= 16, "%s: C=%d unsupported (1..16)", who, C);
    FROB_LIMIT(Ecap >= 1, "%s: Ecap=%d unsupported (an operator holds at least one entry slot)", who, Ecap);
    FROB_LIMIT(N <= DIR_MAX_N && M <= DIR_MAX_N, "%s: N=%d M=%d unsupported (<= %d)", who, N, M, DIR_MAX_N);
    return nullptr;
}

template <int TG>
static void launch_dirichlet_rows(const int32_t *pi_idx, const float *V, const DirichletWs &w, const int32_t *rowptr, const int32_t *col,
                                  const float *wt, int B, int N, int M, int topk, int C, int Ecap, float *g_val, hipStream_t s) {
    const int rows = DIR_THREADS / TG;
    const dim3 grid((N + rows - 1) / rows, B), block(DIR_THREADS);
    if (g_val)
        hipLaunchKernelGGL((dirichlet_row_kernel<TG, true>), grid, block, 0, s, pi_idx, V, w.Y, rowptr, col, wt, N, M, topk, C, Ecap, w.partial,
                           g_val);
    else
        hipLaunchKernelGGL((dirichlet_row_kernel<TG, false>), grid, block, 0, s, pi_idx, V, w.Y, rowptr, col, wt, N, M, topk, C, Ecap, w.partial,
                           g_val);
}

DVM_EXPORT size_t dvm_dirichlet_term_workspace_bytes(int B, int N, int M, int topk, int C, int Ecap) {
    return dirichlet_limits(B, N, M, topk, C, Ecap) ? 0 : null_carve<DirichletWs>(carve_dirichlet, B, N, topk, C);
}

DVM_EXPORT int dvm_dirichlet_term_f32(const float *pi_val, const int32_t *pi_idx, const float *V, const int32_t *rowptr, const int32_t *col,
                                      const float *w, int B, int N, int M, int topk, int C, int Ecap, float *loss, float *g_val, void *ws,
                                      size_t ws_bytes, void *stream) {
    DVM_REQUIRE(pi_val && pi_idx && V && rowptr && col && w && loss, "dvm_dirichlet_term_f32: null pointer");
    const char *why = dirichlet_limits(B, N, M, topk, C, Ecap);
    DVM_REQUIRE(!why, "%s", why);
    DirichletWs k;
    if (!carve_ws(ws, ws_bytes, "dvm_dirichlet_term_f32", k, carve_dirichlet, B, N, topk, C)) return DVM_ENOSPACE;
    hipStream_t s = (hipStream_t)stream;
    const size_t n = (size_t)B * N * topk;
    hipLaunchKernelGGL(dirichlet_sanitise_kernel, dim3((unsigned)((n + DIR_THREADS - 1) / DIR_THREADS)), dim3(DIR_THREADS), 0, s, pi_val, pi_idx,
                       n, M, k.sval, k.sidx);
    launch_apply(k.sval, k.sidx, V, B, N, M, topk, C, k.Y, s);
    if (C <= 4)
        launch_dirichlet_rows<4>(pi_idx, V, k, rowptr, col, w, B, N, M, topk, C, Ecap, g_val, s);
    else if (C <= 8)
        launch_dirichlet_rows<8>(pi_idx, V, k, rowptr, col, w, B, N, M, topk, C, Ecap, g_val, s);
    else
        launch_dirichlet_rows<16>(pi_idx, V, k, rowptr, col, w, B, N, M, topk, C, Ecap, g_val, s);
    launch_reduce_partials(k.partial, B, N, 1.f, loss, 1, 0, s);
    DVM_CHECK_LAUNCH("dirichlet_term");
    return DVM_OK;
}
