// dvm_dense64.h — the float64 dense pieces that dvm_eigenbasis.hip and dvm_zoomout.hip share: the weighted tall-skinny product
// P^T diag(wt) R in its one fixed summation order (rows ascending within min(64, ceil(N / 32)) chunks, the chunks ascending) and
// the scaled Cholesky factorisation of a Gram matrix held in LDS.  Every kernel here is a plain FMA form without float atomics.
#pragma once
#include "dvm_common.h"
#include <math.h>

namespace dvm {
namespace {

constexpr int EIG_THREADS = 256;
constexpr int EIG_MAX_M = 128;        // block width: one m x m float64 matrix in LDS
constexpr int EIG_MAX_N = 1 << 24;
constexpr int EIG_MAX_CHUNKS = 64;    // row chunks of the tall-skinny products
constexpr int EIG_TR = 8;             // rows staged per step of eig_tn_kernel

__device__ __forceinline__ bool mass_active(float m) { return m > 0.f && m < INFINITY; }

// part[b][chunk] [ma][mb] = sum over the chunk's rows r, ascending, of wt_r P[r][:ma]^T R[g(r)][:mb]   (P [N][ldp] float64,
// R [Rrows][ldr]).  g(r) = idx[b][r] when idx is given (the gather is fused into the staging; a row whose index lies outside
// [0, Rrows) is a zero row), else r.  An element whose skip[b * skip_stride] is set is left alone.
template <typename TR_>
__global__ __launch_bounds__(EIG_THREADS) void eig_tn_kernel(const double *__restrict__ P, int ldp, const TR_ *__restrict__ R, int ldr, int Rrows,
                                                             const int32_t *__restrict__ idx, const float *__restrict__ wt, int N, int ma, int mb,
                                                             int rows_per_chunk, double *__restrict__ part, const int32_t *__restrict__ skip,
                                                             int skip_stride) {
    const int b = blockIdx.y, chunk = blockIdx.x, tid = threadIdx.x;
    if (skip && skip[(size_t)b * skip_stride]) return;
    __shared__ double sP[EIG_TR][EIG_MAX_M], sR[EIG_TR][EIG_MAX_M];
    const int tp = tid / 16, tq = tid % 16;
    const int nu = (ma + 15) / 16, nv = (mb + 15) / 16;
    double acc[8][8];
#pragma unroll
    for (int u = 0; u < 8; ++u)
#pragma unroll
        for (int v = 0; v < 8; ++v) acc[u][v] = 0.0;
    const int r0 = chunk * rows_per_chunk, r1 = min(r0 + rows_per_chunk, N);
    const double *Pb = P + (size_t)b * N * ldp;
    const TR_ *Rb = R + (size_t)b * Rrows * ldr;
    for (int base = r0; base < r1; base += EIG_TR) {
        __syncthreads();
        for (int e = tid; e < EIG_TR * EIG_MAX_M; e += EIG_THREADS) {
            const int r = base + e / EIG_MAX_M, c = e % EIG_MAX_M;
            double pv = 0.0, rv = 0.0;
            if (r < r1) {
                if (c < ma) {
                    pv = Pb[(size_t)r * ldp + c];
                    if (wt) {
                        const float mv = wt[(size_t)b * N + r];
                        pv = mass_active(mv) ? pv * (double)mv : 0.0;
                    }
                }
                if (c < mb) {
                    const int g = idx ? idx[(size_t)b * N + r] : r;
                    if ((unsigned)g < (unsigned)Rrows) rv = (double)Rb[(size_t)g * ldr + c];
                }
            }
            sP[e / EIG_MAX_M][c] = pv;
            sR[e / EIG_MAX_M][c] = rv;
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < EIG_TR; ++r) {
            double pv[8], rv[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) pv[u] = sP[r][tp + 16 * u];
#pragma unroll
            for (int v = 0; v < 8; ++v) rv[v] = sR[r][tq + 16 * v];
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (u < nu) {
#pragma unroll
                    for (int v = 0; v < 8; ++v)
                        if (v < nv) acc[u][v] = fma(pv[u], rv[v], acc[u][v]);
                }
        }
    }
    double *out = part + ((size_t)b * gridDim.x + chunk) * ma * mb;
#pragma unroll
    for (int u = 0; u < 8; ++u)
#pragma unroll
        for (int v = 0; v < 8; ++v) {
            const int p = tp + 16 * u, q = tq + 16 * v;
            if (p < ma && q < mb) out[(size_t)p * mb + q] = acc[u][v];
        }
}

// out[b][e] = part[b][0][e] + part[b][1][e] + ..   (e < mm)
__global__ __launch_bounds__(EIG_THREADS) void eig_reduce_kernel(const double *__restrict__ part, int nchunks, int mm, double *__restrict__ out,
                                                                 const int32_t *__restrict__ skip, int skip_stride) {
    const int b = blockIdx.y, e = blockIdx.x * EIG_THREADS + threadIdx.x;
    if (skip && skip[(size_t)b * skip_stride]) return;
    if (e >= mm) return;
    double acc = 0.0;
    for (int c = 0; c < nchunks; ++c) acc += part[((size_t)b * nchunks + c) * mm + e];
    out[(size_t)b * mm + e] = acc;
}

// The m x m Gram matrix Gb -> its scaled Cholesky factor in lds [m][m]: dsc = diag(G)^-1/2, D G D = L L^T with L in the lower
// triangle (both halves of G are averaged; the upper triangle of lds keeps the scaled entries).  Returns false, in every thread
// at the same point, when a diagonal entry is not a positive finite number or a pivot is not a finite number above piv_floor
// (0: any positive pivot passes; the pivots of a unit-diagonal matrix lie in (0, 1]).  dsc [m] and *bad are in LDS.
__device__ __forceinline__ bool chol_scaled_lds(const double *__restrict__ Gb, int m, double *lds, double *dsc, int *bad, double piv_floor) {
    const int tid = threadIdx.x;
    if (tid == 0) *bad = 0;
    __syncthreads();
    if (tid < m) {
        const double d = Gb[(size_t)tid * m + tid];
        if (d > 0.0 && d <= 1.79e308)
            dsc[tid] = 1.0 / sqrt(d);
        else {
            dsc[tid] = 0.0;
            *bad = 1;
        }
    }
    __syncthreads();
    for (int e = tid; e < m * m; e += EIG_THREADS) {
        const int i = e / m, j = e % m;
        // the lower triangle is used; both halves of G are averaged
        lds[e] = 0.5 * (Gb[e] + Gb[(size_t)j * m + i]) * dsc[i] * dsc[j];
    }
    __syncthreads();
    for (int j = 0; j < m; ++j) {   // (`bad` is tested behind a barrier only: every thread leaves at the same j)
        if (tid == 0) {
            const double p = lds[j * m + j];
            if (p > piv_floor && p <= 1.79e308)
                lds[j * m + j] = sqrt(p);
            else
                *bad = 1;
        }
        __syncthreads();
        if (*bad) break;
        const double piv = lds[j * m + j];
        for (int i = j + 1 + tid; i < m; i += EIG_THREADS) lds[i * m + j] /= piv;
        __syncthreads();
        const int n = m - j - 1;
        for (int e = tid; e < n * n; e += EIG_THREADS) {
            const int i = j + 1 + e / n, c = j + 1 + e % n;
            if (c <= i) lds[i * m + c] -= lds[i * m + j] * lds[c * m + j];
        }
        __syncthreads();
    }
    return !*bad;
}

static int tn_chunks(int N) {
    const int c = (N + 4 * EIG_TR - 1) / (4 * EIG_TR);
    return c < EIG_MAX_CHUNKS ? c : EIG_MAX_CHUNKS;
}

// out [B][ma][mb] = P^T diag(wt) R[g] through `part` ([B][tn_chunks(N)][ma][mb])
template <typename TR_>
static void launch_tn(const double *P, int ldp, const TR_ *R, int ldr, int Rrows, const int32_t *idx, const float *wt, int B, int N, int ma,
                      int mb, double *part, double *out, const int32_t *skip, int skip_stride, hipStream_t s) {
    const int nch = tn_chunks(N), rpc = (N + nch - 1) / nch;
    hipLaunchKernelGGL((eig_tn_kernel<TR_>), dim3(nch, B), dim3(EIG_THREADS), 0, s, P, ldp, R, ldr, Rrows, idx, wt, N, ma, mb, rpc, part, skip,
                       skip_stride);
    hipLaunchKernelGGL(eig_reduce_kernel, dim3((ma * mb + EIG_THREADS - 1) / EIG_THREADS, B), dim3(EIG_THREADS), 0, s, part, nch, ma * mb, out, skip,
                       skip_stride);
}

}  // namespace
}  // namespace dvm
