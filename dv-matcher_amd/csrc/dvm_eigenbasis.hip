// dvm_eigenbasis.hip — the first k eigenpairs of L phi = lambda M phi for a CSR operator of dvm_laplacian.hip (rowptr [B,N+1],
// col / w [B,Ecap]) and a lumped mass [B,N] (not in this form in the reference, which calls a sparse shift-invert solver on the
// host), and the projection Phi^T M Y onto such a basis.  float64 throughout; the definition is in include/dvm.h.
//
// The method: Chebyshev-filtered subspace iteration on A = S L S, S = diag(m^-1/2), with a block X [N, m], m = k + guard, row-major.
// One outer iteration:
//   (1) Rayleigh-Ritz: W = A X, H = X^T W, H = Q diag(theta) Q^T (Jacobi), X <- X Q, W = A X again for the pair that is returned,
//       res_j = |W_j - theta_j X_j| / beta; converged when max_{j<k} res_j <= tol;
//   (2) the degree-d Chebyshev filter that damps [theta_m, 1.01 beta], scaled at theta_1 (no overflow: its gain is 1 at theta_1);
//   (3) Cholesky-QR twice, each on the Gram matrix scaled to a unit diagonal (the filter's gain never reaches the factorisation).
//
// Kernels.  eig_op_kernel: one thread per (row, column), lanes along the contiguous 8 m-byte row; a row's entries are walked in
// CSR order and the neighbour rows are read as whole rows: Y' = a (A Y - c Y) - b X, one launch per filter degree.
// eig_tn_kernel (dvm_dense64.h, shared with dvm_zoomout.hip): P^T diag(wt) R over a chunk of rows, a 16 x 16 thread grid with an
// 8 x 8 register tile each, rows staged through LDS and added in ascending row order; eig_reduce_kernel adds the chunks in ascending order (the chunking depends on N
// alone).  eig_update_kernel: X T for an m x m T.  These two are plain FMA forms (profiles/notes_eigenbasis.md).  The dense m x m
// steps run in one workgroup per batch element with one matrix in LDS (m <= 128: 128 KB) and the second in global memory:
// eig_jacobi_kernel (parallel-ordered cyclic Jacobi, round-robin pairs; eigenvalues ascending, ties by column number) and
// eig_chol_kernel (scaled Gram -> Cholesky factor with a pivot check, chol_scaled_lds of dvm_dense64.h -> the inverse factor,
// applied to the block by eig_update_kernel).  No float atomics anywhere: every sum has one order, so an element gives the same bits alone or in a batch.
//
// state [B][8] int32: done, error, outer iterations, converged, inactive vertices, operator applications.  Every kernel of the
// loop leaves at once when its element's `done` is set, so a finished element's pairs (always in block 2 after step (1)) stay.
// The host reads the state back once per outer iteration: the entry waits for its stream and is not capturable.
#include "dvm_dense64.h"
#include <vector>

namespace dvm {
namespace {

constexpr int EIG_MAX_DEGREE = 256;
constexpr int EIG_UR = 16;            // rows per workgroup of eig_update_kernel
constexpr int EIG_SWEEPS = 40;
enum { ST_DONE = 0, ST_ERR = 1, ST_ITER = 2, ST_CONV = 3, ST_INACTIVE = 4, ST_NOPS = 5, ST_WORDS = 8 };
enum { EIG_ERR_ACTIVE = 1, EIG_ERR_PIVOT = 2, EIG_ERR_SCALE = 3 };

// s_i and the row's Gershgorin term (-1 on an inactive row)
__global__ __launch_bounds__(EIG_THREADS) void eig_rows_kernel(const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                               const float *__restrict__ w, const float *__restrict__ mass, int N, int Ecap,
                                                               double *__restrict__ s, double *__restrict__ gersh) {
    const int b = blockIdx.y, i = blockIdx.x * EIG_THREADS + threadIdx.x;
    if (i >= N) return;
    const float *mb = mass ? mass + (size_t)b * N : nullptr;
    const float mi = mb ? mb[i] : 1.f;
    if (!mass_active(mi)) {
        s[(size_t)b * N + i] = 0.0;
        gersh[(size_t)b * N + i] = -1.0;
        return;
    }
    const int beg = max(rowptr[(size_t)b * (N + 1) + i], 0), end = min(rowptr[(size_t)b * (N + 1) + i + 1], Ecap);
    double sum = 0.0, asum = 0.0;
    for (int p = beg; p < end; ++p) {
        const int j = col[(size_t)b * Ecap + p];
        if ((unsigned)j >= (unsigned)N) continue;
        if (mb && !mass_active(mb[j])) continue;
        const double wv = (double)w[(size_t)b * Ecap + p];
        sum += wv;
        asum += fabs(wv);
    }
    s[(size_t)b * N + i] = 1.0 / sqrt((double)mi);
    gersh[(size_t)b * N + i] = (fabs(sum) + asum) / (double)mi;
}

// beta = max of the rows' terms, the inactive count, the element's state
__global__ __launch_bounds__(EIG_THREADS) void eig_setup_kernel(const double *__restrict__ gersh, int N, int m, double *__restrict__ beta,
                                                                int32_t *__restrict__ state) {
    __shared__ double smax[EIG_THREADS];
    __shared__ int sina[EIG_THREADS];
    const int b = blockIdx.x, tid = threadIdx.x;
    double mx = 0.0;
    int ina = 0;
    bool bad = false;
    for (int i = tid; i < N; i += EIG_THREADS) {
        const double g = gersh[(size_t)b * N + i];
        if (g < 0.0)
            ++ina;
        else if (g <= 1.79e308)
            mx = fmax(mx, g);
        else
            bad = true;   // inf or NaN
    }
    smax[tid] = bad ? INFINITY : mx;
    sina[tid] = ina;
    __syncthreads();
    for (int o = EIG_THREADS / 2; o > 0; o >>= 1) {
        if (tid < o) {
            smax[tid] = fmax(smax[tid], smax[tid + o]);
            sina[tid] += sina[tid + o];
        }
        __syncthreads();
    }
    if (tid == 0) {
        const double bt = smax[0];
        int err = 0;
        if (N - sina[0] < m)
            err = EIG_ERR_ACTIVE;
        else if (!(bt > 0.0) || !(bt <= 1.79e308))
            err = EIG_ERR_SCALE;
        beta[b] = bt;
        int32_t *st = state + (size_t)b * ST_WORDS;
        for (int q = 0; q < ST_WORDS; ++q) st[q] = 0;
        st[ST_INACTIVE] = sina[0];
        st[ST_ERR] = err;
        st[ST_DONE] = err ? 1 : 0;
    }
}

// the start block: a counter-based hash of (vertex, column) alone, in [-1, 1); 0 on inactive rows
__global__ __launch_bounds__(EIG_THREADS) void eig_start_kernel(const double *__restrict__ s, int N, int m, double *__restrict__ X,
                                                                const int32_t *__restrict__ state) {
    const int b = blockIdx.y;
    if (state[(size_t)b * ST_WORDS + ST_DONE]) return;
    const size_t t = (size_t)blockIdx.x * EIG_THREADS + threadIdx.x;
    if (t >= (size_t)N * m) return;
    const unsigned i = (unsigned)(t / m), j = (unsigned)(t % m);
    unsigned long long z = ((unsigned long long)i << 32) | j;
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    const double u = (double)(z >> 11) * 0x1p-52 - 1.0;
    X[(size_t)b * N * m + t] = s[(size_t)b * N + i] > 0.0 ? u : 0.0;
}

// Yout = a (A Yin - c Yin) - bb Xprev with (a, c, bb) = coef[b][step] (step < 0: Yout = A Yin)
__global__ __launch_bounds__(EIG_THREADS) void eig_op_kernel(const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                             const float *__restrict__ w, const double *__restrict__ s,
                                                             const double *__restrict__ Yin, const double *__restrict__ Xprev,
                                                             double *__restrict__ Yout, const double *__restrict__ coef, int step, int N, int m,
                                                             int Ecap, const int32_t *__restrict__ state) {
    const int b = blockIdx.y;
    if (state[(size_t)b * ST_WORDS + ST_DONE]) return;
    const size_t t = (size_t)blockIdx.x * EIG_THREADS + threadIdx.x;
    if (t >= (size_t)N * m) return;
    const int i = (int)(t / m), j = (int)(t % m);
    const double *Yb = Yin + (size_t)b * N * m;
    const double *sb = s + (size_t)b * N;
    const double si = sb[i];
    double out = 0.0;
    if (si > 0.0) {
        const int beg = max(rowptr[(size_t)b * (N + 1) + i], 0), end = min(rowptr[(size_t)b * (N + 1) + i + 1], Ecap);
        const int32_t *cb = col + (size_t)b * Ecap;
        const float *wb = w + (size_t)b * Ecap;
        const double y = Yb[t], yi = si * y;
        double acc = 0.0;
        for (int p = beg; p < end; ++p) {
            const int c = cb[p];
            if ((unsigned)c >= (unsigned)N) continue;
            const double sj = sb[c];
            if (!(sj > 0.0)) continue;
            acc += (double)wb[p] * (yi - sj * Yb[(size_t)c * m + j]);
        }
        out = si * acc;
        if (step >= 0) {
            const double *cf = coef + ((size_t)b * EIG_MAX_DEGREE + step) * 3;
            out = cf[0] * (out - cf[1] * y);
            if (cf[2] != 0.0) out -= cf[2] * Xprev[(size_t)b * N * m + t];
        }
    }
    Yout[(size_t)b * N * m + t] = out;
}

// Xout = Xin T for T [m][m]: 16 rows per workgroup in LDS, a thread owns 4 rows x columns (tq, tq + 64)
__global__ __launch_bounds__(EIG_THREADS) void eig_update_kernel(const double *__restrict__ Xin, const double *__restrict__ T,
                                                                 double *__restrict__ Xout, int N, int m, const int32_t *__restrict__ state) {
    const int b = blockIdx.y, tid = threadIdx.x;
    if (state[(size_t)b * ST_WORDS + ST_DONE]) return;
    __shared__ double sX[EIG_UR][EIG_MAX_M];
    const int r0 = blockIdx.x * EIG_UR;
    const double *Xb = Xin + (size_t)b * N * m;
    const double *Tb = T + (size_t)b * m * m;
    for (int e = tid; e < EIG_UR * EIG_MAX_M; e += EIG_THREADS) {
        const int r = r0 + e / EIG_MAX_M, c = e % EIG_MAX_M;
        sX[e / EIG_MAX_M][c] = (r < N && c < m) ? Xb[(size_t)r * m + c] : 0.0;
    }
    __syncthreads();
    const int tq = tid % 64, tr = tid / 64;
    const bool c0 = tq < m, c1 = tq + 64 < m;
    double acc0[4] = {0.0, 0.0, 0.0, 0.0}, acc1[4] = {0.0, 0.0, 0.0, 0.0};
    for (int p = 0; p < m; ++p) {
        const double t0 = c0 ? Tb[(size_t)p * m + tq] : 0.0, t1 = c1 ? Tb[(size_t)p * m + tq + 64] : 0.0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const double x = sX[tr * 4 + r][p];
            acc0[r] = fma(x, t0, acc0[r]);
            acc1[r] = fma(x, t1, acc1[r]);
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = r0 + tr * 4 + r;
        if (row < N) {
            if (c0) Xout[((size_t)b * N + row) * m + tq] = acc0[r];
            if (c1) Xout[((size_t)b * N + row) * m + tq + 64] = acc1[r];
        }
    }
}

// G [m][m] (a Gram matrix) -> T = D L^-T with D = diag(G)^-1/2 and D G D = L L^T: X T is orthonormal.  A pivot that is not a
// positive finite number sets the element's error and `done`.  LDS: the m x m matrix (L below the diagonal, L^-1's columns above).
__global__ __launch_bounds__(EIG_THREADS) void eig_chol_kernel(const double *__restrict__ G, double *__restrict__ T, int m, int32_t *__restrict__ state) {
    extern __shared__ double lds[];
    __shared__ double dsc[EIG_MAX_M];
    __shared__ int bad;
    const int b = blockIdx.x, tid = threadIdx.x;
    if (state[(size_t)b * ST_WORDS + ST_DONE]) return;
    const double *Gb = G + (size_t)b * m * m;
    double *Tb = T + (size_t)b * m * m;
    if (!chol_scaled_lds(Gb, m, lds, dsc, &bad, 0.0)) {
        if (tid == 0) {
            state[(size_t)b * ST_WORDS + ST_ERR] = EIG_ERR_PIVOT;
            state[(size_t)b * ST_WORDS + ST_DONE] = 1;
        }
        return;
    }
    // column j of L^-1 by forward substitution, kept in row j of the upper triangle: z_i at lds[j][i], i > j
    if (tid < m) {
        const int j = tid;
        const double zj = 1.0 / lds[j * m + j];
        for (int i = j + 1; i < m; ++i) {
            double acc = lds[i * m + j] * zj;
            for (int c = j + 1; c < i; ++c) acc += lds[i * m + c] * lds[j * m + c];
            lds[j * m + i] = -acc / lds[i * m + i];
        }
    }
    __syncthreads();
    // T[p][q] = d_p L^-1[q][p]
    for (int e = tid; e < m * m; e += EIG_THREADS) {
        const int p = e / m, q = e % m;
        Tb[e] = q > p ? dsc[p] * lds[e] : q == p ? dsc[p] / lds[e] : 0.0;
    }
}

// H [m][m] symmetric -> theta [m] ascending (ties: lower column first) and Q [m][m], H Q = Q diag(theta).  Qw: the unsorted
// eigenvectors (global scratch).  Parallel-ordered cyclic Jacobi: the round-robin schedule gives n / 2 disjoint pairs per step.
__global__ __launch_bounds__(EIG_THREADS) void eig_jacobi_kernel(const double *__restrict__ H, double *Qw, double *__restrict__ Q,
                                                                 double *__restrict__ theta, int m, const int32_t *__restrict__ state) {
    extern __shared__ double lds[];
    __shared__ double cs[EIG_MAX_M / 2], sn[EIG_MAX_M / 2], red[EIG_THREADS];
    __shared__ int pp[EIG_MAX_M / 2], qq[EIG_MAX_M / 2], rotated;
    const int b = blockIdx.x, tid = threadIdx.x;
    if (state[(size_t)b * ST_WORDS + ST_DONE]) return;
    const double *Hb = H + (size_t)b * m * m;
    double *Vb = Qw + (size_t)b * m * m;
    double fro = 0.0;
    for (int e = tid; e < m * m; e += EIG_THREADS) {
        const int i = e / m, j = e % m;
        const double h = 0.5 * (Hb[e] + Hb[(size_t)j * m + i]);
        lds[e] = h;
        Vb[e] = i == j ? 1.0 : 0.0;
        fro += h * h;
    }
    red[tid] = fro;
    __syncthreads();
    for (int o = EIG_THREADS / 2; o > 0; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    const double thr = sqrt(red[0]) * 0x1p-58;
    const int n = (m + 1) & ~1, half = n / 2;
    for (int sweep = 0; sweep < EIG_SWEEPS; ++sweep) {
        if (tid == 0) rotated = 0;
        __syncthreads();
        for (int t = 0; t < n - 1; ++t) {
            if (tid < half) {
                int p = tid == 0 ? t : (t + tid) % (n - 1), q = tid == 0 ? n - 1 : (t - tid + (n - 1)) % (n - 1);
                if (p > q) {
                    const int x = p;
                    p = q;
                    q = x;
                }
                double c = 1.0, s = 0.0;
                if (q < m) {
                    const double hpq = lds[p * m + q];
                    if (fabs(hpq) > thr) {
                        const double tau = (lds[q * m + q] - lds[p * m + p]) / (2.0 * hpq);
                        const double tt = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
                        c = 1.0 / sqrt(1.0 + tt * tt);
                        s = tt * c;
                        rotated = 1;
                    }
                }
                cs[tid] = c;
                sn[tid] = s;
                pp[tid] = p;
                qq[tid] = q;
            }
            __syncthreads();
            for (int e = tid; e < half * m; e += EIG_THREADS) {   // rows p, q of J^T H
                const int k = e / m, j = e % m;
                const double s = sn[k];
                if (s != 0.0) {
                    const double c = cs[k], hp = lds[pp[k] * m + j], hq = lds[qq[k] * m + j];
                    lds[pp[k] * m + j] = c * hp - s * hq;
                    lds[qq[k] * m + j] = s * hp + c * hq;
                }
            }
            __syncthreads();
            for (int e = tid; e < half * m; e += EIG_THREADS) {   // columns p, q of (J^T H) J and of V J
                const int k = e / m, i = e % m;
                const double s = sn[k];
                if (s != 0.0) {
                    const double c = cs[k], hp = lds[i * m + pp[k]], hq = lds[i * m + qq[k]];
                    lds[i * m + pp[k]] = c * hp - s * hq;
                    lds[i * m + qq[k]] = s * hp + c * hq;
                    const double vp = Vb[i * m + pp[k]], vq = Vb[i * m + qq[k]];
                    Vb[i * m + pp[k]] = c * vp - s * vq;
                    Vb[i * m + qq[k]] = s * vp + c * vq;
                }
            }
            __syncthreads();
        }
        if (!rotated) break;   // (read after the step's last barrier; written again only after the next one)
        __syncthreads();
    }
    __syncthreads();
    // ascending eigenvalues, ties by column number: column j goes to its rank
    if (tid < m) {
        const double tj = lds[tid * m + tid];
        int rank = 0;
        for (int i = 0; i < m; ++i) {
            const double ti = lds[i * m + i];
            rank += (ti < tj || (ti == tj && i < tid)) ? 1 : 0;
        }
        theta[(size_t)b * m + rank] = tj;
        red[tid] = (double)rank;
    }
    __syncthreads();
    for (int e = tid; e < m * m; e += EIG_THREADS) {
        const int i = e / m, j = e % m;
        Q[(size_t)b * m * m + i * m + (int)red[j]] = Vb[e];
    }
}

// part[b][chunk][j] = sum over the chunk's rows, ascending, of (W[r][j] - theta_j X[r][j])^2
__global__ __launch_bounds__(EIG_MAX_M) void eig_colnorm_kernel(const double *__restrict__ X, const double *__restrict__ W,
                                                                const double *__restrict__ theta, int N, int m, int rows_per_chunk,
                                                                double *__restrict__ part, const int32_t *__restrict__ state) {
    const int b = blockIdx.y, chunk = blockIdx.x, j = threadIdx.x;
    if (state[(size_t)b * ST_WORDS + ST_DONE]) return;
    if (j >= m) return;
    const double th = theta[(size_t)b * m + j];
    const int r0 = chunk * rows_per_chunk, r1 = min(r0 + rows_per_chunk, N);
    double acc = 0.0;
    for (int r = r0; r < r1; ++r) {
        const size_t at = ((size_t)b * N + r) * m + j;
        const double d = W[at] - th * X[at];
        acc += d * d;
    }
    part[((size_t)b * gridDim.x + chunk) * m + j] = acc;
}

// the residuals, the convergence decision and the next filter's coefficients
__global__ __launch_bounds__(EIG_MAX_M) void eig_finalize_kernel(const double *__restrict__ part, int nchunks, const double *__restrict__ theta,
                                                                 const double *__restrict__ beta, int m, int k, int degree, int max_iter, double tol,
                                                                 double *__restrict__ resv, double *__restrict__ coef, int32_t *__restrict__ state) {
    __shared__ double red[EIG_MAX_M];
    const int b = blockIdx.x, j = threadIdx.x;
    int32_t *st = state + (size_t)b * ST_WORDS;
    if (st[ST_DONE]) return;
    const double bt = beta[b];
    double r = 0.0;
    if (j < m) {
        double acc = 0.0;
        for (int c = 0; c < nchunks; ++c) acc += part[((size_t)b * nchunks + c) * m + j];
        r = sqrt(acc) / bt;
        resv[(size_t)b * m + j] = r;
    }
    // a NaN residual must not pass for converged: it counts as +inf
    red[j] = j < k ? (r == r ? r : INFINITY) : 0.0;
    __syncthreads();
    for (int o = EIG_MAX_M / 2; o > 0; o >>= 1) {
        if (j < o) red[j] = fmax(red[j], red[j + o]);
        __syncthreads();
    }
    if (j != 0) return;
    const int it = st[ST_ITER] + 1;
    st[ST_ITER] = it;
    st[ST_NOPS] = 2 * it + degree * (it - 1);
    if (red[0] <= tol) {
        st[ST_CONV] = 1;
        st[ST_DONE] = 1;
        return;
    }
    if (it >= max_iter) {
        st[ST_DONE] = 1;
        return;
    }
    // Chebyshev filter on [low, up] scaled at a0: Y1 = (s1 / e)(A X - c X), Y_{d+1} = (2 s' / e)(A Y_d - c Y_d) - (s s') Y_{d-1}
    const double a0 = theta[(size_t)b * m], up = 1.01 * bt;
    const double low = fmin(fmax(theta[(size_t)b * m + m - 1], a0 + 1e-3 * bt), 0.99 * up);
    const double e = 0.5 * (up - low), c = 0.5 * (up + low);
    double sig = e / (a0 - c);
    const double s1 = sig;
    double *cf = coef + (size_t)b * EIG_MAX_DEGREE * 3;
    cf[0] = s1 / e;
    cf[1] = c;
    cf[2] = 0.0;
    for (int d = 1; d < degree; ++d) {
        const double s2 = 1.0 / (2.0 / s1 - sig);
        cf[3 * d] = 2.0 * s2 / e;
        cf[3 * d + 1] = c;
        cf[3 * d + 2] = sig * s2;
        sig = s2;
    }
}

// evecs[b][i][j] = sign_j s_i X[i][j] (the entry of largest magnitude positive, the lowest index on a tie); evals, res, info
__global__ __launch_bounds__(EIG_THREADS) void eig_output_kernel(const double *__restrict__ X, const double *__restrict__ s,
                                                                 const double *__restrict__ theta, const double *__restrict__ resv,
                                                                 const int32_t *__restrict__ state, int N, int m, int k, double *__restrict__ evals,
                                                                 double *__restrict__ evecs, double *__restrict__ res, int32_t *__restrict__ info) {
    __shared__ double bv[EIG_THREADS];
    __shared__ int bi[EIG_THREADS];
    const int b = blockIdx.y, j = blockIdx.x, tid = threadIdx.x;
    const double *Xb = X + (size_t)b * N * m;
    const double *sb = s + (size_t)b * N;
    double best = -1.0;
    int at = 0x7fffffff;
    for (int i = tid; i < N; i += EIG_THREADS) {
        const double v = fabs(sb[i] * Xb[(size_t)i * m + j]);
        if (v > best) {   // ascending i within a thread: the first of equal values stays
            best = v;
            at = i;
        }
    }
    bv[tid] = best;
    bi[tid] = at;
    __syncthreads();
    for (int o = EIG_THREADS / 2; o > 0; o >>= 1) {
        if (tid < o && (bv[tid + o] > bv[tid] || (bv[tid + o] == bv[tid] && bi[tid + o] < bi[tid]))) {
            bv[tid] = bv[tid + o];
            bi[tid] = bi[tid + o];
        }
        __syncthreads();
    }
    const int top = bi[0] < N ? bi[0] : 0;
    const double sign = sb[top] * Xb[(size_t)top * m + j] < 0.0 ? -1.0 : 1.0;
    for (int i = tid; i < N; i += EIG_THREADS) {
        const double si = sb[i];
        evecs[((size_t)b * N + i) * k + j] = si > 0.0 ? sign * (si * Xb[(size_t)i * m + j]) : 0.0;
    }
    if (tid == 0) {
        evals[(size_t)b * k + j] = theta[(size_t)b * m + j];
        res[(size_t)b * k + j] = resv[(size_t)b * m + j];
        if (j == 0) {
            const int32_t *st = state + (size_t)b * ST_WORDS;
            info[b * 4 + 0] = st[ST_ITER];
            info[b * 4 + 1] = st[ST_CONV];
            info[b * 4 + 2] = st[ST_INACTIVE];
            info[b * 4 + 3] = st[ST_NOPS];
        }
    }
}

}  // namespace
}  // namespace dvm

using namespace dvm;

struct EigWs {
    int32_t *state;
    double *beta, *s, *gersh, *blk[3], *H, *Q, *T, *theta, *resv, *coef, *part;
};
static size_t carve_eig(Arena &ar, int B, int N, int m, EigWs &w) {
    const size_t b = (size_t)B, mm = (size_t)m * m;
    w.state = ar.take<int32_t>(b * ST_WORDS);
    w.beta = ar.take<double>(b);
    w.s = ar.take<double>(b * N);
    w.gersh = ar.take<double>(b * N);
    for (int q = 0; q < 3; ++q) w.blk[q] = ar.take<double>(b * N * m);
    w.H = ar.take<double>(b * mm);
    w.Q = ar.take<double>(b * mm);
    w.T = ar.take<double>(b * mm);
    w.theta = ar.take<double>(b * m);
    w.resv = ar.take<double>(b * m);
    w.coef = ar.take<double>(b * EIG_MAX_DEGREE * 3);
    w.part = ar.take<double>(b * tn_chunks(N) * mm);
    return ar.off;
}
static const char *eig_limits(int B, int N, int Ecap, int k, int guard) {
    static thread_local char msg[200];
    const char *who = "dvm_eigenbasis_f64";
#define EIG_LIMIT(cond, ...)                    \
    if (!(cond)) {                              \
        snprintf(msg, sizeof msg, __VA_ARGS__); \
        return msg;                             \
    }
    EIG_LIMIT(B >= 1 && B <= 65535, "%s: B=%d unsupported (1..65535)", who, B);
    EIG_LIMIT(N >= 1 && N <= EIG_MAX_N, "%s: N=%d unsupported (1..%d)", who, N, EIG_MAX_N);
    EIG_LIMIT(Ecap >= 1, "%s: Ecap=%d unsupported (an operator holds at least one entry slot)", who, Ecap);
    EIG_LIMIT(k >= 1 && guard >= 1, "%s: k=%d guard=%d unsupported (both >= 1)", who, k, guard);
    EIG_LIMIT(k <= EIG_MAX_M && guard <= EIG_MAX_M && k + guard <= (N < EIG_MAX_M ? N : EIG_MAX_M),
              "%s: k + guard = %d + %d exceeds min(N, %d) = %d", who, k, guard, EIG_MAX_M, N < EIG_MAX_M ? N : EIG_MAX_M);
    return nullptr;
}
static const char *project_limits(int B, int N, int k, int C) {
    static thread_local char msg[200];
    const char *who = "dvm_basis_project_f64";
    EIG_LIMIT(B >= 1 && B <= 65535, "%s: B=%d unsupported (1..65535)", who, B);
    EIG_LIMIT(N >= 1 && N <= EIG_MAX_N, "%s: N=%d unsupported (1..%d)", who, N, EIG_MAX_N);
    EIG_LIMIT(k >= 1 && k <= EIG_MAX_M && C >= 1 && C <= EIG_MAX_M, "%s: k=%d C=%d unsupported (1..%d)", who, k, C, EIG_MAX_M);
    return nullptr;
}
#undef EIG_LIMIT

DVM_EXPORT int dvm_eigenbasis_max_block(void) { return EIG_MAX_M; }

DVM_EXPORT size_t dvm_eigenbasis_workspace_bytes(int B, int N, int Ecap, int k, int guard) {
    return eig_limits(B, N, Ecap, k, guard) ? 0 : null_carve<EigWs>(carve_eig, B, N, k + guard);
}

DVM_EXPORT int dvm_eigenbasis_f64(const int32_t *rowptr, const int32_t *col, const float *w, const float *mass, int B, int N, int Ecap, int k,
                                  int guard, int degree, int max_iter, double tol, double *evals, double *evecs, double *res, int32_t *info,
                                  void *ws, size_t ws_bytes, void *stream) {
    const char *who = "dvm_eigenbasis_f64";
    DVM_REQUIRE(rowptr && col && w && evals && evecs && res && info, "%s: null pointer", who);
    const char *why = eig_limits(B, N, Ecap, k, guard);
    DVM_REQUIRE(!why, "%s", why);
    DVM_REQUIRE(degree >= 1 && degree <= EIG_MAX_DEGREE, "%s: degree=%d unsupported (1..%d)", who, degree, EIG_MAX_DEGREE);
    DVM_REQUIRE(max_iter >= 1, "%s: max_iter=%d unsupported (>= 1)", who, max_iter);
    DVM_REQUIRE(tol > 0.0, "%s: tol=%g unsupported (> 0)", who, tol);
    const int m = k + guard;
    EigWs z;
    if (!carve_ws(ws, ws_bytes, who, z, carve_eig, B, N, m)) return DVM_ENOSPACE;
    hipStream_t s = (hipStream_t)stream;
    const size_t lds = (size_t)m * m * sizeof(double);
    ensure_dyn_lds((const void *)eig_chol_kernel, EIG_MAX_M * EIG_MAX_M * (int)sizeof(double));
    ensure_dyn_lds((const void *)eig_jacobi_kernel, EIG_MAX_M * EIG_MAX_M * (int)sizeof(double));
    const dim3 rows((N + EIG_THREADS - 1) / EIG_THREADS, B), elems((unsigned)(((size_t)N * m + EIG_THREADS - 1) / EIG_THREADS), B);
    const int nch = tn_chunks(N), rpc = (N + nch - 1) / nch;

    auto op = [&](const double *yin, const double *xprev, double *yout, int step) {
        hipLaunchKernelGGL(eig_op_kernel, elems, dim3(EIG_THREADS), 0, s, rowptr, col, w, z.s, yin, xprev, yout, z.coef, step, N, m, Ecap, z.state);
    };
    auto update = [&](const double *xin, const double *T, double *xout) {
        hipLaunchKernelGGL(eig_update_kernel, dim3((N + EIG_UR - 1) / EIG_UR, B), dim3(EIG_THREADS), 0, s, xin, T, xout, N, m, z.state);
    };
    // Cholesky-QR twice: from block `src` through the block that is neither `src` nor 0, into block 0
    auto orthonormalise = [&](int src) {
        const int mid = src == 0 ? 1 : 3 - src;
        const int path[3] = {src, mid, 0};
        for (int pass = 0; pass < 2; ++pass) {
            launch_tn<double>(z.blk[path[pass]], m, z.blk[path[pass]], m, N, nullptr, nullptr, B, N, m, m, z.part, z.H, z.state, ST_WORDS, s);
            hipLaunchKernelGGL(eig_chol_kernel, dim3(B), dim3(EIG_THREADS), lds, s, z.H, z.T, m, z.state);
            update(z.blk[path[pass]], z.T, z.blk[path[pass + 1]]);
        }
    };

    hipLaunchKernelGGL(eig_rows_kernel, rows, dim3(EIG_THREADS), 0, s, rowptr, col, w, mass, N, Ecap, z.s, z.gersh);
    hipLaunchKernelGGL(eig_setup_kernel, dim3(B), dim3(EIG_THREADS), 0, s, z.gersh, N, m, z.beta, z.state);
    hipLaunchKernelGGL(eig_start_kernel, elems, dim3(EIG_THREADS), 0, s, z.s, N, m, z.blk[0], z.state);
    orthonormalise(0);
    DVM_CHECK_LAUNCH("eigenbasis (start block)");

    std::vector<int32_t> host((size_t)B * ST_WORDS);
    for (int it = 1; it <= max_iter; ++it) {
        // Rayleigh-Ritz: X in block 0 -> the rotated X in block 2, A X in block 1
        op(z.blk[0], z.blk[0], z.blk[1], -1);
        launch_tn<double>(z.blk[0], m, z.blk[1], m, N, nullptr, nullptr, B, N, m, m, z.part, z.H, z.state, ST_WORDS, s);
        hipLaunchKernelGGL(eig_jacobi_kernel, dim3(B), dim3(EIG_THREADS), lds, s, z.H, z.T, z.Q, z.theta, m, z.state);
        update(z.blk[0], z.Q, z.blk[2]);
        op(z.blk[2], z.blk[2], z.blk[1], -1);
        hipLaunchKernelGGL(eig_colnorm_kernel, dim3(nch, B), dim3(EIG_MAX_M), 0, s, z.blk[2], z.blk[1], z.theta, N, m, rpc, z.part, z.state);
        hipLaunchKernelGGL(eig_finalize_kernel, dim3(B), dim3(EIG_MAX_M), 0, s, z.part, nch, z.theta, z.beta, m, k, degree, max_iter, tol, z.resv,
                           z.coef, z.state);
        DVM_CHECK_LAUNCH("eigenbasis (Rayleigh-Ritz)");
        // the one synchronising step per outer iteration (include/dvm.h): the B state rows are copied back and waited for
        if (hipMemcpyAsync(host.data(), z.state, host.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s) != hipSuccess ||
            hipStreamSynchronize(s) != hipSuccess) {
            set_error("%s: reading the convergence flags back failed: %s", who, hipGetErrorString(hipGetLastError()));
            return DVM_ELAUNCH;
        }
        bool all = true;
        for (int b = 0; b < B; ++b) {
            const int32_t *st = &host[(size_t)b * ST_WORDS];
            DVM_REQUIRE(st[ST_ERR] != EIG_ERR_ACTIVE, "%s: element %d has %d active vertices (mass finite and > 0), fewer than k + guard = %d", who,
                        b, N - st[ST_INACTIVE], m);
            DVM_REQUIRE(st[ST_ERR] != EIG_ERR_SCALE, "%s: element %d: the operator's scale beta is 0 or not finite", who, b);
            if (st[ST_ERR] == EIG_ERR_PIVOT) {
                set_error("%s: element %d: a Cholesky pivot of the block's Gram matrix is not a positive finite number (outer iteration %d)",
                          who, b, st[ST_ITER]);
                return DVM_ELAUNCH;
            }
            all = all && st[ST_DONE];
        }
        if (all) break;
        // the filter: X = block 2, Y_1 -> block 0, Y_2 -> block 1, then the three rotate
        int x = 2, y = 0, yn = 1;
        op(z.blk[x], z.blk[x], z.blk[y], 0);
        for (int d = 1; d < degree; ++d) {
            op(z.blk[y], z.blk[x], z.blk[yn], d);
            const int t = x;
            x = y;
            y = yn;
            yn = t;
        }
        orthonormalise(y);
        DVM_CHECK_LAUNCH("eigenbasis (filter)");
    }
    hipLaunchKernelGGL(eig_output_kernel, dim3(k, B), dim3(EIG_THREADS), 0, s, z.blk[2], z.s, z.theta, z.resv, z.state, N, m, k, evals, evecs, res,
                       info);
    DVM_CHECK_LAUNCH("eigenbasis (output)");
    return DVM_OK;
}

DVM_EXPORT size_t dvm_basis_project_workspace_bytes(int B, int N, int k, int C) {
    return project_limits(B, N, k, C) ? 0 : align_up((size_t)B * tn_chunks(N) * k * C * sizeof(double));
}

DVM_EXPORT int dvm_basis_project_f64(const double *evecs, const float *mass, const float *Y, int B, int N, int k, int C, double *out, void *ws,
                                     size_t ws_bytes, void *stream) {
    const char *who = "dvm_basis_project_f64";
    DVM_REQUIRE(evecs && Y && out, "%s: null pointer", who);
    const char *why = project_limits(B, N, k, C);
    DVM_REQUIRE(!why, "%s", why);
    const size_t need = dvm_basis_project_workspace_bytes(B, N, k, C);
    if (!ws || ws_bytes < need) {
        set_error("%s: workspace too small (%zu < %zu)", who, ws ? ws_bytes : (size_t)0, need);
        return DVM_ENOSPACE;
    }
    launch_tn<float>(evecs, k, Y, C, N, nullptr, mass, B, N, k, C, (double *)ws, out, nullptr, 0, (hipStream_t)stream);
    DVM_CHECK_LAUNCH("basis_project");
    return DVM_OK;
}
