// dvm_zoomout.hip — ZoomOut spectral refinement (the reference's Tools/utils.py: pMap2fMap, fMap2pMap, zo_fmap, there a cKDTree
// query and a dense pseudo-inverse on the host per step): point map -> functional map, functional map -> point map, and the loop
// of the two over a growing basis.  float64 throughout; the definitions are in include/dvm.h.
//
// Kernels.  The two tall-skinny products (Phi_X^T diag(m) Phi_Y[T] and the Gram matrix Phi_X^T Phi_X) are eig_tn_kernel /
// eig_reduce_kernel of dvm_dense64.h with the gather fused into the staging: one fixed summation order.  zo_solve_kernel: one
// workgroup per element, the scaled Cholesky factor of the Gram matrix in LDS (chol_scaled_lds, as the eigenbasis' Cholesky-QR),
// then a forward and a backward substitution with one right-hand-side column per thread, the column kept in global memory.
// zo_embed_kernel: E = Phi_Y C^T, 16 rows per workgroup in LDS, one FMA accumulator per entry.
// zo_nn_kernel, the hot path: every pair's distance in the exact sequential form (sub, mul, add each rounded: the library is
// built with -ffp-contract=off).  A workgroup owns ZO_TN = 64 source rows, held transposed in LDS for the whole launch, and one
// segment of the target; target rows come in tiles of ZO_TM = 64 rows and panels of ZO_KC = 16 coordinates (the next panel is in
// registers while the current one is used).  16 x 16 threads with a 4 x 4 register tile of pairs each: per coordinate 8 LDS
// reads of 8 bytes (the source reads are broadcasts, the target reads 16 consecutive doubles per half-wave) for 48 VALU operations.
// A thread keeps a running (d, j) per source row (strict <, j ascending: the lowest index stays); the 16 threads of a row and then
// the segments (zo_merge_kernel) merge by the total order (d, j).  A NaN distance never compares below anything, so it never wins;
// a row without a finite distance keeps (+inf, 0).  Trailing coordinates of the last panel are zeros on both sides: t = 0 adds +0.
//
// info [B][4] int32 is also the loop's state: every kernel leaves at once when its element's status is set.
#include "dvm_dense64.h"

namespace dvm {
namespace {

constexpr int ZO_THREADS = 256;
constexpr int ZO_TN = 64, ZO_TM = 64, ZO_KC = 16;
constexpr int ZO_LDT = ZO_TN + 1;      // row stride of the transposed tiles in LDS (doubles): staging writes hit distinct banks
constexpr int ZO_TARGET_WGS = 512;     // the target is split into segments until a launch has about this many workgroups
constexpr int ZO_MAX_SEGS = 64;
constexpr int ZO_ER = 16;              // rows per workgroup of zo_embed_kernel
enum { ZI_STATUS = 0, ZI_K = 1, ZI_OUTSIDE = 2, ZI_STEPS = 3, ZI_WORDS = 4 };
static_assert(ZO_TN == ZO_TM && ZO_TN * ZO_KC == 4 * ZO_THREADS, "the staging maps below");

// info[b] = {0, 0, entries of T[b] outside [0, M), 0}
__global__ __launch_bounds__(ZO_THREADS) void zo_init_kernel(const int32_t *__restrict__ T, int N, int M, int32_t *__restrict__ info) {
    __shared__ int cnt[ZO_THREADS];
    const int b = blockIdx.x, tid = threadIdx.x;
    int n = 0;
    for (int i = tid; i < N; i += ZO_THREADS) n += (unsigned)T[(size_t)b * N + i] >= (unsigned)M ? 1 : 0;
    cnt[tid] = n;
    __syncthreads();
    for (int o = ZO_THREADS / 2; o > 0; o >>= 1) {
        if (tid < o) cnt[tid] += cnt[tid + o];
        __syncthreads();
    }
    if (tid == 0) {
        int32_t *st = info + (size_t)b * ZI_WORDS;
        st[ZI_STATUS] = 0;
        st[ZI_K] = 0;
        st[ZI_OUTSIDE] = cnt[0];
        st[ZI_STEPS] = 0;
    }
}

// (G C = X) in place: G [k][k] the Gram matrix, X [k][k] the right-hand sides on entry and C on exit.  A pivot of the unit-diagonal
// matrix that is not a finite number above k 2^-52 (a column that depends on the earlier ones, to rounding: with two equal columns
// the second pivot is x - (x / sqrt x)^2, a few 2^-53 either side of 0) sets status 1 and the failing k, and fills
// Cfail [kfail][kfail] with NaN.
__global__ __launch_bounds__(ZO_THREADS) void zo_solve_kernel(const double *__restrict__ G, double *X, int k, int32_t *__restrict__ info,
                                                              double *Cfail, int kfail) {
    extern __shared__ double lds[];
    __shared__ double dsc[EIG_MAX_M];
    __shared__ int bad;
    const int b = blockIdx.x, tid = threadIdx.x;
    if (info[(size_t)b * ZI_WORDS + ZI_STATUS]) return;
    if (!chol_scaled_lds(G + (size_t)b * k * k, k, lds, dsc, &bad, (double)k * 0x1p-52)) {
        if (tid == 0) {
            info[(size_t)b * ZI_WORDS + ZI_STATUS] = 1;
            info[(size_t)b * ZI_WORDS + ZI_K] = k;
        }
        for (int e = tid; e < kfail * kfail; e += ZO_THREADS) Cfail[(size_t)b * kfail * kfail + e] = NAN;
        return;
    }
    if (tid >= k) return;
    // (D G D)(D^-1 C) = D X: column `tid` of L z = D x, then of L^T w = z, then c = D w
    double *x = X + (size_t)b * k * k + tid;
    for (int i = 0; i < k; ++i) {
        double acc = dsc[i] * x[(size_t)i * k];
        for (int j = 0; j < i; ++j) acc -= lds[i * k + j] * x[(size_t)j * k];
        x[(size_t)i * k] = acc / lds[i * k + i];
    }
    for (int i = k - 1; i >= 0; --i) {
        double acc = x[(size_t)i * k];
        for (int j = i + 1; j < k; ++j) acc -= lds[j * k + i] * x[(size_t)j * k];
        x[(size_t)i * k] = acc / lds[i * k + i];
    }
    for (int i = 0; i < k; ++i) x[(size_t)i * k] *= dsc[i];
}

// E[j][c] = sum over a, ascending, of Y[j][a] C[c][a]: a thread owns 4 rows x columns (tq, tq + 64)
__global__ __launch_bounds__(ZO_THREADS) void zo_embed_kernel(const double *__restrict__ Y, int ldy, const double *__restrict__ C, int M, int k,
                                                              double *__restrict__ E, int lde, const int32_t *__restrict__ skip) {
    const int b = blockIdx.y, tid = threadIdx.x;
    if (skip && skip[(size_t)b * ZI_WORDS + ZI_STATUS]) return;
    __shared__ double sY[ZO_ER][EIG_MAX_M];
    const int r0 = blockIdx.x * ZO_ER;
    const double *Yb = Y + (size_t)b * M * ldy;
    const double *Cb = C + (size_t)b * k * k;
    for (int e = tid; e < ZO_ER * EIG_MAX_M; e += ZO_THREADS) {
        const int r = r0 + e / EIG_MAX_M, c = e % EIG_MAX_M;
        sY[e / EIG_MAX_M][c] = (r < M && c < k) ? Yb[(size_t)r * ldy + c] : 0.0;
    }
    __syncthreads();
    const int tq = tid % 64, tr = tid / 64;
    const bool c0 = tq < k, c1 = tq + 64 < k;
    const double *C0 = Cb + (size_t)(c0 ? tq : 0) * k, *C1 = Cb + (size_t)(c1 ? tq + 64 : 0) * k;
    double acc0[4] = {0.0, 0.0, 0.0, 0.0}, acc1[4] = {0.0, 0.0, 0.0, 0.0};
    for (int a = 0; a < k; ++a) {
        const double t0 = C0[a], t1 = C1[a];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const double y = sY[tr * 4 + r][a];
            acc0[r] = fma(y, t0, acc0[r]);
            acc1[r] = fma(y, t1, acc1[r]);
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = r0 + tr * 4 + r;
        if (row < M) {
            if (c0) E[((size_t)b * M + row) * lde + tq] = acc0[r];
            if (c1) E[((size_t)b * M + row) * lde + tq + 64] = acc1[r];
        }
    }
}

// the segment winners: segd / segj [B][segments][N] = min over the segment's columns j of (d(i, j), j)
__global__ __launch_bounds__(ZO_THREADS) void zo_nn_kernel(const double *__restrict__ A, int lda, const double *__restrict__ E, int lde, int N, int M,
                                                           int k, int seg_len, double *__restrict__ segd, int32_t *__restrict__ segj,
                                                           const int32_t *__restrict__ skip) {
    extern __shared__ double lds[];   // sA [kp][ZO_LDT], sE [ZO_KC][ZO_LDT]
    const int b = blockIdx.z, seg = blockIdx.y, tid = threadIdx.x;
    if (skip && skip[(size_t)b * ZI_WORDS + ZI_STATUS]) return;
    const int kp = (k + ZO_KC - 1) / ZO_KC * ZO_KC;
    double *sA = lds, *sE = lds + kp * ZO_LDT;
    const int i0 = blockIdx.x * ZO_TN;
    const double *Ab = A + (size_t)b * N * lda;
    const double *Eb = E + (size_t)b * M * lde;
    for (int e = tid; e < ZO_TN * kp; e += ZO_THREADS) {
        const int r = e / kp, c = e % kp, i = i0 + r;
        sA[c * ZO_LDT + r] = (i < N && c < k) ? Ab[(size_t)i * lda + c] : 0.0;
    }
    const int tx = tid % 16, ty = tid / 16;
    double best[4];
    int bj[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        best[u] = INFINITY;
        bj[u] = 0;
    }
    const int j_beg = seg * seg_len, j_end = min(j_beg + seg_len, M);
    // a panel's staging map: element tid + 256 q is (target row pr + 16 q of the tile, coordinate pc of the panel)
    const int pr = tid / ZO_KC, pc = tid % ZO_KC;
    for (int j0 = j_beg; j0 < j_end; j0 += ZO_TM) {
        double acc[4][4], pre[4];
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int v = 0; v < 4; ++v) acc[u][v] = 0.0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int j = j0 + pr + 16 * q;
            pre[q] = (j < j_end && pc < k) ? Eb[(size_t)j * lde + pc] : 0.0;
        }
        for (int c0 = 0; c0 < kp; c0 += ZO_KC) {
            __syncthreads();   // the previous panel has been read (first pass: nothing yet)
#pragma unroll
            for (int q = 0; q < 4; ++q) sE[pc * ZO_LDT + pr + 16 * q] = pre[q];
            __syncthreads();   // (also orders the staging of sA before its first use)
            if (c0 + ZO_KC < kp) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int j = j0 + pr + 16 * q, c = c0 + ZO_KC + pc;
                    pre[q] = (j < j_end && c < k) ? Eb[(size_t)j * lde + c] : 0.0;
                }
            }
            const double *pa = sA + c0 * ZO_LDT + ty, *pe = sE + tx;
#pragma unroll
            for (int cc = 0; cc < ZO_KC; ++cc) {
                double av[4], ev[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) av[u] = pa[cc * ZO_LDT + 16 * u];
#pragma unroll
                for (int v = 0; v < 4; ++v) ev[v] = pe[cc * ZO_LDT + 16 * v];
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int v = 0; v < 4; ++v) {
                        const double t = ev[v] - av[u];
                        acc[u][v] = acc[u][v] + t * t;
                    }
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int j = j0 + tx + 16 * v;
                if (j < j_end && acc[u][v] < best[u]) {   // j ascends within a thread: the first of equal distances stays
                    best[u] = acc[u][v];
                    bj[u] = j;
                }
            }
    }
    // the 16 threads of a source row, by (d, j); the tiles are free now (kp + ZO_KC >= 32 rows of 520 bytes > 12 KB)
    __syncthreads();
    double *md = lds;
    int *mj = (int *)(lds + ZO_TN * 16);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        md[(ty + 16 * u) * 16 + tx] = best[u];
        mj[(ty + 16 * u) * 16 + tx] = bj[u];
    }
    __syncthreads();
    if (tid < ZO_TN && i0 + tid < N) {
        double d = md[tid * 16];
        int j = mj[tid * 16];
        for (int x = 1; x < 16; ++x) {
            const double dx = md[tid * 16 + x];
            const int jx = mj[tid * 16 + x];
            if (dx < d || (dx == d && jx < j)) {
                d = dx;
                j = jx;
            }
        }
        const size_t at = ((size_t)b * gridDim.y + seg) * N + i0 + tid;
        segd[at] = d;
        segj[at] = j;
    }
}

// T[i] / dmin[i] = the least (d, j) over the segments; the loop's NN step counter
__global__ __launch_bounds__(ZO_THREADS) void zo_merge_kernel(const double *__restrict__ segd, const int32_t *__restrict__ segj, int nseg, int N,
                                                              int32_t *__restrict__ T, double *__restrict__ dmin, int32_t *__restrict__ info) {
    const int b = blockIdx.y, i = blockIdx.x * ZO_THREADS + threadIdx.x;
    if (info && info[(size_t)b * ZI_WORDS + ZI_STATUS]) return;
    if (info && i == 0) info[(size_t)b * ZI_WORDS + ZI_STEPS] += 1;
    if (i >= N) return;
    double d = segd[(size_t)b * nseg * N + i];
    int j = segj[(size_t)b * nseg * N + i];
    for (int s = 1; s < nseg; ++s) {
        const double ds = segd[((size_t)b * nseg + s) * N + i];
        const int js = segj[((size_t)b * nseg + s) * N + i];
        if (ds < d || (ds == d && js < j)) {
            d = ds;
            j = js;
        }
    }
    T[(size_t)b * N + i] = j;
    if (dmin) dmin[(size_t)b * N + i] = d;
}

struct NnPlan {
    int segments, seg_len;
};
static NnPlan nn_plan(int B, int N, int M) {
    const long long rows = (long long)((N + ZO_TN - 1) / ZO_TN) * B;
    const int mt = (M + ZO_TM - 1) / ZO_TM;
    long long want = (ZO_TARGET_WGS + rows - 1) / rows;
    if (want > ZO_MAX_SEGS) want = ZO_MAX_SEGS;
    if (want > mt) want = mt;
    if (want < 1) want = 1;
    const int seg_tiles = (mt + (int)want - 1) / (int)want;
    return NnPlan{(mt + seg_tiles - 1) / seg_tiles, seg_tiles * ZO_TM};
}

}  // namespace
}  // namespace dvm

using namespace dvm;

#define ZO_LIMIT(cond, ...)                     \
    if (!(cond)) {                              \
        snprintf(msg, sizeof msg, __VA_ARGS__); \
        return msg;                             \
    }
// the limits every entry shares: B, the two vertex counts (rows2 = 1 where an entry has one shape only) and k
static const char *zo_limits(const char *who, int B, int N, int M, int k) {
    static thread_local char msg[200];
    ZO_LIMIT(B >= 1 && B <= 65535, "%s: B=%d unsupported (1..65535)", who, B);
    ZO_LIMIT(N >= 1 && N <= EIG_MAX_N && M >= 1 && M <= EIG_MAX_N, "%s: N=%d M=%d unsupported (1..%d)", who, N, M, EIG_MAX_N);
    ZO_LIMIT(k >= 1 && k <= EIG_MAX_M, "%s: k=%d unsupported (1..%d)", who, k, EIG_MAX_M);
    return nullptr;
}
static const char *zo_loop_limits(const char *who, int B, int N, int M, int ldx, int ldy, int k_init, int k_final, int k_step, int n_inter, int mode) {
    static thread_local char msg[200];
    const char *why = zo_limits(who, B, N, M, k_final);
    if (why) return why;
    ZO_LIMIT(k_init >= 1 && k_init <= k_final, "%s: k_init=%d unsupported (1..k_final=%d)", who, k_init, k_final);
    ZO_LIMIT(k_final <= ldx && k_final <= ldy, "%s: k_final=%d exceeds a basis' leading dimension (%d, %d)", who, k_final, ldx, ldy);
    ZO_LIMIT(k_step >= 1 && n_inter >= 1, "%s: k_step=%d n_inter=%d unsupported (both >= 1)", who, k_step, n_inter);
    ZO_LIMIT(mode == 0 || mode == 1, "%s: mode=%d unsupported (0 adjoint, 1 lstsq)", who, mode);
    return nullptr;
}
#undef ZO_LIMIT

struct FromWs {
    double *part, *G;
};
static size_t carve_from(Arena &ar, int B, int N, int k, int mode, FromWs &w) {
    w.part = ar.take<double>((size_t)B * tn_chunks(N) * k * k);
    w.G = mode ? ar.take<double>((size_t)B * k * k) : nullptr;
    return ar.off;
}
struct NnWs {
    double *segd;
    int32_t *segj;
};
static size_t carve_nn(Arena &ar, int B, int N, int M, NnWs &w) {
    const size_t n = (size_t)B * nn_plan(B, N, M).segments * N;
    w.segd = ar.take<double>(n);
    w.segj = ar.take<int32_t>(n);
    return ar.off;
}
struct ToWs {
    double *E;
    NnWs nn;
};
static size_t carve_to(Arena &ar, int B, int N, int M, int k, ToWs &w) {
    w.E = ar.take<double>((size_t)B * M * k);
    return carve_nn(ar, B, N, M, w.nn);
}
struct LoopWs {
    double *C;
    FromWs from;
    ToWs to;
};
static size_t carve_loop(Arena &ar, int B, int N, int M, int k, int mode, LoopWs &w) {
    w.C = ar.take<double>((size_t)B * k * k);
    carve_from(ar, B, N, k, mode, w.from);
    return carve_to(ar, B, N, M, k, w.to);
}

// C = from_pmap(T) at k columns; a failing element fills Cfail [kfail][kfail]
static void enqueue_from(const double *phi_x, int ldx, const float *mass, const double *phi_y, int ldy, const int32_t *T, int B, int N, int M, int k,
                         int mode, double *C, int32_t *info, double *Cfail, int kfail, const FromWs &w, hipStream_t s) {
    if (mode == 0) {
        launch_tn<double>(phi_x, ldx, phi_y, ldy, M, T, mass, B, N, k, k, w.part, C, info, ZI_WORDS, s);
        return;
    }
    launch_tn<double>(phi_x, ldx, phi_x, ldx, N, nullptr, nullptr, B, N, k, k, w.part, w.G, info, ZI_WORDS, s);
    launch_tn<double>(phi_x, ldx, phi_y, ldy, M, T, nullptr, B, N, k, k, w.part, C, info, ZI_WORDS, s);
    ensure_dyn_lds((const void *)zo_solve_kernel, EIG_MAX_M * EIG_MAX_M * (int)sizeof(double));
    hipLaunchKernelGGL(zo_solve_kernel, dim3(B), dim3(ZO_THREADS), (size_t)k * k * sizeof(double), s, w.G, C, k, info, Cfail, kfail);
}
static void enqueue_embed(const double *phi_y, int ldy, const double *C, int B, int M, int k, double *E, int lde, const int32_t *skip, hipStream_t s) {
    hipLaunchKernelGGL(zo_embed_kernel, dim3((M + ZO_ER - 1) / ZO_ER, B), dim3(ZO_THREADS), 0, s, phi_y, ldy, C, M, k, E, lde, skip);
}
static void enqueue_nn(const double *A, int lda, const double *E, int lde, int B, int N, int M, int k, int32_t *T, double *dmin, int32_t *info,
                       const NnWs &w, hipStream_t s) {
    const NnPlan pl = nn_plan(B, N, M);
    const int kp = (k + ZO_KC - 1) / ZO_KC * ZO_KC;
    ensure_dyn_lds((const void *)zo_nn_kernel, (EIG_MAX_M + ZO_KC) * ZO_LDT * (int)sizeof(double));
    hipLaunchKernelGGL(zo_nn_kernel, dim3((N + ZO_TN - 1) / ZO_TN, pl.segments, B), dim3(ZO_THREADS), (size_t)(kp + ZO_KC) * ZO_LDT * sizeof(double), s,
                       A, lda, E, lde, N, M, k, pl.seg_len, w.segd, w.segj, info);
    hipLaunchKernelGGL(zo_merge_kernel, dim3((N + ZO_THREADS - 1) / ZO_THREADS, B), dim3(ZO_THREADS), 0, s, w.segd, w.segj, pl.segments, N, T, dmin,
                       info);
}

DVM_EXPORT size_t dvm_fmap_from_pmap_workspace_bytes(int B, int N, int M, int k, int mode) {
    return (zo_limits("dvm_fmap_from_pmap_f64", B, N, M, k) || (mode != 0 && mode != 1)) ? 0 : null_carve<FromWs>(carve_from, B, N, k, mode);
}

DVM_EXPORT int dvm_fmap_from_pmap_f64(const double *phi_x, int ldx, const float *mass, const double *phi_y, int ldy, const int32_t *T, int B, int N,
                                      int M, int k, int mode, double *C, int32_t *info, void *ws, size_t ws_bytes, void *stream) {
    const char *who = "dvm_fmap_from_pmap_f64";
    DVM_REQUIRE(phi_x && phi_y && T && C && info, "%s: null pointer", who);
    const char *why = zo_loop_limits(who, B, N, M, ldx, ldy, k, k, 1, 1, mode);
    DVM_REQUIRE(!why, "%s", why);
    FromWs w;
    if (!carve_ws(ws, ws_bytes, who, w, carve_from, B, N, k, mode)) return DVM_ENOSPACE;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(zo_init_kernel, dim3(B), dim3(ZO_THREADS), 0, s, T, N, M, info);
    enqueue_from(phi_x, ldx, mass, phi_y, ldy, T, B, N, M, k, mode, C, info, C, k, w, s);
    DVM_CHECK_LAUNCH("fmap_from_pmap");
    return DVM_OK;
}

DVM_EXPORT int dvm_fmap_embed_f64(const double *phi_y, int ldy, const double *C, int B, int M, int k, double *E, int lde, void *stream) {
    const char *who = "dvm_fmap_embed_f64";
    DVM_REQUIRE(phi_y && C && E, "%s: null pointer", who);
    const char *why = zo_limits(who, B, 1, M, k);
    DVM_REQUIRE(!why, "%s", why);
    DVM_REQUIRE(k <= ldy && k <= lde, "%s: k=%d exceeds a leading dimension (ldy=%d, lde=%d)", who, k, ldy, lde);
    enqueue_embed(phi_y, ldy, C, B, M, k, E, lde, nullptr, (hipStream_t)stream);
    DVM_CHECK_LAUNCH("fmap_embed");
    return DVM_OK;
}

DVM_EXPORT int dvm_spectral_nn_plan(int B, int N, int M, int k, int32_t *plan) {
    const char *who = "dvm_spectral_nn_plan";
    DVM_REQUIRE(plan, "%s: null pointer", who);
    const char *why = zo_limits(who, B, N, M, k);
    DVM_REQUIRE(!why, "%s", why);
    const NnPlan pl = nn_plan(B, N, M);
    plan[0] = ZO_TN;
    plan[1] = ZO_TM;
    plan[2] = pl.segments;
    plan[3] = pl.seg_len;
    return DVM_OK;
}

DVM_EXPORT size_t dvm_spectral_nn_workspace_bytes(int B, int N, int M, int k) {
    return zo_limits("dvm_spectral_nn_f64", B, N, M, k) ? 0 : null_carve<NnWs>(carve_nn, B, N, M);
}

DVM_EXPORT int dvm_spectral_nn_f64(const double *A, int lda, const double *E, int lde, int B, int N, int M, int k, int32_t *T, double *dmin, void *ws,
                                   size_t ws_bytes, void *stream) {
    const char *who = "dvm_spectral_nn_f64";
    DVM_REQUIRE(A && E && T, "%s: null pointer", who);
    const char *why = zo_limits(who, B, N, M, k);
    DVM_REQUIRE(!why, "%s", why);
    DVM_REQUIRE(k <= lda && k <= lde, "%s: k=%d exceeds a leading dimension (lda=%d, lde=%d)", who, k, lda, lde);
    NnWs w;
    if (!carve_ws(ws, ws_bytes, who, w, carve_nn, B, N, M)) return DVM_ENOSPACE;
    enqueue_nn(A, lda, E, lde, B, N, M, k, T, dmin, nullptr, w, (hipStream_t)stream);
    DVM_CHECK_LAUNCH("spectral_nn");
    return DVM_OK;
}

DVM_EXPORT size_t dvm_fmap_to_pmap_workspace_bytes(int B, int N, int M, int k) {
    return zo_limits("dvm_fmap_to_pmap_f64", B, N, M, k) ? 0 : null_carve<ToWs>(carve_to, B, N, M, k);
}

DVM_EXPORT int dvm_fmap_to_pmap_f64(const double *phi_x, int ldx, const double *phi_y, int ldy, const double *C, int B, int N, int M, int k,
                                    int32_t *T, double *dmin, double *E_out, void *ws, size_t ws_bytes, void *stream) {
    const char *who = "dvm_fmap_to_pmap_f64";
    DVM_REQUIRE(phi_x && phi_y && C && T, "%s: null pointer", who);
    const char *why = zo_loop_limits(who, B, N, M, ldx, ldy, k, k, 1, 1, 0);
    DVM_REQUIRE(!why, "%s", why);
    ToWs w;
    if (!carve_ws(ws, ws_bytes, who, w, carve_to, B, N, M, k)) return DVM_ENOSPACE;
    hipStream_t s = (hipStream_t)stream;
    enqueue_embed(phi_y, ldy, C, B, M, k, w.E, k, nullptr, s);
    enqueue_nn(phi_x, ldx, w.E, k, B, N, M, k, T, dmin, nullptr, w.nn, s);
    if (E_out && hipMemcpyAsync(E_out, w.E, (size_t)B * M * k * sizeof(double), hipMemcpyDeviceToDevice, s) != hipSuccess) {
        set_error("%s: copying the embedding out failed: %s", who, hipGetErrorString(hipGetLastError()));
        return DVM_ELAUNCH;
    }
    DVM_CHECK_LAUNCH("fmap_to_pmap");
    return DVM_OK;
}

DVM_EXPORT size_t dvm_zoomout_workspace_bytes(int B, int N, int M, int k_init, int k_final, int k_step, int n_inter, int mode) {
    return zo_loop_limits("dvm_zoomout_f64", B, N, M, k_final, k_final, k_init, k_final, k_step, n_inter, mode)
               ? 0
               : null_carve<LoopWs>(carve_loop, B, N, M, k_final, mode);
}

DVM_EXPORT int dvm_zoomout_f64(const double *phi_x, int ldx, const float *mass, const double *phi_y, int ldy, const int32_t *T0, int B, int N, int M,
                               int k_init, int k_final, int k_step, int n_inter, int mode, double *C, int32_t *T, int32_t *info, void *ws,
                               size_t ws_bytes, void *stream) {
    const char *who = "dvm_zoomout_f64";
    DVM_REQUIRE(phi_x && phi_y && T0 && C && T && info, "%s: null pointer", who);
    const char *why = zo_loop_limits(who, B, N, M, ldx, ldy, k_init, k_final, k_step, n_inter, mode);
    DVM_REQUIRE(!why, "%s", why);
    LoopWs w;
    if (!carve_ws(ws, ws_bytes, who, w, carve_loop, B, N, M, k_final, mode)) return DVM_ENOSPACE;
    hipStream_t s = (hipStream_t)stream;
    if (T != T0 && hipMemcpyAsync(T, T0, (size_t)B * N * sizeof(int32_t), hipMemcpyDeviceToDevice, s) != hipSuccess) {
        set_error("%s: copying the start map failed: %s", who, hipGetErrorString(hipGetLastError()));
        return DVM_ELAUNCH;
    }
    hipLaunchKernelGGL(zo_init_kernel, dim3(B), dim3(ZO_THREADS), 0, s, T0, N, M, info);
    // the schedule is the host's: an element that fails skips its remaining launches on the device (info's status)
    for (int k = k_init; k < k_final; k += k_step)
        for (int it = 0; it < n_inter; ++it) {
            enqueue_from(phi_x, ldx, mass, phi_y, ldy, T, B, N, M, k, mode, w.C, info, C, k_final, w.from, s);
            enqueue_embed(phi_y, ldy, w.C, B, M, k, w.to.E, k, info, s);
            enqueue_nn(phi_x, ldx, w.to.E, k, B, N, M, k, T, nullptr, info, w.to.nn, s);
            DVM_CHECK_LAUNCH("zoomout (step)");
        }
    enqueue_from(phi_x, ldx, mass, phi_y, ldy, T, B, N, M, k_final, mode, C, info, C, k_final, w.from, s);
    DVM_CHECK_LAUNCH("zoomout");
    return DVM_OK;
}
