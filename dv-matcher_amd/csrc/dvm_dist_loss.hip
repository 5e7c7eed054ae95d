// dvm_dist_loss.hip — K10, the dist-loss term of LG-Net's criterion and the weights of its backward.
// Reference: models/loss.py:1351-1396 (dist loss), 451-462 (its knn: dvm_knn.hip).
// per (b, anchor n): x_j = |feat[idx_j] - feat[a_n]|_2, y_j = dist[b, idx_j, a_n], j < k;
// term = 1 - |cos(x, y)|;  out[b] = sum_n term.   One wave per (b, n), k <= 512: lane l keeps x_j, y_j of j = l + 64 u, u < 8, in
// xs[u] / ys[u] (0 past k).  The forward works in float32; the backward weights form x_j again in float64 (see dist_x_f64_128), in
// the same lane layout, and differ among their forms only in where y_j comes from, so that the forms agree bit for bit.
#include "dvm_mfma_tile.h"

namespace dvm {

enum DistRows { DIST_ROWS_128, DIST_ROWS_GENERIC, DIST_ROWS_SAVED };   // C == 128 half-wave form | any C % 4 == 0 | the forward's xsave

// any C % 4 == 0: a lane streams its own rows, 16 bytes per instruction
__device__ __forceinline__ void dist_rows_generic(const float *__restrict__ featb, const float *__restrict__ distb, int N, int C, int a,
                                                  const int32_t *__restrict__ ix, int k, int lane, float (&xs)[8], float (&ys)[8]) {
    const float *fa = featb + (size_t)a * C;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int j = lane + 64 * u;
        xs[u] = ys[u] = 0.f;
        if (j < k) {
            const int v = ix[j];
            const float *fv = featb + (size_t)v * C;
            float s2 = 0.f;
            for (int c = 0; c < C; c += 4) {
                f32x4 p = *(const f32x4 *)(fv + c), q = *(const f32x4 *)(fa + c);
                float d0 = p.x - q.x, d1 = p.y - q.y, d2 = p.z - q.z, d3 = p.w - q.w;
                s2 = fmaf(d0, d0, s2);
                s2 = fmaf(d1, d1, s2);
                s2 = fmaf(d2, d2, s2);
                s2 = fmaf(d3, d3, s2);
            }
            xs[u] = sqrt_rn(s2);
            ys[u] = distb[(size_t)v * N + a];
        }
    }
}

// C = 128 (LG-Net's feature width), k <= 512: dist_rows_generic's 64 lanes stream 64 DIFFERENT rows, 16 bytes
// each per instruction — 64 cache lines per load, every line fetched 8 times (0.55 ms per call at 8 x 1000 anchors x 500
// neighbours).  Here a 32-lane half reads ONE whole row per instruction (512 contiguous bytes), the half's partial sums
// are combined on the DPP network, and lane j % 64 keeps x_j, so that what follows is the same arithmetic.
__device__ __forceinline__ void dist_rows128(const float *__restrict__ featb, const float *__restrict__ distb, int N, int a,
                                             const int32_t *__restrict__ ix, int k, int lane, float (&xs)[8], float (&ys)[8]) {
    const int half = lane >> 5, l = lane & 31;
    const f32x4 q = *(const f32x4 *)(featb + (size_t)a * 128 + 4 * l);
    int ixl[8];   // this lane's neighbour indices: j = lane + 64 u (clamped, not predicated: the loads go out together)
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int j = lane + 64 * u;
        ixl[u] = ix[j < k ? j : k - 1];
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {   // the geodesic column entries: scattered 4-byte reads, all requested up front
        const int j = lane + 64 * u;
        const float y = distb[(size_t)ixl[u] * N + a];
        xs[u] = 0.f;
        ys[u] = j < k ? y : 0.f;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        if (64 * u >= k) break;
#pragma unroll 4
        for (int jj = 0; jj < 64; jj += 2) {
            if (64 * u + jj >= k) break;
            const int j = 64 * u + jj + half;
            // neighbour j's index from the lane that holds it (no load in the loop: the row gathers of an unrolled group are
            // independent and go out together)
            const int v0 = __builtin_amdgcn_readlane(ixl[u], jj), v1 = __builtin_amdgcn_readlane(ixl[u], jj + 1);
            const int v = half ? v1 : v0;
            const f32x4 p = *(const f32x4 *)(featb + (size_t)v * 128 + 4 * l);
            const float d0 = p.x - q.x, d1 = p.y - q.y, d2 = p.z - q.z, d3 = p.w - q.w;
            float s2 = d0 * d0;
            s2 = fmaf(d1, d1, s2);
            s2 = fmaf(d2, d2, s2);
            s2 = fmaf(d3, d3, s2);
            s2 = sum32(s2);
            const float x = j < k ? sqrt_rn(s2) : 0.f;
            const float o = lane_xor32(x);
            if (lane == jj) xs[u] = half ? o : x;
            if (lane == jj + 1) xs[u] = half ? x : o;
        }
    }
}

// cos(x, y) of a wave's k pairs: per lane the three fmaf chains over u = 0..7 (the slots past k add +0 to sums that are never -0),
// wave_sum, norms floored at 1e-8
__device__ __forceinline__ float dist_cos(const float (&xs)[8], const float (&ys)[8], float &nx, float &ny) {
    float sxy = 0.f, sxx = 0.f, syy = 0.f;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        sxy = fmaf(xs[u], ys[u], sxy);
        sxx = fmaf(xs[u], xs[u], sxx);
        syy = fmaf(ys[u], ys[u], syy);
    }
    sxy = wave_sum(sxy);
    sxx = wave_sum(sxx);
    syy = wave_sum(syy);
    nx = fmaxf(sqrt_rn(sxx), 1e-8f), ny = fmaxf(sqrt_rn(syy), 1e-8f);
    return sxy / (nx * ny);
}
// The backward weights in float64.  y_j / (|x||y|) - cos x_j / |x|^2 cancels where cos(x, y) is near 1, and the float32 rounding of x_j
// itself is then amplified by 1 / (1 - cos) (per-row errors of 1e-5 .. 7e-4 of the feature gradient's row maximum at N = 64 .. 516,
// profiles/notes_wgrad_elements.md).  So the backward forms x_j again from the feature rows — differences, squares, sum and root in
// float64, exact up to the last root — and W is rounded to float32 once.  The forward's term stays on its float32 x_j, bit for bit.
__device__ __forceinline__ double dist_sq4_f64(const f32x4 &p, const f32x4 &q, double s2) {
    const double d0 = (double)p.x - (double)q.x, d1 = (double)p.y - (double)q.y, d2 = (double)p.z - (double)q.z, d3 = (double)p.w - (double)q.w;
    s2 = fma(d0, d0, s2);
    s2 = fma(d1, d1, s2);
    s2 = fma(d2, d2, s2);
    return fma(d3, d3, s2);
}
// any C % 4 == 0: dist_rows_generic's walk
__device__ __forceinline__ void dist_x_f64_generic(const float *__restrict__ featb, int C, int a, const int32_t *__restrict__ ix, int k, int lane,
                                                   double (&xd)[8]) {
    const float *fa = featb + (size_t)a * C;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int j = lane + 64 * u;
        xd[u] = 0.0;
        if (j < k) {
            const float *fv = featb + (size_t)ix[j] * C;
            double s2 = 0.0;
            for (int c = 0; c < C; c += 4) s2 = dist_sq4_f64(*(const f32x4 *)(fv + c), *(const f32x4 *)(fa + c), s2);
            xd[u] = sqrt(s2);
        }
    }
}
// C = 128: dist_rows128's walk (a 32-lane half reads one whole row, lane j % 64 keeps x_j)
__device__ __forceinline__ void dist_x_f64_128(const float *__restrict__ featb, int a, const int32_t *__restrict__ ix, int k, int lane,
                                               double (&xd)[8]) {
    const int half = lane >> 5, l = lane & 31;
    const f32x4 q = *(const f32x4 *)(featb + (size_t)a * 128 + 4 * l);
    int ixl[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int j = lane + 64 * u;
        ixl[u] = ix[j < k ? j : k - 1];
        xd[u] = 0.0;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        if (64 * u >= k) break;
#pragma unroll 4
        for (int jj = 0; jj < 64; jj += 2) {
            if (64 * u + jj >= k) break;
            const int j = 64 * u + jj + half;
            const int v0 = __builtin_amdgcn_readlane(ixl[u], jj), v1 = __builtin_amdgcn_readlane(ixl[u], jj + 1);
            const int v = half ? v1 : v0;
            double s2 = dist_sq4_f64(*(const f32x4 *)(featb + (size_t)v * 128 + 4 * l), q, 0.0);
#pragma unroll
            for (int o = 16; o > 0; o >>= 1) s2 += __shfl_xor(s2, o, 64);   // within the 32-lane half
            const double x = j < k ? sqrt(s2) : 0.0;
            const double o = __shfl_xor(x, 32, 64);
            if (lane == jj) xd[u] = half ? o : x;
            if (lane == jj + 1) xd[u] = half ? x : o;
        }
    }
}
__device__ __forceinline__ double dist_cos(const double (&xs)[8], const float (&ys)[8], double &nx, double &ny) {
    double sxy = 0.0, sxx = 0.0, syy = 0.0;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const double y = (double)ys[u];
        sxy = fma(xs[u], y, sxy);
        sxx = fma(xs[u], xs[u], sxx);
        syy = fma(y, y, syy);
    }
    sxy = wave_sum(sxy);
    sxx = wave_sum(sxx);
    syy = wave_sum(syy);
    nx = fmax(sqrt(sxx), 1e-8), ny = fmax(sqrt(syy), 1e-8);   // the same floor as the float32 cosine
    return sxy / (nx * ny);
}
// W[b, n, idx_j] = g * d term / d x_j / x_j for x_j > 0, with d term / d x_j = -sgn(cos) (y_j / (|x||y|) - cos x_j / |x|^2): an anchor's
// coefficients once, then a weight per (x_j, y_j)
struct DistWeightF64 {
    double g, inv, cx;
    __device__ __forceinline__ DistWeightF64(float gterm, double cosv, double nx, double ny) {
        const double sg = cosv > 0.0 ? -1.0 : (cosv < 0.0 ? 1.0 : 0.0);
        g = (double)gterm * sg;
        inv = 1.0 / (nx * ny), cx = cosv / (nx * nx);
    }
    __device__ __forceinline__ float operator()(double x, double y) const { return (float)(g * (y * inv - cx * x) / x); }
};

// the forward: one partial per workgroup of 4 anchors, the four terms added pairwise (r0 + r1) + (r2 + r3) — NOT the map term's order
template <DistRows ROWS>
__global__ __launch_bounds__(256) void dist_loss_kernel(const float *__restrict__ feat, const float *__restrict__ dist,
                                                        const int32_t *__restrict__ anchors, const int32_t *__restrict__ idx,
                                                        int N, int C, int nA, int k, double *__restrict__ partial,
                                                        float *__restrict__ xsave /* nullptr, or [B][nA][k] x 2: x_j, y_j kept for the backward */) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = blockIdx.x * (blockDim.x >> 6) + wave;
    const int b = blockIdx.y;
    __shared__ double red[4];
    double term = 0.0;
    if (n < nA) {
        float xs[8], ys[8], nx, ny;
        const int32_t *ix = idx + ((size_t)b * nA + n) * k;
        if (ROWS == DIST_ROWS_128) dist_rows128(feat + (size_t)b * N * 128, dist + (size_t)b * N * N, N, anchors[n], ix, k, lane, xs, ys);
        else dist_rows_generic(feat + (size_t)b * N * C, dist + (size_t)b * N * N, N, C, anchors[n], ix, k, lane, xs, ys);
        if (xsave) {
            float *xr = xsave + ((size_t)b * nA + n) * k * 2;
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (lane + 64 * u < k) xr[lane + 64 * u] = xs[u], xr[k + lane + 64 * u] = ys[u];
        }
        term = 1.0 - (double)fabsf(dist_cos(xs, ys, nx, ny));
    }
    if (lane == 0) red[wave] = term;
    __syncthreads();
    if (threadIdx.x == 0) partial[(size_t)b * gridDim.x + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// Backward of the dist-loss term, first half: the (anchor, point) weights
//     W[b, n, idx_j] = g[b] * d term_n / d x_j / x_j          (0 where x_j = 0; idx rows are distinct points)
// The caller finishes with plain GEMMs:
//     d feat      = diag(colsum W) feat - W^T feat[anchors]
//     d feat[a_n] += rowsum(W)_n feat[a_n] - (W feat)_n
// (k = 500 neighbours x 128 channels per anchor as atomics would be 0.5 G atomics per shape batch).
// W [B][nA][N] must be zero-filled by the caller.  One wave per (b, n), k <= 512.  x_j is formed in float64 from the feature rows
// (dist_x_f64_*, see above); y_j is read from the distance matrix or, DIST_ROWS_SAVED, from what the forward kept (`dist` = its xsave:
// the node's backward has no distance matrix), and then also the row sums rs [B][nA] = sum_v W[b, n, v] of the ROUNDED weights (float64,
// lane order + a wave reduction, rounded once).  gterm read at gterm[b * gstride].
template <DistRows ROWS>
__global__ __launch_bounds__(256) void dist_loss_bwd_weights_kernel(const float *__restrict__ feat, const float *__restrict__ dist /* or xsave */,
                                                                    const int32_t *__restrict__ anchors,
                                                                    const int32_t *__restrict__ idx, const float *__restrict__ gterm,
                                                                    int gstride, int N, int C, int nA, int k, float *__restrict__ W,
                                                                    float *__restrict__ rs) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = blockIdx.x * (blockDim.x >> 6) + wave;
    const int b = blockIdx.y;
    if (n >= nA) return;
    const int32_t *ix = idx + ((size_t)b * nA + n) * k;
    const int a = anchors[n];
    double xd[8], nx, ny;
    float ys[8];
    if (ROWS == DIST_ROWS_GENERIC) dist_x_f64_generic(feat + (size_t)b * N * C, C, a, ix, k, lane, xd);
    else dist_x_f64_128(feat + (size_t)b * N * 128, a, ix, k, lane, xd);
    const float *yr = ROWS == DIST_ROWS_SAVED ? dist + ((size_t)b * nA + n) * k * 2 + k : dist + (size_t)b * N * N + a;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int j = lane + 64 * u;
        ys[u] = 0.f;
        if (j < k) ys[u] = ROWS == DIST_ROWS_SAVED ? yr[j] : yr[(size_t)ix[j] * N];
    }
    const double cosv = dist_cos(xd, ys, nx, ny);
    const DistWeightF64 weight(gterm[(size_t)b * gstride], cosv, nx, ny);
    float *Wr = W + ((size_t)b * nA + n) * N;
    double acc = 0.0;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int j = lane + 64 * u;
        if (j < k && xd[u] > 0.0) {
            const float wv = weight(xd[u], (double)ys[u]);
            Wr[ix[j]] = wv;
            acc += (double)wv;
        }
    }
    if (ROWS == DIST_ROWS_SAVED) {
        acc = wave_sum(acc);
        if (lane == 0) rs[(size_t)b * nA + n] = (float)acc;
    }
}

__global__ void gather_rows_kernel(const float *__restrict__ src, const int32_t *__restrict__ rows, int N, int C, int nR,
                                   float *__restrict__ dst) {
    const int b = blockIdx.y;
    long g = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= (long)nR * C) return;
    int r = (int)(g / C), c = (int)(g % C);
    dst[((size_t)b * nR + r) * C + c] = src[((size_t)b * N + rows[r]) * C + c];
}

// the anchors' rows, their neighbours, one partial per workgroup of 4 anchors, then the kNN's own scratch (anchors against all rows)
struct DistLossWs {
    float *fa;
    int32_t *idx;
    double *partial;
    KnnNegWs knn;
};
static size_t carve_dist_loss(Arena &ar, int B, int N, int C, int nA, int k, DistLossWs &w) {
    w.fa = ar.take<float>((size_t)B * nA * C);
    w.idx = ar.take<int32_t>((size_t)B * nA * k);
    w.partial = ar.take<double>((size_t)B * ((nA + 3) / 4));
    return carve_knn_neg(ar, B, nA, N, w.knn);
}
// dvm_dist_loss_fwd_f32 with the sum written at out[b * out_stride + out_off], the selected neighbours at idx_out (NULL: scratch) and, for
// a backward that does not read the feature rows again, x_j / y_j at xsave [B][nA][k] x 2; fa_out [B][nA][C] = the anchors' rows
int launch_dist_loss_fwd(const float *feat, const float *dist, const int32_t *anchors, int B, int N, int C, int nA, int k, float *out, int out_stride,
                         int out_off, int32_t *idx_out, float *xsave, float *fa_out, void *ws, size_t ws_bytes, hipStream_t s) {
    DistLossWs w;
    if (!carve_ws(ws, ws_bytes, "dvm_dist_loss_fwd_f32", w, carve_dist_loss, B, N, C, nA, k)) return DVM_ENOSPACE;
    const int nblk = (nA + 3) / 4;
    double *const partial = w.partial;
    int32_t *const idx = idx_out ? idx_out : w.idx;
    float *const fa = fa_out ? fa_out : w.fa;
    hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)(((long)nA * C + 255) / 256), B), dim3(256), 0, s, feat, anchors, N, C, nA,
                       fa);
    launch_knn_neg(fa, feat, B, nA, N, C, k, idx, w.knn.na, w.knn.nb, w.knn.S, s);
    if (C == 128)
        hipLaunchKernelGGL(dist_loss_kernel<DIST_ROWS_128>, dim3(nblk, B), dim3(256), 0, s, feat, dist, anchors, idx, N, C, nA, k, partial, xsave);
    else
        hipLaunchKernelGGL(dist_loss_kernel<DIST_ROWS_GENERIC>, dim3(nblk, B), dim3(256), 0, s, feat, dist, anchors, idx, N, C, nA, k, partial, xsave);
    launch_reduce_partials(partial, B, nblk, 1.f, out, out_stride, out_off, s);
    return DVM_OK;
}
// W [B][nA][N] (zeroed here) and its row sums: x_j in float64 from feat [B][N][128], y_j from the forward's xsave; gterm read at
// gterm[b * gstride]
void launch_dist_loss_bwd_weights_saved(const float *feat, const int32_t *anchors, const float *xsave, const int32_t *idx, const float *gterm,
                                        int gstride, int B, int N, int nA, int k, float *W, float *rs, hipStream_t s) {
    (void)hipMemsetAsync(W, 0, (size_t)B * nA * N * sizeof(float), s);
    hipLaunchKernelGGL(dist_loss_bwd_weights_kernel<DIST_ROWS_SAVED>, dim3((nA + 3) / 4, B), dim3(256), 0, s, feat, xsave, anchors, idx, gterm,
                       gstride, N, 128, nA, k, W, rs);
}
}  // namespace dvm

using namespace dvm;

DVM_EXPORT size_t dvm_dist_loss_workspace_bytes(int B, int N, int C, int nA, int k) {
    return null_carve<DistLossWs>(carve_dist_loss, B, N, C, nA, k);
}

DVM_EXPORT int dvm_dist_loss_fwd_f32(const float *feat, const float *dist, const int32_t *anchors, int B, int N, int C, int nA,
                                     int k, float *out, int32_t *idx_out, void *ws, size_t ws_bytes, void *stream) {
    DVM_REQUIRE(feat && dist && anchors && out, "dvm_dist_loss_fwd_f32: null pointer");
    DVM_REQUIRE(B >= 1 && N >= 1 && nA >= 1 && C % 4 == 0, "dvm_dist_loss_fwd_f32: bad sizes");
    DVM_REQUIRE(k >= 1 && k <= 512 && k <= N, "dvm_dist_loss_fwd_f32: k=%d unsupported", k);
    const int rc = launch_dist_loss_fwd(feat, dist, anchors, B, N, C, nA, k, out, 1, 0, idx_out, nullptr, nullptr, ws, ws_bytes, (hipStream_t)stream);
    if (rc != DVM_OK) return rc;
    DVM_CHECK_LAUNCH("dist_loss");
    return DVM_OK;
}

DVM_EXPORT int dvm_dist_loss_bwd_weights_f32(const float *feat, const float *dist, const int32_t *anchors, const int32_t *idx,
                                             const float *g_out, int B, int N, int C, int nA, int k, float *W, void *stream) {
    DVM_REQUIRE(feat && dist && anchors && idx && g_out && W, "dvm_dist_loss_bwd_weights_f32: null pointer");
    DVM_REQUIRE(B >= 1 && N >= 1 && nA >= 1 && C % 4 == 0, "dvm_dist_loss_bwd_weights_f32: bad sizes");
    DVM_REQUIRE(k >= 1 && k <= 512 && k <= N, "dvm_dist_loss_bwd_weights_f32: k=%d unsupported", k);
    hipStream_t s = (hipStream_t)stream;
    (void)hipMemsetAsync(W, 0, (size_t)B * nA * N * sizeof(float), s);
    const dim3 grid((nA + 3) / 4, B);
    if (C == 128)
        hipLaunchKernelGGL(dist_loss_bwd_weights_kernel<DIST_ROWS_128>, grid, dim3(256), 0, s, feat, dist, anchors, idx, g_out, 1, N, C, nA, k, W,
                           (float *)nullptr);
    else
        hipLaunchKernelGGL(dist_loss_bwd_weights_kernel<DIST_ROWS_GENERIC>, grid, dim3(256), 0, s, feat, dist, anchors, idx, g_out, 1, N, C, nA, k, W,
                           (float *)nullptr);
    DVM_CHECK_LAUNCH("dist_loss_bwd_weights");
    return DVM_OK;
}
