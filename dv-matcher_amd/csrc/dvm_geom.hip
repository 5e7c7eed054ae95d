// dvm_geom.hip — small geometric kernels of the correspondence path:
//   arg-min map in the exact-difference form (knnsearch_t), xyz kNN (knn_grad), sparse Pi~ @ V,
//   Chamfer nearest neighbours, the map-loss numerator, and fixed-order reductions.
// All are HBM-light brute-force sweeps with the "other" cloud staged through LDS; every
// floating-point expression is written in the rounding order of the reference's CPU path
// (see oracle/dvm_oracle.c) so that the integer outputs are bit-exact.
#include "dvm_common.h"
#include <stdlib.h>

namespace dvm {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------- argmin (exact form)
// knnsearch_t: reference models/loss.py:91-95, test.py:19-23.  agg = agg + (a-b)*(a-b) summed
// sequentially over the feature index with separately rounded mul and add (d % 4 == 0).
constexpr int AM_KT = 32, AM_DC = 32;

__global__ __launch_bounds__(128) void argmin_exact_kernel(const float *__restrict__ f1, const float *__restrict__ f2,
                                                           int N, int M, int d, int32_t *__restrict__ T,
                                                           float *__restrict__ dmin) {
    extern __shared__ __attribute__((aligned(16))) float smem[];  // [AM_KT][d]
    const int b = blockIdx.y;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int ic = i < N ? i : N - 1;
    const float *q = f1 + ((size_t)b * N + ic) * d;
    const float *kbase = f2 + (size_t)b * M * d;
    float best = INFINITY;
    int bj = 0;
    for (int j0 = 0; j0 < M; j0 += AM_KT) {
        __syncthreads();
        for (int e = threadIdx.x; e < AM_KT * d / 4; e += blockDim.x) {
            int r = e / (d / 4), c = e % (d / 4);
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (j0 + r < M) v = *(const f32x4 *)(kbase + (size_t)(j0 + r) * d + 4 * c);
            *(f32x4 *)(smem + r * d + 4 * c) = v;
        }
        __syncthreads();
        float acc[AM_KT];
#pragma unroll
        for (int j = 0; j < AM_KT; ++j) acc[j] = 0.f;
        for (int c0 = 0; c0 < d; c0 += AM_DC) {
            float qr[AM_DC];
            int cw = d - c0 < AM_DC ? d - c0 : AM_DC;
#pragma unroll
            for (int c = 0; c < AM_DC; c += 4) {
                f32x4 v = {0.f, 0.f, 0.f, 0.f};
                if (c < cw) v = *(const f32x4 *)(q + c0 + c);
                qr[c] = v.x, qr[c + 1] = v.y, qr[c + 2] = v.z, qr[c + 3] = v.w;
            }
#pragma unroll
            for (int j = 0; j < AM_KT; ++j) {
#pragma unroll
                for (int c = 0; c < AM_DC; c += 4) {
                    if (c < cw) {
                        f32x4 kv = *(const f32x4 *)(smem + j * d + c0 + c);
                        float e0 = qr[c] - kv.x, e1 = qr[c + 1] - kv.y, e2 = qr[c + 2] - kv.z, e3 = qr[c + 3] - kv.w;
                        float p0 = e0 * e0, p1 = e1 * e1, p2 = e2 * e2, p3 = e3 * e3;
                        acc[j] = acc[j] + p0;
                        acc[j] = acc[j] + p1;
                        acc[j] = acc[j] + p2;
                        acc[j] = acc[j] + p3;
                    }
                }
            }
        }
#pragma unroll
        for (int j = 0; j < AM_KT; ++j) {
            float dv = sqrt_rn(acc[j]);
            if (j0 + j < M && dv < best) {
                best = dv;
                bj = j0 + j;
            }
        }
    }
    if (i < N) {
        T[(size_t)b * N + i] = bj;
        if (dmin) dmin[(size_t)b * N + i] = best;
    }
}

// ---------------------------------------------------------------- xyz kNN (knn_grad)
// k smallest of torch.cdist (matmul form) per row, ascending (distance, index).  C <= 16.
constexpr int KN_PT = 256;  // points per LDS tile

template <int K>
__global__ __launch_bounds__(128) void knn_cdist_kernel(const float *__restrict__ x, const float *__restrict__ y, int N,
                                                        int M, int C, int k, int32_t *__restrict__ idx) {
    __shared__ float pts[KN_PT * 16];
    __shared__ float pn[KN_PT];
    const int b = blockIdx.y;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int ic = i < N ? i : N - 1;
    float q[16];
    const float *qp = x + ((size_t)b * N + ic) * C;
    for (int c = 0; c < 16; ++c) q[c] = c < C ? qp[c] : 0.f;
    const float nq = aten_sumsq_row(qp, C);
    for (int c = 0; c < 16; ++c) q[c] = -2.f * q[c];
    KBest<K, float> kb;
    kb.init(INFINITY);
    const float *yb = y + (size_t)b * M * C;
    for (int j0 = 0; j0 < M; j0 += KN_PT) {
        __syncthreads();
        for (int e = threadIdx.x; e < KN_PT; e += blockDim.x) {
            if (j0 + e < M) {
                for (int c = 0; c < C; ++c) pts[e * C + c] = yb[(size_t)(j0 + e) * C + c];
                pn[e] = aten_sumsq_row(yb + (size_t)(j0 + e) * C, C);
            } else {
                for (int c = 0; c < C; ++c) pts[e * C + c] = 0.f;
                pn[e] = INFINITY;
            }
        }
        __syncthreads();
        int lim = M - j0 < KN_PT ? M - j0 : KN_PT;
        for (int j = 0; j < lim; ++j) {
            float acc = 0.f;
            for (int c = 0; c < C; ++c) acc = fmaf(q[c], pts[j * C + c], acc);
            acc = acc + nq;
            acc = acc + pn[j];
            acc = acc > 0.f ? acc : 0.f;
            kb.insert(sqrt_rn(acc), j0 + j);
        }
    }
    if (i < N)
        for (int t = 0; t < K; ++t)
            if (t < k) idx[((size_t)b * N + i) * k + t] = t < M ? kb.idx[t] : 0;
}

__shared__ float4 tile3[KN_PT];   // (per kernel that names it)
// One tile of the brute-force scans below (between two barriers): the next KN_PT points of a cloud, `left` of them real, from
// tp [left][3] into LDS as (x, y, z, w).  w is the caller's — |p|^2 in ATen order (the matmul form's operand) where NORM, else
// 0 — and the rows past the cloud's end are (0, 0, 0, pad_w).
template <bool NORM>
__device__ __forceinline__ void stage_tile3(const float *tp, int left, float pad_w) {
    __syncthreads();
    for (int e = threadIdx.x; e < KN_PT; e += blockDim.x) {
        float4 p = {0.f, 0.f, 0.f, pad_w};
        if (e < left) {
            const float *pp = tp + 3 * e;
            p.x = pp[0], p.y = pp[1], p.z = pp[2];
            p.w = NORM ? sumsq3(p.x, p.y, p.z) : 0.f;
        }
        tile3[e] = p;
    }
    __syncthreads();
}

// specialisation for C == 3 (the only shape on the hot path): coordinates in registers
template <int K>
__global__ __launch_bounds__(128) void knn_cdist3_kernel(const float *__restrict__ x, const float *__restrict__ y, int N,
                                                         int M, int k, int32_t *__restrict__ idx) {
    const int b = blockIdx.y;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int ic = i < N ? i : N - 1;
    const float *qp = x + ((size_t)b * N + ic) * 3;
    const float qx = qp[0], qy = qp[1], qz = qp[2];
    const float nq = sumsq3(qx, qy, qz);
    KBest<K, float> kb;
    kb.init(INFINITY);
    const float *yb = y + (size_t)b * M * 3;
    for (int j0 = 0; j0 < M; j0 += KN_PT) {
        stage_tile3<true>(yb + (size_t)j0 * 3, M - j0, INFINITY);
        int lim = M - j0 < KN_PT ? M - j0 : KN_PT;
#pragma unroll 4
        for (int j = 0; j < lim; ++j) {
            float4 p = tile3[j];
            float d2 = d2_mm3(qx, qy, qz, nq, p.x, p.y, p.z, p.w);
            kb.insert(sqrt_rn(d2), j0 + j);
        }
    }
    if (i < N)
        for (int t = 0; t < K; ++t)
            if (t < k) idx[((size_t)b * N + i) * k + t] = t < M ? kb.idx[t] : 0;
}

// ---------------------------------------------------------------- sparse Pi~ @ V
// One thread per (row, 4-channel group); the row's entries are visited in ascending column order
// (the order in which a dense k-ordered GEMM meets the non-zeros).
template <int TOPK>
__device__ __forceinline__ void sort_by_col(float (&v)[TOPK], int (&c)[TOPK]) {
#pragma unroll
    for (int a = 1; a < TOPK; ++a) {
#pragma unroll
        for (int p = a; p > 0; --p) {
            bool sw = c[p] < c[p - 1];
            int c0 = c[p - 1], c1 = c[p];
            float v0 = v[p - 1], v1 = v[p];
            c[p - 1] = sw ? c1 : c0;
            c[p] = sw ? c0 : c1;
            v[p - 1] = sw ? v1 : v0;
            v[p] = sw ? v0 : v1;
        }
    }
}

template <int TOPK>
__global__ __launch_bounds__(256) void apply_kernel(const float *__restrict__ pi_val, const int32_t *__restrict__ pi_idx,
                                                    const float *__restrict__ V, int N, int M, int topk, int C,
                                                    float *__restrict__ out) {
    const int groups = (C + 3) / 4;
    const int b = blockIdx.y;
    const long g = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= (long)N * groups) return;
    const int i = (int)(g / groups), cg = (int)(g % groups);
    const size_t row = (size_t)b * N + i;
    float v[TOPK];
    int c[TOPK];
#pragma unroll
    for (int t = 0; t < TOPK; ++t) {
        const bool live = t < topk;
        const size_t o = row * topk + (live ? t : 0);   // (clamped, then selected: predicated loads go out one round trip at a time)
        const float vt = pi_val[o];
        const int ct = pi_idx[o];
        v[t] = live ? vt : 0.f;
        c[t] = live ? ct : 0x7fffffff;  // padding sorts last, contributes nothing
    }
    sort_by_col<TOPK>(v, c);
    const float *Vb = V + (size_t)b * M * C;
    const int c0 = cg * 4;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    float vr[TOPK][4];   // all gathered values first (clamped addresses), then the chains in order
#pragma unroll
    for (int t = 0; t < TOPK; ++t) {
        const float *p = Vb + (size_t)(t < topk ? c[t] : 0) * C;
#pragma unroll
        for (int e = 0; e < 4; ++e) vr[t][e] = p[c0 + e < C ? c0 + e : C - 1];
    }
#pragma unroll
    for (int t = 0; t < TOPK; ++t) {
        if (t < topk) {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (c0 + e < C) acc[e] = fmaf(v[t], vr[t][e], acc[e]);
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (c0 + e < C) out[row * C + c0 + e] = acc[e];
}

// Pi~ @ verts (C = 3, top-10) of BOTH directions of a pair batch in one launch, with the arg-max maps: one workgroup per (cloud,
// direction) stages the target coordinates (12 M bytes) in LDS, a thread takes rows i, i + 256, ...: T[i] = the row's first
// column (the arg-max, before the sort), then apply_kernel's column-ordered fma chains — the same bits.  (Two apply_kernel and
// two take_col0 launches before; their 10 coordinate gathers per row went through L2.)
struct Apply3Pair {
    const float *val[2], *V[2];
    const int32_t *idx[2];
    float *out[2];
    int32_t *T[2];
    int N[2], M[2];
};
__global__ __launch_bounds__(256) void apply3_pair_kernel(const Apply3Pair a) {
    extern __shared__ __attribute__((aligned(16))) float ap_lds[];   // [M][3]
    const int b = blockIdx.x, d = blockIdx.y;
    const int N = a.N[d], M = a.M[d];
    const float *Vb = a.V[d] + (size_t)b * M * 3;
    for (int e = threadIdx.x; e < M * 3; e += 256) ap_lds[e] = Vb[e];
    __syncthreads();
    for (int i = threadIdx.x; i < N; i += 256) {
        const size_t row = (size_t)b * N + i;
        float v[10];
        int c[10];
#pragma unroll
        for (int t = 0; t < 10; ++t) v[t] = a.val[d][row * 10 + t], c[t] = a.idx[d][row * 10 + t];
        a.T[d][row] = c[0];
        sort_by_col<10>(v, c);
        float acc[3] = {0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < 10; ++t) {
            const float *p = ap_lds + 3 * c[t];
            acc[0] = fmaf(v[t], p[0], acc[0]);
            acc[1] = fmaf(v[t], p[1], acc[1]);
            acc[2] = fmaf(v[t], p[2], acc[2]);
        }
        a.out[d][row * 3] = acc[0], a.out[d][row * 3 + 1] = acc[1], a.out[d][row * 3 + 2] = acc[2];
    }
}

// Backward of apply_kernel: out[i] = sum_t val[i,t] V[idx[i,t]]  =>  d_val[i,t] = g[i] . V[idx[i,t]],
// d_V[idx[i,t]] += val[i,t] g[i] (fp32 atomics).  A row's ceil(C/4) channel groups sit in GP2 (power of two
// >= groups, <= 64) consecutive lanes so the dot products reduce with shuffles.
__global__ __launch_bounds__(256) void apply_bwd_kernel(const float *__restrict__ pi_val, const int32_t *__restrict__ pi_idx,
                                                        const float *__restrict__ V, const float *__restrict__ gout, int N, int M,
                                                        int topk, int C, int gp2, float *__restrict__ dval,
                                                        float *__restrict__ dV /* nullptr: d_V comes from the gather pass */) {
    const int groups = (C + 3) / 4;
    const int b = blockIdx.y;
    const long g = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long i0 = g / gp2;
    const int cg = (int)(g % gp2);
    const bool live = i0 < N && cg < groups;
    const int i = i0 < N ? (int)i0 : N - 1;
    const size_t row = (size_t)b * N + i;
    const int c0 = cg * 4;
    float gv[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) gv[e] = (live && c0 + e < C) ? gout[row * C + c0 + e] : 0.f;
    for (int t = 0; t < topk; ++t) {
        const int j = pi_idx[row * topk + t];
        const bool ok = live && j >= 0 && j < M;
        const float w = pi_val[row * topk + t];
        const size_t vr = ((size_t)b * M + (ok ? j : 0)) * C + c0;
        float part = 0.f;
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (ok && c0 + e < C) {
                part = fmaf(gv[e], V[vr + e], part);
                if (dV) unsafeAtomicAdd(dV + vr + e, w * gv[e]);
            }
        for (int o = 1; o < gp2; o <<= 1) part += __shfl_xor(part, o, 64);
        if (cg == 0 && i0 < N) dval[row * topk + t] = part;
    }
}

// d_V without float atomics: the (row, slot) -> target lists are reversed by a counting sort (launch_rev_csr, dvm_revlist.hip:
// one int atomic per entry), then one wave per target row sums its in-edges, lanes over channels.
// sum of val[e] * gout[row(e)] over the in-edges ed[beg..end) of one target, lanes over channels
__device__ __forceinline__ void gather_edges(const int32_t *__restrict__ ed, int beg, int end, const float *__restrict__ vb,
                                             const float *__restrict__ gb, int topk, int C, int lane, float (&acc)[4]) {
    int e = beg;
    for (; e + 1 < end; e += 2) {  // two in-edges in flight
        const int e0 = ed[e], e1 = ed[e + 1];
        const float w0 = vb[e0], w1 = vb[e1];
        const float *g0 = gb + (size_t)(e0 / topk) * C, *g1 = gb + (size_t)(e1 / topk) * C;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int c = lane + 64 * q;
            if (c < C) {
                const float a = g0[c], bb = g1[c];
                acc[q] = fmaf(w0, a, acc[q]);
                acc[q] = fmaf(w1, bb, acc[q]);
            }
        }
    }
    if (e < end) {
        const int e0 = ed[e];
        const float w0 = vb[e0];
        const float *g0 = gb + (size_t)(e0 / topk) * C;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int c = lane + 64 * q;
            if (c < C) acc[q] = fmaf(w0, g0[c], acc[q]);
        }
    }
}

// One wave per target row; a target with more than AG_HEAVY in-edges (the hubs of a soft correspondence collect
// thousands) is shared by the four waves of its workgroup instead, each taking a quarter of the list.
constexpr int AG_HEAVY = 96;

__global__ __launch_bounds__(256) void apply_bwd_gather_kernel(const float *__restrict__ pi_val, const float *__restrict__ gout,
                                                               const int32_t *__restrict__ offs, const int32_t *__restrict__ edges,
                                                               int N, int M, int topk, int C, float *__restrict__ dV) {
    __shared__ float red[4][256];
    __shared__ int sbeg[4], send[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long j = (long)blockIdx.x * 4 + wave;
    const int b = blockIdx.y;
    const long E = (long)N * topk;
    const int32_t *ed = edges + (size_t)b * E;
    const float *vb = pi_val + (size_t)b * E, *gb = gout + (size_t)b * N * C;
    int beg = 0, end = 0;
    if (j < M) beg = offs[(size_t)b * (M + 1) + j], end = offs[(size_t)b * (M + 1) + j + 1];
    if (lane == 0) sbeg[wave] = beg, send[wave] = end;
    const bool heavy = end - beg > AG_HEAVY;
    if (j < M && !heavy) {
        float acc[4] = {0.f, 0.f, 0.f, 0.f};  // C <= 256: channels lane, lane+64, lane+128, lane+192
        gather_edges(ed, beg, end, vb, gb, topk, C, lane, acc);
        float *o = dV + ((size_t)b * M + j) * C;
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (lane + 64 * q < C) o[lane + 64 * q] = acc[q];
    }
    __syncthreads();
    for (int t = 0; t < 4; ++t) {  // workgroup-uniform: the heavy targets of this workgroup, one after the other
        const int tb = sbeg[t], te = send[t];
        if (te - tb <= AG_HEAVY) continue;
        const int part = (te - tb + 3) / 4;
        const int pb = tb + wave * part, pe = pb + part < te ? pb + part : te;
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        if (pb < pe) gather_edges(ed, pb, pe, vb, gb, topk, C, lane, acc);
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 4; ++q) red[wave][lane + 64 * q] = acc[q];
        __syncthreads();
        const int c = threadIdx.x;
        if (c < C) dV[((size_t)b * M + (long)blockIdx.x * 4 + t) * C + c] = (red[0][c] + red[1][c]) + (red[2][c] + red[3][c]);
    }
}

// ---------------------------------------------------------------- Chamfer NN
// d1[i] = min_j |a_i - b_j|^2 ((dx^2+dy^2)+dz^2, no contraction), first minimum wins.
__global__ __launch_bounds__(128) void chamfer_kernel(const float *__restrict__ a, const float *__restrict__ bpts, int N,
                                                      int M, float *__restrict__ dout, int32_t *__restrict__ iout) {
    const int b = blockIdx.y;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int ic = i < N ? i : N - 1;
    const float *qp = a + ((size_t)b * N + ic) * 3;
    const float qx = qp[0], qy = qp[1], qz = qp[2];
    float best = INFINITY;
    int bj = 0;
    const float *yb = bpts + (size_t)b * M * 3;
    for (int j0 = 0; j0 < M; j0 += KN_PT) {
        stage_tile3<false>(yb + (size_t)j0 * 3, M - j0, 0.f);
        int lim = M - j0 < KN_PT ? M - j0 : KN_PT;
#pragma unroll 4
        for (int j = 0; j < lim; ++j) {
            float4 p = tile3[j];
            float dv = d2_diff3(qx, qy, qz, p.x, p.y, p.z);
            if (dv < best) {
                best = dv;
                bj = j0 + j;
            }
        }
    }
    if (i < N) {
        dout[(size_t)b * N + i] = best;
        if (iout) iout[(size_t)b * N + i] = bj;
    }
}

// The same search with 4 lanes per query, each scanning a quarter of the target cloud (held whole in LDS, M <= 8192), then
// the better of the four (lower distance, then lower index = lower quarter): the per-query chain of M dependent
// compare-and-keep steps is what the kernel above waits on at training batch sizes (84 us for 8 x 2048 x 2048).
constexpr int CH_PARTS = 4;
__global__ __launch_bounds__(256) void chamfer_split_kernel(const float *__restrict__ a, const float *__restrict__ bpts, int N, int M,
                                                            float *__restrict__ dout, int32_t *__restrict__ iout) {
    extern __shared__ float4 ch_pts[];   // [M]
    const int b = blockIdx.y;
    const float *yb = bpts + (size_t)b * M * 3;
    for (int e = threadIdx.x; e < M; e += 256) ch_pts[e] = make_float4(yb[3 * e], yb[3 * e + 1], yb[3 * e + 2], 0.f);
    __syncthreads();
    const int i = blockIdx.x * (256 / CH_PARTS) + threadIdx.x / CH_PARTS, part = threadIdx.x % CH_PARTS;
    const int ic = i < N ? i : N - 1;
    const float *qp = a + ((size_t)b * N + ic) * 3;
    const float qx = qp[0], qy = qp[1], qz = qp[2];
    const int per = (M + CH_PARTS - 1) / CH_PARTS, j0 = part * per, j1 = j0 + per < M ? j0 + per : M;
    float best = INFINITY;
    int bj = 0x7fffffff;   // "nothing found": a part that is empty, or whose distances are all NaN / +inf
#pragma unroll 4
    for (int j = j0; j < j1; ++j) {
        const float4 p = ch_pts[j];
        const float dv = d2_diff3(qx, qy, qz, p.x, p.y, p.z);
        if (dv < best) best = dv, bj = j;
    }
#pragma unroll
    for (int o = 1; o < CH_PARTS; o <<= 1) {   // quarters are index-ordered: on equal distances the lower index wins
        const float od = __shfl_xor(best, o, 64);
        const int oj = __shfl_xor(bj, o, 64);
        if (od < best || (od == best && oj < bj)) best = od, bj = oj;
    }
    // non-finite coordinates (a diverged step) leave every comparison false: the index must still be a valid row, because
    // the backward pass gathers and scatters through it unchecked (index 0, like chamfer_kernel above)
    bj = bj < M ? bj : 0;
    if (i < N && part == 0) {
        dout[(size_t)b * N + i] = best;
        if (iout) iout[(size_t)b * N + i] = bj;
    }
}

// ---------------------------------------------------------------- map-loss numerator
// The pieces every form of the map term shares, so that the forms agree bit for bit.
// One slot's residual from the TOPK weights and the TOPK coordinates already gathered: e = p12 - sum_t w[t] p[t], the products
// summed by fmaf in t order over t < topk (the row's own order, not the dense matmul's column order: a loss term, compared at
// 1e-4); returns (e0^2 + e1^2) + e2^2.
template <int TOPK>
__device__ __forceinline__ float map_term_resid(const float (&w)[TOPK], const float (&px)[TOPK], const float (&py)[TOPK],
                                                const float (&pz)[TOPK], int topk, float p12x, float p12y, float p12z, float &e0,
                                                float &e1, float &e2c) {
    float acc[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < TOPK; ++t) {
        if (t < topk) {
            acc[0] = fmaf(w[t], px[t], acc[0]);
            acc[1] = fmaf(w[t], py[t], acc[1]);
            acc[2] = fmaf(w[t], pz[t], acc[2]);
        }
    }
    e0 = p12x - acc[0], e1 = p12y - acc[1], e2c = p12z - acc[2];
    return (e0 * e0 + e1 * e1) + e2c * e2c;
}
// Epilogue of the 256-thread (point, slot) forms: a wave's sum in double, the block's four wave sums added in order
// (((0 + r0) + r1) + r2) + r3 — NOT the pairwise order of the dist term — one partial per block.
__device__ __forceinline__ void map_term_block_partial(float e2, int b, double *__restrict__ partial) {
    __shared__ double red[256 / 64];
    const double w = wave_sum((double)e2);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = w;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int q = 0; q < 256 / 64; ++q) s += red[q];
        partial[(size_t)b * gridDim.x + blockIdx.x] = s;
    }
}

// thread per (i, s): e_c = verts12[idx11[i,s],c] - sum_t P[i,t] verts2[idx22[pidx[i,t],s],c]
template <int TOPK>
__global__ __launch_bounds__(256) void map_term_kernel(const float *__restrict__ verts12, const float *__restrict__ verts2,
                                                       const int32_t *__restrict__ idx11, const int32_t *__restrict__ idx22,
                                                       const float *__restrict__ pi_val, const int32_t *__restrict__ pi_idx,
                                                       int N, int M, int k, int topk, double *__restrict__ partial,
                                                       float *__restrict__ resid /* nullptr, or [B][N][k][3]: e_c kept for the backward */) {
    const int b = blockIdx.y;
    const long g = (long)blockIdx.x * blockDim.x + threadIdx.x;
    float e2 = 0.f;
    if (g < (long)N * k) {
        const int i = (int)(g / k), s = (int)(g % k);
        const size_t row = (size_t)b * N + i;
        const float *v2 = verts2 + (size_t)b * M * 3;
        const int32_t *i22 = idx22 + (size_t)b * M * k;
        int nb[TOPK];
        float v[TOPK];
        // three levels of dependent loads (weights / columns -> second-level indices -> coordinates), each level requested as a
        // whole: the addresses are clamped and the values selected (a predicated load goes out alone, after a full wait)
        int col[TOPK];
#pragma unroll
        for (int t = 0; t < TOPK; ++t) {
            const size_t o = row * topk + (t < topk ? t : 0);
            v[t] = pi_val[o];
            col[t] = pi_idx[o];
        }
#pragma unroll
        for (int t = 0; t < TOPK; ++t) nb[t] = i22[(size_t)col[t] * k + s];
        float px[TOPK], py[TOPK], pz[TOPK];
#pragma unroll
        for (int t = 0; t < TOPK; ++t) {
            const float *p = v2 + 3 * (size_t)nb[t];
            px[t] = p[0], py[t] = p[1], pz[t] = p[2];
        }
        const float *p12 = verts12 + ((size_t)b * N + idx11[row * k + s]) * 3;
        float e0, e1, e2c;
        e2 = map_term_resid<TOPK>(v, px, py, pz, topk, p12[0], p12[1], p12[2], e0, e1, e2c);
        if (resid) {
            float *r = resid + ((size_t)b * N * k + g) * 3;
            r[0] = e0, r[1] = e1, r[2] = e2c;
        }
    }
    map_term_block_partial(e2, b, partial);
}

// Round 4: the map term with the TARGET side resident in LDS — one workgroup of 1024 threads per cloud stages verts2 (12 M bytes)
// and idx22 (4 M k bytes: 24 + 80 KB at 2048 points, k = 10) once, and every (index -> coordinate) lookup of the 10 correspondences
// of a (point, slot) thread is two LDS reads instead of L2 round trips; no [M][k][3] neighbour table is built (gather_nbr_xyz_kernel
// and its 250 MB per launch disappear).  The workgroup walks the 256-thread blocks of map_term_kernel four at a time and writes
// the SAME partial sums in the same slots (a wave's sum, then the block's four waves in order): bit-identical to both older forms.
// (round 6: blockIdx.y = direction, so that both directions of the pair path are ONE launch — one workgroup per cloud is 64 - 128
// workgroups on 256 compute units at the small resident batches of a strong-scaling rank)
struct MapTermSide {
    const float *verts12, *verts2;
    const int32_t *idx11, *idx22;
    const float *pi_val;
    const int32_t *pi_idx;
    int N, M, nblk;
    double *partial;
};
struct MapTermArgs {
    MapTermSide d[2];
    int k;
};
// Round 6: ONE THREAD PER POINT (all k slots), verts12 staged as well: 0.66 -> 0.58 ms per launch of 1 024 clouds x 2 directions (what is
// left is the LDS pipe: 5.2 M LDS instructions per launch, 60 % of their cycles bank conflicts of the random 16-byte coordinate reads, 41 %
// of the wave cycles waiting on them; neither 8-byte loads of the three 40-byte global rows nor the batched staging moved it further).  As one thread per (point, slot) the 10 threads of a point each
// loaded the point's whole Pi row (20 global loads per thread and trip, then a dependent gather of verts12) and the workgroup — 16 waves
// on the compute unit, 104 KB of LDS — waited out those round trips 20 times per cloud: 0.66 ms per launch of 1 024 clouds x 2 directions.
// Here a thread loads its Pi row and its xyz-neighbour row once (120 B), and every other lookup is an LDS read — vector reads: the
// coordinates are staged as float4, a correspondence's 10 neighbour indices are five 8-byte reads (430 scalar LDS reads per point as
// first written: bank-conflict-bound at 0.63 ms; 160 vector reads: see below).  Partial sums: per point
// the k squared residuals in slot order (fp32 -> double), a wave's 64 points by wave_sum, one partial per wave, the rest of the `nblk`
// slots zero (reduce_partials_kernel adds them all): same value to rounding of the double sums (the oracle's bar is rtol 1e-4).
template <int TOPK>
__global__ __launch_bounds__(1024) void map_term_lds_kernel(const MapTermArgs args) {
    extern __shared__ __attribute__((aligned(16))) char mt_lds[];
    const MapTermSide &A = args.d[blockIdx.y];
    const float *__restrict__ verts12 = A.verts12, *__restrict__ verts2 = A.verts2, *__restrict__ pi_val = A.pi_val;
    const int32_t *__restrict__ idx11 = A.idx11, *__restrict__ idx22 = A.idx22, *__restrict__ pi_idx = A.pi_idx;
    double *__restrict__ partial = A.partial;
    const int N = A.N, M = A.M, nblk = A.nblk;
    constexpr int K = 10;                                          // xyz neighbours per point (checked by the launcher)
    float4 *v2 = (float4 *)mt_lds;                                 // [M] (x, y, z, -)
    float4 *v12 = v2 + M;                                          // [N]
    int32_t *i22 = (int32_t *)(v12 + N);                           // [M][K]: rows of 40 B, 8-byte aligned
    const int b = blockIdx.x;
    {
        const float *gv = verts2 + (size_t)b * M * 3, *gw = verts12 + (size_t)b * N * 3;
        const int32_t *gi = idx22 + (size_t)b * M * K;
        for (int e = threadIdx.x; e < M; e += 1024) v2[e] = float4{gv[3 * e], gv[3 * e + 1], gv[3 * e + 2], 0.f};
        for (int e = threadIdx.x; e < N; e += 1024) v12[e] = float4{gw[3 * e], gw[3 * e + 1], gw[3 * e + 2], 0.f};
        // (the table is 80 KB at 2048 points: 16-byte loads, all of a thread's requested before its first LDS store — as a loop of
        // 4-byte load / store pairs the staging was 20 dependent round trips)
        const int n4 = (M * K) / 4;
        if (((size_t)gi & 15) == 0) {
            typedef int i32x4_t __attribute__((ext_vector_type(4)));
            for (int e0 = 0; e0 < n4; e0 += 8 * 1024) {
                i32x4_t t[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int e = e0 + u * 1024 + (int)threadIdx.x;
                    t[u] = e < n4 ? *(const i32x4_t *)(gi + 4 * e) : i32x4_t{0, 0, 0, 0};
                }
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int e = e0 + u * 1024 + (int)threadIdx.x;
                    if (e < n4) *(i32x4_t *)(i22 + 4 * e) = t[u];
                }
            }
            for (int e = 4 * n4 + threadIdx.x; e < M * K; e += 1024) i22[e] = gi[e];
        } else {
            for (int e = threadIdx.x; e < M * K; e += 1024) i22[e] = gi[e];
        }
    }
    __syncthreads();
    const int wave = threadIdx.x >> 6, npass = (N + 1023) / 1024;
    for (int p = 0; p < npass; ++p) {
        const int i = p * 1024 + (int)threadIdx.x;
        double e2 = 0.0;
        if (i < N) {
            const size_t row = (size_t)b * N + i;
            int col[TOPK], n11[K];
            float w[TOPK];
            // (the three 40-byte rows as 8-byte loads: rows are 8-byte aligned, and a wave's load instruction touches the same ~20 cache
            // lines whatever its width — five instructions per row instead of ten)
            static_assert(TOPK % 2 == 0 && K % 2 == 0, "8-byte row loads");
            {
                const int2 *ri = (const int2 *)(pi_idx + row * TOPK), *rn = (const int2 *)(idx11 + row * K);
                const float2 *rw = (const float2 *)(pi_val + row * TOPK);
#pragma unroll
                for (int u = 0; u < TOPK / 2; ++u) {
                    const int2 ci = ri[u];
                    const float2 cw = rw[u];
                    col[2 * u] = ci.x, col[2 * u + 1] = ci.y, w[2 * u] = cw.x, w[2 * u + 1] = cw.y;
                }
#pragma unroll
                for (int u = 0; u < K / 2; ++u) {
                    const int2 cn = rn[u];
                    n11[2 * u] = cn.x, n11[2 * u + 1] = cn.y;
                }
            }
            // Pi-weighted sums of the targets' neighbour coordinates: slot s of correspondence t is neighbour s of column col[t]; a
            // correspondence's K neighbour indices are one 40-byte LDS row (five 8-byte reads), a coordinate one 16-byte read; the
            // sum over t runs in t order for every slot (the order of the (point, slot) form).  map_term_resid's arithmetic, written out:
            // with all K slots of a point in one thread the chains advance together, one correspondence's index row at a time, and
            // gathering a slot's TOPK coordinates first (the helper's shape) costs 32 registers or spills (profiles/notes_loss_kernels.md)
            float acc[K][3];
#pragma unroll
            for (int s = 0; s < K; ++s) acc[s][0] = acc[s][1] = acc[s][2] = 0.f;
#pragma unroll
            for (int t = 0; t < TOPK; ++t) {
                int nb[K];
                const int2 *r = (const int2 *)(i22 + col[t] * K);
#pragma unroll
                for (int u = 0; u < K / 2; ++u) {
                    const int2 v = r[u];
                    nb[2 * u] = v.x, nb[2 * u + 1] = v.y;
                }
#pragma unroll
                for (int s = 0; s < K; ++s) {
                    const float4 q = v2[nb[s]];
                    acc[s][0] = fmaf(w[t], q.x, acc[s][0]);
                    acc[s][1] = fmaf(w[t], q.y, acc[s][1]);
                    acc[s][2] = fmaf(w[t], q.z, acc[s][2]);
                }
            }
#pragma unroll
            for (int s = 0; s < K; ++s) {
                const float4 p12 = v12[n11[s]];
                const float e0 = p12.x - acc[s][0], e1 = p12.y - acc[s][1], e2c = p12.z - acc[s][2];
                e2 += (double)((e0 * e0 + e1 * e1) + e2c * e2c);
            }
        }
        const double ws = wave_sum(e2);
        const int slot = p * 16 + wave;
        if ((threadIdx.x & 63) == 0 && slot < nblk) partial[(size_t)b * nblk + slot] = ws;
    }
    for (int q = npass * 16 + (int)threadIdx.x; q < nblk; q += 1024) partial[(size_t)b * nblk + q] = 0.0;
}

// Two-level gathers flattened (fused pair path): nbr[b][j][s][3] = verts[b][idx[b][j][s]] once per cloud, then the map
// term reads ONE contiguous 12*k-byte row per correspondence instead of k (index, coordinate) pairs.
__global__ void gather_nbr_xyz_kernel(const float *__restrict__ verts, const int32_t *__restrict__ idx, int M, int k,
                                      float *__restrict__ nbr) {
    const int b = blockIdx.y;
    const long g = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= (long)M * k) return;
    const float *p = verts + ((size_t)b * M + idx[(size_t)b * M * k + g]) * 3;
    float *o = nbr + ((size_t)b * M * k + g) * 3;
    o[0] = p[0], o[1] = p[1], o[2] = p[2];
}

template <int TOPK>
__global__ __launch_bounds__(256) void map_term_nbr_kernel(const float *__restrict__ verts12, const float *__restrict__ nbr2,
                                                           const int32_t *__restrict__ idx11, const float *__restrict__ pi_val,
                                                           const int32_t *__restrict__ pi_idx, int N, int M, int k, int topk,
                                                           double *__restrict__ partial) {
    const int b = blockIdx.y;
    const long g = (long)blockIdx.x * blockDim.x + threadIdx.x;
    float e2 = 0.f;
    if (g < (long)N * k) {
        const int i = (int)(g / k), s = (int)(g % k);
        const size_t row = (size_t)b * N + i;
        const float *nb2 = nbr2 + (size_t)b * M * k * 3 + 3 * s;
        // columns and weights, then all gathers, then the chain: addresses clamped, values selected by the chain's t < topk
        int col[TOPK];
        float w[TOPK], px[TOPK], py[TOPK], pz[TOPK];
#pragma unroll
        for (int t = 0; t < TOPK; ++t) {
            const size_t o = row * topk + (t < topk ? t : 0);
            col[t] = pi_idx[o], w[t] = pi_val[o];
        }
#pragma unroll
        for (int t = 0; t < TOPK; ++t) {
            const float *p = nb2 + (size_t)col[t] * k * 3;
            px[t] = p[0], py[t] = p[1], pz[t] = p[2];
        }
        const float *p12 = verts12 + ((size_t)b * N + idx11[row * k + s]) * 3;
        float e0, e1, e2c;
        e2 = map_term_resid<TOPK>(w, px, py, pz, topk, p12[0], p12[1], p12[2], e0, e1, e2c);
    }
    map_term_block_partial(e2, b, partial);
}

// out[b] = scale * sum_q partial[b,q]   (one block per b, fixed order)
__global__ void reduce_partials_kernel(const double *__restrict__ partial, int nparts, float scale, float *__restrict__ out,
                                       int out_stride, int out_off) {
    const int b = blockIdx.x;
    double s = 0.0;
    for (int q = threadIdx.x; q < nparts; q += blockDim.x) s += partial[(size_t)b * nparts + q];
    s = block_tree_sum(s);
    if (threadIdx.x == 0) out[(size_t)b * out_stride + out_off] = (float)(s * (double)scale);
}

// out[q][b*stride+off[q]] = scale * mean(in[q][b, 0..n[q])) for up to eight inputs in one launch (blockIdx.y = input), fixed-order double
// accumulation: the pair path reduces its eight Chamfer terms at once, launch_mean is the one-input case
struct MeanGroups {
    const float *in[8];
    float *out[8];
    int n[8], off[8];
};
__global__ void mean_grouped_kernel(const MeanGroups g, float scale, int out_stride) {
    const int b = blockIdx.x, q8 = blockIdx.y;
    const float *in = g.in[q8];
    const int n = g.n[q8];
    double s = 0.0;
    for (int q = threadIdx.x; q < n; q += blockDim.x) s += (double)in[(size_t)b * n + q];
    s = block_tree_sum(s);
    if (threadIdx.x == 0) g.out[q8][(size_t)b * out_stride + g.off[q8]] = (float)(s / (double)n * (double)scale);
}

}  // namespace dvm

using namespace dvm;

static int argmin_all_columns(const float *f1, const float *f2, int B, int N, int M, int d, int32_t *T, float *dmin, hipStream_t s) {
    size_t lds = (size_t)AM_KT * d * sizeof(float);
    ensure_dyn_lds((const void *)argmin_exact_kernel, 65536);
    hipLaunchKernelGGL(argmin_exact_kernel, dim3((N + 127) / 128, B), dim3(128), lds, s, f1, f2, N, M, d, T, dmin);
    DVM_CHECK_LAUNCH("argmin_exact");
    return DVM_OK;
}

DVM_EXPORT size_t dvm_argmin_workspace_bytes(int B, int N, int M, int d, int both_directions) {
    return d == 128 ? argmin_f16_ws_bytes(B, N, M, both_directions != 0) : 0;
}

DVM_EXPORT int dvm_argmin_exact_f32(const float *f1, const float *f2, int B, int N, int M, int d, int32_t *T, float *dmin,
                                    void *ws, size_t ws_bytes, void *stream) {
    DVM_REQUIRE(f1 && f2 && T, "dvm_argmin_exact_f32: null pointer");
    DVM_REQUIRE(B >= 1 && N >= 1 && M >= 1, "dvm_argmin_exact_f32: empty input (B=%d N=%d M=%d)", B, N, M);
    DVM_REQUIRE(d >= 4 && d % 4 == 0 && d <= 512, "dvm_argmin_exact_f32: d=%d unsupported (need d%%4==0, 4<=d<=512)", d);
    if (ws != nullptr && d == 128) {
        const K1HardOut out{T, dmin};
        int rc = launch_argmin_f16(K1Sides{{f1, f2}, {nullptr, nullptr}, B, {N, M}, false}, &out, ws, ws_bytes, (hipStream_t)stream);
        if (rc != DVM_OK) return rc;
        DVM_CHECK_LAUNCH("argmin_exact(sweep)");
        return DVM_OK;
    }
    return argmin_all_columns(f1, f2, B, N, M, d, T, dmin, (hipStream_t)stream);
}

DVM_EXPORT int dvm_argmin_pair_f32(const float *f1, const float *f2, int B, int N, int M, int d, int32_t *T12, int32_t *T21,
                                   float *dmin12, float *dmin21, void *ws, size_t ws_bytes, void *stream) {
    DVM_REQUIRE(f1 && f2 && T12 && T21, "dvm_argmin_pair_f32: null pointer");
    DVM_REQUIRE(B >= 1 && N >= 1 && M >= 1, "dvm_argmin_pair_f32: empty input (B=%d N=%d M=%d)", B, N, M);
    DVM_REQUIRE(d >= 4 && d % 4 == 0 && d <= 512, "dvm_argmin_pair_f32: d=%d unsupported (need d%%4==0, 4<=d<=512)", d);
    if (ws != nullptr && d == 128) {
        const K1HardOut out[2] = {{T12, dmin12}, {T21, dmin21}};
        int rc = launch_argmin_f16(K1Sides{{f1, f2}, {nullptr, nullptr}, B, {N, M}, true}, out, ws, ws_bytes, (hipStream_t)stream);
        if (rc != DVM_OK) return rc;
        DVM_CHECK_LAUNCH("argmin_pair(sweep)");
        return DVM_OK;
    }
    int rc = argmin_all_columns(f1, f2, B, N, M, d, T12, dmin12, (hipStream_t)stream);
    if (rc != DVM_OK) return rc;
    return argmin_all_columns(f2, f1, B, M, N, d, T21, dmin21, (hipStream_t)stream);
}

DVM_EXPORT size_t dvm_knn_cdist_workspace_bytes(int B, int N, int M, int C) {
    (void)M;
    return C == 3 ? grid_bytes(B, N) : 256;   // (the grid of the self-search; any other case needs none)
}

DVM_EXPORT int dvm_knn_cdist_f32(const float *x, const float *y, int B, int N, int M, int C, int k, int32_t *idx, void *ws,
                                 size_t ws_bytes, void *stream) {
    DVM_REQUIRE(x && y && idx, "dvm_knn_cdist_f32: null pointer");
    DVM_REQUIRE(B >= 1 && N >= 1 && M >= 1, "dvm_knn_cdist_f32: empty input (B=%d N=%d M=%d)", B, N, M);
    DVM_REQUIRE(C >= 1 && C <= 16, "dvm_knn_cdist_f32: C=%d unsupported (1..16)", C);
    DVM_REQUIRE(k >= 1 && k <= 16, "dvm_knn_cdist_f32: k=%d unsupported (1..16)", k);
    dim3 grid((N + 127) / 128, B), block(128);
    hipStream_t s = (hipStream_t)stream;
    if (C == 3 && x == y && N == M && N >= 64 && ws != nullptr) {
        // a cloud against itself (the hot-path case): exact search on a uniform grid
        Arena ar(ws, ws_bytes);
        GridBuf gb = grid_carve(ar, B, N);
        if (!arena_fits(ar, "dvm_knn_cdist_f32")) return DVM_ENOSPACE;
        launch_grid_build(x, B, N, nullptr, gb, s);
        launch_grid_knn_self(gb, B, k, idx, s);
        DVM_CHECK_LAUNCH("knn_cdist(grid)");
        return DVM_OK;
    }
    if (C == 3) {
        if (k <= 3)
            hipLaunchKernelGGL(knn_cdist3_kernel<3>, grid, block, 0, s, x, y, N, M, k, idx);
        else if (k <= 10)
            hipLaunchKernelGGL(knn_cdist3_kernel<10>, grid, block, 0, s, x, y, N, M, k, idx);
        else
            hipLaunchKernelGGL(knn_cdist3_kernel<16>, grid, block, 0, s, x, y, N, M, k, idx);
    } else {
        if (k <= 10)
            hipLaunchKernelGGL(knn_cdist_kernel<10>, grid, block, 0, s, x, y, N, M, C, k, idx);
        else
            hipLaunchKernelGGL(knn_cdist_kernel<16>, grid, block, 0, s, x, y, N, M, C, k, idx);
    }
    DVM_CHECK_LAUNCH("knn_cdist");
    return DVM_OK;
}

DVM_EXPORT int dvm_softcorr_apply_f32(const float *pi_val, const int32_t *pi_idx, const float *V, int B, int N, int M,
                                      int topk, int C, float *out, void *stream) {
    DVM_REQUIRE(pi_val && pi_idx && V && out, "dvm_softcorr_apply_f32: null pointer");
    DVM_REQUIRE(B >= 1 && N >= 1 && M >= 1 && C >= 1, "dvm_softcorr_apply_f32: empty input");
    DVM_REQUIRE(topk >= 1 && topk <= 16, "dvm_softcorr_apply_f32: topk=%d unsupported (1..16)", topk);
    launch_apply(pi_val, pi_idx, V, B, N, M, topk, C, out, (hipStream_t)stream);
    DVM_CHECK_LAUNCH("softcorr_apply");
    return DVM_OK;
}

namespace dvm {
// dvm_softcorr_apply_f32 without its checks (topk <= 16; every index must lie in [0, M): it becomes an address)
void launch_apply(const float *pi_val, const int32_t *pi_idx, const float *V, int B, int N, int M, int topk, int C, float *out, hipStream_t s) {
    long threads = (long)N * ((C + 3) / 4);
    dim3 grid((unsigned)((threads + 255) / 256), B), block(256);
    if (topk <= 10)
        hipLaunchKernelGGL(apply_kernel<10>, grid, block, 0, s, pi_val, pi_idx, V, N, M, topk, C, out);
    else
        hipLaunchKernelGGL(apply_kernel<16>, grid, block, 0, s, pi_val, pi_idx, V, N, M, topk, C, out);
}
// The pieces of dvm_softcorr_apply_bwd_f32's gather form, for callers that keep the reversed lists (dvm_criterion_train.hip)
void launch_apply_bwd_dval(const float *pi_val, const int32_t *pi_idx, const float *V, const float *g_out, int B, int N, int M, int topk, int C,
                           float *d_val, hipStream_t s) {
    int gp2 = 1;
    while (gp2 < (C + 3) / 4) gp2 <<= 1;
    dim3 grid((unsigned)(((long)N * gp2 + 255) / 256), B);
    hipLaunchKernelGGL(apply_bwd_kernel, grid, dim3(256), 0, s, pi_val, pi_idx, V, g_out, N, M, topk, C, gp2, d_val, (float *)nullptr);
}
void launch_apply_bwd_gather(const float *pi_val, const float *g_out, const int32_t *offs, const int32_t *edges, int B, int N, int M, int topk, int C,
                             float *d_V, hipStream_t s) {
    hipLaunchKernelGGL(apply_bwd_gather_kernel, dim3((M + 3) / 4, B), dim3(256), 0, s, pi_val, g_out, offs, edges, N, M, topk, C, d_V);
}
}  // namespace dvm

static size_t carve_rev_csr(Arena &ar, int B, int N, int M, int topk, RevLists &w) {
    w.take(ar, B, M, (size_t)N * topk);
    return ar.off;
}

DVM_EXPORT size_t dvm_softcorr_apply_bwd_workspace_bytes(int B, int N, int M, int topk) { return null_carve<RevLists>(carve_rev_csr, B, N, M, topk); }

DVM_EXPORT int dvm_softcorr_apply_bwd_f32(const float *pi_val, const int32_t *pi_idx, const float *V, const float *g_out, int B,
                                          int N, int M, int topk, int C, float *d_val, float *d_V, void *ws, size_t ws_bytes,
                                          void *stream) {
    DVM_REQUIRE(pi_val && pi_idx && V && g_out && d_val && d_V, "dvm_softcorr_apply_bwd_f32: null pointer");
    DVM_REQUIRE(B >= 1 && N >= 1 && M >= 1 && C >= 1, "dvm_softcorr_apply_bwd_f32: empty input");
    DVM_REQUIRE(C <= 256, "dvm_softcorr_apply_bwd_f32: C=%d unsupported (<= 256)", C);
    DVM_REQUIRE(topk >= 1 && topk <= 64, "dvm_softcorr_apply_bwd_f32: topk=%d unsupported (1..64)", topk);
    int gp2 = 1;
    while (gp2 < (C + 3) / 4) gp2 <<= 1;
    hipStream_t s = (hipStream_t)stream;
    long threads = (long)N * gp2;
    dim3 grid((unsigned)((threads + 255) / 256), B), block(256);
    if (ws != nullptr) {  // reversed lists + gather: no float atomics
        RevLists w;
        if (!carve_ws(ws, ws_bytes, "dvm_softcorr_apply_bwd_f32", w, carve_rev_csr, B, N, M, topk)) return DVM_ENOSPACE;
        launch_rev_csr(pi_idx, B, (long)N * topk, M, w, s);
        launch_apply_bwd_dval(pi_val, pi_idx, V, g_out, B, N, M, topk, C, d_val, s);
        launch_apply_bwd_gather(pi_val, g_out, w.offs, w.edges, B, N, M, topk, C, d_V, s);
        DVM_CHECK_LAUNCH("softcorr_apply_bwd(gather)");
        return DVM_OK;
    }
    (void)hipMemsetAsync(d_V, 0, (size_t)B * M * C * sizeof(float), s);
    hipLaunchKernelGGL(apply_bwd_kernel, grid, block, 0, s, pi_val, pi_idx, V, g_out, N, M, topk, C, gp2, d_val, d_V);
    DVM_CHECK_LAUNCH("softcorr_apply_bwd");
    return DVM_OK;
}

struct ChamferWs {
    GridBuf ga, gb;   // the grids of both clouds
};
static size_t carve_chamfer(Arena &ar, int B, int N, int M, ChamferWs &w) {
    w.ga = grid_carve(ar, B, N), w.gb = grid_carve(ar, B, M);
    return ar.off;
}

DVM_EXPORT size_t dvm_chamfer_workspace_bytes(int B, int N, int M) { return null_carve<ChamferWs>(carve_chamfer, B, N, M); }

DVM_EXPORT int dvm_chamfer_fwd_f32(const float *a, const float *b, int B, int N, int M, float *d1, float *d2, int32_t *i1,
                                   int32_t *i2, void *ws, size_t ws_bytes, void *stream) {
    DVM_REQUIRE(a && b && (d1 || d2), "dvm_chamfer_fwd_f32: null pointer");
    DVM_REQUIRE(B >= 1 && N >= 1 && M >= 1, "dvm_chamfer_fwd_f32: empty input (B=%d N=%d M=%d)", B, N, M);
    hipStream_t s = (hipStream_t)stream;
    // Few queries (a training batch: 8 x 2048 per side): the uniform-grid search is a per-thread walk whose length is set
    // by the queries farthest from the target's box (an untrained warp: most of the grid) — 279 us per call with 128
    // workgroups in flight; scanning the whole target from LDS tiles costs 2048 x 8 flops per query and finishes in a
    // fraction of that.  Same minima, same tie rule (lowest index).  The grid pays from ~100 k queries on (the pair bench).
    const bool few = (long)B * ((d1 ? N : 0) + (d2 ? M : 0)) <= 65536 && (long)N * M <= (1L << 25);
    if (ws != nullptr && N >= 64 && M >= 64 && !few) {
        ChamferWs w;
        if (!carve_ws(ws, ws_bytes, "dvm_chamfer_fwd_f32", w, carve_chamfer, B, N, M)) return DVM_ENOSPACE;
        const GridBuf &ga = w.ga, &gb = w.gb;
        GridBuf qg[2] = {ga, gb}, tg[2] = {gb, ga};
        float *dout[2] = {d1, d2};
        int32_t *iout[2] = {i1, i2};
        launch_grid_build(b, B, M, nullptr, gb, s);
        launch_grid_build(a, B, N, nullptr, ga, s);
        if (d1 && d2) {
            launch_grid_chamfer(qg, tg, dout, iout, 2, B, s);
        } else if (d1) {
            launch_grid_chamfer(qg, tg, dout, iout, 1, B, s);
        } else {
            launch_grid_chamfer(qg + 1, tg + 1, dout + 1, iout + 1, 1, B, s);
        }
        DVM_CHECK_LAUNCH("chamfer(grid)");
        return DVM_OK;
    }
    auto nn = [&](const float *q, const float *t, int nq, int nt, float *d, int32_t *ix) {
        if (nt <= 8192) {   // 16 bytes per target point: 128 KB of the CU's 160 KB at most
            const size_t lds = (size_t)nt * sizeof(float4);
            ensure_dyn_lds((const void *)chamfer_split_kernel, 128 * 1024);
            hipLaunchKernelGGL(chamfer_split_kernel, dim3((nq + 63) / 64, B), dim3(256), lds, s, q, t, nq, nt, d, ix);
        } else {
            hipLaunchKernelGGL(chamfer_kernel, dim3((nq + 127) / 128, B), dim3(128), 0, s, q, t, nq, nt, d, ix);
        }
    };
    if (d1) nn(a, b, N, M, d1, i1);
    if (d2) nn(b, a, M, N, d2, i2);
    DVM_CHECK_LAUNCH("chamfer");
    return DVM_OK;
}

static size_t carve_map_term(Arena &ar, int B, int N, int k, double *&partial) {   // one partial per workgroup
    partial = ar.take<double>((size_t)B * map_term_blocks(N, k));
    return ar.off;
}

DVM_EXPORT size_t dvm_map_term_workspace_bytes(int B, int N) {
    return null_carve<double *>(carve_map_term, B, N, 16);   // (the query does not know k: sized for the largest, 16)
}

DVM_EXPORT int dvm_map_term_f32(const float *verts12, const float *verts2, const int32_t *idx11, const int32_t *idx22,
                                const float *pi_val, const int32_t *pi_idx, int B, int N, int M, int k, int topk, float *out,
                                void *ws, size_t ws_bytes, void *stream) {
    DVM_REQUIRE(verts12 && verts2 && idx11 && idx22 && pi_val && pi_idx && out, "dvm_map_term_f32: null pointer");
    DVM_REQUIRE(B >= 1 && N >= 1 && M >= 1, "dvm_map_term_f32: empty input");
    DVM_REQUIRE(k >= 1 && k <= 16 && topk >= 1 && topk <= 16, "dvm_map_term_f32: k/topk out of range");
    const int nblk = map_term_blocks(N, k);
    double *partial;
    if (!carve_ws(ws, ws_bytes, "dvm_map_term_f32", partial, carve_map_term, B, N, k)) return DVM_ENOSPACE;
    hipStream_t s = (hipStream_t)stream;
    if (topk <= 10)
        hipLaunchKernelGGL(map_term_kernel<10>, dim3(nblk, B), dim3(256), 0, s, verts12, verts2, idx11, idx22, pi_val, pi_idx,
                           N, M, k, topk, partial, (float *)nullptr);
    else
        hipLaunchKernelGGL(map_term_kernel<16>, dim3(nblk, B), dim3(256), 0, s, verts12, verts2, idx11, idx22, pi_val, pi_idx,
                           N, M, k, topk, partial, (float *)nullptr);
    hipLaunchKernelGGL(reduce_partials_kernel, dim3(B), dim3(256), 0, s, partial, nblk, 1.0f, out, 1, 0);
    DVM_CHECK_LAUNCH("map_term");
    return DVM_OK;
}

// internal helpers used by dvm_pair.hip
namespace dvm {
int launch_mean_grouped(const float *const *in, const int *n, float *const *out, const int *off, int ngroups, int B, float scale,
                        int stride, hipStream_t s) {
    MeanGroups g;
    for (int q = 0; q < 8; ++q) {
        const int r = q < ngroups ? q : 0;
        g.in[q] = in[r], g.out[q] = out[r], g.n[q] = n[r], g.off[q] = off[r];
    }
    hipLaunchKernelGGL(mean_grouped_kernel, dim3(B, ngroups), dim3(256), 0, s, g, scale, stride);
    return DVM_OK;
}
int launch_mean(const float *in, int B, int n, float scale, float *out, int stride, int off, hipStream_t s) {
    return launch_mean_grouped(&in, &n, &out, &off, 1, B, scale, stride, s);
}
int launch_reduce_partials(const double *partial, int B, int nparts, float scale, float *out, int stride, int off,
                           hipStream_t s) {
    hipLaunchKernelGGL(reduce_partials_kernel, dim3(B), dim3(256), 0, s, partial, nparts, scale, out, stride, off);
    return DVM_OK;
}
int map_term_blocks(int N, int k) { return (int)(((long)N * k + 255) / 256); }
void launch_gather_nbr_xyz(const float *verts, const int32_t *idx, int B, int M, int k, float *nbr, hipStream_t s) {
    hipLaunchKernelGGL(gather_nbr_xyz_kernel, dim3((unsigned)(((long)M * k + 255) / 256), B), dim3(256), 0, s, verts, idx, M, k, nbr);
}
int launch_map_term_nbr(const float *verts12, const float *nbr2, const int32_t *idx11, const float *pi_val, const int32_t *pi_idx,
                        int B, int N, int M, int k, int topk, double *partial, hipStream_t s) {
    int nblk = map_term_blocks(N, k);
    hipLaunchKernelGGL(map_term_nbr_kernel<10>, dim3(nblk, B), dim3(256), 0, s, verts12, nbr2, idx11, pi_val, pi_idx, N, M, k, topk,
                       partial);
    return DVM_OK;
}
// -> false if a target cloud does not fit LDS (the caller then uses apply_kernel + take_col0)
bool launch_apply3_pair(const float *val12, const int32_t *idx12, const float *verts2, float *verts12, int32_t *T12, const float *val21,
                        const int32_t *idx21, const float *verts1, float *verts21, int32_t *T21, int B, int N, int M, hipStream_t s) {
    const size_t lds = (size_t)(N > M ? N : M) * 3 * sizeof(float);
    if (lds > 150 * 1024) return false;
    Apply3Pair a;
    a.val[0] = val12, a.idx[0] = idx12, a.V[0] = verts2, a.out[0] = verts12, a.T[0] = T12, a.N[0] = N, a.M[0] = M;
    a.val[1] = val21, a.idx[1] = idx21, a.V[1] = verts1, a.out[1] = verts21, a.T[1] = T21, a.N[1] = M, a.M[1] = N;
    ensure_dyn_lds((const void *)apply3_pair_kernel, (int)lds);
    hipLaunchKernelGGL(apply3_pair_kernel, dim3(B, 2), dim3(256), lds, s, a);
    return true;
}
// LDS of a workgroup: the target's coordinates and xyz-kNN table + the mapped cloud's coordinates (up to 2 x M points of it)
static size_t map_term_lds_bytes(int N, int M, int k) { return (size_t)(M + N) * sizeof(float4) + (size_t)M * k * sizeof(int32_t); }
bool map_term_lds_applies(int N, int M, int k) { return k == 10 && map_term_lds_bytes(N, M, k) <= 150 * 1024; }
// the LDS form on nd = 1 or 2 directions of B pairs in one launch (blockIdx.y = direction) -> true if it ran (topk == 10, k == 10, the
// larger side's tables fit 150 KB of LDS); else nothing is launched and the caller uses one of the older forms
static bool map_term_lds_run(const MapTermSide &d0, const MapTermSide &d1, int nd, int B, int k, int topk, hipStream_t s) {
    const size_t l0 = map_term_lds_bytes(d0.N, d0.M, k), l1 = map_term_lds_bytes(d1.N, d1.M, k), lds = l0 > l1 ? l0 : l1;
    if (topk != 10 || k != 10 || lds > 150 * 1024) return false;
    ensure_dyn_lds((const void *)map_term_lds_kernel<10>, (int)lds);
    MapTermArgs a;
    a.d[0] = d0, a.d[1] = d1;
    a.k = k;
    hipLaunchKernelGGL(map_term_lds_kernel<10>, dim3(B, nd), dim3(1024), lds, s, a);
    return true;
}
bool launch_map_term_lds(const float *verts12, const float *verts2, const int32_t *idx11, const int32_t *idx22, const float *pi_val,
                         const int32_t *pi_idx, int B, int N, int M, int k, int topk, double *partial, hipStream_t s) {
    const MapTermSide d{verts12, verts2, idx11, idx22, pi_val, pi_idx, N, M, map_term_blocks(N, k), partial};
    return map_term_lds_run(d, d, 1, B, k, topk, s);
}
// both directions of B pairs in one launch (direction 0: N sources against M targets; direction 1: the reverse); same partial sums
bool launch_map_term_lds_pair(const float *verts12, const float *verts21, const float *verts1, const float *verts2, const int32_t *idx11,
                              const int32_t *idx22, const float *val12, const int32_t *pidx12, const float *val21, const int32_t *pidx21, int B,
                              int N, int M, int k, int topk, double *partial12, double *partial21, hipStream_t s) {
    return map_term_lds_run(MapTermSide{verts12, verts2, idx11, idx22, val12, pidx12, N, M, map_term_blocks(N, k), partial12},
                            MapTermSide{verts21, verts1, idx22, idx11, val21, pidx21, M, N, map_term_blocks(M, k), partial21}, 2, B, k, topk, s);
}
int launch_map_term(const float *verts12, const float *verts2, const int32_t *idx11, const int32_t *idx22,
                    const float *pi_val, const int32_t *pi_idx, int B, int N, int M, int k, int topk, double *partial,
                    hipStream_t s, float *resid) {
    int nblk = map_term_blocks(N, k);
    hipLaunchKernelGGL(map_term_kernel<10>, dim3(nblk, B), dim3(256), 0, s, verts12, verts2, idx11, idx22, pi_val, pi_idx, N,
                       M, k, topk, partial, resid);
    return DVM_OK;
}
}  // namespace dvm
