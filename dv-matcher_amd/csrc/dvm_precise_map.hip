// dvm_precise_map.hip — the precise (vertex-to-point) map: for a source feature p, the closest point of the target's triangle
// mesh embedded in feature space, as a face and three barycentric weights.  Not in the reference (include/dvm.h has the
// definition); opt-in beside the vertex map of dvm_argmin_exact_f32.
//
// Notation for one face (a,b,c) and one row p: A = f2[a], w = A - p, e1 = f2[b] - A, e2 = f2[c] - A, and the six numbers
//   ww = w.w   d1 = e1.w   d2 = e2.w   e11 = e1.e1   e12 = e1.e2   e22 = e2.e2        (e33 = |f2[c] - f2[b]|^2)
// A point of the face is A + s e1 + t e2 with (s,t) in the simplex s,t >= 0, s + t <= 1, and its squared distance to p is
//   Q(s,t) = ww + 2 (s d1 + t d2) + s^2 e11 + 2 s t e12 + t^2 e22.
// Four candidates are formed: the closest point of each edge as a segment (a clamped 1-D minimum) and, where the face's Gram
// determinant det = e11 e22 - e12^2 exceeds its own product rounding (det > 8u e11 e22, u = 2^-24; below that the face is the
// union of its edges), the stationary point of Q if it lies in the simplex.  Every candidate is a point OF the face.
//
// EXACT FORM (pass 2, and the definition of the result).  ww, d1, d2 are k-ordered fmaf chains over the differences
// fl(A_k - p_k), fl(B_k - A_k), fl(C_k - A_k); e11, e12, e22, e33 are such chains from the face record; the four (s,t) by
// correctly rounded divisions; then the four residuals r = w + s e1 + t e2 are formed and v = |r|^2 summed, and the smallest v
// is the face's value (a NaN counts as +inf).  The row's answer is the smallest (v, face index).  v is the squared distance
// of a real point of the face to within (d + 4) u relative, whatever the cancellation in Q.
//
// SCREEN (pass 1).  The prologue writes per face: its indices, naa = |A|^2, ae1 = A.e1, ae2 = A.e2 (chains over differences),
// e11, e12, e22, e33, det, 1/det (0: no interior candidate), nmax = max |f2[.]|^2 of its corners and the curvature bound xr
// below.  A workgroup holds G[j] = p.f2[j] for its rows in LDS and, with P = |p|^2, takes
//   ww~ = (P - 2 G[a]) + naa      d1~ = ae1 - (G[b] - G[a])      d2~ = ae2 - (G[c] - G[a])
// and T~ = the smallest Q~ over the same four candidates, from the formula.  With S = P + nmax (so |w|^2 <= 2S, |e|^2 <= 4S,
// |d1|, |d2| <= 2.83 S) and g = d u / (1 - d u) for a d-term sum in any order:
//   |ww~ - ww| <= g (P + 2 |p||A| + naa) + 4u S <= (2d + 4) u S
//   |d1~ - d1| <= (g + u) |A||e1| + g (|p||A| + |p||B|) + 4u S <= (3d + 6) u S =: eta       (d2 alike)
//   min over the simplex moves by at most |dww| + 2 max(|dd1|, |dd2|) <= (8d + 16) u S        (s + t <= 1)
//   the record's e11, e12, e22 against the real ones: (d + 1) u (e11 + 2|e12| + e22) <= 16 (d + 1) u S
//   evaluating Q~ at a point of the simplex in fp32 (terms sum to at most 30 S, 8 nested roundings, 1-ulp reciprocals):
//   <= 512 u S;  pass 2's own chains against the real numbers: (8d + 16) u S, its v: (d + 4) u 2S.
// These first-order terms of both passes sum to (34d + 568) u S; E = (40d + 1024) u S is taken (the slack also covers
// g against d u and S as computed against S).  What is left is second order: a candidate's (s,t) is computed from perturbed
// d1, d2, and Q at a point that misses a minimum by delta exceeds it by delta^T H delta.  On an edge of squared length e that
// is eta^2 / e (4 eta^2 / e33 on the edge b-c, whose numerator carries both d1 and d2), in the interior at most
// 2 eta^2 (e11 + e22) / det (the smallest eigenvalue of [[e11,e12],[e12,e22]] is at least det / (e11 + e22); the guard on det
// keeps the stored matrix positive definite, so a stationary point the fp32 test places just outside the simplex is matched
// by an edge point within the same excess).  With xr = max(1/e11, 1/e22, 4/e33, 2 (e11 + e22) / det) from the record,
// X = 32 (d + 2)^2 u^2 S^2 xr bounds the excess of both passes (eta^2 = 9 (d + 2)^2 u^2 S^2 in pass 1, at most 8 (d + 2)^2
// u^2 S^2 in pass 2).  An edge of length exactly 0 has d1 = 0 in both passes (identical rows give identical G) and no excess.
//   Hence for every face   T~ - (E + X) <= v <= T~ + (E + X).
// Pass 1 keeps m = min over faces of T~ + (E + X); pass 2 evaluates every face with NOT (T~ - (E + X) > m).  The face g that
// attains m is evaluated and has v_g <= m; a face left out has v > m >= v_g, strictly, so it cannot win or tie: the result is
// the exact form's arg-min over all faces.  The band between two faces is the sum of their two bounds — twice the bound.  It
// scales with |p|^2 + max |f2|^2, not with the distance: where the Gram form cancels (a large common offset) every face passes
// and the call costs N F exact evaluations — slower, not wrong.  NaN or Inf anywhere makes the comparison false and the face
// is evaluated.
#include "dvm_common.h"

namespace dvm {

// source rows per workgroup (their G rows share LDS and every record load), threads, target rows per G-fill step (waves x 4
// x 8: eight lanes share a target row), the largest M (PM_ROWS x M words of LDS: 128 KiB) and d (dvm_softcorr's)
constexpr int PM_ROWS = 4, PM_THREADS = 512, PM_WAVES = PM_THREADS / 64, PM_CHUNK = PM_WAVES * 32, PM_MAX_M = 8192, PM_MAX_D = 512;
constexpr float PM_U = 5.9604644775390625e-8f;   // 2^-24
static_assert(PM_ROWS == 4, "the rows' products with one target vertex are one float4 of LDS");

struct PmWs {
    float4 *rec;               // [4][B][F]: (a, b, c, -) | (naa, ae1, ae2, nmax) | (e11, e12, e22, e33) | (1/det, xr, det, -)
    unsigned long long *cnt;   // where the caller wants no stats
};
static size_t carve_precise_map(Arena &ar, int B, int F, PmWs &w) {
    w.rec = ar.take<float4>((size_t)4 * B * F);
    w.cnt = ar.take<unsigned long long>(2);
    return ar.off;
}

__device__ __forceinline__ float pm_clamp01(float x) { return fminf(fmaxf(x, 0.f), 1.f); }   // (a NaN becomes 0)
// the smaller of two, a NaN if either is one
__device__ __forceinline__ float pm_min_nan(float a, float b) { return a < b ? a : (b <= a ? b : NAN); }
__device__ __forceinline__ float pm_sticky_max(float a, float b) { return (b > a || b != b) ? b : a; }

// Prologue: one thread per (b, face).  A face with an index outside [0, M) gets a = -1 and is counted once (for b = 0).
__global__ __launch_bounds__(256) void pm_record_kernel(const float *__restrict__ f2, const int32_t *__restrict__ faces, int M, int d, int F,
                                                        float4 *__restrict__ rec, unsigned long long *__restrict__ cnt) {
    const int b = blockIdx.y, f = blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    const size_t BF = (size_t)gridDim.y * F, at = (size_t)b * F + f;
    const int ia = faces[3 * (size_t)f], ib = faces[3 * (size_t)f + 1], ic = faces[3 * (size_t)f + 2];
    if ((unsigned)ia >= (unsigned)M || (unsigned)ib >= (unsigned)M || (unsigned)ic >= (unsigned)M) {
        const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
        rec[at] = make_float4(__int_as_float(-1), __int_as_float(-1), __int_as_float(-1), 0.f);
        rec[BF + at] = z, rec[2 * BF + at] = z, rec[3 * BF + at] = z;
        if (b == 0) atomicAdd(cnt, 1ull);
        return;
    }
    const float4 *__restrict__ A = (const float4 *)(f2 + ((size_t)b * M + ia) * d);
    const float4 *__restrict__ Bv = (const float4 *)(f2 + ((size_t)b * M + ib) * d);
    const float4 *__restrict__ C = (const float4 *)(f2 + ((size_t)b * M + ic) * d);
    float naa = 0.f, nbb = 0.f, ncc = 0.f, ae1 = 0.f, ae2 = 0.f, e11 = 0.f, e12 = 0.f, e22 = 0.f, e33 = 0.f;
    for (int k4 = 0; k4 < d / 4; ++k4) {
        const float4 a4 = A[k4], b4 = Bv[k4], c4 = C[k4];
        const float av[4] = {a4.x, a4.y, a4.z, a4.w}, bv[4] = {b4.x, b4.y, b4.z, b4.w}, cv[4] = {c4.x, c4.y, c4.z, c4.w};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float u1 = bv[q] - av[q], u2 = cv[q] - av[q], u3 = cv[q] - bv[q];
            naa = fmaf(av[q], av[q], naa), nbb = fmaf(bv[q], bv[q], nbb), ncc = fmaf(cv[q], cv[q], ncc);
            ae1 = fmaf(av[q], u1, ae1), ae2 = fmaf(av[q], u2, ae2);
            e11 = fmaf(u1, u1, e11), e12 = fmaf(u1, u2, e12), e22 = fmaf(u2, u2, e22), e33 = fmaf(u3, u3, e33);
        }
    }
    const float pr = e11 * e22, det = pr - e12 * e12;
    const bool interior = det > 8.f * PM_U * pr;   // (false for a NaN)
    const float idet = interior ? 1.f / det : 0.f;
    float xr = 0.f;
    if (e11 > 0.f) xr = pm_sticky_max(xr, 1.f / e11);
    if (e22 > 0.f) xr = pm_sticky_max(xr, 1.f / e22);
    if (e33 > 0.f) xr = pm_sticky_max(xr, 4.f / e33);
    if (interior) xr = pm_sticky_max(xr, 2.f * (e11 + e22) * idet);
    if (e11 != e11 || e22 != e22 || e33 != e33 || e12 != e12) xr = NAN;
    rec[at] = make_float4(__int_as_float(ia), __int_as_float(ib), __int_as_float(ic), 0.f);
    rec[BF + at] = make_float4(naa, ae1, ae2, fmaxf(naa, fmaxf(nbb, ncc)));
    rec[2 * BF + at] = make_float4(e11, e12, e22, e33);
    rec[3 * BF + at] = make_float4(idet, xr, det, 0.f);
}

// what pass 1 and pass 2 need of a record beside the row: reciprocals once per face
struct PmFace {
    float naa, ae1, ae2, nmax, e11, e12, e22, e33, idet, xr, i11, i22, i33;
};
__device__ __forceinline__ PmFace pm_face(float4 r1, float4 r2, float4 r3) {
    PmFace fc;
    fc.naa = r1.x, fc.ae1 = r1.y, fc.ae2 = r1.z, fc.nmax = r1.w;
    fc.e11 = r2.x, fc.e12 = r2.y, fc.e22 = r2.z, fc.e33 = r2.w;
    fc.idet = r3.x, fc.xr = r3.y;
    fc.i11 = fc.e11 > 0.f ? __builtin_amdgcn_rcpf(fc.e11) : 0.f;
    fc.i22 = fc.e22 > 0.f ? __builtin_amdgcn_rcpf(fc.e22) : 0.f;
    fc.i33 = fc.e33 > 0.f ? __builtin_amdgcn_rcpf(fc.e33) : 0.f;
    return fc;
}

// The Gram form of one (row, face): T~ and its margin E + X (header comment).
__device__ __forceinline__ void pm_screen(float P, float ga, float gb, float gc, const PmFace &fc, float cE, float cX, float &T, float &margin) {
    const float ww = fmaf(-2.f, ga, P) + fc.naa;
    const float d1 = fc.ae1 - (gb - ga), d2 = fc.ae2 - (gc - ga);
    const float t1 = pm_clamp01(-d1 * fc.i11), t2 = pm_clamp01(-d2 * fc.i22);
    const float qab = fmaf(t1, fmaf(t1, fc.e11, 2.f * d1), ww);
    const float qac = fmaf(t2, fmaf(t2, fc.e22, 2.f * d2), ww);
    const float wb = fmaf(2.f, d1, ww) + fc.e11, nb = (d2 - d1) + (fc.e12 - fc.e11);
    const float t3 = pm_clamp01(-nb * fc.i33);
    const float qbc = fmaf(t3, fmaf(t3, fc.e33, 2.f * nb), wb);
    const float s = (fc.e12 * d2 - fc.e22 * d1) * fc.idet, t = (fc.e12 * d1 - fc.e11 * d2) * fc.idet;
    const bool in = fc.idet > 0.f && s >= 0.f && t >= 0.f && s + t <= 1.f;
    const float qi = fmaf(s, fmaf(s, fc.e11, fmaf(2.f * t, fc.e12, 2.f * d1)), fmaf(t, fmaf(t, fc.e22, 2.f * d2), ww));
    T = pm_min_nan(pm_min_nan(qab, qac), qbc);
    T = in ? pm_min_nan(T, qi) : T;
    const float S = P + fc.nmax;
    margin = fmaf(cX * S, S * fc.xr, cE * S);
}

// The exact form of one (row, face): p in LDS, the three target rows gathered.  -> v, the weights of the winning candidate.
__device__ __forceinline__ float pm_exact(const float4 *__restrict__ p4, const float4 *__restrict__ A, const float4 *__restrict__ Bv,
                                          const float4 *__restrict__ C, int d4, float e11, float e12, float e22, float e33, float det,
                                          bool interior, float &w0, float &w1, float &w2) {
    float ww = 0.f, d1 = 0.f, d2 = 0.f;
    for (int k4 = 0; k4 < d4; ++k4) {
        const float4 a4 = A[k4], b4 = Bv[k4], c4 = C[k4], q4 = p4[k4];
        const float av[4] = {a4.x, a4.y, a4.z, a4.w}, bv[4] = {b4.x, b4.y, b4.z, b4.w}, cv[4] = {c4.x, c4.y, c4.z, c4.w};
        const float pv[4] = {q4.x, q4.y, q4.z, q4.w};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float w = av[q] - pv[q], u1 = bv[q] - av[q], u2 = cv[q] - av[q];
            ww = fmaf(w, w, ww), d1 = fmaf(u1, w, d1), d2 = fmaf(u2, w, d2);
        }
    }
    const float t1 = e11 > 0.f ? pm_clamp01(-d1 / e11) : 0.f, t2 = e22 > 0.f ? pm_clamp01(-d2 / e22) : 0.f;
    const float nb = (d2 - d1) + (e12 - e11);
    const float t3 = e33 > 0.f ? pm_clamp01(-nb / e33) : 0.f, s3 = 1.f - t3;
    float s = 0.f, t = 0.f;
    bool in = false;
    if (interior) {
        s = (e12 * d2 - e22 * d1) / det, t = (e12 * d1 - e11 * d2) / det;
        in = s >= 0.f && t >= 0.f && s + t <= 1.f;
    }
    if (!in) s = t1, t = 0.f;   // (the edge a-b again: no fifth case below)
    float v0 = 0.f, v1 = 0.f, v2 = 0.f, v3 = 0.f;
    for (int k4 = 0; k4 < d4; ++k4) {
        const float4 a4 = A[k4], b4 = Bv[k4], c4 = C[k4], q4 = p4[k4];
        const float av[4] = {a4.x, a4.y, a4.z, a4.w}, bv[4] = {b4.x, b4.y, b4.z, b4.w}, cv[4] = {c4.x, c4.y, c4.z, c4.w};
        const float pv[4] = {q4.x, q4.y, q4.z, q4.w};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float w = av[q] - pv[q], u1 = bv[q] - av[q], u2 = cv[q] - av[q];
            const float r0 = fmaf(t1, u1, w), r1 = fmaf(t2, u2, w), r2 = fmaf(t3, u2, fmaf(s3, u1, w)), r3 = fmaf(t, u2, fmaf(s, u1, w));
            v0 = fmaf(r0, r0, v0), v1 = fmaf(r1, r1, v1), v2 = fmaf(r2, r2, v2), v3 = fmaf(r3, r3, v3);
        }
    }
    float v = v0;
    w0 = 1.f - t1, w1 = t1, w2 = 0.f;
    if (v1 < v) v = v1, w0 = 1.f - t2, w1 = 0.f, w2 = t2;
    if (v2 < v) v = v2, w0 = 0.f, w1 = s3, w2 = t3;
    if (in && v3 < v) v = v3, w0 = 1.f - (s + t), w1 = s, w2 = t;
    return v;
}

__device__ __forceinline__ unsigned long long pm_wave_min(unsigned long long k) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long other = __shfl_xor(k, o, 64);
        k = other < k ? other : k;
    }
    return k;
}

// Workgroup = PM_ROWS source rows of one batch entry.  LDS: G [M] float4 (the PM_ROWS rows' products with target j side by
// side: one 16-byte read per corner serves all rows), the rows themselves [PM_ROWS][d], and the reduction words.
__global__ __launch_bounds__(PM_THREADS) void pm_search_kernel(const float *__restrict__ f1, const float *__restrict__ f2,
                                                               const float4 *__restrict__ rec, int N, int M, int d, int F, float cE, float cX,
                                                               int32_t *__restrict__ face, float *__restrict__ bary, int32_t *__restrict__ pi_idx,
                                                               float *__restrict__ dist, unsigned long long *__restrict__ cnt) {
    extern __shared__ __attribute__((aligned(16))) float4 pm_lds[];
    float4 *G4 = pm_lds;                                        // [M]
    float4 *p4 = pm_lds + M;                                    // [PM_ROWS][d / 4]
    float *redf = (float *)(p4 + (size_t)PM_ROWS * (d / 4));    // [PM_WAVES][PM_ROWS]
    unsigned long long *redk = (unsigned long long *)(redf + PM_WAVES * PM_ROWS);   // [PM_WAVES][PM_ROWS] (8-byte aligned: a multiple of 4 floats before it)
    const int b = blockIdx.y, row0 = blockIdx.x * PM_ROWS, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int d4 = d / 4;
    const size_t BF = (size_t)gridDim.y * F;
    const float4 *__restrict__ rec0 = rec + (size_t)b * F, *__restrict__ rec1 = rec0 + BF, *__restrict__ rec2 = rec1 + BF,
                               *__restrict__ rec3 = rec2 + BF;
    const float *__restrict__ f2b = f2 + (size_t)b * M * d;

    // the rows (a row past N repeats row N - 1 and writes nothing)
    for (int i = tid; i < PM_ROWS * d4; i += PM_THREADS) {
        const int r = i / d4, k4 = i - r * d4;
        const int row = min(row0 + r, N - 1);
        p4[i] = ((const float4 *)(f1 + ((size_t)b * N + row) * d))[k4];
    }
    __syncthreads();
    float P[PM_ROWS];
#pragma unroll
    for (int r = 0; r < PM_ROWS; ++r) P[r] = 0.f;
    for (int k4 = 0; k4 < d4; ++k4) {
#pragma unroll
        for (int r = 0; r < PM_ROWS; ++r) {
            const float4 x = p4[r * d4 + k4];
            P[r] = fmaf(x.w, x.w, fmaf(x.z, x.z, fmaf(x.y, x.y, fmaf(x.x, x.x, P[r]))));
        }
    }

    // G: eight lanes share a target row (lane q takes the float4 columns q, q + 8, ..: a 128-byte line per row and load),
    // four target rows per lane group in flight; the eight partial sums are added by the xor-1, -2, -4 butterfly
    {
        const int q = lane & 7, g = lane >> 3;
        for (int j0 = wave * 32; j0 < M; j0 += PM_CHUNK) {
            float acc[4][PM_ROWS];
            int src[4];   // (M d / 4 <= 2^20)
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                src[u] = min(j0 + u * 8 + g, M - 1) * d4;
#pragma unroll
                for (int r = 0; r < PM_ROWS; ++r) acc[u][r] = 0.f;
            }
            for (int kb = 0; kb < d4; kb += 8) {
                const bool on = kb + q < d4;
                const int k4 = on ? kb + q : 0;
                float4 x[4], pr[PM_ROWS];   // (loaded at a valid column, then zeroed where this lane has none)
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const float4 t = ((const float4 *)f2b)[src[u] + k4];
                    x[u] = make_float4(on ? t.x : 0.f, on ? t.y : 0.f, on ? t.z : 0.f, on ? t.w : 0.f);
                }
#pragma unroll
                for (int r = 0; r < PM_ROWS; ++r) {
                    const float4 t = p4[r * d4 + k4];
                    pr[r] = make_float4(on ? t.x : 0.f, on ? t.y : 0.f, on ? t.z : 0.f, on ? t.w : 0.f);
                }
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int r = 0; r < PM_ROWS; ++r)
                        acc[u][r] = fmaf(x[u].w, pr[r].w, fmaf(x[u].z, pr[r].z, fmaf(x[u].y, pr[r].y, fmaf(x[u].x, pr[r].x, acc[u][r]))));
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
#pragma unroll
                for (int r = 0; r < PM_ROWS; ++r) {
                    float v = acc[u][r];
                    v += dpp_move<0xB1>(v);    // lane ^ 1
                    v += dpp_move<0x4E>(v);    // lane ^ 2
                    v += dpp_move<0x141>(v);   // the other quad of the 8
                    acc[u][r] = v;
                }
                const int j = j0 + u * 8 + g;
                if (q == 0 && j < M) G4[j] = make_float4(acc[u][0], acc[u][1], acc[u][2], acc[u][3]);
            }
        }
    }
    __syncthreads();

    // pass 1: m[r] = min over faces of T~ + (E + X)
    float m[PM_ROWS];
#pragma unroll
    for (int r = 0; r < PM_ROWS; ++r) m[r] = INFINITY;
    for (int f = tid; f < F; f += PM_THREADS) {
        const float4 r0 = rec0[f];
        const int ia = __float_as_int(r0.x);
        if (ia < 0) continue;
        const PmFace fc = pm_face(rec1[f], rec2[f], rec3[f]);
        const float4 ga = G4[ia], gb = G4[__float_as_int(r0.y)], gc = G4[__float_as_int(r0.z)];
        const float gav[4] = {ga.x, ga.y, ga.z, ga.w}, gbv[4] = {gb.x, gb.y, gb.z, gb.w}, gcv[4] = {gc.x, gc.y, gc.z, gc.w};
#pragma unroll
        for (int r = 0; r < PM_ROWS; ++r) {
            float T, mg;
            pm_screen(P[r], gav[r], gbv[r], gcv[r], fc, cE, cX, T, mg);
            const float hi = T + mg;
            m[r] = hi < m[r] ? hi : m[r];   // (a NaN never enters)
        }
    }
#pragma unroll
    for (int r = 0; r < PM_ROWS; ++r) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float other = __shfl_xor(m[r], o, 64);
            m[r] = other < m[r] ? other : m[r];
        }
        if (lane == 0) redf[wave * PM_ROWS + r] = m[r];
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < PM_ROWS; ++r) {
        float v = redf[r];
#pragma unroll
        for (int w = 1; w < PM_WAVES; ++w) {
            const float other = redf[w * PM_ROWS + r];
            v = other < v ? other : v;
        }
        m[r] = v;
    }

    // pass 2: the exact form of every face the screen cannot exclude; the row's smallest (v, face)
    unsigned long long best[PM_ROWS];
    float bw[PM_ROWS][3];
    unsigned evals = 0;
#pragma unroll
    for (int r = 0; r < PM_ROWS; ++r) best[r] = ~0ull, bw[r][0] = bw[r][1] = bw[r][2] = 0.f;
    for (int f = tid; f < F; f += PM_THREADS) {
        const float4 r0 = rec0[f];
        const int ia = __float_as_int(r0.x), ib = __float_as_int(r0.y), ic = __float_as_int(r0.z);
        if (ia < 0) continue;
        const float4 r2 = rec2[f], r3 = rec3[f];
        const PmFace fc = pm_face(rec1[f], r2, r3);
        const float4 ga = G4[ia], gb = G4[ib], gc = G4[ic];
        const float gav[4] = {ga.x, ga.y, ga.z, ga.w}, gbv[4] = {gb.x, gb.y, gb.z, gb.w}, gcv[4] = {gc.x, gc.y, gc.z, gc.w};
#pragma unroll
        for (int r = 0; r < PM_ROWS; ++r) {
            float T, mg;
            pm_screen(P[r], gav[r], gbv[r], gcv[r], fc, cE, cX, T, mg);
            if (row0 + r < N && !(T - mg > m[r])) {
                float w0, w1, w2;
                float v = pm_exact(p4 + r * d4, (const float4 *)(f2b + (size_t)ia * d), (const float4 *)(f2b + (size_t)ib * d),
                                   (const float4 *)(f2b + (size_t)ic * d), d4, r2.x, r2.y, r2.z, r2.w, r3.z, r3.x > 0.f, w0, w1, w2);
                v = (v != v) ? INFINITY : v;   // a NaN never wins
                const unsigned long long key = ((unsigned long long)__float_as_uint(v) << 32) | (unsigned)f;
                if (key < best[r]) best[r] = key, bw[r][0] = w0, bw[r][1] = w1, bw[r][2] = w2;
                ++evals;
            }
        }
    }
#pragma unroll
    for (int r = 0; r < PM_ROWS; ++r) {
        const unsigned long long k = pm_wave_min(best[r]);
        if (lane == 0) redk[wave * PM_ROWS + r] = k;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < PM_ROWS; ++r) {
        unsigned long long k = redk[r];
#pragma unroll
        for (int w = 1; w < PM_WAVES; ++w) {
            const unsigned long long other = redk[w * PM_ROWS + r];
            k = other < k ? other : k;
        }
        const int row = row0 + r;
        if (row >= N) continue;
        const size_t o = (size_t)b * N + row;
        if (k == ~0ull) {   // no admissible face
            if (tid == 0) {
                face[o] = -1;
                bary[3 * o] = bary[3 * o + 1] = bary[3 * o + 2] = 0.f;
                pi_idx[3 * o] = pi_idx[3 * o + 1] = pi_idx[3 * o + 2] = 0;
                if (dist) dist[o] = INFINITY;
            }
        } else if (best[r] == k) {   // one thread: the face index is part of the key
            const int f = (int)(unsigned)(k & 0xffffffffu);
            const float v = __uint_as_float((unsigned)(k >> 32));
            const float4 r0 = rec0[f];
            const bool fin = v < INFINITY;
            face[o] = f;
            bary[3 * o] = fin ? bw[r][0] : 1.f, bary[3 * o + 1] = fin ? bw[r][1] : 0.f, bary[3 * o + 2] = fin ? bw[r][2] : 0.f;
            pi_idx[3 * o] = __float_as_int(r0.x), pi_idx[3 * o + 1] = __float_as_int(r0.y), pi_idx[3 * o + 2] = __float_as_int(r0.z);
            if (dist) dist[o] = sqrtf(v);
        }
    }
    // exact evaluations made (none for a row past N)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) evals += __shfl_xor(evals, o, 64);
    if (lane == 0 && evals) atomicAdd(cnt + 1, (unsigned long long)evals);
}

static size_t pm_lds_bytes(int M, int d) {
    return ((size_t)M + (size_t)PM_ROWS * (d / 4)) * sizeof(float4) + PM_WAVES * PM_ROWS * (sizeof(float) + sizeof(unsigned long long));
}

}  // namespace dvm

using namespace dvm;

static int precise_map_check(const char *who, int B, int N, int M, int d, int F) {
    DVM_REQUIRE(B >= 1 && B <= 65535 && N >= 1 && M >= 1 && F >= 1, "%s: bad sizes (B=%d N=%d M=%d F=%d; need all >= 1, B <= 65535)", who, B, N, M, F);
    DVM_REQUIRE(d >= 4 && d % 4 == 0 && d <= PM_MAX_D, "%s: d=%d unsupported (a multiple of 4, at most %d)", who, d, PM_MAX_D);
    DVM_REQUIRE(M <= PM_MAX_M, "%s: M=%d exceeds %d (dvm_precise_map_max_m)", who, M, PM_MAX_M);
    return DVM_OK;
}

DVM_EXPORT int dvm_precise_map_max_m(void) { return PM_MAX_M; }

DVM_EXPORT int dvm_precise_map_plan(int B, int N, int M, int d, int F, int *rows, int *threads, int *chunk, int *max_m) {
    DVM_REQUIRE(rows && threads && chunk && max_m, "dvm_precise_map_plan: null pointer");
    const int rc = precise_map_check("dvm_precise_map_plan", B, N, M, d, F);
    if (rc != DVM_OK) return rc;
    *rows = PM_ROWS, *threads = PM_THREADS, *chunk = PM_CHUNK, *max_m = PM_MAX_M;
    return DVM_OK;
}

DVM_EXPORT size_t dvm_precise_map_workspace_bytes(int B, int N, int M, int d, int F) {
    if (B < 1 || B > 65535 || N < 1 || M < 1 || F < 1 || M > PM_MAX_M || d < 4 || d % 4 || d > PM_MAX_D) return 0;
    return null_carve<PmWs>(carve_precise_map, B, F);
}

DVM_EXPORT int dvm_precise_map_f32(const float *f1, const float *f2, const int32_t *faces, int B, int N, int M, int d, int F, int32_t *face,
                                   float *bary, int32_t *pi_idx, float *dist, int64_t *stats, void *ws, size_t ws_bytes, void *stream) {
    DVM_REQUIRE(f1 && f2 && faces && face && bary && pi_idx, "dvm_precise_map_f32: null pointer");
    const int rc = precise_map_check("dvm_precise_map_f32", B, N, M, d, F);
    if (rc != DVM_OK) return rc;
    PmWs w;
    if (!carve_ws(ws, ws_bytes, "dvm_precise_map_f32", w, carve_precise_map, B, F)) return DVM_ENOSPACE;
    hipStream_t s = (hipStream_t)stream;
    unsigned long long *cnt = stats ? (unsigned long long *)stats : w.cnt;
    const hipError_t e = hipMemsetAsync(cnt, 0, 2 * sizeof(unsigned long long), s);
    if (e != hipSuccess) {
        set_error("dvm_precise_map_f32: zeroing the counters failed: %s", hipGetErrorString(e));
        return DVM_ELAUNCH;
    }
    hipLaunchKernelGGL(pm_record_kernel, dim3((F + 255) / 256, B), dim3(256), 0, s, f2, faces, M, d, F, w.rec, cnt);
    DVM_CHECK_LAUNCH("precise_map (face records)");
    const float cE = (40.f * (float)d + 1024.f) * PM_U, cX = 32.f * (float)(d + 2) * (float)(d + 2) * PM_U * PM_U;
    ensure_dyn_lds((const void *)pm_search_kernel, (int)pm_lds_bytes(PM_MAX_M, PM_MAX_D));
    hipLaunchKernelGGL(pm_search_kernel, dim3((N + PM_ROWS - 1) / PM_ROWS, B), dim3(PM_THREADS), pm_lds_bytes(M, d), s, f1, f2, w.rec, N, M, d, F,
                       cE, cX, face, bary, pi_idx, dist, cnt);
    DVM_CHECK_LAUNCH("precise_map (search)");
    return DVM_OK;
}
