// dvm_laplacian.hip — the weighted neighbour matrix of a source shape in CSR, the operator of the Dirichlet term
// (dvm_dirichlet.hip): dvm_mesh_laplacian_f32 (cotangent weights of a triangle mesh) and dvm_knn_laplacian_f32 (W + W^T of a
// neighbour list).  Per batch element rowptr [N + 1], col [Ecap], w [Ecap] (fp32), norm (the energy of the shape's own
// coordinates, closed form), stats [4] int32.  Entries are a multiset — duplicates of (i, j) are kept — and every entry (i, j, w)
// has its mirror (j, i, w).  The definitions are stated once, in float64 numpy, in tests/dirichlet_term_ref.py; this file
// evaluates the same expressions in the same order (no contraction: -ffp-contract=off).
//
// Both builders are one counting sort of a CANDIDATE list, E = Ecap directed entries per batch element in a fixed numbering:
//   mesh   e = 6 f + 2 c, 6 f + 2 c + 1: corner c of face f, at vertex v = face[c] with a = face[(c + 1) % 3], b = face[(c + 2) % 3]:
//          the entries (a, b, w) and (b, a, w) of the opposite edge, w = fp32(cot / 2), cot = (u . v) / |u x v|, u = a - v, v = b - v
//   list   e = 2 (i K + s), 2 (i K + s) + 1: slot s of point i, j = nbr[i, s]: the entries (i, j, w) and (j, i, w)
// A candidate that is left out has row -1.  THE CANONICAL ORDER of a row: ascending candidate number.  It comes from the ordered
// route of launch_rev_lists (dvm_revlist.hip: per-chunk histograms, a scan, every chunk placed by one thread walking its entries in
// order), so no atomic's arrival order can reach rowptr, col or w, and there is no sort.  Steps: candidates (one thread per face /
// per slot) -> launch_rev_lists(REV_ORDERED) with rowptr as its offsets -> col, w gathered through the sorted candidate numbers (the
// tail of col / w behind rowptr[N] is set to -1 / 0) -> per-row sums in row order (mass; the list operator's norm) -> norm.
// stats are integer atomics: a count does not depend on the order of its increments.
#include "dvm_frob.h"

namespace dvm {
namespace {

constexpr int LAP_THREADS = 256;
// the ordered route keeps one int per row in LDS (96 KB)
constexpr int LAP_MAX_N = 24576;
// stats [B][4]: candidates' owners with an index outside [0, N); with degenerate geometry (a face whose |u x v|^2 is 0 or not
// finite at a corner; in stretch mode a squared distance that is 0 or not finite); self entries (j == i, list only); entries kept
constexpr int LAP_ST_RANGE = 0, LAP_ST_DEGEN = 1, LAP_ST_SELF = 2, LAP_ST_KEPT = 3;

struct Vec3d {
    double x, y, z;
};
__device__ __forceinline__ Vec3d load3(const float *__restrict__ p, int i) {
    return Vec3d{(double)p[3 * (size_t)i], (double)p[3 * (size_t)i + 1], (double)p[3 * (size_t)i + 2]};
}
__device__ __forceinline__ Vec3d sub3(const Vec3d &a, const Vec3d &b) { return Vec3d{a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ double dot3(const Vec3d &a, const Vec3d &b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
// |u x v|^2
__device__ __forceinline__ double cross2(const Vec3d &u, const Vec3d &v) {
    const double cx = u.y * v.z - u.z * v.y, cy = u.z * v.x - u.x * v.z, cz = u.x * v.y - u.y * v.x;
    return (cx * cx + cy * cy) + cz * cz;
}

// one thread per (face, batch element): its six candidates and its area (0 for a face that is left out)
__global__ __launch_bounds__(LAP_THREADS) void mesh_lap_candidates_kernel(const float *__restrict__ verts, const int32_t *__restrict__ faces,
                                                                          int N, int F, int32_t *__restrict__ rowkey,
                                                                          int32_t *__restrict__ colkey, float *__restrict__ wkey,
                                                                          double *__restrict__ area, int32_t *__restrict__ stats) {
    const int f = blockIdx.x * LAP_THREADS + threadIdx.x, b = blockIdx.y;
    if (f >= F) return;
    const size_t base = (size_t)b * 6 * F + 6 * (size_t)f;
    const int id[3] = {faces[3 * (size_t)f], faces[3 * (size_t)f + 1], faces[3 * (size_t)f + 2]};
    int bad = -1;
    double cot[3] = {0.0, 0.0, 0.0}, ar = 0.0;
    if ((unsigned)id[0] >= (unsigned)N || (unsigned)id[1] >= (unsigned)N || (unsigned)id[2] >= (unsigned)N) {
        bad = LAP_ST_RANGE;   // checked before an index becomes an address
    } else {
        const float *vb = verts + (size_t)b * N * 3;
        const Vec3d P[3] = {load3(vb, id[0]), load3(vb, id[1]), load3(vb, id[2])};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const Vec3d u = sub3(P[(c + 1) % 3], P[c]), v = sub3(P[(c + 2) % 3], P[c]);
            const double c2 = cross2(u, v);
            if (!(c2 > 0.0 && c2 < INFINITY)) bad = LAP_ST_DEGEN;
            const double len = sqrt(c2);
            cot[c] = dot3(u, v) / len;
            if (c == 0) ar = 0.5 * len;
        }
    }
    if (bad >= 0) atomicAdd(&stats[4 * b + bad], 1);
    area[(size_t)b * F + f] = bad >= 0 ? 0.0 : ar;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int a = id[(c + 1) % 3], bb = id[(c + 2) % 3];
        const float w = bad >= 0 ? 0.f : (float)(0.5 * cot[c]);
        rowkey[base + 2 * c] = bad >= 0 ? -1 : a;
        colkey[base + 2 * c] = bad >= 0 ? -1 : bb;
        wkey[base + 2 * c] = w;
        rowkey[base + 2 * c + 1] = bad >= 0 ? -1 : bb;
        colkey[base + 2 * c + 1] = bad >= 0 ? -1 : a;
        wkey[base + 2 * c + 1] = w;
    }
}

// one thread per (slot of the list, batch element): its two candidates
__global__ __launch_bounds__(LAP_THREADS) void knn_lap_candidates_kernel(const float *__restrict__ xyz, const int32_t *__restrict__ nbr, int N,
                                                                         int K, int mode, int32_t *__restrict__ rowkey,
                                                                         int32_t *__restrict__ colkey, float *__restrict__ wkey,
                                                                         int32_t *__restrict__ stats) {
    const long t = (long)blockIdx.x * LAP_THREADS + threadIdx.x;
    const int b = blockIdx.y;
    if (t >= (long)N * K) return;
    const int i = (int)(t / K);
    const int j = nbr[(size_t)b * N * K + t];
    const size_t base = (size_t)b * 2 * N * K + 2 * (size_t)t;
    int bad = -1;
    float w = 1.f;
    if (j == i) {
        bad = LAP_ST_SELF;
    } else if ((unsigned)j >= (unsigned)N) {
        bad = LAP_ST_RANGE;
    } else if (mode == 0) {
        const float *xb = xyz + (size_t)b * N * 3;
        const Vec3d d = sub3(load3(xb, i), load3(xb, j));
        const double d2 = dot3(d, d);
        if (!(d2 > 0.0 && d2 < INFINITY)) bad = LAP_ST_DEGEN;
        w = (float)(1.0 / d2);
    }
    if (bad >= 0) atomicAdd(&stats[4 * b + bad], 1);
    rowkey[base] = bad >= 0 ? -1 : i;
    colkey[base] = bad >= 0 ? -1 : j;
    wkey[base] = bad >= 0 ? 0.f : w;
    rowkey[base + 1] = bad >= 0 ? -1 : j;
    colkey[base + 1] = bad >= 0 ? -1 : i;
    wkey[base + 1] = bad >= 0 ? 0.f : w;
}

// col [E], w [E] through the sorted candidate numbers; -1 / 0 behind the used length rowptr[N]
__global__ __launch_bounds__(LAP_THREADS) void lap_gather_kernel(const int32_t *__restrict__ rowptr, const int32_t *__restrict__ sorted,
                                                                 const int32_t *__restrict__ colkey, const float *__restrict__ wkey, int N, int E,
                                                                 int32_t *__restrict__ col, float *__restrict__ w, int32_t *__restrict__ stats) {
    const int p = blockIdx.x * LAP_THREADS + threadIdx.x, b = blockIdx.y;
    if (p >= E) return;
    const int used = rowptr[(size_t)b * (N + 1) + N];
    if (p == 0) stats[4 * b + LAP_ST_KEPT] = used;
    const size_t o = (size_t)b * E;
    const int e = p < used ? sorted[o + p] : 0;   // a candidate number, < E by construction of the lists
    col[o + p] = p < used ? colkey[o + e] : -1;
    w[o + p] = p < used ? wkey[o + e] : 0.f;
}

// mass[i] = the sum over the faces at vertex i, in row order, of area / 3: every kept face has exactly one even candidate
// 6 f + 2 c in the row of each of its vertices
__global__ __launch_bounds__(LAP_THREADS) void mesh_lap_mass_kernel(const int32_t *__restrict__ rowptr, const int32_t *__restrict__ sorted,
                                                                    const double *__restrict__ area, int N, int F, float *__restrict__ mass) {
    const int i = blockIdx.x * LAP_THREADS + threadIdx.x, b = blockIdx.y;
    if (i >= N) return;
    const int32_t *rp = rowptr + (size_t)b * (N + 1);
    const int32_t *sb = sorted + (size_t)b * 6 * F;
    const double *ab = area + (size_t)b * F;
    double m = 0.0;
    const int end = rp[i + 1];
    for (int p = rp[i]; p < end; ++p) {
        const int e = sb[p];
        if ((e & 1) == 0) m += ab[e / 6] / 3.0;
    }
    mass[(size_t)b * N + i] = (float)m;
}

// rowsum[i] = the sum over the row, in row order, of w |x_i - x_j|^2 (the list operator's norm in uniform mode)
__global__ __launch_bounds__(LAP_THREADS) void knn_lap_rowsum_kernel(const float *__restrict__ xyz, const int32_t *__restrict__ rowptr,
                                                                     const int32_t *__restrict__ col, const float *__restrict__ w, int N, int E,
                                                                     double *__restrict__ rowsum) {
    const int i = blockIdx.x * LAP_THREADS + threadIdx.x, b = blockIdx.y;
    if (i >= N) return;
    const int32_t *rp = rowptr + (size_t)b * (N + 1);
    const float *xb = xyz + (size_t)b * N * 3;
    const Vec3d xi = load3(xb, i);
    double s = 0.0;
    const int end = rp[i + 1];
    for (int p = rp[i]; p < end; ++p) {
        const Vec3d d = sub3(xi, load3(xb, col[(size_t)b * E + p]));   // a kept column lies in [0, N)
        s += (double)w[(size_t)b * E + p] * dot3(d, d);
    }
    rowsum[(size_t)b * N + i] = s;
}

// stretch mode: norm = half the number of kept entries
__global__ void knn_lap_count_norm_kernel(const int32_t *__restrict__ rowptr, int B, int N, float *__restrict__ norm) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B) norm[b] = (float)(rowptr[(size_t)b * (N + 1) + N] / 2);
}

}  // namespace
}  // namespace dvm

using namespace dvm;

struct LapWs {
    int32_t *rowkey, *colkey;
    float *wkey;
    double *sums;    // mesh: area [B][F]; list: rowsum [B][N]
    RevLists rev;    // offs is the caller's rowptr; edges = the candidate numbers grouped by row, ascending
};
static size_t carve_lap(Arena &ar, int B, int N, size_t E, size_t nsums, LapWs &w) {
    w.rowkey = ar.take<int32_t>(B * E);
    w.colkey = ar.take<int32_t>(B * E);
    w.wkey = ar.take<float>(B * E);
    w.sums = ar.take<double>((size_t)B * nsums);
    w.rev.cursor = nullptr;
    w.rev.edges = ar.take<int32_t>(B * E);
    w.rev.hist = ar.take<int32_t>((size_t)B * REV_DET_CHUNKS * N);
    return ar.off;
}
static const char *lap_limits(const char *who, int B, int N, long per_row_unit, const char *unit, long count) {
    FROB_LIMIT(B >= 1 && N >= 1 && count >= 1, "%s: empty input (B=%d N=%d %s=%ld)", who, B, N, unit, count);
    FROB_LIMIT(B <= 65535, "%s: B=%d unsupported (<= 65535)", who, B);
    FROB_LIMIT(N <= LAP_MAX_N, "%s: N=%d unsupported (the sort keeps one counter per row in LDS: N <= %d)", who, N, LAP_MAX_N);
    FROB_LIMIT(count <= (long)(INT32_MAX / 2) / per_row_unit, "%s: %s=%ld unsupported (the entries are counted in int32)", who, unit, count);
    return nullptr;
}
static const char *mesh_lap_limits(int B, int N, int F) { return lap_limits("dvm_mesh_laplacian_f32", B, N, 6, "F", F); }
static const char *knn_lap_limits(int B, int N, int K, int mode) {
    const char *who = "dvm_knn_laplacian_f32";
    FROB_LIMIT(K >= 1 && K <= 64, "%s: K=%d unsupported (1..64)", who, K);
    FROB_LIMIT(mode == 0 || mode == 1, "%s: bad mode %d (0 = stretch, 1 = uniform)", who, mode);
    return lap_limits(who, B, N, 2 * K, "N", N);
}

// the sort and the gather both builders share; E entries per batch element
static void lap_sort_gather(const LapWs &w, int B, int N, int E, int32_t *rowptr, int32_t *col, float *wout, int32_t *stats, hipStream_t s) {
    RevLists r = w.rev;
    r.offs = rowptr;
    launch_rev_lists(w.rowkey, B, (long)E, N, 1, r, REV_ORDERED, s);
    hipLaunchKernelGGL(lap_gather_kernel, dim3((E + LAP_THREADS - 1) / LAP_THREADS, B), dim3(LAP_THREADS), 0, s, rowptr, w.rev.edges, w.colkey,
                       w.wkey, N, E, col, wout, stats);
}

DVM_EXPORT size_t dvm_mesh_laplacian_workspace_bytes(int B, int N, int F) {
    return mesh_lap_limits(B, N, F) ? 0 : null_carve<LapWs>(carve_lap, B, N, 6 * (size_t)F, (size_t)F);
}

DVM_EXPORT int dvm_mesh_laplacian_f32(const float *verts, const int32_t *faces, int B, int N, int F, int32_t *rowptr, int32_t *col, float *w,
                                      float *norm, float *mass, int32_t *stats, void *ws, size_t ws_bytes, void *stream) {
    const char *who = "dvm_mesh_laplacian_f32";
    DVM_REQUIRE(verts && faces && rowptr && col && w && norm && mass && stats, "%s: null pointer", who);
    const char *why = mesh_lap_limits(B, N, F);
    DVM_REQUIRE(!why, "%s", why);
    LapWs k;
    if (!carve_ws(ws, ws_bytes, who, k, carve_lap, B, N, 6 * (size_t)F, (size_t)F)) return DVM_ENOSPACE;
    hipStream_t s = (hipStream_t)stream;
    const int E = 6 * F;
    if (hipMemsetAsync(stats, 0, (size_t)B * 4 * sizeof(int32_t), s) != hipSuccess) {
        set_error("%s: hipMemsetAsync failed", who);
        return DVM_ELAUNCH;
    }
    hipLaunchKernelGGL(mesh_lap_candidates_kernel, dim3((F + LAP_THREADS - 1) / LAP_THREADS, B), dim3(LAP_THREADS), 0, s, verts, faces, N, F,
                       k.rowkey, k.colkey, k.wkey, k.sums, stats);
    lap_sort_gather(k, B, N, E, rowptr, col, w, stats, s);
    hipLaunchKernelGGL(mesh_lap_mass_kernel, dim3((N + LAP_THREADS - 1) / LAP_THREADS, B), dim3(LAP_THREADS), 0, s, rowptr, k.rev.edges, k.sums, N,
                       F, mass);
    launch_reduce_partials(k.sums, B, F, 2.f, norm, 1, 0, s);   // norm = 2 x the total area
    DVM_CHECK_LAUNCH("mesh_laplacian");
    return DVM_OK;
}

DVM_EXPORT size_t dvm_knn_laplacian_workspace_bytes(int B, int N, int K, int mode) {
    return knn_lap_limits(B, N, K, mode) ? 0 : null_carve<LapWs>(carve_lap, B, N, 2 * (size_t)N * K, (size_t)N);
}

DVM_EXPORT int dvm_knn_laplacian_f32(const float *xyz, const int32_t *nbr, int B, int N, int K, int mode, int32_t *rowptr, int32_t *col,
                                     float *w, float *norm, int32_t *stats, void *ws, size_t ws_bytes, void *stream) {
    const char *who = "dvm_knn_laplacian_f32";
    DVM_REQUIRE(xyz && nbr && rowptr && col && w && norm && stats, "%s: null pointer", who);
    const char *why = knn_lap_limits(B, N, K, mode);
    DVM_REQUIRE(!why, "%s", why);
    LapWs k;
    if (!carve_ws(ws, ws_bytes, who, k, carve_lap, B, N, 2 * (size_t)N * K, (size_t)N)) return DVM_ENOSPACE;
    hipStream_t s = (hipStream_t)stream;
    const int E = 2 * N * K;
    if (hipMemsetAsync(stats, 0, (size_t)B * 4 * sizeof(int32_t), s) != hipSuccess) {
        set_error("%s: hipMemsetAsync failed", who);
        return DVM_ELAUNCH;
    }
    hipLaunchKernelGGL(knn_lap_candidates_kernel, dim3((unsigned)(((long)N * K + LAP_THREADS - 1) / LAP_THREADS), B), dim3(LAP_THREADS), 0, s, xyz,
                       nbr, N, K, mode, k.rowkey, k.colkey, k.wkey, stats);
    lap_sort_gather(k, B, N, E, rowptr, col, w, stats, s);
    if (mode == 0) {
        hipLaunchKernelGGL(knn_lap_count_norm_kernel, dim3((B + 255) / 256), dim3(256), 0, s, rowptr, B, N, norm);
    } else {
        hipLaunchKernelGGL(knn_lap_rowsum_kernel, dim3((N + LAP_THREADS - 1) / LAP_THREADS, B), dim3(LAP_THREADS), 0, s, xyz, rowptr, col, w, N, E,
                           k.sums);
        launch_reduce_partials(k.sums, B, N, 0.5f, norm, 1, 0, s);
    }
    DVM_CHECK_LAUNCH("knn_laplacian");
    return DVM_OK;
}
