// dvm_mesh_geodesic.hip — geodesic distances on a triangle mesh by the first-order upwind ("fast-marching") update on
// triangles, relaxed to its fixed point: the surface metric's discretisation beside dvm_geodesic.hip's edge paths, which cannot
// cut across a triangle and overestimate by 5 - 8 % however fine the mesh.  The scheme is stated once, in float64 numpy, in
// tests/mesh_geodesic_ref.py; this file evaluates the same expressions in the same order (no contraction: -ffp-contract=off).
//
// Every requested source is an independent problem: one workgroup per source keeps the V tentative distances in LDS (fp64) and
// sweeps all corners (v; a, b) — vertex v, opposite edge a b — until a sweep accepts nothing.  As in graph_sssp_kernel, updates
// within a sweep are made in place: every value a thread can read is >= the fixed point and the update is order-preserving, so
// reading a neighbour's old or new value only changes how many sweeps are needed.  An update is accepted only if it lowers the
// value by the factor 1 - 2^-40 (or replaces +inf), so rounding cannot make the sweeps creep on for ever; two update orders
// differ by that margin's effect only.
//
// A vertex none of whose corner neighbours changed since it was last evaluated is skipped: its candidates are the ones it has taken
// or refused already, and values only ever fall, so it would refuse them again.  One dirty byte per vertex in LDS says so (see
// mesh_front_kernel); plain sweeps, which evaluate every corner in every sweep, are kept behind -DMG_DIRTY_SKIP=0 for the
// comparison in profiles/notes_mesh_geodesics.md.
//
// The geometry is computed once per call, not per sweep and per source: a prologue builds a corner table in the caller's
// workspace, CSR by vertex (count, scan, fill by integer atomics; the order of a vertex's corners is free, its update is a min).
#include "dvm_common.h"

namespace dvm {
namespace {

#ifndef MG_DIRTY_SKIP
#define MG_DIRTY_SKIP 1
#endif
constexpr int MG_THREADS = 256;
// dist[V] (fp64) and the V dirty bytes must fit the 152 KB of dynamic LDS graph_sssp_kernel requests as well: 16384 * 9 = 144 KB
constexpr int MG_MAX_V = 16384;
constexpr int MG_LDS_BYTES = 152 * 1024;
constexpr int MG_SCAN_THREADS = 1024;   // one workgroup scans the V + 1 counts, MG_MAX_V / MG_SCAN_THREADS per thread
constexpr int MG_ERR_FACE = 1, MG_ERR_SOURCE = 2, MG_ERR_SWEEPS = 4;   // bits of the device flag

// what a sweep needs of a corner (v; a, b): 48 bytes
struct Corner {
    int32_t a, b;
    double la, lb;          // |a - v|, |b - v|
    double q11, q12, q22;   // (X^T X)^-1, X = [a - v, b - v]; q11 < 0: degenerate, the corner has only its edge candidate
};

__device__ __forceinline__ bool face_ok(int i0, int i1, int i2, int V) {
    return (unsigned)i0 < (unsigned)V && (unsigned)i1 < (unsigned)V && (unsigned)i2 < (unsigned)V;
}

// count[v] += the corners at v; a face with an index outside [0, V) raises the flag and is left out (here and in the fill)
__global__ __launch_bounds__(MG_THREADS) void mesh_corner_count_kernel(const int32_t *__restrict__ faces, int V, int F, int32_t *__restrict__ count,
                                                                      int32_t *__restrict__ flag) {
    const int f = blockIdx.x * MG_THREADS + threadIdx.x;
    if (f >= F) return;
    const int i0 = faces[3 * (size_t)f], i1 = faces[3 * (size_t)f + 1], i2 = faces[3 * (size_t)f + 2];
    if (!face_ok(i0, i1, i2, V)) {
        atomicOr(flag, MG_ERR_FACE);
        return;
    }
    atomicAdd(&count[i0], 1);
    atomicAdd(&count[i1], 1);
    atomicAdd(&count[i2], 1);
}

// offs [V + 1] = exclusive scan of count [V] (one workgroup), cursor [V] = offs [V]
__global__ __launch_bounds__(MG_SCAN_THREADS) void mesh_corner_scan_kernel(const int32_t *__restrict__ count, int V, int32_t *__restrict__ offs,
                                                                          int32_t *__restrict__ cursor) {
    const int total = block_scan_counts<MG_SCAN_THREADS>(V, [&](int v) { return count[v]; }, [&](int v, int run) { offs[v] = cursor[v] = run; });
    if (threadIdx.x == 0) offs[V] = total;
}

__device__ __forceinline__ void corner_fill(const double *__restrict__ verts, int v, int a, int b, int32_t *__restrict__ cursor,
                                            Corner *__restrict__ table) {
    const double vx = verts[3 * (size_t)v], vy = verts[3 * (size_t)v + 1], vz = verts[3 * (size_t)v + 2];
    const double ax = verts[3 * (size_t)a] - vx, ay = verts[3 * (size_t)a + 1] - vy, az = verts[3 * (size_t)a + 2] - vz;
    const double bx = verts[3 * (size_t)b] - vx, by = verts[3 * (size_t)b + 1] - vy, bz = verts[3 * (size_t)b + 2] - vz;
    const double g11 = ax * ax + ay * ay + az * az;
    const double g12 = ax * bx + ay * by + az * bz;
    const double g22 = bx * bx + by * by + bz * bz;
    const double det = g11 * g22 - g12 * g12;
    const bool ok = det >= 2.2250738585072014e-308 && det < INFINITY;   // a normal positive number
    Corner c;
    c.a = a;
    c.b = b;
    c.la = sqrt(g11);
    c.lb = sqrt(g22);
    c.q11 = ok ? g22 / det : -1.0;
    c.q12 = ok ? -g12 / det : 0.0;
    c.q22 = ok ? g11 / det : 0.0;
    table[atomicAdd(&cursor[v], 1)] = c;   // the slot is inside v's row: cursor[v] started at offs[v] and the count kernel counted this corner
}

__global__ __launch_bounds__(MG_THREADS) void mesh_corner_fill_kernel(const double *__restrict__ verts, const int32_t *__restrict__ faces, int V,
                                                                     int F, int32_t *__restrict__ cursor, Corner *__restrict__ table) {
    const int f = blockIdx.x * MG_THREADS + threadIdx.x;
    if (f >= F) return;
    const int i0 = faces[3 * (size_t)f], i1 = faces[3 * (size_t)f + 1], i2 = faces[3 * (size_t)f + 2];
    if (!face_ok(i0, i1, i2, V)) return;
    corner_fill(verts, i0, i1, i2, cursor, table);
    corner_fill(verts, i1, i2, i0, cursor, table);
    corner_fill(verts, i2, i0, i1, cursor, table);
}

// the candidate of one corner for its neighbours' values da, db (tests/mesh_geodesic_ref.py::_candidates)
__device__ __forceinline__ double corner_candidate(const Corner &c, double da, double db) {
    const double ea = da + c.la, eb = db + c.lb;
    double cand = ea < eb ? ea : eb;
    if (c.q11 >= 0.0 && da < INFINITY && db < INFINITY) {
        const double s1 = c.q11 + c.q12, s2 = c.q12 + c.q22;
        const double A = s1 + s2;
        const double bb = s1 * da + s2 * db;
        const double cc = c.q11 * da * da + 2.0 * c.q12 * da * db + c.q22 * db * db - 1.0;
        const double disc = bb * bb - A * cc;
        if (disc >= 0.0) {
            const double front = (bb + sqrt(disc)) / A;
            const double ua = da - front, ub = db - front;
            const double n1 = c.q11 * ua + c.q12 * ub;
            const double n2 = c.q12 * ua + c.q22 * ub;
            if (n1 < 0.0 && n2 < 0.0 && front < cand) cand = front;   // upwind: the front enters through the edge a b
        }
    }
    return cand;
}

// one workgroup per requested source; D [gridDim.x][V]; sweeps [min(gridDim.x, V)]: the sweeps each of the first V sources took.
// dirty[v] != 0: a corner neighbour of v changed since v was last evaluated.  A thread clears its vertex's byte BEFORE it reads
// the neighbours' distances, and a thread that lowers dist[u] writes it BEFORE it sets the bytes of u's neighbours (workgroup
// fences keep both orders).  So whichever way the two interleave, v either reads the new dist[u] or is left dirty for the next
// sweep; and a sweep that accepts nothing sets no byte and has consumed every byte set before it: nothing is pending when the
// sweeps end.
__global__ __launch_bounds__(MG_THREADS) void mesh_front_kernel(const int32_t *__restrict__ offs, const Corner *__restrict__ table,
                                                               const int32_t *__restrict__ sources, int V, double *__restrict__ D,
                                                               int32_t *__restrict__ sweeps, int32_t *__restrict__ flag) {
    extern __shared__ __attribute__((aligned(16))) double dist[];   // [V]
    const int tid = threadIdx.x;
    const int src = sources ? sources[blockIdx.x] : (int)blockIdx.x;
    if ((unsigned)src >= (unsigned)V) {   // checked before it is used as an index; uniform over the workgroup
        if (tid == 0) atomicOr(flag, MG_ERR_SOURCE);
        return;
    }
    unsigned char *dirty = (unsigned char *)(dist + V);             // [V]
    for (int v = tid; v < V; v += MG_THREADS) {
        dist[v] = v == src ? 0.0 : INFINITY;
        dirty[v] = 1;
    }
    __syncthreads();
    const double margin = 1.0 - 0x1p-40;
    const int cap = 4 * V;
    int sweep = 0;
    for (;;) {
        int any = 0;
        for (int v = tid; v < V; v += MG_THREADS) {
#if MG_DIRTY_SKIP
            if (!__hip_atomic_load(&dirty[v], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) continue;
            __hip_atomic_store(&dirty[v], (unsigned char)0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
#endif
            const double dv = dist[v];
            double best = INFINITY;
            const int end = offs[v + 1];
            for (int c = offs[v]; c < end; ++c) {
                const Corner k = table[c];
                const double cand = corner_candidate(k, dist[k.a], dist[k.b]);
                best = cand < best ? cand : best;
            }
            if (dv == INFINITY ? best < INFINITY : best < dv * margin) {
                dist[v] = best;
                any = 1;
#if MG_DIRTY_SKIP
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                for (int c = offs[v]; c < end; ++c) {   // v's corner neighbours are the vertices whose corners read v
                    const int2 ab = *(const int2 *)&table[c];
                    __hip_atomic_store(&dirty[ab.x], (unsigned char)1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    __hip_atomic_store(&dirty[ab.y], (unsigned char)1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
#endif
            }
        }
        ++sweep;
        if (!__syncthreads_or(any)) break;   // also orders this sweep's writes before the next sweep and the write-out
        if (sweep >= cap) {
            if (tid == 0) atomicOr(flag, MG_ERR_SWEEPS);
            break;
        }
    }
    for (int v = tid; v < V; v += MG_THREADS) D[(size_t)blockIdx.x * V + v] = dist[v];
    if (tid == 0 && (int)blockIdx.x < V) sweeps[blockIdx.x] = sweep;
}

}  // namespace
}  // namespace dvm

using namespace dvm;

// the workspace: the flag word, the sweep counts (both read back by callers that want them: include/dvm.h), the CSR and its table
struct MeshGeoWs {
    int32_t *flag, *sweeps, *count, *offs, *cursor;
    Corner *table;
};
static size_t carve_mesh_geo(Arena &ar, int V, int F, MeshGeoWs &w) {
    w.flag = ar.take<int32_t>(1);
    w.sweeps = ar.take<int32_t>((size_t)V);
    w.count = ar.take<int32_t>((size_t)V);
    w.offs = ar.take<int32_t>((size_t)V + 1);
    w.cursor = ar.take<int32_t>((size_t)V);
    w.table = ar.take<Corner>(3 * (size_t)F);
    return ar.off;
}
static const char *mesh_geo_limits(int V, int F) {
    static thread_local char msg[160];
    const char *who = "dvm_mesh_geodesics_f64";
    if (V < 1 || F < 0) {
        snprintf(msg, sizeof msg, "%s: empty or negative sizes (V=%d F=%d)", who, V, F);
        return msg;
    }
    if (V > MG_MAX_V) {
        snprintf(msg, sizeof msg, "%s: V=%d exceeds the %d vertices whose distances fit in LDS", who, V, MG_MAX_V);
        return msg;
    }
    if (F > INT32_MAX / 3) {
        snprintf(msg, sizeof msg, "%s: F=%d exceeds the %d faces whose corners an int32 counts", who, F, INT32_MAX / 3);
        return msg;
    }
    return nullptr;
}

DVM_EXPORT int dvm_mesh_geodesics_max_v(void) { return MG_MAX_V; }

DVM_EXPORT size_t dvm_mesh_geodesics_workspace_bytes(int V, int F) {
    return mesh_geo_limits(V, F) ? 0 : null_carve<MeshGeoWs>(carve_mesh_geo, V, F);
}

DVM_EXPORT int dvm_mesh_geodesics_f64(const double *verts, const int32_t *faces, int V, int F, const int32_t *sources, int S, double *D, void *ws,
                                      size_t ws_bytes, void *stream) {
    const char *who = "dvm_mesh_geodesics_f64";
    DVM_REQUIRE(verts && D && (faces || F == 0), "%s: null pointer", who);
    const char *why = mesh_geo_limits(V, F);
    DVM_REQUIRE(!why, "%s", why);
    DVM_REQUIRE(!sources || S >= 1, "%s: S=%d sources in a list that was given (need S >= 1)", who, S);
    MeshGeoWs w;
    if (!carve_ws(ws, ws_bytes, who, w, carve_mesh_geo, V, F)) return DVM_ENOSPACE;
    hipStream_t s = (hipStream_t)stream;
    const int nsrc = sources ? S : V;
    // flag, sweeps and count lie back to back: one memset
    if (hipMemsetAsync(w.flag, 0, (size_t)((char *)w.offs - (char *)w.flag), s) != hipSuccess) {
        set_error("%s: hipMemsetAsync failed", who);
        return DVM_ELAUNCH;
    }
    if (F > 0) {
        const dim3 fgrid((F + MG_THREADS - 1) / MG_THREADS);
        hipLaunchKernelGGL(mesh_corner_count_kernel, fgrid, dim3(MG_THREADS), 0, s, faces, V, F, w.count, w.flag);
        hipLaunchKernelGGL(mesh_corner_scan_kernel, dim3(1), dim3(MG_SCAN_THREADS), 0, s, w.count, V, w.offs, w.cursor);
        hipLaunchKernelGGL(mesh_corner_fill_kernel, fgrid, dim3(MG_THREADS), 0, s, verts, faces, V, F, w.cursor, w.table);
    } else {
        hipLaunchKernelGGL(mesh_corner_scan_kernel, dim3(1), dim3(MG_SCAN_THREADS), 0, s, w.count, V, w.offs, w.cursor);
    }
    ensure_dyn_lds((const void *)mesh_front_kernel, MG_LDS_BYTES);
    hipLaunchKernelGGL(mesh_front_kernel, dim3(nsrc), dim3(MG_THREADS), (size_t)V * (sizeof(double) + 1), s, w.offs, w.table, sources, V, D, w.sweeps,
                       w.flag);
    DVM_CHECK_LAUNCH("mesh_geodesics");
    // the one synchronising step (include/dvm.h): the flag word alone is copied back and waited for
    int32_t flag = 0;
    if (hipMemcpyAsync(&flag, w.flag, sizeof flag, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) {
        set_error("%s: reading the error flag back failed: %s", who, hipGetErrorString(hipGetLastError()));
        return DVM_ELAUNCH;
    }
    DVM_REQUIRE(!(flag & MG_ERR_FACE), "%s: a face names a vertex outside [0, %d)", who, V);
    DVM_REQUIRE(!(flag & MG_ERR_SOURCE), "%s: a source index lies outside [0, %d)", who, V);
    if (flag & MG_ERR_SWEEPS) {
        set_error("%s: no fixed point within 4 V = %d sweeps", who, 4 * V);
        return DVM_ELAUNCH;
    }
    return DVM_OK;
}
