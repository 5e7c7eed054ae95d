// dvm_dg_geod.hip — skinning and node rings of a deformation graph by a caller-supplied distance matrix.
//
// The reference's construct_graph_euclidean / construct_graph (lib/deformation_graph_point.py:186-198, 219-224) pick a vertex's
// influence nodes as the top-k of geod[nodes_idx].T: whatever matrix the caller passes decides the skinning.  Here that is one
// pass over the node rows of the matrix: vertex v and node position j meet at d(v, j) = dist[b, nodes_idx[b, j], v] (node rows,
// read along v), candidates are ordered by the key (d, j) — d as fp32 with NaN ranked as +inf and -0 == +0, the lower j first
// among equals — and the first 3 entries of that order are the influences, the first K entries for the vertex nodes_idx[i] the
// ring of node i.  The key is a total order, so no split of the node range can reach the result.
#include "dvm_common.h"

namespace dvm {

// A candidate as one 64-bit word, (order-preserving bits of d) << 32 | j: an unsigned compare is the key's order.
__device__ __forceinline__ unsigned long long geod_key(float d, int j) {
    d = (d != d) ? INFINITY : d + 0.f;   // NaN ranks as +inf; -0 + 0 = +0
    const unsigned u = __float_as_uint(d);
    const unsigned o = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ((unsigned long long)o << 32) | (unsigned)j;
}

// sorted insertion into a register list by compare / select (every index a compile-time constant: no scratch)
template <int L>
__device__ __forceinline__ void geod_insert(unsigned long long (&key)[L], unsigned long long k) {
    if (k < key[L - 1]) {
#pragma unroll
        for (int t = L - 1; t > 0; --t) {
            const unsigned long long up = key[t - 1];
            key[t] = (k < up) ? up : ((k < key[t]) ? k : key[t]);
        }
        key[0] = (k < key[0]) ? k : key[0];
    }
}

// Workgroup = one tile of DG_GEOD_TILE vertices (one lane each) x S waves; wave s walks the node positions
// [s * chunk, (s + 1) * chunk) — every load a 256-byte segment of one node row — and keeps its lane's L smallest keys in
// registers.  Waves 1 .. S-1 pass their lists through LDS to wave 0, which inserts them into its own (the same insertion, the
// same order).  Wave 0 writes the influences; the ring rows go through LDS to whichever node positions name a vertex of the tile
// (a vertex listed twice gets its row twice).
// LDS: max((S - 1) * L * 64 * 8, 64 * L * 4) bytes.
template <int L>
__global__ __launch_bounds__(DG_GEOD_TILE *DG_GEOD_MAX_SLICES) void dg_skin_geod_kernel(
    const float *__restrict__ dist, const int32_t *__restrict__ nodes_idx, int N, int Nn, int ring_k, int32_t *__restrict__ infl_idx,
    float *__restrict__ dists, int32_t *__restrict__ ring) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long geod_lds[];
    const int b = blockIdx.y, lane = threadIdx.x & (DG_GEOD_TILE - 1);
    const int s = __builtin_amdgcn_readfirstlane((int)threadIdx.x / DG_GEOD_TILE), S = (int)blockDim.x / DG_GEOD_TILE;
    const int v0 = blockIdx.x * DG_GEOD_TILE, v = v0 + lane;
    const int vr = v < N ? v : N - 1;   // lanes past the end read the last column and write nothing
    const float *__restrict__ D = dist + (size_t)b * N * N;
    const int32_t *__restrict__ nodes = nodes_idx + (size_t)b * Nn;
    unsigned long long key[L];
#pragma unroll
    for (int t = 0; t < L; ++t) key[t] = ~0ull;   // behind every candidate: a real j is below 2^31
    const int chunk = (Nn + S - 1) / S;
    const int j0 = s * chunk, j1 = min(Nn, j0 + chunk);
    int j = j0;
    for (; j + 4 <= j1; j += 4) {   // four independent row segments in flight
        float d[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int r = min(max(nodes[j + q], 0), N - 1);   // an entry outside [0, N) cannot leave the matrix
            d[q] = D[(size_t)r * N + vr];
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) geod_insert<L>(key, geod_key(d[q], j + q));
    }
    for (; j < j1; ++j) {
        const int r = min(max(nodes[j], 0), N - 1);
        geod_insert<L>(key, geod_key(D[(size_t)r * N + vr], j));
    }
    if (s > 0) {
#pragma unroll
        for (int t = 0; t < L; ++t) geod_lds[((size_t)(s - 1) * L + t) * DG_GEOD_TILE + lane] = key[t];
    }
    __syncthreads();
    if (s == 0) {
        for (int w = 0; w < S - 1; ++w)
#pragma unroll
            for (int t = 0; t < L; ++t) geod_insert<L>(key, geod_lds[((size_t)w * L + t) * DG_GEOD_TILE + lane]);
        if (v < N) {
            const size_t row = ((size_t)b * N + v) * 3;
#pragma unroll
            for (int t = 0; t < 3; ++t) {
                const int jt = min((int)((unsigned)key[t] & 0x7fffffffu), Nn - 1);   // (a list entry is a real position: Nn >= 3)
                const int r = min(max(nodes[jt], 0), N - 1);
                infl_idx[row + t] = jt;
                dists[row + t] = D[(size_t)r * N + v];   // the matrix entry itself: a NaN or a -0 stays what it was
            }
        }
    }
    if (ring_k > 0) {   // (uniform over the launch)
        int32_t *rl = (int32_t *)geod_lds;   // wave 0 has read the other waves' lists: the same LDS now takes its ring rows
        if (s == 0) {
#pragma unroll
            for (int t = 0; t < L; ++t) rl[lane * L + t] = (int)(unsigned)key[t];
        }
        __syncthreads();
        for (int i = threadIdx.x; i < Nn; i += blockDim.x) {
            const int u = nodes[i] - v0;
            if (u >= 0 && u < DG_GEOD_TILE && u + v0 < N) {
                int32_t *o = ring + ((size_t)b * Nn + i) * ring_k;
                for (int q = 0; q < ring_k; ++q) o[q] = rl[u * L + q];
            }
        }
    }
}

// weights = exp(-d^2 / float(2 sigma^2)) row-normalised — dg_weights_kernel's expressions in its order (dvm_graph.hip) — for
// distances that may be infinite: an infinite (or NaN) d weighs 0, a row whose sum is 0 or not finite becomes (1, 0, 0)
__global__ __launch_bounds__(256) void dg_skin_weights_kernel(const float *__restrict__ dists, const double *__restrict__ sigma, int N,
                                                              float *__restrict__ weights) {
    const int b = blockIdx.y;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const double sg = sigma[b];
    const float den = (float)(2.0 * sg * sg);
    const size_t row = ((size_t)b * N + i) * 3;
    float w[3], tot = 0.f;
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        const float dv = dists[row + t];
        const float e = expf(-((dv * dv) / den));
        w[t] = (fabsf(dv) < INFINITY) ? e : 0.f;   // (false for a NaN as well)
        tot = tot + w[t];
    }
    const bool ok = tot > 0.f && tot < INFINITY;   // (false for a NaN sum: sigma == 0 at d == 0, a NaN sigma)
#pragma unroll
    for (int t = 0; t < 3; ++t) weights[row + t] = ok ? w[t] / tot : (t == 0 ? 1.f : 0.f);
}

static int dg_skin_geod_list(int ring_k) { return ring_k <= 3 ? 3 : ring_k <= 9 ? 9 : DG_GEOD_MAX_RING; }

// waves per vertex tile: the fewest (a power of two up to DG_GEOD_MAX_SLICES) that put DG_GEOD_TARGET_WAVES waves on the
// chip, each with at least DG_GEOD_MIN_SLICE node rows
static int dg_skin_geod_slices(int B, int N, int Nn) {
    const long tiles = (long)B * ((N + DG_GEOD_TILE - 1) / DG_GEOD_TILE);
    int S = 1;
    while (S < DG_GEOD_MAX_SLICES && tiles * S < DG_GEOD_TARGET_WAVES && Nn >= 2 * S * DG_GEOD_MIN_SLICE) S *= 2;
    return S;
}

template <int L>
static void launch_skin_t(const float *dist, const int32_t *nodes_idx, int B, int N, int Nn, int ring_k, int S, int32_t *infl_idx, float *dists,
                          int32_t *ring, hipStream_t s) {
    size_t lds = (size_t)(S - 1) * L * DG_GEOD_TILE * sizeof(unsigned long long);
    const size_t rl = ring_k > 0 ? (size_t)DG_GEOD_TILE * L * sizeof(int32_t) : 0;
    lds = lds > rl ? lds : rl;
    ensure_dyn_lds((const void *)dg_skin_geod_kernel<L>, (DG_GEOD_MAX_SLICES - 1) * L * DG_GEOD_TILE * (int)sizeof(unsigned long long));
    hipLaunchKernelGGL((dg_skin_geod_kernel<L>), dim3((N + DG_GEOD_TILE - 1) / DG_GEOD_TILE, B), dim3(DG_GEOD_TILE * S), lds, s, dist, nodes_idx,
                       N, Nn, ring_k, infl_idx, dists, ring);
}

void launch_dg_skin_geod(const float *dist, const int32_t *nodes_idx, int B, int N, int Nn, int ring_k, int32_t *infl_idx, float *dists,
                         int32_t *ring, hipStream_t s, int slices) {
    const int S = slices > 0 ? slices : dg_skin_geod_slices(B, N, Nn);
    switch (dg_skin_geod_list(ring_k)) {
    case 3: launch_skin_t<3>(dist, nodes_idx, B, N, Nn, ring_k, S, infl_idx, dists, ring, s); break;
    case 9: launch_skin_t<9>(dist, nodes_idx, B, N, Nn, ring_k, S, infl_idx, dists, ring, s); break;
    default: launch_skin_t<DG_GEOD_MAX_RING>(dist, nodes_idx, B, N, Nn, ring_k, S, infl_idx, dists, ring, s); break;
    }
}

void launch_dg_skin_weights(const float *dists, const double *sigma, int B, int N, float *weights, hipStream_t s) {
    hipLaunchKernelGGL(dg_skin_weights_kernel, dim3((N + 255) / 256, B), dim3(256), 0, s, dists, sigma, N, weights);
}

}  // namespace dvm

using namespace dvm;

static int skin_geod_check(const char *who, bool ptrs, int B, int N, int Nn, int ring_k) {
    DVM_REQUIRE(ptrs, "%s: null pointer", who);
    DVM_REQUIRE(B >= 1 && B <= 65535 && N >= 3 && Nn >= 3 && Nn <= N, "%s: bad sizes (B=%d N=%d Nn=%d; need 3 <= Nn <= N, B <= 65535)", who, B, N, Nn);
    DVM_REQUIRE(ring_k >= 0 && ring_k <= DG_GEOD_MAX_RING && ring_k <= Nn, "%s: ring_k=%d unsupported (0..%d, at most Nn=%d)", who, ring_k,
                DG_GEOD_MAX_RING, Nn);
    return DVM_OK;
}

DVM_EXPORT int dvm_dg_skin_geod_f32(const float *dist, const int32_t *nodes_idx, int B, int N, int Nn, int ring_k, int32_t *infl_idx,
                                    float *dists, int32_t *ring, void *stream) {
    const int rc = skin_geod_check("dvm_dg_skin_geod_f32", dist && nodes_idx && infl_idx && dists && (ring || ring_k == 0), B, N, Nn, ring_k);
    if (rc != DVM_OK) return rc;
    launch_dg_skin_geod(dist, nodes_idx, B, N, Nn, ring_k, infl_idx, dists, ring, (hipStream_t)stream);
    DVM_CHECK_LAUNCH("dg_skin_geod");
    return DVM_OK;
}

DVM_EXPORT int dvm_dg_skin_geod_slices_f32(const float *dist, const int32_t *nodes_idx, int B, int N, int Nn, int ring_k, int slices,
                                           int32_t *infl_idx, float *dists, int32_t *ring, void *stream) {
    const int rc = skin_geod_check("dvm_dg_skin_geod_slices_f32", dist && nodes_idx && infl_idx && dists && (ring || ring_k == 0), B, N, Nn, ring_k);
    if (rc != DVM_OK) return rc;
    DVM_REQUIRE(slices >= 1 && slices <= DG_GEOD_MAX_SLICES, "dvm_dg_skin_geod_slices_f32: slices=%d unsupported (1..%d)", slices,
                DG_GEOD_MAX_SLICES);
    launch_dg_skin_geod(dist, nodes_idx, B, N, Nn, ring_k, infl_idx, dists, ring, (hipStream_t)stream, slices);
    DVM_CHECK_LAUNCH("dg_skin_geod_slices");
    return DVM_OK;
}

DVM_EXPORT int dvm_dg_skin_geod_plan(int B, int N, int Nn, int ring_k, int *tile, int *slices, int *list) {
    DVM_REQUIRE(tile && slices && list, "dvm_dg_skin_geod_plan: null pointer");
    const int rc = skin_geod_check("dvm_dg_skin_geod_plan", true, B, N, Nn, ring_k);
    if (rc != DVM_OK) return rc;
    *tile = DG_GEOD_TILE, *slices = dg_skin_geod_slices(B, N, Nn), *list = dg_skin_geod_list(ring_k);
    return DVM_OK;
}

DVM_EXPORT int dvm_dg_skin_weights_f32(const float *dists, const double *sigma, int B, int N, float *weights, void *stream) {
    DVM_REQUIRE(dists && sigma && weights, "dvm_dg_skin_weights_f32: null pointer");
    DVM_REQUIRE(B >= 1 && B <= 65535 && N >= 1, "dvm_dg_skin_weights_f32: bad sizes (B=%d N=%d)", B, N);
    launch_dg_skin_weights(dists, sigma, B, N, weights, (hipStream_t)stream);
    DVM_CHECK_LAUNCH("dg_skin_weights");
    return DVM_OK;
}
