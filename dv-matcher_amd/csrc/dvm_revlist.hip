// dvm_revlist.hip — reversed index lists: for every target j of idx [B][E], the entries e that point at it.  Every backward that
// turns a scatter into a gather starts here (the N2P attention core, dvm_softcorr_apply_bwd_f32, the rank and cycle terms, the
// training criterion): a counting sort of idx — count per target, exclusive scan (= offs), fill — so that one wave per target
// sums its in-edges in registers, with one int atomic per entry instead of float atomics per channel.  Three routes (RevRoute,
// dvm_internal.h), all over the same record types and all with the same rule for a target outside [0, M): the entry is left out
// of count and fill alike.  The scans are block_scan_counts (dvm_common.h).
#include "dvm_common.h"

namespace dvm {
namespace {

// edges[pos] = e for the int32_t record; (e, source point) with e = point * K + slot for the int2 record (the point is stored,
// not derived: an integer division by the run-time K per edge was a fifth of the gather kernel's instructions)
__device__ __forceinline__ void put_edge(int32_t *dst, int e, int) { *dst = e; }
__device__ __forceinline__ void put_edge(int2 *dst, int e, int K) { *dst = make_int2(e, e / K); }
__device__ __forceinline__ bool in_range(int j, int M) { return (unsigned)j < (unsigned)M; }

// ---- the global route: three launches, global integer atomics
__global__ void rev_count_kernel(const int32_t *__restrict__ idx, long E, int M, int32_t *__restrict__ cnt) {
    const int b = blockIdx.y;
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    const int j = idx[(size_t)b * E + e];
    if (in_range(j, M)) atomicAdd(cnt + (size_t)b * (M + 1) + j, 1);
}

// exclusive scan of cnt[b][0..M) in place -> offs (cnt[b][M] = total); cursor = copy of the offsets
__global__ __launch_bounds__(1024) void rev_scan_kernel(int32_t *__restrict__ cnt, int M, int32_t *__restrict__ cursor) {
    int32_t *c = cnt + (size_t)blockIdx.x * (M + 1), *cur = cursor + (size_t)blockIdx.x * M;
    const int total = block_scan_counts<1024>(M, [&](int i) { return c[i]; }, [&](int i, int run) { c[i] = cur[i] = run; });
    if (threadIdx.x == 0) c[M] = total;
}

template <class Edge>
__global__ void rev_fill_kernel(const int32_t *__restrict__ idx, long E, int M, int K, int32_t *__restrict__ cursor, Edge *__restrict__ edges) {
    const int b = blockIdx.y;
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    const int j = idx[(size_t)b * E + e];
    if (!in_range(j, M)) return;
    const int pos = atomicAdd(cursor + (size_t)b * M + j, 1);
    put_edge(edges + (size_t)b * E + pos, (int)e, K);
}

// ---- the LDS route.  The three kernels above in one, for lists whose counters fit in LDS (2 M + 1 ints): ONE workgroup per
// cloud counts, scans and fills with LDS atomics — 8 workgroups instead of 3 launches of global atomics (35 + 5 + 46 us per layer
// at 8 x 2048 x 40); it runs beside the other stream's kernels, and the order inside a list carries no contract (the gather
// sums fp32 either way).
template <class Edge>
__global__ __launch_bounds__(1024) void rev_build_lds_kernel(const int32_t *__restrict__ idx, int E, int M, int K, int32_t *__restrict__ offs,
                                                             Edge *__restrict__ edges) {
    extern __shared__ int rev_lds[];          // cnt[M + 1] | cursor[M]
    int *cnt = rev_lds, *cursor = rev_lds + M + 1;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int32_t *ib = idx + (size_t)b * E;
    for (int i = tid; i <= M; i += 1024) cnt[i] = 0;
    __syncthreads();
    // (8 index loads in flight per thread: one workgroup per cloud has only its own 16 waves to cover the load latency)
    for (int e0 = tid; e0 < E; e0 += 8 * 1024) {
        int t[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) t[u] = e0 + u * 1024 < E ? ib[e0 + u * 1024] : -1;
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (in_range(t[u], M)) atomicAdd(&cnt[t[u]], 1);
    }
    __syncthreads();
    int32_t *ob = offs + (size_t)b * (M + 1);
    const int total = block_scan_counts<1024>(M, [&](int i) { return cnt[i]; }, [&](int i, int run) { cursor[i] = ob[i] = run; });
    if (tid == 0) ob[M] = total;
    __syncthreads();
    Edge *eb = edges + (size_t)b * E;
    for (int e0 = tid; e0 < E; e0 += 8 * 1024) {
        int t[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) t[u] = e0 + u * 1024 < E ? ib[e0 + u * 1024] : -1;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            if (!in_range(t[u], M)) continue;
            const int pos = atomicAdd(&cursor[t[u]], 1);
            put_edge(eb + pos, e0 + u * 1024, K);
        }
    }
}

// ---- the ordered route (deterministic mode, dvm_set_deterministic): the reversed lists in ASCENDING EDGE ORDER without atomics
// between threads.  The edges of a cloud are cut into REV_DET_CHUNKS contiguous chunks: (1) a histogram of targets per chunk (LDS
// counters, integer atomics inside one workgroup: order-free), (2) per target an exclusive scan over the chunks on top of the
// exclusive scan over the targets (= offs), (3) every chunk placed by ONE thread walking its edges in order from those bases.
__global__ __launch_bounds__(256) void rev_det_hist_kernel(const int32_t *__restrict__ idx, int E, int M, int32_t *__restrict__ hist) {
    extern __shared__ int rev_lds[];   // cnt[M]
    const int b = blockIdx.y, ch = blockIdx.x;
    const int per = (E + REV_DET_CHUNKS - 1) / REV_DET_CHUNKS, e0 = ch * per, e1 = min(E, e0 + per);
    for (int i = threadIdx.x; i < M; i += blockDim.x) rev_lds[i] = 0;
    __syncthreads();
    const int32_t *ib = idx + (size_t)b * E;
    for (int e = e0 + threadIdx.x; e < e1; e += blockDim.x) {
        const int j = ib[e];
        if (in_range(j, M)) atomicAdd(&rev_lds[j], 1);
    }
    __syncthreads();
    int32_t *h = hist + ((size_t)b * REV_DET_CHUNKS + ch) * M;
    for (int i = threadIdx.x; i < M; i += blockDim.x) h[i] = rev_lds[i];
}
// hist[b][ch][t] -> base position of chunk ch's first edge into target t; offs[b][0..M]
__global__ __launch_bounds__(1024) void rev_det_scan_kernel(int32_t *__restrict__ hist, int M, int32_t *__restrict__ offs) {
    int32_t *h = hist + (size_t)blockIdx.x * REV_DET_CHUNKS * M, *ob = offs + (size_t)blockIdx.x * (M + 1);
    const int total = block_scan_counts<1024>(
        M,
        [&](int t) {
            int s = 0;
            for (int ch = 0; ch < REV_DET_CHUNKS; ++ch) s += h[(size_t)ch * M + t];
            return s;
        },
        [&](int t, int run) {
            ob[t] = run;
            for (int ch = 0; ch < REV_DET_CHUNKS; ++ch) {
                const int v = h[(size_t)ch * M + t];
                h[(size_t)ch * M + t] = run;
                run += v;
            }
        });
    if (threadIdx.x == 0) ob[M] = total;
}
template <class Edge>
__global__ __launch_bounds__(256) void rev_det_fill_kernel(const int32_t *__restrict__ idx, int E, int M, int K, const int32_t *__restrict__ hist,
                                                           Edge *__restrict__ edges) {
    extern __shared__ int rev_lds[];   // cursor[M]
    const int b = blockIdx.y, ch = blockIdx.x;
    const int per = (E + REV_DET_CHUNKS - 1) / REV_DET_CHUNKS, e0 = ch * per, e1 = min(E, e0 + per);
    const int32_t *h = hist + ((size_t)b * REV_DET_CHUNKS + ch) * M;
    for (int i = threadIdx.x; i < M; i += blockDim.x) rev_lds[i] = h[i];
    __syncthreads();
    if (threadIdx.x != 0) return;
    const int32_t *ib = idx + (size_t)b * E;
    Edge *eb = edges + (size_t)b * E;
    for (int e = e0; e < e1; ++e) {
        const int j = ib[e];
        if (in_range(j, M)) put_edge(eb + rev_lds[j]++, e, K);
    }
}

}  // namespace

RevRoute rev_route(int B, long E, int M) {
    if (deterministic() && (size_t)M * sizeof(int) <= 96 * 1024) return REV_ORDERED;
    // (one workgroup per cloud: from 4 clouds on; fewer, larger clouds keep the chip busier with the three-kernel form)
    if (B >= 4 && (2 * (size_t)M + 1) * sizeof(int) <= 96 * 1024 && E < (1L << 31)) return REV_LDS;
    return REV_GLOBAL;
}

template <class Edge>
void launch_rev_lists(const int32_t *idx, int B, long E, int M, int K, const RevListsT<Edge> &r, RevRoute route, hipStream_t s) {
    if (route == REV_ORDERED) {
        const size_t lds = (size_t)M * sizeof(int);
        ensure_dyn_lds((const void *)rev_det_hist_kernel, (int)lds);
        ensure_dyn_lds((const void *)rev_det_fill_kernel<Edge>, (int)lds);
        hipLaunchKernelGGL(rev_det_hist_kernel, dim3(REV_DET_CHUNKS, B), dim3(256), lds, s, idx, (int)E, M, r.hist);
        hipLaunchKernelGGL(rev_det_scan_kernel, dim3(B), dim3(1024), 0, s, r.hist, M, r.offs);
        hipLaunchKernelGGL(rev_det_fill_kernel<Edge>, dim3(REV_DET_CHUNKS, B), dim3(256), lds, s, idx, (int)E, M, K, r.hist, r.edges);
    } else if (route == REV_LDS) {
        const size_t lds = (2 * (size_t)M + 1) * sizeof(int);
        ensure_dyn_lds((const void *)rev_build_lds_kernel<Edge>, (int)lds);
        hipLaunchKernelGGL(rev_build_lds_kernel<Edge>, dim3(B), dim3(1024), lds, s, idx, (int)E, M, K, r.offs, r.edges);
    } else {
        dim3 egrid((unsigned)((E + 255) / 256), B);
        (void)hipMemsetAsync(r.offs, 0, (size_t)B * (M + 1) * sizeof(int32_t), s);
        hipLaunchKernelGGL(rev_count_kernel, egrid, dim3(256), 0, s, idx, E, M, r.offs);
        hipLaunchKernelGGL(rev_scan_kernel, dim3(B), dim3(1024), 0, s, r.offs, M, r.cursor);
        hipLaunchKernelGGL(rev_fill_kernel<Edge>, egrid, dim3(256), 0, s, idx, E, M, K, r.cursor, r.edges);
    }
}
template void launch_rev_lists<int32_t>(const int32_t *, int, long, int, int, const RevListsT<int32_t> &, RevRoute, hipStream_t);
template void launch_rev_lists<int2>(const int32_t *, int, long, int, int, const RevListsT<int2> &, RevRoute, hipStream_t);

}  // namespace dvm
