// dvm_sa.hip — K5, the offset self-attention core of LG-Net's SA_Layer on the fp32 matrix instruction: symmetric energy, row
// softmax, column re-normalisation.  Reference: models/model.py:97-123 (SA_Layer).  The fp16-split kernels of the same two
// passes are in dvm_sa_f16.hip (inference), the backward in dvm_sa_bwd.hip.
// p [B][N][16] = Wqk x, v [B][N][64] = Wv x + bv (host GEMMs), point-major.  E_ij = p_i . p_j is symmetric.
//   pass 1: row statistics (m_i, l_i) of softmax_j(E_ij)
//   pass 2: for every column j:  x_r[j,:] = sum_i v_i w_ij / (1e-9 + sum_i w_ij),  w_ij = exp(E_ij - m_i)/l_i
#include "dvm_mfma_tile.h"

namespace dvm {

// Both passes: one workgroup owns 32 query rows / output columns; its 4 waves take the four 32-key tiles of every
// staged 128-key block and their partial results are merged through LDS at the end, so that B*N/32 workgroups
// (512 at B = 8, N = 2048) keep all 256 CUs busy where 128-row workgroups left half of them idle.
constexpr int SA_KB = 128;  // keys staged per iteration

// The next 128-key block of p travels in registers while the current one is consumed: rows [j0, j0 + 128) x 4 float4 of
// pb [N][16] into two registers per thread (zero past N) ...
__device__ __forceinline__ void sa_fetch_p(const float *pb, int j0, int N, int tid, f32x4 (&pre)[2]) {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        int e = tid + q * 256, r = e >> 2, c = e & 3;  // 128 rows x 4 float4
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (j0 + r < N) v = *(const f32x4 *)(pb + (size_t)(j0 + r) * SA_P + 4 * c);
        pre[q] = v;
    }
}
// ... and from them into pt [128][SA_LDP], with the even/odd channel split of stage_rows
__device__ __forceinline__ void sa_commit_p(float *pt, int tid, const f32x4 (&pre)[2]) {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        int e = tid + q * 256, r = e >> 2, c = e & 3;
        float2 ev = {pre[q].x, pre[q].z}, od = {pre[q].y, pre[q].w};
        *(float2 *)(pt + r * SA_LDP + 2 * c) = ev;
        *(float2 *)(pt + r * SA_LDP + 8 + 2 * c) = od;
    }
}

// grid.z = key chunks of `kchunk` keys (multiple of SA_KB).  With one chunk the kernels write the final results; with
// more (small B * N: B = 1, N = 4995 has only 157 column groups) they write per-chunk partials that two tiny merge
// kernels combine.
__global__ __launch_bounds__(256) void sa_rowstats_kernel(const float *__restrict__ p, int N, int kchunk, float *__restrict__ stats) {
    __shared__ __attribute__((aligned(16))) float pt[SA_KB * SA_LDP];
    __shared__ float red[4][32][2];
    const int b = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r32 = lane & 31, h = lane >> 5;
    const int irow = blockIdx.x * 32 + r32;
    const int irc = irow < N ? irow : N - 1;
    const float *pb = p + (size_t)b * N * SA_P;
    float pi[SA_P / 2];
    load_frag<SA_P>(pb + (size_t)irc * SA_P, h, pi);
    float m = -INFINITY, l = 0.f;
    const int zbeg = blockIdx.z * kchunk, zend = zbeg + kchunk < N ? zbeg + kchunk : N;
    const bool partial = gridDim.z > 1;
    f32x4 pre[2];
    auto fetch = [&](int j0) { sa_fetch_p(pb, j0, N, tid, pre); };
    fetch(zbeg);
    for (int j0 = zbeg; j0 < zend; j0 += SA_KB) {
        __syncthreads();
        sa_commit_p(pt, tid, pre);
        __syncthreads();
        if (j0 + SA_KB < zend) fetch(j0 + SA_KB);
        const int jt = j0 + wave * 32;
        if (jt >= N) continue;
        f32x16 acc = tile_dot<SA_P, SA_LDP>(pt + wave * 32 * SA_LDP, r32, h, pi);
        // this lane: row i = irow, 16 columns j = jt + lane_key(r, h)
        float tmax = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            int j = jt + lane_key(r, h);
            float e = j < N ? acc[r] : -INFINITY;
            acc[r] = e;
            tmax = fmaxf(tmax, e);
        }
        if (tmax > m) {
            l = l * __expf(m - tmax);  // m = -inf, l = 0 -> 0 * 0
            m = tmax;
        }
        if (tmax != -INFINITY) {
#pragma unroll
            for (int r = 0; r < 16; ++r) l += __expf(acc[r] - m);
        }
    }
    float mo = __shfl_xor(m, 32, 64), lo = __shfl_xor(l, 32, 64);
    float mm = fmaxf(m, mo);
    float ll = (m == -INFINITY ? 0.f : l * __expf(m - mm)) + (mo == -INFINITY ? 0.f : lo * __expf(mo - mm));
    if (h == 0) {
        red[wave][r32][0] = mm;
        red[wave][r32][1] = ll;
    }
    __syncthreads();
    if (tid < 32 && irow < N) {
        float gm = fmaxf(fmaxf(red[0][tid][0], red[1][tid][0]), fmaxf(red[2][tid][0], red[3][tid][0]));
        float gl = 0.f;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            float wm = red[w][tid][0];
            if (wm != -INFINITY) gl += red[w][tid][1] * __expf(wm - gm);
        }
        const size_t o = (((size_t)blockIdx.z * gridDim.y + b) * N + irow) * 2;  // chunk-major partials
        stats[o] = gm;
        stats[o + 1] = partial ? gl : 1.0f / gl;
    }
}

// (m, l) of S key chunks -> (m, 1 / l)
__global__ void sa_stats_merge_kernel(const float *__restrict__ part, long rows, int S, float *__restrict__ stats) {
    const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows) return;
    float gm = -INFINITY;
    for (int z = 0; z < S; ++z) gm = fmaxf(gm, part[((size_t)z * rows + r) * 2]);
    float gl = 0.f;
    for (int z = 0; z < S; ++z) {
        const float wm = part[((size_t)z * rows + r) * 2];
        if (wm != -INFINITY) gl += part[((size_t)z * rows + r) * 2 + 1] * __expf(wm - gm);
    }
    stats[r * 2] = gm;
    stats[r * 2 + 1] = 1.0f / gl;
}

// sum of S partial (unnormalised x_r, column sum) -> x_r, 1 / (1e-9 + column sum)
__global__ void sa_apply_merge_kernel(const float *__restrict__ po, const float *__restrict__ pc, long rows, int S,
                                      float *__restrict__ xr, float *__restrict__ cinv_out) {
    const long g = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= rows * SA_C) return;
    const long r = g / SA_C;
    float cs = 0.f, acc = 0.f;
    for (int z = 0; z < S; ++z) {
        cs += pc[(size_t)z * rows + r];
        acc += po[(size_t)z * rows * SA_C + g];
    }
    const float inv = 1.0f / (1e-9f + cs);
    xr[g] = acc * inv;
    if (cinv_out && (g % SA_C) == 0) cinv_out[r] = inv;
}

__global__ __launch_bounds__(256) void sa_apply_kernel(const float *__restrict__ p, const float *__restrict__ v,
                                                       const float *__restrict__ stats, int N, int kchunk, float *__restrict__ xr,
                                                       float *__restrict__ cinv_out /* partial mode: column sums */) {
    __shared__ __attribute__((aligned(16))) float pt[SA_KB * SA_LDP];
    __shared__ __attribute__((aligned(16))) float vt[SA_KB * SA_C];  // reused as the [wave][reg][lane] merge buffer
    __shared__ float st[SA_KB * 2];
    __shared__ float csum[4][32];
    const int b = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r32 = lane & 31, h = lane >> 5;
    const int jcol = blockIdx.x * 32 + r32;
    const int jc = jcol < N ? jcol : N - 1;
    const float *pb = p + (size_t)b * N * SA_P;
    const float *vb = v + (size_t)b * N * SA_C;
    float pj[SA_P / 2];
    load_frag<SA_P>(pb + (size_t)jc * SA_P, h, pj);
    f32x16 o0 = zero16(), o1 = o0;
    float colsum = 0.f;
    const int zbeg = blockIdx.z * kchunk, zend = zbeg + kchunk < N ? zbeg + kchunk : N;
    const bool partial = gridDim.z > 1;
    // the next 128-key block (p, v, stats) travels in registers while the current one is consumed
    f32x4 prep[2], prev[8];
    float pres;
    auto fetch = [&](int i0) {
        sa_fetch_p(pb, i0, N, tid, prep);
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            int e = tid + q * 256, r = e >> 4, c = e & 15;
            f32x4 t = {0.f, 0.f, 0.f, 0.f};
            if (i0 + r < N) t = *(const f32x4 *)(vb + (size_t)(i0 + r) * SA_C + 4 * c);
            prev[q] = t;
        }
        pres = (i0 + (tid >> 1) < N) ? stats[((size_t)b * N + i0 + (tid >> 1)) * 2 + (tid & 1)] : 0.f;  // invl = 0 kills padding
    };
    fetch(zbeg);
    for (int i0 = zbeg; i0 < zend; i0 += SA_KB) {
        __syncthreads();
        sa_commit_p(pt, tid, prep);
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            int e = tid + q * 256, r = e >> 4, c = e & 15;
            *(f32x4 *)(vt + r * SA_C + 4 * c) = prev[q];
        }
        st[tid] = pres;
        __syncthreads();
        if (i0 + SA_KB < zend) fetch(i0 + SA_KB);
        if (i0 + wave * 32 >= N) continue;
        // E tile: rows = this wave's 32 keys i (A operand from LDS), cols = this lane's column j
        const f32x16 acc = tile_dot<SA_P, SA_LDP>(pt + wave * 32 * SA_LDP, r32, h, pj);
        // w_r = exp(E - m_i) / l_i for the 16 key rows of this lane; then x_r += V^T w on the matrix cores:
        // MFMA step r pairs key rho_r (lanes h=0) with key rho_r+4 (lanes h=1) in both operands.
        const float *stw = st + wave * 64, *vtw = vt + wave * 32 * SA_C;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            int key = lane_key(r, h);
            float w = __expf(acc[r] - stw[key * 2]) * stw[key * 2 + 1];
            colsum += w;
            float va = vtw[key * SA_C + r32], vb2 = vtw[key * SA_C + 32 + r32];
            o0 = __builtin_amdgcn_mfma_f32_32x32x2f32(va, w, o0, 0, 0, 0);
            o1 = __builtin_amdgcn_mfma_f32_32x32x2f32(vb2, w, o1, 0, 0, 0);
        }
    }
    colsum += __shfl_xor(colsum, 32, 64);
    __syncthreads();  // every wave is done with vt
    if (h == 0) csum[wave][r32] = colsum;
    float *red = vt + wave * (32 * 64);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        red[r * 64 + lane] = o0[r];
        red[(16 + r) * 64 + lane] = o1[r];
    }
    __syncthreads();
    const float cs = (csum[0][r32] + csum[1][r32]) + (csum[2][r32] + csum[3][r32]);
    const float inv = partial ? 1.0f : 1.0f / (1e-9f + cs);
    const size_t orow = ((size_t)blockIdx.z * gridDim.y + b) * N + jcol;  // chunk-major partials (chunk 0 = the output itself)
    if (cinv_out && wave == 0 && h == 0 && jcol < N) cinv_out[orow] = partial ? cs : inv;
    if (jcol < N) {
        float *o = xr + orow * SA_C;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int r = wave * 8 + q;  // merged register index: 0..15 -> o0, 16..31 -> o1
            const float *src = vt + r * 64 + lane;
            float sum = (src[0] + src[32 * 64]) + (src[2 * 32 * 64] + src[3 * 32 * 64]);
            o[(r >> 4) * 32 + lane_key(r & 15, h)] = sum * inv;
        }
    }
}

// key chunks per column group: enough workgroups to fill the chip (B * N/32 alone: 157 at B = 1, N = 4995)
static int sa_splits(int B, int N) {
    const int groups = B * ((N + 31) / 32);
    if (groups >= 400) return 1;  // measured: at 512 groups (B = 8, N = 2048) the merge passes cost more than the split gains
    int S = 1;
    while (groups * S < 1024 && S < 8 && (N + 2 * S - 1) / (2 * S) >= 4 * SA_KB) S *= 2;
    return S;
}
static size_t sa_partial_floats(int B, int N) {
    const int S = sa_splits(B, N);
    return S > 1 ? (size_t)S * B * N * (2 + SA_C + 1) : 0;
}
// stats [B][N][2] and xr [B][N][64] (and cinv [B][N] when given) from p, v; `part` holds sa_partial_floats(B, N) floats,
// pp / vp the split planes (sa_f16_carve), or null
static void launch_sa_forward(const float *p, const float *v, int B, int N, float *xr, float *stats, float *cinv, float *part,
                              _Float16 *pp, _Float16 *vp, hipStream_t s) {
    const int S = sa_splits(B, N);
    const int kchunk = ((N + S - 1) / S + SA_KB - 1) / SA_KB * SA_KB;
    const int Z = (N + kchunk - 1) / kchunk;
    dim3 grid((N + 31) / 32, B, Z);
    const long rows = (long)B * N;
    float *pstats = part, *po = Z > 1 ? pstats + (size_t)Z * rows * 2 : nullptr, *pc = Z > 1 ? po + (size_t)Z * rows * SA_C : nullptr;
    const bool f16 = pp != nullptr;   // (a caller without the split planes' workspace — the training forward — keeps both contractions on the fp32 matrix instruction)
    if (f16) launch_sa_split_f16(p, v, B, N, pp, vp, s);
    // pass 1
    float *st1 = Z == 1 ? stats : pstats;
    if (f16)
        launch_sa_rowstats_f16(pp, B, N, kchunk, Z, st1, s);
    else
        hipLaunchKernelGGL(sa_rowstats_kernel, grid, dim3(256), 0, s, p, N, kchunk, st1);
    if (Z > 1) hipLaunchKernelGGL(sa_stats_merge_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s, pstats, rows, Z, stats);
    // pass 2
    float *xo = Z == 1 ? xr : po, *co = Z == 1 ? cinv : pc;
    if (f16)
        launch_sa_apply_f16(pp, vp, stats, B, N, kchunk, Z, xo, co, s);
    else
        hipLaunchKernelGGL(sa_apply_kernel, grid, dim3(256), 0, s, p, v, stats, N, kchunk, xo, co);
    if (Z > 1) hipLaunchKernelGGL(sa_apply_merge_kernel, dim3((unsigned)((rows * SA_C + 255) / 256)), dim3(256), 0, s, po, pc, rows, Z, xr, cinv);
}
struct SaWs {
    float *stats, *part;
    _Float16 *pp, *vp;
};
static size_t carve_sa(Arena &ar, int B, int N, SaWs &w) {
    w.stats = ar.take<float>((size_t)B * N * 2);
    w.part = ar.take<float>(sa_partial_floats(B, N));
    return sa_f16_carve(ar, B, N, w.pp, w.vp);
}
static size_t carve_sa_train(Arena &ar, int B, int N, float *&part) {   // the training forward: the partials alone
    part = ar.take<float>(sa_partial_floats(B, N));
    return ar.off;
}
}  // namespace dvm

using namespace dvm;

DVM_EXPORT size_t dvm_sa_attention_workspace_bytes(int B, int N) { return null_carve<SaWs>(carve_sa, B, N); }

DVM_EXPORT int dvm_sa_attention_fwd_f32(const float *p, const float *v, int B, int N, float *xr, void *ws, size_t ws_bytes,
                                        void *stream) {
    DVM_REQUIRE(p && v && xr && B >= 1 && N >= 1, "dvm_sa_attention_fwd_f32: bad arguments");
    SaWs w;
    if (!carve_ws(ws, ws_bytes, "dvm_sa_attention_fwd_f32", w, carve_sa, B, N)) return DVM_ENOSPACE;
    launch_sa_forward(p, v, B, N, xr, w.stats, nullptr, w.part, w.pp, w.vp, (hipStream_t)stream);
    DVM_CHECK_LAUNCH("sa_attention");
    return DVM_OK;
}

// The training forward stays on the fp32 matrix instruction: the backward kernels recompute E in fp32 and take the row
// statistics and column sums from here — with the fp16-split E (2.4e-7 * sum|p_i p_j| off) the two would disagree by
// up to 1e-4 relative in dp at large logits.  Inference (dvm_sa_attention_fwd_f32) has no such coupling.
DVM_EXPORT size_t dvm_sa_attention_train_fwd_workspace_bytes(int B, int N) { return null_carve<float *>(carve_sa_train, B, N); }

DVM_EXPORT int dvm_sa_attention_train_fwd_f32(const float *p, const float *v, int B, int N, float *xr, float *stats, float *cinv,
                                              void *ws, size_t ws_bytes, void *stream) {
    DVM_REQUIRE(p && v && xr && stats && cinv && B >= 1 && N >= 1, "dvm_sa_attention_train_fwd_f32: bad arguments");
    const size_t need = sa_partial_floats(B, N) * sizeof(float);
    DVM_REQUIRE(need == 0 || (ws != nullptr && ws_bytes >= need), "dvm_sa_attention_train_fwd_f32: workspace too small (%zu < %zu)",
                ws_bytes, need);
    launch_sa_forward(p, v, B, N, xr, stats, cinv, (float *)ws, nullptr, nullptr, (hipStream_t)stream);
    DVM_CHECK_LAUNCH("sa_attention_train_fwd");
    return DVM_OK;
}
