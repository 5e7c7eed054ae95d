// dvm_n2p.hip — K4, neighbour-to-point attention of LG-Net (N2PAttention[_DIM]) on gathered projections; the backward is in
// dvm_n2p_bwd.hip.  Reference: models/model.py:325-395.
// Layout: point-major [B][N][C] fp32 in HBM, so neighbour rows are contiguous 256/512-B gathers.
#include "dvm_common.h"

namespace dvm {

// q, kp, vp [B][N][C] (= Wq x, Wk x, Wv x), idx [B][N][K].  One wave per point:
//   e_hj = q_h . (kp_j - kp_i)_h / sqrt(D),  a = softmax_j,  out_h = sum_j a_hj (vp_j - vp_i)_h
template <int C>
__global__ __launch_bounds__(256) void n2p_attention_kernel(const float *__restrict__ q, const float *__restrict__ kp,
                                                            const float *__restrict__ vp, const int32_t *__restrict__ idx,
                                                            int N, int K, int heads, float *__restrict__ out) {
    constexpr int CPL = C / 64;  // channels per lane
    const int lane = threadIdx.x & 63;
    const long pt = (long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int b = blockIdx.y;
    if (pt >= N) return;
    const size_t base = (size_t)b * N;
    const int D = C / heads;                 // 16 or 32
    const int lanes_per_head = D / CPL;      // 16
    const float scale = sqrtf((float)D);
    float qv[CPL], ki[CPL], vi[CPL];
#pragma unroll
    for (int c = 0; c < CPL; ++c) {
        qv[c] = q[(base + pt) * C + lane * CPL + c];
        ki[c] = kp[(base + pt) * C + lane * CPL + c];
        vi[c] = vp[(base + pt) * C + lane * CPL + c];
    }
    const int32_t *nb = idx + (base + pt) * K;
    float m = -INFINITY, l = 0.f, acc[CPL];
#pragma unroll
    for (int c = 0; c < CPL; ++c) acc[c] = 0.f;
    for (int j = 0; j < K; ++j) {
        const size_t nrow = (base + nb[j]) * C + lane * CPL;
        float part = 0.f;
#pragma unroll
        for (int c = 0; c < CPL; ++c) part = fmaf(qv[c], kp[nrow + c] - ki[c], part);
        for (int o = 1; o < lanes_per_head; o <<= 1) part += __shfl_xor(part, o, 64);
        const float e = part / scale;
        const float mn = fmaxf(m, e);
        const float sc = __expf(m - mn);  // first neighbour: exp(-inf) = 0
        const float w = __expf(e - mn);
        l = l * sc + w;
#pragma unroll
        for (int c = 0; c < CPL; ++c) acc[c] = fmaf(w, vp[nrow + c] - vi[c], acc[c] * sc);
        m = mn;
    }
    const float inv = 1.0f / l;
#pragma unroll
    for (int c = 0; c < CPL; ++c) out[(base + pt) * C + lane * CPL + c] = acc[c] * inv;
}

}  // namespace dvm

using namespace dvm;

DVM_EXPORT int dvm_n2p_attention_fwd_f32(const float *q, const float *kp, const float *vp, const int32_t *idx, int B, int N,
                                         int C, int K, int heads, float *out, void *stream) {
    DVM_REQUIRE(q && kp && vp && idx && out, "dvm_n2p_attention_fwd_f32: null pointer");
    DVM_REQUIRE(B >= 1 && N >= 1, "dvm_n2p_attention_fwd_f32: empty input");
    DVM_REQUIRE((C == 64 || C == 128) && heads == 4, "dvm_n2p_attention_fwd_f32: C=%d heads=%d unsupported", C, heads);
    DVM_REQUIRE(K >= 1 && K <= 64, "dvm_n2p_attention_fwd_f32: K=%d unsupported (1..64)", K);
    dim3 grid((N + 3) / 4, B);
    hipStream_t s = (hipStream_t)stream;
    if (C == 64)
        hipLaunchKernelGGL(n2p_attention_kernel<64>, grid, dim3(256), 0, s, q, kp, vp, idx, N, K, heads, out);
    else
        hipLaunchKernelGGL(n2p_attention_kernel<128>, grid, dim3(256), 0, s, q, kp, vp, idx, N, K, heads, out);
    DVM_CHECK_LAUNCH("n2p_attention");
    return DVM_OK;
}
