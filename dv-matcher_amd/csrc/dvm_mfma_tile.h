// dvm_mfma_tile.h — the pieces every user of the 32x32 fp32-accumulator matrix tile shares, defined once: the vector types, the
// accumulator's register <-> row map, and the fp32 32x32x2 tile of a staged [32][W] block against a register fragment (the SA
// attention core, forward and backward).  Stateless __device__ __forceinline__ pieces only.  (The squared-distance tile of the
// soft-correspondence family, dvm_dist_tile.h, scales by -2, fixes D = 128 and streams 64-key tiles: its chain is its own.)
#pragma once

#include "dvm_common.h"

namespace dvm {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ f32x16 zero16() {
    return f32x16{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
}

// register r of lane-half h of a 32x32 accumulator <-> row of the tile (the lane's column is lane & 31)
__device__ __forceinline__ int lane_key(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// stage rows [j0, j0+32) of a [N][W] matrix into LDS with the even/odd channel split the A operand wants:
// position q < W/2 holds channel 2q, position W/2 + q holds channel 2q + 1
template <int W, int LD>
__device__ __forceinline__ void stage_rows(const float *__restrict__ src, int j0, int N, float *__restrict__ dst, int tid) {
    constexpr int V = W / 4;  // float4 per row
    for (int e = tid; e < 32 * V; e += 256) {
        const int r = e / V, c = e % V;
        f32x4 q = {0.f, 0.f, 0.f, 0.f};
        if (j0 + r < N) q = *(const f32x4 *)(src + (size_t)(j0 + r) * W + 4 * c);
        float2 ev = {q.x, q.z}, od = {q.y, q.w};
        *(float2 *)(dst + r * LD + 2 * c) = ev;
        *(float2 *)(dst + r * LD + W / 2 + 2 * c) = od;
    }
}

// B-operand fragment of one outer row: frag[s] = row[2s + h]
template <int W>
__device__ __forceinline__ void load_frag(const float *__restrict__ row, int h, float (&frag)[W / 2]) {
#pragma unroll
    for (int c = 0; c < W / 4; ++c) {
        f32x4 q = *(const f32x4 *)(row + 4 * c);
        frag[2 * c] = h ? q.y : q.x;
        frag[2 * c + 1] = h ? q.w : q.z;
    }
}

// C[j][i] = sum_c tile[j][c] * frag_i[c]   (A from the staged tile, B from registers)
template <int W, int LD>
__device__ __forceinline__ f32x16 tile_dot(const float *__restrict__ tile, int r32, int h, const float (&frag)[W / 2]) {
    const float *jr = tile + r32 * LD + h * (W / 2);
    f32x16 acc = zero16();
#pragma unroll
    for (int c = 0; c < W / 8; ++c) {
        f32x4 a = *(const f32x4 *)(jr + 4 * c);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, frag[4 * c], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, frag[4 * c + 1], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, frag[4 * c + 2], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, frag[4 * c + 3], acc, 0, 0, 0);
    }
    return acc;
}

}  // namespace dvm
