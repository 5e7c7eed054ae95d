// dvm_softcorr_f16.hip — the soft-correspondence kernel (K1) on the 16-bit matrix cores, exact results.
//
// gfx950's fp32 MFMA runs at the vector rate on the vector ALUs; the 16-bit MFMA is a separate
// pipe and 16x faster.  The N x M distance sweep is done on an exact 2-way fp16 split of the (power-of-two
// scaled) features, x s = h + m + r with |r| <= 2^-22 |x s|: the three partial products hh + hm + mh with fp32
// accumulation reproduce the dot product to 2^-22 relative per term — the accuracy class of the fp32 chain —
// at 3/16 of its matrix time, with the LDS traffic and register footprint of the fp32 kernel ("pass A").
// (A 3-way bf16 split needs six products and, worse, 96 VGPRs of query fragments and 1.5x the LDS reads.)
// Pass A keeps, per row, the 12 best columns by approximate squared distance and the softmax sum over all
// OTHER columns.  "Pass B" re-evaluates those 12 with the reference's own arithmetic (the k-ordered fp32 fma
// chain, correctly rounded sqrt: bit-identical to the fp32-MFMA kernel and the oracle), ranks them by
// (distance, column), adds their exact softmax terms and writes the top-10.  A row is certified when its
// exact 10th distance lies below the approximate 12th by more than the error bound of pass A; the few rows
// that are not (ties, duplicates, near-degenerate clouds) are recomputed exactly by a third kernel.
// Integer outputs (top-k columns, arg-max map) are thus bit-exact by construction, not by luck.
// (reference: models/loss.py:110-114, 1339-1347, 1404-1407)
#include <stdlib.h>
#include <type_traits>

#include "dvm_softcorr_f16.h"

namespace dvm {
namespace {

using namespace k1;

// ---------------------------------------------------------------- scale + split: fp32 rows -> fp16 planes
// largest |x| of a tensor as its bit pattern (non-negative floats order like integers)
__global__ __launch_bounds__(256) void absmax_kernel(const float *__restrict__ x, long n4, int *__restrict__ out) {
    float m = 0.f;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
        const f32x4 v = *(const f32x4 *)(x + 4 * i);
        m = fmaxf(fmaxf(m, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    if ((threadIdx.x & 63) == 0 && __float_as_int(m) > __atomic_load_n(out, __ATOMIC_RELAXED)) atomicMax(out, __float_as_int(m));
}

// Two scaled values -> their packed fp16 planes: h = rn16(a), m = rn16(a - h) (a - h is exact in fp32): the packed round-to-nearest
// conversion and one v_fma_mix per value (it reads the fp16 h directly).  Every kernel that writes planes goes through this, so the
// one-pass and the two-pass preparation leave the same bytes (checked against a host computation: tools/check_planes.py).
__device__ __forceinline__ void split2x2_f16(float a0, float a1, unsigned &h, unsigned &m) {
    asm("v_cvt_pk_f16_f32 %0, %1, %2" : "=v"(h) : "v"(a0), "v"(a1));
    asm("v_fma_mixlo_f16 %0, %1, 1.0, -%2 op_sel_hi:[0,0,1]" : "=v"(m) : "v"(a0), "v"(h));
    asm("v_fma_mixhi_f16 %0, %1, 1.0, -%2 op_sel:[0,0,1] op_sel_hi:[0,0,1]" : "+v"(m) : "v"(a1), "v"(h));
}
typedef unsigned u32x4_rs __attribute__((ext_vector_type(4)));
// 8 columns (two float4s) of a row, scaled by sc, to the row's planes at p (h) and p + 256 (m)
__device__ __forceinline__ void split8_store(const f32x4 &v0, const f32x4 &v1, float sc, char *p) {
    unsigned hh[4], mm[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float a0 = (e < 2 ? v0[2 * e] : v1[2 * e - 4]) * sc, a1 = (e < 2 ? v0[2 * e + 1] : v1[2 * e - 3]) * sc;   // exact
        split2x2_f16(a0, a1, hh[e], mm[e]);
    }
    const u32x4_rs h = {hh[0], hh[1], hh[2], hh[3]}, m = {mm[0], mm[1], mm[2], mm[3]};
    *(u32x4_rs *)(p) = h;
    *(u32x4_rs *)(p + 256) = m;
}

__global__ __launch_bounds__(256) void split_planes_kernel(const float *__restrict__ x, long rows, const int *__restrict__ maxbits,
                                                           char *__restrict__ planes) {
    const long g = (long)blockIdx.x * blockDim.x + threadIdx.x;  // eight columns per thread: two 16-byte loads, two 16-byte stores
    if (g >= rows * (HB_D / 8)) return;
    const float sc = pow2i(scale_exp(*maxbits));
    const long row = g / (HB_D / 8);
    const int c = (int)(g % (HB_D / 8));
    const f32x4 v0 = *(const f32x4 *)(x + row * HB_D + 8 * c), v1 = *(const f32x4 *)(x + row * HB_D + 8 * c + 4);
    split8_store(v0, v1, sc, planes + row * HB_ROWB + 16 * c);
}

// ---- the pair path's preparation in ONE pass over the features (instead of row norms + absmax, then the split: the 2 x 537 MB of
// the bench were read twice).  The split needs the tensor's absmax (its exponent fixes the scale) before the first element can
// be written, so the pass runs with a PROVISIONAL scale from a 1/64 sample of the rows; the true absmax comes out of the same
// pass, and only if its exponent differs from the sample's (spec[1]) are the planes written again by the gated split below -
// the result is the two-pass result either way.
__global__ __launch_bounds__(256) void sample_absmax_kernel(const float *__restrict__ x1, long rows1, const float *__restrict__ x2, long rows2,
                                                            int *__restrict__ spec) {
    float m = 0.f;
    const long n1 = (rows1 + 63) / 64 * 32, n2 = (rows2 + 63) / 64 * 32;   // float4s of every 64th row
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n1 + n2; i += (long)gridDim.x * blockDim.x) {
        const bool second = i >= n1;
        const long j = second ? i - n1 : i;
        const float *x = second ? x2 : x1;
        const f32x4 v = *(const f32x4 *)(x + (j / 32) * 64 * HB_D + 4 * (j % 32));
        m = fmaxf(fmaxf(m, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    if ((threadIdx.x & 63) == 0 && __float_as_int(m) > __atomic_load_n(spec, __ATOMIC_RELAXED)) atomicMax(spec, __float_as_int(m));
}

// Loads and stores: 16 lanes per row, 8 consecutive columns each (two 16-byte loads, two 16-byte stores); 16 rows per wave and trip.
// The row norm needs ATen's summation order (rownorm2_k128_kernel, dvm_softcorr.hip: lane l of 32 adds x_l^2, x_{l+32}^2, x_{l+64}^2,
// x_{l+96}^2 in that order, then ((s_j + s_{j+8}) + s_{j+16}) + s_{j+24}, then r_0 .. r_7 left to right), which is cheap with 32
// lanes per row and column l + 32 i in lane l - so the wave's 16 rows go through LDS once (rows 640 B apart: the two rows a wave
// reduces at a time then sit in different banks) and are reduced with that kernel's DPP / v_permlane16_swap steps: ~25 vector
// instructions per row pair.  (The same order on the 8-columns-per-lane layout costs 48 DPP additions per row and lane: built
// first, 355 us per launch.)
constexpr int RS_LROW = 160;          // floats between rows in LDS
struct RownormSplit {   // blockIdx.y = side (both feature sets in one launch: round 6)
    const float *x[2];
    long rows[2];
    float *nrm[2];
    int *slots[2];
    char *planes[2];
};
template <int RS_ROWS>   // rows per 16-lane group and trip (all requested before the first is used); 2 ships
__global__ __launch_bounds__(256) void rownorm_split_kernel(const RownormSplit a, const int *__restrict__ spec) {
    const float *__restrict__ x = a.x[blockIdx.y];
    const long rows = a.rows[blockIdx.y];
    if ((long)blockIdx.x * (16 * RS_ROWS) >= rows) return;   // (the grid spans the larger side)
    float *__restrict__ nrm = a.nrm[blockIdx.y];
    int *__restrict__ absmax_slots = a.slots[blockIdx.y];
    char *__restrict__ planes = a.planes[blockIdx.y];
    __shared__ __attribute__((aligned(16))) float xs_all[4][4 * RS_ROWS * RS_LROW];
    const int lane = threadIdx.x & 63, l16 = lane & 15, g4 = lane >> 4;
    float *xs = xs_all[threadIdx.x >> 6];
    const long wave_row0 = (((long)blockIdx.x * blockDim.x + threadIdx.x) >> 6) * (4 * RS_ROWS);   // this wave's 16 rows
    const float sc = pow2i(scale_exp(*spec));
    f32x4 v0[RS_ROWS], v1[RS_ROWS];
#pragma unroll
    for (int q = 0; q < RS_ROWS; ++q) {   // local row 4 q + g4
        const long row0 = wave_row0 + 4 * q + g4, row = row0 < rows ? row0 : rows - 1;
        const float *p = x + row * HB_D + 8 * l16;
        v0[q] = *(const f32x4 *)p, v1[q] = *(const f32x4 *)(p + 4);
    }
    float am = 0.f;
#pragma unroll
    for (int q = 0; q < RS_ROWS; ++q) {
        const long row0 = wave_row0 + 4 * q + g4;
        float *lp = xs + (4 * q + g4) * RS_LROW + 8 * l16;
        *(f32x4 *)lp = v0[q];
        *(f32x4 *)(lp + 4) = v1[q];
#pragma unroll
        for (int e = 0; e < 8; ++e) am = fmaxf(am, fabsf(e < 4 ? v0[q][e & 3] : v1[q][e & 3]));
        if (row0 < rows) split8_store(v0[q], v1[q], sc, planes + row0 * HB_ROWB + 16 * l16);
    }
    __builtin_amdgcn_s_waitcnt(0xc07f);   // lgkmcnt(0): the wave's rows are in LDS (one wave per region: no barrier)
    __builtin_amdgcn_wave_barrier();
    const int l32 = lane & 31, half = lane >> 5;
    float vv[2 * RS_ROWS][4];
#pragma unroll
    for (int pr = 0; pr < 2 * RS_ROWS; ++pr) {   // local rows 2 pr + half
        const float *lp = xs + (2 * pr + half) * RS_LROW + l32;
#pragma unroll
        for (int i = 0; i < 4; ++i) vv[pr][i] = lp[32 * i];
    }
#pragma unroll
    for (int pr = 0; pr < 2 * RS_ROWS; ++pr) {
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) s = s + vv[pr][i] * vv[pr][i];
        // lanes 8 k + l of a 32-lane half: k = 1 is 8 lanes up in the same 16-lane row, k = 2, 3 sit in the next row
        const unsigned su = __float_as_uint(s);
        const auto sw = __builtin_amdgcn_permlane16_swap(su, su, false, false);   // sw[1]: even rows <- the odd row above them
        const float up = __uint_as_float(sw[1]);
        const float ror_s = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(s), 0x128, 0xf, 0xf, false));
        const float ror_up = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(up), 0x128, 0xf, 0xf, false));
        const float r = ((s + ror_s) + up) + ror_up;  // valid in lanes l32 < 8 (k = 0)
        float u = r;   // u_j <- u_{j-1} + r_j seven times leaves (((r0 + r1) + r2) ... + r7) in lane 7 of the half
#pragma unroll
        for (int st = 0; st < 7; ++st) u = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(u), 0x111, 0xf, 0xf, false)) + r;
        const long row0 = wave_row0 + 2 * pr + half;
        if (l32 == 7 && row0 < rows) nrm[row0] = u;
    }
    int mb = __float_as_int(am);   // non-negative floats order like their bit patterns
    mb = max(mb, __builtin_amdgcn_update_dpp(0, mb, 0x111, 0xf, 0xf, false));  // row_shr:1
    mb = max(mb, __builtin_amdgcn_update_dpp(0, mb, 0x112, 0xf, 0xf, false));  // row_shr:2
    mb = max(mb, __builtin_amdgcn_update_dpp(0, mb, 0x114, 0xf, 0xf, false));  // row_shr:4
    mb = max(mb, __builtin_amdgcn_update_dpp(0, mb, 0x118, 0xf, 0xf, false));  // row_shr:8
    mb = max(mb, __builtin_amdgcn_update_dpp(0, mb, 0x142, 0xa, 0xf, false));  // row_bcast:15
    mb = max(mb, __builtin_amdgcn_update_dpp(0, mb, 0x143, 0xc, 0xf, false));  // row_bcast:31 -> lane 63 = the wave's max
    int *slot = absmax_slots + (blockIdx.x & 255);
    if (lane == 63 && mb > __atomic_load_n(slot, __ATOMIC_RELAXED)) atomicMax(slot, mb);
}
// slots -> the two absmax values, their common maximum (ONE scale for both sides), and whether the provisional scale was wrong
__global__ void spec_finalize_kernel(const int *__restrict__ slots, int *__restrict__ amax_pair, int *__restrict__ amax_common,
                                     int *__restrict__ spec) {
    int v = 0;
    for (int i = threadIdx.x & 63; i < 256; i += 64) v = max(v, slots[(threadIdx.x >> 6) * 256 + i]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
    __shared__ int two[2];
    if ((threadIdx.x & 63) == 0) two[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int c = max(two[0], two[1]);
        amax_pair[0] = two[0], amax_pair[1] = two[1];
        amax_common[0] = c, amax_common[1] = c;
        spec[1] = scale_exp(spec[0]) != scale_exp(c) ? 1 : 0;
    }
}
// (blockIdx.y = side: both feature sets in one launch)
struct SplitGated {
    const float *x[2];
    long rows[2];
    char *planes[2];
};
__global__ __launch_bounds__(256) void split_planes_gated_kernel(const SplitGated a, const int *__restrict__ maxbits2, const int *__restrict__ spec) {
    if (spec[1] == 0) return;   // (the usual case: the provisional scale was the right one)
    const float *__restrict__ x = a.x[blockIdx.y];
    const long rows = a.rows[blockIdx.y];
    char *__restrict__ planes = a.planes[blockIdx.y];
    const float sc = pow2i(scale_exp(maxbits2[blockIdx.y]));
    for (long g = (long)blockIdx.x * blockDim.x + threadIdx.x; g < rows * (HB_D / 8); g += (long)gridDim.x * blockDim.x) {
        const long row = g / (HB_D / 8);
        const int c = (int)(g % (HB_D / 8));
        const f32x4 v0 = *(const f32x4 *)(x + row * HB_D + 8 * c), v1 = *(const f32x4 *)(x + row * HB_D + 8 * c + 4);
        split8_store(v0, v1, sc, planes + row * HB_ROWB + 16 * c);
    }
}

// ---------------------------------------------------------------- pass A
// One workgroup's share of the sweep: logical block `block` of `nblocks` (the kernels below pass their hardware block number, or walk
// several blocks).  CHECK_ROUTE: return at once unless the block's (direction, pair) is routed to this form.
template <bool LEAN, bool CHECK_ROUTE = true>
__device__ __forceinline__ void sweep_f16_block(const HBArgs &args, int block, int nblocks, char *smem_b) {
    char *const ktile0 = smem_b;                                             // [2][HB_KT][512], 16-B chunks XOR-swizzled
    float *const knorm0 = (float *)(smem_b + (size_t)2 * HB_KT * HB_ROWB);   // [2][HB_KT]
    float *const stage = knorm0 + 2 * HB_KT + (threadIdx.x >> 6) * HB_STAGE + (threadIdx.x & 63);

    int lid = xcd_remap(block, nblocks);
    const int grp = lid >= args.blocks0 ? 1 : 0;
    lid -= grp ? args.blocks0 : 0;
    const HBGroup &G = args.g[grp];
    const int N = G.N, M = G.M;
    const int b = lid / G.tiles, qt = lid % G.tiles;
    if (CHECK_ROUTE && args.route && args.route[grp * args.nb + b] != (LEAN ? K1_ROUTE_LEAN : K1_ROUTE_FULL)) return;   // another kernel's pair
    const float neg_alpha = args.neg_alpha;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r32 = lane & 31, h = lane >> 5;

    const char *kbase = G.kp + (size_t)b * M * HB_ROWB;
    const float *knb = G.nk + (size_t)b * G.Mpad;
    const int qrow = qt * HB_QB + wave * 32 + r32;
    const int qrc = qrow < N ? qrow : N - 1;
    const char *qptr = G.qp + ((size_t)b * N + qrc) * HB_ROWB + 16 * h;
    f16x8 qh[8], qm[8];  // B-operand fragments: k = 16 s + 8 h + j
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        qh[s] = *(const f16x8 *)(qptr + 32 * s);
        qm[s] = *(const f16x8 *)(qptr + 256 + 32 * s);
    }
    const float na = G.nq[(size_t)b * N + qrc];
    const float cfac = -2.f * pow2i(-(scale_exp(*G.qmax) + scale_exp(*G.kmax)));  // -2 / (s_q s_k), exact

    PackedBest<HB_KC> kb;  // keyed on the approximate squared distance
    kb.init();
    float cref = -INFINITY, l = 0.f;
    float lim2 = INFINITY, cut2 = INFINITY;
    const float a2 = neg_alpha * LOG2E, cutw = args.cutw;

    const int ntiles = (M + HB_KT - 1) / HB_KT;
    // Key tiles go global -> LDS by LDS-DMA (no VGPRs, in flight for a whole iteration).  The DMA writes
    // lane-linearly (base + lane * 16), so rows are unpadded and the bank spread comes from an XOR swizzle of the
    // 16-B chunk index with the row number, applied to the per-lane SOURCE address here and to the reads below.
    auto stage_tile = [&](int t, int buf) {
        const int j0 = t * HB_KT;
        char *kt = ktile0 + (size_t)buf * HB_KT * HB_ROWB;
#pragma unroll
        for (int e = 0; e < HB_GLDS_PER_WAVE; ++e) {
            const int piece = wave * HB_GLDS_PER_WAVE + e;       // 2 rows
            const int r = 2 * piece + h;                          // lanes 0-31: first row, 32-63: second
            const int jr = j0 + r < M ? j0 + r : M - 1;           // padding keys re-read the last row (their norm is +inf)
            const char *src = kbase + (size_t)jr * HB_ROWB + ((r32 ^ (r & 31)) << 4);
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)src,
                                             (__attribute__((address_space(3))) void *)(kt + piece * 1024), 16, 0, 0);
        }
        if (wave == 0)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(knb + j0 + lane),
                                             (__attribute__((address_space(3))) void *)(knorm0 + buf * HB_KT), 4, 0, 0);
    };

    auto add_term = [&](float d2v) {  // l += exp(s - cref) for squared distance d2v (+inf: nothing)
        const bool live = d2v < INFINITY;
        const float s = __builtin_amdgcn_sqrtf(fmaxf(d2v, 0.f)) * neg_alpha;
        const float cnew = live ? fmaxf(cref, s) : cref;
        const float sc = (cnew == cref) ? 1.f : __builtin_amdgcn_exp2f((cref - cnew) * LOG2E);
        const float term = live ? __builtin_amdgcn_exp2f((s - cnew) * LOG2E) : 0.f;
        l = l * sc + term;
        cref = cnew;
    };

    auto subtile = [&](const char *kt, int sub, int buf, int jbase) {
        const char *arow = kt + (sub * 32 + r32) * HB_ROWB;
        const int t16 = (h ^ r32) << 4;  // chunk 2s + h of plane p sits at ((2s + 16p) ^ h ^ row) * 16
        f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        // all 16 A fragments of the sub-tile are requested up front (64 VGPRs, free during this phase)
        f16x8 ah[8], am[8];
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            ah[s] = *(const f16x8 *)(arow + ((32 * s) ^ t16));
            am[s] = *(const f16x8 *)(arow + ((32 * s) ^ t16 ^ 256));
        }
#pragma unroll
        for (int s = 0; s < 8; ++s) {  // (one accumulation chain of this instruction needs no interleaving)
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(am[s], qh[s], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[s], qm[s], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[s], qh[s], acc, 0, 0, 0);
        }
        // this lane's 16 keys: local key = (r&3) + 8*(r>>2) + 4*h
        const float *kn = knorm0 + buf * HB_KT + sub * 32 + 4 * h;
        unsigned mask = 0;
        if (LEAN) {
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                const f32x4 nb = *(const f32x4 *)(kn + 8 * g4);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int r = 4 * g4 + e;
                    const float v = fmaf(cfac, acc[r], na) + nb[e];
                    stage[r * 64] = v;
                    mask |= (v <= lim2) ? (1u << r) : 0u;
                }
            }
        } else {
            float df[16], tminf = INFINITY;
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                const f32x4 nb = *(const f32x4 *)(kn + 8 * g4);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int r = 4 * g4 + e;
                    const float v = fmaf(cfac, acc[r], na) + nb[e];
                    stage[r * 64] = v;
                    const bool fl = v <= lim2;
                    mask |= fl ? (1u << r) : 0u;
                    const float f = __builtin_amdgcn_sqrtf(fmaxf(v, 0.f));  // +inf for padding keys
                    df[r] = fl ? INFINITY : f;  // flagged ones are accounted for when they leave the list (below)
                    tminf = fminf(tminf, f);
                }
            }
            const float cnew = tminf * neg_alpha;
            if (cnew > cref) {
                l = l * exp2f((cref - cnew) * LOG2E);
                cref = cnew;
            }
            const float c2 = cref * LOG2E;
            float lsum = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) lsum += __builtin_amdgcn_exp2f(fmaf(df[r], a2, -c2));
            l += lsum;
        }
        // The softmax sum l covers every column EXCEPT the current members of the list: a column's term is added
        // when it leaves the list (or fails to enter it), so pass B can add the exact terms of the final
        // candidates without subtracting approximations of them.
        // (a counted loop with a wave-uniform trip count: the `while (__any(mask))` form makes the compiler copy the
        // whole list — 50 v_mov — around a structurised exit on every iteration)
        int iters = __popc(mask);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) iters = max(iters, __shfl_xor(iters, o, 64));
        iters = __builtin_amdgcn_readfirstlane(iters);
        for (int it = 0; it < iters; ++it) {
            const bool act = mask != 0;
            const int bpos = act ? (__ffs(mask) - 1) : 0;
            mask &= mask - 1;
            float v2 = stage[bpos * 64];
            v2 = act ? v2 : INFINITY;
            const double out = kb.insert(PackedBest<HB_KC>::pack(v2, jbase + (bpos & 3) + 8 * (bpos >> 2)));
            const float ok = PackedBest<HB_KC>::key_of(out);  // what is outside the list after this step
            if (LEAN) {
                // the lean sweep drops softmax terms beyond the cut (< e^-20 of the largest); an entry pushed out of the
                // list is nearly always beyond it — the whole wave skips the two exponentials unless one lane needs them
                const bool within = ok <= cut2;
                if (__builtin_amdgcn_ballot_w64(within) != 0) add_term(within ? ok : INFINITY);
            } else {
                add_term(ok);
            }
        }
        // bound for the next sub-tile: the row's KC-th best is at most min(a_K, b_K, max(a_m, b_m)), m = KC/2
        {
            const float wk = kb.key(HB_KC - 1), wm = kb.key(HB_KC / 2 - 1), w0 = kb.key(0);
            const float pk = __shfl_xor(wk, 32, 64), pm = __shfl_xor(wm, 32, 64);
            const float thr2 = fminf(fminf(wk, pk), fmaxf(wm, pm));
            if (LEAN) {
                const float dmin = __builtin_amdgcn_sqrtf(fmaxf(fminf(w0, __shfl_xor(w0, 32, 64)), 0.f));
                const float cut = dmin + cutw;  // beyond this the softmax term is < e^-20 of the largest
                cut2 = (cut * cut) * 1.000001f;
                lim2 = fmaxf(thr2, cut2);
            } else {
                lim2 = thr2;
            }
        }
    };

    stage_tile(0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // every wave waits for ITS pieces before the barrier (see dvm_softcorr_sweep2.hip)
    __syncthreads();
    for (int t = 0; t < ntiles; ++t) {
        const int buf = t & 1;
        const char *kt = ktile0 + (size_t)buf * HB_KT * HB_ROWB;
        if (t + 1 < ntiles) stage_tile(t + 1, buf ^ 1);  // the other buffer was last read before the previous barrier
        subtile(kt, 0, buf, t * HB_KT + 4 * h);
        subtile(kt, 1, buf, t * HB_KT + 32 + 4 * h);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }

    // merge the two half-lanes that share a query (lane, lane^32)
    {
        const float co = __shfl_xor(cref, 32, 64), lo = __shfl_xor(l, 32, 64);
        const float cm = fmaxf(cref, co);
        const float a = (cref == -INFINITY) ? 0.f : l * exp2f((cref - cm) * LOG2E);
        const float bb = (co == -INFINITY) ? 0.f : lo * exp2f((co - cm) * LOG2E);
        l = a + bb;
        cref = cm;
        double other[HB_KC];
#pragma unroll
        for (int t = 0; t < HB_KC; ++t)
            other[t] = __hiloint2double(__shfl_xor(__double2hiint(kb.e[t]), 32, 64), __shfl_xor(__double2loint(kb.e[t]), 32, 64));
#pragma unroll
        for (int t = 0; t < HB_KC; ++t) add_term(PackedBest<HB_KC>::key_of(kb.insert(other[t])));  // dropped from the union
    }
    if (h == 0 && qrow < N) {
        const size_t row = (size_t)b * N + qrow;
#pragma unroll
        for (int t = 0; t < HB_KC; ++t) {
            G.cidx[row * HB_KC + t] = PackedBest<HB_KC>::col_of(kb.e[t]);
            G.cd2[row * HB_KC + t] = kb.key(t);
        }
        G.lsum[row * 2] = l;
        G.lsum[row * 2 + 1] = cref;
    }
}
template <bool LEAN>
__global__ __launch_bounds__(HB_THREADS, 2) void softcorr_sweep_f16_kernel(const HBArgs args) {
    extern __shared__ __attribute__((aligned(16))) char smem_b[];
    sweep_f16_block<LEAN>(args, blockIdx.x, gridDim.x, smem_b);
}
// Routed first pass (round 6): ONE launch for the lean and the full first form — a workgroup takes the form its (direction, pair) is
// routed to, and returns at once if that is the coarse screen's.  (As two launches, each form cost its whole grid of returning
// workgroups — two per compute unit at a time, they need the form's LDS — in the feature half's dependent chain.)
__global__ __launch_bounds__(HB_THREADS, 2) void softcorr_sweep_f16_routed_kernel(const HBArgs args) {
    extern __shared__ __attribute__((aligned(16))) char smem_b[];
    int lid = xcd_remap(blockIdx.x, gridDim.x);
    const int grp = lid >= args.blocks0 ? 1 : 0;
    lid -= grp ? args.blocks0 : 0;
    const int route = args.route[grp * args.nb + lid / args.g[grp].tiles];
    if (route == K1_ROUTE_LEAN) sweep_f16_block<true, false>(args, blockIdx.x, gridDim.x, smem_b);
    else if (route == K1_ROUTE_FULL) sweep_f16_block<false, false>(args, blockIdx.x, gridDim.x, smem_b);
}
// The gate's second pass (lean form): a SMALL grid whose workgroups walk the logical blocks — in the usual case that the gate sent
// nothing back every workgroup returns after two scalar loads (the full grid cost 15 us at 64 pairs, 40 us at 512, for nothing).
__global__ __launch_bounds__(HB_THREADS, 2) void softcorr_sweep_f16_gated_kernel(const HBArgs args, int nblocks) {
    extern __shared__ __attribute__((aligned(16))) char smem_b[];
    const bool on0 = args.route[0] == K1_ROUTE_LEAN, on1 = nblocks > args.blocks0 && args.route[args.nb] == K1_ROUTE_LEAN;
    if (!on0 && !on1) return;
    for (int vb = blockIdx.x; vb < nblocks; vb += gridDim.x) {
        sweep_f16_block<true>(args, vb, nblocks, smem_b);
        __syncthreads();   // (the next block re-stages the LDS tiles)
    }
}

// both sides share ONE scale (the larger absmax): the norm pieces are sized for max |x s| < 2^12
__global__ void common_absmax_kernel(const int *__restrict__ in, int *__restrict__ out) {
    const int m = max(in[0], in[1]);
    out[0] = m;
    out[1] = m;
}

// ---------------------------------------------------------------- routing probe
// Which pass-A kernel suits a (direction, pair) depends on how many columns of a row lie within the softmax cut
// (d <= d_min + 20 / alpha): a handful on wide-spread features at large alpha (the coarse screen: one fp16 plane, lists of 16,
// no softmax term owed outside the list — pass B certifies that per row), a few dozen (first form, lean: per-entry loop, terms
// only for what leaves a list), or most of the row (flat rows, small alpha x small spread: the lean bookkeeping only costs —
// first form, every term).  An alpha rule alone got this wrong on clustered features (profiles/r3_bench_alpha.txt), so each pair
// is measured: K1P_ROWS query rows x K1P_COLS key columns (evenly spaced) of exact fp32 distances per (direction, pair) — 1024
// distances per group: the decision is taken on the mean over the launch's groups, so the sample per group can be small.  A
// row's minimum over ALL columns is estimated as min(sample minimum, mean - z(M) sigma), z(M) the normal quantile of 1 / M;
// p = fraction of the sampled distances within the cut of that minimum, averaged over the rows, then over the pairs of the
// launch (k1_route_kernel).  Thresholds: the coarse screen up to a mean fraction of 0.14 % (3 of 2048 columns within the cut:
// measured on random features it beats the lean first form up to 0.11 % and loses from 0.16 % on, where 2 % of the rows have
// more columns within the cut than its list of 16 can certify; profiles/notes_k1.md), the lean first form up to 2 %, the full
// first form beyond.  k1_gate_kernel catches what the probe gets wrong.
constexpr int K1P_ROWS = 4, K1P_COLS = 256;   // (8 x 256 with a wave per row pair measured 122 us per launch of 1024 groups: every wave
                                              // streamed the sampled key rows again, and that per-lane row streaming is L1-bound)
struct K1ProbeArgs {
    const float *f[2], *n[2];   // features [B][rows][128] and squared norms of side 0 / 1
    int rows[2];
    float cutw, p_coarse, p_lean;
    int have_coarse;
    int *route;                 // [dirs][B]
    float *frac;                // [dirs][B]
};
__global__ __launch_bounds__(256) void k1_probe_kernel(const K1ProbeArgs a) {
    // thread = one sampled key column, against all K1P_ROWS sampled query rows: every key row is read once per workgroup
    __shared__ float q[K1P_ROWS][HB_D];
    __shared__ float part[4][K1P_ROWS][3], pcnt[4][K1P_ROWS];
    const int b = blockIdx.x, dir = blockIdx.y, B = gridDim.x;
    const int N = a.rows[dir], M = a.rows[dir ^ 1];
    const float *fq = a.f[dir] + (size_t)b * N * HB_D, *fk = a.f[dir ^ 1] + (size_t)b * M * HB_D;
    const float *nq = a.n[dir] + (size_t)b * N, *nk = a.n[dir ^ 1] + (size_t)b * M;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < K1P_ROWS * HB_D; i += 256) {
        const int r = i / HB_D;
        q[r][i % HB_D] = fq[(size_t)((long)r * N / K1P_ROWS) * HB_D + i % HB_D];
    }
    __syncthreads();
    const int C = M < K1P_COLS ? M : K1P_COLS;
    const bool on = tid < C;
    const int col = on ? (int)((long)tid * M / C) : 0;
    float dot[K1P_ROWS];
#pragma unroll
    for (int r = 0; r < K1P_ROWS; ++r) dot[r] = 0.f;
    const float4 *kr = (const float4 *)(fk + (size_t)col * HB_D);
#pragma unroll 8
    for (int k = 0; k < HB_D / 4; ++k) {
        const float4 kv = kr[k];
#pragma unroll
        for (int r = 0; r < K1P_ROWS; ++r) {
            const float4 qv = *(const float4 *)&q[r][4 * k];
            dot[r] = fmaf(kv.x, qv.x, fmaf(kv.y, qv.y, fmaf(kv.z, qv.z, fmaf(kv.w, qv.w, dot[r]))));
        }
    }
    const float nkc = nk[col];
    float d[K1P_ROWS];
#pragma unroll
    for (int r = 0; r < K1P_ROWS; ++r) {
        d[r] = sqrtf(fmaxf(nq[(long)r * N / K1P_ROWS] + nkc - 2.f * dot[r], 0.f));
        float s1 = on ? d[r] : 0.f, s2 = on ? d[r] * d[r] : 0.f, mn = on ? d[r] : INFINITY;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            s1 += __shfl_xor(s1, o, 64);
            s2 += __shfl_xor(s2, o, 64);
            mn = fminf(mn, __shfl_xor(mn, o, 64));
        }
        if (lane == 0) part[wave][r][0] = s1, part[wave][r][1] = s2, part[wave][r][2] = mn;
    }
    __syncthreads();
    const float z = 1.1f + 0.2f * log2f((float)M);   // 2.9 / 3.3 / 3.7 at M = 512 / 2048 / 8192
#pragma unroll
    for (int r = 0; r < K1P_ROWS; ++r) {
        const float s1 = (part[0][r][0] + part[1][r][0]) + (part[2][r][0] + part[3][r][0]);
        const float s2 = (part[0][r][1] + part[1][r][1]) + (part[2][r][1] + part[3][r][1]);
        const float mn = fminf(fminf(part[0][r][2], part[1][r][2]), fminf(part[2][r][2], part[3][r][2]));
        const float mu = s1 / C, sg = sqrtf(fmaxf(s2 / C - mu * mu, 0.f));
        const float thr = fminf(mn, mu - z * sg) + a.cutw;
        float cnt = (on && d[r] <= thr) ? 1.f : 0.f;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
        if (lane == 0) pcnt[wave][r] = cnt;
    }
    __syncthreads();
    if (tid == 0) {
        float p = 0.f;
#pragma unroll
        for (int r = 0; r < K1P_ROWS; ++r) p += ((pcnt[0][r] + pcnt[1][r]) + (pcnt[2][r] + pcnt[3][r])) / C;
        a.frac[dir * B + b] = p / K1P_ROWS;
    }
}
// One route per direction of the launch, from the mean fraction over its pairs.  (Routing every pair by its own fraction was
// measured first: near a threshold the batch splits between two kernels, each runs with half the workgroups, and the launch
// is slower than either kernel alone — 9.47 vs 9.11 / 9.31 ms per 256 pairs on random features at alpha 33.)
__global__ __launch_bounds__(256) void k1_route_kernel(const K1ProbeArgs a, int B) {
    __shared__ float part[4];
    const int dir = blockIdx.x, tid = threadIdx.x;
    float sum = 0.f;
    for (int i = tid; i < B; i += 256) sum += a.frac[dir * B + i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    if ((tid & 63) == 0) part[tid >> 6] = sum;
    __syncthreads();
    const float p = (part[0] + part[1] + part[2] + part[3]) / B;
    const int route = (a.have_coarse && p <= a.p_coarse) ? K1_ROUTE_COARSE : p <= a.p_lean ? K1_ROUTE_LEAN : K1_ROUTE_FULL;
    for (int i = tid; i < B; i += 256) a.route[dir * B + i] = route;
}

// the reference's squared distance: k-ordered fp32 fma chain of (-2 q) . k, then + |q|^2, + |k|^2
__device__ __forceinline__ float exact_d2(const float *__restrict__ q, const float *__restrict__ k, float na, float nb) {
    float acc = 0.f;
#pragma unroll 8
    for (int c = 0; c < HB_D; c += 4) {
        const f32x4 qv = *(const f32x4 *)(q + c), kv = *(const f32x4 *)(k + c);
        acc = fmaf(-2.f * qv.x, kv.x, acc);
        acc = fmaf(-2.f * qv.y, kv.y, acc);
        acc = fmaf(-2.f * qv.z, kv.z, acc);
        acc = fmaf(-2.f * qv.w, kv.w, acc);
    }
    const float d2 = (acc + na) + nb;
    return d2 > 0.f ? d2 : 0.f;
}

// ---------------------------------------------------------------- pass B: exact re-evaluation of the candidates
struct HRGroup {
    const float *q, *k, *nq, *nk;  // fp32 rows and norms
    const float *nkmax;            // [B] max |k|^2 of the batch element
    int N, M;
    const int32_t *cidx;
    const float *cd2, *lsum;
    float *val;
    int32_t *idx;
    float *smax, *sum;
    int32_t *flagged;              // rows (b*N + i) that need the exact full recompute; flagged[-1..] see below
    int32_t *nflagged;
};
struct HRArgs {
    HRGroup g[2];
    long rows0;       // B * g[0].N
    long rows_total;
    float neg_alpha, cutw;
    int topk;
    const int *route; // per (group, batch entry) as for pass A, or nullptr = this launch takes every row
    int nb;
};

// compile-time loop: f(std::integral_constant<int, I>) for I in [B, E) (DPP controls must be constants)
template <int B, int E, class F>
__device__ __forceinline__ void static_for(F &&f) {
    if constexpr (B < E) {
        f(std::integral_constant<int, B>{});
        static_for<B + 1, E>(f);
    }
}

// The exact evaluation gathers KC candidate rows of 512 B per query row.  Four lanes load a whole 64-byte piece of a candidate
// row, the lane <-> row transpose goes through LDS, the chain is one v_fmac_f32_dpp per dimension (query values by row_share):
// 1.04 ms per launch of 512 pairs x 2 at KC = 12.  A quarter of the L1 accesses of "every lane streams its own row" (652 per wave),
// no line fetched twice; what then sets the time is how long a wave lives (two dependent round trips + the chain) times how many
// fit: a rolling window of HR4W pieces in flight (3: 126 VGPRs = 4 waves per SIMD), the group wave-uniform (pointers in scalar
// registers), XCD-aware block numbering (a pair's key rows in one L2: 5 %).  Four other access shapes were measured in round 3
// (per-lane streaming with and without a DPP-shared query row, a systolic chain over the 16 lanes of a row, persistent waves fed
// by LDS-DMA: 2.1 - 2.9 ms, each bound by something of its own) and are gone: profiles/notes_k1.md.
// acc = fma(x of lane L of the 16-lane row, y, acc) in ONE instruction (the compiler keeps update_dpp + v_fma apart, with a
// v_mov 0 for the DPP's `old` operand: three instructions).  x must have been written at least two instructions earlier (the DPP
// read-after-write hazard is not tracked through inline assembly): here the scaled query values, written before the row loads.
template <int L>
__device__ __forceinline__ void fma_row_share(float &acc, float x, float y) {
    asm volatile("v_fmac_f32_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf" : "+v"(acc) : "v"(x), "v"(y), "n"(L));
}
struct HRRow {     // what a lane needs of its row before the candidate rows can be requested
    long row;      // within the group
    int grp, jc;
    bool rvalid;
    float va, na, nkm, ls0, ls1;
};
static inline long hr_quads(const HRArgs &r) { return (r.rows0 + 3) / 4 + (r.rows_total - r.rows0 + 3) / 4; }
// KC: candidates per row in cidx / cd2 (HB_KC from the three-product sweeps, K1_KC_COARSE from the coarse screen).
// COARSE: the list comes from the one-plane screen — error band HC_ERR instead of HB_ERR, pass A's partial sum is empty: every
// entry that can rank among the first `need` OR lie within the softmax cut is evaluated exactly, the others owe no term, and the
// row is certified only if no column outside the evaluated ones can do either.
// GATED: the second pass behind k1_gate_kernel — only the directions it sent back to the first form (route == K1_ROUTE_LEAN).
template <int KC, bool COARSE, int HR4W, bool GATED>
__device__ __forceinline__ void refine_quad(const HRArgs &args, long quad, char *hr_lds) {
    constexpr int SLOTS = 4 * KC, NL = SLOTS / 16;     // candidate rows of a wave; loads per lane and 64-byte piece
    const int lane = threadIdx.x & 63, l16 = lane & 15, base = lane & 48;
    const float neg_alpha = args.neg_alpha;
    const int topk = args.topk;
    const bool cand = l16 < KC;
    // A quad (the 4 rows of a wave) never straddles the two groups, so the group - and with it every pointer of HRGroup - is
    // wave-uniform and lives in scalar registers (per-lane groups cost ~20 VGPRs, which is a wave per SIMD).
    const long nq0 = (args.rows0 + 3) / 4;
    HRRow p;
    {
        const int qd = __builtin_amdgcn_readfirstlane((int)quad);
        p.grp = qd >= nq0 ? 1 : 0;
        // (one route per direction of a launch: k1_route_kernel)
        if (GATED ? args.route[p.grp * args.nb] != K1_ROUTE_LEAN : (args.route && (args.route[p.grp * args.nb] == K1_ROUTE_COARSE) != COARSE)) return;
        const long rows = p.grp ? args.rows_total - args.rows0 : args.rows0;
        p.row = (long)(qd - (p.grp ? (int)nq0 : 0)) * 4 + (lane >> 4);
        p.rvalid = p.row < rows;
        if (!p.rvalid) p.row = rows - 1;
        const HRGroup &G = args.g[p.grp];
        p.jc = cand ? G.cidx[p.row * KC + l16] : 0x7fffffff;
        p.va = cand ? G.cd2[p.row * KC + l16] : INFINITY;
        p.na = G.nq[p.row];
        p.nkm = G.nkmax[p.row / G.N];
        p.ls0 = G.lsum[p.row * 2];
        p.ls1 = G.lsum[p.row * 2 + 1];
    }
    const HRGroup &G = args.g[p.grp];
    const long row = p.row;
    const int M = G.M;
    const int b = (int)(row / G.N);
    const int jc = p.jc;
    const bool valid = cand && jc >= 0 && jc < M;
    // (empty slots — fewer than KC columns — rank behind every column and among themselves by slot, so that every output
    // position below topk is written: with one shared "no column" value they would all take the same rank)
    const int j = valid ? jc : (0x7fffff00 | l16);
    const float na = p.na;
    const int need = topk < M ? topk : M;        // entries that must be exact
    const float delta = (COARSE ? HC_ERR : HB_ERR) * (na + p.nkm);
    const float va = valid ? p.va : INFINITY;
    // Candidates beyond the `need`-th whose approximate distance exceeds the need-th's by more than the error band cannot
    // rank among the first `need` (their exact value is above every one of those): their rows are not fetched.  From the
    // three-product sweeps they keep their approximate softmax term (usually the two margin candidates: 1/6 of the gather).
    // From the coarse screen an approximate term is worth nothing, so an entry is also evaluated if it can lie within the
    // cut — sqrt(va - delta) <= d_min + cutw with d_min <= sqrt(va_0 + delta) — and the others owe none.
    const float va_need = __shfl(va, base + need - 1, 64);
    bool skip = valid && l16 >= need && va > va_need + 2.f * delta;
    if (COARSE) {
        const float dcut = __builtin_amdgcn_sqrtf(__shfl(va, base, 64) + delta) * 1.000001f + args.cutw;
        skip = skip && (va - delta) > (dcut * dcut) * 1.000001f;
    }
    const bool eval = valid && !skip;
    float v = INFINITY;
    {
        // Lane L loads chunk L % 4 of the 64-byte piece p of candidate row L / 4 + 16 i (i < NL): 16 full accesses per
        // instruction; piece by piece the registers go to LDS (chunk c of slot s at position c ^ (s / 4 % 4): conflict-free
        // both ways) from where each candidate lane reads ITS row's piece and continues its k-ordered chain.  Two piece buffers
        // per wave; the LDS pipe serves a wave's instructions in order, so the write of piece p + 2 cannot overtake the reads
        // of piece p.
        const float *qrow = G.q + (size_t)row * HB_D;
        const f32x4 qa = *(const f32x4 *)(qrow + 8 * l16), qb = *(const f32x4 *)(qrow + 8 * l16 + 4);
        float qs[8] = {-2.f * qa.x, -2.f * qa.y, -2.f * qa.z, -2.f * qa.w, -2.f * qb.x, -2.f * qb.y, -2.f * qb.z, -2.f * qb.w};
        // (fma_row_share reads these through DPP from inline assembly: the two wait states a DPP read needs after the write of its
        // source are not tracked there - pin the writes in front of an explicit s_nop, wherever the scheduler moves things)
        asm volatile("s_nop 1" : "+v"(qs[0]), "+v"(qs[1]), "+v"(qs[2]), "+v"(qs[3]), "+v"(qs[4]), "+v"(qs[5]), "+v"(qs[6]), "+v"(qs[7]));
        const float *const kptr = eval ? G.k + ((size_t)b * M + j) * HB_D : qrow;   // (a row that is not needed: the query row)
        const float nb = eval ? G.nk[(size_t)b * M + j] : 0.f;
        const unsigned klo = (unsigned)(uintptr_t)kptr, khi = (unsigned)((uintptr_t)kptr >> 32);
        char *const wl = hr_lds + (threadIdx.x >> 6) * (2 * SLOTS * 64);
        const int ck = lane & 3, s0 = lane >> 2;
        // Slot of a candidate row in the wave's piece buffers.  Lists of 12: slot = 12 x (row of the quad) + entry, static.  Lists
        // of 16 (coarse screen): only ~11 of a row's 16 entries are evaluated, so the evaluated ones of the four rows are
        // COMPACTED — slot = number of evaluated lanes below this one — and 3 loads per lane and piece cover them (48 slots) in
        // all but ~1e-3 of the waves, which take 4; ds_permute hands every slot's pointer to the lane of that number (the
        // other lanes' query-row pointers fill the slots behind: a permutation, every lane receives one).
        int myslot = (lane >> 4) * KC + (cand ? l16 : 0);
        unsigned plo = klo, phi = khi;
        int nslots = SLOTS;
        if (COARSE) {
            const unsigned long long em = __builtin_amdgcn_ballot_w64(eval);
            const int below = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(em >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)em, 0u));
            nslots = __builtin_popcountll(em);
            const int dest = eval ? below : nslots + (lane - below);
            plo = (unsigned)__builtin_amdgcn_ds_permute(dest << 2, (int)klo);
            phi = (unsigned)__builtin_amdgcn_ds_permute(dest << 2, (int)khi);
            myslot = eval ? below : 0;
        }
        const int wsw = (s0 >> 2) & 3, rsw = (myslot >> 2) & 3;   // (s0 + 16 i) / 4 % 4 does not depend on i
        float acc = 0.f;
        typedef const __attribute__((address_space(1))) float gfloat;   // (an address rebuilt from integers is a flat one otherwise,
                                                                         // and flat loads count on the LDS counter as well)
        auto gather = [&](auto nlc) __attribute__((always_inline)) {
            constexpr int NLR = decltype(nlc)::value;   // loads per lane and 64-byte piece: 16 NLR slots
            gfloat *src[NLR];
#pragma unroll
            for (int i = 0; i < NLR; ++i) {
                const int sl = s0 + 16 * i, owner = COARSE ? sl : (sl / KC) * 16 + sl % KC;
                const unsigned lo = (unsigned)__shfl((int)plo, owner, 64), hi = (unsigned)__shfl((int)phi, owner, 64);
                src[i] = (gfloat *)(((uintptr_t)hi << 32) | lo) + 4 * ck;
            }
            constexpr int WIN = HR4W;   // pieces in flight per lane (x NLR loads)
            f32x4 kv[WIN][NLR];
#pragma unroll
            for (int pc = 0; pc < WIN; ++pc)
#pragma unroll
                for (int i = 0; i < NLR; ++i) kv[pc][i] = *(const __attribute__((address_space(1))) f32x4 *)(src[i] + 16 * pc);
            static_for<0, 8>([&](auto pcc) __attribute__((always_inline)) {
                constexpr int pc = decltype(pcc)::value;
                char *const buf = wl + (pc & 1) * (SLOTS * 64);
#pragma unroll
                for (int i = 0; i < NLR; ++i) *(f32x4 *)(buf + (s0 + 16 * i) * 64 + ((ck ^ wsw) << 4)) = kv[pc % WIN][i];
                if constexpr (pc + WIN < 8) {   // the registers just stored take the piece WIN further on
#pragma unroll
                    for (int i = 0; i < NLR; ++i) kv[pc % WIN][i] = *(const __attribute__((address_space(1))) f32x4 *)(src[i] + 16 * (pc + WIN));
                }
                __builtin_amdgcn_wave_barrier();
                f32x4 kc[4];
#pragma unroll
                for (int c = 0; c < 4; ++c) kc[c] = *(const f32x4 *)(buf + myslot * 64 + ((c ^ rsw) << 4));
                __builtin_amdgcn_wave_barrier();
                static_for<0, 4>([&](auto cc) __attribute__((always_inline)) {
                    constexpr int c = decltype(cc)::value;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        fma_row_share<2 * pc + c / 2>(acc, qs[4 * (c & 1) + e], kc[c][e]);
                    }
                });
            });
        };
        if (COARSE && nslots <= 16 * (NL - 1)) gather(std::integral_constant<int, NL - 1>{});
        else gather(std::integral_constant<int, NL>{});
        if (eval) {
            const float d2 = (acc + na) + nb;
            v = d2 > 0.f ? d2 : 0.f;
        }
    }
    const float de = eval ? sqrt_rn(v) : INFINITY;
    int rank = 0;
#pragma unroll
    for (int t = 0; t < KC; ++t) {
        const float dt = __shfl(de, base + t, 64);
        const int jt = __shfl(j, base + t, 64);
        rank += (dt < de || (dt == de && jt < j)) ? 1 : 0;
    }
    // exact softmax terms relative to the exact maximum (pass A's sum covers exactly the columns outside the list)
    float dmin = de;
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) dmin = fminf(dmin, __shfl_xor(dmin, o, 64));
    const float smax = dmin * neg_alpha;
    const float s = (eval ? de : __builtin_amdgcn_sqrtf(fmaxf(va, 0.f))) * neg_alpha;
    const float ex = (COARSE ? eval : valid) ? exp2f((s - smax) * LOG2E) : 0.f;
    float esum = ex;
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) esum += __shfl_xor(esum, o, 64);
    const float lsm = p.ls0 * exp2f((p.ls1 - smax) * LOG2E) + esum;
    // certification: every column that was not evaluated exactly — outside the list, or skipped — has approximate
    // d2 >= theta
    float vlast = (rank == need - 1) ? v : -INFINITY;  // exact d2 of the last needed entry
    float tmax = valid ? va : -INFINITY;                // approximate KC-th best
    float tskip = skip ? va : INFINITY;
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) {
        vlast = fmaxf(vlast, __shfl_xor(vlast, o, 64));
        tmax = fmaxf(tmax, __shfl_xor(tmax, o, 64));
        tskip = fminf(tskip, __shfl_xor(tskip, o, 64));
    }
    const float theta = fminf(tmax, tskip);
    bool certain = (M <= KC) || (vlast < theta - 2.f * delta);
    if (COARSE) {
        // A skipped entry needs no test here: va > va_need + 2 delta puts its exact value above va_need + delta, which is
        // at least the exact value of each of the first `need` entries, hence above vlast; and it lies outside the cut by the
        // rule that skipped it.  (Testing it against theta as above would flag a row whenever the exact `need`-th value exceeds
        // its approximation by more than the first skipped entry clears the band: 0.8 % of random rows at this error level.)
        // What is left are the columns OUTSIDE the list, all at or above tmax: none of them ranks among the first `need`, and
        // none lies within the cut of the EXACT minimum.
        const float dcut = dmin * 1.000001f + args.cutw;
        certain = (M <= KC) || (vlast < tmax - delta && (dcut * dcut) * 1.000001f < tmax - delta);
    }
    if (p.rvalid && !certain) {
        if (l16 == 0) G.flagged[atomicAdd(G.nflagged, 1)] = (int32_t)row;   // the exact kernel writes this row
    } else if (p.rvalid) {
        if (cand && rank < topk && !skip) {
            G.val[row * topk + rank] = valid ? ex / lsm : 0.f;
            G.idx[row * topk + rank] = valid ? j : 0;
        }
        if (l16 == 0) {
            if (G.smax) G.smax[row] = smax;
            if (G.sum) G.sum[row] = lsm;
        }
    }
}
// one quad per wave (XCD-aware numbering: a pair's key rows in one L2)
template <int KC, bool COARSE, int HR4W>
__global__ __launch_bounds__(256) void softcorr_refine_kernel(const HRArgs args) {
    __shared__ __attribute__((aligned(16))) char hr_lds[4 * 2 * 4 * KC * 64];
    const long nquads = (args.rows0 + 3) / 4 + (args.rows_total - args.rows0 + 3) / 4;
    const long quad = ((long)xcd_remap(blockIdx.x, gridDim.x) * blockDim.x + threadIdx.x) >> 6;
    if (quad < nquads) refine_quad<KC, COARSE, HR4W, false>(args, quad, hr_lds);
}
// Routed launch with the coarse screen among the candidates: ONE kernel for both list lengths — a wave takes the form of its direction's
// route (one route per direction: wave-uniform).  As two launches, the form that did not apply still cost its whole grid of returning
// waves IN the feature half's dependent chain: 14 us at 64 pairs, 62 us at 512 (round 6).
template <int HR4W>
__global__ __launch_bounds__(256) void softcorr_refine_routed_kernel(const HRArgs args) {
    __shared__ __attribute__((aligned(16))) char hr_lds[4 * 2 * 4 * K1_KC_COARSE * 64];
    const long nq0 = (args.rows0 + 3) / 4, nquads = nq0 + (args.rows_total - args.rows0 + 3) / 4;
    const long quad = ((long)xcd_remap(blockIdx.x, gridDim.x) * blockDim.x + threadIdx.x) >> 6;
    if (quad >= nquads) return;
    const int grp = __builtin_amdgcn_readfirstlane(quad >= nq0 ? 1 : 0);
    if (args.route[grp * args.nb] == K1_ROUTE_COARSE) refine_quad<K1_KC_COARSE, true, HR4W, false>(args, quad, hr_lds);
    else refine_quad<HB_KC, false, HR4W, false>(args, quad, hr_lds);
}
// the gate's second pass: a small grid whose waves walk the quads — it returns at once (every wave, after one scalar load per
// direction) in the usual case that the gate sent nothing back
template <int KC, int HR4W>
__global__ __launch_bounds__(256) void softcorr_refine_gated_kernel(const HRArgs args) {
    __shared__ __attribute__((aligned(16))) char hr_lds[4 * 2 * 4 * KC * 64];
    const long nq0 = (args.rows0 + 3) / 4, nquads = nq0 + (args.rows_total - args.rows0 + 3) / 4;
    const bool on0 = args.route[0] == K1_ROUTE_LEAN, on1 = nquads > nq0 && args.route[args.nb] == K1_ROUTE_LEAN;
    if (!on0 && !on1) return;
    const long nw = ((long)gridDim.x * blockDim.x) >> 6;
    for (long quad = ((long)blockIdx.x * blockDim.x + threadIdx.x) >> 6; quad < nquads; quad += nw) refine_quad<KC, false, HR4W, true>(args, quad, hr_lds);
}

// The coarse screen serves a direction well only while few of its rows fail pass B's certification: a flagged row costs the
// exact-rows kernel a whole key side (1 MB at M = 2048, ~0.3 us), a row of the lean first form ~3 ns.  The probe keeps most
// unsuitable launches away from it, but it sees 4 rows x 256 columns per pair, not the spacing of a row's 16 best.  So behind
// the coarse pass a direction with more than 1 / 128 of its rows flagged is sent through the lean first form after all: this
// kernel writes the second pass's routes (K1_ROUTE_LEAN for such a direction — its flag list emptied — and -1 for every other),
// and the lean sweep + pass B launched behind it return at once unless their direction is marked.  Nothing is read back.
struct K1GateArgs {
    const int *route;         // first-pass routes [dirs][B], or nullptr = every direction took the coarse screen
    int *route2;              // [dirs][B]
    int32_t *nflagged[2];
    long rows[2];
    int dirs, nb;
};
__global__ void k1_gate_kernel(const K1GateArgs a) {
    for (int d = 0; d < a.dirs; ++d) {
        const bool coarse = !a.route || a.route[d * a.nb] == K1_ROUTE_COARSE;
        const bool again = coarse && *a.nflagged[d] > (a.rows[d] >> 7);
        __syncthreads();
        if (again && threadIdx.x == 0) *a.nflagged[d] = 0;
        for (int b = threadIdx.x; b < a.nb; b += blockDim.x) a.route2[d * a.nb + b] = again ? K1_ROUTE_LEAN : -1;
    }
}

// ---------------------------------------------------------------- exact recompute of the uncertified rows
// One workgroup per flagged row: every lane sweeps its share of the keys with the exact arithmetic, keeps its own
// top-10 (ascending j, so ties keep the lower column) and online softmax; each wave's 64 lists are merged by
// repeated wave arg-min over the list heads, the four waves by ranking their 40 entries.
struct HXGroup {
    const float *q, *k, *nq, *nk;
    int N, M;
    float *val;
    int32_t *idx;
    float *smax, *sum;
    const int32_t *flagged, *nflagged;
};
struct HXArgs {
    HXGroup g[2];
    float neg_alpha;
    int topk;
};

// The keys go through LDS, 256 at a time, in whole coalesced rows (a wave's load instruction covers two 512-byte rows) and every thread
// runs ONE chain over ITS key's LDS row (stride 132 floats: a 16-lane group of a ds_read_b128 covers the 64 banks once).  (Rounds 2 - 5:
// every lane loaded its own key rows from global memory, 64 different cache lines per load instruction, four chains per lane in flight:
// 60 -> 50 us per launch at 64 pairs, 197 -> 119 us at 512 — round 6, same chains, same order of columns per thread: bit-identical;
// with 1 024 threads staging — 8 loads each per tile instead of 32 — and the first 256 running the chains: 42 / 109 us.)
constexpr int HX_LD = 132;   // floats per staged key row
constexpr int HX_T = 1024;   // threads: all of them stage (8 loads each per tile: the staging is what a row waits for), the first 256 run the chains
__global__ __launch_bounds__(HX_T) void softcorr_exact_rows_kernel(const HXArgs args) {
    __shared__ float sk[4][10], sm[4], sl[4];
    __shared__ int sj[4][10];
    extern __shared__ __attribute__((aligned(16))) float hx_keys[];   // [256][HX_LD]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float neg_alpha = args.neg_alpha;
    const int topk = args.topk;
    // the flagged rows of BOTH directions as one list: workgroups [0, cnt0) take direction 0's, [cnt0, cnt0 + cnt1) direction 1's — a
    // launch lasts as long as ONE row's dependent chain (round 6; the directions used to follow each other inside a workgroup: two
    // chains, 105 - 125 us per launch whatever the batch)
    const int cnt0 = args.g[0].flagged ? *args.g[0].nflagged : 0, cnt1 = args.g[1].flagged ? *args.g[1].nflagged : 0;
    {
        for (int v = blockIdx.x; v < cnt0 + cnt1; v += gridDim.x) {  // one workgroup per row: the sweep is latency-bound
            const HXGroup &G = args.g[v < cnt0 ? 0 : 1];
            const int N = G.N, M = G.M;
            const long row = G.flagged[v < cnt0 ? v : v - cnt0];
            const int b = (int)(row / N);
            const float *q = G.q + (size_t)row * HB_D;
            const float na = G.nq[row];
            KBest<10, float> kb;
            kb.init(INFINITY);
            float m = -INFINITY, l = 0.f;
            {
                const float *kb0 = G.k + (size_t)b * M * HB_D;
                for (int t0 = 0; t0 < M; t0 += 256) {
                    __syncthreads();   // (the previous tile's chains are done)
#pragma unroll
                    for (int i = 0; i < 256 * 32 / HX_T; ++i) {
                        const int r = (threadIdx.x >> 5) + (HX_T / 32) * i, c = threadIdx.x & 31;
                        const int j = t0 + r < M ? t0 + r : M - 1;
                        *(f32x4 *)(hx_keys + r * HX_LD + 4 * c) = *(const f32x4 *)(kb0 + (size_t)j * HB_D + 4 * c);
                    }
                    __syncthreads();
                    if (threadIdx.x >= 256) continue;   // (wave-uniform; the barriers above are reached by every thread on the next trip)
                    const float *kr = hx_keys + threadIdx.x * HX_LD;
                    float acc = 0.f;
#pragma unroll 8
                    for (int c = 0; c < HB_D; c += 4) {
                        const f32x4 qv = *(const f32x4 *)(q + c);
                        const f32x4 kv = *(const f32x4 *)(kr + c);
                        acc = fmaf(-2.f * qv.x, kv.x, acc);
                        acc = fmaf(-2.f * qv.y, kv.y, acc);
                        acc = fmaf(-2.f * qv.z, kv.z, acc);
                        acc = fmaf(-2.f * qv.w, kv.w, acc);
                    }
                    const int j = t0 + (int)threadIdx.x;
                    if (j < M) {
                        const float d2 = (acc + na) + G.nk[(size_t)b * M + j];
                        const float de = sqrt_rn(d2 > 0.f ? d2 : 0.f);
                        const float s = de * neg_alpha;
                        const float mn = fmaxf(m, s);
                        l = l * exp2f((m - mn) * LOG2E) + exp2f((s - mn) * LOG2E);
                        m = mn;
                        kb.insert(de, j);
                    }
                }
            }
            if (wave < 4) {   // (the staging-only waves hold no chains)
                float mm = m;
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) mm = fmaxf(mm, __shfl_xor(mm, o, 64));
                float lt = (m == -INFINITY) ? 0.f : l * exp2f((m - mm) * LOG2E);
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) lt += __shfl_xor(lt, o, 64);
                // the wave's 10 best: pop the minimum of the 64 list heads ten times
                for (int t = 0; t < 10; ++t) {
                    float bd = kb.key[0];
                    int bj = kb.idx[0];
#pragma unroll
                    for (int o = 32; o > 0; o >>= 1) {
                        const float od = __shfl_xor(bd, o, 64);
                        const int oj = __shfl_xor(bj, o, 64);
                        if (od < bd || (od == bd && oj < bj)) bd = od, bj = oj;
                    }
                    if (kb.idx[0] == bj && kb.key[0] == bd) {  // the owner pops its head
#pragma unroll
                        for (int p = 0; p < 9; ++p) kb.key[p] = kb.key[p + 1], kb.idx[p] = kb.idx[p + 1];
                        kb.key[9] = INFINITY, kb.idx[9] = 0x7fffffff;
                    }
                    if (lane == 0) sk[wave][t] = bd, sj[wave][t] = bj;
                }
                if (lane == 0) sm[wave] = mm, sl[wave] = lt;
            }
            __syncthreads();
            if (wave == 0) {  // merge the four waves: rank the 40 entries by (distance, column)
                const float gm = fmaxf(fmaxf(sm[0], sm[1]), fmaxf(sm[2], sm[3]));  // = max_j s_j exactly (s monotone in de)
                float gl = 0.f;
#pragma unroll
                for (int w = 0; w < 4; ++w) gl += (sm[w] == -INFINITY) ? 0.f : sl[w] * exp2f((sm[w] - gm) * LOG2E);
                const float md = lane < 40 ? sk[lane / 10][lane % 10] : INFINITY;
                const int mj = lane < 40 ? sj[lane / 10][lane % 10] : 0x7fffffff;
                int rank = 0;
                for (int t = 0; t < 40; ++t) {
                    const float od = sk[t / 10][t % 10];
                    const int oj = sj[t / 10][t % 10];
                    rank += (od < md || (od == md && oj < mj)) ? 1 : 0;
                }
                if (lane < 40 && rank < topk) {
                    const bool live = md != INFINITY;
                    G.val[row * topk + rank] = live ? exp2f((md * neg_alpha - gm) * LOG2E) / gl : 0.f;
                    G.idx[row * topk + rank] = live ? mj : 0;
                }
                if (lane == 0) {
                    if (G.smax) G.smax[row] = gm;
                    if (G.sum) G.sum[row] = gl;
                }
            }
            __syncthreads();
        }
    }
}

// ---------------------------------------------------------------- hard map (knnsearch_t) on the same sweep
// T[i] = argmin_j sqrt(sum_c (q_c - k_c)^2) in the reference's exact-difference form (models/loss.py:91-95,
// test.py:19-23): sequential sub / mul / add over the feature index, ties -> lowest j.  That form cannot run on the
// matrix cores, but it only has to be evaluated for the columns that can still be the minimum: pass A's candidate
// list holds the smallest mm-form distances up to its error bound E (na + nk) (coarse screen: 16 entries, HC_ERR; first form:
// 12, HB_ERR); the exact-difference value differs from the real distance by at most (d + 1) ulp-relative.  A column is
// examined when its approximate squared distance is within 2 (E + AM_DIFF) (na + nkmax) of the row's smallest; a row whose
// band reaches past its list (duplicate points, tight clusters) is re-done by a full exact scan.  The coarse screen's band is
// 40 x the first form's: if it sends more than 1 / 16 of a direction's rows to the full scan, that direction is swept again by
// the first form (argmin_gate_kernel: the extra launches are gated on the device, nothing is read back).
constexpr float AM_DIFF = 2e-5f;   // the exact-difference form against the real distance, relative to the norms

__device__ __forceinline__ float diff_d2(const float *__restrict__ q, const float *__restrict__ k) {
    float acc = 0.f;
#pragma unroll 8
    for (int c = 0; c < HB_D; c += 4) {
        const f32x4 qv = *(const f32x4 *)(q + c), kv = *(const f32x4 *)(k + c);
        const float e0 = qv.x - kv.x, e1 = qv.y - kv.y, e2 = qv.z - kv.z, e3 = qv.w - kv.w;
        const float p0 = e0 * e0, p1 = e1 * e1, p2 = e2 * e2, p3 = e3 * e3;
        acc = acc + p0;
        acc = acc + p1;
        acc = acc + p2;
        acc = acc + p3;
    }
    return acc;
}

struct AMGroup {
    const float *q, *k, *nq, *nkmax;
    int N, M;
    const int32_t *cidx;
    const float *cd2;
    int32_t *T;
    float *dmin;
    int32_t *flagged, *nflagged;
};
struct AMArgs {
    AMGroup g[2];
    long rows0, rows_total;
    const int *route;   // per (group, batch entry): K1_ROUTE_LEAN = this direction was swept again by the first form; nullptr: no gate
    int nb;
};

// KC / ERR: list length and error bound of the screen that made the lists.  GATED: the second pass (first-form lists) — only
// the directions the gate sent back.
template <int KC, bool COARSE, bool GATED>
__global__ __launch_bounds__(256) void argmin_refine_kernel(const AMArgs args) {
    long row = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= args.rows_total) return;
    const int grp = row >= args.rows0 ? 1 : 0;
    row -= grp ? args.rows0 : 0;
    if (GATED && args.route[grp * args.nb] != K1_ROUTE_LEAN) return;
    const AMGroup &G = args.g[grp];
    const int b = (int)(row / G.N);
    const float *q = G.q + (size_t)row * HB_D;
    const float band = 2.f * ((COARSE ? HC_ERR : HB_ERR) + AM_DIFF) * (G.nq[row] + G.nkmax[b]);
    const float v0 = G.cd2[row * KC];
    float best = INFINITY;
    int bj = 0x7fffffff;
    // does the band reach past the list?  It does not once a listed column lies beyond it: every column outside the list is
    // at or above the list's last valid entry.  (A list may hold fewer than KC valid entries: the coarse screen drops what
    // lies above its completeness bound.)
    bool open = true;
    for (int t = 0; t < KC; ++t) {
        const float v = G.cd2[row * KC + t];
        const int j = G.cidx[row * KC + t];
        if (j < 0 || j >= G.M) break;
        if (!(v <= v0 + band)) {
            open = false;
            break;
        }
        const float dv = sqrt_rn(diff_d2(q, G.k + ((size_t)b * G.M + j) * HB_D));
        if (dv < best || (dv == best && j < bj)) best = dv, bj = j;
    }
    if (open && G.M > KC) {
        G.flagged[atomicAdd(G.nflagged, 1)] = (int32_t)row;
        return;
    }
    G.T[row] = bj;
    if (G.dmin) G.dmin[row] = best;
}

// after the coarse pass: a direction with more than 1 / 16 of its rows flagged goes through the first form again (its flag list is
// emptied; the gated launches behind this kernel return at once for the other direction)
__global__ void argmin_gate_kernel(const AMArgs args, int dirs, int *route) {
    const int d = threadIdx.x;
    if (d >= dirs) return;
    const long rows = d ? args.rows_total - args.rows0 : args.rows0;
    const bool again = *args.g[d].nflagged > (rows >> 4);
    if (again) *args.g[d].nflagged = 0;
    for (int b = 0; b < args.nb; ++b) route[d * args.nb + b] = again ? K1_ROUTE_LEAN : K1_ROUTE_COARSE;
}

// full exact scan of the flagged rows, one workgroup per row
__global__ __launch_bounds__(256) void argmin_exact_rows_kernel(const AMArgs args) {
    __shared__ float sd[256];
    __shared__ int sj[256];
    for (int grp = 0; grp < 2; ++grp) {
        const AMGroup &G = args.g[grp];
        if (!G.flagged) continue;
        const int cnt = *G.nflagged;
        for (int f = blockIdx.x; f < cnt; f += gridDim.x) {
            const long row = G.flagged[f];
            const int b = (int)(row / G.N);
            const float *q = G.q + (size_t)row * HB_D;
            float best = INFINITY;
            int bj = 0x7fffffff;
            for (int j = threadIdx.x; j < G.M; j += 256) {  // ascending j per thread: strict < keeps the lowest
                const float dv = sqrt_rn(diff_d2(q, G.k + ((size_t)b * G.M + j) * HB_D));
                if (dv < best) best = dv, bj = j;
            }
            __syncthreads();
            sd[threadIdx.x] = best;
            sj[threadIdx.x] = bj;
            __syncthreads();
            for (int o = 128; o > 0; o >>= 1) {
                if ((int)threadIdx.x < o) {
                    const float od = sd[threadIdx.x + o];
                    const int oj = sj[threadIdx.x + o];
                    if (od < sd[threadIdx.x] || (od == sd[threadIdx.x] && oj < sj[threadIdx.x])) sd[threadIdx.x] = od, sj[threadIdx.x] = oj;
                }
                __syncthreads();
            }
            if (threadIdx.x == 0) {
                G.T[row] = sj[0];
                if (G.dmin) G.dmin[row] = sd[0];
            }
        }
    }
}

}  // namespace

// routing: Options::k1_route forces one route (K1_ROUTE_*: 0 full, 1 lean, 3 coarse; -1 = the probe decides), k1_p_coarse / k1_p_lean
// are the probe's thresholds (fractions of a row within the cut), DVM_DEBUG & 1 prints the routes of every launch (synchronous)
static void report_routes(const int *route, const float *frac, int n, hipStream_t s) {   // diagnostic
    std::vector<int> r(n);
    std::vector<float> p(n);
    (void)hipStreamSynchronize(s);
    (void)hipMemcpy(r.data(), route, n * sizeof(int), hipMemcpyDeviceToHost);
    (void)hipMemcpy(p.data(), frac, n * sizeof(float), hipMemcpyDeviceToHost);
    int cnt[4] = {0, 0, 0, 0};
    double ps = 0, pmin = 1, pmax = 0;
    for (int i = 0; i < n; ++i) {
        ++cnt[r[i] < 0 || r[i] > 3 ? 0 : r[i]];
        ps += p[i];
        pmin = p[i] < pmin ? p[i] : pmin;
        pmax = p[i] > pmax ? p[i] : pmax;
    }
    fprintf(stderr, "K1 routes: %d full, %d lean, %d coarse; fraction within the cut: mean %.4f%% (min %.4f%%, max %.4f%%)\n", cnt[0], cnt[1],
            cnt[3], 100 * ps / n, 100 * pmin, 100 * pmax);
}

// what the most recent launch_softcorr_f16 of this host thread did with its (direction, pair) entries: device pointers into the
// caller's workspace (valid until it is rewritten), read back by dvm_k1_last_routes
struct K1LastLaunch {
    const int *route = nullptr, *route2 = nullptr;   // first-pass routes (nullptr: `fixed` for every entry), the gate's second pass
    int n = 0, fixed = -1;
    hipStream_t s = nullptr;
};
static thread_local K1LastLaunch g_k1_last;

// The K1 workspace for (B, N, M): planes of both sides, candidates of both directions (one without `both`), flags.  ONE layout for
// launch_softcorr_f16 and launch_argmin_f16 (which uses neither spec, route2 nor pfrac) and for the two size queries.
struct K1Ws {
    float *nmax[2];   // [B] maxima of the norms, zero-initialised
    int *amax;        // [2] bit patterns of max|f1|, max|f2| when the caller did not fuse them into the norms
    int *spec;        // fused preparation: [0] absmax of the sampled rows (provisional scale), [1] planes must be re-made
    char *p[2];       // fp16 planes [B][rows][HB_ROWB]
    float *npad[2];   // norms padded to whole key tiles
    char *nfrag[2];   // norm fragments of the coarse screen
    int *route, *route2;   // [2B] routes of the first pass and of the gate's second pass
    float *pfrac;          // [2B] the probe's fractions
    int32_t *cidx[2], *flag[2];   // per direction: candidate columns; flag [0] = counter, [1..] = rows
    float *cd2[2], *lsum[2];
    int pad[2];       // rows of either side padded to whole key tiles
};
static size_t carve_k1(Arena &ar, int B, int N, int M, bool both, K1Ws &w) {
    // The small zero-initialised slots first, back to back (a 256-byte slot each): nmax[0], nmax[1], amax, spec are cleared by ONE
    // fill from nmax[0] to the end of spec (launch_softcorr_f16) or of amax (launch_argmin_f16); in the pair path the caller's 514
    // absmax slots lie right in front of nmax[0] and the same fill starts there (launch_softcorr_f16 tests that adjacency).
    w.nmax[0] = ar.take<float>(B), w.nmax[1] = ar.take<float>(B);
    w.amax = ar.take<int>(2);
    w.spec = ar.take<int>(2);
    w.p[0] = ar.take<char>((size_t)B * N * HB_ROWB), w.p[1] = ar.take<char>((size_t)B * M * HB_ROWB);
    w.pad[0] = (N + HB_KT - 1) / HB_KT * HB_KT, w.pad[1] = (M + HB_KT - 1) / HB_KT * HB_KT;
    w.npad[0] = ar.take<float>((size_t)B * w.pad[0]), w.npad[1] = ar.take<float>((size_t)B * w.pad[1]);
    w.nfrag[0] = ar.take<char>((size_t)B * w.pad[0] * 32), w.nfrag[1] = ar.take<char>((size_t)B * w.pad[1] * 32);
    w.route = ar.take<int>(2 * (size_t)B), w.route2 = ar.take<int>(2 * (size_t)B);
    w.pfrac = ar.take<float>(2 * (size_t)B);
    for (int d = 0; d < 2; ++d) w.cidx[d] = w.flag[d] = nullptr, w.cd2[d] = w.lsum[d] = nullptr;
    for (int d = 0; d < (both ? 2 : 1); ++d) {
        const size_t R = (size_t)B * (d == 0 ? N : M);
        w.cidx[d] = ar.take<int32_t>(R * K1_KC_COARSE);   // (candidate lists sized for the longest form's)
        w.cd2[d] = ar.take<float>(R * K1_KC_COARSE);
        w.lsum[d] = ar.take<float>(R * 2);
        w.flag[d] = ar.take<int32_t>(R + 1);
    }
    return ar.off;
}
size_t softcorr_f16_ws_bytes(int B, int N, int M, bool both) { return null_carve<K1Ws>(carve_k1, B, N, M, both); }
// bytes of nmax[0] .. the two ints at `last` (w.spec or w.amax): the one fill of the zero-initialised slots
static size_t k1_zero_bytes(const K1Ws &w, const int *last) { return (size_t)((const char *)last - (const char *)w.nmax[0]) + 2 * sizeof(int); }
// What both launchers hand to the norm preparation and to pass A, from the one layout: norms n1 / n2, scales at amax[0], amax[1];
// frags: the coarse screen's norm fragments are made.  Returns the number of pass-A workgroups.
static int k1_pass_a_args(const K1Ws &w, const float *n1, const float *n2, int B, int N, int M, bool both, bool frags, const int *amax, NormPrep &np,
                          HBArgs &a) {
    np = NormPrep{{n1, n2}, {N, M}, {w.pad[0], w.pad[1]}, {w.nmax[0], w.nmax[1]}, {both ? w.npad[0] : nullptr, w.npad[1]},
                  {frags && both ? w.nfrag[0] : nullptr, frags ? w.nfrag[1] : nullptr}, amax, {w.flag[0], both ? w.flag[1] : nullptr}};
    a.g[0] = HBGroup{w.p[0], w.p[1], amax, amax + 1, n1, w.npad[1], N, M, w.pad[1], (N + HB_QB - 1) / HB_QB, w.cidx[0], w.cd2[0], w.lsum[0]};
    a.g[1] = both ? HBGroup{w.p[1], w.p[0], amax + 1, amax, n2, w.npad[0], M, N, w.pad[0], (M + HB_QB - 1) / HB_QB, w.cidx[1], w.cd2[1], w.lsum[1]}
                  : a.g[0];
    a.blocks0 = B * a.g[0].tiles;
    a.nb = B;
    return a.blocks0 + (both ? B * a.g[1].tiles : 0);
}

// f1 [B][N][128], f2 [B][M][128] with norms n1, n2; direction 0 = rows of f1 against f2; direction 1 (optional) the
// reverse.  Outputs as the fp32 kernel: top-`topk` values/columns (topk <= 10), optional row stats.
int launch_softcorr_f16(const float *f1, const float *f2, const float *n1, const float *n2, int B, int N, int M, float neg_alpha,
                         int topk, float *val12, int32_t *idx12, float *smax12, float *sum12, float *val21, int32_t *idx21,
                         float *smax21, float *sum21, const int *amax_in, void *ws, size_t ws_bytes, hipStream_t s, int *fuse_slots) {
    // fuse_slots != nullptr (the pair path): n1 / n2 and the absmax values at amax_in are NOT computed yet - this call makes them
    // in the same pass that writes the fp16 planes (rownorm_split_kernel); fuse_slots = 512 ints of scratch
    const bool both = val21 != nullptr;
    K1Ws w;
    if (!carve_ws(ws, ws_bytes, "softcorr (fp16 path)", w, carve_k1, B, N, M, both)) return DVM_ENOSPACE;
    float *const nmax1 = w.nmax[0], *const nmax2 = w.nmax[1];
    int *const amax_own = w.amax, *const spec = w.spec;
    char *const p1 = w.p[0], *const p2 = w.p[1], *const nf1 = w.nfrag[0], *const nf2 = w.nfrag[1];
    const int *amax = amax_own;   // ONE scale for both sides (the larger absmax), see common_absmax_kernel
    int *const route = w.route, *const route2 = w.route2;
    float *const pfrac = w.pfrac;
    int32_t *const *cidx = w.cidx, *const *flag = w.flag;
    float *const *cd2 = w.cd2, *const *lsum = w.lsum;
    const long r1 = (long)B * N, r2 = (long)B * M;
    // nmax1, nmax2, amax_own and spec lie back to back in the arena (carve_k1), and in the pair path right behind the caller's
    // 514 absmax slots: one fill
    if (fuse_slots && (char *)fuse_slots + align_up(514 * sizeof(int)) == (char *)nmax1) {
        (void)hipMemsetAsync(fuse_slots, 0, align_up(514 * sizeof(int)) + k1_zero_bytes(w, spec), s);
    } else {
        (void)hipMemsetAsync(nmax1, 0, k1_zero_bytes(w, spec), s);
        if (fuse_slots) (void)hipMemsetAsync(fuse_slots, 0, 512 * sizeof(int), s);
    }
    if (fuse_slots) {
        hipLaunchKernelGGL(sample_absmax_kernel, dim3(256), dim3(256), 0, s, f1, r1, f2, r2, spec);
        {   // 2 rows per 16-lane group and trip (1: 315 us, 2: 296, 4: 365): a workgroup = 4 waves x 8 rows
            const long rmax = r1 > r2 ? r1 : r2;
            hipLaunchKernelGGL(rownorm_split_kernel<2>, dim3((unsigned)((rmax + 31) / 32), 2), dim3(256), 0, s,
                               RownormSplit{{f1, f2}, {r1, r2}, {(float *)n1, (float *)n2}, {fuse_slots, fuse_slots + 256}, {p1, p2}}, spec);
        }
        hipLaunchKernelGGL(spec_finalize_kernel, dim3(1), dim3(128), 0, s, fuse_slots, (int *)amax_in, amax_own, spec);
        hipLaunchKernelGGL(split_planes_gated_kernel, dim3(1024, 2), dim3(256), 0, s, SplitGated{{f1, f2}, {r1, r2}, {p1, p2}}, amax, spec);
    } else {
        if (!amax_in) {
            hipLaunchKernelGGL(absmax_kernel, dim3(2048), dim3(256), 0, s, f1, r1 * 32, amax_own);
            hipLaunchKernelGGL(absmax_kernel, dim3(2048), dim3(256), 0, s, f2, r2 * 32, amax_own + 1);
        }
        hipLaunchKernelGGL(common_absmax_kernel, dim3(1), dim3(1), 0, s, amax_in ? amax_in : amax_own, amax_own);
        hipLaunchKernelGGL(split_planes_kernel, dim3((unsigned)((r1 * 16 + 255) / 256)), dim3(256), 0, s, f1, r1, amax, p1);
        hipLaunchKernelGGL(split_planes_kernel, dim3((unsigned)((r2 * 16 + 255) / 256)), dim3(256), 0, s, f2, r2, amax + 1, p2);
    }
    // alpha < 32: every softmax term counts, the first form in full.  From 32 on each (direction, pair) is routed by the
    // probe; DVM_K1_ROUTE = 0 / 1 / 3 (K1_ROUTE_FULL / LEAN / COARSE) forces one kernel for all of them (A/B measurements,
    // tests/test_gpu_k1_routes.py).
    const bool lean = -neg_alpha >= 32.f;
    const Options &pol = options();
    const bool havec = coarse_supports(N, M);
    const bool routed = lean && pol.k1_route < 0;
    const int fixed = !lean ? K1_ROUTE_FULL : pol.k1_route < 0 ? -1
                     : (pol.k1_route == K1_ROUTE_COARSE && havec) ? K1_ROUTE_COARSE : pol.k1_route == K1_ROUTE_FULL ? K1_ROUTE_FULL : K1_ROUTE_LEAN;
    if (routed) {
        K1ProbeArgs pa;
        pa.f[0] = f1, pa.f[1] = f2, pa.n[0] = n1, pa.n[1] = n2;
        pa.rows[0] = N, pa.rows[1] = M;
        pa.cutw = 20.f / -neg_alpha;
        pa.p_coarse = pol.k1_p_coarse, pa.p_lean = pol.k1_p_lean;
        pa.have_coarse = havec;
        pa.route = route, pa.frac = pfrac;
        hipLaunchKernelGGL(k1_probe_kernel, dim3(B, both ? 2 : 1), dim3(256), 0, s, pa);
        hipLaunchKernelGGL(k1_route_kernel, dim3(both ? 2 : 1), dim3(256), 0, s, pa, B);
        if (pol.debug & DVM_DEBUG_K1_ROUTES) report_routes(route, pfrac, B * (both ? 2 : 1), s);
    }
    NormPrep np;
    HBArgs a;
    const int blocks = k1_pass_a_args(w, n1, n2, B, N, M, both, routed ? havec : fixed == K1_ROUTE_COARSE, amax, np, a);
    // the norms' maxima, the first form's padded norms (also behind the coarse screen, for the gate's second pass), the coarse
    // screen's norm fragments and the flagged-row counters: one launch
    launch_norm_prep(np, B, s);
    a.neg_alpha = neg_alpha;
    a.cutw = 20.f / -neg_alpha;
    a.route = routed ? route : nullptr;
    prof_note(DVM_PROF_K1_SWEEP, routed ? (havec ? "routed: softcorr_coarse_kernel | softcorr_sweep_f16_kernel<lean> | softcorr_sweep_f16_kernel<full>"
                                                 : "routed: softcorr_sweep_f16_kernel<lean> | softcorr_sweep_f16_kernel<full>")
                                        : fixed == K1_ROUTE_COARSE ? "softcorr_coarse_kernel"
                                        : fixed == K1_ROUTE_LEAN   ? "softcorr_sweep_f16_kernel<lean>"
                                                                   : "softcorr_sweep_f16_kernel<full>");
    prof_begin(s);
    // (routed: all three kernels are launched and a workgroup whose pair belongs to another one returns at once)
    if (routed ? havec : fixed == K1_ROUTE_COARSE) launch_coarse(a, nf2, nf1, amax, blocks, s);
    if (routed) {
        ensure_dyn_lds((const void *)softcorr_sweep_f16_routed_kernel, (int)HB_LDS_BYTES);
        hipLaunchKernelGGL(softcorr_sweep_f16_routed_kernel, dim3(blocks), dim3(HB_THREADS), HB_LDS_BYTES, s, a);
    } else if (fixed == K1_ROUTE_LEAN) {
        ensure_dyn_lds((const void *)softcorr_sweep_f16_kernel<true>, (int)HB_LDS_BYTES);
        hipLaunchKernelGGL(softcorr_sweep_f16_kernel<true>, dim3(blocks), dim3(HB_THREADS), HB_LDS_BYTES, s, a);
    } else if (fixed == K1_ROUTE_FULL) {
        ensure_dyn_lds((const void *)softcorr_sweep_f16_kernel<false>, (int)HB_LDS_BYTES);
        hipLaunchKernelGGL(softcorr_sweep_f16_kernel<false>, dim3(blocks), dim3(HB_THREADS), HB_LDS_BYTES, s, a);
    }
    prof_end(s);

    HRArgs r;
    r.g[0] = HRGroup{f1, f2, n1, n2, nmax2, N, M, cidx[0], cd2[0], lsum[0], val12, idx12, smax12, sum12, flag[0] + 1, flag[0]};
    r.g[1] = both ? HRGroup{f2, f1, n2, n1, nmax1, M, N, cidx[1], cd2[1], lsum[1], val21, idx21, smax21, sum21, flag[1] + 1, flag[1]}
                  : r.g[0];
    r.rows0 = r1;
    r.rows_total = r1 + (both ? r2 : 0);
    r.neg_alpha = neg_alpha;
    r.cutw = 20.f / -neg_alpha;
    r.topk = topk;
    r.route = routed ? route : nullptr;
    r.nb = B;
    prof_begin(s, DVM_PROF_K1_REFINE);
    {
        // (routed: both list lengths are launched and a wave whose direction went through the other kind of screen returns at once)
        const dim3 grid((unsigned)((hr_quads(r) * 64 + 255) / 256));
        const bool coarse = routed ? havec : fixed == K1_ROUTE_COARSE;
        // (window 3: 112 VGPRs, 4 waves per SIMD, 1.11 ms per launch of the bench; window 2: 96, 5 waves, 1.17 ms)
        if (routed && coarse) {
            hipLaunchKernelGGL((softcorr_refine_routed_kernel<3>), grid, dim3(256), 0, s, r);
        } else {
            if (coarse) hipLaunchKernelGGL((softcorr_refine_kernel<K1_KC_COARSE, true, 3>), grid, dim3(256), 0, s, r);
            if (routed || fixed != K1_ROUTE_COARSE) hipLaunchKernelGGL((softcorr_refine_kernel<HB_KC, false, 3>), grid, dim3(256), 0, s, r);
        }
        if (coarse) {   // the gate and its second pass (k1_gate_kernel)
            K1GateArgs ga{routed ? route : nullptr, route2, {flag[0], both ? flag[1] : flag[0]}, {r1, r2}, both ? 2 : 1, B};
            hipLaunchKernelGGL(k1_gate_kernel, dim3(1), dim3(256), 0, s, ga);
            a.route = route2, r.route = route2;
            ensure_dyn_lds((const void *)softcorr_sweep_f16_gated_kernel, (int)HB_LDS_BYTES);
            hipLaunchKernelGGL(softcorr_sweep_f16_gated_kernel, dim3(blocks < 2048 ? blocks : 2048), dim3(HB_THREADS), HB_LDS_BYTES, s, a, blocks);
            hipLaunchKernelGGL((softcorr_refine_gated_kernel<HB_KC, 3>), dim3(4096), dim3(256), 0, s, r);
        }
    }
    prof_end(s, DVM_PROF_K1_REFINE);
    g_k1_last = K1LastLaunch{routed ? route : nullptr, (routed ? havec : fixed == K1_ROUTE_COARSE) ? route2 : nullptr, B * (both ? 2 : 1), fixed, s};

    HXArgs x;
    x.g[0] = HXGroup{f1, f2, n1, n2, N, M, val12, idx12, smax12, sum12, flag[0] + 1, flag[0]};
    x.g[1] = both ? HXGroup{f2, f1, n2, n1, M, N, val21, idx21, smax21, sum21, flag[1] + 1, flag[1]}
                  : HXGroup{nullptr, nullptr, nullptr, nullptr, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    x.neg_alpha = neg_alpha;
    x.topk = topk;
    if (options().debug & DVM_DEBUG_K1_FLAGGED) {   // diagnostic (synchronous): rows pass B could not certify
        int n[2] = {0, 0};
        (void)hipStreamSynchronize(s);
        (void)hipMemcpy(&n[0], flag[0], sizeof(int), hipMemcpyDeviceToHost);
        if (both) (void)hipMemcpy(&n[1], flag[1], sizeof(int), hipMemcpyDeviceToHost);
        fprintf(stderr, "K1 pass B: %d + %d of %ld rows go through the exact-rows kernel\n", n[0], n[1], r.rows_total);
    }
    ensure_dyn_lds((const void *)softcorr_exact_rows_kernel, 256 * HX_LD * (int)sizeof(float));
    hipLaunchKernelGGL(softcorr_exact_rows_kernel, dim3(512), dim3(HX_T), 256 * HX_LD * sizeof(float), s, x);
    return DVM_OK;
}

// the arg-min sweep's workspace: the norms of both sides in front of the K1 layout
struct ArgminWs {
    float *n1, *n2;
    K1Ws k1;
};
static size_t carve_argmin(Arena &ar, int B, int N, int M, bool both, ArgminWs &w) {
    w.n1 = ar.take<float>((size_t)B * N), w.n2 = ar.take<float>((size_t)B * M);
    return carve_k1(ar, B, N, M, both, w.k1);
}
size_t argmin_f16_ws_bytes(int B, int N, int M, bool both) { return null_carve<ArgminWs>(carve_argmin, B, N, M, both); }

// hard maps of f1 -> f2 (T12 [B][N]) and, when T21 != nullptr, f2 -> f1 (T21 [B][M]); d = 128
int launch_argmin_f16(const float *f1, const float *f2, int B, int N, int M, int32_t *T12, float *dmin12, int32_t *T21,
                      float *dmin21, void *ws, size_t ws_bytes, hipStream_t s) {
    const bool both = T21 != nullptr;
    ArgminWs aw;
    if (!carve_ws(ws, ws_bytes, "argmin (fp16 sweep)", aw, carve_argmin, B, N, M, both)) return DVM_ENOSPACE;
    const K1Ws &w = aw.k1;
    float *const n1 = aw.n1, *const n2 = aw.n2;
    int *const amax = w.amax, *const route = w.route;
    char *const p1 = w.p[0], *const p2 = w.p[1];
    const long r1 = (long)B * N, r2 = (long)B * M;
    launch_rownorm2(f1, (int)r1, HB_D, n1, s);
    launch_rownorm2(f2, (int)r2, HB_D, n2, s);
    (void)hipMemsetAsync(w.nmax[0], 0, k1_zero_bytes(w, amax), s);   // nmax[0], nmax[1], amax: back to back (carve_k1)
    hipLaunchKernelGGL(absmax_kernel, dim3(2048), dim3(256), 0, s, f1, r1 * 32, amax);
    hipLaunchKernelGGL(absmax_kernel, dim3(2048), dim3(256), 0, s, f2, r2 * 32, amax + 1);
    hipLaunchKernelGGL(common_absmax_kernel, dim3(1), dim3(1), 0, s, amax, amax);
    hipLaunchKernelGGL(split_planes_kernel, dim3((unsigned)((r1 * 16 + 255) / 256)), dim3(256), 0, s, f1, r1, amax, p1);
    hipLaunchKernelGGL(split_planes_kernel, dim3((unsigned)((r2 * 16 + 255) / 256)), dim3(256), 0, s, f2, r2, amax + 1, p2);
    // coarse screen first (lists of 16), the first form behind the device-side gate for directions it serves badly
    const bool havec = coarse_supports(N, M);
    NormPrep np;
    HBArgs a;
    const int blocks = k1_pass_a_args(w, n1, n2, B, N, M, both, havec, amax, np, a);
    launch_norm_prep(np, B, s);
    a.neg_alpha = -100.f;  // only the candidate lists are used; the lean sweep keeps them exactly as the full one does
    a.cutw = 0.f;
    a.route = nullptr;
    AMArgs r;
    r.g[0] = AMGroup{f1, f2, n1, w.nmax[1], N, M, w.cidx[0], w.cd2[0], T12, dmin12, w.flag[0] + 1, w.flag[0]};
    r.g[1] = both ? AMGroup{f2, f1, n2, w.nmax[0], M, N, w.cidx[1], w.cd2[1], T21, dmin21, w.flag[1] + 1, w.flag[1]}
                  : AMGroup{nullptr, nullptr, nullptr, nullptr, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    r.rows0 = r1;
    r.rows_total = r1 + (both ? r2 : 0);
    r.route = nullptr;
    r.nb = B;
    const dim3 rgrid((unsigned)((r.rows_total + 255) / 256));
    if (havec) {
        launch_coarse(a, w.nfrag[1], w.nfrag[0], amax, blocks, s);
        hipLaunchKernelGGL((argmin_refine_kernel<K1_KC_COARSE, true, false>), rgrid, dim3(256), 0, s, r);
        hipLaunchKernelGGL(argmin_gate_kernel, dim3(1), dim3(64), 0, s, r, both ? 2 : 1, route);
        a.route = route, r.route = route;
    }
    ensure_dyn_lds((const void *)softcorr_sweep_f16_kernel<true>, (int)HB_LDS_BYTES);
    hipLaunchKernelGGL(softcorr_sweep_f16_kernel<true>, dim3(blocks), dim3(HB_THREADS), HB_LDS_BYTES, s, a);
    if (havec) hipLaunchKernelGGL((argmin_refine_kernel<HB_KC, false, true>), rgrid, dim3(256), 0, s, r);
    else hipLaunchKernelGGL((argmin_refine_kernel<HB_KC, false, false>), rgrid, dim3(256), 0, s, r);
    hipLaunchKernelGGL(argmin_exact_rows_kernel, dim3(512), dim3(256), 0, s, r);
    return DVM_OK;
}

}  // namespace dvm

// Diagnostic, SYNCHRONOUS (it waits for the launch's stream and copies a few hundred bytes to the host): which pass-A kernel the
// most recent soft-correspondence launch of this host thread sent its (direction, pair) entries to.  counts[0] = full first form,
// [1] = lean first form, [2] = coarse screen, [3] = entries the gate swept AGAIN with the lean form behind the coarse screen,
// [4] = entries in all.  Valid only while the launch's workspace has not been rewritten (call it right after the launch).
DVM_EXPORT int dvm_k1_last_routes(int *counts) {
    DVM_REQUIRE(counts, "dvm_k1_last_routes: null pointer");
    const dvm::K1LastLaunch &L = dvm::g_k1_last;
    for (int i = 0; i < 5; ++i) counts[i] = 0;
    DVM_REQUIRE(L.n > 0, "dvm_k1_last_routes: no soft-correspondence launch on this thread yet");
    counts[4] = L.n;
    if (hipStreamSynchronize(L.s) != hipSuccess) {
        dvm::set_error("dvm_k1_last_routes: stream synchronisation failed");
        return DVM_ELAUNCH;
    }
    std::vector<int> r(L.n, L.fixed), r2(L.n, -1);
    if (L.route && hipMemcpy(r.data(), L.route, L.n * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return DVM_ELAUNCH;
    if (L.route2 && hipMemcpy(r2.data(), L.route2, L.n * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return DVM_ELAUNCH;
    for (int i = 0; i < L.n; ++i) {
        counts[r[i] == dvm::k1::K1_ROUTE_COARSE ? 2 : r[i] == dvm::k1::K1_ROUTE_LEAN ? 1 : 0] += 1;
        if (r2[i] == dvm::k1::K1_ROUTE_LEAN) counts[3] += 1;
    }
    return DVM_OK;
}
