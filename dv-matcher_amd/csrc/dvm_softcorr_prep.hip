// dvm_softcorr_prep.hip — the preparation of a K1 call (dvm_softcorr_f16.h): squared row norms, the common power-of-two scale
// and the fp16 planes x s = h + m of both feature sets, in one of two forms (launch_prep) that leave the same bytes.
#include "dvm_softcorr_f16.h"

namespace dvm {
namespace {

using namespace k1;

// ---------------------------------------------------------------- scale + split: fp32 rows -> fp16 planes
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

// both sides share ONE scale (the larger absmax): the norm pieces are sized for max |x s| < 2^12
__global__ void common_absmax_kernel(const int *__restrict__ in, int *__restrict__ out) {
    const int m = max(in[0], in[1]);
    out[0] = m;
    out[1] = m;
}

}  // namespace

void k1::launch_prep(const K1Sides &c, const K1Ws &w, K1Prep form, hipStream_t s) {
    const float *const f1 = c.f[0], *const f2 = c.f[1];
    const long r1 = c.total(0), r2 = c.total(1);
    int *const side_amax = w.slots + 512;
    (void)hipMemsetAsync(w.slots, 0, w.zero_bytes, s);   // slots, nmax, amax, spec
    if (form == K1_PREP_FUSED) {
        hipLaunchKernelGGL(sample_absmax_kernel, dim3(256), dim3(256), 0, s, f1, r1, f2, r2, w.spec);
        {   // 2 rows per 16-lane group and trip (1: 315 us, 2: 296, 4: 365): a workgroup = 4 waves x 8 rows
            const long rmax = r1 > r2 ? r1 : r2;
            hipLaunchKernelGGL(rownorm_split_kernel<2>, dim3((unsigned)((rmax + 31) / 32), 2), dim3(256), 0, s,
                               RownormSplit{{f1, f2}, {r1, r2}, {c.n[0], c.n[1]}, {w.slots, w.slots + 256}, {w.p[0], w.p[1]}}, w.spec);
        }
        // (the kernel leaves the absmax of either side at side_amax as well; nothing reads it in this form: the gated split and
        // every later kernel take the common value at w.amax)
        hipLaunchKernelGGL(spec_finalize_kernel, dim3(1), dim3(128), 0, s, w.slots, side_amax, w.amax, w.spec);
        hipLaunchKernelGGL(split_planes_gated_kernel, dim3(1024, 2), dim3(256), 0, s, SplitGated{{f1, f2}, {r1, r2}, {w.p[0], w.p[1]}}, w.amax, w.spec);
    } else {
        for (int sd = 0; sd < 2; ++sd) launch_rownorm2_absmax(c.f[sd], (int)c.total(sd), c.n[sd], w.slots + 256 * sd, s);
        launch_absmax_finalize(w.slots, 2, side_amax, s);
        hipLaunchKernelGGL(common_absmax_kernel, dim3(1), dim3(1), 0, s, side_amax, w.amax);
        hipLaunchKernelGGL(split_planes_kernel, dim3((unsigned)((r1 * 16 + 255) / 256)), dim3(256), 0, s, f1, r1, w.amax, w.p[0]);
        hipLaunchKernelGGL(split_planes_kernel, dim3((unsigned)((r2 * 16 + 255) / 256)), dim3(256), 0, s, f2, r2, w.amax + 1, w.p[1]);
    }
}

}  // namespace dvm
