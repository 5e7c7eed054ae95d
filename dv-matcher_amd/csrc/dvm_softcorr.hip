// dvm_softcorr.hip — K1: fused feature-distance + row-softmax + top-k soft correspondence.
//
// Replaces knnsearch_t_grad + topk_pi (reference models/loss.py:110-114, 1339-1347, 1404-1407):
// the N x M distance / softmax matrices are never written to HBM.  Squared distances are the
// matmul form of torch.cdist, [-2a,|a|^2,1].[b,1,|b|^2], evaluated as a k-ordered fp32 fma
// chain — on the matrix cores v_mfma_f32_32x32x2_f32 computes exactly that chain, so the
// distances equal the reference's CPU (MKL sgemm) values bit for bit and the top-k columns /
// arg-max map are bit-exact integers.
//
// One workgroup owns 256 query rows (8 waves x 32) and sweeps all M keys through the distance tile of
// dvm_dist_tile.h, which defines the layout, the chain, the workgroup geometry, a lane's row frame and the sweep loops
// (two_role_sweep, scalar_sweep); the top-k list's half-lane merge and flagged-candidate loop are next to KBest in
// dvm_common.h.  What is here: the row norms, the epilogues, the launchers and the entry points.
#include <stdlib.h>

#include "dvm_dist_tile.h"

namespace dvm {

using namespace dtile;


// ------------------------------------------------------------------ row norms
__global__ void rownorm2_kernel(const float *__restrict__ x, int rows, int K, float *__restrict__ out) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows) return;
    out[i] = aten_sumsq_row(x + (size_t)i * K, K);
}

// K = 128, coalesced: 32 lanes per row.  Same additions in the same order as aten_sumsq_row (K = 128:
// vec_size 16, size_ilp 4 -> lane l, ILP slot k accumulate x[(4i+k)*8 + l]^2 over i = 0..3, then
// ((k0 + k1) + k2) + k3, then lanes 0..7 added in order): element 32 i + 8 k + l sits in lane 8 k + l.
// All cross-lane traffic stays on the DPP network / v_permlane16_swap (17 dependent ds_bpermute round trips per wave
// otherwise: the kernel ran at 1.3 TB/s).
__device__ __forceinline__ float dpp_ror8(float v) {      // lane j of a 16-lane row <- lane (j + 8) % 16
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x128, 0xf, 0xf, false));
}
__device__ __forceinline__ float dpp_shr1_zero(float v) {  // lane j <- lane j - 1 of its row; lane 0 of a row <- 0
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x111, 0xf, 0xf, false));
}
constexpr int RN_ROWS = 8;   // rows per 32-lane half: 4 KB of loads in flight per half before the first reduction
__global__ __launch_bounds__(256) void rownorm2_k128_kernel(const float *__restrict__ x, int rows, float *__restrict__ out,
                                                            int *__restrict__ absmax) {
    const int lane = threadIdx.x & 63, l32 = lane & 31;
    const long half = ((long)blockIdx.x * blockDim.x + threadIdx.x) >> 5;   // 32-lane half -> rows [half * 8, half * 8 + 8)
    float v[RN_ROWS][4];
#pragma unroll
    for (int q = 0; q < RN_ROWS; ++q) {
        const long row0 = half * RN_ROWS + q, row = row0 < rows ? row0 : rows - 1;
        const float *p = x + row * 128 + l32;
#pragma unroll
        for (int i = 0; i < 4; ++i) v[q][i] = p[32 * i];
    }
    float am = 0.f;
#pragma unroll
    for (int q = 0; q < RN_ROWS; ++q) {
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            s = s + v[q][i] * v[q][i];
            am = fmaxf(am, fabsf(v[q][i]));
        }
        // lanes 8k + l of a 32-lane half: k = 1 is 8 lanes up in the same 16-lane row, k = 2, 3 sit in the next row
        const unsigned su = __float_as_uint(s);
        const auto sw = __builtin_amdgcn_permlane16_swap(su, su, false, false);   // sw[1]: even rows <- the odd row above them
        const float up = __uint_as_float(sw[1]);
        const float r = ((s + dpp_ror8(s)) + up) + dpp_ror8(up);  // valid in lanes l32 < 8 (k = 0)
        // fin = (((r0 + r1) + r2) ... + r7): u_j <- u_{j-1} + r_j seven times leaves it in lane 7 of the half
        float u = r;
#pragma unroll
        for (int st = 0; st < 7; ++st) u = dpp_shr1_zero(u) + r;
        const long row0 = half * RN_ROWS + q;
        if (l32 == 7 && row0 < rows) out[row0] = u;
    }
    if (absmax) {  // optional: bit pattern of max |x| of the tensor (the fp16 split's scale, dvm_softcorr_prep.hip)
        int m = __float_as_int(am);   // non-negative floats order like their bit patterns
        m = max(m, __builtin_amdgcn_update_dpp(0, m, 0x111, 0xf, 0xf, false));  // row_shr:1
        m = max(m, __builtin_amdgcn_update_dpp(0, m, 0x112, 0xf, 0xf, false));  // row_shr:2
        m = max(m, __builtin_amdgcn_update_dpp(0, m, 0x114, 0xf, 0xf, false));  // row_shr:4
        m = max(m, __builtin_amdgcn_update_dpp(0, m, 0x118, 0xf, 0xf, false));  // row_shr:8
        m = max(m, __builtin_amdgcn_update_dpp(0, m, 0x142, 0xa, 0xf, false));  // row_bcast:15
        m = max(m, __builtin_amdgcn_update_dpp(0, m, 0x143, 0xc, 0xf, false));  // row_bcast:31 -> lane 63 = the wave's max
        // 256 slots (one address would serialise the waves); only waves that would raise a slot's maximum touch it
        int *slot = absmax + (blockIdx.x & 255);
        if (lane == 63 && m > __atomic_load_n(slot, __ATOMIC_RELAXED)) atomicMax(slot, m);
    }
}

// ------------------------------------------------------- per-row running state
template <int TOPK>
struct RowState {
    KBest<TOPK, float> kb;  // keyed on the post-sqrt distance, as torch.topk sees it
    float smax;             // running max of s = d * neg_alpha   (-inf initially)
    float l;                // sum exp(s - smax)
    __device__ __forceinline__ void init() {
        kb.init(INFINITY);
        smax = -INFINITY;
        l = 0.f;
    }
    __device__ __forceinline__ void rescale(float new_smax) {
        if (new_smax > smax) {
            l = l * exp2f((smax - new_smax) * LOG2E);  // smax=-inf, l=0 -> 0*0
            smax = new_smax;
        }
    }
};

// a finished row: the list, smax = max of s and l = sum exp(s - smax)
template <int TOPK>
__device__ __forceinline__ void store_row(const KBest<TOPK, float> &kb, float smax, float l, int topk, int M, float neg_alpha, float *val,
                                          int32_t *idx, float *row_smax, float *row_sum) {
    float inv = 1.0f / l;
#pragma unroll
    for (int t = 0; t < TOPK; ++t) {
        if (t < topk) {
            bool live = t < M;
            float s = kb.key[t] * neg_alpha;
            val[t] = live ? exp2f((s - smax) * LOG2E) * inv : 0.f;
            idx[t] = live ? kb.idx[t] : 0;
        }
    }
    if (row_smax) *row_smax = smax;
    if (row_sum) *row_sum = l;
}

// ------------------------------------------------------------ scalar variant
// One thread per query row (the scalar sweep of dvm_dist_tile.h).  Any d % 4 == 0.  Reference kernel for the
// MFMA variant and the fallback for d != 128.

template <int TOPK>
__global__ __launch_bounds__(128) void softcorr_scalar_kernel(const float *__restrict__ f1, const float *__restrict__ f2,
                                                              const float *__restrict__ n1, const float *__restrict__ n2,
                                                              int N, int M, int d, float neg_alpha, int topk,
                                                              float *__restrict__ pi_val, int32_t *__restrict__ pi_idx,
                                                              float *__restrict__ row_smax, float *__restrict__ row_sum) {
    const ScalarFrame f = scalar_frame(f1, n1, N, d);
    const float na = f.na;
    RowState<TOPK> st;
    st.init();
    scalar_sweep(
        f, f2, n2, M, d, [](int, bool, float *) {},
        [&](int j0, const float (&acc)[SC_KT], const float *kn) {   // distances, online softmax, top-k
            float dd[SC_KT];
            float tmin = INFINITY;
#pragma unroll
            for (int j = 0; j < SC_KT; ++j) {
                dd[j] = sqrt_rn(sqdist<false>(acc[j], na, kn[j]));
                tmin = fminf(tmin, dd[j]);
            }
            st.rescale(tmin * neg_alpha);
#pragma unroll
            for (int j = 0; j < SC_KT; ++j) {
                float s = dd[j] * neg_alpha;
                st.l += exp2f((s - st.smax) * LOG2E);
                st.kb.insert(dd[j], j0 + j);
            }
        });
    if (f.i < N) {
        size_t row = (size_t)f.b * N + f.i;
        store_row<TOPK>(st.kb, st.smax, st.l, topk, M, neg_alpha, pi_val + row * topk, pi_idx + row * topk,
                        row_smax ? row_smax + row : nullptr, row_sum ? row_sum + row : nullptr);
    }
}

// ------------------------------------------------------------ dense Pi (API compatibility)
// knnsearch_t_grad as a dense (N x M) matrix for callers that really want it (reference
// models/loss.py:110-114, deform.py:241).  Recomputes the distances tile by tile and normalises
// with the row statistics of the fused kernel.
template <int DUMMY>
__global__ __launch_bounds__(128) void softcorr_dense_kernel(const float *__restrict__ f1, const float *__restrict__ f2,
                                                             const float *__restrict__ n1, const float *__restrict__ n2,
                                                             const float *__restrict__ row_smax, const float *__restrict__ row_sum,
                                                             int N, int M, int d, float neg_alpha, float *__restrict__ P) {
    // (its own loop and chain, one key at a time: scalar_sweep's 32 accumulators would cost it 3 of its 8 waves per SIMD)
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float *kt = smem;
    float *kn = smem + SC_KT * d;
    const ScalarFrame f = scalar_frame(f1, n1, N, d);
    const int b = f.b, i = f.i;
    const float *q = f.q;
    const float na = f.na;
    const float smax = row_smax[(size_t)b * N + f.ic];
    const float inv = 1.0f / row_sum[(size_t)b * N + f.ic];
    const float *kbase = f2 + (size_t)b * M * d;
    for (int j0 = 0; j0 < M; j0 += SC_KT) {
        __syncthreads();
        scalar_stage_keys(kt, kbase, j0, M, d);
        if (threadIdx.x < SC_KT) kn[threadIdx.x] = (j0 + threadIdx.x < M) ? n2[(size_t)b * M + j0 + threadIdx.x] : INFINITY;
        __syncthreads();
        for (int j = 0; j < SC_KT && j0 + j < M; ++j) {
            float acc = 0.f;
            for (int c = 0; c < d; c += 4) {
                f32x4 qv = *(const f32x4 *)(q + c), kv = *(const f32x4 *)(kt + j * d + c);
                acc = fmaf(-2.f * qv.x, kv.x, acc);
                acc = fmaf(-2.f * qv.y, kv.y, acc);
                acc = fmaf(-2.f * qv.z, kv.z, acc);
                acc = fmaf(-2.f * qv.w, kv.w, acc);
            }
            float s = sqrt_rn(sqdist<false>(acc, na, kn[j])) * neg_alpha;
            if (i < N) P[((size_t)b * N + i) * M + j0 + j] = exp2f((s - smax) * LOG2E) * inv;
        }
    }
}

// -------------------------------------------------------------- MFMA variant
// [2] x { keys, norms } + per wave the staging block of this sub-tile's 16 squared distances of each lane
constexpr size_t MF_LDS_BYTES = ((size_t)2 * (ROWS_FLOATS + KT) + (size_t)SW_WAVES * SW_STAGE) * sizeof(float);

__device__ __forceinline__ float select16(const float (&v)[16], int b) {
    float a0 = (b & 1) ? v[1] : v[0], a1 = (b & 1) ? v[3] : v[2], a2 = (b & 1) ? v[5] : v[4], a3 = (b & 1) ? v[7] : v[6];
    float a4 = (b & 1) ? v[9] : v[8], a5 = (b & 1) ? v[11] : v[10], a6 = (b & 1) ? v[13] : v[12],
          a7 = (b & 1) ? v[15] : v[14];
    float b0 = (b & 2) ? a1 : a0, b1 = (b & 2) ? a3 : a2, b2 = (b & 2) ? a5 : a4, b3 = (b & 2) ? a7 : a6;
    float c0 = (b & 4) ? b1 : b0, c1 = (b & 4) ? b3 : b2;
    return (b & 8) ? c1 : c0;
}

// One launch covers up to two "groups" (the two directions of a pair batch: (f1 -> f2) and
// (f2 -> f1)), each with its own query/key tensors and outputs.
struct SCGroup {
    const float *q, *k, *nq, *nk;  // queries [B][N][128], keys [B][M][128], their |.|^2
    int N, M, tiles;               // tiles = ceil(N / SW_QB)
    float *val;
    int32_t *idx;
    float *smax, *sum;
};
struct SCArgs {
    SCGroup g[2];
    int blocks0;  // B * g[0].tiles : logical block ids below this belong to group 0
    float neg_alpha;
    float cutw;  // 20 / alpha: distance window above the row minimum whose softmax terms are kept (LEAN)
    int topk;
};

// Epilogue design: per candidate the fast path is {2 add, max, v_sqrt_f32, fma, v_exp_f32, add,
// 2 cmp} — the 1-ulp hardware sqrt feeds only softmax terms whose weight is < 3e-4.  Candidates
// that may enter the top-k (d2 <= threshold^2) or carry a significant weight are re-evaluated
// with the correctly rounded sqrt and the reference's rounding sequence (s = d*neg_alpha, s - c)
// inside a compacted, wave-uniform loop, so the ranking and the dominant terms stay exact.
template <int TOPK, bool LEAN>
__global__ __launch_bounds__(SW_THREADS, 2) void softcorr_mfma_kernel(const SCArgs args) {
    // __launch_bounds__(512, 2): two waves per SIMD, i.e. ONE 512-thread workgroup per CU
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float *const ktile0 = smem;                    // [2][KT][LDK]
    float *const knorm0 = smem + 2 * ROWS_FLOATS;  // [2][KT]
    float *const stage = knorm0 + 2 * KT + (threadIdx.x >> 6) * SW_STAGE + (threadIdx.x & 63);  // this lane's column

    int lid = xcd_remap(blockIdx.x, gridDim.x);
    const int grp = lid >= args.blocks0 ? 1 : 0;
    lid -= grp ? args.blocks0 : 0;
    const SCGroup &G = args.g[grp];
    const int N = G.N, M = G.M;
    const float neg_alpha = args.neg_alpha;
    RowFrame f;   // this lane's query row
    row_frame(f, lid, G.tiles, N, G.q, G.nq);
    const int b = f.b, tid = f.tid, r32 = f.r32, h = f.h;
    const float na = f.nrm;

    const float *kbase = G.k + (size_t)b * M * D;
    const float *knb = G.nk + (size_t)b * M;

    KBest<TOPK, float> kb;  // keyed on the correctly rounded distance
    kb.init(INFINITY);
    float cref = -INFINITY;  // running reference shift (~ max of s = d*neg_alpha), softmax is shift-invariant
    float l = 0.f;           // sum exp(s - cref)
    float thr2 = INFINITY;   // conservative squared-distance bound for "may enter the top-k"
    const float a2 = neg_alpha * LOG2E;

    const int ntiles = (M + KT - 1) / KT;
    f32x4 pre[SW_LD_PER_THREAD];
    float pren = 0.f;

    auto issue_loads = [&](int t) {
        const int j0 = t * KT;
        issue_tile<SW_THREADS>(kbase, j0, M, tid, pre);
        if (tid < KT) pren = (j0 + tid < M) ? knb[j0 + tid] : INFINITY;
    };
    auto commit_loads = [&](int buf) {
        commit_tile<SW_THREADS>(ktile0 + buf * ROWS_FLOATS, tid, pre);
        if (tid < KT) knorm0[buf * KT + tid] = pren;
    };

    // the chain and |key|^2 of this lane's 16 keys
    f32x16 acc;
    float nbv[16];
    auto mfma_chain = [&](int buf, int sub) {
        dist_chain(ktile0 + buf * ROWS_FLOATS, sub, r32, h, f.q, acc);
        lane_scalars(knorm0 + buf * KT, sub, h, nbv);
    };

    // Epilogue.  fp32 MFMA executes on the same ALUs as VALU code (tools/probe_interleave.hip: every
    // VALU instruction adds its full issue time to the chain), so the epilogue is kept lean:
    //   LEAN (alpha >= 32): per candidate only {2 adds, 1 compare}: it is looked at again iff its squared
    //     distance is below lim2 = max(top-k bound, significance bound); everything else contributes
    //     < e^-20 to the softmax sum and is dropped.  Flagged candidates go through the exact path.
    //   !LEAN (flat softmax): every candidate adds a fast exp term; flagged ones are replaced exactly.
    // The 16 squared distances are parked in LDS ([r][lane], conflict-free) for the dynamic pick.
    float lim2 = INFINITY;
    const float cutw = args.cutw;
    auto epilogue = [&](int t, int sub) {
        unsigned mask = 0;
        float c2 = 0.f;
        if (LEAN) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                float v = sqdist_sum<false>(acc[r], na, nbv[r]);
                stage[r * 64] = v;
                mask |= (v <= lim2) ? (1u << r) : 0u;
            }
        } else {
            float df[16];
            float tminf = INFINITY;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                float v = sqdist_sum<false>(acc[r], na, nbv[r]);
                stage[r * 64] = v;
                mask |= (v <= lim2) ? (1u << r) : 0u;
                float f = __builtin_amdgcn_sqrtf(fabsf(v));
                df[r] = f;
                tminf = fminf(tminf, f);
            }
            const float cnew = tminf * neg_alpha;
            if (cnew > cref) {
                l = l * exp2f((cref - cnew) * LOG2E);  // cref = -inf, l = 0 -> 0 * 0
                cref = cnew;
            }
            c2 = cref * LOG2E;
            float lsum = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                float arg = fmaf(df[r], a2, -c2);
                lsum += __builtin_amdgcn_exp2f(arg);
                mask |= (arg > -11.5f) ? (1u << r) : 0u;
            }
            l += lsum;
        }
        // the exact path of the flagged candidates (inactive lanes process +inf, a no-op)
        for_each_flagged(mask, stage, [&](bool act, int bpos, float v2) {
            v2 = act ? (v2 > 0.f ? v2 : 0.f) : INFINITY;
            const float de = sqrt_rn(v2);
            const float s = de * neg_alpha;  // -inf for inactive lanes
            if (LEAN) {
                const float cnew = fmaxf(cref, s);
                const float sc = (cnew == cref) ? 1.f : __builtin_amdgcn_exp2f((cref - cnew) * LOG2E);
                const float term = act ? __builtin_amdgcn_exp2f((s - cnew) * LOG2E) : 0.f;
                l = l * sc + term;
                cref = cnew;
            } else {
                const float dfast = __builtin_amdgcn_sqrtf(v2);
                // replace this term's fast value by the reference-rounded one (both 0 for +inf)
                l += __builtin_amdgcn_exp2f((s - cref) * LOG2E) - __builtin_amdgcn_exp2f(fmaf(dfast, a2, -c2));
            }
            kb.insert_nb(de, t * KT + sub * 32 + lane_key(bpos, h));
        });
        // bounds for the next sub-tile.  Top-k: the row's k-th best is at most min(a_k, b_k, max(a_m, b_m))
        // with a, b the sorted lists of the two half-lanes and m = k/2 (2m elements lie below that max).
        {
            const float wk = kb.key[TOPK - 1], wm = kb.key[TOPK / 2 - 1], w0 = kb.key[0];
            const float pk = __shfl_xor(wk, 32, 64), pm = __shfl_xor(wm, 32, 64);
            const float w = fminf(fminf(wk, pk), fmaxf(wm, pm));
            thr2 = (w * w) * 1.0000004f;
            if (LEAN) {
                const float dmin = fminf(w0, __shfl_xor(w0, 32, 64));
                const float cut = dmin + cutw;  // beyond this the softmax term is < e^-20 of the largest
                lim2 = fmaxf(thr2, (cut * cut) * 1.000001f);
            } else {
                lim2 = thr2;
            }
        }
    };

    const int role = __builtin_amdgcn_readfirstlane(f.wave >> 2);
    two_role_sweep<false>(ntiles, role, issue_loads, commit_loads, mfma_chain, epilogue);

    // merge the two half-lanes that share a query (lane, lane^32)
    {
        float co = __shfl_xor(cref, 32, 64), lo = __shfl_xor(l, 32, 64);
        float cm = fmaxf(cref, co);
        float a = (cref == -INFINITY) ? 0.f : l * exp2f((cref - cm) * LOG2E);
        float bb = (co == -INFINITY) ? 0.f : lo * exp2f((co - cm) * LOG2E);
        l = a + bb;
        cref = cm;
        merge_halves(kb);
    }
    if (h == 0 && f.row < N) {
        const size_t row = (size_t)b * N + f.row;
        const int topk = args.topk;
        const float smax = kb.key[0] * neg_alpha;                  // exact max of s
        const float lsm = l * exp2f((cref - smax) * LOG2E);        // sum exp(s - smax)
        store_row<TOPK>(kb, smax, lsm, topk, M, neg_alpha, G.val + row * topk, G.idx + row * topk, G.smax ? G.smax + row : nullptr,
                        G.sum ? G.sum + row : nullptr);
    }
}

constexpr float LEAN_MIN_ALPHA = 32.f;

template <int TOPK>
static void launch_softcorr_mfma(SCArgs &a, int blocks, hipStream_t s) {
    ensure_dyn_lds((const void *)softcorr_mfma_kernel<TOPK, true>, (int)MF_LDS_BYTES);
    ensure_dyn_lds((const void *)softcorr_mfma_kernel<TOPK, false>, (int)MF_LDS_BYTES);
    const float alpha = -a.neg_alpha;
    a.cutw = 20.f / alpha;
    if (alpha >= LEAN_MIN_ALPHA)
        hipLaunchKernelGGL((softcorr_mfma_kernel<TOPK, true>), dim3(blocks), dim3(SW_THREADS), MF_LDS_BYTES, s, a);
    else
        hipLaunchKernelGGL((softcorr_mfma_kernel<TOPK, false>), dim3(blocks), dim3(SW_THREADS), MF_LDS_BYTES, s, a);
}

// K == 128 only: also maxes the bit pattern of max |x| into the 256 slots of `absmax_slots` (zero them first);
// launch_absmax_finalize folds nt x 256 slots into nt values
void launch_rownorm2_absmax(const float *x, int rows, float *out, int *absmax_slots, hipStream_t s) {
    hipLaunchKernelGGL(rownorm2_k128_kernel, dim3((unsigned)((((long)rows + RN_ROWS - 1) / RN_ROWS * 32 + 255) / 256)), dim3(256), 0, s, x, rows, out,
                       absmax_slots);
}
__global__ void absmax_finalize_kernel(const int *__restrict__ slots, int *__restrict__ out) {
    int v = 0;
    for (int i = threadIdx.x; i < 256; i += 64) v = max(v, slots[blockIdx.x * 256 + i]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
    if (threadIdx.x == 0) out[blockIdx.x] = v;
}
void launch_absmax_finalize(const int *slots, int nt, int *out, hipStream_t s) {
    hipLaunchKernelGGL(absmax_finalize_kernel, dim3(nt), dim3(64), 0, s, slots, out);
}

void launch_rownorm2(const float *x, int rows, int K, float *out, hipStream_t s) {
    if (K == 128)
        launch_rownorm2_absmax(x, rows, out, nullptr, s);
    else
        hipLaunchKernelGGL(rownorm2_kernel, dim3((rows + 255) / 256), dim3(256), 0, s, x, rows, K, out);
}

}  // namespace dvm

using namespace dvm;

DVM_EXPORT int dvm_rownorm2_f32(const float *x, int rows, int K, float *out, void *stream) {
    DVM_REQUIRE(x && out && rows >= 0 && K >= 1, "dvm_rownorm2_f32: bad arguments");
    if (rows == 0) return DVM_OK;
    launch_rownorm2(x, rows, K, out, (hipStream_t)stream);
    DVM_CHECK_LAUNCH("rownorm2");
    return DVM_OK;
}

DVM_EXPORT size_t dvm_softcorr_workspace_bytes(int B, int N, int M, int d) {
    return null_carve<K1NormsWs>(carve_k1_norms, B, N, M, false, d == D);   // (d == 128: sized for the fp16-split sweep, whichever variant is asked for)
}

DVM_EXPORT int dvm_softcorr_fwd_f32(const float *f1, const float *f2, int B, int N, int M, int d, float neg_alpha,
                                    int topk, float *pi_val, int32_t *pi_idx, float *row_smax, float *row_sum,
                                    int variant, void *ws, size_t ws_bytes, void *stream) {
    const int rc0 = softcorr_family_check("dvm_softcorr_fwd_f32", f1 && f2 && pi_val && pi_idx, B, N, M, d, topk, neg_alpha, variant, 3);
    if (rc0 != DVM_OK) return rc0;
    DVM_REQUIRE(variant < 2 || d == D, "dvm_softcorr_fwd_f32: the matrix-core variants need d == 128");
    DVM_REQUIRE(variant != 3 || topk <= 10, "dvm_softcorr_fwd_f32: the bf16 variant keeps 12 candidates (topk <= 10)");
    if (variant == 0 && d == D && topk <= 10) variant = 3;   // auto: the fp16-split sweep (variants 1 / 2: the `variant` argument)
    K1NormsWs w;   // the norms of both sides and, for the fp16-split sweep, its workspace
    if (!carve_ws(ws, ws_bytes, "dvm_softcorr_fwd_f32", w, carve_k1_norms, B, N, M, false, variant == 3)) return DVM_ENOSPACE;
    float *const n1 = w.n1, *const n2 = w.n2;
    hipStream_t s = (hipStream_t)stream;
    if (variant == 3) {
        const K1SoftOut out{pi_val, pi_idx, row_smax, row_sum};
        int rc = launch_softcorr_f16(K1Sides{{f1, f2}, {n1, n2}, B, {N, M}, false}, &out, neg_alpha, topk, K1_PREP_TWO_PASS, w.k1ws, w.k1_bytes, s);
        if (rc != DVM_OK) return rc;
        DVM_CHECK_LAUNCH("softcorr (fp16)");
        return DVM_OK;
    }
    launch_rownorm2(f1, B * N, d, n1, s);
    launch_rownorm2(f2, B * M, d, n2, s);
    bool mfma = (variant == 2) || (variant == 0 && d == D);
    prof_note(DVM_PROF_K1_SWEEP, mfma ? "softcorr_mfma_kernel" : "softcorr_scalar_kernel");
    prof_begin(s);
    if (mfma) {
        SCArgs a;
        a.g[0] = SCGroup{f1, f2, n1, n2, N, M, (N + SW_QB - 1) / SW_QB, pi_val, pi_idx, row_smax, row_sum};
        a.g[1] = a.g[0];
        a.blocks0 = B * a.g[0].tiles;
        a.neg_alpha = neg_alpha;
        a.topk = topk;
        if (topk <= 10)
            launch_softcorr_mfma<10>(a, a.blocks0, s);
        else
            launch_softcorr_mfma<16>(a, a.blocks0, s);
    } else {
        dim3 grid((N + 127) / 128, B);
        size_t lds = scalar_sweep_lds_bytes(d, 0);
        ensure_dyn_lds((const void *)softcorr_scalar_kernel<10>, 66 * 1024);
        ensure_dyn_lds((const void *)softcorr_scalar_kernel<16>, 66 * 1024);
        if (topk <= 10)
            hipLaunchKernelGGL(softcorr_scalar_kernel<10>, grid, dim3(128), lds, s, f1, f2, n1, n2, N, M, d, neg_alpha, topk,
                               pi_val, pi_idx, row_smax, row_sum);
        else
            hipLaunchKernelGGL(softcorr_scalar_kernel<16>, grid, dim3(128), lds, s, f1, f2, n1, n2, N, M, d, neg_alpha, topk,
                               pi_val, pi_idx, row_smax, row_sum);
    }
    prof_end(s);
    DVM_CHECK_LAUNCH("softcorr");
    return DVM_OK;
}

// dvm_softcorr_fwd_f32's workspace in front (its norms are read again here), then the row statistics and the top-1 outputs
struct SoftcorrDenseWs {
    K1NormsWs sc;
    size_t sc_bytes;
    float *smax, *ssum, *v1;
    int32_t *i1;
};
static size_t carve_softcorr_dense(Arena &ar, int B, int N, int M, int d, SoftcorrDenseWs &w) {
    w.sc_bytes = carve_k1_norms(ar, B, N, M, false, d == D, w.sc);   // (first in the arena: its end offset is its size)
    w.smax = ar.take<float>((size_t)B * N), w.ssum = ar.take<float>((size_t)B * N);
    w.v1 = ar.take<float>((size_t)B * N);
    w.i1 = ar.take<int32_t>((size_t)B * N);
    return ar.off;
}
DVM_EXPORT size_t dvm_softcorr_dense_workspace_bytes(int B, int N, int M, int d) {
    return null_carve<SoftcorrDenseWs>(carve_softcorr_dense, B, N, M, d);
}

DVM_EXPORT int dvm_softcorr_dense_f32(const float *f1, const float *f2, int B, int N, int M, int d, float neg_alpha, float *P,
                                      void *ws, size_t ws_bytes, void *stream) {
    DVM_REQUIRE(f1 && f2 && P, "dvm_softcorr_dense_f32: null pointer");
    DVM_REQUIRE(B >= 1 && N >= 1 && M >= 1, "dvm_softcorr_dense_f32: empty input");
    DVM_REQUIRE(d >= 4 && d % 4 == 0 && d <= 512, "dvm_softcorr_dense_f32: d=%d unsupported", d);
    DVM_REQUIRE(neg_alpha < 0.f, "dvm_softcorr_dense_f32: neg_alpha must be negative");
    SoftcorrDenseWs w;
    if (!carve_ws(ws, ws_bytes, "dvm_softcorr_dense_f32", w, carve_softcorr_dense, B, N, M, d)) return DVM_ENOSPACE;
    float *const smax = w.smax, *const ssum = w.ssum;
    // (the soft-correspondence call carves the head of `ws` as carve_k1_norms did here: its norms are w.sc.n1 / n2)
    int rc = dvm_softcorr_fwd_f32(f1, f2, B, N, M, d, neg_alpha, 1, w.v1, w.i1, smax, ssum, 0, ws, w.sc_bytes, stream);
    if (rc != DVM_OK) return rc;
    const float *n1 = w.sc.n1, *n2 = w.sc.n2;
    size_t lds = scalar_sweep_lds_bytes(d, 0);
    (void)hipFuncSetAttribute((const void *)softcorr_dense_kernel<0>, hipFuncAttributeMaxDynamicSharedMemorySize, 66 * 1024);
    hipLaunchKernelGGL(softcorr_dense_kernel<0>, dim3((N + 127) / 128, B), dim3(128), lds, (hipStream_t)stream, f1, f2, n1, n2, smax,
                       ssum, N, M, d, neg_alpha, P);
    DVM_CHECK_LAUNCH("softcorr_dense");
    return DVM_OK;
}

