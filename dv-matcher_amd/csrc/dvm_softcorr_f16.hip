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
// This file: the first form of pass A (three products; full, lean, routed and gated kernels) and its launcher.
#include "dvm_softcorr_f16.h"

namespace dvm {
namespace {

using namespace k1;

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

}  // namespace

void k1::launch_sweep_f16(const HBArgs &a, int blocks, int form, hipStream_t s) {
    auto go = [&](auto kernel, int grid, auto... more) {
        ensure_dyn_lds((const void *)kernel, (int)HB_LDS_BYTES);
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(HB_THREADS), HB_LDS_BYTES, s, a, more...);
    };
    if (form == K1_SWEEP_ROUTED) go(softcorr_sweep_f16_routed_kernel, blocks);
    else if (form == K1_SWEEP_GATED) go(softcorr_sweep_f16_gated_kernel, blocks < 2048 ? blocks : 2048, blocks);
    else if (form == K1_ROUTE_LEAN) go(softcorr_sweep_f16_kernel<true>, blocks);
    else go(softcorr_sweep_f16_kernel<false>, blocks);
}

}  // namespace dvm
