// dvm_softcorr_passb.hip — K1 behind pass A (dvm_softcorr_f16.h): the routing probe in front of it, pass B (the exact re-evaluation
// of the candidate lists), the gate behind the coarse screen, and the exact recompute of the rows pass B could not certify.
#include "dvm_softcorr_f16.h"

namespace dvm {
namespace {

using namespace k1;

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

// the two directions' groups: direction d has side d as queries and side d ^ 1 as keys (without `both`, group 1 repeats group 0)
static HRArgs hr_args(const K1Sides &c, const K1SoftOut *out, const K1Ws &w, float neg_alpha, int topk, const int *route) {
    HRArgs r;
    for (int g = 0; g < 2; ++g) {
        const int d = c.both ? g : 0, k = d ^ 1;
        r.g[g] = HRGroup{c.f[d], c.f[k], c.n[d], c.n[k], w.nmax[k], c.rows[d], c.rows[k], w.cidx[d], w.cd2[d], w.lsum[d],
                         out[d].val, out[d].idx, out[d].smax, out[d].sum, w.flag[d] + 1, w.flag[d]};
    }
    r.rows0 = c.total(0);
    r.rows_total = r.rows0 + (c.both ? c.total(1) : 0);
    r.neg_alpha = neg_alpha;
    r.cutw = 20.f / -neg_alpha;
    r.topk = topk;
    r.route = route;
    r.nb = c.B;
    return r;
}

}  // namespace

void k1::launch_probe(const K1Sides &c, const K1Ws &w, float neg_alpha, bool have_coarse, hipStream_t s) {
    const Options &pol = options();
    const K1ProbeArgs pa{{c.f[0], c.f[1]}, {c.n[0], c.n[1]}, {c.rows[0], c.rows[1]}, 20.f / -neg_alpha, pol.k1_p_coarse, pol.k1_p_lean,
                         have_coarse, w.route, w.pfrac};
    hipLaunchKernelGGL(k1_probe_kernel, dim3(c.B, c.dirs()), dim3(256), 0, s, pa);
    hipLaunchKernelGGL(k1_route_kernel, dim3(c.dirs()), dim3(256), 0, s, pa, c.B);
}

void k1::launch_refine(const K1Sides &c, const K1SoftOut *out, const K1Ws &w, const K1Plan &p, float neg_alpha, int topk, bool second,
                       hipStream_t s) {
    const HRArgs r = hr_args(c, out, w, neg_alpha, topk, second ? w.route2 : p.route(w));
    // (window 3: 112 VGPRs, 4 waves per SIMD, 1.11 ms per launch of the bench; window 2: 96, 5 waves, 1.17 ms)
    if (second) {
        hipLaunchKernelGGL((softcorr_refine_gated_kernel<HB_KC, 3>), dim3(4096), dim3(256), 0, s, r);
        return;
    }
    const dim3 grid((unsigned)((hr_quads(r) * 64 + 255) / 256));
    if (p.routed && p.coarse) hipLaunchKernelGGL((softcorr_refine_routed_kernel<3>), grid, dim3(256), 0, s, r);
    else if (p.coarse) hipLaunchKernelGGL((softcorr_refine_kernel<K1_KC_COARSE, true, 3>), grid, dim3(256), 0, s, r);
    else hipLaunchKernelGGL((softcorr_refine_kernel<HB_KC, false, 3>), grid, dim3(256), 0, s, r);
    if (!p.coarse) return;
    const K1GateArgs ga{p.route(w), w.route2, {w.flag[0], w.flag[c.both ? 1 : 0]}, {c.total(0), c.total(1)}, c.dirs(), c.B};
    hipLaunchKernelGGL(k1_gate_kernel, dim3(1), dim3(256), 0, s, ga);
}

void k1::launch_exact_rows(const K1Sides &c, const K1SoftOut *out, const K1Ws &w, float neg_alpha, int topk, hipStream_t s) {
    HXArgs x{};   // (without `both`, group 1 is empty)
    for (int d = 0; d < c.dirs(); ++d)
        x.g[d] = HXGroup{c.f[d], c.f[d ^ 1], c.n[d], c.n[d ^ 1], c.rows[d], c.rows[d ^ 1], out[d].val, out[d].idx, out[d].smax, out[d].sum,
                         w.flag[d] + 1, w.flag[d]};
    x.neg_alpha = neg_alpha;
    x.topk = topk;
    if (options().debug & DVM_DEBUG_K1_FLAGGED) {   // diagnostic (synchronous): rows pass B could not certify
        int n[2] = {0, 0};
        (void)hipStreamSynchronize(s);
        for (int d = 0; d < c.dirs(); ++d) (void)hipMemcpy(&n[d], w.flag[d], sizeof(int), hipMemcpyDeviceToHost);
        fprintf(stderr, "K1 pass B: %d + %d of %ld rows go through the exact-rows kernel\n", n[0], n[1], c.total(0) + (c.both ? c.total(1) : 0));
    }
    ensure_dyn_lds((const void *)softcorr_exact_rows_kernel, 256 * HX_LD * (int)sizeof(float));
    hipLaunchKernelGGL(softcorr_exact_rows_kernel, dim3(512), dim3(HX_T), 256 * HX_LD * sizeof(float), s, x);
}

}  // namespace dvm
