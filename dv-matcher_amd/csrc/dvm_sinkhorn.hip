// dvm_sinkhorn.hip — Sinkhorn-normalised soft correspondence, forward, sparse top-k.
//
// NOT in the reference (the reference has a row softmax only).  With S_ij = cdist(f1, f2)_ij * neg_alpha,
// formed exactly as dvm_softcorr_fwd_f32 forms it, the operator alternates
//     u_i = -LSE_j(S_ij + v_j)                (rows of P = exp(S + u + v) sum to 1)
//     v_j = log(N / M) - LSE_i(S_ij + u_i)    (columns sum to N / M)
// n_iter times from v = 0 and ends with a row step that also keeps the top-k of L_ij = S_ij + v_j per row.  n_iter = 0
// is the reference's operator (v = 0, one row softmax): that case is pinned to dvm_softcorr_fwd_f32, which is pinned to
// the reference.
//
// One kernel does every step: a workgroup owns 256 "query" rows and streams all "key" rows through the distance tile of
// dvm_dist_tile.h (layout, chain, geometry, row frame and sweep loops are defined there; the top-k list's half-lane merge
// and flagged-candidate loop next to KBest in dvm_common.h) together with the keys' |.|^2 and potential, and keeps
// an online (max, sum) of L per query row in registers.  The row step is (queries, keys, potential) = (f1, f2, v), the
// column step the same kernel with (f2, f1, u): every potential is owned by one lane pair, so there are no float atomics
// and two runs give the same bits.  The N x M matrix is never written to HBM; the potentials (4 (N + M) bytes per entry)
// live in L2.
//
// Every candidate takes the exact path (correctly rounded sqrt, s = d * neg_alpha, L = s + v): the potentials are
// compared against a float64 evaluation at a few fp32 roundings of max |S|, which leaves no room for the 1-ulp hardware
// sqrt under alpha = 100.  The running sum is kept in fp64 (one add per 16 candidates), so that its error does not grow
// with the number of key tiles.
//
// dvm_sinkhorn_fwd_hist_f32 is the same run with every iterate's potentials left in memory (u_hist, v_hist) for the
// backward, dvm_sinkhorn_bwd.hip: only the destination of each sweep's output changes.
//
// dvm_sinkhorn_ub_fwd_f32 / dvm_sinkhorn_ub_fwd_hist_f32 are the unbalanced (KL-relaxed) operator of include/dvm.h on the same
// sweeps: a potential sweep leaves tau * (log weight + normaliser) where the balanced one leaves add - LSE, the final sweep
// scales the values by the row's mass exp(u^f - m^f) and writes its logarithm.  The history of that form keeps the
// normalisers m^t, n^t; a potential is re-made from one wherever it is needed as tau * (log weight + normaliser), a sum, then a
// product (this file is compiled without contraction), so that the forward and the backward hold the same bits.
#include <float.h>
#include <math.h>

#include "dvm_dist_tile.h"

namespace dvm {
namespace {

using namespace dtile;

// running (max, sum exp(. - max)) of one row
struct LseState {
    float m;    // running max of L (-inf initially)
    double l;   // sum exp(L - m)
    __device__ __forceinline__ void init() {
        m = -INFINITY;
        l = 0.0;
    }
    __device__ __forceinline__ void rescale(float new_m) {
        if (new_m > m) {
            l = l * (double)__builtin_amdgcn_exp2f((m - new_m) * LOG2E);   // m = -inf, l = 0 -> 0 * 0
            m = new_m;
        }
    }
    // the shift the terms are taken against: finite even while every L seen so far is -inf (padding columns only), so that
    // L - shift is -inf and the term 0 instead of (-inf) - (-inf)
    __device__ __forceinline__ float shift() const { return fmaxf(m, -FLT_MAX); }
    __device__ __forceinline__ void merge(float om, double ol) {
        const float mm = fmaxf(m, om);
        const double a = (m == -INFINITY) ? 0.0 : l * (double)exp2f((m - mm) * LOG2E);
        const double b = (om == -INFINITY) ? 0.0 : ol * (double)exp2f((om - mm) * LOG2E);
        l = a + b;
        m = mm;
    }
};

// top-k list of a final row sweep.  With a potential the key is -L (ascending = descending logit, ties -> lowest column);
// without one (n_iter = 0: L = d * neg_alpha, a monotone function of d) the key is the distance itself, as
// dvm_softcorr_fwd_f32 ranks — two distances that round to one logit stay in distance order, which is what that
// operator returns.
template <int TOPK>
__device__ __forceinline__ void store_final(const KBest<TOPK, float> &kb, bool hasv, const LseState &st, int topk, int M, float neg_alpha,
                                            float *val, int32_t *idx, float *row_lmax, float *row_sum, float *u, bool relaxed,
                                            float tau, float logw, float *nrm, float *row_lmass) {
    const float lmax = hasv ? -kb.key[0] : kb.key[0] * neg_alpha;   // = st.m: every candidate went through the same L
    const float lsum = (float)st.l;
    const float mf = -(lmax + logf(lsum));
    // relaxed: u^f = tau (log_a + m^f), the row's mass exp(u^f - m^f) on every value (0, never NaN, where it underflows)
    const float uf = relaxed ? tau * (logw + mf) : mf;
    const float lmass = relaxed ? uf - mf : 0.f;
    const float inv = relaxed ? (1.0f / lsum) * exp2f(lmass * LOG2E) : 1.0f / lsum;
#pragma unroll
    for (int t = 0; t < TOPK; ++t) {
        if (t < topk) {
            const bool live = t < M;
            const float L = hasv ? -kb.key[t] : kb.key[t] * neg_alpha;
            val[t] = live ? exp2f((L - lmax) * LOG2E) * inv : 0.f;
            idx[t] = live ? kb.idx[t] : 0;
        }
    }
    if (row_lmax) *row_lmax = lmax;
    if (row_sum) *row_sum = lsum;
    if (u) *u = uf;
    if (nrm) *nrm = mf;
    if (row_lmass) *row_lmass = lmass;
}

struct SKArgs {
    const float *q, *k;     // queries [B][N][d], keys [B][M][d]
    const float *nq, *nk;   // their |.|^2
    const float *pot;       // the keys' potential, entry b at pot + b * pot_bs; NULL = 0
    long pot_bs, out_bs;    // batch strides (floats) of pot and of out / u: M and N, or a slice of a potential history
    int N, M, d, tiles;     // tiles = query blocks per entry
    float neg_alpha;
    float add;              // potential sweep: out = tau * (add - LSE) (0 for the row step, log(N / M) for the column step)
    float tau;              // 1 in the balanced operator
    const float *logw;      // the queries' log weight [B][N] in place of add; NULL = add
    float *out;             // potential sweep: the queries' new potential [B][N]
    float *nrm;             // the queries' normaliser -LSE, entry b at nrm + b * nrm_bs; NULL = not kept
    long nrm_bs;
    bool relaxed;           // final row sweep: tau / logw apply (u^f = tau (logw + m^f), values scaled by the row's mass)
    float *lmass;           // final row sweep: log of the row's mass [B][N]; may be NULL
    int topk;               // final row sweep
    float *val;
    int32_t *idx;
    float *lmax, *sum, *u;
};

// a potential sweep's result for query i of entry b (row = b * N + i): the normaliser -LSE, kept if asked for, and the
// potential tau * (log weight + normaliser) — with tau = 1 and no weights the balanced add - LSE, bit for bit
__device__ __forceinline__ void store_potential(const SKArgs &a, int b, int i, size_t row, const LseState &st) {
    const float nrm = -(st.m + logf((float)st.l));
    const float w = a.logw ? a.logw[row] : a.add;
    if (a.nrm) a.nrm[(size_t)b * a.nrm_bs + i] = nrm;
    a.out[(size_t)b * a.out_bs + i] = a.tau * (w + nrm);
}

// ------------------------------------------------------------ scalar variant
// One thread per query row (the scalar sweep of dvm_dist_tile.h).  Any d % 4 == 0.  The cross-check form of the
// matrix-core kernel and the path for d != 128; not tuned.  SWAP: the queries are f2 (column step), see sqdist.
template <bool FINAL, bool SWAP, int TOPK>
__global__ __launch_bounds__(128) void sinkhorn_scalar_kernel(const SKArgs a) {
    // one sidecar plane: the keys' potentials
    const int N = a.N, M = a.M;
    const ScalarFrame f = scalar_frame(a.q, a.nq, N, a.d);
    const int b = f.b, i = f.i;
    const float na = f.na;
    const bool hasv = a.pot != nullptr;
    const float neg_alpha = a.neg_alpha;
    LseState st;
    st.init();
    KBest<TOPK, float> kb;
    if (FINAL) kb.init(INFINITY);
    scalar_sweep(
        f, a.k, a.nk, M, a.d, [&](int j, bool in, float *side) { side[SC_KT] = (in && hasv) ? a.pot[(size_t)b * a.pot_bs + j] : 0.f; },
        [&](int j0, const float (&acc)[SC_KT], const float *kn) {
            const float *kp = kn + SC_KT;
            float Lv[SC_KT], dv[SC_KT];
            float tmax = -INFINITY;
#pragma unroll
            for (int j = 0; j < SC_KT; ++j) {
                dv[j] = sqrt_rn(sqdist<SWAP>(acc[j], na, kn[j]));
                Lv[j] = dv[j] * neg_alpha + kp[j];
                tmax = fmaxf(tmax, Lv[j]);
            }
            st.rescale(tmax);
            const float sh = st.shift();
            float ls = 0.f;
#pragma unroll
            for (int j = 0; j < SC_KT; ++j) {
                ls += __builtin_amdgcn_exp2f((Lv[j] - sh) * LOG2E);
                if (FINAL) kb.insert(hasv ? -Lv[j] : dv[j], j0 + j);
            }
            st.l += (double)ls;
        });
    if (i < N) {
        const size_t row = (size_t)b * N + i;
        if (FINAL)
            store_final<TOPK>(kb, hasv, st, a.topk, M, neg_alpha, a.val + row * a.topk, a.idx + row * a.topk,
                              a.lmax ? a.lmax + row : nullptr, a.sum ? a.sum + row : nullptr,
                              a.u ? a.u + (size_t)b * a.out_bs + i : nullptr, a.relaxed, a.tau, a.logw ? a.logw[row] : 0.f,
                              a.nrm ? a.nrm + (size_t)b * a.nrm_bs + i : nullptr, a.lmass ? a.lmass + row : nullptr);
        else
            store_potential(a, b, i, row, st);
    }
}

// -------------------------------------------------------------- matrix-core variant (d == 128)
// Tile, LDS layout, geometry and the two-role phase structure: dvm_dist_tile.h.  The online (max, sum) and the top-k list
// need no cross-lane traffic until the two half-lanes of a query merge at the end.
constexpr int SK_TILE_FLOATS = ROWS_FLOATS + 2 * KT;        // keys + their norms + their potentials
constexpr size_t SK_LDS_BYTES = (size_t)2 * SK_TILE_FLOATS * sizeof(float);
// final row sweep: + per wave the staging block of this sub-tile's 16 ranking keys of each lane
constexpr size_t SK_LDS_BYTES_FINAL = SK_LDS_BYTES + (size_t)SW_WAVES * SW_STAGE * sizeof(float);

// FINAL: the last row sweep (top-k, pi_val / pi_idx / row_lmax / row_sum / u); HASV (FINAL only): rank by -L, else by d.
template <bool FINAL, bool HASV, bool SWAP, int TOPK>
__global__ __launch_bounds__(SW_THREADS, 2) void sinkhorn_mfma_kernel(const SKArgs a) {
    // [2] x { [KT][LDK] keys, [KT] norms, [KT] potentials }; FINAL: + [SW_WAVES][16][64] ranking keys
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float *const stage = smem + 2 * SK_TILE_FLOATS + (threadIdx.x >> 6) * SW_STAGE + (threadIdx.x & 63);   // this lane's column

    const int N = a.N, M = a.M;
    const float neg_alpha = a.neg_alpha;
    RowFrame f;   // this lane's query row
    row_frame(f, a.tiles, N, a.q, a.nq);
    const int b = f.b, tid = f.tid, r32 = f.r32, h = f.h, qrow = f.row;
    const float na = f.nrm;

    const float *kbase = a.k + (size_t)b * M * D;
    const float *knb = a.nk + (size_t)b * M;
    const float *kpb = a.pot ? a.pot + (size_t)b * a.pot_bs : nullptr;

    LseState st;
    st.init();
    KBest<TOPK, float> kb;
    if (FINAL) kb.init(INFINITY);

    const int ntiles = (M + KT - 1) / KT;
    f32x4 pre[SW_LD_PER_THREAD];
    float pren = 0.f;   // threads 0..63: a key's norm; threads 64..127: a key's potential

    auto issue_loads = [&](int t) {
        const int j0 = t * KT;
        issue_tile<SW_THREADS>(kbase, j0, M, tid, pre);
        if (tid < KT)
            pren = (j0 + tid < M) ? knb[j0 + tid] : INFINITY;
        else if (tid < 2 * KT)
            pren = (kpb && j0 + tid - KT < M) ? kpb[j0 + tid - KT] : 0.f;
    };
    auto commit_loads = [&](int buf) {
        float *kt = smem + buf * SK_TILE_FLOATS;
        commit_tile<SW_THREADS>(kt, tid, pre);
        if (tid < 2 * KT) kt[ROWS_FLOATS + tid] = pren;   // norms, then potentials
    };

    // the chain, |key|^2 and potential of this lane's 16 keys
    f32x16 acc;
    float nbv[16], pv[16];
    auto mfma_chain = [&](int buf, int sub) {
        const float *kt = smem + buf * SK_TILE_FLOATS;
        dist_chain(kt, sub, r32, h, f.q, acc);
        lane_scalars(kt + ROWS_FLOATS, sub, h, nbv);
        lane_scalars(kt + ROWS_FLOATS + KT, sub, h, pv);
    };

    auto epilogue = [&](int t, int sub) {
        float Lv[16];
        unsigned mask = 0;
        const float worst = FINAL ? kb.key[TOPK - 1] : 0.f;
        float tmax = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float de = sqrt_rn(sqdist<SWAP>(acc[r], na, nbv[r]));   // +inf for padding keys
            const float L = de * neg_alpha + pv[r];   // (-ffp-contract=off: a product, then a sum)
            Lv[r] = L;
            if (FINAL) {   // the ranking keys are parked in LDS ([r][lane], conflict-free) for the dynamic pick below
                const float key = HASV ? -L : de;
                stage[r * 64] = key;
                mask |= (key < worst) ? (1u << r) : 0u;
            }
            tmax = fmaxf(tmax, L);
        }
        st.rescale(tmax);
        const float sh = st.shift();
        float ls = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) ls += __builtin_amdgcn_exp2f((Lv[r] - sh) * LOG2E);
        st.l += (double)ls;
        if (FINAL) {
            // candidates that beat this lane's current worst, in ascending column order
            for_each_flagged(mask, stage, [&](bool act, int bpos, float key) {
                kb.insert_nb(act ? key : INFINITY, t * KT + sub * 32 + lane_key(bpos, h));
            });
        }
    };

    // the 16-entry list leaves no room for the next tile's 32 prefetch registers next to it: that variant loads the tile after
    // its epilogues (the other wave of the SIMD covers the latency) instead of spilling
    constexpr bool LATE_LOADS = FINAL && TOPK > 10;
    const int role = __builtin_amdgcn_readfirstlane(f.wave >> 2);
    two_role_sweep<LATE_LOADS>(ntiles, role, issue_loads, commit_loads, mfma_chain, epilogue);

    // merge the two half-lanes that share a query (lane, lane ^ 32); the lower lane writes the row
    {
        const float om = __shfl_xor(st.m, 32, 64);
        const double ol = __shfl_xor(st.l, 32, 64);
        st.merge(om, ol);
    }
    if (FINAL) merge_halves(kb);
    if (h == 0 && qrow < N) {
        const size_t row = (size_t)b * N + qrow;
        if (FINAL)
            store_final<TOPK>(kb, HASV, st, a.topk, M, neg_alpha, a.val + row * a.topk, a.idx + row * a.topk,
                              a.lmax ? a.lmax + row : nullptr, a.sum ? a.sum + row : nullptr,
                              a.u ? a.u + (size_t)b * a.out_bs + qrow : nullptr, a.relaxed, a.tau, a.logw ? a.logw[row] : 0.f,
                              a.nrm ? a.nrm + (size_t)b * a.nrm_bs + qrow : nullptr, a.lmass ? a.lmass + row : nullptr);
        else
            store_potential(a, b, qrow, row, st);
    }
}

template <bool FINAL, bool HASV, bool SWAP, int TOPK>
void launch_mfma(const SKArgs &a, int B, hipStream_t s) {
    const size_t lds = FINAL ? SK_LDS_BYTES_FINAL : SK_LDS_BYTES;
    ensure_dyn_lds((const void *)sinkhorn_mfma_kernel<FINAL, HASV, SWAP, TOPK>, (int)lds);
    hipLaunchKernelGGL((sinkhorn_mfma_kernel<FINAL, HASV, SWAP, TOPK>), dim3((unsigned)(B * a.tiles)), dim3(SW_THREADS), lds, s, a);
}

template <bool FINAL, bool SWAP, int TOPK>
void launch_scalar(const SKArgs &a, int B, hipStream_t s) {
    const size_t lds = scalar_sweep_lds_bytes(a.d, 1);
    ensure_dyn_lds((const void *)sinkhorn_scalar_kernel<FINAL, SWAP, TOPK>, 66 * 1024);
    hipLaunchKernelGGL((sinkhorn_scalar_kernel<FINAL, SWAP, TOPK>), dim3((a.N + 127) / 128, B), dim3(128), lds, s, a);
}

// one potential sweep: out [B][Nq] = add - LSE_keys(S + pot)
void launch_sweep(bool mfma, bool swap, SKArgs a, int B, hipStream_t s) {
    if (mfma) {
        a.tiles = (a.N + SW_QB - 1) / SW_QB;
        if (swap)
            launch_mfma<false, true, true, 1>(a, B, s);
        else
            launch_mfma<false, true, false, 1>(a, B, s);
    } else {
        if (swap)
            launch_scalar<false, true, 1>(a, B, s);
        else
            launch_scalar<false, false, 1>(a, B, s);
    }
}

template <int TOPK>
void launch_final(bool mfma, SKArgs a, int B, hipStream_t s) {
    if (mfma) {
        a.tiles = (a.N + SW_QB - 1) / SW_QB;
        if (a.pot)
            launch_mfma<true, true, false, TOPK>(a, B, s);
        else
            launch_mfma<true, false, false, TOPK>(a, B, s);
    } else {
        launch_scalar<true, false, TOPK>(a, B, s);
    }
}

__global__ void sinkhorn_zero_slice_kernel(float *p, int n, long bs) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[(size_t)blockIdx.y * bs + i] = 0.f;
}

// The whole operator.  Iterate t = 1..n_iter reads v^(t-1) at V + (t-1) * v_step and writes u^t to U + (t-1) * u_step and
// v^t to V + t * v_step (batch strides u_bs / v_bs); the final row step reads v^T and writes its u to uf (batch stride
// u_bs, may be NULL).  dvm_sinkhorn_fwd_f32 runs it with steps 0 (one buffer per side), dvm_sinkhorn_fwd_hist_f32 with a
// history slice per iterate: the same kernels on the same operands, so the same bits.
// The unbalanced entries pass a Relax: the factors and log weights of the two sides, row_lmass, and (history form) where the
// normalisers go — m^t to RN + (t-1) * N, m^f to RN + T * N, n^t to CN + t * M, batch strides (T + 1) N and (T + 1) M.
struct Relax {
    float tau_row, tau_col;
    const float *log_a, *log_b;
    float *row_lmass, *RN, *CN;
};
int sinkhorn_run(const float *f1, const float *f2, int B, int N, int M, int d, float neg_alpha, int n_iter, int topk, float *pi_val,
                 int32_t *pi_idx, float *row_lmax, float *row_sum, float *n1, float *n2, float *U, long u_step, long u_bs, float *V,
                 long v_step, long v_bs, float *uf, bool mfma, hipStream_t s, const Relax *rx = nullptr) {
    launch_rownorm2(f1, B * N, d, n1, s);
    launch_rownorm2(f2, B * M, d, n2, s);
    const float log_ratio = (float)log((double)N / (double)M);
    SKArgs row{}, col{};
    row.q = f1, row.k = f2, row.nq = n1, row.nk = n2, row.N = N, row.M = M, row.d = d, row.neg_alpha = neg_alpha;
    col.q = f2, col.k = f1, col.nq = n2, col.nk = n1, col.N = M, col.M = N, col.d = d, col.neg_alpha = neg_alpha;
    row.pot_bs = v_bs, row.out_bs = u_bs, col.pot_bs = u_bs, col.out_bs = v_bs;
    row.tau = col.tau = 1.f;
    row.add = 0.f, col.add = log_ratio;
    if (rx) {
        row.tau = rx->tau_row, col.tau = rx->tau_col, row.logw = rx->log_a, col.logw = rx->log_b;
        row.nrm_bs = (long)(n_iter + 1) * N, col.nrm_bs = (long)(n_iter + 1) * M;
    }
    for (int it = 0; it < n_iter; ++it) {
        row.pot = it ? V + it * v_step : nullptr;   // v = 0 before the first row step: nothing is read from the buffer
        row.out = U + it * u_step;
        row.nrm = rx && rx->RN ? rx->RN + (size_t)it * N : nullptr;
        launch_sweep(mfma, false, row, B, s);
        col.pot = row.out;
        col.out = V + (it + 1) * v_step;
        col.nrm = rx && rx->CN ? rx->CN + (size_t)(it + 1) * M : nullptr;
        launch_sweep(mfma, true, col, B, s);
    }
    row.pot = n_iter ? V + n_iter * v_step : nullptr;
    row.out = nullptr;
    row.nrm = rx && rx->RN ? rx->RN + (size_t)n_iter * N : nullptr;
    // (tau_row = 1 without row weights is the balanced row step: u^f = m^f, mass 1, row_lmass 0)
    row.relaxed = rx && (rx->tau_row != 1.f || rx->log_a), row.lmass = rx ? rx->row_lmass : nullptr;
    row.topk = topk, row.val = pi_val, row.idx = pi_idx, row.lmax = row_lmax, row.sum = row_sum, row.u = uf;
    if (topk <= 10)
        launch_final<10>(mfma, row, B, s);
    else
        launch_final<16>(mfma, row, B, s);
    DVM_CHECK_LAUNCH("sinkhorn");
    return DVM_OK;
}

}  // namespace
}  // namespace dvm

using namespace dvm;

// |f1|^2, |f2|^2 (both entry points) and, with `potentials`, u and v (used when the caller does not ask for them; the hist form
// writes the caller's histories instead)
struct SinkhornWs {
    float *n1, *n2, *wu, *wv;
};
static size_t carve_sinkhorn(Arena &ar, int B, int N, int M, bool potentials, SinkhornWs &w) {
    w.n1 = ar.take<float>((size_t)B * N);
    w.n2 = ar.take<float>((size_t)B * M);
    w.wu = potentials ? ar.take<float>((size_t)B * N) : nullptr;
    w.wv = potentials ? ar.take<float>((size_t)B * M) : nullptr;
    return ar.off;
}

DVM_EXPORT size_t dvm_sinkhorn_workspace_bytes(int B, int N, int M, int d) {
    (void)d;
    if (B < 1 || N < 1 || M < 1) return 0;
    return null_carve<SinkhornWs>(carve_sinkhorn, B, N, M, true);
}

DVM_EXPORT int dvm_sinkhorn_fwd_f32(const float *f1, const float *f2, int B, int N, int M, int d, float neg_alpha, int n_iter,
                                    int topk, float *pi_val, int32_t *pi_idx, float *row_lmax, float *row_sum, float *u, float *v,
                                    int variant, void *ws, size_t ws_bytes, void *stream) {
    const int rc = softcorr_family_check("dvm_sinkhorn_fwd_f32", f1 && f2 && pi_val && pi_idx, B, N, M, d, topk, neg_alpha, variant, 1, n_iter);
    if (rc != DVM_OK) return rc;
    SinkhornWs w;
    if (!carve_ws(ws, ws_bytes, "dvm_sinkhorn_fwd_f32", w, carve_sinkhorn, B, N, M, true)) return DVM_ENOSPACE;
    hipStream_t s = (hipStream_t)stream;
    float *ub = u ? u : w.wu, *vb = v ? v : w.wv;
    const bool mfma = variant == 0 && d == D;
    if (n_iter == 0 && v) (void)hipMemsetAsync(v, 0, (size_t)B * M * sizeof(float), s);
    return sinkhorn_run(f1, f2, B, N, M, d, neg_alpha, n_iter, topk, pi_val, pi_idx, row_lmax, row_sum, w.n1, w.n2, ub, 0, N, vb, 0, M, u,
                        mfma, s);
}

DVM_EXPORT size_t dvm_sinkhorn_hist_workspace_bytes(int B, int N, int M, int d) {
    (void)d;
    if (B < 1 || N < 1 || M < 1) return 0;
    return null_carve<SinkhornWs>(carve_sinkhorn, B, N, M, false);
}

DVM_EXPORT int dvm_sinkhorn_fwd_hist_f32(const float *f1, const float *f2, int B, int N, int M, int d, float neg_alpha, int n_iter,
                                         int topk, float *pi_val, int32_t *pi_idx, float *row_lmax, float *row_sum, float *u_hist,
                                         float *v_hist, int variant, void *ws, size_t ws_bytes, void *stream) {
    const int rc = softcorr_family_check("dvm_sinkhorn_fwd_hist_f32", f1 && f2 && pi_val && pi_idx && u_hist && v_hist, B, N, M, d, topk,
                                         neg_alpha, variant, 1, n_iter);
    if (rc != DVM_OK) return rc;
    SinkhornWs w;
    if (!carve_ws(ws, ws_bytes, "dvm_sinkhorn_fwd_hist_f32", w, carve_sinkhorn, B, N, M, false)) return DVM_ENOSPACE;
    hipStream_t s = (hipStream_t)stream;
    const long u_bs = (long)(n_iter + 1) * N, v_bs = (long)(n_iter + 1) * M;
    hipLaunchKernelGGL(sinkhorn_zero_slice_kernel, dim3((M + 255) / 256, B), dim3(256), 0, s, v_hist, M, v_bs);   // v^0
    return sinkhorn_run(f1, f2, B, N, M, d, neg_alpha, n_iter, topk, pi_val, pi_idx, row_lmax, row_sum, w.n1, w.n2, u_hist, N, u_bs, v_hist,
                        M, v_bs, u_hist + (size_t)n_iter * N, variant == 0 && d == D, s);
}

// ---------------------------------------------------------------------------------------- unbalanced (KL-relaxed) entries
// the argument checks the two entries share: the family's, with the tau pair (tested after neg_alpha, before variant)
static int sinkhorn_ub_check(const char *who, const void *f1, const void *f2, const void *pi_val, const void *pi_idx, int B, int N, int M, int d,
                             float neg_alpha, int n_iter, int topk, float tau_row, float tau_col, int variant) {
    return softcorr_family_check(who, f1 && f2 && pi_val && pi_idx, B, N, M, d, topk, neg_alpha, variant, 1, n_iter, -1, tau_row, tau_col);
}

// both entries: |f1|^2, |f2|^2 and the current potentials of the two sides (the caller's u / v where given)
static size_t carve_sinkhorn_ub(Arena &ar, int B, int N, int M, SinkhornWs &w) { return carve_sinkhorn(ar, B, N, M, true, w); }

DVM_EXPORT size_t dvm_sinkhorn_ub_workspace_bytes(int B, int N, int M, int d) {
    (void)d;
    if (B < 1 || N < 1 || M < 1) return 0;
    return null_carve<SinkhornWs>(carve_sinkhorn_ub, B, N, M);
}

DVM_EXPORT int dvm_sinkhorn_ub_fwd_f32(const float *f1, const float *f2, int B, int N, int M, int d, float neg_alpha, int n_iter, int topk,
                                       float tau_row, float tau_col, const float *log_a, const float *log_b, float *pi_val,
                                       int32_t *pi_idx, float *row_lmax, float *row_sum, float *row_lmass, float *u, float *v, int variant,
                                       void *ws, size_t ws_bytes, void *stream) {
    const int rc = sinkhorn_ub_check("dvm_sinkhorn_ub_fwd_f32", f1, f2, pi_val, pi_idx, B, N, M, d, neg_alpha, n_iter, topk, tau_row, tau_col, variant);
    if (rc != DVM_OK) return rc;
    SinkhornWs w;
    if (!carve_ws(ws, ws_bytes, "dvm_sinkhorn_ub_fwd_f32", w, carve_sinkhorn_ub, B, N, M)) return DVM_ENOSPACE;
    hipStream_t s = (hipStream_t)stream;
    float *ub = u ? u : w.wu, *vb = v ? v : w.wv;
    if (n_iter == 0 && v) (void)hipMemsetAsync(v, 0, (size_t)B * M * sizeof(float), s);
    const Relax rx{tau_row, tau_col, log_a, log_b, row_lmass, nullptr, nullptr};
    return sinkhorn_run(f1, f2, B, N, M, d, neg_alpha, n_iter, topk, pi_val, pi_idx, row_lmax, row_sum, w.n1, w.n2, ub, 0, N, vb, 0, M, u,
                        variant == 0 && d == D, s, &rx);
}

DVM_EXPORT size_t dvm_sinkhorn_ub_hist_workspace_bytes(int B, int N, int M, int d) {
    (void)d;
    if (B < 1 || N < 1 || M < 1) return 0;
    return null_carve<SinkhornWs>(carve_sinkhorn_ub, B, N, M);
}

DVM_EXPORT int dvm_sinkhorn_ub_fwd_hist_f32(const float *f1, const float *f2, int B, int N, int M, int d, float neg_alpha, int n_iter,
                                            int topk, float tau_row, float tau_col, const float *log_a, const float *log_b, float *pi_val,
                                            int32_t *pi_idx, float *row_lmax, float *row_sum, float *row_lmass, float *rn_hist,
                                            float *cn_hist, int variant, void *ws, size_t ws_bytes, void *stream) {
    const char *who = "dvm_sinkhorn_ub_fwd_hist_f32";
    const int rc = sinkhorn_ub_check(who, f1, f2, pi_val, pi_idx, B, N, M, d, neg_alpha, n_iter, topk, tau_row, tau_col, variant);
    if (rc != DVM_OK) return rc;
    DVM_REQUIRE(rn_hist && cn_hist, "%s: null pointer", who);
    SinkhornWs w;
    if (!carve_ws(ws, ws_bytes, who, w, carve_sinkhorn_ub, B, N, M)) return DVM_ENOSPACE;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(sinkhorn_zero_slice_kernel, dim3((M + 255) / 256, B), dim3(256), 0, s, cn_hist, M, (long)(n_iter + 1) * M);   // slot 0
    const Relax rx{tau_row, tau_col, log_a, log_b, row_lmass, rn_hist, cn_hist};
    return sinkhorn_run(f1, f2, B, N, M, d, neg_alpha, n_iter, topk, pi_val, pi_idx, row_lmax, row_sum, w.n1, w.n2, w.wu, 0, N, w.wv, 0, M,
                        nullptr, variant == 0 && d == D, s, &rx);
}
