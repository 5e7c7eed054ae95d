// dvm_dist_tile.h — the fp32 squared-distance tile of the soft-correspondence family and the frame around it, defined once.
//
// Users:
//   sweeps (SW_* geometry, row_frame, two_role_sweep)    softcorr_mfma_kernel (dvm_softcorr.hip), sinkhorn_mfma_kernel
//                                                        (dvm_sinkhorn.hip), skb_sweep_mfma_kernel (dvm_sinkhorn_bwd.hip; no frame)
//   phase B (BW_* geometry and the phase-B pieces)       softcorr_bwd_mfma_kernel (dvm_softcorr_bwd.hip), skb_apply_mfma_kernel
//                                                        (dvm_sinkhorn_bwd.hip); each keeps its own prologue and tile loop
//   scalar sweeps (scalar_frame, scalar_sweep)           softcorr_scalar_kernel, sinkhorn_scalar_kernel, skb_sweep_scalar_kernel;
//                                                        softcorr_dense_kernel (the frame only)
//   scalar phase B (wave_row_*)                          softcorr_bwd_scalar_kernel, skb_apply_scalar_kernel
// The operators are correct only if every one of them forms the same S_ij bit for bit (Sinkhorn at
// n_iter = 0 is pinned to dvm_softcorr_fwd_f32, phase A of the Sinkhorn backward to the forward, a row step to its
// transpose, the two phase-B kernels to each other) and only if their workgroup geometries agree, so the tile, the
// geometry, a lane's view of its row and the sweep loops live here and nowhere else.  Everything below is a constant or a
// stateless __device__ __forceinline__ piece; argument structs, sidecar planes, epilogue arithmetic, __launch_bounds__
// and launchers belong to the kernels.  (The fp16 pass A, dvm_softcorr_f16.h, is a different tile.)
//
// The distance.  Squared distances are the matmul form of torch.cdist, [-2a, |a|^2, 1] . [b, 1, |b|^2], evaluated as a
// k-ordered fp32 fma chain; v_mfma_f32_32x32x2_f32 computes exactly that chain, so the matrix-core and the scalar forms
// agree with the reference's CPU (MKL sgemm) values bit for bit.
//
// Layout.  Features are row-major [B][rows][128] fp32 in HBM.  A wave keeps 32 "query" rows in registers (lane = row
// r32 = lane & 31, half h = lane >> 5 owns channels 2s + h as the B operand q[s] = -2 * row[2s + h]); "key" rows stream
// through a double-buffered LDS tile of KT = 64 rows (two 32-key sub-tiles), padded to LDK = 132 floats (528 B: keeps
// ds_read_b128 conflict-free) and k-deinterleaved on the way in: global channel k = 4c + {0, 1, 2, 3} goes to
// (h, s) = (0, 2c) (1, 2c) (0, 2c + 1) (1, 2c + 1), i.e. position p < 64 holds channel 2p and position 64 + p channel
// 2p + 1, so half h reads its 64 A operands as 16 contiguous float4 at kt + row * LDK + 64 h.
// The accumulator tile is [key][query]: a query's 16 candidates of a sub-tile sit in ONE lane's registers (entry r of
// half h is local key (r & 3) + 8 (r >> 2) + 4 h, lane_key below), so top-k insertion, online softmax and LSE need no
// cross-lane traffic until the two half-lanes of a query (lane, lane ^ 32) merge at the end.
//
// Phase structure of the three sweeps (8 waves x 32 queries; waves w and w + 4 share a SIMD).  Every wave alternates an
// MFMA phase M (64 dependent MFMAs, 4096 matrix-pipe cycles) with a VALU phase V (the epilogue) of about the same
// length.  The two waves of a SIMD would run them in lockstep — matrix pipe contended, then idle — so waves 4-7
// (role 1) defer the epilogue of each tile's second sub-tile across the barrier:
//     role 0:   M0 V0 M1 V1 | barrier        role 1:   V1' M0 V0 M1 | barrier
// After every barrier one wave of the SIMD starts in M and its partner in V.  Every wave still folds its sub-tiles in
// ascending key order: a row's result does not depend on the wave that owns it.  Role 1 runs V1' after the barrier that
// frees the tile's buffer, so a kernel's "chain" step must take everything its epilogue needs out of LDS.
// two_role_sweep below is that loop.
#pragma once

#include "dvm_mfma_tile.h"

namespace dvm {


constexpr float LOG2E = 1.4426950408889634f;

namespace dtile {

constexpr int D = 128;
constexpr int KT = 64;               // keys per LDS tile (two 32-key MFMA sub-tiles)
constexpr int LDK = D + 4;           // padded row (floats)
constexpr int ROWS_FLOATS = KT * LDK;   // the key rows of one tile; a kernel's [KT] sidecar planes follow

// entry r of half h of an accumulator <-> key of the 32-key sub-tile

// B-operand fragment of a lane's own row: q[s] = -2 * row[2s + h]
__device__ __forceinline__ void load_query_frag(const float *row, int h, float (&q)[D / 2]) {
#pragma unroll
    for (int c = 0; c < D / 4; ++c) {
        f32x4 v = *(const f32x4 *)(row + 4 * c);
        q[2 * c] = -2.f * (h ? v.y : v.x);
        q[2 * c + 1] = -2.f * (h ? v.w : v.z);
    }
}

// rows [j0, j0 + KT) of base [rows][D] into registers, zero-filled past the end
template <int THREADS>
__device__ __forceinline__ void issue_tile(const float *base, int j0, int rows, int tid, f32x4 (&pre)[KT * D / 4 / THREADS]) {
#pragma unroll
    for (int e = 0; e < KT * D / 4 / THREADS; ++e) {
        int id = tid + e * THREADS;
        int r = id >> 5, c = id & 31;   // 32 float4 per 128-float row
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (j0 + r < rows) v = *(const f32x4 *)(base + (size_t)(j0 + r) * D + 4 * c);
        pre[e] = v;
    }
}

// ... and from the registers into the tile kt [KT][LDK], deinterleaved
template <int THREADS>
__device__ __forceinline__ void commit_tile(float *kt, int tid, const f32x4 (&pre)[KT * D / 4 / THREADS]) {
#pragma unroll
    for (int e = 0; e < KT * D / 4 / THREADS; ++e) {
        int id = tid + e * THREADS;
        int r = id >> 5, c = id & 31;
        float2 ev = {pre[e].x, pre[e].z}, od = {pre[e].y, pre[e].w};
        *(float2 *)(kt + r * LDK + 2 * c) = ev;
        *(float2 *)(kt + r * LDK + 64 + 2 * c) = od;
    }
}

// acc[r] = sum_k -2 query[k] key[lane_key(r, h)][k] over sub-tile `sub` of the tile kt, for the lane's query
__device__ __forceinline__ void dist_chain(const float *kt, int sub, int r32, int h, const float (&q)[D / 2], f32x16 &acc) {
    const float *arow = kt + (sub * 32 + r32) * LDK + h * 64;
    acc = f32x16{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < 16; ++c) {
        f32x4 a = *(const f32x4 *)(arow + 4 * c);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, q[4 * c], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, q[4 * c + 1], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, q[4 * c + 2], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, q[4 * c + 3], acc, 0, 0, 0);
    }
}

// the lane's 16 scalars of a [KT] sidecar plane (norms, potentials, coefficients, ...): v[r] = plane[32 sub + lane_key(r, h)]
__device__ __forceinline__ void lane_scalars(const float *plane, int sub, int h, float (&v)[16]) {
    const float *p = plane + sub * 32 + 4 * h;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        f32x4 x = *(const f32x4 *)(p + 8 * g);
        v[4 * g] = x.x, v[4 * g + 1] = x.y, v[4 * g + 2] = x.z, v[4 * g + 3] = x.w;
    }
}

// The squared distance from the chain's value.  cdist adds |f1|^2 first: (acc + |f1_i|^2) + |f2_j|^2 whichever side the
// queries are (SWAP: the queries are f2, the column step), so that a step and its transpose see the same S_ij bit for
// bit.  +inf for a padding key (norm +inf).
template <bool SWAP>
__device__ __forceinline__ float sqdist_sum(float acc, float nq, float nk) {
    return SWAP ? (acc + nk) + nq : (acc + nq) + nk;
}
template <bool SWAP>
__device__ __forceinline__ float sqdist(float acc, float nq, float nk) {
    const float d2 = sqdist_sum<SWAP>(acc, nq, nk);
    return d2 > 0.f ? d2 : 0.f;
}

// Geometry of the three sweeps: a workgroup owns 256 query rows.
constexpr int SW_QW = 32;                  // queries per wave
constexpr int SW_WAVES = 8;                // waves 0-3 and 4-7 pair up on the 4 SIMDs (two per SIMD)
constexpr int SW_QB = SW_QW * SW_WAVES;    // 256 queries per workgroup
constexpr int SW_THREADS = 64 * SW_WAVES;
constexpr int SW_LD_PER_THREAD = KT * D / 4 / SW_THREADS;   // float4 loads per thread per tile = 4
constexpr int SW_STAGE = 16 * 64;          // floats per wave of a top-k epilogue's staging block: a sub-tile's 16 values of each lane, [r][lane]

// A lane's view of its query row.  lid: the logical block id within the launch's group; tiles: blocks of SW_QB rows per entry;
// feat [B][rows][D], norms [B][rows].
struct RowFrame {
    int b, tile;               // entry, block of SW_QB rows of the entry
    int tid, lane, wave, r32, h;
    int row, rc;               // the lane's row of the entry; clamped to the entry's last row (row >= rows: nothing is stored)
    const float *p;            // features of row rc
    float q[D / 2];            // its B-operand fragment
    float nrm;                 // |row|^2
};
__device__ __forceinline__ void row_frame(RowFrame &f, int lid, int tiles, int rows, const float *feat, const float *norms) {
    f.b = lid / tiles, f.tile = lid % tiles;
    f.tid = threadIdx.x, f.lane = f.tid & 63, f.wave = f.tid >> 6;
    f.r32 = f.lane & 31, f.h = f.lane >> 5;
    f.row = f.tile * SW_QB + f.wave * SW_QW + f.r32;
    f.rc = f.row < rows ? f.row : rows - 1;
    f.p = feat + ((size_t)f.b * rows + f.rc) * D;
    load_query_frag(f.p, f.h, f.q);
    f.nrm = norms[(size_t)f.b * rows + f.rc];
}
// ... of a launch with one group: the logical block id is the hardware one, remapped
__device__ __forceinline__ void row_frame(RowFrame &f, int tiles, int rows, const float *feat, const float *norms) {
    row_frame(f, xcd_remap(blockIdx.x, gridDim.x), tiles, rows, feat, norms);
}

// The two-role loop over the ntiles key tiles of a sweep; role = wave >> 2, wave-uniform.  The kernel supplies
//   issue(t) / commit(buf)   tile t and its sidecar planes into registers / from them into buffer buf,
//   chain(buf, sub)          the distance chain of a sub-tile plus everything its epilogue needs from LDS,
//   epilogue(t, sub)         the operator, on what the last chain left in registers.
// LATE_LOADS issues the next tile's loads after the epilogues instead of before them (the other wave of the SIMD covers
// the latency): for a kernel whose epilogue state leaves no room for the prefetch registers.
template <bool LATE_LOADS, class Issue, class Commit, class Chain, class Epilogue>
__device__ __forceinline__ void two_role_sweep(int ntiles, int role, Issue issue, Commit commit, Chain chain, Epilogue epilogue) {
    issue(0);
    commit(0);
    __syncthreads();
    for (int t = 0; t < ntiles; ++t) {
        const int buf = t & 1;
        if (!LATE_LOADS && t + 1 < ntiles) issue(t + 1);
        if (role == 1 && t > 0) epilogue(t - 1, 1);   // V1' of the previous tile
        chain(buf, 0);
        epilogue(t, 0);
        chain(buf, 1);
        if (role == 0) epilogue(t, 1);
        if (LATE_LOADS && t + 1 < ntiles) issue(t + 1);
        if (t + 1 < ntiles) commit(buf ^ 1);
        __syncthreads();
    }
    if (role == 1) epilogue(ntiles - 1, 1);
}

// ------------------------------------------------------------------------------------------------ phase B
// Shared by softcorr_bwd_mfma_kernel and skb_apply_mfma_kernel: WAVES waves own 32 WAVES "outer" rows in registers,
// "inner" rows stream through the tile.  Group 0 is the df1 pass (outer = f1 rows), group 1 the df2 pass.
constexpr int BW_WAVES = 4;
constexpr int BW_OB = 32 * BW_WAVES;       // 128 outer rows per workgroup
constexpr int BW_THREADS = 64 * BW_WAVES;
constexpr int BW_LD_PER_THREAD = KT * D / 4 / BW_THREADS;   // float4 loads per thread per tile = 8
constexpr int BW_MASK = 64 * BW_WAVES;     // skip-mask words per tile (skip_mask_load)

// the norm expansion's v is redone from the exact difference below this share of |f_o|^2 + |f_i|^2; both kernels (and
// their scalar forms) must take the redo on the same entries
constexpr float TAU = 1.f / 64.f;

// v[r] = |f_o - f_i|^2 of the lane's outer row (op: its features in global memory, cached) against its 16 inner rows of
// sub-tile `sub`: the chain, (acc + |f_o|^2) + |f_i|^2 with the norms from `norms` [KT], and where that cancelled
// (v < TAU (|f_o|^2 + |f_i|^2): a cluster of rows near one outer row) the difference itself, in a wave-uniform branch
// that ordinary features never take.  Not clamped.
__device__ __forceinline__ void outer_inner_sqdist(const float *kt, const float *norms, int sub, int r32, int h, const float (&q)[D / 2],
                                                   const float *op, float nrm_o, f32x16 &acc) {
    dist_chain(kt, sub, r32, h, q, acc);
    const float *sc = norms + sub * 32 + 4 * h;
    unsigned exact = 0;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const f32x4 nb = *(const f32x4 *)(sc + 8 * g);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int r = 4 * g + u;
            acc[r] = sqdist_sum<false>(acc[r], nrm_o, nb[u]);
            exact |= (acc[r] < TAU * (nrm_o + nb[u]) ? 1u : 0u) << r;
        }
    }
    if (__any(exact != 0)) {
#pragma unroll 1
        for (int r = 0; r < 16; ++r) {
            if (!__any((exact >> r) & 1u)) continue;
            // entry r against LDS row lane_key(r, h) of the sub-tile, all 128 channels by one lane
            const float *xr = kt + (sub * 32 + lane_key(r, h)) * LDK;
            float v = 0.f;
#pragma unroll 4
            for (int c = 0; c < D / 4; ++c) {
                const f32x4 o4 = *(const f32x4 *)(op + 4 * c);
                const float2 ev = *(const float2 *)(xr + 2 * c), od = *(const float2 *)(xr + 64 + 2 * c);
                const float d0 = ev.x - o4.x, d1 = od.x - o4.y, d2 = ev.y - o4.z, d3 = od.y - o4.w;
                v = fmaf(d0, d0, v);
                v = fmaf(d1, d1, v);
                v = fmaf(d2, d2, v);
                v = fmaf(d3, d3, v);
            }
#pragma unroll
            for (int rr = 0; rr < 16; ++rr)
                if (rr == r && ((exact >> r) & 1u)) acc[rr] = v;
        }
    }
}

// The top-k skip mask (bits [B][N][wpr]: bit j of f1 row i) of a tile x the workgroup's outer block ot, one word per
// thread, 64 WAVES words in LDS.  Group 0: word [outer row tid / 2][32-column half tid % 2]; group 1: word
// [inner row tid / WAVES][32-column group tid % WAVES of the block].  (Phase A's masked sweep, whose queries are
// columns, uses the group-1 form with its 8 waves.)
template <int WAVES>
__device__ __forceinline__ uint32_t skip_mask_load(int grp, const uint32_t *bits, int wpr, int b, int ot, int j0, int No, int Ni, int tid) {
    if (grp == 0) {
        const int mrow = ot * (32 * WAVES) + (tid >> 1), wc = (j0 >> 5) + (tid & 1);
        return (mrow < No && wc < wpr) ? bits[((size_t)b * No + mrow) * wpr + wc] : 0u;
    }
    const int irow = j0 + (int)((unsigned)tid / WAVES), wc = ot * WAVES + (int)((unsigned)tid % WAVES);
    return (irow < Ni && wc < wpr) ? bits[((size_t)b * Ni + irow) * wpr + wc] : 0u;
}
// the lane's 16 entries of sub-tile `sub`: bit r set where (its outer row, inner row lane_key(r, h)) is one of the f1
// row's top-k entries
template <int WAVES>
__device__ __forceinline__ unsigned skip_mask_lane(int grp, const uint32_t *msk, int wave, int r32, int sub, int h) {
    unsigned skip = 0;
    if (grp == 0) {
        const uint32_t word = msk[(wave * 32 + r32) * 2 + sub];
#pragma unroll
        for (int r = 0; r < 16; ++r) skip |= ((word >> lane_key(r, h)) & 1u) << r;
    } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) skip |= ((msk[(sub * 32 + lane_key(r, h)) * WAVES + wave] >> r32) & 1u) << r;
    }
    return skip;
}

// apply: out[o][pos] += sum_t W[t][o] * X[t][pos].  W's C-layout registers are fed straight back as the A operand (step
// r contracts inner row t = lane_key(r, h); the B side reads X at the same rows), so W never touches LDS.
// acc2[cb] : out[outer row (C layout)][position 4 r32 + cb]
__device__ __forceinline__ void apply_chain(const float *kt, int sub, int r32, int h, const float (&w)[16], f32x16 (&acc2)[4]) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const f32x4 x = *(const f32x4 *)(kt + (sub * 32 + lane_key(r, h)) * LDK + 4 * r32);
        acc2[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(w[r], x.x, acc2[0], 0, 0, 0);
        acc2[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(w[r], x.y, acc2[1], 0, 0, 0);
        acc2[2] = __builtin_amdgcn_mfma_f32_32x32x2f32(w[r], x.z, acc2[2], 0, 0, 0);
        acc2[3] = __builtin_amdgcn_mfma_f32_32x32x2f32(w[r], x.w, acc2[3], 0, 0, 0);
    }
}

// d_out[o] += (sum_t W[t][o]) * f_o - acc2[o] for the wave's 32 outer rows (row0 = the first of them, fo / dout
// [B][No][D], b the entry); rl is the lane's share of sum_t W[t][o], rsum [32 WAVES] LDS.  Positions go back to channels.
// ATOMIC: other workgroups add to the same rows (split inner loop, the top-k entries' scatter); else this workgroup
// owns them.
template <bool ATOMIC>
__device__ __forceinline__ void store_outer_rows(float *rsum, float rl, const float *fo, float *dout, int b, int row0, int No, int wave,
                                                 int r32, int h, const f32x16 (&acc2)[4]) {
    const float rtot = rl + __shfl_xor(rl, 32, 64);
    if (h == 0) rsum[wave * 32 + r32] = rtot;
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int o = lane_key(r, h);
        const int row = row0 + o;
        if (row >= No) continue;
        const float rr = rsum[wave * 32 + o];
        const float *src = fo + ((size_t)b * No + row) * D;
        float *dst = dout + ((size_t)b * No + row) * D;
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) {
            const int pos = 4 * r32 + cb;
            const int ch = pos < 64 ? 2 * pos : 2 * (pos - 64) + 1;
            const float val = rr * src[ch] - acc2[cb][r];
            if (ATOMIC)
                unsafeAtomicAdd(dst + ch, val);
            else
                dst[ch] += val;
        }
    }
}

// ------------------------------------------------------------------------------------------------ scalar forms
// Cross-checks of the matrix-core kernels and the paths for d != 128 (any d % 4 == 0); not tuned.
// Sweeps: one thread per query row, keys staged through LDS in tiles of SC_KT, the dot product an explicit k-ordered
// fmaf chain — the chain the matrix cores evaluate.
constexpr int SC_KT = 32;   // keys per tile
constexpr int SC_DC = 32;   // feature chunk held in registers

// keys [j0, j0 + SC_KT) of kbase [M][d] into kt [SC_KT][d], zero-filled past the end (the caller's barriers around it)
__device__ __forceinline__ void scalar_stage_keys(float *kt, const float *kbase, int j0, int M, int d) {
    for (int e = threadIdx.x; e < SC_KT * d / 4; e += blockDim.x) {
        int r = e / (d / 4), c = e % (d / 4);
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (j0 + r < M) v = *(const f32x4 *)(kbase + (size_t)(j0 + r) * d + 4 * c);
        *(f32x4 *)(kt + r * d + 4 * c) = v;
    }
}

// acc[j] = sum_k -2 q[k] kt[j][k], k ascending
__device__ __forceinline__ void scalar_dist_chain(const float *q, const float *kt, int d, float (&acc)[SC_KT]) {
#pragma unroll
    for (int j = 0; j < SC_KT; ++j) acc[j] = 0.f;
    for (int c0 = 0; c0 < d; c0 += SC_DC) {
        float qr[SC_DC];
        int cw = d - c0 < SC_DC ? d - c0 : SC_DC;
#pragma unroll
        for (int c = 0; c < SC_DC; c += 4) {
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (c < cw) v = *(const f32x4 *)(q + c0 + c);
            qr[c] = -2.f * v.x, qr[c + 1] = -2.f * v.y, qr[c + 2] = -2.f * v.z, qr[c + 3] = -2.f * v.w;
        }
#pragma unroll
        for (int j = 0; j < SC_KT; ++j) {
#pragma unroll
            for (int c = 0; c < SC_DC; c += 4) {
                if (c < cw) {
                    f32x4 kv = *(const f32x4 *)(kt + j * d + c0 + c);
                    acc[j] = fmaf(qr[c], kv.x, acc[j]);
                    acc[j] = fmaf(qr[c + 1], kv.y, acc[j]);
                    acc[j] = fmaf(qr[c + 2], kv.z, acc[j]);
                    acc[j] = fmaf(qr[c + 3], kv.w, acc[j]);
                }
            }
        }
    }
}

// A thread's query row: workgroup blockIdx.x of entry blockIdx.y owns blockDim.x consecutive rows of feat [B][N][d].
struct ScalarFrame {
    int b, i, ic;      // entry, row, row clamped to the entry's last (i >= N: nothing is stored)
    const float *q;    // features of row ic
    float na;          // |row|^2
};
__device__ __forceinline__ ScalarFrame scalar_frame(const float *feat, const float *norms, int N, int d) {
    ScalarFrame f;
    f.b = blockIdx.y;
    f.i = blockIdx.x * blockDim.x + threadIdx.x;
    f.ic = f.i < N ? f.i : N - 1;
    f.q = feat + ((size_t)f.b * N + f.ic) * d;
    f.na = norms[(size_t)f.b * N + f.ic];
    return f;
}
// dynamic LDS of a scalar sweep with `planes` sidecar planes of the kernel's own next to the norms
constexpr size_t scalar_sweep_lds_bytes(int d, int planes) { return (size_t)(SC_KT * d + (1 + planes) * SC_KT) * sizeof(float); }

// The loop over the M keys of entry f.b (keys [B][M][d], knorms [B][M]) in tiles of SC_KT.  LDS: [SC_KT][d] keys, the [SC_KT]
// plane of their norms (+inf past the end: a padding key is at distance +inf), then the kernel's planes.  The kernel supplies
//   fill(j, in, side)           key j = j0 + threadIdx.x (in: j < M) of threads < SC_KT: its planes' values to side[p * SC_KT], p = 1 ..
//   epilogue(j0, acc, kn)       on acc[j] = the chain of key j0 + j; kn[j] its norm, kn[p * SC_KT + j] its plane p.
template <class Fill, class Epilogue>
__device__ __forceinline__ void scalar_sweep(const ScalarFrame &f, const float *keys, const float *knorms, int M, int d, Fill fill, Epilogue epilogue) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float *kt = smem;
    float *kn = smem + SC_KT * d;
    const float *kbase = keys + (size_t)f.b * M * d;
    for (int j0 = 0; j0 < M; j0 += SC_KT) {
        __syncthreads();
        scalar_stage_keys(kt, kbase, j0, M, d);
        if (threadIdx.x < SC_KT) {
            const int j = j0 + threadIdx.x;
            kn[threadIdx.x] = j < M ? knorms[(size_t)f.b * M + j] : INFINITY;
            fill(j, j < M, kn + threadIdx.x);
        }
        __syncthreads();
        float acc[SC_KT];
        scalar_dist_chain(f.q, kt, d, acc);
        epilogue(j0, acc, kn);
    }
}

// Phase B: one wave per outer row, lanes own channels lane + 64u (ov / xv: the outer and the inner row, d <= 512).
// The inner row and this lane's share of the dot product ...
__device__ __forceinline__ float wave_row_load_dot(const float *fi, int d, int lane, const float (&ov)[8], float (&xv)[8]) {
    float part = 0.f;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int c = lane + 64 * u;
        xv[u] = c < d ? fi[c] : 0.f;
        part = fmaf(ov[u], xv[u], part);
    }
    return part;
}
// ... and the squared distance from it (uniform over the wave), with the TAU redo; clamped
__device__ __forceinline__ float wave_row_sqdist(float part, const float (&ov)[8], const float (&xv)[8], float nrm_o, float ni) {
    float v = (-2.f * wave_sum(part) + nrm_o) + ni;
    if (v < TAU * (nrm_o + ni)) {   // uniform: the expansion cancelled, redo v from the difference
        float p2 = 0.f;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const float dd = ov[u] - xv[u];
            p2 = fmaf(dd, dd, p2);
        }
        v = wave_sum(p2);
    }
    return fmaxf(v, 0.f);
}

}  // namespace dtile
}  // namespace dvm
