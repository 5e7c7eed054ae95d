// dvm_knn.hip — K3, feature-space kNN of LG-Net (knn_new / knn): fp32-MFMA score tiles, then a per-row top-k selection.
// Reference: models/model.py:267-278 (knn_new); models/loss.py:451-462 (knn).
// Layout: features are point-major [B][N][C] fp32 in HBM (the host transposes the reference's (B,C,N) once per block).
#include "dvm_mfma_tile.h"

namespace dvm {

// ============================================================== scores
// s_ij = (-|a_i|^2 - (-2 * a_i.b_j)) - |b_j|^2, the dot product a k-ordered fma chain.
// MFMA orientation: A = queries, B = keys, so a lane owns one key column and a register one
// query row: rows of S are written as contiguous 128-B segments.
constexpr int KS_KT = 64, KS_QB = 128, KS_THREADS = 256;  // 4 waves x 32 query rows per workgroup

// What the two matrix-core score kernels share.  A wave owns the 32 query rows from row0; a lane keeps the A-operand fragment of
// query row0 + r32, the norms of the 16 query rows its accumulator registers cover, and its workgroup's key range.
template <int D>
struct KnnScoreFrame {
    int b, row0, tid, lane, wave, r32, h;
    float q[D / 2], nq[16];
    const float *kb;   // the entry's keys
    int jbeg, jend;    // this workgroup's key range
};
template <int D>
__device__ __forceinline__ void knn_score_frame(KnnScoreFrame<D> &f, const float *__restrict__ a, const float *__restrict__ bq,
                                                const float *__restrict__ na, int N, int M, int kchunk) {
    f.b = blockIdx.y;
    f.tid = threadIdx.x, f.lane = f.tid & 63, f.wave = f.tid >> 6, f.r32 = f.lane & 31, f.h = f.lane >> 5;
    f.row0 = blockIdx.x * KS_QB + f.wave * 32;
    const int qrow = f.row0 + f.r32;
    load_frag<D>(a + ((size_t)f.b * N + (qrow < N ? qrow : N - 1)) * D, f.h, f.q);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        int row = f.row0 + lane_key(r, f.h);
        f.nq[r] = na[(size_t)f.b * N + (row < N ? row : N - 1)];
    }
    f.kb = bq + (size_t)f.b * M * D;
    f.jbeg = blockIdx.z * kchunk, f.jend = f.jbeg + kchunk < M ? f.jbeg + kchunk : M;
}
// the lane's 16 scores of key j (norm nbj) from the chain's accumulator
template <int D>
__device__ __forceinline__ void knn_store_scores(const KnnScoreFrame<D> &f, const f32x16 &acc, int j, float nbj, int N, int M,
                                                 float *__restrict__ S) {
    if (j < M) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            int row = f.row0 + lane_key(r, f.h);
            float inner = -2.f * acc[r];
            float s = (-f.nq[r] - inner) - nbj;
            if (row < N) S[((size_t)f.b * N + row) * M + j] = s;
        }
    }
}

// key tiles staged through registers into a k-deinterleaved LDS tile (shipped for C = 64)
template <int D>
__global__ __launch_bounds__(KS_THREADS, 2) void knn_scores_mfma_kernel(const float *__restrict__ a, const float *__restrict__ bq,
                                                                       const float *__restrict__ na, const float *__restrict__ nb,
                                                                       int N, int M, int kchunk, float *__restrict__ S) {
    constexpr int LDK = D + 4, H = D / 2;
    __shared__ __attribute__((aligned(16))) float kt[KS_KT * LDK];
    __shared__ float kn[KS_KT];
    KnnScoreFrame<D> f;
    knn_score_frame(f, a, bq, na, N, M, kchunk);
    const int tid = f.tid, r32 = f.r32, h = f.h;
    for (int j0 = f.jbeg; j0 < f.jend; j0 += KS_KT) {
        __syncthreads();
        for (int e = tid; e < KS_KT * D / 4; e += KS_THREADS) {
            int r = e / (D / 4), c = e % (D / 4);
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (j0 + r < M) v = *(const f32x4 *)(f.kb + (size_t)(j0 + r) * D + 4 * c);
            float2 ev = {v.x, v.z}, od = {v.y, v.w};
            *(float2 *)(kt + r * LDK + 2 * c) = ev;
            *(float2 *)(kt + r * LDK + H + 2 * c) = od;
        }
        if (tid < KS_KT) kn[tid] = (j0 + tid < M) ? nb[(size_t)f.b * M + j0 + tid] : 0.f;
        __syncthreads();
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
            const float *krow = kt + (sub * 32 + r32) * LDK + h * H;
            f32x16 acc = zero16();
#pragma unroll
            for (int c = 0; c < H / 4; ++c) {
                const f32x4 kv = *(const f32x4 *)(krow + 4 * c);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(f.q[4 * c], kv.x, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(f.q[4 * c + 1], kv.y, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(f.q[4 * c + 2], kv.z, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(f.q[4 * c + 3], kv.w, acc, 0, 0, 0);
            }
            knn_store_scores(f, acc, j0 + sub * 32 + r32, kn[sub * 32 + r32], N, M, S);
        }
    }
}

// The same scores with the key tiles brought by LDS-DMA (shipped for C = 128, the form above for C = 64):
// two alternating buffers of 64 keys in their natural [key][D] layout, the 16-byte chunks of a row XOR-swizzled with the row
// number on the SOURCE address, the next tile requested before this tile's matrix instructions; a lane reads its two operands
// of a chunk (k = 4 c + h and 4 c + 2 + h) with one ds_read2_b32.  No staging registers, no ds_write, one barrier per tile.
// Same k-ordered chain per (query, key), same bits.
template <int D>
__global__ __launch_bounds__(KS_THREADS, 2) void knn_scores_dma_kernel(const float *__restrict__ a, const float *__restrict__ bq,
                                                                      const float *__restrict__ na, const float *__restrict__ nb,
                                                                      int N, int M, int kchunk, float *__restrict__ S) {
    constexpr int ROWB = D * 4, TILEB = KS_KT * ROWB, NI = TILEB / 1024 / 4;   // 1-KiB pieces per wave and tile
    constexpr int RPI = 1024 / ROWB, CPR = ROWB / 16;                          // rows per piece, chunks per row
    extern __shared__ __attribute__((aligned(16))) char ks_lds[];   // [2][64 keys][D] + [2][64] norms
    float *const kn0 = (float *)(ks_lds + 2 * TILEB);
    KnnScoreFrame<D> f;
    knn_score_frame(f, a, bq, na, N, M, kchunk);
    const int lane = f.lane, wave = f.wave, r32 = f.r32, h = f.h;
    const float *kb = f.kb;
    const float *nbb = nb + (size_t)f.b * M;
    // this lane's part of a piece: row lr of the piece, source chunk (position ^ row) — the row number's low bits are the
    // same for every piece (a piece starts on a multiple of RPI rows, RPI | 8 ... only RPI <= 8 rows per piece)
    const int lr = lane / CPR, lc = lane % CPR;
    auto stage = [&](int j0, int buf) {
        char *dst = ks_lds + buf * TILEB + wave * NI * 1024;
#pragma unroll
        for (int e = 0; e < NI; ++e) {
            const int r = (wave * NI + e) * RPI + lr;                 // key row of the tile
            const int j = j0 + r < M ? j0 + r : M - 1;                // (rows past the end: the last key again, never stored)
            const float *src = kb + (size_t)j * D + 4 * (lc ^ (r & 7));
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)src,
                                             (__attribute__((address_space(3))) void *)(dst + e * 1024), 16, 0, 0);
        }
        if (wave == 0) {
            const int j = j0 + lane < M ? j0 + lane : M - 1;
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(nbb + j),
                                             (__attribute__((address_space(3))) void *)(kn0 + buf * KS_KT), 4, 0, 0);
        }
    };
    int roff[8];   // byte offset of chunk c (mod 8) in this lane's key row, first operand
#pragma unroll
    for (int c = 0; c < 8; ++c) roff[c] = ((c ^ (r32 & 7)) << 4) + 4 * h;
    int cur = 0;
    stage(f.jbeg, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (int j0 = f.jbeg; j0 < f.jend; j0 += KS_KT) {
        if (j0 + KS_KT < f.jend) stage(j0 + KS_KT, cur ^ 1);   // (the other buffer was last read before the previous barrier)
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
            const char *krow = ks_lds + cur * TILEB + (sub * 32 + r32) * ROWB;
            f32x16 acc = zero16();
            // the key operands are requested 8 chunks at a time ahead of their matrix instructions (the scheduler otherwise
            // issues each read right before its MFMAs and the wave waits out the LDS latency every time)
#pragma unroll
            for (int c0 = 0; c0 < D / 4; c0 += 8) {
                float k0[8], k1[8];
#pragma unroll
                for (int c = 0; c < 8; ++c) {
                    const float *p = (const float *)(krow + (c0 / 8) * 128 + roff[c]);
                    k0[c] = p[0], k1[c] = p[2];
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int c = 0; c < 8; ++c) {
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(f.q[2 * (c0 + c)], k0[c], acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(f.q[2 * (c0 + c) + 1], k1[c], acc, 0, 0, 0);
                }
            }
            knn_store_scores(f, acc, j0 + sub * 32 + r32, kn0[cur * KS_KT + sub * 32 + r32], N, M, S);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        cur ^= 1;
    }
}

// generic-C scalar scores (any C): thread per (query, key tile)
__global__ __launch_bounds__(128) void knn_scores_scalar_kernel(const float *__restrict__ a, const float *__restrict__ bq,
                                                                const float *__restrict__ na, const float *__restrict__ nb, int N,
                                                                int M, int C, float *__restrict__ S) {
    const int b = blockIdx.y;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const float *qp = a + ((size_t)b * N + i) * C;
    const float nqi = na[(size_t)b * N + i];
    for (int j = 0; j < M; ++j) {
        const float *kp = bq + ((size_t)b * M + j) * C;
        float dot = 0.f;
        for (int c = 0; c < C; ++c) dot = fmaf(qp[c], kp[c], dot);
        float inner = -2.f * dot;
        S[((size_t)b * N + i) * M + j] = (-nqi - inner) - nb[(size_t)b * M + j];
    }
}

// ============================================================== top-k selection
// order-preserving map float -> uint (ascending), then inverted: smaller key == larger score
__device__ __forceinline__ unsigned desc_key(float f) {
    unsigned u = __float_as_uint(f);
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ~u;
}

// One workgroup per row: exact k-th key by 4 radix passes, compaction in index order (ties ->
// lowest index), bitonic sort of the k winners by (key, index).
template <int EPT>
__global__ __launch_bounds__(256) void topk_select_kernel(const float *__restrict__ S, int M, int k, int32_t *__restrict__ idx) {
    __shared__ int hist[256];
    __shared__ int sc[4];
    __shared__ int bc[4];
    __shared__ unsigned long long sel[512];
    const size_t row = blockIdx.x;
    const float *s = S + row * M;
    const int tid = threadIdx.x;
    unsigned key[EPT];
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
        int j = tid * EPT + e;
        key[e] = j < M ? desc_key(s[j]) : 0xffffffffu;  // padding sorts last (NaN-free inputs assumed)
    }
    unsigned prefix = 0, mask = 0;
    int remaining = k;
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        hist[tid] = 0;
        __syncthreads();
#pragma unroll
        for (int e = 0; e < EPT; ++e) {
            int j = tid * EPT + e;
            if (j < M && (key[e] & mask) == prefix) atomicAdd(&hist[(key[e] >> shift) & 255], 1);
        }
        __syncthreads();
        int total;
        int mine = hist[tid];
        int excl = block_exclusive_scan<256>(mine, sc, total);
        if (excl < remaining && excl + mine >= remaining) {  // exactly one bin
            bc[0] = tid;
            bc[1] = excl;
        }
        __syncthreads();
        prefix |= (unsigned)bc[0] << shift;
        mask |= 255u << shift;
        remaining -= bc[1];
        __syncthreads();
    }
    // prefix == k-th smallest key; take all keys < prefix and the first `remaining` keys == prefix
    int nlt = 0, neq = 0;
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
        int j = tid * EPT + e;
        if (j < M) {
            nlt += key[e] < prefix;
            neq += key[e] == prefix;
        }
    }
    int tot_lt, tot_eq;
    int plt = block_exclusive_scan<256>(nlt, sc, tot_lt);
    int peq = block_exclusive_scan<256>(neq, sc, tot_eq);
    int kp2 = 1;
    while (kp2 < k) kp2 <<= 1;
    for (int e = tid; e < kp2; e += 256) sel[e] = ~0ull;
    __syncthreads();
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
        int j = tid * EPT + e;
        if (j < M) {
            if (key[e] < prefix) {
                sel[plt++] = ((unsigned long long)key[e] << 32) | (unsigned)j;
            } else if (key[e] == prefix) {
                if (peq < remaining) sel[tot_lt + peq] = ((unsigned long long)key[e] << 32) | (unsigned)j;
                peq++;
            }
        }
    }
    __syncthreads();
    for (int size = 2; size <= kp2; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = tid; t < kp2 / 2; t += 256) {
                int lo = (t / stride) * stride * 2 + (t % stride), hi = lo + stride;
                bool up = ((lo & size) == 0);
                unsigned long long x = sel[lo], y = sel[hi];
                if ((x > y) == up) {
                    sel[lo] = y;
                    sel[hi] = x;
                }
            }
            __syncthreads();
        }
    }
    for (int t = tid; t < k; t += 256) idx[row * k + t] = (int32_t)(sel[t] & 0xffffffffu);
}

// ---- the wave top-k kernels (k <= 64): one WAVE per row, no workgroup barriers (the block kernel above spends ~50 of them per row).
//   1. every lane finds the two smallest of its keys (columns e * 64 + lane);
//   2. Tc = the k-th smallest of those 128 lane minima, by a 32-step bit search with ballots: an upper bound of the
//      row's k-th smallest key, and tight (it is exact unless some lane holds three of the row's k best);
//   3. the keys <= Tc (about k of them) are compacted into (key << 32 | column) words and bitonic-sorted across the
//      wave; the first k are the answer, ties in column order.
//   If more than 128 keys pass (heavy ties) the exact k-th key is searched over all keys instead and only the
//   winners are compacted (wave_select_ties).
// The pieces below are shared by the two kernels; each keeps its own way of holding the row.

// a lane's running two smallest keys
__device__ __forceinline__ void two_smallest(unsigned x, unsigned &m1, unsigned &m2) {
    m2 = min(m2, max(m1, x));
    m1 = min(m1, x);
}

// The k-th smallest of the keys a wave holds: the largest T with count(keys < T) < k, found bit by bit.  count_below(c) = how
// many of the wave's keys are < c (wave-uniform).
template <class CountBelow>
__device__ __forceinline__ unsigned kth_smallest(int k, CountBelow count_below) {
    unsigned T = 0;
    for (int bit = 31; bit >= 0; --bit) {
        const unsigned c = T | (1u << bit);
        if (count_below(c) < k) T = c;
    }
    return T;
}
// ... of the 128 lane minima (step 2)
__device__ __forceinline__ unsigned kth_of_minima(int k, unsigned m1, unsigned m2) {
    return kth_smallest(k, [&](unsigned c) { return __popcll(__ballot(m1 < c)) + __popcll(__ballot(m2 < c)); });
}

// the wave's candidate words, all ~0 (they sort last)
__device__ __forceinline__ void wave_cand_reset(unsigned long long *cw, int lane) {
    cw[lane] = ~0ull;
    cw[lane + 64] = ~0ull;
}

// Heavy ties: the exact k-th smallest key T over all keys of the row, then only the winners — every key < T and the first
// k - count(keys < T) keys == T in column order — compacted into cw; returns their number (k).  key_at(e) = the lane's key of column
// e * 64 + lane (0xffffffff past M).  EPL > 0: the row is EPL slots long at compile time and the loops unroll, so that a
// register array behind key_at stays statically indexed; EPL == 0: E slots, key_at re-reads the row.
template <int EPL, class KeyAt>
__device__ __forceinline__ int wave_select_ties(int E, int M, int k, int lane, KeyAt key_at, unsigned long long *cw) {
    constexpr int UNROLL = EPL > 0 ? EPL : 1;   // (1: the runtime loops stay rolled)
    const int n = EPL > 0 ? EPL : E;
    const unsigned long long below = (1ull << lane) - 1ull;
    const unsigned T = kth_smallest(k, [&](unsigned c) {
        int cnt = 0;
#pragma unroll UNROLL
        for (int e = 0; e < n; ++e) cnt += __popcll(__ballot(key_at(e) < c));
        return cnt;
    });
    int lt = 0;
#pragma unroll UNROLL
    for (int e = 0; e < n; ++e) lt += __popcll(__ballot(key_at(e) < T));
    const int ties = k - lt;
    int base = 0, tbase = 0;
#pragma unroll UNROLL
    for (int e = 0; e < n; ++e) {
        const int j = e * 64 + lane;
        const unsigned x = key_at(e);
        const bool eq = x == T && j < M;   // (a padding key equals a real one only for a NaN score)
        const unsigned long long meq = __ballot(eq);
        const int teq = tbase + __popcll(meq & below);   // this key's rank among the ties, column order
        const bool take = (x < T && j < M) || (eq && teq < ties);
        const unsigned long long mt = __ballot(take);
        if (take) cw[base + __popcll(mt & below)] = ((unsigned long long)x << 32) | (unsigned)j;
        base += __popcll(mt);
        tbase += __popcll(meq);
    }
    return base;
}

// Tail: the (key << 32 | column) words compacted into cw[0..base) (rest ~0) are bitonic-sorted across the wave, element
// i = lane + 64 * slot (LDS operations of one wave execute in order), and the first k columns written out.
__device__ __forceinline__ void wave_sort_and_store(const unsigned long long *cw, int base, int lane, int k, int32_t *__restrict__ out) {
    unsigned long long a0 = cw[lane], a1 = cw[lane + 64];
    const bool small = base <= 64;  // everything sits in slot 0 then (slot 1 is all ~0)
    for (int size = 2; size <= (small ? 64 : 128); size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            if (stride == 64) {  // partner is the other slot of this lane; i = lane (slot 0) is the lower index, ascending
                const unsigned long long lo = a0 < a1 ? a0 : a1, hi = a0 < a1 ? a1 : a0;
                a0 = lo, a1 = hi;
            } else {
                const bool lower = (lane & stride) == 0;
#pragma unroll
                for (int slot = 0; slot < 2; ++slot) {
                    if (slot == 1 && small) break;
                    unsigned long long &x = slot ? a1 : a0;
                    const int i = lane + 64 * slot;
                    const bool up = (i & size) == 0 || size == 128;
                    const unsigned long long y =
                        ((unsigned long long)__shfl_xor((unsigned)(x >> 32), stride, 64) << 32) | __shfl_xor((unsigned)x, stride, 64);
                    const bool keep_min = (lower == up);
                    x = keep_min ? (x < y ? x : y) : (x < y ? y : x);
                }
            }
        }
    }
    if (lane < k) out[lane] = (int32_t)(unsigned)a0;
    if (!small && lane + 64 < k) out[lane + 64] = (int32_t)(unsigned)a1;
}

// Rows of up to EPL * 64 columns: every lane keeps its EPL keys in registers.
template <int EPL>
__global__ __launch_bounds__(256) void topk_wave_kernel(const float *__restrict__ S, int M, int k, long rows,
                                                        int32_t *__restrict__ idx) {
    __shared__ unsigned long long cand[4][128];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long row = (long)blockIdx.x * 4 + wave;
    if (row >= rows) return;
    const float *s = S + row * M;
    unsigned key[EPL];
    unsigned m1 = 0xffffffffu, m2 = 0xffffffffu;
    // all EPL loads are requested before the first is used: the index is clamped instead of the load being predicated (a
    // conditional load is a branch around a load + wait: the row arrived in 32 dependent round trips, 63 us per layer)
    float sv[EPL];
    if (M == EPL * 64) {   // (wave-uniform) full rows: one base register, immediate offsets, EPL loads back to back
#pragma unroll
        for (int e = 0; e < EPL; ++e) sv[e] = s[e * 64 + lane];
    } else {
#pragma unroll
        for (int e = 0; e < EPL; ++e) {
            const int j = e * 64 + lane;
            sv[e] = s[j < M ? j : M - 1];
        }
    }
#pragma unroll
    for (int e = 0; e < EPL; ++e) {
        const int j = e * 64 + lane;
        key[e] = j < M ? desc_key(sv[e]) : 0xffffffffu;
        two_smallest(key[e], m1, m2);
    }
    const unsigned T = kth_of_minima(k, m1, m2);
    unsigned long long *cw = cand[wave];
    wave_cand_reset(cw, lane);
    int base = 0;
    // Each lane marks its own keys <= Tc (about one per lane); a wave prefix sum gives every lane its slots and the lane
    // writes its few winners itself — the final sort orders by (key, column), so the compaction order is free.  (The
    // previous form ranked all EPL key slots with two ballots + two lane counts each: 12 VALU x 32 slots.)
    static_assert(EPL <= 32, "one 32-bit pass mask per lane");
    unsigned pm = 0;
#pragma unroll
    for (int e = 0; e < EPL; ++e) pm |= key[e] <= T ? (1u << e) : 0u;
    const int mine = __popc(pm);
    int incl = mine;  // inclusive prefix over lanes
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_up(incl, o, 64);
        if (lane >= o) incl += up;
    }
    const int C = __shfl(incl, 63, 64);
    if (C <= 128) {
        int pos = incl - mine;
        const int iters = __reduce_max_sync(~0ull, mine);
        for (int it = 0; it < iters; ++it) {
            if (pm) {
                const int e = __ffs(pm) - 1;
                pm &= pm - 1;
                const int j = e * 64 + lane;
                const unsigned x = j < M ? desc_key(s[j < M ? j : M - 1]) : 0xffffffffu;  // re-read (L1 hit): no dynamic register index
                cw[pos++] = ((unsigned long long)x << 32) | (unsigned)j;
            }
        }
        base = C;
    } else {
        base = wave_select_ties<EPL>(EPL, M, k, lane, [&](int e) { return key[e]; }, cw);
    }
    wave_sort_and_store(cw, base, lane, k, idx + row * k);
}

// Rows longer than 2048 columns: the same algorithm without the per-lane key array (128 VGPRs at EPL = 128 left two
// waves per SIMD and ran 7x slower per byte than EPL = 32).  The row is streamed three times instead — lane minima,
// then count + optimistic compaction of the keys <= Tc — and stays L2-resident between the passes (20 KB at M = 4995).
__global__ __launch_bounds__(256) void topk_wave_stream_kernel(const float *__restrict__ S, int M, int k, long rows,
                                                               int32_t *__restrict__ idx) {
    __shared__ unsigned long long cand[4][128];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long row = (long)blockIdx.x * 4 + wave;
    if (row >= rows) return;
    const float *s = S + row * M;
    const int E = (M + 63) / 64;
    const unsigned long long below = (1ull << lane) - 1ull;
    unsigned m1 = 0xffffffffu, m2 = 0xffffffffu;
    for (int e0 = 0; e0 < E; e0 += 8) {   // eight loads in flight (clamped, not predicated: see topk_wave_kernel)
        float sv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int j = (e0 + u) * 64 + lane;
            sv[u] = s[j < M ? j : M - 1];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int j = (e0 + u) * 64 + lane;
            two_smallest(j < M ? desc_key(sv[u]) : 0xffffffffu, m1, m2);
        }
    }
    const unsigned T = kth_of_minima(k, m1, m2);
    unsigned long long *cw = cand[wave];
    wave_cand_reset(cw, lane);
    int base = 0;
    for (int e0 = 0; e0 < E; e0 += 8) {  // optimistic: at most 128 keys pass unless the row has heavy ties
        float sv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int j = (e0 + u) * 64 + lane;
            sv[u] = s[j < M ? j : M - 1];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int j = (e0 + u) * 64 + lane;
            const unsigned x = j < M ? desc_key(sv[u]) : 0xffffffffu;
            const bool take = x <= T && j < M;
            const unsigned long long mt = __ballot(take);
            const int pos = base + __popcll(mt & below);
            if (take && pos < 128) cw[pos] = ((unsigned long long)x << 32) | (unsigned)j;
            base += __popcll(mt);
        }
    }
    if (base > 128) {
        wave_cand_reset(cw, lane);
        base = wave_select_ties<0>(E, M, k, lane, [&](int e) {
            const int j = e * 64 + lane;
            return j < M ? desc_key(s[j < M ? j : M - 1]) : 0xffffffffu;   // (clamped, not predicated: see topk_wave_kernel)
        }, cw);
    }
    wave_sort_and_store(cw, base, lane, k, idx + row * k);
}

// ============================================================== host
int launch_knn_neg(const float *a, const float *bq, int B, int N, int M, int C, int k, int32_t *idx, float *na, float *nb,
                   float *S, hipStream_t s) {
    launch_rownorm2(a, B * N, C, na, s);
    if (a == bq && N == M) nb = na;   // self-kNN (every N2P layer): one set of norms
    else launch_rownorm2(bq, B * M, C, nb, s);
    // key range split over grid.z until >= 1024 workgroups are in flight (B * N/128 alone is 128 at B = 8, N = 2048)
    const int qtiles = (N + KS_QB - 1) / KS_QB, ktiles = (M + KS_KT - 1) / KS_KT;
    int nz = 1;
    while (B * qtiles * nz < 1024 && nz * 2 <= ktiles) nz *= 2;
    const int kchunk = ((ktiles + nz - 1) / nz) * KS_KT;
    nz = (M + kchunk - 1) / kchunk;
    // measured at 8 x 2048 / 1 x 4995 points, scores + top-k per call: C = 128: 187 -> 171 us / 184 -> 163 us with the DMA form;
    // C = 64: 130 -> 137 us (half the bytes per key: the register path already hides them) — so C = 128 only
    if (C == 128) {
        constexpr int lds = 2 * KS_KT * 128 * 4 + 2 * KS_KT * 4;
        ensure_dyn_lds((const void *)knn_scores_dma_kernel<128>, lds);
        hipLaunchKernelGGL(knn_scores_dma_kernel<128>, dim3(qtiles, B, nz), dim3(KS_THREADS), lds, s, a, bq, na, nb, N, M, kchunk, S);
    } else if (C == 64)
        hipLaunchKernelGGL(knn_scores_mfma_kernel<64>, dim3(qtiles, B, nz), dim3(KS_THREADS), 0, s, a, bq, na, nb, N, M, kchunk, S);
    else
        hipLaunchKernelGGL(knn_scores_scalar_kernel, dim3((N + 127) / 128, B), dim3(128), 0, s, a, bq, na, nb, N, M, C, S);
    if (k <= 64 && M <= 8192) {
        const long rows = (long)B * N;
        const dim3 wgrid((unsigned)((rows + 3) / 4));
        if (M <= 2048)
            hipLaunchKernelGGL(topk_wave_kernel<32>, wgrid, dim3(256), 0, s, S, M, k, rows, idx);
        else
            hipLaunchKernelGGL(topk_wave_stream_kernel, wgrid, dim3(256), 0, s, S, M, k, rows, idx);
        return DVM_OK;
    }
    int ept = (M + 255) / 256;
    dim3 grid((unsigned)((size_t)B * N));
    if (ept <= 8)
        hipLaunchKernelGGL(topk_select_kernel<8>, grid, dim3(256), 0, s, S, M, k, idx);
    else if (ept <= 16)
        hipLaunchKernelGGL(topk_select_kernel<16>, grid, dim3(256), 0, s, S, M, k, idx);
    else
        hipLaunchKernelGGL(topk_select_kernel<32>, grid, dim3(256), 0, s, S, M, k, idx);
    return DVM_OK;
}

size_t carve_knn_neg(Arena &ar, int B, int N, int M, KnnNegWs &w) {
    w.na = ar.take<float>((size_t)B * N);
    w.nb = ar.take<float>((size_t)B * M);
    w.S = ar.take<float>((size_t)B * N * M);
    return ar.off;
}

}  // namespace dvm

using namespace dvm;

DVM_EXPORT size_t dvm_knn_neg_workspace_bytes(int B, int N, int M, int C, int k) { return null_carve<KnnNegWs>(carve_knn_neg, B, N, M); }

DVM_EXPORT int dvm_knn_neg_f32(const float *a, const float *b, int B, int N, int M, int C, int k, int32_t *idx, void *ws,
                               size_t ws_bytes, void *stream) {
    DVM_REQUIRE(a && b && idx, "dvm_knn_neg_f32: null pointer");
    DVM_REQUIRE(B >= 1 && N >= 1 && M >= 1 && C >= 1, "dvm_knn_neg_f32: empty input (B=%d N=%d M=%d C=%d)", B, N, M, C);
    DVM_REQUIRE(k >= 1 && k <= 512 && k <= M, "dvm_knn_neg_f32: k=%d unsupported (1..min(512,M=%d))", k, M);
    DVM_REQUIRE(M <= 8192, "dvm_knn_neg_f32: M=%d exceeds 8192", M);
    KnnNegWs w;
    if (!carve_ws(ws, ws_bytes, "dvm_knn_neg_f32", w, carve_knn_neg, B, N, M)) return DVM_ENOSPACE;
    launch_knn_neg(a, b, B, N, M, C, k, idx, w.na, w.nb, w.S, (hipStream_t)stream);
    DVM_CHECK_LAUNCH("knn_neg");
    return DVM_OK;
}
