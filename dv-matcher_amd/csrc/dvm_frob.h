// dvm_frob.h — the frame the sparse Frobenius-norm terms share: the rank term ||P P^T - I||_F (dvm_rank.hip), the cycle term
// ||P12 P21 - I||_F (dvm_cycle.hip) and the distortion term ||P D2 P^T - D1||_F (dvm_distortion.hip).  Every term is
//   F^2 = sum over rows i of (sum over the row of residual^2),
// one workgroup of FROB_THREADS per row: the row of the product in LDS as fp32, its squares summed in float64 through the fixed tree
// of block_tree_sum -> partial[b][i]; launch_reduce_partials -> f2[b]; frob_finish_kernel (dvm_frob.hip): loss = sqrt(F^2) and every
// gradient array, which the row kernels leave as num dF^2 / d val, *= num / F, 0 where F == 0 (torch.norm's subgradient there).
//
// No float atomics anywhere, so a term gives the same bits from run to run, alone or in a batch.  Where the terms of a sum arrive in
// an order that integer atomics set (the reversed lists of launch_rev_csr, the column sums of the distortion term), the sum is
// formed in the fixed point of dvm_common.h (fix_unit_exp / fix_quant / fix_value), which no order can change: a first pass takes the
// largest |term| m (a maximum does not depend on the order either), a second one adds the terms as 64-bit integers in units of
// 2^(ilogb(m) + 1 - 50) — every term below 2^50, a sum holds at most FROB_MAX_N = 2^13 of them.  The quantisation, at most
// N 2^-50 m, is far below one fp32 rounding of the result's own terms.
#pragma once
#include <stdarg.h>

#include <initializer_list>

#include "dvm_common.h"

namespace dvm {

constexpr int FROB_THREADS = 256;   // block_tree_sum's width: every row kernel runs one workgroup of this size
constexpr int FROB_MAX_N = 8192;    // rows (and, for the distortion term, columns): the row of the product takes N fp32 words of LDS
static_assert(12 * FROB_MAX_N + 4 * FROB_MAX_N <= 128 * 1024, "the distortion kernel's LDS with gradients, 12 M + 4 N bytes at the limit");

// ---- limits: each term states them once, as a function of its shape that answers nullptr or the refusal message (valid until the
// thread's next refusal).  dvm_*_term_workspace_bytes returns 0 exactly when it refuses; dvm_*_term_f32 raises its message.
static inline const char *frob_refusal(const char *fmt, ...) {
    static thread_local char msg[256];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(msg, sizeof msg, fmt, ap);
    va_end(ap);
    return msg;
}
#define FROB_LIMIT(cond, ...)                          \
    do {                                               \
        if (!(cond)) return frob_refusal(__VA_ARGS__); \
    } while (0)
// the limits every term has, the first ones every entry reports
#define FROB_BATCH_LIMITS(who, B, N, M)                                                       \
    FROB_LIMIT(B >= 1 && N >= 1 && M >= 1, "%s: empty input (B=%d N=%d M=%d)", who, B, N, M); \
    FROB_LIMIT(B <= 65535, "%s: B=%d unsupported (<= 65535)", who, B)
#define FROB_TOPK_LIMIT(who, k) FROB_LIMIT(k >= 1 && k <= 16, "%s: " #k "=%d unsupported (1..16)", who, k)

// ---- workspace: one double per row and the batch's F^2
struct FrobSums {
    double *partial;   // [B][N]: one per row
    float *f2;         // [B]
    void take(Arena &ar, int B, int N) {
        partial = ar.take<double>((size_t)B * N);
        f2 = ar.take<float>((size_t)B);
    }
};

// ---- the tail of every entry (dvm_frob.hip): partial [B][N] -> f2 -> loss [B], then each gradient array g [B][E] *= num / F (the
// first one may be NULL: loss only; a later NULL one is skipped), and the launch check under `name`
struct FrobGrad {
    float *g;
    size_t E;
};
int frob_finish(const FrobSums &w, int B, int N, double num, float *loss, std::initializer_list<FrobGrad> grads, const char *name, hipStream_t s);

// ---- device: sum over r of (row[r] - delta_ri)^2 of a row of N fp32 words in LDS, in float64, thread x over r = x, x + 256, ..,
// then the fixed tree; returned in every thread
__device__ __forceinline__ double frob_row_sq_sum(const float *row, int N, int i) {
    double acc = 0.0;
    for (int r = threadIdx.x; r < N; r += FROB_THREADS) {
        const double x = (double)row[r] - (r == i ? 1.0 : 0.0);
        acc += x * x;
    }
    return block_tree_sum(acc);
}

}  // namespace dvm
