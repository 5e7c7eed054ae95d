/*
 * dvm.h — C ABI of libdvm_hip.so: the MI355X (gfx950) implementation of
 * DV-Matcher's correspondence hot path.
 *
 * The reference has no FFI layer (it is pure Python/PyTorch); its boundary
 * for this path is the Python module API.  Each entry point
 * below names the reference function(s) it replaces (paths relative to the
 * reference checkout).  The Python mirror of the reference's modules in
 * dv-matcher_amd/{models,lib}/ binds these through ctypes; INTEGRATION.md
 * shows the stub a maintainer of the reference would add.
 *
 * Conventions
 *  - every function returns 0 on success or a negative DVM_E* code;
 *    dvm_last_error() returns a thread-local message for the last failure;
 *  - all tensor pointers are caller-owned DEVICE pointers, contiguous,
 *    row-major, fp32 / int32 (double where stated), 16-byte aligned;
 *  - `stream` is a hipStream_t (NULL = default stream); calls are
 *    asynchronous on it, never synchronise, never allocate (graph-capturable);
 *    scratch comes from the caller: query the size with *_workspace_bytes.
 *    The library keeps no per-call global state: kernel attributes are set once
 *    per (device, kernel) under a lock, and the only HIP objects it owns are the
 *    helper streams of dvm_pair_init / the events of dvm_profile_enable;
 *  - calls on distinct streams or devices may come from different host threads;
 *  - B is the batch (pairs or shapes); per-batch tensors are stacked on dim 0;
 *  - indices are 0-based int32.
 */
#ifndef DVM_H
#define DVM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DVM_ABI_VERSION 1

#define DVM_OK 0
#define DVM_EINVAL (-1)    /* bad argument (shape, null pointer, unsupported size) */
#define DVM_ELAUNCH (-2)   /* HIP launch / runtime error */
#define DVM_ENOSPACE (-3)  /* workspace too small */

/* The caller's collective for data-parallel statistics (the *_sync_f32 entry points): `allreduce` is called on the HOST while
 * the library enqueues its launches and must enqueue, ordered on `stream`, an IN-PLACE all-reduce over all ranks of `count`
 * elements at the device pointer `buf` (inside memory the caller handed to that entry point); dtype: 0 = float32, 1 = float64;
 * op: 0 = SUM, 1 = MIN, 2 = MAX.  Returns 0 on success.  (RCCL: ncclAllReduce(buf, buf, count, type, op, comm, stream);
 * torch.distributed: all_reduce of a view of the caller's tensor under torch.cuda.stream(ExternalStream(stream)).) */
typedef int (*dvm_allreduce_fn)(void *user, void *buf, size_t count, int dtype, int op, void *stream);
typedef struct dvm_collective {
    dvm_allreduce_fn allreduce;
    void *user;
} dvm_collective;

/* ---------------------------------------------------------------------------------------------------------------------
 * Environment options of the library: SIX variables, read once when the library is loaded (csrc/dvm_api.cpp::options()).
 * Nothing else in the library reads the environment; every option selects among HIP paths (there is no CPU path).
 * (The Python host side, dv-matcher_amd/, reads one variable of its own — DVM_RANK_CPUS, the host cores of a rank, set by
 * `bench.py --gpus N` — and no execution-path switches: those are module attributes and driver flags, listed in README.md.)
 *
 *   DVM_DETERMINISTIC=1        initial value of the dvm_set_deterministic flag (fixed summation order in LG-Net's backward)
 *   DVM_K1_ROUTE=0|1|3         force pass A of the soft correspondence at alpha >= 32: 0 full first form, 1 lean first form,
 *                              3 coarse screen; default: a probe picks per launch and direction, and a device-side gate sends a
 *                              direction the coarse screen serves badly through the lean form (results never depend on the route)
 *   DVM_K1_ROUTE_P="pc,pl"     the probe's thresholds (fractions of a row within the softmax cut; default 0.0014,0.02)
 *   DVM_LINEAR_CFG=0..7        tile configuration of dvm_linear_f32 (default: chosen per shape; all give the same bits:
 *                              tests/test_gpu_linear_cfgs.py)
 *   DVM_PAIR_OVERLAP=0         initial value of dvm_pair_set_overlap (helper-stream overlap of the pair forward)
 *   DVM_DEBUG=<bits>           synchronous diagnostics on stderr: 1 K1 routes per launch, 2 rows sent to the exact-rows kernel,
 *                              4 grid-Chamfer query statistics, 8 K1 coarse-screen cycle stamps, 16 Deformer-MLP cycle stamps
 * --------------------------------------------------------------------------------------------------------------------- */

int dvm_abi_version(void);
const char *dvm_last_error(void);
/* number of visible HIP devices (<=0: none) — lets callers fail loudly. */
int dvm_device_count(void);

/* Launch timing of the pair path's kernels with HIP events recorded on the stream each kernel is
 * launched on (bench.py's roofline legs; the reference has no counterpart: its profiling is
 * wall-clock around train.py's step, train.py:93-112).  enable pre-creates 2*max_launches events
 * and opens a window; the read functions synchronise on the window's events and return the summed
 * kernel time and bracket count of one slot (dvm_profile_read = slot DVM_PROF_K1_SWEEP); disable
 * closes the window.  dvm_profile_select chooses which slots record (bit k = slot k; default:
 * the sweep only, so the timed region of bench.py carries two event records per step). */
#define DVM_PROF_K1_SWEEP 0   /* pass A of K1: softcorr_sweep2_kernel, or softcorr_sweep_f16_kernel where the probe routes */
#define DVM_PROF_K1_REFINE 1  /* softcorr_refine_kernel (pass B: exact re-evaluation) */
#define DVM_PROF_MLP 2        /* mlp_f16x2_kernel (Deformer MLP) */
#define DVM_PROF_CHAMFER 3    /* grid_chamfer_kernel */
#define DVM_PROF_POOL 4       /* pool_kernel (Deformer Conv2d(k->1) pooling) */
#define DVM_PROF_KNN_XYZ 5    /* grid_knn_self_kernel (xyz kNN) */
#define DVM_PROF_FPS 6        /* fps_kernel */
#define DVM_PROF_ASSEMBLE 7   /* assemble_pooled_kernel (Deformer input rows) */
#define DVM_PROF_COUNT 8
int dvm_profile_enable(int max_launches);
int dvm_profile_select(unsigned kernel_mask);
int dvm_profile_read(double *total_ms, int *launches);
int dvm_profile_read_kernel(int kernel, double *total_ms, int *launches);
const char *dvm_profile_kernel_name(int kernel);
int dvm_profile_disable(void);

/* x.pow(2).sum(-1) in ATen's summation order (the |a|^2 terms of torch.cdist's
 * matmul form and of knn_new/knn: models/model.py:274-275, models/loss.py:458-459).
 * x [rows,K] -> out [rows]. */
int dvm_rownorm2_f32(const float *x, int rows, int K, float *out, void *stream);

/* 1x1 convolution / linear layer with its epilogue: nn.Conv1d(kernel_size=1) (+bias) -> [+ residual] ->
 * eval-mode nn.BatchNorm1d -> (Leaky)ReLU of LG-Net (models/model.py:506-529 conv..conv6 blocks, the ff / q / k / v
 * projections of N2PAttention[_DIM] 325-395, SA_Layer's q/k/v/trans_conv 97-123).
 * The contraction is the k-ordered fp32 fma chain acc = fma(w[co][k], x[k], acc) on v_mfma_f32_32x32x2_f32, restarted
 * and summed per K-block exactly like the CPU sgemm behind the reference's Conv1d / matmul (blocks of 384 while more
 * than 768 remain, then one block or two halves): bit-identical to the reference evaluated by one CPU thread,
 * independent of B, N and of the tile configuration.  Then, in this order:
 *   y += bias[co];  y += res;  y = fma(y, bn_alpha[co], bn_beta[co]);  y = y > 0 ? y : y * slope
 * (each step skipped when its pointer is NULL / slope == 1; slope 0 = ReLU; slope < 0 = ELU with alpha 1: y > 0 ? y : exp(y) - 1,
 * the Deformer's decoder MLP, models/model.py:433-452).
 *   channel_major == 0: x [B*N, K], y / res [B*N, Co]          (inference, activations point-major)
 *   channel_major == 1: x [B, K, N], y / res [B, Co, N]        (the reference's Conv1d layout, training forward)
 * w [Co, K]; K <= 8448 (16-byte aligned rows, K % 4 == 0, take the vector-load path). */
int dvm_linear_f32(const float *x, const float *w, int B, int N, int K, int Co, int channel_major, const float *bias,
                   const float *res, const float *bn_alpha, const float *bn_beta, float slope, float *y, void *stream);

/* The same layer (point-major) on rows [xg[b] (Cg) | x[b,n] (K - Cg)]: a 1x1 conv over torch.cat((g.repeat(1,1,N), x), 1)
 * without building the concatenation — conv3 / conv4 of Uni3FC.forward (models/model.py:735-747: the max-pooled
 * 512-vector of a shape in front of its 256 per-point channels), same K-blocked chain over the K = Cg + (K - Cg)
 * concatenated channels.  xg [B, Cg], x [B*N, K - Cg], w [Co, K], y / res [B*N, Co]; Cg % 4 == 0. */
int dvm_linear_prefix_f32(const float *xg, int Cg, const float *x, const float *w, int B, int N, int K, int Co,
                          const float *bias, const float *res, const float *bn_alpha, const float *bn_beta, float slope,
                          float *y, void *stream);

/* The "fixup" form of FeatUp's JBU stages (featup/upsamplers.py: `x + 0.1 * conv1x1(x')`):  y = res + scale * (x . w^T + bias)
 * in one launch, `res` laid out like y; the product is the same chain as dvm_linear_f32, then one multiply and one add
 * (two roundings, as the torch expression). */
int dvm_linear_scaled_residual_f32(const float *x, const float *w, int B, int N, int K, int Co, int channel_major, const float *bias,
                                   float scale, const float *res, float *y, void *stream);

/* Diagnostic, host only: what the most recent forward GEMM launch (the three entry points above, or a layer of a fused entry
 * point) of the calling host thread was.  No counterpart in the reference.  No device work, no synchronisation; DVM_EINVAL
 * before the first such launch on the thread.  info[0] channel_major, [1] the index launched in the tile-configuration table
 * (point-major 0..7, channel-major 0..3; for DVM_LINEAR_CFG=4..7 the register-staged twin 1, 1, 2, 3 where LDS-DMA staging does
 * not apply: K-blocks that are no multiples of 32, a row prefix, operands off the 16-byte grid), [2] 1 = LDS-DMA staging,
 * [3] number of K-blocks, [4] 1 = 16-byte operand loads along K, [5] 1 = 16-byte accesses in the epilogue, [6] row tiles,
 * [7] column tiles.  tests/test_gpu_linear_cfgs.py reads it to prove which instantiation a forced configuration ran. */
int dvm_linear_last_launch(int *info);

/* Weight gradient of the point-major layer above (what autograd computes for nn.Conv1d.weight in `loss.backward()`,
 * train.py:110):  dW[co][k] += sum_r gy[r][co] * x[r][k]  over the R = B*N rows; gy [R, Co], x [R, K], dW [Co, K] must be
 * ZEROED by the caller (row chunks are combined with fp32 atomics: summation order not fixed).  The input gradient of the
 * same layer needs no entry point of its own: dX = gy W is dvm_linear_f32(x := W as [1, Co, K], w := gy, channel_major = 1). */
int dvm_linear_wgrad_f32(const float *gy, const float *x, long R, int Co, int K, float *dW, void *stream);
/* The same weight gradient with an optional workspace (dvm_linear_wgrad_workspace_bytes): in the deterministic mode (below) every
 * row chunk writes its partial tile there and the tiles are added to dW in chunk order — bit-reproducible from run to run;
 * otherwise (or with ws == NULL) identical to dvm_linear_wgrad_f32. */
size_t dvm_linear_wgrad_workspace_bytes(long R, int Co, int K);
int dvm_linear_wgrad_ws_f32(const float *gy, const float *x, long R, int Co, int K, float *dW, void *ws, size_t ws_bytes, void *stream);

/* Deterministic gradient sums for LG-Net's backward (the reference's `loss.backward()`, train.py:110, sums in whatever order
 * its CUDA kernels' atomics land): on = 1 fixes the summation order of the three places that combine partial sums of different
 * workgroups with fp32 atomics — the row chunks of dvm_linear_wgrad_ws_f32, the split inner loop of dvm_sa_attention_bwd_f32, the
 * in-edge order of dvm_n2p_core_bwd_f32 — so that dvm_uni3fc_train_bwd_f32 returns the same bits on every run (measured:
 * LG-Net forward + backward, 2 x 8 x 2048 points, 18.5 ms instead of 14.3 ms).  Returns the previous setting; environment default DVM_DETERMINISTIC=1.  Process-wide. */
int dvm_set_deterministic(int on);
/* the current setting, read-only (a reader must not toggle the process-wide flag to learn it: another thread's backward could run in between) */
int dvm_get_deterministic(void);

/* Diagnostic, SYNCHRONOUS: which pass-A kernel of knnsearch_t_grad + topk_pi (models/loss.py:110-114, 1339-1347) the most recent
 * soft-correspondence launch of the calling host thread sent its (direction, pair) entries to — the probe and the gate decide on
 * the device, nothing else reads them back.  counts[0] full first form (3 fp16 products), [1] lean first form (3), [2] coarse
 * screen (1), [3] entries swept again by the lean form behind the coarse screen, [4] entries in all.  bench.py prices the
 * roofline line from it.  Waits for that launch's stream; valid only until its workspace is rewritten. */
int dvm_k1_last_routes(int *counts);

/* knnsearch_t_grad + topk_pi (+ the argmax map)  —  models/loss.py:110-114,
 * 1339-1347, 1404-1407.   D = cdist(f1,f2) (matmul form, bit-identical squared
 * distances); P = softmax(D*neg_alpha) over M; keep the `topk` largest of each
 * row, no renormalisation.  Sparse result, rows ordered by descending P
 * (ascending distance, ties -> lowest column):
 *   pi_val [B,N,topk], pi_idx [B,N,topk];
 *   row_smax [B,N] = max_j s_ij, row_sum [B,N] = sum_j exp(s_ij - smax)  (s = D*neg_alpha)
 * f1 [B,N,d], f2 [B,M,d]; neg_alpha = (float)(-alpha) < 0; 1 <= topk <= 16; d % 4 == 0, d <= 512.
 * variant: 0 = auto, 1 = scalar-FMA kernel, 2 = fp32-MFMA kernel (d == 128), 3 = sweep on the 16-bit matrix cores
 * over an exact 2-way fp16 split of the scaled features (3 partial products, fp32 accumulate) with exact fp32
 * re-evaluation of the 12 best columns per row and exact recompute of uncertified rows (d == 128, topk <= 10);
 * all variants give identical columns and row_smax. */
size_t dvm_softcorr_workspace_bytes(int B, int N, int M, int d);
int dvm_softcorr_fwd_f32(const float *f1, const float *f2, int B, int N, int M, int d, float neg_alpha, int topk,
                         float *pi_val, int32_t *pi_idx, float *row_smax, float *row_sum, int variant, void *ws,
                         size_t ws_bytes, void *stream);

/* Sinkhorn-normalised soft correspondence, forward, sparse top-k.  NOT in the reference (which has the row softmax above
 * only); pinned instead to dvm_softcorr_fwd_f32 at n_iter = 0 and to a float64 evaluation of this definition otherwise.
 * With D = cdist(f1,f2) formed exactly as above and S = D*neg_alpha, per batch entry:
 *   v = 0;  repeat n_iter times:  u_i = -LSE_j(S_ij + v_j);  v_j = log(N/M) - LSE_i(S_ij + u_i)
 *   L_ij = S_ij + v_j;  row_lmax_i = max_j L_ij;  row_sum_i = sum_j exp(L_ij - row_lmax_i)
 *   P_ij = exp(L_ij - row_lmax_i) / row_sum_i  (the last step is always a row step: rows of P sum to 1, columns approach N/M)
 *   u_i  = -(row_lmax_i + log(row_sum_i)),  so that P_ij = exp(S_ij + u_i + v_j)
 * pi_val / pi_idx [B,N,topk]: the topk largest of each row of P ranked by the logit L (descending, ties -> lowest column;
 * at n_iter = 0 by the distance, as dvm_softcorr_fwd_f32 ranks), no renormalisation, slots beyond M as (0, 0).
 * row_lmax, row_sum [B,N], u [B,N], v [B,M] may each be NULL.  n_iter = 0 returns what dvm_softcorr_fwd_f32 returns (and v = 0).
 * A fixed iteration count, no float atomics, no host synchronisation: capturable, and bit-reproducible from run to run.
 * f1 [B,N,d], f2 [B,M,d]; neg_alpha = (float)(-alpha) < 0; n_iter >= 0; 1 <= topk <= 16; d % 4 == 0, d <= 512.
 * variant: 0 = auto (fp32-MFMA sweeps for d == 128, else the scalar kernel), 1 = scalar-FMA kernel.  This entry keeps no
 * history; the differentiable pair follows. */
size_t dvm_sinkhorn_workspace_bytes(int B, int N, int M, int d);
int dvm_sinkhorn_fwd_f32(const float *f1, const float *f2, int B, int N, int M, int d, float neg_alpha, int n_iter,
                         int topk, float *pi_val, int32_t *pi_idx, float *row_lmax, float *row_sum, float *u, float *v,
                         int variant, void *ws, size_t ws_bytes, void *stream);

/* The differentiable pair of the Sinkhorn operator: the forward that keeps every iterate, and the exact gradient of the
 * unrolled, fixed-n_iter operator with respect to f1 and f2 (T = n_iter).
 * dvm_sinkhorn_fwd_hist_f32 runs dvm_sinkhorn_fwd_f32's sweeps on the same operands and leaves
 *   u_hist [B,T+1,N] = u^1 .. u^T, u^final      v_hist [B,T+1,M] = v^0 (= 0) .. v^T
 * pi_val, pi_idx, row_lmax, row_sum and the last slices of the histories equal dvm_sinkhorn_fwd_f32's outputs bit for bit.
 * dvm_sinkhorn_bwd_f32: given g_val [B,N,topk] = dL/d pi_val and the forward's pi_val, pi_idx, u_hist, v_hist, writes
 * d_f1 [B,N,d] and d_f2 [B,M,d] (overwritten, not accumulated).  A reverse sweep over the saved potentials, 2 n_iter
 * sweeps of the forward's kind for their adjoints and one row-major / column-major pair of passes for the features; no
 * N x M array is stored.  Entries with distance exactly 0 contribute 0, like cdist's backward.  No float atomics and no
 * host synchronisation (n_iter = 0 included): every output row is owned by one workgroup, two runs give the same bits,
 * and the call can be captured.  0 <= n_iter <= 32; other limits and variant as in the forward. */
size_t dvm_sinkhorn_hist_workspace_bytes(int B, int N, int M, int d);
int dvm_sinkhorn_fwd_hist_f32(const float *f1, const float *f2, int B, int N, int M, int d, float neg_alpha, int n_iter,
                              int topk, float *pi_val, int32_t *pi_idx, float *row_lmax, float *row_sum, float *u_hist,
                              float *v_hist, int variant, void *ws, size_t ws_bytes, void *stream);
size_t dvm_sinkhorn_bwd_workspace_bytes(int B, int N, int M, int d, int n_iter);
int dvm_sinkhorn_bwd_f32(const float *f1, const float *f2, int B, int N, int M, int d, float neg_alpha, int n_iter, int topk,
                         const float *pi_val, const int32_t *pi_idx, const float *u_hist, const float *v_hist,
                         const float *g_val, float *d_f1, float *d_f2, int variant, void *ws, size_t ws_bytes,
                         void *stream);

/* Unbalanced (KL-relaxed) Sinkhorn correspondence: relaxed marginals, per-point weights, the mass of every row.  NOT in the
 * reference.  The balanced operator above gives every source row mass 1, also a row that has no partner (partial shapes);
 * here every potential update is damped by tau = rho / (rho + 1/alpha) in (0, 1], and the final row step leaves a row whose
 * matches are all expensive with a small mass.  S as above; tau_row, tau_col in (0, 1]; log_a [B,N] (NULL = 0) and
 * log_b [B,M] (NULL = the constant log(N/M)) are the log weights of the two sides.  With T = n_iter, v^0 = 0, for t = 1..T:
 *   m^t_i = -LSE_j(S_ij + v^(t-1)_j)     u^t_i = tau_row (log_a_i + m^t_i)
 *   n^t_j = -LSE_i(S_ij + u^t_i)         v^t_j = tau_col (log_b_j + n^t_j)
 * and the final row step
 *   m^f_i = -LSE_j(S_ij + v^T_j)     u^f_i = tau_row (log_a_i + m^f_i)     L_ij = S_ij + v^T_j
 *   P_ij = exp(S_ij + u^f_i + v^T_j)     row_lmass_i = u^f_i - m^f_i = log sum_j P_ij
 * pi_val / pi_idx [B,N,topk]: the topk largest of each row of P ranked by L; ranking, tie rule and the (0, 0) slots beyond M
 * as in dvm_sinkhorn_fwd_f32; no renormalisation.  row_lmax, row_sum (of L, as above), row_lmass [B,N], u = u^f [B,N],
 * v = v^T [B,M] may each be NULL.  The mass is returned as a logarithm: at alpha = 100 on unnormalised features it is e^-100
 * and smaller; pi_val may then be 0, it is never NaN or Inf.  tau_row = tau_col = 1 with both weights NULL is
 * dvm_sinkhorn_fwd_f32, bit for bit (and row_lmass = 0).  Every potential is formed as tau * (log weight + normaliser), a sum
 * and then a product in fp32.
 * dvm_sinkhorn_ub_fwd_hist_f32 is the same run, keeping the normalisers:
 *   rn_hist [B,T+1,N] = m^1 .. m^T, m^f      cn_hist [B,T+1,M] = 0, n^1 .. n^T
 * (the potentials are re-made from them by the expression above wherever they are needed: u / tau - log_a is not the same
 * number in fp32); its pi_val, pi_idx, row_* equal dvm_sinkhorn_ub_fwd_f32's bit for bit.
 * dvm_sinkhorn_ub_bwd_f32: the exact gradient of the unrolled operator.  Given g_val [B,N,topk] = dL/d pi_val, g_lmass [B,N]
 * = dL/d row_lmass (NULL = 0), the forward's pi_val, pi_idx, row_lmass and the two histories, with gp_t = g_t val_t,
 * G_i = sum_t gp_t, R^f_ij = exp(S_ij + m^f_i + v^T_j) and H_i = tau_row G_i - (1 - tau_row) g_lmass_i:
 *   Sbar_ij = [j = idx_t] gp_t - H_i R^f_ij - sum_t ( nbar^t_j Q^t_ij + mbar^t_i R^t_ij )
 *   Q^t_ij = exp(S_ij + u^t_i + n^t_j)     R^t_ij = exp(S_ij + m^t_i + v^(t-1)_j)
 *   vbar^T_j = sum_i ([j = idx_t] gp_t - H_i R^f_ij)     nbar^t = tau_col vbar^t     ubar^t_i = -sum_j nbar^t_j Q^t_ij
 *   mbar^t = tau_row ubar^t     vbar^(t-1)_j = -sum_i mbar^t_i R^t_ij
 *   d_log_a_i = tau_row (G_i + g_lmass_i) + sum_t mbar^t_i     d_log_b_j = sum_t nbar^t_j
 * d_f1 [B,N,d], d_f2 [B,M,d] from W = neg_alpha Sbar / D as in dvm_sinkhorn_bwd_f32 (entries with D = 0 contribute 0);
 * d_log_a [B,N], d_log_b [B,M] may be NULL.  All are overwritten.  Every exponent is that of a probability, built from the
 * step's own normaliser.  Structure, limits (n_iter <= 32), variants and guarantees (no float atomics, no host
 * synchronisation, capturable, the same bits from run to run) as dvm_sinkhorn_bwd_f32.  At tau = 1 this is the balanced
 * gradient computed from the normalisers; it is not bit-equal to dvm_sinkhorn_bwd_f32. */
size_t dvm_sinkhorn_ub_workspace_bytes(int B, int N, int M, int d);
int dvm_sinkhorn_ub_fwd_f32(const float *f1, const float *f2, int B, int N, int M, int d, float neg_alpha, int n_iter, int topk,
                            float tau_row, float tau_col, const float *log_a, const float *log_b, float *pi_val,
                            int32_t *pi_idx, float *row_lmax, float *row_sum, float *row_lmass, float *u, float *v, int variant,
                            void *ws, size_t ws_bytes, void *stream);
size_t dvm_sinkhorn_ub_hist_workspace_bytes(int B, int N, int M, int d);
int dvm_sinkhorn_ub_fwd_hist_f32(const float *f1, const float *f2, int B, int N, int M, int d, float neg_alpha, int n_iter,
                                 int topk, float tau_row, float tau_col, const float *log_a, const float *log_b, float *pi_val,
                                 int32_t *pi_idx, float *row_lmax, float *row_sum, float *row_lmass, float *rn_hist,
                                 float *cn_hist, int variant, void *ws, size_t ws_bytes, void *stream);
size_t dvm_sinkhorn_ub_bwd_workspace_bytes(int B, int N, int M, int d, int n_iter);
int dvm_sinkhorn_ub_bwd_f32(const float *f1, const float *f2, int B, int N, int M, int d, float neg_alpha, int n_iter, int topk,
                            float tau_row, float tau_col, const float *log_a, const float *log_b, const float *pi_val,
                            const int32_t *pi_idx, const float *row_lmass, const float *rn_hist, const float *cn_hist,
                            const float *g_val, const float *g_lmass, float *d_f1, float *d_f2, float *d_log_a, float *d_log_b,
                            int variant, void *ws, size_t ws_bytes, void *stream);

/* Backward of dvm_softcorr_fwd_f32 (autograd through models/loss.py:110-114 + the top-k keep of
 * 1339-1347): given g_val [B,N,topk] = dL/d pi_val and the forward's outputs (pi_val, pi_idx, row_smax,
 * row_sum), writes d_f1 [B,N,d] and d_f2 [B,M,d] (overwritten, not accumulated).  The dense N x M term is
 * recomputed tile by tile (never stored); rows with distance exactly 0 contribute 0, like cdist's backward.
 * Sums over rows/columns use fp32 atomics (order not fixed).  variant as in the forward. */
size_t dvm_softcorr_bwd_workspace_bytes(int B, int N, int M, int d);
int dvm_softcorr_bwd_f32(const float *f1, const float *f2, int B, int N, int M, int d, float neg_alpha, int topk,
                         const float *pi_val, const int32_t *pi_idx, const float *row_smax, const float *row_sum,
                         const float *g_val, float *d_f1, float *d_f2, int variant, void *ws, size_t ws_bytes,
                         void *stream);

/* knnsearch_t / search_t — models/loss.py:91-95,121-124; test.py:19-28.
 * T[b,i] = argmin_j cdist(f1,f2, 'donot_use_mm_for_euclid_dist') (0-based; the
 * test scripts add 1), ties -> lowest j; dmin [B,N] optional (may be NULL).
 * With a workspace and d == 128 the columns are first screened by the matrix-core sweep of the soft correspondence
 * and only those that can still be the minimum are evaluated in the exact-difference form (same result, ~50x
 * faster at N = M = 4995); ws == NULL evaluates every column.  dvm_argmin_pair_f32 returns both maps of a pair
 * (T12 [B,N] into f2, T21 [B,M] into f1) from ONE sweep launch, as test.py needs them. */
size_t dvm_argmin_workspace_bytes(int B, int N, int M, int d, int both_directions);
int dvm_argmin_exact_f32(const float *f1, const float *f2, int B, int N, int M, int d, int32_t *T, float *dmin,
                         void *ws, size_t ws_bytes, void *stream);
int dvm_argmin_pair_f32(const float *f1, const float *f2, int B, int N, int M, int d, int32_t *T12, int32_t *T21,
                        float *dmin12, float *dmin21, void *ws, size_t ws_bytes, void *stream);

/* The precise (vertex-to-point) map beside the vertex map above: the closest point of the target's triangle mesh embedded
 * in feature space.  Not in the reference, which stops at knnsearch_t.
 * f1 [B,N,d], f2 [B,M,d] fp32 (rows 16-byte aligned), faces [F,3] int32, one connectivity shared by the B entries.  For every
 * (b,i), p = f1[b,i]: over all faces (a,b,c) whose three indices lie in [0,M), q = the point of the triangle f2[b,a], f2[b,b],
 * f2[b,c] in R^d closest to p; the face with the smallest distance wins, ties in the compared fp32 value go to the lowest face
 * index.  The compared value is the exact-difference form: per face the closest point of each edge as a segment and, where the
 * face's Gram determinant exceeds its own rounding (det > 2^-21 e11 e22), the interior projection if all its weights are >= 0;
 * for each the residual (f2[a] - p) + s (f2[b] - f2[a]) + t (f2[c] - f2[a]) is formed and its squared norm summed by a k-ordered
 * fmaf chain.  A face with a repeated index or collinear features is the union of its edges: a valid candidate, never a NaN.  A
 * face whose value is NaN never wins (NaN counts as +inf, as in dvm_dg_skin_geod_f32).  A face with an index outside [0,M) is
 * left out and counted.
 * Outputs: face [B,N] int32; bary [B,N,3] (each >= 0, summing to 1 within 4 ulp, in the vertex order of the face);
 * pi_idx [B,N,3] = faces[face] — (bary, pi_idx) is the (pi_val, pi_idx) layout of dvm_sparse_apply_f32 and the loss terms;
 * dist [B,N] = |p - q| (may be NULL); stats [2] int64 on the device (may be NULL): faces left out, exact evaluations made.  A
 * row with no admissible face gets face = -1, bary = 0, pi_idx = 0, dist = +inf; a row whose best value is +inf (a non-finite
 * row, or non-finite corners everywhere) gets the lowest admissible face with bary = (1,0,0) and dist = +inf.
 * Limits: d % 4 == 0, 4 <= d <= 512, M <= dvm_precise_map_max_m() (8192: the row's products with every target vertex are held
 * in LDS), B <= 65535, all sizes >= 1; outside them, or with a null required pointer, DVM_EINVAL and a size query of 0; a short
 * workspace DVM_ENOSPACE; both before anything is launched.
 * The faces are screened by the Gram form and every face within a proved error band of the row's minimum is evaluated in the
 * exact form (csrc/dvm_precise_map.hip derives the band): the result is the exact form's arg-min over all faces.  Asynchronous
 * on `stream`, no host synchronisation, no float atomics, the same bits from run to run, capturable.
 * dvm_precise_map_plan reports, without a device, the source rows and threads per workgroup, the target rows per step of the
 * LDS fill and the cap on M. */
int dvm_precise_map_max_m(void);
int dvm_precise_map_plan(int B, int N, int M, int d, int F, int *rows, int *threads, int *chunk, int *max_m);
size_t dvm_precise_map_workspace_bytes(int B, int N, int M, int d, int F);
int dvm_precise_map_f32(const float *f1, const float *f2, const int32_t *faces, int B, int N, int M, int d, int F, int32_t *face,
                        float *bary, int32_t *pi_idx, float *dist, int64_t *stats, void *ws, size_t ws_bytes, void *stream);

/* knn_grad — models/loss.py:97-101: the k smallest of cdist(x,y) (matmul form)
 * per row, ascending.  x [B,N,C], y [B,M,C] -> idx [B,N,k]; C <= 16, k <= 16.  A 3-D cloud against
 * itself (x == y) is searched exactly on a uniform grid; otherwise brute force (ws may be NULL). */
size_t dvm_knn_cdist_workspace_bytes(int B, int N, int M, int C);
int dvm_knn_cdist_f32(const float *x, const float *y, int B, int N, int M, int C, int k, int32_t *idx, void *ws,
                      size_t ws_bytes, void *stream);

/* knn_new / knn — models/model.py:267-278, models/loss.py:451-462: the k largest of
 * (-|a|^2 - (-2 a.b)) - |b|^2 per row, descending (ties -> lowest column).
 * a [B,N,C], b [B,M,C] -> idx [B,N,k]; k <= min(512, M), M <= 8192.  C in {64,128} uses the
 * fp32 matrix cores; any other C a scalar kernel. */
size_t dvm_knn_neg_workspace_bytes(int B, int N, int M, int C, int k);
int dvm_knn_neg_f32(const float *a, const float *b, int B, int N, int M, int C, int k, int32_t *idx, void *ws,
                    size_t ws_bytes, void *stream);

/* knnsearch_t_grad as a dense matrix — models/loss.py:110-114 (compatibility entry; the
 * criterion uses dvm_softcorr_fwd_f32).  P [B,N,M] = softmax(cdist(f1,f2) * neg_alpha). */
size_t dvm_softcorr_dense_workspace_bytes(int B, int N, int M, int d);
int dvm_softcorr_dense_f32(const float *f1, const float *f2, int B, int N, int M, int d, float neg_alpha, float *P,
                           void *ws, size_t ws_bytes, void *stream);

/* Pi~ @ V for the sparse Pi~ — models/loss.py:1408-1409 (verts), models/model.py:471
 * (pooled features).  out[b,i,:] = sum_t val[b,i,t] * V[b, idx[b,i,t], :], summed in
 * ascending column order.  V [B,M,C] -> out [B,N,C]. */
int dvm_softcorr_apply_f32(const float *pi_val, const int32_t *pi_idx, const float *V, int B, int N, int M, int topk,
                           int C, float *out, void *stream);

/* Backward of dvm_softcorr_apply_f32: g_out [B,N,C] -> d_val [B,N,topk] = g_out[i] . V[idx[i,t]] and
 * d_V [B,M,C] (overwritten).  With a workspace the (row, slot) -> target lists are reversed by a counting sort
 * and every target row gathers its in-edges (no float atomics); ws == NULL scatter-accumulates with fp32 atomics.
 * C <= 256, topk <= 64. */
size_t dvm_softcorr_apply_bwd_workspace_bytes(int B, int N, int M, int topk);
int dvm_softcorr_apply_bwd_f32(const float *pi_val, const int32_t *pi_idx, const float *V, const float *g_out, int B,
                               int N, int M, int topk, int C, float *d_val, float *d_V, void *ws, size_t ws_bytes,
                               void *stream);

/* The rank term of the criterion — models/loss.py:1427-1433: loss[b] = ||P P^T - I_N||_F for the sparse top-k correspondence
 * P [N,M] given as pi_val / pi_idx [B,N,topk], and (g_val != NULL) g_val [B,N,topk] = d loss[b] / d pi_val.
 * PRECONDITION: the indices of a row lie in [0, M) and are distinct within the row — what every top-k producer of this library
 * emits (softcorr, sinkhorn, their unbalanced forms).  Repeated slots are harmless only where their value is 0 (the (0, 0) slots
 * of a row with M < topk); an index outside [0, M) contributes nothing.  Values need not be normalised.
 * Neither P^T P nor P P^T is formed.  With S = P P^T,
 *   F^2 = sum_i [ (S_ii - 1)^2 + sum_{i' != i} S_ii'^2 ]
 * is evaluated row by row: nothing cancels.  Row i of S is non-zero only at rows that share a column with row i; the entries of
 * every column come from the reversed lists of dvm_softcorr_apply_bwd_f32.  One workgroup per row keeps the row of S in LDS
 * (fp32, every entry an fma chain of at most topk terms in slot order), reduces its squared residual in float64, and for the
 * gradient sums  dF^2 / d pi_val[i,t] = 4 sum_i' (S - I)[i,i'] P[i', pi_idx[i,t]]  over the column's list in 64-bit fixed point
 * (units of 2^-50 of the list's largest term, found by a first walk: the float64 terms added as integers, so the order of the
 * lists, which integer atomics set, cannot reach the result; quantisation at most N 2^-50 of that term).  Row sums
 * are reduced per batch element in float64, fixed order; loss = sqrt(F^2) and g_val = (dF^2 / d pi_val) / (2 loss).  Where
 * loss[b] == 0 (an exact permutation) g_val[b] is 0, torch.norm's gradient at zero.
 * Work: sum_j c_j^2 for the column counts c_j (with g_val: three walks of the lists instead of one), N LDS words per row.  Memory: the workspace only,
 * 4 B (2 M + N topk) + 8 B N bytes — no N x N, M x M or N x M array.  No float atomics, no host synchronisation, capturable, the
 * same bits from run to run and for a batch element alone or in a batch.
 * Limits: N <= dvm_rank_term_max_n() (8192, the criterion's own gate: the row must fit LDS), any M, topk <= 16,
 * B <= 65535.  Outside them dvm_rank_term_workspace_bytes returns 0 and dvm_rank_term_f32 DVM_EINVAL, before any launch. */
int dvm_rank_term_max_n(void);
size_t dvm_rank_term_workspace_bytes(int B, int N, int M, int topk);
int dvm_rank_term_f32(const float *pi_val, const int32_t *pi_idx, int B, int N, int M, int topk, float *loss,
                      float *g_val /* may be NULL */, void *ws, size_t ws_bytes, void *stream);

/* The cycle term of a pair's two correspondences (not in the reference, whose loss terms each look at one direction):
 * loss[b] = ||P12 P21 - I_N||_F for the sparse top-k P12 [N,M] given as val12 / idx12 [B,N,k12] (columns in [0, M)) and
 * P21 [M,N] given as val21 / idx21 [B,M,k21] (columns in [0, N)); N != M is allowed.  With C = P12 P21 (N x N), R = C - I_N and
 * F = ||R||_F, the gradients (g12, g21: both NULL or both given) are
 *   g12[i,t] = d F / d val12[i,t] = (1/F) sum_s R[i, idx21[j,s]] val21[j,s],   j = idx12[i,t]
 *   g21[j,s] = d F / d val21[j,s] = (1/F) sum_{(i,t): idx12[i,t] = j} val12[i,t] R[i, idx21[j,s]]
 * and both are exactly 0 where F == 0 (the two maps are mutual inverses), torch.norm's gradient at zero.
 * PRECONDITION: the indices of a row are distinct within the row — what every top-k producer of this library emits.  An index
 * outside its range contributes nothing (to C or to either gradient; it never becomes an address), and a slot whose value is 0
 * is skipped when C is formed, so the repeated (0, 0) slots of a row with fewer columns than topk are harmless.  Values need not
 * be normalised.
 * No dense array is formed.  One workgroup per row i keeps row i of C in LDS (fp32, every entry an fma chain of at most k12 terms
 * in slot order: C[i,c] += val12[i,t] val21[j,s] at c = idx21[j,s]), reduces the squared residual in float64 and, for the
 * gradients, adds g12[i,t]'s k21 terms in slot order in float64 and leaves the k12 k21 entries C[i, idx21[idx12[i,t], s]] in the
 * workspace.  g21 needs one of them from every row that picks column j: one wave per column walks the reversed list of idx12
 * (as dvm_softcorr_apply_bwd_f32's) and sums in 64-bit fixed point, units of 2^-50 of the list's largest term, found by a first
 * walk, so the order of the list, which integer atomics set, cannot reach the result (as dvm_rank_term_f32's gradient).  Row
 * sums are reduced per batch element in float64, fixed order; loss = sqrt(F^2), both gradients are scaled by 1 / F.
 * The loss-only call builds no lists and leaves no samples, and gives the loss bits of the call with gradients.
 * Memory: the workspace only, 4 B (2 M + N k12) + 8 B N + 4 B N k12 k21 bytes — no N x N, N x M or M x M array.  No float
 * atomics, no host synchronisation, capturable, the same bits from run to run and for a batch element alone or in a batch.
 * Limits: N <= dvm_cycle_term_max_n() (8192: the row must fit LDS), any M, 1 <= k12, k21 <= 16, B <= 65535.  Outside them
 * dvm_cycle_term_workspace_bytes returns 0 and dvm_cycle_term_f32 DVM_EINVAL, before any launch. */
int dvm_cycle_term_max_n(void);
size_t dvm_cycle_term_workspace_bytes(int B, int N, int M, int k12, int k21);
int dvm_cycle_term_f32(const float *val12, const int32_t *idx12, const float *val21, const int32_t *idx21, int B, int N, int M,
                       int k12, int k21, float *loss, float *g12 /* may be NULL */, float *g21 /* may be NULL */, void *ws,
                       size_t ws_bytes, void *stream);

/* The geodesic distortion term of a correspondence (not in the reference, which uses the two distance matrices only for its
 * anchor-sampled cosine): loss[b] = ||P D2 P^T - D1||_F for the sparse top-k P [N,M] given as pi_val / pi_idx [B,N,topk] (columns in
 * [0, M)), the source shape's distance matrix D1 = dist_src [B,N,N] and the target's D2 = dist_tgt [B,M,M]; N != M is allowed.
 * With S = P D2 P^T (N x N), R = S - D1 and F = ||R||_F the gradient (g_val != NULL) is
 *   g_val[i,t] = d F / d pi_val[i,t] = (2/F) sum_m D2[c,m] q_i[m],   c = pi_idx[i,t],   q_i[m] = sum_{(j,s): pi_idx[j,s] = m} pi_val[j,s] R[i,j]
 * (the halves of the derivative that come from row i and from column i of S are equal), exactly 0 where F == 0 (an exact
 * isometry), torch.norm's gradient at zero.  The distance matrices are constants: no gradient is formed for them.
 * PRECONDITIONS: D1 and D2 are finite and SYMMETRIC (the entry does not symmetrise and does not check; the formula above is the
 * gradient only then); the indices of a row are distinct within the row — what every top-k producer of this library emits.  An
 * index outside [0, M) contributes nothing (to S or to the gradient, whose element for that slot is 0; it never becomes an
 * address), and a slot whose value is 0 adds nothing to S.  Values need not be normalised.
 * No dense product is formed.  One workgroup per row i: u_i[m] = sum_t pi_val[i,t] D2[pi_idx[i,t], m] in LDS (fp32, an fma chain in
 * slot order over topk coalesced rows of D2), then S[i,j] = sum_s pi_val[j,s] u_i[pi_idx[j,s]] for every j (an fma chain in slot
 * order), the residual against the row of D1 and its squared sum in float64.  For the gradient the residual row stays in LDS
 * (fp32) and q_i is summed there in 64-bit fixed point, units of 2^-50 of every column's largest term, found by a first sweep: LDS
 * integer maxima and integer adds, which commute, so no order of arrival can reach the result (as the fixed-point sums of
 * dvm_rank_term_f32, without the reversed lists); topk more rows of D2 are then dotted with q_i in float64.  Row sums are
 * reduced per batch element in float64, fixed order; loss = sqrt(F^2), the gradient is scaled by 2 / F.  The loss-only call
 * keeps no residual row and gives the loss bits of the call with gradients.
 * Work per row: 2 topk rows of D2 (topk without g_val), one sweep over P (three with g_val), one row of D1.
 * Memory: the workspace only, 8 B N + 4 B bytes — no N x N, N x M or M x M array.  LDS per workgroup: 12 M + 4 N bytes with
 * g_val, 4 M without.  No float atomics, no host synchronisation, capturable, the same bits from run to run and for a batch
 * element alone or in a batch.
 * Limits: N, M <= dvm_distortion_term_max_n() (8192: the rows must fit LDS), 1 <= topk <= 16, B <= 65535.  Outside them
 * dvm_distortion_term_workspace_bytes returns 0 and dvm_distortion_term_f32 DVM_EINVAL, before any launch. */
int dvm_distortion_term_max_n(void);
size_t dvm_distortion_term_workspace_bytes(int B, int N, int M, int topk);
int dvm_distortion_term_f32(const float *pi_val, const int32_t *pi_idx, const float *dist_src /* [B,N,N] */,
                            const float *dist_tgt /* [B,M,M] */, int B, int N, int M, int topk, float *loss /* [B] */,
                            float *g_val /* [B,N,topk], may be NULL */, void *ws, size_t ws_bytes, void *stream);

/* The weighted neighbour matrix of a source shape in CSR: the operator of dvm_dirichlet_term_f32 (not in the reference).  Per
 * batch element rowptr [N+1], col [Ecap] int32, w [Ecap] fp32 — batched as [B][..] with one Ecap — norm [B] (the energy of the
 * shape's own coordinates under the operator, closed form) and stats [B][4] int32: owners of entries left out for an index
 * outside [0, N); for degenerate geometry; self entries (the list builder only); entries kept (= rowptr[N]).  The entries are a
 * multiset (duplicates of (i, j) are kept) and every entry (i, j, w) has its mirror (j, i, w).  Both builders number their
 * CANDIDATE entries in a fixed way and a row holds its kept candidates in ASCENDING CANDIDATE NUMBER (the ordered counting sort of
 * csrc/dvm_revlist.hip: no atomic's order reaches the arrays, and nothing is sorted by value); col / w behind rowptr[N] are -1 / 0.
 * Everything is evaluated in float64 and rounded once; tests/dirichlet_term_ref.py states the same in numpy.
 * dvm_mesh_laplacian_f32: verts [B,N,3] fp32, faces [F,3] int32 shared by the batch, Ecap = 6 F.  Corner c of face f, at vertex
 * v = face[c] with a = face[(c+1)%3], b = face[(c+2)%3], u = a - v, v' = b - v: candidates 6f+2c = (a, b, w) and 6f+2c+1 = (b, a, w),
 * w = fp32(cot / 2), cot = (u . v') / |u x v'| (negative at an obtuse corner, kept).  A face with an index outside [0, N), or whose
 * |u x v'|^2 is 0 or not finite at any corner, is left out whole and counted.  mass [B,N] = one third of the areas of the kept
 * faces at the vertex, summed in ascending face order; norm = 2 x the total area of the kept faces (area = |u x v'| / 2 at
 * corner 0), which is the Dirichlet energy of the embedding itself.  A vertex without faces has an empty row.
 * dvm_knn_laplacian_f32: xyz [B,N,3], nbr [B,N,K] int32 (dvm_knn_cdist_f32's lists, self included), Ecap = 2 N K.  Slot s of
 * point i, j = nbr[i,s]: candidates 2(iK+s) = (i, j, w) and 2(iK+s)+1 = (j, i, w) — the operator is W + W^T, a mutual pair appears
 * twice in each row.  mode 0 ("stretch"): w = fp32(1 / |x_i - x_j|^2), norm = half the number of kept entries (E / norm is then the
 * mean squared local stretch); mode 1 ("uniform"): w = 1, norm = 1/2 sum w |x_i - x_j|^2 (per row in row order, the rows through
 * the fixed tree).  Left out and counted: j == i; j outside [0, N); in mode 0 a squared distance that is 0 or not finite.
 * Limits: N <= 24576 (one counter per row in LDS), B <= 65535, 1 <= K <= 64, 6 F and 2 N K below 2^30; outside them, DVM_EINVAL and
 * a size query of 0, before any launch.  No float atomics, no host synchronisation, capturable, the same bits from run to run. */
size_t dvm_mesh_laplacian_workspace_bytes(int B, int N, int F);
int dvm_mesh_laplacian_f32(const float *verts, const int32_t *faces, int B, int N, int F, int32_t *rowptr, int32_t *col, float *w,
                           float *norm, float *mass, int32_t *stats, void *ws, size_t ws_bytes, void *stream);
size_t dvm_knn_laplacian_workspace_bytes(int B, int N, int K, int mode);
int dvm_knn_laplacian_f32(const float *xyz, const int32_t *nbr, int B, int N, int K, int mode, int32_t *rowptr, int32_t *col, float *w,
                          float *norm, int32_t *stats, void *ws, size_t ws_bytes, void *stream);

/* The Dirichlet energy of a correspondence under such an operator (not in the reference): with Y = P V for the sparse top-k
 * P [N,M] given as pi_val / pi_idx [B,N,topk] and the target's values V [B,M,C] (its coordinates: C = 3),
 *   loss[b] = E = 1/2 sum over the entries (i, j, w) of w |y_i - y_j|^2,
 *   g_val[i,s] = dE / d pi_val[i,s] = (2 sum over the entries of row i of w (y_i - y_j)) . V[pi_idx[i,s]]   (g_val != NULL)
 * — the gradient exactly under the operator's structural symmetry (not checked).  V and the operator are constants.  The loss
 * is E itself (no square root); E / norm is 1 for a map that keeps local lengths.
 * Y has the bits of dvm_softcorr_apply_f32 (its launches, into the workspace); everything after it is accumulated in float64 in CSR
 * order: a group of 4, 8 or 16 lanes per row, one lane per channel, every lane walks the row's entries in order; the channels
 * are joined by a fixed butterfly, the rows by the fixed-order reduction of the other loss terms.  A slot with pi_idx outside
 * [0, M) and an entry with col outside [0, N) contribute nothing and never become an address (the slot's g_val is 0); rowptr is
 * clamped to [0, Ecap].  No N x N or N x M array, no LDS, no float atomics, no host synchronisation, capturable, the same bits
 * from run to run, with or without g_val, and for a batch element alone or in a batch.  Workspace: 4 B N (C + 2 topk) + 8 B N.
 * Limits: 1 <= topk <= 16, 1 <= C <= 16, B <= 65535, N, M <= 2^24, Ecap >= 1.  Outside them dvm_dirichlet_term_workspace_bytes
 * returns 0 and dvm_dirichlet_term_f32 DVM_EINVAL, before any launch. */
size_t dvm_dirichlet_term_workspace_bytes(int B, int N, int M, int topk, int C, int Ecap);
int dvm_dirichlet_term_f32(const float *pi_val, const int32_t *pi_idx, const float *V /* [B,M,C] */, const int32_t *rowptr /* [B,N+1] */,
                           const int32_t *col /* [B,Ecap] */, const float *w /* [B,Ecap] */, int B, int N, int M, int topk, int C,
                           int Ecap, float *loss /* [B] */, float *g_val /* [B,N,topk], may be NULL */, void *ws, size_t ws_bytes,
                           void *stream);

/* The Laplace-Beltrami eigenbasis of such an operator: the first k eigenpairs of L phi = lambda M phi (the reference's
 * Tools/mesh.py::mesh.spectral, which calls a sparse shift-invert solver on the host; here everything runs on the device).
 * Inputs: the CSR operator exactly as the two builders emit it (rowptr [B,N+1], col / w [B,Ecap], a symmetric multiset of entries,
 * duplicates kept) and mass [B,N] fp32, or NULL for a mass of 1 everywhere.
 * Active set: a vertex is ACTIVE when its mass is finite and > 0.  An entry whose column lies outside [0, N) or is inactive
 * contributes nothing and never becomes an address; rowptr is clamped to [0, Ecap].
 * Operator, in float64 from the fp32 inputs, with s_i = m_i^-1/2 on active rows:
 *   (L x)_i = sum over the entries e of row i of w_e (x_i - x_col(e))
 *   (A y)_i = s_i sum_e w_e (s_i y_i - s_j y_j),  j = col(e)          (A = S L S, symmetric)
 *   phi = s * y, so that Phi^T M Phi = I; the rows of inactive vertices are 0
 *   beta = max over active i of s_i^2 (|sum_e w_e| + sum_e |w_e|)      (a Gershgorin bound of A; cotangent weights may be negative)
 * Outputs: evals [B,k] ascending, float64; evecs [B,N,k] float64, every column's sign fixed so that its entry of largest magnitude
 * is positive (the lowest index wins a tie); res [B,k] float64, res_j = |A y_j - theta_j y_j|_2 / beta of the RETURNED pair;
 * info [B,4] int32 = outer iterations run, converged (1 / 0), inactive vertices, operator applications.
 * Convergence: an element has converged when max_j res_j <= tol.  An element that reaches max_iter returns its current Ritz pairs
 * with info[1] = 0 and truthful res: the caller decides what a basis that has not converged is worth.
 * Method: Chebyshev-filtered subspace iteration on a block of m = k + guard columns.  Per outer iteration: Rayleigh-Ritz (H = X^T A X,
 * a parallel-ordered cyclic Jacobi eigensolver, eigenvalues ascending with ties by column number, X <- X Q, residuals from a fresh
 * A X); a degree-`degree` Chebyshev filter that damps [theta_m, 1.01 beta], scaled at theta_1 (one launch per degree:
 * Y' = a (A Y - c Y) - b X, a row's entries walked in CSR order); Cholesky-QR twice, each on the Gram matrix scaled to a unit
 * diagonal.  A Cholesky pivot that is not a positive finite number fails the call (DVM_ELAUNCH), it does not produce NaNs.  The
 * start block is a counter-based hash of (vertex, column) alone.  Every sum has one fixed order and there are no float atomics:
 * an element gives the same bits alone or in a batch, and from run to run; the workgroups of a converged element leave at once.
 * Slow case: when lambda_k and lambda_{k+guard} lie in one near-degenerate cluster the filter cannot separate them and many outer
 * iterations are needed; move k or guard off the cluster, or raise degree / max_iter.
 * THE ENTRY WAITS FOR ITS STREAM: like dvm_mesh_geodesics_f64 it is a dataset-time call.  It reads the B state rows back once per
 * outer iteration and stops launching when every element is done, so it is NOT capturable.  This is its only synchronisation.
 * An element with fewer than k + guard active vertices, or whose beta is 0 or not finite, fails the call (DVM_EINVAL) at the first
 * read-back; the outputs are then not written.
 * Limits: 1 <= k, guard >= 1, k + guard <= min(N, dvm_eigenbasis_max_block() = 128), 1 <= degree <= 256, max_iter >= 1, tol > 0,
 * N <= 2^24, B <= 65535, Ecap >= 1.  Outside them DVM_EINVAL (and a size query of 0 for the sizes it takes), before any launch.
 * Workspace: three [B,N,m] float64 blocks, 16 B N bytes of row data, min(64, ceil(N / 32)) + 3 m x m matrices per element.
 *
 * dvm_basis_project_f64: out[b] = Phi[b]^T diag(mass[b]) Y[b] for Phi [B,N,k] float64, Y [B,N,C] fp32, out [B,k,C] float64 (mass
 * NULL: 1; a mass that is not a positive finite number counts as 0) — the solver's weighted tall-skinny product: rows added in
 * ascending order within min(64, ceil(N / 32)) chunks, the chunks in ascending order.  Capturable, no synchronisation, no float
 * atomics.  Limits: k, C <= 128, N <= 2^24, B <= 65535; outside them DVM_EINVAL and a size query of 0. */
int    dvm_eigenbasis_max_block(void);
size_t dvm_eigenbasis_workspace_bytes(int B, int N, int Ecap, int k, int guard);
int    dvm_eigenbasis_f64(const int32_t *rowptr, const int32_t *col, const float *w, const float *mass /* or NULL */,
                          int B, int N, int Ecap, int k, int guard, int degree, int max_iter, double tol,
                          double *evals, double *evecs, double *res, int32_t *info, void *ws, size_t ws_bytes, void *stream);
size_t dvm_basis_project_workspace_bytes(int B, int N, int k, int C);
int    dvm_basis_project_f64(const double *evecs, const float *mass /* or NULL */, const float *Y, int B, int N, int k, int C,
                             double *out, void *ws, size_t ws_bytes, void *stream);

/* ZoomOut spectral refinement: maps to and from a basis (the reference's Tools/utils.py: pMap2fMap, fMap2pMap, zo_fmap /
 * func_zm_fmap, there a cKDTree query and pinv(B1) @ B2[T] on the host per step).  float64 throughout.
 * The source shape X has N vertices, the target Y has M.  The bases are Phi_X [B,N,K] and Phi_Y [B,M,K] float64 as
 * dvm_eigenbasis_f64 returns them; a truncated basis Phi[:, :k] is the same buffer with its row stride (ldx, ldy = K) given as a
 * leading dimension, so nothing is copied (element b starts at b * rows * ld).  A point map is T [B,N] int32 into Y.  C is
 * [B,k,k] float64, row-major, with Phi_X[:, :k] C ~ Phi_Y[T, :k] (the reference's C21 = pinv(B1) @ B2[T12]).
 *
 * dvm_fmap_from_pmap_f64 (pMap2fMap).  G = Phi_Y[T, :k]; a row with T[i] outside [0, M) is a zero row and is counted.
 *   mode 0 (adjoint): C = Phi_X[:, :k]^T diag(m) G, m = mass [B,N] fp32 or NULL for 1; a mass that is not positive and finite
 *     counts as 0, as in dvm_basis_project_f64.  For an M-orthonormal basis this is the weighted least-squares solution (the form of
 *     the ZoomOut paper).
 *   mode 1 (lstsq): pinv(Phi_X[:, :k]) @ G through the normal equations (Phi_X^T Phi_X) C = Phi_X^T G (mass is not used).  Both
 *     products come from the tall-skinny kernel; one workgroup per element then averages the Gram matrix' triangles, scales it to
 *     a unit diagonal, factorises it (Cholesky, the matrix in LDS) and does two triangular solves.
 *   The gather is fused into the product (no [N,k] copy of G is made).  Sums run in one fixed order: rows ascending within
 *   min(64, ceil(N / 32)) chunks, the chunks ascending; no float atomics.
 *   info [B,4] int32 = status (0 ok, 1 a Cholesky pivot that is not positive and finite: a diagonal entry of the Gram matrix
 *   that is not positive and finite, or a pivot of the unit-diagonal matrix that is not a finite number above k 2^-52, which is
 *   where two equal columns land), the k at which that happened, the entries of T outside [0, M), 0.  A failed element's C is
 *   filled with NaN.
 * dvm_fmap_embed_f64.  E [B,M,k] (row stride lde) = Phi_Y[:, :k] C^T: E_jc = sum_a Phi_Y[j,a] C[c,a], a ascending, one accumulator.
 * dvm_spectral_nn_f64 (the k-d tree query of fMap2pMap).  A [B,N,k] with row stride lda, E [B,M,k] with row stride lde ->
 *   T[i] = argmin_j d(i,j), d(i,j) = (..((t_0 t_0) + t_1 t_1) + ..) with t_c = E[j,c] - A[i,c], c ascending; every subtraction,
 *   product and sum is rounded separately (no fused multiply-add), so the distance can be reproduced bit for bit.  Every pair is
 *   evaluated in this form; there is no screen.  Ties go to the lowest j; a NaN distance counts as +inf; a row whose every
 *   distance is +inf returns 0.  dmin [B,N] (may be NULL) is the winning d.
 *   Tiling: a workgroup takes 64 source rows and one segment of the target, in tiles of 64 target rows; the target is cut into
 *   `segments` segments of `seg_len` rows (a multiple of 64) and the segment winners are merged by the total order (d, j) in a
 *   second launch.  dvm_spectral_nn_plan writes plan [4] (host memory) = source tile, target tile, segments, seg_len.  The result
 *   does not depend on the plan.
 * dvm_fmap_to_pmap_f64 (fMap2pMap): the two steps above with A = Phi_X[:, :k] and E in the workspace; dmin [B,N] and
 *   E_out [B,M,k] (contiguous) may be NULL.
 * dvm_zoomout_f64 (zo_fmap): T = T0; for k = k_init, k_init + k_step, .. < k_final: n_inter times { C = from_pmap(T, k);
 *   T = to_pmap(C, k) }; C = from_pmap(T, k_final).  Outputs C [B,k_final,k_final], T [B,N] (the map that produced C, as in the
 *   reference; may be T0's buffer) and info [B,4] = status, the failing k, the entries of T0 outside [0, M), the NN steps run.
 *   The schedule is the host's and the entry only enqueues launches: no synchronisation, capturable.  An element whose Cholesky
 *   fails sets its status, skips its remaining steps and returns C filled with NaN together with its last T; the call itself
 *   still returns DVM_OK (the caller reads info).  The outputs are, bit for bit, those of the stage entries called in that order;
 *   an element gives the same bits alone or in a batch, and from run to run.
 * Limits: 1 <= k_init <= k_final <= 128 (k <= 128 at the stage entries), k <= every leading dimension, k_step >= 1, n_inter >= 1,
 * N, M <= 2^24, B <= 65535, mode 0 or 1.  Outside them DVM_EINVAL and a size query of 0, before any launch. */
size_t dvm_fmap_from_pmap_workspace_bytes(int B, int N, int M, int k, int mode);
int    dvm_fmap_from_pmap_f64(const double *phi_x, int ldx, const float *mass /* or NULL */, const double *phi_y, int ldy,
                              const int32_t *T, int B, int N, int M, int k, int mode, double *C, int32_t *info, void *ws,
                              size_t ws_bytes, void *stream);
int    dvm_fmap_embed_f64(const double *phi_y, int ldy, const double *C, int B, int M, int k, double *E, int lde, void *stream);
int    dvm_spectral_nn_plan(int B, int N, int M, int k, int32_t *plan /* host, [4] */);
size_t dvm_spectral_nn_workspace_bytes(int B, int N, int M, int k);
int    dvm_spectral_nn_f64(const double *A, int lda, const double *E, int lde, int B, int N, int M, int k, int32_t *T,
                           double *dmin /* or NULL */, void *ws, size_t ws_bytes, void *stream);
size_t dvm_fmap_to_pmap_workspace_bytes(int B, int N, int M, int k);
int    dvm_fmap_to_pmap_f64(const double *phi_x, int ldx, const double *phi_y, int ldy, const double *C, int B, int N, int M, int k,
                            int32_t *T, double *dmin /* or NULL */, double *E_out /* or NULL */, void *ws, size_t ws_bytes,
                            void *stream);
size_t dvm_zoomout_workspace_bytes(int B, int N, int M, int k_init, int k_final, int k_step, int n_inter, int mode);
int    dvm_zoomout_f64(const double *phi_x, int ldx, const float *mass /* or NULL */, const double *phi_y, int ldy, const int32_t *T0,
                       int B, int N, int M, int k_init, int k_final, int k_step, int n_inter, int mode, double *C, int32_t *T,
                       int32_t *info, void *ws, size_t ws_bytes, void *stream);

/* farthest_point_sample — lib/deformation_graph_point.py:18-33 with the random
 * start index made an input.  xyz [B,N,3], start [B] -> out [B,npoint].
 * Limit: N <= 12288 (the cloud is held in LDS); a larger N is DVM_EINVAL before anything is launched — as at every entry
 * below that builds a deformation graph. */
int dvm_fps_f32(const float *xyz, int B, int N, int npoint, const int32_t *start, int32_t *out, void *stream);

/* DeformationGraph_geod.construct_graph_euclidean via deformation_graph_node —
 * lib/deformation_graph_point.py:177-201, models/loss.py:1325-1337.
 * xyz [B,N,3], start [B] -> nodes_idx [B,Nn] (Nn = N/2), ring [B,Nn,9] (node-local),
 * infl_idx [B,N,3] (node-local), dists [B,N,3], weights [B,N,3], sigma [B] (double).
 * Limit: N <= 12288 (dvm_fps_f32's). */
size_t dvm_dg_build_workspace_bytes(int B, int N);
int dvm_dg_build_f32(const float *xyz, int B, int N, const int32_t *start, int32_t *nodes_idx, int32_t *ring,
                     int32_t *infl_idx, float *dists, float *weights, double *sigma, void *ws, size_t ws_bytes,
                     void *stream);

/* Skinning (and node rings) by a caller-supplied distance matrix — what the reference's construct_graph_euclidean /
 * construct_graph do with their `geod` argument (lib/deformation_graph_point.py:186-198, 219-224: top-k of geod[nodes_idx].T).
 * dist [B,N,N] fp32 row-major, nodes_idx [B,Nn] with entries in [0,N) (an entry outside is read as the nearest end), any
 * 3 <= Nn <= N.
 * Orientation: vertex v and node position j meet at d(v,j) = dist[b, nodes_idx[b,j], v] — node ROWS, read along v; it matters
 * for a matrix that is not symmetric.
 * Order: candidates are sorted by the key (d, j): d compares as fp32 with NaN ranked as +inf and -0 == +0; among equal d the
 * lower j comes first.  infl_idx [B,N,3] (node-local, as dvm_dg_build_f32's) and dists [B,N,3] (the selected matrix entries,
 * copied unchanged: a NaN stays a NaN) are the first three entries of that order; ring [B,Nn,ring_k] (node-local; ring_k = 0:
 * none, ring may be NULL) holds for node i the first ring_k entries of the same order for the vertex nodes_idx[b,i] — the node
 * itself comes first only because dist[i,i] = 0, as in a KDTree's answer.
 * Limits: 0 <= ring_k <= 16, ring_k <= Nn, B <= 65535; outside them DVM_EINVAL before anything is launched.
 * One lane per vertex, 64 vertices per workgroup; the node range is split over up to 8 waves whose lists are merged in LDS by
 * the same key (a total order: the split cannot reach the result).  Asynchronous on `stream`, no workspace, no atomics,
 * capturable.  dvm_dg_skin_geod_slices_f32 is the same call with the waves per workgroup (1..8) chosen by the caller
 * (measurements, tests); dvm_dg_skin_geod_plan reports, without a device, the vertex tile, the waves per workgroup the plain
 * call takes and the length of the per-lane list (3, 9 or 16). */
int dvm_dg_skin_geod_f32(const float *dist, const int32_t *nodes_idx, int B, int N, int Nn, int ring_k /* 0 = none */,
                         int32_t *infl_idx, float *dists, int32_t *ring, void *stream);
int dvm_dg_skin_geod_slices_f32(const float *dist, const int32_t *nodes_idx, int B, int N, int Nn, int ring_k, int slices,
                                int32_t *infl_idx, float *dists, int32_t *ring, void *stream);
int dvm_dg_skin_geod_plan(int B, int N, int Nn, int ring_k, int *tile, int *slices, int *list);
/* Skinning weights of such distances: dists [B,N,3], sigma [B] (double, device) -> weights [B,N,3] =
 * exp(-d^2 / float(2 sigma^2)) row-normalised, the expressions of dvm_dg_build_f32 in its order.  Non-finite rule: an infinite
 * (or NaN) d weighs 0; a row whose sum is 0 or not finite becomes (1,0,0); no NaN is written. */
int dvm_dg_skin_weights_f32(const float *dists, const double *sigma, int B, int N, float *weights, void *stream);
/* dvm_dg_build_f32 with the skinning taken from dist [B,N,N] (the rules of dvm_dg_skin_geod_f32, Nn = N/2): nodes_idx (the
 * Euclidean FPS of xyz), sigma (20 x the mean Euclidean nearest-neighbour spacing, as the reference keeps it under any geod)
 * and, for ring_metric 0, ring are dvm_dg_build_f32's bit for bit; infl_idx, dists, weights — and for ring_metric 1 the ring
 * [B,Nn,9] — come from dist.  Limits: 6 <= N <= 12288 (dvm_fps_f32's), N >= 18 for ring_metric 1, B <= 65535. */
size_t dvm_dg_build_geod_workspace_bytes(int B, int N);
int dvm_dg_build_geod_f32(const float *xyz, const float *dist, int B, int N, const int32_t *start,
                          int ring_metric /* 0 Euclidean, 1 geodesic */, int32_t *nodes_idx, int32_t *ring, int32_t *infl_idx,
                          float *dists, float *weights, double *sigma, void *ws, size_t ws_bytes, void *stream);

/* rotation_6d_to_matrix — models/loss.py:39-45.  d6 [rows,6] -> R [rows,9] (rows b1,b2,b1xb2). */
int dvm_rot6d_f32(const float *d6, int rows, float *R, void *stream);
/* Backward of dvm_rot6d_f32: g_R [rows,9] -> g_d6 [rows,6] (Gram-Schmidt differentiated). */
int dvm_rot6d_bwd_f32(const float *d6, const float *g_R, int rows, float *g_d6, void *stream);

/* DeformationGraph_geod.forward — lib/deformation_graph_point.py:233-261.
 * R [B,Nn,9], T [B,Nn,3] -> warped [B,N,3], arap [B], sr [B] (optional). */
int dvm_dg_warp_arap_fwd_f32(const float *xyz, int B, int N, const int32_t *nodes_idx, const int32_t *ring,
                             const int32_t *infl_idx, const float *weights, const float *R, const float *T,
                             float *warped, float *arap, float *sr, void *stream);
/* The same forward for a graph with an explicit node count and ring width — the mesh-mode graph of
 * DeformationGraph_geod.construct_graph (lib/deformation_graph_point.py:203-231): Nn decimated vertices, rings of
 * max_neigh_num = 18 adjacent nodes padded with the node itself.  nodes_idx [B,Nn], ring [B,Nn,ring_width]. */
int dvm_dg_warp_arap_graph_f32(const float *xyz, int B, int N, int Nn, int ring_width, const int32_t *nodes_idx,
                               const int32_t *ring, const int32_t *infl_idx, const float *weights, const float *R,
                               const float *T, float *warped, float *arap, float *sr, void *stream);
/* Backward of dvm_dg_warp_arap_fwd_f32 w.r.t. the node transforms: g_warped [B,N,3], g_arap [B] ->
 * d_R [B,Nn,9], d_T [B,Nn,3] (overwritten; fp32 atomics).  The vertices carry no gradient (inputs). */
int dvm_dg_warp_arap_bwd_f32(const float *xyz, int B, int N, const int32_t *nodes_idx, const int32_t *ring,
                             const int32_t *infl_idx, const float *weights, const float *R, const float *T,
                             const float *g_warped, const float *g_arap, float *d_R, float *d_T, void *stream);

/* chamfer_3DDist — third-party ChamferDistancePytorch (un-vendored); call sites
 * models/loss.py:1120,1223,874.  a [B,N,3], b [B,M,3] -> d1 [B,N], d2 [B,M] squared NN
 * distances, i1 [B,N], i2 [B,M] (optional). */
size_t dvm_chamfer_workspace_bytes(int B, int N, int M);
int dvm_chamfer_fwd_f32(const float *a, const float *b, int B, int N, int M, float *d1, float *d2, int32_t *i1,
                        int32_t *i2, void *ws, size_t ws_bytes, void *stream);
/* Backward of dvm_chamfer_fwd_f32 through the arg-min indices held fixed (as the upstream CUDA extension
 * does): g_d1 [B,N], g_d2 [B,M] -> d_a [B,N,3], d_b [B,M,3] (overwritten; fp32 atomics). */
int dvm_chamfer_bwd_f32(const float *a, const float *b, const int32_t *idx1, const int32_t *idx2, const float *g_d1,
                        const float *g_d2, int B, int N, int M, float *d_a, float *d_b, void *stream);

/* Deformer.forward — models/model.py:464-478 (+ MLP 433-452), fed the raw features and
 * kNN indices instead of the (B,N,k,128) gathers of models/loss.py:1254-1255.
 * feat1 [B,N,128], feat2 [B,M,128], verts1 [B,N,3], verts12 [B,N,3], idx11 [B,N,k],
 * idx22 [B,M,k], pi_val/pi_idx [B,N,topk], fps1 [B,Nn]; weights: conv_w [k], conv_b [1],
 * W0 [512,262] b0, W1 [256,512] b1, W2 [128,256] b2, W3 [9,128] b3 -> out [B,Nn,9].
 * variant: 0 = fp16x2-split matrix-core MLP, 64 nodes per workgroup (fp32-accurate; a value outside fp16's range
 * raises a device flag and the bf16x3 kernel, gated on it, overwrites the result), 3 = bf16x3-split matrix-core MLP
 * (fp32-accurate, any range), 2 = fp32-MFMA MLP (k-ordered fma chain, bit-identical to the oracle's),
 * 1 = scalar-FMA MLP (cross-check). */
size_t dvm_deformer_workspace_bytes(int B, int N, int M, int Nn);
int dvm_deformer_fwd_f32(const float *feat1, const float *feat2, const float *verts1, const float *verts12,
                         const int32_t *idx11, const int32_t *idx22, const float *pi_val, const int32_t *pi_idx,
                         const int32_t *fps1, int B, int N, int M, int Nn, int k, int topk, const float *conv_w,
                         const float *conv_b, const float *W0, const float *b0, const float *W1, const float *b1,
                         const float *W2, const float *b2, const float *W3, const float *b3, float *out, int variant,
                         void *ws, size_t ws_bytes, void *stream);

/* The Deformer's decoder MLP alone — models/model.py:433-452, 476-477.
 * z [rows,262] -> out [rows,9] (262 -> 512 -> 256 -> 128 -> 9, ELU). */
size_t dvm_deformer_mlp_workspace_bytes(int rows);
int dvm_deformer_mlp_fwd_f32(const float *z, int rows, const float *W0, const float *b0, const float *W1,
                             const float *b1, const float *W2, const float *b2, const float *W3, const float *b3,
                             float *out, void *ws, size_t ws_bytes, void *stream);

/* Uni3FC.pos_encoding_sin_wave — models/model.py:544-561.  x [B,3,N] -> out [B,384,N]:
 * nc = 2*((x-min)/(max-min))-1 with the min/max of the WHOLE tensor, 64 octaves pi*2^j. */
size_t dvm_pos_encoding_workspace_bytes(void);
int dvm_pos_encoding_f32(const float *x, int B, int N, float *out, void *ws, size_t ws_bytes, void *stream);
/* Same encoding with the normalisation range supplied: minmax[0] = min, minmax[1] = max (device pointer).  For a
 * pair batch sharded over ranks the reference's whole-tensor min/max (models/model.py:548) is the min/max over
 * ALL ranks' shards; the host reduces the two numbers (MIN / MAX all-reduce) and passes them here. */
int dvm_pos_encoding_minmax_f32(const float *x, const float *minmax, int B, int N, float *out, void *stream);
/* ... with the range over all ranks: this rank's (min, max) -> minmax2 (two floats of caller-owned device memory), the caller's
 * collective (MIN on the first, MAX on the second), then the encoding */
int dvm_pos_encoding_sync_f32(const float *x, int B, int N, float *out, void *ws, size_t ws_bytes, const dvm_collective *coll,
                              float *minmax2, void *stream);

/* Training-mode nn.BatchNorm1d over [B,C,N] fused with the residual add in front of it and the (Leaky)ReLU behind it
 * (models/model.py:97-123 SA_Layer, 325-395 N2PAttention, 506-529 conv blocks):
 *   z = x (+ res);  y = act(gamma (z - mean_c) / sqrt(var_c + eps) + beta),  act(t) = t > 0 ? t : slope t
 * (slope 1: none, 0: ReLU, 0.2: LeakyReLU).  save_mean / save_invstd [C] feed the backward; running_mean / running_var
 * (may be NULL) get PyTorch's momentum update with the unbiased variance.  Backward: dx (= d res) [B,C,N],
 * dgamma / dbeta [C] (may be NULL); the activation's derivative is taken from the sign of y. */
size_t dvm_bn_workspace_bytes(int B, int C, int N);
/* The same fused BatchNorm (forward and backward below) on POINT-MAJOR activations x [R, C] (R = B*N rows, C % 4 == 0), the
 * layout of the training path: statistics per column, in a fixed summation order (row chunk by row chunk).  The backward
 * with accumulate = 1 ADDS the parameter gradients to dgamma / dbeta (autograd's `p.grad += g` without the extra launches). */
size_t dvm_bn_pm_workspace_bytes(long R, int C);
int dvm_bn_act_train_fwd_pm_f32(const float *x, const float *res, const float *gamma, const float *beta, long R, int C, float eps,
                                float slope, float momentum, float *y, float *save_mean, float *save_invstd, float *running_mean,
                                float *running_var, void *ws, size_t ws_bytes, void *stream);
/* The same forward that also returns the UNBIASED batch variance (save_var_unbiased [C], may be NULL): with running_mean ==
 * running_var == NULL the running statistics are left alone and can be updated later from (save_mean, save_var_unbiased) with
 * exactly the fused kernel's expression — dvm_uni3fc_train_running_stats_f32 does so for a whole network call. */
int dvm_bn_act_train_fwd_pm_var_f32(const float *x, const float *res, const float *gamma, const float *beta, long R, int C, int groups,
                                    float eps, float slope, float momentum, float *y, float *save_mean, float *save_invstd,
                                    float *save_var_unbiased, float *running_mean, float *running_var, void *ws, size_t ws_bytes,
                                    void *stream);
/* groups > 1 (here and in dvm_bn_act_train_bwd_pm_groups_f32): x holds `groups` consecutive blocks of R rows, each normalised
 * with ITS OWN batch statistics (several network calls merged into one batch: the reference normalises per call); save_* are
 * [groups][C]; the running statistics take the groups' updates one after the other; dgamma / dbeta sum over the groups.
 * Workspace: dvm_bn_pm_groups_workspace_bytes(R, C, groups). */
size_t dvm_bn_pm_groups_workspace_bytes(long R, int C, int groups);
/* Cross-rank statistics for a data-parallel step (train.py under DDP: the reference's single-process batch normalises over ALL
 * pairs, models/model.py:496-503).  With a collective, the per-(group, channel) totals (sum x, sum x^2 — backward: sum dz,
 * sum dz xhat) and the groups' row counts are written to `sync_buf` (dvm_bn_pm_sync_bytes(C, groups) bytes of caller-owned device
 * memory), handed to the caller's all-reduce (float64, SUM, in place, enqueued on `stream`), and the normalisation uses the global
 * totals; dgamma / dbeta stay this rank's sums (the gradient all-reduce adds the ranks').  coll == NULL: the plain calls above. */
size_t dvm_bn_pm_sync_bytes(int C, int groups);
int dvm_bn_act_train_fwd_pm_sync_f32(const float *x, const float *res, const float *gamma, const float *beta, long R, int C, int groups,
                                     float eps, float slope, float momentum, float *y, float *save_mean, float *save_invstd,
                                     float *save_var_unbiased, float *running_mean, float *running_var, void *ws, size_t ws_bytes,
                                     const dvm_collective *coll, void *sync_buf, void *stream);
int dvm_bn_act_train_bwd_pm_sync_f32(const float *dy, const float *y, const float *x, const float *res, const float *gamma,
                                     const float *save_mean, const float *save_invstd, long R, int C, int groups, float slope,
                                     float *dx, float *dgamma, float *dbeta, int accumulate, void *ws, size_t ws_bytes,
                                     const dvm_collective *coll, void *sync_buf, void *stream);
int dvm_bn_act_train_bwd_pm_groups_f32(const float *dy, const float *y, const float *x, const float *res, const float *gamma,
                                       const float *save_mean, const float *save_invstd, long R, int C, int groups, float slope,
                                       float *dx, float *dgamma, float *dbeta, int accumulate, void *ws, size_t ws_bytes, void *stream);
int dvm_bn_act_train_bwd_pm_f32(const float *dy, const float *y, const float *x, const float *res, const float *gamma,
                                const float *save_mean, const float *save_invstd, long R, int C, float slope, float *dx,
                                float *dgamma, float *dbeta, int accumulate, void *ws, size_t ws_bytes, void *stream);
int dvm_bn_act_train_fwd_f32(const float *x, const float *res, const float *gamma, const float *beta, int B, int C, int N,
                             float eps, float slope, float momentum, float *y, float *save_mean, float *save_invstd,
                             float *running_mean, float *running_var, void *ws, size_t ws_bytes, void *stream);
int dvm_bn_act_train_bwd_f32(const float *dy, const float *y, const float *x, const float *res, const float *gamma,
                             const float *save_mean, const float *save_invstd, int B, int C, int N, float slope, float *dx,
                             float *dgamma, float *dbeta, void *ws, size_t ws_bytes, void *stream);

/* cal_geo — models/dataset.py:49-54 (potpourri3d heat method in the reference; graph shortest paths here, as in the
 * reference's eval/geo_mat.py:15-41).  All-pairs shortest paths of an undirected graph given as padded neighbour lists:
 * nbr [N,K] (-1 ends a list), w [N,K] fp64 edge lengths -> D [N,N] fp64 (+inf between components).  N <= 19200. */
int dvm_graph_geodesics_f64(const int32_t *nbr, const double *w, int N, int K, double *D, void *stream);

/* cal_geo(method="mesh") — geodesic distances on a triangle mesh by the first-order upwind ("fast-marching") update on triangles,
 * relaxed to its fixed point (the scheme is stated in tests/mesh_geodesic_ref.py): unlike the edge paths above, which cannot cut
 * across a triangle and overestimate by 5 - 8 % at any resolution, a discretisation of the surface metric (error 1 - 2 % on the test
 * meshes, falling with refinement; never above the edge-path distance).  Not the reference's heat method either: its values stay
 * unpinned.  verts [V,3] fp64, faces [F,3] int32 (degenerate, repeated and duplicate faces are allowed; vertices in no face stay at
 * +inf), sources [S] int32 vertex ids (repeats allowed) or NULL = all V vertices in order, D [S or V, V] fp64: D[r, v] = distance
 * from source r to vertex v, +inf between components.  The result is asymmetric at the 0.5 % level (as the heat method's).
 * Updates are made in place, in the order the hardware runs the threads: two calls agree to the acceptance margin's effect
 * (relative differences of some 1e-12), not bit for bit.
 * One workgroup per source with its V distances in LDS: V <= dvm_mesh_geodesics_max_v() (16384).  A prologue writes the corner
 * table (48 bytes per corner, CSR by vertex) into the workspace: dvm_mesh_geodesics_workspace_bytes(V, F), 0 for sizes the entry
 * refuses.
 * Errors.  Before any launch: null pointers, V < 1, F < 0, V over the limit, S < 1 with a list (DVM_EINVAL), a short workspace
 * (DVM_ENOSPACE).  On the device: a face or source index outside [0, V) (checked before it is used: such a face is left out, such
 * a source's row is not written; DVM_EINVAL) and a source that has not settled after 4 V sweeps (DVM_ELAUNCH) set a flag word in
 * the workspace.  THIS ENTRY SYNCHRONISES: after its last launch it copies that one word back and waits for `stream`, so that
 * the error is this call's return value — the exception to the conventions above (it is once-per-shape preprocessing; do not
 * call it under stream capture).
 * Diagnostics: after the call the workspace holds, at byte 256, int32 sweeps[min(S or V, V)], the sweeps each of the first sources
 * took. */
int dvm_mesh_geodesics_max_v(void);
size_t dvm_mesh_geodesics_workspace_bytes(int V, int F);
int dvm_mesh_geodesics_f64(const double *verts, const int32_t *faces, int V, int F, const int32_t *sources, int S, double *D, void *ws,
                           size_t ws_bytes, void *stream);

/* Uni3FC.proj2img — models/model.py:584-650 (+ get_colored_depth_maps 563-581).  pts [B,N,3] (one of the three
 * axis-permuted views) -> img [B,3,224,224]: every point adds its depth (3rd coordinate) to the 5x5 pixels around its
 * cell, sigmoid, ImageNet-normalise, min-max rescale per image, 'PiYG' colour table, pixels whose depth sum is exactly 0
 * -> -1.  Also returns what I2P needs: pc_min [B,2], grid_size [B], offsets [B,2] (float-valued integers).  The depth
 * sums are accumulated in 64-bit fixed point, so the image is bit-reproducible from run to run.
 * Resolution: a depth enters the sum as round(z * 2^e), e = min(40, 60 - floor(log2(25 N max|z|))) (40 while
 * 25 N max|z| < 2^21), so a term below 2^-(e+1) is dropped: a point alone in a pixel with |z| < 2^-(e+1) renders as background
 * where the reference colours it.  An image whose depths are all 0 is -1 everywhere. */
size_t dvm_proj2img_workspace_bytes(int B);
int dvm_proj2img_f32(const float *pts, int B, int N, float *img, float *pc_min, float *grid_size, float *offsets, void *ws,
                     size_t ws_bytes, void *stream);

/* The per-pixel filtering step of the FeatUp joint-bilateral upsampler that stands between proj2img and I2P (the
 * `upsampler` of models/model.py:693, train.py:72; FeatUp's `AdaptiveConv` CUDA op):
 *   out[b,c,h,w] = sum_{i,j<d} in[b,c,h+i,w+j] * kern[b,h,w,i,j]
 * in [B,C,H+d-1,W+d-1] (the padded, bicubically upsampled features), kern [B,H,W,d,d] — or [B,d*d,H,W] when
 * kern_tap_major != 0 —, out [B,C,H,W]; d odd, <= 15. */
int dvm_adaptive_conv_f32(const float *in, const float *kern, int B, int C, int H, int W, int d, int kern_tap_major, float *out,
                          void *stream);

/* F.interpolate(x, size=(Ho,Wo), mode='bicubic', align_corners=False) followed by F.pad(.., [pad]*4, mode='reflect') in
 * one pass (the high-resolution source of a joint-bilateral stage): in [BC,Hi,Wi] -> out [BC,Ho+2*pad,Wo+2*pad]. */
int dvm_bicubic_resize_pad_f32(const float *in, int BC, int Hi, int Wi, int Ho, int Wo, int pad, float *out, void *stream);

/* The combined range x spatial kernel of one joint-bilateral stage, before its learned correction (FeatUp
 * JBULearnedRange: get_range_kernel, get_spatial_kernel and their normalised product): for pixel p and tap t of the
 * d x d window (reflect padding)  k[p,t] ~ softmax_t(exp(range_temp) * <proj[p], proj[p+t]>) * exp(-|t|^2 / (2 sigma^2)),
 * normalised over t.  proj [B,key_dim,H,W] (the guidance image through range_proj); range_temp, sigma_spatial: device
 * scalars (the module's parameters); out [B,d*d,H,W].  key_dim = 32, d = 7 (FeatUp's JBU stack). */
int dvm_jbu_kernel_f32(const float *proj, const float *range_temp, const float *sigma_spatial, int B, int key_dim, int H, int W, int d,
                       float *out, void *stream);

/* Uni3FC.I2P (+ F.normalize) — models/model.py:653-678, 701-708.  f [B,C,H,W] image features; for every point the
 * bicubic (A=-0.75, align_corners=False) resample of f to 224x224 is evaluated ONLY at the point's pixel — the
 * (B,C,224,224) resized tensor is never built — and written to out[b,i,0:C] (row stride ldo >= C floats, so the three
 * views can land side by side in one (B,N,3C) tensor); normalize != 0 divides by max(|row|_2, 1e-12). */
int dvm_i2p_f32(const float *pts, const float *f, const float *pc_min, const float *grid_size, const float *offsets, int B,
                int N, int C, int H, int W, int normalize, float *out, int ldo, void *stream);

/* SA_Layer attention core — models/model.py:113-121.  p [B,N,16] = Wqk x (q and k share the
 * weight), v [B,N,64] = Wv x + bv, point-major.  energy = p p^T, row softmax, every column
 * divided by (1e-9 + its sum over rows), x_r = attention^T-weighted sum of v -> xr [B,N,64]. */
size_t dvm_sa_attention_workspace_bytes(int B, int N);
int dvm_sa_attention_fwd_f32(const float *p, const float *v, int B, int N, float *xr, void *ws, size_t ws_bytes,
                             void *stream);

/* Training twins of the SA attention core.  train_fwd: as dvm_sa_attention_fwd_f32, also returning what the
 * backward recomputes from: stats [B,N,2] = (row max m_i, 1/l_i) and cinv [B,N] = 1/(1e-9 + column sum).
 * bwd: g_xr [B,N,64] -> d_p [B,N,16], d_v [B,N,64] (overwritten).  Nothing N x N is stored: two
 * tile-recompute passes on the fp32 matrix cores (E is symmetric, so both dE_ij and dE_ji come from one tile). */
size_t dvm_sa_attention_train_fwd_workspace_bytes(int B, int N);
int dvm_sa_attention_train_fwd_f32(const float *p, const float *v, int B, int N, float *xr, float *stats, float *cinv,
                                   void *ws, size_t ws_bytes, void *stream);
size_t dvm_sa_attention_bwd_workspace_bytes(int B, int N);
int dvm_sa_attention_bwd_f32(const float *p, const float *v, const float *xr, const float *stats, const float *cinv,
                             const float *g_xr, int B, int N, float *d_p, float *d_v, void *ws, size_t ws_bytes,
                             void *stream);

/* N2PAttention[_DIM] attention core — models/model.py:339-350, 375-386.  q/kp/vp [B,N,C] =
 * Wq x, Wk x, Wv x (point-major; k(x_j - x_i) = kp_j - kp_i by linearity), idx [B,N,K] the
 * feature-space neighbours -> out [B,N,C] = sum_j softmax_j(q.(kp_j-kp_i)/sqrt(D)) (vp_j - vp_i)
 * per head.  C in {64,128}, heads = 4, K <= 64. */
int dvm_n2p_attention_fwd_f32(const float *q, const float *kp, const float *vp, const int32_t *idx, int B, int N,
                              int C, int K, int heads, float *out, void *stream);

/* Training twins of the N2P attention core.  qkv [B,N,3C] = [Wq x | Wk x | Wv x] per point (one GEMM's
 * output, used in place), idx [B,N,K].  fwd: out [B,N,C] as dvm_n2p_attention_fwd_f32, plus the attention
 * weights attn [B,N,K,heads] kept for the backward.  bwd: g_out [B,N,C] -> d_qkv [B,N,3C] (overwritten; the
 * scatter onto neighbour rows runs as a gather over the reversed neighbour lists — a counting sort of idx
 * in the workspace — so no float atomics; idx entries must lie in [0,N)).  C in {64,128}, heads = 4, K <= 64. */
int dvm_n2p_core_fwd_f32(const float *qkv, const int32_t *idx, int B, int N, int C, int K, int heads, float *out,
                         float *attn, void *stream);
size_t dvm_n2p_core_bwd_workspace_bytes(int B, int N, int K);
int dvm_n2p_core_bwd_f32(const float *qkv, const int32_t *idx, const float *attn, const float *g_out, int B, int N,
                         int C, int K, int heads, float *d_qkv, void *ws, size_t ws_bytes, void *stream);

/* dist-loss term — models/loss.py:1351-1396 for one shape batch: anchors [nA] (shared by the
 * batch), idx = knn(feat[:,anchors], feat, k); x = |feat[idx] - feat[anchor]|, y = dist[b, idx, anchor];
 * out[b] = sum_n (1 - |cos(x_n, y_n)|).  feat [B,N,C], dist [B,N,N]; idx_out [B,nA,k] optional. */
size_t dvm_dist_loss_workspace_bytes(int B, int N, int C, int nA, int k);
int dvm_dist_loss_fwd_f32(const float *feat, const float *dist, const int32_t *anchors, int B, int N, int C, int nA,
                          int k, float *out, int32_t *idx_out, void *ws, size_t ws_bytes, void *stream);

/* Backward of dvm_dist_loss_fwd_f32, first half: with idx [B,nA,k] from the forward (idx_out) and
 * g_out [B] = dL/d out, writes the dense weights W [B,nA,N] (overwritten; zero outside idx):
 *   W[b,n,v] = g_out[b] * d term_n/d x_v / x_v   (x_v = |feat[v] - feat[a_n]|, 0 where x_v = 0).
 * The feature gradient follows with library GEMMs:
 *   d feat = diag(colsum W) feat - W^T feat[anchors];  d feat[a_n] += rowsum(W)_n feat[a_n] - (W feat)_n. */
int dvm_dist_loss_bwd_weights_f32(const float *feat, const float *dist, const int32_t *anchors, const int32_t *idx,
                                  const float *g_out, int B, int N, int C, int nA, int k, float *W, void *stream);

/* map-loss numerator — models/loss.py:1232-1238 + FrobeniusLoss 476-482:
 * out[b] = sum_{i,s,c} (verts12[idx11[i,s],c] - sum_t P[i,t] verts2[idx22[pidx[i,t],s],c])^2. */
size_t dvm_map_term_workspace_bytes(int B, int N);
int dvm_map_term_f32(const float *verts12, const float *verts2, const int32_t *idx11, const int32_t *idx22,
                     const float *pi_val, const int32_t *pi_idx, int B, int N, int M, int k, int topk, float *out,
                     void *ws, size_t ws_bytes, void *stream);

/* One direction of GraphDeformLoss_Neural.deform() for B pairs, forward only, with no
 * host round trip — models/loss.py:1228-1296, 1401-1410; deform.py:232-257:
 *   graph(verts1) -> Pi_12 -> verts12 -> kNN(verts1), kNN(verts2) -> Deformer -> rot6d ->
 *   ED warp + ARAP -> chamfer(warped,verts2), chamfer(verts12,verts2) (+ map term).
 * Inputs: feat1 [B,N,128], feat2 [B,M,128], verts1 [B,N,3], verts2 [B,M,3], fps_start [B],
 * Deformer weights as in dvm_deformer_fwd_f32 (k = topk = 10).
 * Outputs: warped [B,N,3], verts12 [B,N,3], T12 [B,N] (argmax of Pi),
 *          losses [B,6] = {mean d(warped->verts2), mean d(verts2->warped), arap,
 *                          mean d(verts12->verts2), mean d(verts2->verts12), map_sum}
 *          (squared NN distances; chamfer_loss = [0]+[1], the partial variant keeps one side).
 * Limit: N <= 12288, the cloud whose graph is built (dvm_fps_f32's limit; DVM_EINVAL before anything is launched). */
size_t dvm_pair_direction_workspace_bytes(int B, int N, int M);
int dvm_pair_direction_fwd_f32(const float *feat1, const float *feat2, const float *verts1, const float *verts2,
                               int B, int N, int M, float neg_alpha, const int32_t *fps_start, const float *conv_w,
                               const float *conv_b, const float *W0, const float *b0, const float *W1,
                               const float *b1, const float *W2, const float *b2, const float *W3, const float *b3,
                               int with_map, float *warped, float *verts12, int32_t *T12, float *losses, void *ws,
                               size_t ws_bytes, void *stream);

/* Both directions of the deformation part of GraphDeformLoss_Neural.forward for B pairs —
 * models/loss.py:1401-1411 (graphs of both clouds, Pi_12 and Pi_21, deform() twice) with the work
 * shared between the directions (xyz kNN, pooled features, one soft-correspondence launch, one MLP
 * launch, one grouped Chamfer launch).  Outputs as in dvm_pair_direction_fwd_f32, once per direction
 * (`12`: cloud 1 deformed towards cloud 2; `21`: the reverse).
 * Limit: N, M <= 12288 (a graph is built on both clouds: dvm_fps_f32's limit; DVM_EINVAL before anything is launched) — here,
 * at dvm_pair_fwd_cached_f32 and at dvm_pair_geometry_f32. */
size_t dvm_pair_workspace_bytes(int B, int N, int M);
int dvm_pair_fwd_f32(const float *feat1, const float *feat2, const float *verts1, const float *verts2, int B, int N,
                     int M, float neg_alpha, const int32_t *start1, const int32_t *start2, const float *conv_w,
                     const float *conv_b, const float *W0, const float *b0, const float *W1, const float *b1,
                     const float *W2, const float *b2, const float *W3, const float *b3, int with_map, float *warped12,
                     float *verts12, int32_t *T12, float *losses12, float *warped21, float *verts21, int32_t *T21,
                     float *losses21, void *ws, size_t ws_bytes, void *stream);

/* dvm_pair_fwd_f32 with the per-shape graph cache of SURVEY 8f-2: the coordinate-only products of a call — both clouds'
 * deformation graphs (FPS nodes, node rings, skinning weights: lib/deformation_graph_point.py:177-201 via
 * models/loss.py:1325-1337), their uniform grids, the xyz kNN (models/loss.py:97-101) and the neighbour coordinates of the map
 * term — stay in the caller's workspace.  reuse_geometry = 0 builds them (identical to dvm_pair_fwd_f32); reuse_geometry != 0
 * uses what an earlier call left in THIS workspace: valid iff that call had the same B, N, M, coordinates and FPS starts and
 * nothing else wrote the workspace since (the caller keeps one workspace per cache key).  Outputs are bit-identical to the
 * uncached call.  The reference rebuilds the graphs on every call; the cache is the caller's opt-in. */
int dvm_pair_fwd_cached_f32(const float *feat1, const float *feat2, const float *verts1, const float *verts2, int B, int N,
                            int M, float neg_alpha, const int32_t *start1, const int32_t *start2, const float *conv_w,
                            const float *conv_b, const float *W0, const float *b0, const float *W1, const float *b1,
                            const float *W2, const float *b2, const float *W3, const float *b3, int with_map, float *warped12,
                            float *verts12, int32_t *T12, float *losses12, float *warped21, float *verts21, int32_t *T21,
                            float *losses21, void *ws, size_t ws_bytes, int reuse_geometry, void *stream);

/* The coordinate-only half of dvm_pair_fwd_f32 as its own call, for a pipelined caller: both clouds' deformation graphs (FPS nodes,
 * node rings, skinning weights: lib/deformation_graph_point.py:18-33, 177-201 via models/loss.py:1325-1337), their uniform grids,
 * the xyz kNN (models/loss.py:97-101) and, when the map term needs them, the neighbour coordinates are written into `ws`
 * (dvm_pair_workspace_bytes(B, N, M)); a later dvm_pair_fwd_cached_f32(..., reuse_geometry = 1) on the SAME workspace, B, N, M,
 * coordinates, starts and with_map consumes them.  Typical use: the geometry of batch t + 1 on a second stream while batch t's
 * feature-dependent half runs (dv-matcher_amd/dvm/ops.py::PairPipeline; the caller orders the two calls with its own events and
 * keeps one workspace per batch in flight).  Nothing is cached: each batch's graphs are built once, only earlier; outputs are
 * bit-identical to dvm_pair_fwd_f32.  With a dvm_pair_init context for `stream`, vertex grid + xyz kNN run on the context's second
 * helper stream beside the FPS chain and are joined into `stream` before the call returns. */
int dvm_pair_geometry_f32(const float *verts1, const float *verts2, int B, int N, int M, const int32_t *start1,
                          const int32_t *start2, int with_map, void *ws, size_t ws_bytes, void *stream);

/* ---- LG-Net, the whole eval-mode forward in one call (reference models/model.py:680-761 `Uni3FC.forward` with
 * torch.no_grad() / model.eval(); layers 506-529, N2P blocks 325-395, SA_Layer 97-123).  xyz [B][3][N] coordinates, dino
 * [B][N][1152] per-point visual features -> feat [B][N][128], tmp [B][N][64] (the second return value of the reference's
 * forward).  Every layer is one of this library's own launches, enqueued natively in the order of the reference's forward:
 * the same kernels and operands as dv-matcher_amd/models/model.py::Uni3FC._forward_infer, ~250 launches without a Python call
 * in between.  k = neighbours of the N2P blocks (the reference's 40).  With a context from dvm_pair_init(stream) the global
 * (self-attention) chain runs on the context's helper stream next to the local (kNN attention) chain.
 * `weights`: DVM_U3_NWEIGHTS device pointers, fp32, in this order (W = conv weight [Co][K]; alpha, beta = the eval-mode
 * BatchNorm folded as ATen's CPU kernel evaluates it, y = fma(x, alpha, beta), alpha = w / sqrt(var + eps), beta =
 * fma(-mean, alpha, b) — dv-matcher_amd/models/model.py::_bn_affine):
 *   8 conv blocks {W, alpha, beta}: conv (1152->384), conv0 (384->64), conv1 (256->512), conv2 (256->512),
 *     conv3 (768->128), conv4 (768->128), conv5 (256->128), conv6 (512->128)                                  [0 .. 23]
 *   4 SA layers sa1..sa4 {k_conv W [16][64], v_conv W [64][64], v_conv bias, trans_conv W [64][64], trans_conv bias,
 *     after_norm alpha, after_norm beta}                                                                      [24 .. 51]
 *   7 N2P blocks n2p_attention1..7 (C = 64 x 4, 128 x 3) {stacked q|k|v W [3C][C], bn1 alpha, bn1 beta, ff[0] W [4C][C],
 *     ff[2] W [C][4C], bn2 alpha, bn2 beta}                                                                   [52 .. 100] */
#define DVM_U3_NWEIGHTS 101
size_t dvm_uni3fc_fwd_workspace_bytes(int B, int N, int k);
int dvm_uni3fc_fwd_f32(const float *xyz, const float *dino, int B, int N, const float *const *weights, int nweights, int k,
                       float *feat, float *tmp, void *ws, size_t ws_bytes, void *stream);

/* ---- LG-Net, the TRAINING forward and backward in two calls (reference `Uni3FC.forward` in train mode under autograd,
 * models/model.py:680-761 — conv blocks 506-529 with batch-statistics BatchNorm, N2PAttention[_DIM] 325-395, SA_Layer
 * 97-123 — and the part of `loss.backward()`, train.py:110, that runs through it).  Same launches as
 * dv-matcher_amd/models/model.py::Uni3FC._forward_train_pm and the autograd graph it records, enqueued natively.
 * fwd: xyz [B][3][N], dino [B][N][1152] -> feat [B][N][128], tmp [B][N][64]; every activation the backward needs is
 *      written into `arena` (dvm_uni3fc_train_workspace_bytes(B, N, k) bytes, caller-owned, must stay untouched until
 *      the matching bwd); running_mean / running_var get PyTorch's momentum update (unbiased variance) — or, with
 *      defer_running_stats != 0, are left alone: the batch statistics stay in the arena and
 *      dvm_uni3fc_train_running_stats_f32(params, arena) applies the 26 updates later in one launch (two network calls
 *      that run side by side on two streams share every BatchNorm; their updates are applied afterwards in the
 *      reference's call order, train.py:100-101); the num_batches_tracked counters are the caller's business.  knn_forced / knn_log (each NULL or 7 device pointers
 *      [B][N][k] int32, entries may be NULL) are the parity tests' handles on the 7 feature-space kNN layers: the
 *      library's own neighbour sets are copied to knn_log[l], and knn_forced[l], when given, is what the layer and
 *      its backward then use (teacher forcing: the discrete sets of the reference, tests/test_gpu_network.py).
 * bwd: g_feat [B][N][128], g_tmp [B][N][64] (may be NULL = zero), the forward's dino / feat / tmp and arena ->
 *      parameter gradients ADDED into grads[i] (same indexing as params; entries of running statistics ignored, may
 *      be NULL).  Inputs carry no gradient (the reference feeds data tensors).  Weight gradients are combined with
 *      fp32 atomics over row chunks (dvm_linear_wgrad_f32); bias / BatchNorm gradients in a fixed order.
 * groups (1 or 2): SEVERAL network calls of the reference in one — the B shapes are `groups` consecutive blocks of B / groups
 *      shapes, each with its own BatchNorm batch statistics and position-encoding range (and the running statistics updated
 *      block after block), i.e. exactly the results of `groups` separate calls (the criterion calls the network once per shape
 *      of a pair, train.py:100-101: same point count -> ONE call with groups = 2, every row-wise kernel over twice the rows).
 * With a context from dvm_pair_init(stream) the global (self-attention) chain runs on the helper stream in both passes.
 * `params`: DVM_U3_TRAIN_NPARAMS device pointers, fp32, in this order:
 *   8 conv blocks {W [Co][K], bn gamma, bn beta, running_mean, running_var}: conv, conv0 .. conv6            [0 .. 39]
 *   4 SA layers sa1..sa4 {k_conv W [16][64] (tied with q_conv), v_conv W [64][64], v_conv bias, trans_conv W [64][64],
 *     trans_conv bias, after_norm gamma, beta, running_mean, running_var}                                     [40 .. 75]
 *   7 N2P blocks n2p_attention1..7 (C = 64 x 4, 128 x 3) {q_conv W [C][C], k_conv W, v_conv W, bn1 gamma, beta,
 *     running_mean, running_var, ff[0] W [4C][C], ff[2] W [C][4C], bn2 gamma, beta, running_mean, running_var} [76 .. 166]
 * (q / k / v weights — and their gradient buffers — that lie back to back in memory are used as one stacked [3C][C]
 * matrix in place; otherwise a packed copy is made per call.) */
#define DVM_U3_TRAIN_NPARAMS 167
size_t dvm_uni3fc_train_workspace_bytes(int B, int N, int k);
int dvm_uni3fc_train_fwd_f32(const float *xyz, const float *dino, int B, int N, const float *const *params, int nparams, int k,
                             float eps, float momentum, int groups, int defer_running_stats, const int32_t *const *knn_forced,
                             int32_t *const *knn_log, float *feat, float *tmp, void *arena, size_t arena_bytes, void *stream);
int dvm_uni3fc_train_running_stats_f32(const float *const *params, int nparams, int B, int N, int k, int groups, float momentum,
                                       void *arena, size_t arena_bytes, void *stream);
int dvm_uni3fc_train_bwd_f32(const float *g_feat, const float *g_tmp, const float *dino, const float *feat, const float *tmp,
                             int B, int N, const float *const *params, float *const *grads, int nparams, int k, int groups,
                             void *arena, size_t arena_bytes, void *stream);
/* The same two calls inside a DATA-PARALLEL step (train.py:30-33 picks one device; the 8-GPU run shards the pair batch): with
 * `coll` every batch statistic the reference takes over its whole batch is combined over the ranks by the caller's collective —
 * the 26 BatchNorms' totals in both passes (dvm_bn_act_train_*_pm_sync_f32) and the position encoding's min / max
 * (dvm_pos_encoding_sync_f32, models/model.py:548) — so the sharded step reproduces the single-process one on THIS native node.
 * The buffers handed to the collective lie inside `arena`.  coll == NULL: identical to the calls above. */
int dvm_uni3fc_train_fwd_sync_f32(const float *xyz, const float *dino, int B, int N, const float *const *params, int nparams, int k,
                                  float eps, float momentum, int groups, int defer_running_stats, const int32_t *const *knn_forced,
                                  int32_t *const *knn_log, float *feat, float *tmp, void *arena, size_t arena_bytes,
                                  const dvm_collective *coll, void *stream);
int dvm_uni3fc_train_bwd_sync_f32(const float *g_feat, const float *g_tmp, const float *dino, const float *feat, const float *tmp,
                                  int B, int N, const float *const *params, float *const *grads, int nparams, int k, int groups,
                                  void *arena, size_t arena_bytes, const dvm_collective *coll, void *stream);

/* The deformation part of GraphDeformLoss_Neural.forward in TRAINING, natively — models/loss.py:1228-1296 (deform(), both
 * directions), the Deformer models/model.py:454-478 and its MLP 433-452; the weighting 1413-1432 stays with the caller.
 * The B pairs of a step are handled as ONE batch of P = 2B directional pairs [(1 -> 2) x B | (2 -> 1) x B]:
 *   feat [P][N][C=128], verts [P][N][3]  : the B first shapes followed by the B second shapes (LG-Net's merged training call
 *                                          and the batched graph build lay them out like this); pair p maps shape p onto
 *                                          shape (p + B) mod P
 *   nodes_idx [P][N/2], ring [P][N/2][9], infl_idx [P][N][3], weights [P][N][3] : dvm_dg_build_f32 of verts
 *   knn_idx [P][N][k]                    : dvm_knn_cdist_f32(verts, verts, k)
 *   params: DVM_CRIT_TRAIN_NPARAMS device pointers — Deformer.conv_layer.weight [k], .bias [1], then the decoder's
 *           (weight, bias) x 4: [512][262], [512], [256][512], [256], [128][256], [128], [9][128], [9]
 *   dist term (models/loss.py:1351-1396), n_anchors > 0: dist1 / dist2 [B][N][N] the geodesic matrices of the first / second shapes,
 *           anchors1 / anchors2 [n_anchors] the anchor draws, k_dist <= 512 neighbours — what dvm_dist_loss_fwd_f32 takes, for all 2B
 *           shapes; runs on the helper stream of the caller's dvm_pair_init context beside the deformation part.  n_anchors == 0: off.
 * fwd -> terms [P][7] = [map numerator (0 when with_map == 0) | mean d(warped -> target), mean d(target -> warped) |
 *        mean d(verts12 -> target), mean d(target -> verts12) | ARAP | dist term of SHAPE p (0 when off)]; everything the backward
 *        needs stays in `arena` (dvm_criterion_train_workspace_bytes bytes, caller-owned, untouched until the matching bwd).
 * bwd: g_terms [P][7] = dL / d terms -> d_feat [P][N][C] (overwritten; the coordinates carry no gradient), the parameter
 *      gradients ADDED into grads[i] (fp32 atomics; same indexing as params).
 * N a multiple of 4 in 64..8192, k <= 16, topk <= 10, neg_alpha < 0 as in dvm_softcorr_fwd_f32. */
#define DVM_CRIT_TRAIN_NPARAMS 10
size_t dvm_criterion_train_workspace_bytes(int B, int N, int k, int topk, int n_anchors, int k_dist);
int dvm_criterion_train_fwd_f32(const float *feat, const float *verts, const int32_t *nodes_idx, const int32_t *ring,
                                const int32_t *infl_idx, const float *weights, const int32_t *knn_idx, int B, int N, int C, int k,
                                int topk, float neg_alpha, const float *const *params, int nparams, int with_map, const float *dist1,
                                const float *dist2, const int32_t *anchors1, const int32_t *anchors2, int n_anchors, int k_dist,
                                float *terms, void *arena, size_t arena_bytes, void *stream);
int dvm_criterion_train_bwd_f32(const float *g_terms, const float *feat, const float *verts, const int32_t *nodes_idx,
                                const int32_t *ring, const int32_t *infl_idx, const float *weights, const int32_t *knn_idx, int B,
                                int N, int C, int k, int topk, float neg_alpha, const float *const *params, float *const *grads,
                                int nparams, int with_map, const int32_t *anchors1, const int32_t *anchors2, int n_anchors, int k_dist,
                                float *d_feat, void *arena, size_t arena_bytes, void *stream);

/* The same node for ONE direction of deform() with sources of N and targets of M points (the partial-shape configs:
 * GraphDeformLoss_Neural_Partial, models/loss.py:986-1073; train_partial.py:93-112): P pairs, feat_s [P][N][128] / verts_s [P][N][3] /
 * knn_s [P][N][k] and the graph of the SOURCES, feat_t [P][M][128] / verts_t [P][M][3] / knn_t [P][M][k] of the targets.
 * -> terms [P][7] as above (column 6 = 0: the dist term stays with the caller); bwd -> d_feat_s [P][N][128], d_feat_t [P][M][128]
 * (overwritten), parameter gradients ADDED.  N, M in 64..8192 (any parity). */
size_t dvm_criterion_dir_train_workspace_bytes(int P, int N, int M, int k, int topk);
int dvm_criterion_dir_train_fwd_f32(const float *feat_s, const float *feat_t, const float *verts_s, const float *verts_t,
                                    const int32_t *nodes_idx, const int32_t *ring, const int32_t *infl_idx, const float *weights,
                                    const int32_t *knn_s, const int32_t *knn_t, int P, int N, int M, int C, int k, int topk,
                                    float neg_alpha, const float *const *params, int nparams, int with_map, float *terms, void *arena,
                                    size_t arena_bytes, void *stream);
int dvm_criterion_dir_train_bwd_f32(const float *g_terms, const float *feat_s, const float *feat_t, const float *verts_s,
                                    const float *verts_t, const int32_t *nodes_idx, const int32_t *ring, const int32_t *infl_idx,
                                    const float *weights, const int32_t *knn_s, const int32_t *knn_t, int P, int N, int M, int C, int k,
                                    int topk, float neg_alpha, const float *const *params, float *const *grads, int nparams, int with_map,
                                    float *d_feat_s, float *d_feat_t, void *arena, size_t arena_bytes, void *stream);

/* dvm_pair_fwd_f32 can run its coordinate-only chain (FPS, graph, xyz kNN: latency-bound) on helper streams, forked
 * from and joined back into `stream` by events, next to the feature-only soft-correspondence chain.  The helper streams
 * and events are NOT created by the compute call: dvm_pair_init(stream) makes them for (current device, `stream`) —
 * idempotent, the one call of this library that allocates HIP objects — and dvm_pair_destroy() frees every context of
 * the process.  A dvm_pair_fwd_f32 on a (device, stream) without a context runs everything on `stream`: same results,
 * no overlap.  Contexts are per caller stream, so calls on distinct streams / devices / host threads never share an
 * event; calls on the SAME stream must come from one thread at a time (as for any stream-ordered API).
 * dvm_pair_set_overlap(0) ignores the contexts (A/B measurements); returns the previous setting.
 * Environment default: DVM_PAIR_OVERLAP=0. */
int dvm_pair_init(void *stream);
int dvm_pair_destroy(void);
int dvm_pair_set_overlap(int on);

#ifdef __cplusplus
}
#endif
#endif /* DVM_H */
