// dvm_internal.h — every dvm:: function that one translation unit of libdvm_hip.so defines and another one calls, declared
// ONCE, grouped by the file that defines it (with the workspace struct or constants its callers need); default arguments appear
// here and nowhere else.  Included at the end of
// dvm_common.h: no .hip file declares a function it does not define.  (What the K1 sweep's own files call of each other, whose
// signatures need its argument structs, is in dvm_softcorr_f16.h; the Frobenius-norm terms' frob_finish in dvm_frob.h; set_error / prof_* / options and their kin, defined in dvm_api.cpp, in dvm_common.h.)
#pragma once

namespace dvm {

// ---- dvm_dist_loss.hip
// dvm_dist_loss_fwd_f32 with the sum at out[b * out_stride + out_off]; idx_out, xsave ([B][nA][k] x 2: x_j, y_j), fa_out: NULL or kept for the backward
int launch_dist_loss_fwd(const float *feat, const float *dist, const int32_t *anchors, int B, int N, int C, int nA, int k, float *out, int out_stride,
                         int out_off, int32_t *idx_out, float *xsave, float *fa_out, void *ws, size_t ws_bytes, hipStream_t s);
// W [B][nA][N] (zeroed here) and its row sums: x_j in float64 from feat [B][N][128], y_j from the forward's xsave; gterm read at gterm[b * gstride]
void launch_dist_loss_bwd_weights_saved(const float *feat, const int32_t *anchors, const float *xsave, const int32_t *idx, const float *gterm,
                                        int gstride, int B, int N, int nA, int k, float *W, float *rs, hipStream_t s);

// ---- dvm_bn.hip
int launch_bn_running_update(float *const *rm, float *const *rv, const float *const *mean, const float *const *var, const int *C, int count, float
                             momentum, hipStream_t s);

// ---- dvm_deformer.hip
void launch_pool_all(const float *feat, const int32_t *idx, int B, int P, int k, const float *cw, const float *cb, float *out, hipStream_t s, const
                     int32_t *order = nullptr);
size_t mlp_pack_floats();
// z [rows][264] -> out [rows][9]; wp = scratch of mlp_pack_floats() floats; variant as dvm_deformer_fwd_f32
void launch_mlp_rows(const float *z, int rows, const float *W0, const float *b0, const float *W1, const float *b1, const float *W2, const float *b2,
                     const float *W3, const float *b3, float *wp, float *out, hipStream_t s, int variant, void *zp);
int launch_deformer(const float *feat1, const float *feat2, const float *verts1, const float *verts12, const int32_t *idx11, const int32_t *idx22,
                    const float *pi_val, const int32_t *pi_idx, const int32_t *fps1, int B, int N, int M, int Nn, int k, int topk, const float
                    *conv_w, const float *conv_b, const float *W0, const float *b0, const float *W1, const float *b1, const float *W2, const float
                    *b2, const float *W3, const float *b3, float *out, int variant, void *ws, size_t ws_bytes, hipStream_t s);
size_t deformer_ws_bytes(int B, int M, int Nn);
// both directions of the pair path in one launch; planes: the plane form (z*), else the fp32 rows behind `gate`
void launch_assemble_pooled_pair(const float *verts1, const float *verts2, const float *verts12, const float *verts21, const float *g1, const float
                                 *g2, const float *val12, const int32_t *idx12, const float *val21, const int32_t *idx21, const int32_t *nodes1, const
                                 int32_t *nodes2, int B, int N, int M, void *z12, void *z21, bool planes, const int *gate, hipStream_t s);
// variant 0 on rows that are in the plane form already; returns the range flag for launch_mlp_fallback
const int *launch_mlp_planes(const void *zp, int rows, const float *W0, const float *b0, const float *W1, const float *b1, const float *W2, const
                             float *b2, const float *W3, const float *b3, float *wp, float *out, hipStream_t s);
// the bf16x3 kernel on the fp32 rows, gated on the flag
void launch_mlp_fallback(const float *z, int rows, const float *W0, const float *b0, const float *W1, const float *b1, const float *W2, const float
                         *b2, const float *W3, const float *b3, float *wp, float *out, hipStream_t s, const int *flag);

// ---- dvm_gemm.hip
void launch_linear(const float *x, const float *w, int B, int N, int K, int Co, int channel_major, const float *bias, const float *res, const float
                   *alpha, const float *beta, float slope, float *y, hipStream_t s, const float *xg, int Cg, const float *post_res, float post_scale);
// dW[b] [Co][K] += gy[b]^T x[b] for nb products of one shape, operands and results back to back (dW zeroed by the caller)
void launch_wgrad_batched(const float *gy, const float *x, int nb, long R, int Co, int K, float *dW, hipStream_t s);
void launch_linear_bmm(const float *x, const float *w, int B, int N, int K, int Co, float *y, hipStream_t s);

// ---- dvm_geom.hip
int launch_reduce_partials(const double *partial, int B, int nparts, float scale, float *out, int stride, int off, hipStream_t s);
int launch_mean_grouped(const float *const *in, const int *n, float *const *out, const int *off, int ngroups, int B, float scale, int stride,
                        hipStream_t s);
int map_term_blocks(int N, int k);
int launch_map_term(const float *verts12, const float *verts2, const int32_t *idx11, const int32_t *idx22, const float *pi_val, const int32_t *pi_idx,
                    int B, int N, int M, int k, int topk, double *partial, hipStream_t s, float *resid = nullptr);
// out [B][N][C] = Pi V, the launches of dvm_softcorr_apply_f32 (topk <= 16; every index in [0, M))
void launch_apply(const float *pi_val, const int32_t *pi_idx, const float *V, int B, int N, int M, int topk, int C, float *out, hipStream_t s);
void launch_apply_bwd_dval(const float *pi_val, const int32_t *pi_idx, const float *V, const float *g_out, int B, int N, int M, int topk, int C, float
                           *d_val, hipStream_t s);
void launch_apply_bwd_gather(const float *pi_val, const float *g_out, const int32_t *offs, const int32_t *edges, int B, int N, int M, int topk, int C,
                             float *d_V, hipStream_t s);
int launch_mean(const float *in, int B, int n, float scale, float *out, int stride, int off, hipStream_t s);   // launch_mean_grouped with one input
void launch_gather_nbr_xyz(const float *verts, const int32_t *idx, int B, int M, int k, float *nbr, hipStream_t s);
int launch_map_term_nbr(const float *verts12, const float *nbr2, const int32_t *idx11, const float *pi_val, const int32_t *pi_idx, int B, int N, int
                        M, int k, int topk, double *partial, hipStream_t s);
// -> true if the LDS form ran (topk == 10, the target side fits 150 KB of LDS); else the caller uses one of the older forms
bool launch_map_term_lds(const float *verts12, const float *verts2, const int32_t *idx11, const int32_t *idx22, const float *pi_val, const int32_t
                         *pi_idx, int B, int N, int M, int k, int topk, double *partial, hipStream_t s);
bool map_term_lds_applies(int N, int M, int k);
bool launch_map_term_lds_pair(const float *verts12, const float *verts21, const float *verts1, const float *verts2, const int32_t *idx11, const
                              int32_t *idx22, const float *val12, const int32_t *pidx12, const float *val21, const int32_t *pidx21, int B, int N, int
                              M, int k, int topk, double *partial12, double *partial21, hipStream_t s);
// -> false if a target cloud does not fit LDS (the caller then uses apply_kernel + take_col0)
bool launch_apply3_pair(const float *val12, const int32_t *idx12, const float *verts2, float *verts12, int32_t *T12, const float *val21, const int32_t
                        *idx21, const float *verts1, float *verts21, int32_t *T21, int B, int N, int M, hipStream_t s);

// ---- dvm_revlist.hip: reversed index lists by a counting sort (count, exclusive scan, fill)
// idx [B][E] (an entry with a target outside [0, M) is left out) -> offs [B][M+1], edges [B][E] (entries grouped by target).
// The entry record: int32_t = the entry number e; int2 = (e, e / K), the entry and its source row.
// The arrays as a workspace piece, B batches, M targets, E entries per batch: cursor [B][M] is scratch of the global route,
// hist [B][REV_DET_CHUNKS][M] (taken last, on request) that of the ordered one.
constexpr int REV_DET_CHUNKS = 64;
template <class Edge>
struct RevListsT {
    int32_t *offs = nullptr, *cursor = nullptr;
    Edge *edges = nullptr;
    int32_t *hist = nullptr;
    void take(Arena &ar, size_t B, size_t M, size_t E, bool ordered = false) {
        offs = ar.take<int32_t>(B * (M + 1));
        cursor = ar.take<int32_t>(B * M);
        edges = ar.take<Edge>(B * E);
        if (ordered) hist = ar.take<int32_t>(B * REV_DET_CHUNKS * M);
    }
};
typedef RevListsT<int32_t> RevLists;
// global: count, scan and fill as three launches of global atomics; LDS: one workgroup per batch element (needs (2 M + 1) ints
// of LDS and E < 2^31); ordered: REV_DET_CHUNKS histograms, every list in ascending entry order, no atomics between threads
// (needs M ints of LDS and r.hist)
enum RevRoute { REV_GLOBAL, REV_LDS, REV_ORDERED };
RevRoute rev_route(int B, long E, int M);   // the N2P backward's rule
template <class Edge>
void launch_rev_lists(const int32_t *idx, int B, long E, int M, int K, const RevListsT<Edge> &r, RevRoute route, hipStream_t s);
static inline void launch_rev_csr(const int32_t *idx, int B, long E, int M, const RevLists &r, hipStream_t s, RevRoute route = REV_GLOBAL) {
    launch_rev_lists(idx, B, E, M, 1, r, route, s);
}

// ---- dvm_graph.hip
// The largest cloud a deformation graph is built on: fps_kernel keeps the cloud in LDS (12288 * 12 B = 144 KiB) and 24 points
// per thread at 512 threads.  dvm_fps_f32, dvm_dg_build_f32 and the pair entries refuse a larger one before they launch anything.
constexpr int DVM_MAX_POINTS = 12288;
// launch_dg_build: DVM_EINVAL with nothing launched for N > DVM_MAX_POINTS (every later kernel gathers through nodes_idx)
int launch_dg_warp(const float *xyz, int B, int N, const int32_t *nodes_idx, const int32_t *ring, const int32_t *infl_idx, const float *weights, const
                   float *def9, float *R, float *T, float *warped, float *arap, int arap_stride, float *sr, hipStream_t s);
int launch_dg_build(const float *xyz, int B, int N, const int32_t *start, int32_t *nodes_idx, int32_t *ring, int32_t *infl_idx, float *dists, float
                    *weights, double *sigma, double *nnd, const GridBuf &gverts, const GridBuf &gnodes, bool build_gverts, hipStream_t s, hipEvent_t
                    gverts_ready = nullptr);
bool launch_dg_warp_pair(const float *xyz1, const float *xyz2, int B, int N, int M, const int32_t *const nodes[2], const int32_t *const ring[2], const
                         int32_t *const infl[2], const float *const weights[2], const float *def9_12, const float *def9_21, float *R12, float *R21,
                         float *T12, float *T21, float *warped12, float *warped21, float *arap12, float *arap21, int arap_stride, hipStream_t s);

// ---- dvm_dg_geod.hip: skinning and rings by a caller-supplied distance matrix
// vertices per workgroup (one lane each); most waves that share a tile's node range; longest ring; the wave count below which
// the node range is split, and the fewest node rows a wave is left with
constexpr int DG_GEOD_TILE = 64, DG_GEOD_MAX_SLICES = 8, DG_GEOD_MAX_RING = 16, DG_GEOD_TARGET_WAVES = 4096, DG_GEOD_MIN_SLICE = 16;
// dvm_dg_skin_geod_f32 without its checks; slices: waves per tile, 0 = dg_skin_geod_slices(B, N, Nn)
void launch_dg_skin_geod(const float *dist, const int32_t *nodes_idx, int B, int N, int Nn, int ring_k, int32_t *infl_idx, float *dists, int32_t *ring,
                         hipStream_t s, int slices = 0);
void launch_dg_skin_weights(const float *dists, const double *sigma, int B, int N, float *weights, hipStream_t s);

// ---- dvm_grid.hip: uniform-grid neighbour search over GridBuf (dvm_common.h)
size_t grid_bytes(int B, int P);
GridBuf grid_carve(Arena &ar, int B, int P);
void launch_grid_build(const float *xyz, int B, int Nsrc, const int32_t *sel, const GridBuf &gb, hipStream_t s);
void launch_grid_build_sets(const float *const *xyz, const int *Nsrc, const GridBuf *gb, int nsets, int B, hipStream_t s);   // up to 4 cloud sets, one launch
void launch_grid_knn_self(const GridBuf &gb, int B, int k, int32_t *idx, hipStream_t s);
void launch_grid_ring(const GridBuf &gnodes, int B, int32_t *ring, hipStream_t s);
void launch_grid_infl(const float *xyz, int B, int N, const GridBuf &gnodes, const GridBuf &gverts, int32_t *infl, float *dists, double *nnd,
                      hipStream_t s);
void launch_grid_chamfer(const GridBuf *gq, const GridBuf *gb, float *const *dout, int32_t *const *iout, int ngroups, int B, hipStream_t s);

// ---- dvm_knn.hip
// idx [B][N][k] = the k largest of s_ij = -|a_i - b_j|^2 per row of a [B][N][C] against bq [B][M][C], ties to the lower column; na, nb, S: scratch
int launch_knn_neg(const float *a, const float *bq, int B, int N, int M, int C, int k, int32_t *idx, float *na, float *nb, float *S, hipStream_t s);
// that scratch: the norms of both sides and the scores [B][N][M]
struct KnnNegWs {
    float *na, *nb, *S;
};
size_t carve_knn_neg(Arena &ar, int B, int N, int M, KnnNegWs &w);

// ---- dvm_loss_bwd.hip
void launch_dg_warp_arap_bwd(const float *xyz, int B, int N, const int32_t *nodes_idx, const int32_t *ring, const int32_t *infl_idx, const float
                             *weights, const float *R, const float *T, const float *g_warped, const float *g_arap, int garap_stride, float *d_R, float
                             *d_T, hipStream_t s);
void launch_def9_bwd(const float *def9, const float *dR, const float *dT, int rows, float *ddef9, hipStream_t s);
void launch_chamfer_bwd_src2(const float *a0, const float *a1, const float *b0, const float *b1, const int32_t *i1a, const int32_t *i2a, const int32_t
                             *i1b, const int32_t *i2b, const float *gt, int gstride, int off0, int off1, int B, int N, int M, float *da0, float *da1,
                             hipStream_t s);

// ---- dvm_mlp_bf16.hip
size_t mlp_bf16_pack_bytes();
void launch_mlp_rows_bf16(const float *z, int rows, const float *W0, const float *b0, const float *W1, const float *b1, const float *W2, const float
                          *b2, const float *W3, const float *b3, void *scratch, float *out, hipStream_t s, const int *gate);

// ---- dvm_mlp_f16.hip
size_t mlp_f16_pack_bytes();
void launch_split_rows(const float *z, int rows, int stride, void *zp, hipStream_t s);
int *launch_mlp_planes_f16(const void *zp, int rows, const float *W0, const float *b0, const float *W1, const float *b1, const float *W2, const float
                           *b2, const float *W3, const float *b3, void *scratch, float *out, hipStream_t s);
size_t mlp_zplane_bytes(int rows);   // bytes of the plane form of `rows` z rows (padded to whole 64-row blocks)
size_t mlp_zplane_row_bytes();   // MH_SZ

// ---- the SA attention core (dvm_sa.hip, dvm_sa_bwd.hip): channels of p and of v, padded p row of the staged tiles (floats)
constexpr int SA_P = 16, SA_C = 64, SA_LDP = 20;

// ---- dvm_sa_f16.hip: fp16x2-split kernels of the SA attention core
size_t sa_f16_carve(Arena &ar, int B, int N, _Float16 *&pp, _Float16 *&vp);   // the split planes of p and v, carved from the caller's arena
void launch_sa_split_f16(const float *p, const float *v, int B, int N, _Float16 *pp, _Float16 *vp, hipStream_t s);
void launch_sa_rowstats_f16(const _Float16 *pp, int B, int N, int kchunk, int Z, float *stats, hipStream_t s);
void launch_sa_apply_f16(const _Float16 *pp, const _Float16 *vp, const float *stats, int B, int N, int kchunk, int Z, float *xr, float *cinv,
                         hipStream_t s);

// ---- dvm_softcorr.hip
void launch_rownorm2(const float *x, int rows, int K, float *out, hipStream_t s);
// K == 128 only: also maxes the bit pattern of max |x| into the 256 slots of `absmax_slots` (zero them first);
// launch_absmax_finalize folds nt x 256 slots into nt values
void launch_rownorm2_absmax(const float *x, int rows, float *out, int *absmax_slots, hipStream_t s);
void launch_absmax_finalize(const int *slots, int nt, int *out, hipStream_t s);

// ---- dvm_softcorr_k1.hip: the fp16-split sweep (K1), d = 128
// The two sides of a call: features f[0] [B][rows[0]][128], f[1] [B][rows[1]][128] and their squared row norms n[sd] [B][rows[sd]]
// — buffers the call's preparation WRITES (launch_argmin_f16 takes them from its own workspace and ignores these).  Direction d =
// rows of side d against side d ^ 1: direction 0 always, direction 1 with `both`.
struct K1Sides {
    const float *f[2];
    float *n[2];
    int B, rows[2];
    bool both;
    long total(int sd) const { return (long)B * rows[sd]; }
    int dirs() const { return both ? 2 : 1; }
};
// one direction's outputs: top-`topk` values / columns and the optional row statistics; the hard map and its optional distances
struct K1SoftOut {
    float *val;
    int32_t *idx;
    float *smax, *sum;
};
struct K1HardOut {
    int32_t *T;
    float *dmin;
};
// how norms, scale and planes are made: norms + absmax, then the split (two passes over the features), or the pair path's one pass
enum K1Prep { K1_PREP_TWO_PASS, K1_PREP_FUSED };
// out[d] = direction d's outputs (out[1] is read only with c.both); topk <= 10
int launch_softcorr_f16(const K1Sides &c, const K1SoftOut *out, float neg_alpha, int topk, K1Prep prep, void *ws, size_t ws_bytes, hipStream_t s);
size_t softcorr_f16_ws_bytes(int B, int N, int M, bool both);
// the norms of both sides and, with k1, the K1 workspace behind them: ONE layout for dvm_softcorr_fwd_f32 and the hard map
struct K1NormsWs {
    float *n1, *n2;
    char *k1ws;
    size_t k1_bytes;
};
size_t carve_k1_norms(Arena &ar, int B, int N, int M, bool both, bool k1, K1NormsWs &w);
int launch_argmin_f16(const K1Sides &c, const K1HardOut *out, void *ws, size_t ws_bytes, hipStream_t s);
size_t argmin_f16_ws_bytes(int B, int N, int M, bool both);

// ---- the fp32 soft-correspondence family's entry points (dvm_softcorr.hip, dvm_softcorr_bwd.hip, dvm_sinkhorn.hip,
// dvm_sinkhorn_bwd.hip): the checks of the arguments they share, in the order every entry tests them; `who` names the entry.
// ptrs: the entry's own "all required pointers given".  variant in 0..variant_max.  n_iter_max < 0: no upper limit (and the
// defaults pass for an entry without n_iter or tau).
static inline int softcorr_family_check(const char *who, bool ptrs, int B, int N, int M, int d, int topk, float neg_alpha, int variant,
                                        int variant_max, int n_iter = 0, int n_iter_max = -1, float tau_row = 1.f, float tau_col = 1.f) {
    DVM_REQUIRE(ptrs, "%s: null pointer", who);
    DVM_REQUIRE(B >= 1 && N >= 1 && M >= 1, "%s: empty input (B=%d N=%d M=%d)", who, B, N, M);
    DVM_REQUIRE(d >= 4 && d % 4 == 0 && d <= 512, "%s: d=%d unsupported (need d%%4==0, 4<=d<=512)", who, d);
    DVM_REQUIRE(topk >= 1 && topk <= 16, "%s: topk=%d unsupported (1..16)", who, topk);
    if (n_iter_max < 0)
        DVM_REQUIRE(n_iter >= 0, "%s: n_iter=%d must not be negative", who, n_iter);
    else
        DVM_REQUIRE(n_iter >= 0 && n_iter <= n_iter_max, "%s: n_iter=%d unsupported (0..%d)", who, n_iter, n_iter_max);
    DVM_REQUIRE(neg_alpha < 0.f, "%s: neg_alpha must be negative (got %g)", who, (double)neg_alpha);
    DVM_REQUIRE(tau_row > 0.f && tau_row <= 1.f && tau_col > 0.f && tau_col <= 1.f, "%s: tau=(%g, %g) outside (0, 1]", who, (double)tau_row,
                (double)tau_col);
    if (variant_max == 1)
        DVM_REQUIRE(variant == 0 || variant == 1, "%s: bad variant %d (0 = auto, 1 = scalar)", who, variant);
    else
        DVM_REQUIRE(variant >= 0 && variant <= variant_max, "%s: bad variant %d", who, variant);
    return DVM_OK;
}

}  // namespace dvm
