// dvm_softcorr_hardmap.hip — the hard map's own kernels; norms, planes and the candidate lists come from the K1 sweep it shares
// with the soft correspondence (dvm_softcorr_f16.h; the sequence: launch_argmin_f16, dvm_softcorr_k1.hip).
#include "dvm_softcorr_f16.h"

namespace dvm {
namespace {

using namespace k1;

// ---------------------------------------------------------------- hard map (knnsearch_t) on the same sweep
// T[i] = argmin_j sqrt(sum_c (q_c - k_c)^2) in the reference's exact-difference form (models/loss.py:91-95,
// test.py:19-23): sequential sub / mul / add over the feature index, ties -> lowest j.  That form cannot run on the
// matrix cores, but it only has to be evaluated for the columns that can still be the minimum: pass A's candidate
// list holds the smallest mm-form distances up to its error bound E (na + nk) (coarse screen: 16 entries, HC_ERR; first form:
// 12, HB_ERR); the exact-difference value differs from the real distance by at most (d + 1) ulp-relative.  A column is
// examined when its approximate squared distance is within 2 (E + AM_DIFF) (na + nkmax) of the row's smallest; a row whose
// band reaches past its list (duplicate points, tight clusters) is re-done by a full exact scan.  The coarse screen's band is
// 40 x the first form's: if it sends more than 1 / 16 of a direction's rows to the full scan, that direction is swept again by
// the first form (argmin_gate_kernel: the extra launches are gated on the device, nothing is read back).
constexpr float AM_DIFF = 2e-5f;   // the exact-difference form against the real distance, relative to the norms

__device__ __forceinline__ float diff_d2(const float *__restrict__ q, const float *__restrict__ k) {
    float acc = 0.f;
#pragma unroll 8
    for (int c = 0; c < HB_D; c += 4) {
        const f32x4 qv = *(const f32x4 *)(q + c), kv = *(const f32x4 *)(k + c);
        const float e0 = qv.x - kv.x, e1 = qv.y - kv.y, e2 = qv.z - kv.z, e3 = qv.w - kv.w;
        const float p0 = e0 * e0, p1 = e1 * e1, p2 = e2 * e2, p3 = e3 * e3;
        acc = acc + p0;
        acc = acc + p1;
        acc = acc + p2;
        acc = acc + p3;
    }
    return acc;
}

struct AMGroup {
    const float *q, *k, *nq, *nkmax;
    int N, M;
    const int32_t *cidx;
    const float *cd2;
    int32_t *T;
    float *dmin;
    int32_t *flagged, *nflagged;
};
struct AMArgs {
    AMGroup g[2];
    long rows0, rows_total;
    const int *route;   // per (group, batch entry): K1_ROUTE_LEAN = this direction was swept again by the first form; nullptr: no gate
    int nb;
};

// KC / ERR: list length and error bound of the screen that made the lists.  GATED: the second pass (first-form lists) — only
// the directions the gate sent back.
template <int KC, bool COARSE, bool GATED>
__global__ __launch_bounds__(256) void argmin_refine_kernel(const AMArgs args) {
    long row = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= args.rows_total) return;
    const int grp = row >= args.rows0 ? 1 : 0;
    row -= grp ? args.rows0 : 0;
    if (GATED && args.route[grp * args.nb] != K1_ROUTE_LEAN) return;
    const AMGroup &G = args.g[grp];
    const int b = (int)(row / G.N);
    const float *q = G.q + (size_t)row * HB_D;
    const float band = 2.f * ((COARSE ? HC_ERR : HB_ERR) + AM_DIFF) * (G.nq[row] + G.nkmax[b]);
    const float v0 = G.cd2[row * KC];
    float best = INFINITY;
    int bj = 0x7fffffff;
    // does the band reach past the list?  It does not once a listed column lies beyond it: every column outside the list is
    // at or above the list's last valid entry.  (A list may hold fewer than KC valid entries: the coarse screen drops what
    // lies above its completeness bound.)
    bool open = true;
    for (int t = 0; t < KC; ++t) {
        const float v = G.cd2[row * KC + t];
        const int j = G.cidx[row * KC + t];
        if (j < 0 || j >= G.M) break;
        if (!(v <= v0 + band)) {
            open = false;
            break;
        }
        const float dv = sqrt_rn(diff_d2(q, G.k + ((size_t)b * G.M + j) * HB_D));
        if (dv < best || (dv == best && j < bj)) best = dv, bj = j;
    }
    if (open && G.M > KC) {
        G.flagged[atomicAdd(G.nflagged, 1)] = (int32_t)row;
        return;
    }
    G.T[row] = bj;
    if (G.dmin) G.dmin[row] = best;
}

// after the coarse pass: a direction with more than 1 / 16 of its rows flagged goes through the first form again (its flag list is
// emptied; the gated launches behind this kernel return at once for the other direction)
__global__ void argmin_gate_kernel(const AMArgs args, int dirs, int *route) {
    const int d = threadIdx.x;
    if (d >= dirs) return;
    const long rows = d ? args.rows_total - args.rows0 : args.rows0;
    const bool again = *args.g[d].nflagged > (rows >> 4);
    if (again) *args.g[d].nflagged = 0;
    for (int b = 0; b < args.nb; ++b) route[d * args.nb + b] = again ? K1_ROUTE_LEAN : K1_ROUTE_COARSE;
}

// full exact scan of the flagged rows, one workgroup per row
__global__ __launch_bounds__(256) void argmin_exact_rows_kernel(const AMArgs args) {
    __shared__ float sd[256];
    __shared__ int sj[256];
    for (int grp = 0; grp < 2; ++grp) {
        const AMGroup &G = args.g[grp];
        if (!G.flagged) continue;
        const int cnt = *G.nflagged;
        for (int f = blockIdx.x; f < cnt; f += gridDim.x) {
            const long row = G.flagged[f];
            const int b = (int)(row / G.N);
            const float *q = G.q + (size_t)row * HB_D;
            float best = INFINITY;
            int bj = 0x7fffffff;
            for (int j = threadIdx.x; j < G.M; j += 256) {  // ascending j per thread: strict < keeps the lowest
                const float dv = sqrt_rn(diff_d2(q, G.k + ((size_t)b * G.M + j) * HB_D));
                if (dv < best) best = dv, bj = j;
            }
            __syncthreads();
            sd[threadIdx.x] = best;
            sj[threadIdx.x] = bj;
            __syncthreads();
            for (int o = 128; o > 0; o >>= 1) {
                if ((int)threadIdx.x < o) {
                    const float od = sd[threadIdx.x + o];
                    const int oj = sj[threadIdx.x + o];
                    if (od < sd[threadIdx.x] || (od == sd[threadIdx.x] && oj < sj[threadIdx.x])) sd[threadIdx.x] = od, sj[threadIdx.x] = oj;
                }
                __syncthreads();
            }
            if (threadIdx.x == 0) {
                G.T[row] = sj[0];
                if (G.dmin) G.dmin[row] = sd[0];
            }
        }
    }
}

// (without `both`, group 1 is empty)
static AMArgs am_args(const K1Sides &c, const K1HardOut *out, const K1Ws &w, const int *route) {
    AMArgs r{};
    for (int d = 0; d < c.dirs(); ++d)
        r.g[d] = AMGroup{c.f[d], c.f[d ^ 1], c.n[d], w.nmax[d ^ 1], c.rows[d], c.rows[d ^ 1], w.cidx[d], w.cd2[d], out[d].T, out[d].dmin,
                         w.flag[d] + 1, w.flag[d]};
    r.rows0 = c.total(0);
    r.rows_total = r.rows0 + (c.both ? c.total(1) : 0);
    r.route = route;
    r.nb = c.B;
    return r;
}

}  // namespace

void k1::launch_argmin_refine(const K1Sides &c, const K1HardOut *out, const K1Ws &w, int pass, bool have_coarse, hipStream_t s) {
    const AMArgs r = am_args(c, out, w, pass == 1 && have_coarse ? w.route : nullptr);
    const dim3 rgrid((unsigned)((r.rows_total + 255) / 256));
    if (pass == 0) {
        hipLaunchKernelGGL((argmin_refine_kernel<K1_KC_COARSE, true, false>), rgrid, dim3(256), 0, s, r);
        hipLaunchKernelGGL(argmin_gate_kernel, dim3(1), dim3(64), 0, s, r, c.dirs(), w.route);
        return;
    }
    if (have_coarse) hipLaunchKernelGGL((argmin_refine_kernel<HB_KC, false, true>), rgrid, dim3(256), 0, s, r);
    else hipLaunchKernelGGL((argmin_refine_kernel<HB_KC, false, false>), rgrid, dim3(256), 0, s, r);
    hipLaunchKernelGGL(argmin_exact_rows_kernel, dim3(512), dim3(256), 0, s, r);
}

}  // namespace dvm
