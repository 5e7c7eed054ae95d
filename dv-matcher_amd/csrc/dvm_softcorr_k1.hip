// dvm_softcorr_k1.hip — the host side of the fp16-split sweep (K1; kernels and steps: dvm_softcorr_f16.h): the workspace layout,
// the launch plan, and the two launchers — soft correspondence (launch_softcorr_f16) and hard map (launch_argmin_f16).
#include <vector>

#include "dvm_softcorr_f16.h"

namespace dvm {

using namespace k1;

// routing: Options::k1_route forces one route (K1_ROUTE_*: 0 full, 1 lean, 3 coarse; -1 = the probe decides), k1_p_coarse / k1_p_lean
// are the probe's thresholds (fractions of a row within the cut), DVM_DEBUG & 1 prints the routes of every launch (synchronous)
static void report_routes(const int *route, const float *frac, int n, hipStream_t s) {   // diagnostic
    std::vector<int> r(n);
    std::vector<float> p(n);
    (void)hipStreamSynchronize(s);
    (void)hipMemcpy(r.data(), route, n * sizeof(int), hipMemcpyDeviceToHost);
    (void)hipMemcpy(p.data(), frac, n * sizeof(float), hipMemcpyDeviceToHost);
    int cnt[4] = {0, 0, 0, 0};
    double ps = 0, pmin = 1, pmax = 0;
    for (int i = 0; i < n; ++i) {
        ++cnt[r[i] < 0 || r[i] > 3 ? 0 : r[i]];
        ps += p[i];
        pmin = p[i] < pmin ? p[i] : pmin;
        pmax = p[i] > pmax ? p[i] : pmax;
    }
    fprintf(stderr, "K1 routes: %d full, %d lean, %d coarse; fraction within the cut: mean %.4f%% (min %.4f%%, max %.4f%%)\n", cnt[0], cnt[1],
            cnt[3], 100 * ps / n, 100 * pmin, 100 * pmax);
}

// what the most recent launch_softcorr_f16 of this host thread did with its (direction, pair) entries: device pointers into the
// caller's workspace (valid until it is rewritten), read back by dvm_k1_last_routes
struct K1LastLaunch {
    const int *route = nullptr, *route2 = nullptr;   // first-pass routes (nullptr: `fixed` for every entry), the gate's second pass
    int n = 0, fixed = -1;
    hipStream_t s = nullptr;
};
static thread_local K1LastLaunch g_k1_last;

// The zero-initialised head comes first, one 256-byte slot after the other, so that one fill clears it (K1Ws::zero_bytes).
static size_t carve_k1(Arena &ar, int B, int N, int M, bool both, K1Ws &w) {
    const size_t head = ar.off;
    w.slots = ar.take<int>(2 * 256 + 2);
    w.nmax[0] = ar.take<float>(B), w.nmax[1] = ar.take<float>(B);
    w.amax = ar.take<int>(2);
    w.spec = ar.take<int>(2);
    w.zero_bytes = ar.off - head;
    w.p[0] = ar.take<char>((size_t)B * N * HB_ROWB), w.p[1] = ar.take<char>((size_t)B * M * HB_ROWB);
    w.pad[0] = (N + HB_KT - 1) / HB_KT * HB_KT, w.pad[1] = (M + HB_KT - 1) / HB_KT * HB_KT;
    w.npad[0] = ar.take<float>((size_t)B * w.pad[0]), w.npad[1] = ar.take<float>((size_t)B * w.pad[1]);
    w.nfrag[0] = ar.take<char>((size_t)B * w.pad[0] * 32), w.nfrag[1] = ar.take<char>((size_t)B * w.pad[1] * 32);
    w.route = ar.take<int>(2 * (size_t)B), w.route2 = ar.take<int>(2 * (size_t)B);
    w.pfrac = ar.take<float>(2 * (size_t)B);
    for (int d = 0; d < 2; ++d) w.cidx[d] = w.flag[d] = nullptr, w.cd2[d] = w.lsum[d] = nullptr;
    for (int d = 0; d < (both ? 2 : 1); ++d) {
        const size_t R = (size_t)B * (d == 0 ? N : M);
        w.cidx[d] = ar.take<int32_t>(R * K1_KC_COARSE);   // (candidate lists sized for the longest form's)
        w.cd2[d] = ar.take<float>(R * K1_KC_COARSE);
        w.lsum[d] = ar.take<float>(R * 2);
        w.flag[d] = ar.take<int32_t>(R + 1);
    }
    return ar.off;
}
size_t softcorr_f16_ws_bytes(int B, int N, int M, bool both) { return null_carve<K1Ws>(carve_k1, B, N, M, both); }

// What both launchers hand to the norm preparation and to pass A, from the one layout: norms c.n, ONE scale for both sides (the
// larger absmax) at w.amax[0], [1]; frags: the coarse screen's norm fragments are made.  Returns the number of pass-A workgroups.
static int k1_pass_a_args(const K1Sides &c, const K1Ws &w, bool frags, float neg_alpha, float cutw, const int *route, NormPrep &np, HBArgs &a) {
    np = NormPrep{{c.n[0], c.n[1]}, {c.rows[0], c.rows[1]}, {w.pad[0], w.pad[1]}, {w.nmax[0], w.nmax[1]}, {c.both ? w.npad[0] : nullptr, w.npad[1]},
                  {frags && c.both ? w.nfrag[0] : nullptr, frags ? w.nfrag[1] : nullptr}, w.amax, {w.flag[0], c.both ? w.flag[1] : nullptr}};
    for (int g = 0; g < 2; ++g) {   // direction d: side d's rows against side d ^ 1 (without `both`, group 1 repeats group 0)
        const int d = c.both ? g : 0, k = d ^ 1;
        a.g[g] = HBGroup{w.p[d], w.p[k], w.amax + d, w.amax + k, c.n[d], w.npad[k], c.rows[d], c.rows[k], w.pad[k], (c.rows[d] + HB_QB - 1) / HB_QB,
                         w.cidx[d], w.cd2[d], w.lsum[d]};
    }
    a.blocks0 = c.B * a.g[0].tiles;
    a.neg_alpha = neg_alpha, a.cutw = cutw;
    a.route = route;
    a.nb = c.B;
    return a.blocks0 + (c.both ? c.B * a.g[1].tiles : 0);
}

// alpha < 32: every softmax term counts, the first form in full.  From 32 on each (direction, pair) is routed by the
// probe; DVM_K1_ROUTE = 0 / 1 / 3 (K1_ROUTE_FULL / LEAN / COARSE) forces one kernel for all of them (A/B measurements,
// tests/test_gpu_k1_routes.py).
static K1Plan k1_plan(float neg_alpha, bool havec) {
    const int forced = options().k1_route;
    const bool lean = -neg_alpha >= 32.f;
    K1Plan p;
    p.routed = lean && forced < 0;
    p.fixed = !lean ? K1_ROUTE_FULL : forced < 0 ? -1 : (forced == K1_ROUTE_COARSE && havec) ? K1_ROUTE_COARSE : forced == K1_ROUTE_FULL ? K1_ROUTE_FULL : K1_ROUTE_LEAN;
    p.coarse = p.routed ? havec : p.fixed == K1_ROUTE_COARSE;
    return p;
}
// Outputs as the fp32 kernel: top-`topk` values / columns (topk <= 10), optional row stats.  prep: K1_PREP_FUSED makes the norms in the
// same pass that writes the planes (the pair path), K1_PREP_TWO_PASS in a pass of their own; either way c.n is written here.
int launch_softcorr_f16(const K1Sides &c, const K1SoftOut *out, float neg_alpha, int topk, K1Prep prep, void *ws, size_t ws_bytes, hipStream_t s) {
    K1Ws w;
    if (!carve_ws(ws, ws_bytes, "softcorr (fp16 path)", w, carve_k1, c.B, c.rows[0], c.rows[1], c.both)) return DVM_ENOSPACE;
    const K1Plan plan = k1_plan(neg_alpha, coarse_supports(c.rows[0], c.rows[1]));
    launch_prep(c, w, prep, s);
    if (plan.routed) {
        launch_probe(c, w, neg_alpha, plan.coarse, s);
        if (options().debug & DVM_DEBUG_K1_ROUTES) report_routes(w.route, w.pfrac, c.B * c.dirs(), s);
    }
    NormPrep np;
    HBArgs a;
    const int blocks = k1_pass_a_args(c, w, plan.coarse, neg_alpha, 20.f / -neg_alpha, plan.route(w), np, a);
    // the norms' maxima, the first form's padded norms (also behind the coarse screen, for the gate's second pass), the coarse
    // screen's norm fragments and the flagged-row counters: one launch
    launch_norm_prep(np, c.B, s);
    prof_note(DVM_PROF_K1_SWEEP, plan.routed ? (plan.coarse ? "routed: softcorr_coarse_kernel | softcorr_sweep_f16_kernel<lean> | softcorr_sweep_f16_kernel<full>"
                                                            : "routed: softcorr_sweep_f16_kernel<lean> | softcorr_sweep_f16_kernel<full>")
                                 : plan.fixed == K1_ROUTE_COARSE ? "softcorr_coarse_kernel"
                                 : plan.fixed == K1_ROUTE_LEAN   ? "softcorr_sweep_f16_kernel<lean>"
                                                                 : "softcorr_sweep_f16_kernel<full>");
    prof_begin(s);
    // (routed: the coarse screen and the routed first form are both launched; a workgroup whose pair belongs to the other returns at once)
    if (plan.coarse) launch_coarse(a, w.nfrag[1], w.nfrag[0], w.amax, blocks, s);
    if (plan.routed) launch_sweep_f16(a, blocks, K1_SWEEP_ROUTED, s);
    else if (plan.fixed != K1_ROUTE_COARSE) launch_sweep_f16(a, blocks, plan.fixed, s);
    prof_end(s);

    prof_begin(s, DVM_PROF_K1_REFINE);
    launch_refine(c, out, w, plan, neg_alpha, topk, false, s);
    if (plan.coarse) {   // the second pass behind the gate (k1_gate_kernel)
        a.route = w.route2;
        launch_sweep_f16(a, blocks, K1_SWEEP_GATED, s);
        launch_refine(c, out, w, plan, neg_alpha, topk, true, s);
    }
    prof_end(s, DVM_PROF_K1_REFINE);
    g_k1_last = K1LastLaunch{plan.route(w), plan.coarse ? w.route2 : nullptr, c.B * c.dirs(), plan.fixed, s};
    launch_exact_rows(c, out, w, neg_alpha, topk, s);
    return DVM_OK;
}

size_t carve_k1_norms(Arena &ar, int B, int N, int M, bool both, bool k1, K1NormsWs &w) {
    w.n1 = ar.take<float>((size_t)B * N), w.n2 = ar.take<float>((size_t)B * M);
    w.k1_bytes = k1 ? softcorr_f16_ws_bytes(B, N, M, both) : 0;
    w.k1ws = k1 ? ar.take<char>(w.k1_bytes) : nullptr;
    return ar.off;
}
size_t argmin_f16_ws_bytes(int B, int N, int M, bool both) { return null_carve<K1NormsWs>(carve_k1_norms, B, N, M, both, true); }

// hard maps out[0].T [B][N] of f1 -> f2 and, with `both`, out[1].T [B][M] of f2 -> f1; d = 128
int launch_argmin_f16(const K1Sides &sides, const K1HardOut *out, void *ws, size_t ws_bytes, hipStream_t s) {
    K1NormsWs nw;
    if (!carve_ws(ws, ws_bytes, "argmin (fp16 sweep)", nw, carve_k1_norms, sides.B, sides.rows[0], sides.rows[1], sides.both, true)) return DVM_ENOSPACE;
    Arena k1ar(nw.k1ws, nw.k1_bytes);   // (fits: carve_k1_norms sized it)
    K1Ws w;
    carve_k1(k1ar, sides.B, sides.rows[0], sides.rows[1], sides.both, w);
    K1Sides c = sides;
    c.n[0] = nw.n1, c.n[1] = nw.n2;
    launch_prep(c, w, K1_PREP_TWO_PASS, s);
    // coarse screen first (lists of 16), the first form behind the device-side gate for directions it serves badly
    const bool havec = coarse_supports(c.rows[0], c.rows[1]);
    NormPrep np;
    HBArgs a;
    // (alpha 100, no cut: only the candidate lists are used; the lean sweep keeps them exactly as the full one does)
    const int blocks = k1_pass_a_args(c, w, havec, -100.f, 0.f, nullptr, np, a);
    launch_norm_prep(np, c.B, s);
    if (havec) {
        launch_coarse(a, w.nfrag[1], w.nfrag[0], w.amax, blocks, s);
        launch_argmin_refine(c, out, w, 0, havec, s);
        a.route = w.route;
    }
    launch_sweep_f16(a, blocks, K1_ROUTE_LEAN, s);
    launch_argmin_refine(c, out, w, 1, havec, s);
    return DVM_OK;
}

}  // namespace dvm

// Diagnostic, SYNCHRONOUS (it waits for the launch's stream and copies a few hundred bytes to the host): which pass-A kernel the
// most recent soft-correspondence launch of this host thread sent its (direction, pair) entries to.  counts[0] = full first form,
// [1] = lean first form, [2] = coarse screen, [3] = entries the gate swept AGAIN with the lean form behind the coarse screen,
// [4] = entries in all.  Valid only while the launch's workspace has not been rewritten (call it right after the launch).
DVM_EXPORT int dvm_k1_last_routes(int *counts) {
    DVM_REQUIRE(counts, "dvm_k1_last_routes: null pointer");
    const dvm::K1LastLaunch &L = dvm::g_k1_last;
    for (int i = 0; i < 5; ++i) counts[i] = 0;
    DVM_REQUIRE(L.n > 0, "dvm_k1_last_routes: no soft-correspondence launch on this thread yet");
    counts[4] = L.n;
    if (hipStreamSynchronize(L.s) != hipSuccess) {
        dvm::set_error("dvm_k1_last_routes: stream synchronisation failed");
        return DVM_ELAUNCH;
    }
    std::vector<int> r(L.n, L.fixed), r2(L.n, -1);
    if (L.route && hipMemcpy(r.data(), L.route, L.n * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return DVM_ELAUNCH;
    if (L.route2 && hipMemcpy(r2.data(), L.route2, L.n * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return DVM_ELAUNCH;
    for (int i = 0; i < L.n; ++i) {
        counts[r[i] == dvm::k1::K1_ROUTE_COARSE ? 2 : r[i] == dvm::k1::K1_ROUTE_LEAN ? 1 : 0] += 1;
        if (r2[i] == dvm::k1::K1_ROUTE_LEAN) counts[3] += 1;
    }
    return DVM_OK;
}
