// Host-side sanitizer harness (test infrastructure): drives the C ABI's host code — argument validation, workspace
// sizing, arena carving, the context registry — under AddressSanitizer + UBSan.  No kernel is launched: every call
// either is a pure host function or is made with arguments that must be rejected before the launch (NULL pointers,
// bad sizes, a workspace one byte too small).  Run by tests/test_sanitizers.py on a machine without a GPU.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../../include/dvm.h"

static int fails = 0;
#define EXPECT(cond)                                                   \
    do {                                                               \
        if (!(cond)) {                                                 \
            printf("san_host: FAILED %s (line %d)\n", #cond, __LINE__); \
            ++fails;                                                   \
        }                                                              \
    } while (0)

int main() {
    EXPECT(dvm_abi_version() == DVM_ABI_VERSION);
    (void)dvm_device_count();
    // workspace queries: monotone in every size, never zero for real shapes, no overflow at the largest shipped shapes
    const int shapes[][3] = {{1, 20, 20}, {2, 256, 256}, {8, 2048, 2048}, {2, 4995, 2200}, {512, 2048, 2048}, {1, 8192, 8192}};
    size_t prev = 0;
    for (auto &sh : shapes) {
        const int B = sh[0], N = sh[1], M = sh[2];
        size_t a = dvm_softcorr_workspace_bytes(B, N, M, 128), b = dvm_pair_workspace_bytes(B, N, M),
               c = dvm_pair_direction_workspace_bytes(B, N, M), d = dvm_knn_neg_workspace_bytes(B, N, M, 128, 40),
               e = dvm_softcorr_bwd_workspace_bytes(B, N, M, 128), f = dvm_argmin_workspace_bytes(B, N, M, 128, 1),
               g = dvm_chamfer_workspace_bytes(B, N, M), h = dvm_dg_build_workspace_bytes(B, N), i = dvm_deformer_workspace_bytes(B, N, M, 10);
        EXPECT(a > 0 && b > 0 && c > 0 && d >= (size_t)B * N * M * 4 && e > 0 && f > 0 && g > 0 && h > 0 && i > 0);
        EXPECT(b >= c / 2);
        EXPECT(dvm_sinkhorn_workspace_bytes(B, N, M, 128) >= (size_t)8 * B * ((size_t)N + M));   // norms + potentials of both sides
        (void)prev;
        prev = b;
    }
    EXPECT(dvm_bn_workspace_bytes(8, 128, 2048) > 0 && dvm_sa_attention_workspace_bytes(8, 2048) > 0);
    EXPECT(dvm_pos_encoding_workspace_bytes() > 0 && dvm_proj2img_workspace_bytes(3) > 0);
    // argument validation: all of these must return DVM_EINVAL / DVM_ENOSPACE and set a message, touching nothing
    float dummy[64] = {0};
    int32_t idummy[64] = {0};
    EXPECT(dvm_softcorr_fwd_f32(nullptr, nullptr, 1, 8, 8, 128, -1.f, 10, nullptr, nullptr, nullptr, nullptr, 0, nullptr, 0, nullptr) == DVM_EINVAL);
    EXPECT(strlen(dvm_last_error()) > 0);
    EXPECT(dvm_softcorr_fwd_f32(dummy, dummy, 1, 8, 8, 128, +1.f, 10, dummy, idummy, dummy, dummy, 0, dummy, 64, nullptr) == DVM_EINVAL);   // alpha sign
    EXPECT(dvm_softcorr_fwd_f32(dummy, dummy, 1, 8, 8, 128, -1.f, 99, dummy, idummy, dummy, dummy, 0, dummy, 64, nullptr) == DVM_EINVAL);   // topk range
    // dvm_sinkhorn_fwd_f32: every rejection path, then a workspace one byte short of what the query asks for
    const size_t skb = dvm_sinkhorn_workspace_bytes(1, 8, 8, 128);
    std::vector<char> skws(skb);
    EXPECT(dvm_sinkhorn_workspace_bytes(0, 8, 8, 128) == 0);
    EXPECT(dvm_sinkhorn_fwd_f32(nullptr, nullptr, 1, 8, 8, 128, -1.f, 5, 10, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, 0, nullptr) == DVM_EINVAL);
    EXPECT(strstr(dvm_last_error(), "null pointer") != nullptr);
    EXPECT(dvm_sinkhorn_fwd_f32(dummy, dummy, 0, 8, 8, 128, -1.f, 5, 10, dummy, idummy, dummy, dummy, dummy, dummy, 0, skws.data(), skb, nullptr) == DVM_EINVAL);   // empty
    EXPECT(dvm_sinkhorn_fwd_f32(dummy, dummy, 1, 8, 8, 130, -1.f, 5, 10, dummy, idummy, dummy, dummy, dummy, dummy, 0, skws.data(), skb, nullptr) == DVM_EINVAL);   // d
    EXPECT(dvm_sinkhorn_fwd_f32(dummy, dummy, 1, 8, 8, 516, -1.f, 5, 10, dummy, idummy, dummy, dummy, dummy, dummy, 0, skws.data(), skb, nullptr) == DVM_EINVAL);   // d too large
    EXPECT(dvm_sinkhorn_fwd_f32(dummy, dummy, 1, 8, 8, 128, -1.f, 5, 17, dummy, idummy, dummy, dummy, dummy, dummy, 0, skws.data(), skb, nullptr) == DVM_EINVAL);   // topk range
    EXPECT(dvm_sinkhorn_fwd_f32(dummy, dummy, 1, 8, 8, 128, -1.f, 5, 0, dummy, idummy, dummy, dummy, dummy, dummy, 0, skws.data(), skb, nullptr) == DVM_EINVAL);
    EXPECT(dvm_sinkhorn_fwd_f32(dummy, dummy, 1, 8, 8, 128, -1.f, -1, 10, dummy, idummy, dummy, dummy, dummy, dummy, 0, skws.data(), skb, nullptr) == DVM_EINVAL);  // n_iter
    EXPECT(dvm_sinkhorn_fwd_f32(dummy, dummy, 1, 8, 8, 128, 0.f, 5, 10, dummy, idummy, dummy, dummy, dummy, dummy, 0, skws.data(), skb, nullptr) == DVM_EINVAL);    // alpha sign
    EXPECT(dvm_sinkhorn_fwd_f32(dummy, dummy, 1, 8, 8, 128, -1.f, 5, 10, dummy, idummy, dummy, dummy, dummy, dummy, 7, skws.data(), skb, nullptr) == DVM_EINVAL);   // variant
    EXPECT(dvm_sinkhorn_fwd_f32(dummy, dummy, 1, 8, 8, 128, -1.f, 5, 10, dummy, idummy, nullptr, nullptr, nullptr, nullptr, 0, skws.data(), skb - 1, nullptr) == DVM_ENOSPACE);
    EXPECT(strstr(dvm_last_error(), "workspace") != nullptr);
    EXPECT(dvm_sinkhorn_fwd_f32(dummy, dummy, 1, 8, 8, 128, -1.f, 5, 10, dummy, idummy, dummy, dummy, dummy, dummy, 0, nullptr, 0, nullptr) == DVM_ENOSPACE);
    // dvm_sinkhorn_fwd_hist_f32 / dvm_sinkhorn_bwd_f32: the same rejection paths
    const size_t shb = dvm_sinkhorn_hist_workspace_bytes(1, 8, 8, 128), sbb = dvm_sinkhorn_bwd_workspace_bytes(1, 8, 8, 128, 5);
    std::vector<char> shws(shb), sbws(sbb);
    EXPECT(shb >= (size_t)4 * (8 + 8) && sbb > shb);
    EXPECT(dvm_sinkhorn_hist_workspace_bytes(0, 8, 8, 128) == 0 && dvm_sinkhorn_bwd_workspace_bytes(1, 8, 8, 128, 33) == 0);
    EXPECT(dvm_sinkhorn_bwd_workspace_bytes(1, 8, 8, 128, 20) > sbb);   // grows with the history
    EXPECT(dvm_sinkhorn_fwd_hist_f32(dummy, dummy, 1, 8, 8, 128, -1.f, 5, 10, dummy, idummy, dummy, dummy, nullptr, dummy, 0, shws.data(), shb, nullptr) == DVM_EINVAL);
    EXPECT(strstr(dvm_last_error(), "null pointer") != nullptr);
    EXPECT(dvm_sinkhorn_fwd_hist_f32(dummy, dummy, 0, 8, 8, 128, -1.f, 5, 10, dummy, idummy, dummy, dummy, dummy, dummy, 0, shws.data(), shb, nullptr) == DVM_EINVAL);   // empty
    EXPECT(dvm_sinkhorn_fwd_hist_f32(dummy, dummy, 1, 8, 8, 130, -1.f, 5, 10, dummy, idummy, dummy, dummy, dummy, dummy, 0, shws.data(), shb, nullptr) == DVM_EINVAL);   // d
    EXPECT(dvm_sinkhorn_fwd_hist_f32(dummy, dummy, 1, 8, 8, 128, -1.f, 5, 17, dummy, idummy, dummy, dummy, dummy, dummy, 0, shws.data(), shb, nullptr) == DVM_EINVAL);   // topk
    EXPECT(dvm_sinkhorn_fwd_hist_f32(dummy, dummy, 1, 8, 8, 128, -1.f, -1, 10, dummy, idummy, dummy, dummy, dummy, dummy, 0, shws.data(), shb, nullptr) == DVM_EINVAL);  // n_iter
    EXPECT(dvm_sinkhorn_fwd_hist_f32(dummy, dummy, 1, 8, 8, 128, 0.f, 5, 10, dummy, idummy, dummy, dummy, dummy, dummy, 0, shws.data(), shb, nullptr) == DVM_EINVAL);    // alpha sign
    EXPECT(dvm_sinkhorn_fwd_hist_f32(dummy, dummy, 1, 8, 8, 128, -1.f, 5, 10, dummy, idummy, dummy, dummy, dummy, dummy, 7, shws.data(), shb, nullptr) == DVM_EINVAL);   // variant
    EXPECT(dvm_sinkhorn_fwd_hist_f32(dummy, dummy, 1, 8, 8, 128, -1.f, 5, 10, dummy, idummy, nullptr, nullptr, dummy, dummy, 0, shws.data(), shb - 1, nullptr) == DVM_ENOSPACE);
    EXPECT(strstr(dvm_last_error(), "workspace") != nullptr);
    EXPECT(dvm_sinkhorn_bwd_f32(dummy, dummy, 1, 8, 8, 128, -1.f, 5, 10, dummy, idummy, dummy, dummy, dummy, dummy, nullptr, 0, sbws.data(), sbb, nullptr) == DVM_EINVAL);
    EXPECT(strstr(dvm_last_error(), "null pointer") != nullptr);
    EXPECT(dvm_sinkhorn_bwd_f32(dummy, dummy, 1, 0, 8, 128, -1.f, 5, 10, dummy, idummy, dummy, dummy, dummy, dummy, dummy, 0, sbws.data(), sbb, nullptr) == DVM_EINVAL);   // empty
    EXPECT(dvm_sinkhorn_bwd_f32(dummy, dummy, 1, 8, 8, 516, -1.f, 5, 10, dummy, idummy, dummy, dummy, dummy, dummy, dummy, 0, sbws.data(), sbb, nullptr) == DVM_EINVAL);   // d
    EXPECT(dvm_sinkhorn_bwd_f32(dummy, dummy, 1, 8, 8, 128, -1.f, 5, 0, dummy, idummy, dummy, dummy, dummy, dummy, dummy, 0, sbws.data(), sbb, nullptr) == DVM_EINVAL);     // topk
    EXPECT(dvm_sinkhorn_bwd_f32(dummy, dummy, 1, 8, 8, 128, -1.f, 33, 10, dummy, idummy, dummy, dummy, dummy, dummy, dummy, 0, sbws.data(), sbb, nullptr) == DVM_EINVAL);   // n_iter limit
    EXPECT(strstr(dvm_last_error(), "n_iter") != nullptr);
    EXPECT(dvm_sinkhorn_bwd_f32(dummy, dummy, 1, 8, 8, 128, 1.f, 5, 10, dummy, idummy, dummy, dummy, dummy, dummy, dummy, 0, sbws.data(), sbb, nullptr) == DVM_EINVAL);     // alpha sign
    EXPECT(dvm_sinkhorn_bwd_f32(dummy, dummy, 1, 8, 8, 128, -1.f, 5, 10, dummy, idummy, dummy, dummy, dummy, dummy, dummy, 2, sbws.data(), sbb, nullptr) == DVM_EINVAL);    // variant
    EXPECT(dvm_sinkhorn_bwd_f32(dummy, dummy, 1, 8, 8, 128, -1.f, 5, 10, dummy, idummy, dummy, dummy, dummy, dummy, dummy, 0, sbws.data(), dvm_sinkhorn_bwd_workspace_bytes(1, 8, 8, 128, 0), nullptr) == DVM_ENOSPACE);
    EXPECT(strstr(dvm_last_error(), "workspace") != nullptr);
    EXPECT(dvm_sinkhorn_bwd_f32(dummy, dummy, 1, 8, 8, 128, -1.f, 5, 10, dummy, idummy, dummy, dummy, dummy, dummy, dummy, 0, nullptr, 0, nullptr) == DVM_ENOSPACE);
    // the unbalanced entries (dvm_sinkhorn_ub_*): the workspace queries, then the same rejection paths plus tau outside (0, 1]
    {
        const size_t ufb = dvm_sinkhorn_ub_workspace_bytes(1, 8, 8, 128), uhb = dvm_sinkhorn_ub_hist_workspace_bytes(1, 8, 8, 128),
                     ubb = dvm_sinkhorn_ub_bwd_workspace_bytes(1, 8, 8, 128, 5);
        std::vector<char> ufws(ufb), uhws(uhb), ubws(ubb);
        float *const F = dummy;
        int32_t *const I = idummy;
        EXPECT(ufb >= (size_t)8 * (8 + 8) && uhb >= (size_t)8 * (8 + 8) && ubb > sbb);   // bwd: a third group of planes and the re-made potentials
        EXPECT(dvm_sinkhorn_ub_workspace_bytes(0, 8, 8, 128) == 0 && dvm_sinkhorn_ub_hist_workspace_bytes(0, 8, 8, 128) == 0);
        EXPECT(dvm_sinkhorn_ub_bwd_workspace_bytes(0, 8, 8, 128, 5) == 0 && dvm_sinkhorn_ub_bwd_workspace_bytes(1, 8, 8, 128, 33) == 0);
        EXPECT(dvm_sinkhorn_ub_bwd_workspace_bytes(1, 8, 8, 128, 20) > ubb);   // grows with the history
        for (auto &sh : shapes) EXPECT(dvm_sinkhorn_ub_bwd_workspace_bytes(sh[0], sh[1], sh[2], 128, 32) > dvm_sinkhorn_bwd_workspace_bytes(sh[0], sh[1], sh[2], 128, 32));
#define UBF(B, d, na, T, k, tr, tc, var, ws, nb) dvm_sinkhorn_ub_fwd_f32(F, F, B, 8, 8, d, na, T, k, tr, tc, F, F, F, I, F, F, F, F, F, var, ws, nb, nullptr)
#define UBH(B, d, na, T, k, tr, tc, var, ws, nb) dvm_sinkhorn_ub_fwd_hist_f32(F, F, B, 8, 8, d, na, T, k, tr, tc, F, F, F, I, F, F, F, F, F, var, ws, nb, nullptr)
#define UBB(B, d, na, T, k, tr, tc, var, ws, nb) \
    dvm_sinkhorn_ub_bwd_f32(F, F, B, 8, 8, d, na, T, k, tr, tc, F, F, F, I, F, F, F, F, F, F, F, F, F, var, ws, nb, nullptr)
        EXPECT(dvm_sinkhorn_ub_fwd_f32(nullptr, nullptr, 1, 8, 8, 128, -1.f, 5, 10, .9f, .9f, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                       nullptr, nullptr, 0, nullptr, 0, nullptr) == DVM_EINVAL);
        EXPECT(strstr(dvm_last_error(), "null pointer") != nullptr);
        EXPECT(dvm_sinkhorn_ub_fwd_hist_f32(F, F, 1, 8, 8, 128, -1.f, 5, 10, .9f, .9f, F, F, F, I, F, F, F, nullptr, F, 0, uhws.data(), uhb, nullptr) == DVM_EINVAL);
        EXPECT(strstr(dvm_last_error(), "null pointer") != nullptr);
        EXPECT(dvm_sinkhorn_ub_bwd_f32(F, F, 1, 8, 8, 128, -1.f, 5, 10, .9f, .9f, F, F, F, I, nullptr, F, F, F, F, F, F, F, F, 0, ubws.data(), ubb, nullptr) == DVM_EINVAL);
        EXPECT(strstr(dvm_last_error(), "null pointer") != nullptr);
        EXPECT(UBF(0, 128, -1.f, 5, 10, .9f, .9f, 0, ufws.data(), ufb) == DVM_EINVAL && UBH(0, 128, -1.f, 5, 10, .9f, .9f, 0, uhws.data(), uhb) == DVM_EINVAL &&
               UBB(0, 128, -1.f, 5, 10, .9f, .9f, 0, ubws.data(), ubb) == DVM_EINVAL);   // empty
        EXPECT(UBF(1, 130, -1.f, 5, 10, .9f, .9f, 0, ufws.data(), ufb) == DVM_EINVAL && UBH(1, 516, -1.f, 5, 10, .9f, .9f, 0, uhws.data(), uhb) == DVM_EINVAL &&
               UBB(1, 130, -1.f, 5, 10, .9f, .9f, 0, ubws.data(), ubb) == DVM_EINVAL);   // d
        EXPECT(UBF(1, 128, -1.f, 5, 17, .9f, .9f, 0, ufws.data(), ufb) == DVM_EINVAL && UBH(1, 128, -1.f, 5, 0, .9f, .9f, 0, uhws.data(), uhb) == DVM_EINVAL &&
               UBB(1, 128, -1.f, 5, 17, .9f, .9f, 0, ubws.data(), ubb) == DVM_EINVAL);   // topk
        EXPECT(UBF(1, 128, -1.f, -1, 10, .9f, .9f, 0, ufws.data(), ufb) == DVM_EINVAL && UBH(1, 128, -1.f, -1, 10, .9f, .9f, 0, uhws.data(), uhb) == DVM_EINVAL &&
               UBB(1, 128, -1.f, 33, 10, .9f, .9f, 0, ubws.data(), ubb) == DVM_EINVAL);   // n_iter (the backward's limit is 32)
        EXPECT(strstr(dvm_last_error(), "n_iter") != nullptr);
        EXPECT(UBF(1, 128, 0.f, 5, 10, .9f, .9f, 0, ufws.data(), ufb) == DVM_EINVAL && UBH(1, 128, 1.f, 5, 10, .9f, .9f, 0, uhws.data(), uhb) == DVM_EINVAL &&
               UBB(1, 128, 0.f, 5, 10, .9f, .9f, 0, ubws.data(), ubb) == DVM_EINVAL);   // alpha sign
        EXPECT(UBF(1, 128, -1.f, 5, 10, 0.f, .9f, 0, ufws.data(), ufb) == DVM_EINVAL && UBF(1, 128, -1.f, 5, 10, .9f, 1.5f, 0, ufws.data(), ufb) == DVM_EINVAL);
        EXPECT(strstr(dvm_last_error(), "tau") != nullptr);
        EXPECT(UBH(1, 128, -1.f, 5, 10, -.5f, .9f, 0, uhws.data(), uhb) == DVM_EINVAL && UBB(1, 128, -1.f, 5, 10, .9f, 0.f, 0, ubws.data(), ubb) == DVM_EINVAL);
        EXPECT(strstr(dvm_last_error(), "tau") != nullptr);
        EXPECT(UBF(1, 128, -1.f, 5, 10, .9f, .9f, 7, ufws.data(), ufb) == DVM_EINVAL && UBH(1, 128, -1.f, 5, 10, .9f, .9f, 2, uhws.data(), uhb) == DVM_EINVAL &&
               UBB(1, 128, -1.f, 5, 10, .9f, .9f, 2, ubws.data(), ubb) == DVM_EINVAL);   // variant
        EXPECT(UBF(1, 128, -1.f, 5, 10, 1.f, 1.f, 0, ufws.data(), ufb - 1) == DVM_ENOSPACE && strstr(dvm_last_error(), "workspace") != nullptr);
        EXPECT(UBH(1, 128, -1.f, 5, 10, 1.f, 1.f, 0, uhws.data(), uhb - 1) == DVM_ENOSPACE && strstr(dvm_last_error(), "workspace") != nullptr);
        EXPECT(UBB(1, 128, -1.f, 5, 10, 1.f, 1.f, 0, ubws.data(), dvm_sinkhorn_ub_bwd_workspace_bytes(1, 8, 8, 128, 0)) == DVM_ENOSPACE);
        EXPECT(strstr(dvm_last_error(), "workspace") != nullptr);
        EXPECT(UBF(1, 128, -1.f, 5, 10, .9f, .9f, 0, nullptr, 0) == DVM_ENOSPACE && UBH(1, 128, -1.f, 5, 10, .9f, .9f, 0, nullptr, 0) == DVM_ENOSPACE &&
               UBB(1, 128, -1.f, 5, 10, .9f, .9f, 0, nullptr, 0) == DVM_ENOSPACE);
#undef UBF
#undef UBH
#undef UBB
    }
    // the rank term: sized without any N x N / M x M array, refused over its row limit before any launch
    {
        const int nmax = dvm_rank_term_max_n();
        const size_t rb = dvm_rank_term_workspace_bytes(2, 300, 170, 10);
        std::vector<char> rws(rb);
        EXPECT(nmax >= 8192 && rb >= (size_t)4 * 2 * (2 * 170 + 1 + 300 * 10) + 8 * 2 * 300 && rb < (size_t)64 * 1024);
        EXPECT(dvm_rank_term_workspace_bytes(1, nmax, 1 << 20, 16) > 0 && dvm_rank_term_workspace_bytes(1, nmax + 1, 64, 1) == 0);
        EXPECT(dvm_rank_term_workspace_bytes(0, 8, 8, 4) == 0 && dvm_rank_term_workspace_bytes(1, 8, 8, 17) == 0);
        EXPECT(dvm_rank_term_f32(nullptr, idummy, 2, 300, 170, 10, dummy, nullptr, rws.data(), rb, nullptr) == DVM_EINVAL);
        EXPECT(strstr(dvm_last_error(), "null pointer") != nullptr);
        EXPECT(dvm_rank_term_f32(dummy, idummy, 2, 300, 170, 17, dummy, dummy, rws.data(), rb, nullptr) == DVM_EINVAL);
        EXPECT(dvm_rank_term_f32(dummy, idummy, 1, nmax + 1, 64, 1, dummy, nullptr, rws.data(), rb, nullptr) == DVM_EINVAL);
        EXPECT(strstr(dvm_last_error(), "N=") != nullptr);
        EXPECT(dvm_rank_term_f32(dummy, idummy, 2, 300, 170, 10, dummy, dummy, rws.data(), rb - 1, nullptr) == DVM_ENOSPACE);
        EXPECT(strstr(dvm_last_error(), "workspace") != nullptr);
        EXPECT(dvm_rank_term_f32(dummy, idummy, 2, 300, 170, 10, dummy, nullptr, nullptr, 0, nullptr) == DVM_ENOSPACE);
    }
    // the cycle term: the same frame; its sizes hold the samples (B N k12 k21 floats) and no N x N / N x M array, both gradients or none
    {
        float *const F = dummy;
        int32_t *const I = idummy;
        const int nmax = dvm_cycle_term_max_n();
        const size_t cb = dvm_cycle_term_workspace_bytes(2, 300, 170, 10, 10);
        std::vector<char> cws(cb);
        EXPECT(nmax >= 8192 && cb >= (size_t)4 * 2 * (2 * 170 + 1 + 300 * 10 + 300 * 100) + 8 * 2 * 300 && cb < (size_t)2 * 300 * 170 * 4);
        EXPECT(dvm_cycle_term_workspace_bytes(1, nmax, 1 << 20, 16, 16) > 0 && dvm_cycle_term_workspace_bytes(1, nmax + 1, 64, 1, 1) == 0);
        EXPECT(dvm_cycle_term_workspace_bytes(0, 8, 8, 4, 4) == 0 && dvm_cycle_term_workspace_bytes(1, 8, 8, 17, 4) == 0 &&
               dvm_cycle_term_workspace_bytes(1, 8, 8, 4, 17) == 0 && dvm_cycle_term_workspace_bytes(65536, 8, 8, 4, 4) == 0);
#define CYC(v12, B, N, M, k12, k21, g12, g21, ws, nb) dvm_cycle_term_f32(v12, I, F, I, B, N, M, k12, k21, F, g12, g21, ws, nb, nullptr)
        EXPECT(CYC(nullptr, 2, 300, 170, 10, 10, nullptr, nullptr, cws.data(), cb) == DVM_EINVAL && strstr(dvm_last_error(), "null pointer"));
        EXPECT(CYC(F, 2, 300, 0, 10, 10, F, F, cws.data(), cb) == DVM_EINVAL && strstr(dvm_last_error(), "empty input"));
        EXPECT(CYC(F, 65536, 300, 170, 10, 10, F, F, cws.data(), cb) == DVM_EINVAL && strstr(dvm_last_error(), "B=65536"));
        EXPECT(CYC(F, 2, 300, 170, 17, 10, F, F, cws.data(), cb) == DVM_EINVAL && strstr(dvm_last_error(), "k12=17"));
        EXPECT(CYC(F, 2, 300, 170, 10, 0, F, F, cws.data(), cb) == DVM_EINVAL && strstr(dvm_last_error(), "k21=0"));
        EXPECT(CYC(F, 1, nmax + 1, 64, 1, 1, nullptr, nullptr, cws.data(), cb) == DVM_EINVAL && strstr(dvm_last_error(), "N="));
        EXPECT(CYC(F, 2, 300, 170, 10, 10, F, nullptr, cws.data(), cb) == DVM_EINVAL && strstr(dvm_last_error(), "both"));
        EXPECT(CYC(F, 2, 300, 170, 10, 10, nullptr, F, cws.data(), cb) == DVM_EINVAL && strstr(dvm_last_error(), "both"));
        EXPECT(CYC(F, 2, 300, 170, 10, 10, F, F, cws.data(), cb - 1) == DVM_ENOSPACE && strstr(dvm_last_error(), "workspace"));
        EXPECT(CYC(F, 2, 300, 170, 10, 10, nullptr, nullptr, nullptr, 0) == DVM_ENOSPACE);
#undef CYC
    }
    // the distortion term: B N doubles and B floats whatever M and topk; N and M each have the limit
    {
        float *const F = dummy;
        int32_t *const I = idummy;
        const int nmax = dvm_distortion_term_max_n();
        const size_t db = dvm_distortion_term_workspace_bytes(2, 300, 170, 10);
        std::vector<char> dws(db);
        EXPECT(nmax >= 8192 && db >= (size_t)8 * 2 * 300 + 4 * 2 && db < (size_t)16 * 1024);
        EXPECT(dvm_distortion_term_workspace_bytes(1, nmax, nmax, 16) > 0 && dvm_distortion_term_workspace_bytes(1, nmax + 1, 64, 1) == 0 &&
               dvm_distortion_term_workspace_bytes(1, 64, nmax + 1, 1) == 0);
        EXPECT(dvm_distortion_term_workspace_bytes(0, 8, 8, 4) == 0 && dvm_distortion_term_workspace_bytes(1, 8, 8, 17) == 0 &&
               dvm_distortion_term_workspace_bytes(65536, 8, 8, 4) == 0);
#define DST(d1, B, N, M, k, g, ws, nb) dvm_distortion_term_f32(F, I, d1, F, B, N, M, k, F, g, ws, nb, nullptr)
        EXPECT(DST(nullptr, 2, 300, 170, 10, nullptr, dws.data(), db) == DVM_EINVAL && strstr(dvm_last_error(), "null pointer"));
        EXPECT(DST(F, 2, 0, 170, 10, F, dws.data(), db) == DVM_EINVAL && strstr(dvm_last_error(), "empty input"));
        EXPECT(DST(F, 65536, 300, 170, 10, F, dws.data(), db) == DVM_EINVAL && strstr(dvm_last_error(), "B=65536"));
        EXPECT(DST(F, 2, 300, 170, 17, F, dws.data(), db) == DVM_EINVAL && strstr(dvm_last_error(), "topk=17"));
        EXPECT(DST(F, 1, nmax + 1, 64, 1, nullptr, dws.data(), db) == DVM_EINVAL && strstr(dvm_last_error(), "N="));
        EXPECT(DST(F, 1, 64, nmax + 1, 1, nullptr, dws.data(), db) == DVM_EINVAL && strstr(dvm_last_error(), "M="));
        EXPECT(DST(F, 1, nmax + 1, nmax + 1, 1, nullptr, dws.data(), db) == DVM_EINVAL && strstr(dvm_last_error(), "N="));   // N is reported first
        EXPECT(DST(F, 2, 300, 170, 10, F, dws.data(), db - 1) == DVM_ENOSPACE && strstr(dvm_last_error(), "workspace"));
        EXPECT(DST(F, 2, 300, 170, 10, nullptr, nullptr, 0) == DVM_ENOSPACE);
#undef DST
    }
    EXPECT(dvm_linear_f32(nullptr, dummy, 1, 4, 4, 4, 0, nullptr, nullptr, nullptr, nullptr, 1.f, dummy, nullptr) == DVM_EINVAL);
    EXPECT(dvm_linear_f32(dummy, dummy, 1, 4, 4, 4, 0, nullptr, nullptr, dummy, nullptr, 1.f, dummy, nullptr) == DVM_EINVAL);               // alpha without beta
    EXPECT(dvm_linear_f32(dummy, dummy, 1, 4, 100000, 4, 0, nullptr, nullptr, nullptr, nullptr, 1.f, dummy, nullptr) == DVM_EINVAL);        // K too large
    EXPECT(dvm_linear_prefix_f32(dummy, 6, dummy, dummy, 1, 4, 16, 4, nullptr, nullptr, nullptr, nullptr, 1.f, dummy, nullptr) == DVM_EINVAL);   // Cg % 4
    EXPECT(dvm_knn_neg_f32(dummy, dummy, 1, 4, 4, 4, 9, idummy, dummy, 64, nullptr) == DVM_EINVAL);                                        // k > M
    EXPECT(dvm_knn_neg_f32(dummy, dummy, 1, 4, 4, 4, 2, idummy, dummy, 8, nullptr) == DVM_ENOSPACE);                                       // workspace too small
    EXPECT(dvm_knn_neg_f32(dummy, dummy, 1, 4, 4, 4, 2, idummy, nullptr, 0, nullptr) == DVM_ENOSPACE);
    EXPECT(dvm_pair_fwd_f32(nullptr, nullptr, nullptr, nullptr, 1, 64, 64, -1.f, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                            nullptr, nullptr, nullptr, nullptr, nullptr, 1, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                            nullptr, 0, nullptr) == DVM_EINVAL);
    EXPECT(dvm_rot6d_f32(nullptr, 4, nullptr, nullptr) == DVM_EINVAL);
    EXPECT(dvm_pair_geometry_f32(nullptr, nullptr, 1, 64, 64, nullptr, nullptr, 1, nullptr, 0, nullptr) == DVM_EINVAL);
    EXPECT(dvm_pair_geometry_f32(dummy, dummy, 1, 64, 64, idummy, idummy, 1, nullptr, 0, nullptr) == DVM_ENOSPACE);
    // every entry point with a workspace: valid small sizes, a non-null workspace, one byte less than its query asks for ->
    // DVM_ENOSPACE and a message that says what was too small, before anything is launched (the buffers are never touched)
    {
        const int B = 1, N = 64, M = 64, d = 128, k = 10;
        float *const F = dummy;
        int32_t *const I = idummy;
        double dd[8] = {0};
        void *const ws = dummy;
        const float *ptab[DVM_U3_TRAIN_NPARAMS];
        float *gtab[DVM_U3_TRAIN_NPARAMS];
        for (int q = 0; q < DVM_U3_TRAIN_NPARAMS; ++q) ptab[q] = F, gtab[q] = F;
        static_assert(DVM_U3_TRAIN_NPARAMS >= DVM_U3_NWEIGHTS && DVM_U3_TRAIN_NPARAMS >= DVM_CRIT_TRAIN_NPARAMS, "one table serves all three");
        const dvm_collective coll = {[](void *, void *, size_t, int, int, void *) { return 0; }, nullptr};
        size_t q = 0;
#define SHORT(query, call)                                                                    \
    do {                                                                                      \
        q = (query);                                                                          \
        EXPECT(q > 0);                                                                        \
        EXPECT((call) == DVM_ENOSPACE);                                                       \
        EXPECT(strstr(dvm_last_error(), "workspace too small") || strstr(dvm_last_error(), "arena too small")); \
    } while (0)
        const int det = dvm_set_deterministic(1);   // (the weight gradient uses its workspace in the deterministic mode only)
        SHORT(dvm_linear_wgrad_workspace_bytes(4096, 128, 128), dvm_linear_wgrad_ws_f32(F, F, 4096, 128, 128, F, ws, q - 1, nullptr));
        dvm_set_deterministic(det);
        SHORT(dvm_softcorr_workspace_bytes(B, N, M, d), dvm_softcorr_fwd_f32(F, F, B, N, M, d, -1.f, 10, F, I, F, F, 0, ws, q - 1, nullptr));
        SHORT(dvm_softcorr_workspace_bytes(B, N, M, 64), dvm_softcorr_fwd_f32(F, F, B, N, M, 64, -1.f, 10, F, I, F, F, 0, ws, q - 1, nullptr));
        SHORT(dvm_softcorr_bwd_workspace_bytes(B, N, M, d), dvm_softcorr_bwd_f32(F, F, B, N, M, d, -1.f, 10, F, I, F, F, F, F, F, 0, ws, q - 1, nullptr));
        SHORT(dvm_argmin_workspace_bytes(B, N, M, d, 0), dvm_argmin_exact_f32(F, F, B, N, M, d, I, F, ws, q - 1, nullptr));
        SHORT(dvm_argmin_workspace_bytes(B, N, M, d, 1), dvm_argmin_pair_f32(F, F, B, N, M, d, I, I, F, F, ws, q - 1, nullptr));
        SHORT(dvm_knn_cdist_workspace_bytes(B, N, N, 3), dvm_knn_cdist_f32(F, F, B, N, N, 3, k, I, ws, q - 1, nullptr));
        SHORT(dvm_knn_neg_workspace_bytes(B, N, M, d, k), dvm_knn_neg_f32(F, F, B, N, M, d, k, I, ws, q - 1, nullptr));
        SHORT(dvm_softcorr_dense_workspace_bytes(B, N, M, d), dvm_softcorr_dense_f32(F, F, B, N, M, d, -1.f, F, ws, q - 1, nullptr));
        SHORT(dvm_softcorr_apply_bwd_workspace_bytes(B, N, M, 10), dvm_softcorr_apply_bwd_f32(F, I, F, F, B, N, M, 10, 3, F, F, ws, q - 1, nullptr));
        SHORT(dvm_dg_build_workspace_bytes(B, N), dvm_dg_build_f32(F, B, N, I, I, I, I, F, F, dd, ws, q - 1, nullptr));
        SHORT(dvm_dg_build_geod_workspace_bytes(B, N), dvm_dg_build_geod_f32(F, F, B, N, I, 1, I, I, I, F, F, dd, ws, q - 1, nullptr));
        // ... and the refusals of the geodesic skinning, which has no workspace: too few nodes, a ring longer than the node list or
        // than 16, a cloud above the FPS limit, a bad ring metric
        EXPECT(dvm_dg_skin_geod_f32(F, I, B, N, 2, 0, I, F, nullptr, nullptr) == DVM_EINVAL);
        EXPECT(dvm_dg_skin_geod_f32(F, I, B, N, 8, 9, I, F, I, nullptr) == DVM_EINVAL);
        EXPECT(dvm_dg_skin_geod_f32(F, I, B, N, N / 2, 17, I, F, I, nullptr) == DVM_EINVAL);
        EXPECT(dvm_dg_skin_geod_slices_f32(F, I, B, N, N / 2, 9, 9, I, F, I, nullptr) == DVM_EINVAL);
        EXPECT(dvm_dg_skin_weights_f32(F, nullptr, B, N, F, nullptr) == DVM_EINVAL);
        EXPECT(dvm_dg_build_geod_f32(F, F, B, 12289, I, 0, I, I, I, F, F, dd, ws, q, nullptr) == DVM_EINVAL);
        EXPECT(dvm_dg_build_geod_f32(F, F, B, N, I, 2, I, I, I, F, F, dd, ws, q, nullptr) == DVM_EINVAL);
        // the precise map: a short workspace, then its refusals — a null required pointer, sizes below 1, a d that is no multiple
        // of 4 or above 512, M above the cap (the size query answers 0 there), a plan query without its outputs
        SHORT(dvm_precise_map_workspace_bytes(B, N, M, d, 32), dvm_precise_map_f32(F, F, I, B, N, M, d, 32, I, F, I, F, nullptr, ws, q - 1, nullptr));
        {
            int64_t st[2];
            int pr = 0, pt = 0, pc = 0, pm = 0;
            const int cap = dvm_precise_map_max_m();
            EXPECT(dvm_precise_map_f32(nullptr, F, I, B, N, M, d, 32, I, F, I, F, st, ws, q, nullptr) == DVM_EINVAL);
            EXPECT(dvm_precise_map_f32(F, F, nullptr, B, N, M, d, 32, I, F, I, F, st, ws, q, nullptr) == DVM_EINVAL);
            EXPECT(dvm_precise_map_f32(F, F, I, B, N, M, d, 32, I, nullptr, I, F, st, ws, q, nullptr) == DVM_EINVAL);
            EXPECT(dvm_precise_map_f32(F, F, I, 0, N, M, d, 32, I, F, I, F, st, ws, q, nullptr) == DVM_EINVAL);
            EXPECT(dvm_precise_map_f32(F, F, I, B, 0, M, d, 32, I, F, I, F, st, ws, q, nullptr) == DVM_EINVAL);
            EXPECT(dvm_precise_map_f32(F, F, I, B, N, 0, d, 32, I, F, I, F, st, ws, q, nullptr) == DVM_EINVAL);
            EXPECT(dvm_precise_map_f32(F, F, I, B, N, M, d, 0, I, F, I, F, st, ws, q, nullptr) == DVM_EINVAL);
            EXPECT(dvm_precise_map_f32(F, F, I, B, N, M, 130, 32, I, F, I, F, st, ws, q, nullptr) == DVM_EINVAL);
            EXPECT(dvm_precise_map_f32(F, F, I, B, N, M, 516, 32, I, F, I, F, st, ws, q, nullptr) == DVM_EINVAL);
            EXPECT(dvm_precise_map_f32(F, F, I, B, N, cap + 1, d, 32, I, F, I, F, st, ws, q, nullptr) == DVM_EINVAL);
            EXPECT(strstr(dvm_last_error(), "dvm_precise_map_max_m"));
            EXPECT(dvm_precise_map_workspace_bytes(B, N, cap + 1, d, 32) == 0 && dvm_precise_map_workspace_bytes(B, N, cap, d, 32) == q);
            EXPECT(dvm_precise_map_plan(B, N, M, d, 32, &pr, &pt, &pc, nullptr) == DVM_EINVAL);
            EXPECT(dvm_precise_map_plan(B, N, cap + 1, d, 32, &pr, &pt, &pc, &pm) == DVM_EINVAL);
            EXPECT(dvm_precise_map_plan(B, N, M, d, 32, &pr, &pt, &pc, &pm) == DVM_OK && pr >= 1 && pt % 64 == 0 && pc >= 1 && pm == cap);
        }
        SHORT(dvm_chamfer_workspace_bytes(B, 8192, 8192), dvm_chamfer_fwd_f32(F, F, B, 8192, 8192, F, F, I, I, ws, q - 1, nullptr));   // (large enough for the grid form)
        SHORT(dvm_deformer_workspace_bytes(B, N, M, N / 2),
              dvm_deformer_fwd_f32(F, F, F, F, I, I, F, I, I, B, N, M, N / 2, k, 10, F, F, F, F, F, F, F, F, F, F, F, 0, ws, q - 1, nullptr));
        SHORT(dvm_deformer_mlp_workspace_bytes(N), dvm_deformer_mlp_fwd_f32(F, N, F, F, F, F, F, F, F, F, F, ws, q - 1, nullptr));
        SHORT(dvm_pos_encoding_workspace_bytes(), dvm_pos_encoding_f32(F, B, N, F, ws, q - 1, nullptr));
        SHORT(dvm_pos_encoding_workspace_bytes(), dvm_pos_encoding_sync_f32(F, B, N, F, ws, q - 1, &coll, F, nullptr));
        SHORT(dvm_bn_workspace_bytes(B, d, N), dvm_bn_act_train_fwd_f32(F, nullptr, F, F, B, d, N, 1e-5f, 0.2f, 0.1f, F, F, F, nullptr, nullptr, ws, q - 1, nullptr));
        SHORT(dvm_bn_workspace_bytes(B, d, N), dvm_bn_act_train_bwd_f32(F, F, F, nullptr, F, F, F, B, d, N, 0.2f, F, F, F, ws, q - 1, nullptr));
        SHORT(dvm_bn_pm_workspace_bytes(N, d),
              dvm_bn_act_train_fwd_pm_f32(F, nullptr, F, F, N, d, 1e-5f, 0.2f, 0.1f, F, F, F, nullptr, nullptr, ws, q - 1, nullptr));
        SHORT(dvm_bn_pm_workspace_bytes(N, d), dvm_bn_act_train_bwd_pm_f32(F, F, F, nullptr, F, F, F, N, d, 0.2f, F, F, F, 0, ws, q - 1, nullptr));
        SHORT(dvm_bn_pm_groups_workspace_bytes(N, d, 2),
              dvm_bn_act_train_fwd_pm_var_f32(F, nullptr, F, F, N, d, 2, 1e-5f, 0.2f, 0.1f, F, F, F, F, nullptr, nullptr, ws, q - 1, nullptr));
        SHORT(dvm_bn_pm_groups_workspace_bytes(N, d, 2),
              dvm_bn_act_train_fwd_pm_sync_f32(F, nullptr, F, F, N, d, 2, 1e-5f, 0.2f, 0.1f, F, F, F, F, nullptr, nullptr, ws, q - 1, &coll, dd, nullptr));
        SHORT(dvm_bn_pm_groups_workspace_bytes(N, d, 2),
              dvm_bn_act_train_bwd_pm_groups_f32(F, F, F, nullptr, F, F, F, N, d, 2, 0.2f, F, F, F, 0, ws, q - 1, nullptr));
        SHORT(dvm_bn_pm_groups_workspace_bytes(N, d, 2),
              dvm_bn_act_train_bwd_pm_sync_f32(F, F, F, nullptr, F, F, F, N, d, 2, 0.2f, F, F, F, 0, ws, q - 1, &coll, dd, nullptr));
        SHORT(dvm_proj2img_workspace_bytes(B), dvm_proj2img_f32(F, B, N, F, F, F, F, ws, q - 1, nullptr));
        SHORT(dvm_sa_attention_workspace_bytes(B, N), dvm_sa_attention_fwd_f32(F, F, B, N, F, ws, q - 1, nullptr));
        SHORT(dvm_sa_attention_bwd_workspace_bytes(B, N), dvm_sa_attention_bwd_f32(F, F, F, F, F, F, B, N, F, F, ws, q - 1, nullptr));
        SHORT(dvm_n2p_core_bwd_workspace_bytes(B, N, 16), dvm_n2p_core_bwd_f32(F, I, F, F, B, N, d, 16, 4, F, ws, q - 1, nullptr));
        SHORT(dvm_dist_loss_workspace_bytes(B, N, d, 16, k), dvm_dist_loss_fwd_f32(F, F, I, B, N, d, 16, k, F, I, ws, q - 1, nullptr));
        SHORT(dvm_map_term_workspace_bytes(B, N), dvm_map_term_f32(F, F, I, I, F, I, B, N, M, 16, 10, F, ws, q - 1, nullptr));
        SHORT(dvm_rank_term_workspace_bytes(B, N, M, 10), dvm_rank_term_f32(F, I, B, N, M, 10, F, F, ws, q - 1, nullptr));
        SHORT(dvm_cycle_term_workspace_bytes(B, N, M, 10, 10), dvm_cycle_term_f32(F, I, F, I, B, N, M, 10, 10, F, F, F, ws, q - 1, nullptr));
        SHORT(dvm_distortion_term_workspace_bytes(B, N, M, 10), dvm_distortion_term_f32(F, I, F, F, B, N, M, 10, F, F, ws, q - 1, nullptr));
        SHORT(dvm_mesh_laplacian_workspace_bytes(B, N, 2 * N), dvm_mesh_laplacian_f32(F, I, B, N, 2 * N, I, I, F, F, F, I, ws, q - 1, nullptr));
        SHORT(dvm_knn_laplacian_workspace_bytes(B, N, 10, 0), dvm_knn_laplacian_f32(F, I, B, N, 10, 0, I, I, F, F, I, ws, q - 1, nullptr));
        SHORT(dvm_dirichlet_term_workspace_bytes(B, N, M, 10, 3, 20 * N),
              dvm_dirichlet_term_f32(F, I, F, I, I, F, B, N, M, 10, 3, 20 * N, F, F, ws, q - 1, nullptr));
        SHORT(dvm_pair_direction_workspace_bytes(B, N, M),
              dvm_pair_direction_fwd_f32(F, F, F, F, B, N, M, -1.f, I, F, F, F, F, F, F, F, F, F, F, 1, F, F, I, F, ws, q - 1, nullptr));
        SHORT(dvm_pair_workspace_bytes(B, N, M),
              dvm_pair_fwd_f32(F, F, F, F, B, N, M, -1.f, I, I, F, F, F, F, F, F, F, F, F, F, 1, F, F, I, F, F, F, I, F, ws, q - 1, nullptr));
        SHORT(dvm_pair_workspace_bytes(B, N, M),
              dvm_pair_fwd_cached_f32(F, F, F, F, B, N, M, -1.f, I, I, F, F, F, F, F, F, F, F, F, F, 1, F, F, I, F, F, F, I, F, ws, q - 1, 1, nullptr));
        SHORT(dvm_pair_workspace_bytes(B, N, M), dvm_pair_geometry_f32(F, F, B, N, M, I, I, 1, ws, q - 1, nullptr));
        SHORT(dvm_uni3fc_fwd_workspace_bytes(B, N, k), dvm_uni3fc_fwd_f32(F, F, B, N, ptab, DVM_U3_NWEIGHTS, k, F, F, ws, q - 1, nullptr));
        SHORT(dvm_uni3fc_train_workspace_bytes(B, N, k),
              dvm_uni3fc_train_fwd_f32(F, F, B, N, ptab, DVM_U3_TRAIN_NPARAMS, k, 1e-5f, 0.1f, 1, 0, nullptr, nullptr, F, F, ws, q - 1, nullptr));
        SHORT(dvm_uni3fc_train_workspace_bytes(B, N, k),
              dvm_uni3fc_train_fwd_sync_f32(F, F, B, N, ptab, DVM_U3_TRAIN_NPARAMS, k, 1e-5f, 0.1f, 1, 0, nullptr, nullptr, F, F, ws, q - 1, &coll, nullptr));
        SHORT(dvm_uni3fc_train_workspace_bytes(B, N, k),
              dvm_uni3fc_train_bwd_f32(F, F, F, F, F, B, N, ptab, gtab, DVM_U3_TRAIN_NPARAMS, k, 1, ws, q - 1, nullptr));
        SHORT(dvm_uni3fc_train_workspace_bytes(B, N, k),
              dvm_uni3fc_train_bwd_sync_f32(F, F, F, F, F, B, N, ptab, gtab, DVM_U3_TRAIN_NPARAMS, k, 1, ws, q - 1, &coll, nullptr));
        SHORT(dvm_uni3fc_train_workspace_bytes(B, N, k),
              dvm_uni3fc_train_running_stats_f32(ptab, DVM_U3_TRAIN_NPARAMS, B, N, k, 1, 0.1f, ws, q - 1, nullptr));
        SHORT(dvm_criterion_train_workspace_bytes(B, N, k, 10, 16, k),
              dvm_criterion_train_fwd_f32(F, F, I, I, I, F, I, B, N, d, k, 10, -1.f, ptab, DVM_CRIT_TRAIN_NPARAMS, 1, F, F, I, I, 16, k, F, ws, q - 1, nullptr));
        SHORT(dvm_criterion_train_workspace_bytes(B, N, k, 10, 16, k),
              dvm_criterion_train_bwd_f32(F, F, F, I, I, I, F, I, B, N, d, k, 10, -1.f, ptab, gtab, DVM_CRIT_TRAIN_NPARAMS, 1, I, I, 16, k, F, ws, q - 1, nullptr));
        SHORT(dvm_criterion_dir_train_workspace_bytes(B, N, M, k, 10),
              dvm_criterion_dir_train_fwd_f32(F, F, F, F, I, I, I, F, I, I, B, N, M, d, k, 10, -1.f, ptab, DVM_CRIT_TRAIN_NPARAMS, 1, F, ws, q - 1, nullptr));
        SHORT(dvm_criterion_dir_train_workspace_bytes(B, N, M, k, 10),
              dvm_criterion_dir_train_bwd_f32(F, F, F, F, F, I, I, I, F, I, I, B, N, M, d, k, 10, -1.f, ptab, gtab, DVM_CRIT_TRAIN_NPARAMS, 1, F, F, ws, q - 1,
                                              nullptr));
#undef SHORT
        // dvm_sa_attention_train_fwd_f32 needs no workspace at this size; where it needs one, a short one is an argument error
        EXPECT(dvm_sa_attention_train_fwd_workspace_bytes(B, N) == 0);
        q = dvm_sa_attention_train_fwd_workspace_bytes(1, 4995);
        EXPECT(q > 0 && dvm_sa_attention_train_fwd_f32(F, F, 1, 4995, F, F, F, ws, q / 2, nullptr) == DVM_EINVAL);
        EXPECT(strstr(dvm_last_error(), "workspace too small") != nullptr);
    }
    EXPECT(dvm_graph_geodesics_f64(nullptr, nullptr, 10, 4, nullptr, nullptr) == DVM_EINVAL);
    {
        // dvm_mesh_geodesics_f64: every refusal that comes before a launch
        double *Dd = (double *)0x1000;
        int32_t *Ii = (int32_t *)0x1000;
        const int vmax = dvm_mesh_geodesics_max_v();
        const size_t mb = dvm_mesh_geodesics_workspace_bytes(100, 162);
        EXPECT(mb >= 3 * 162 * 48 && dvm_mesh_geodesics_workspace_bytes(vmax, 4) > 0);
        EXPECT(dvm_mesh_geodesics_workspace_bytes(0, 4) == 0 && dvm_mesh_geodesics_workspace_bytes(8, -1) == 0 &&
               dvm_mesh_geodesics_workspace_bytes(vmax + 1, 4) == 0);
        EXPECT(dvm_mesh_geodesics_f64(nullptr, Ii, 100, 162, nullptr, 0, Dd, Dd, mb, nullptr) == DVM_EINVAL);
        EXPECT(dvm_mesh_geodesics_f64(Dd, Ii, vmax + 1, 162, nullptr, 0, Dd, Dd, (size_t)1 << 40, nullptr) == DVM_EINVAL);
        EXPECT(dvm_mesh_geodesics_f64(Dd, Ii, 100, 162, Ii, 0, Dd, Dd, mb, nullptr) == DVM_EINVAL);
        EXPECT(dvm_mesh_geodesics_f64(Dd, Ii, 100, 162, nullptr, 0, Dd, Dd, mb - 1, nullptr) == DVM_ENOSPACE);
        EXPECT(dvm_mesh_geodesics_f64(Dd, Ii, 100, 162, nullptr, 0, Dd, nullptr, 0, nullptr) == DVM_ENOSPACE);
    }
    {
        // dvm_eigenbasis_f64 / dvm_basis_project_f64: every limit exceeded by one, and the short workspace, before a launch
        double *Dd = (double *)0x1000;
        int32_t *Ii = (int32_t *)0x1000;
        float *Ff = (float *)0x1000;
        const int mmax = dvm_eigenbasis_max_block();
        const size_t eb = dvm_eigenbasis_workspace_bytes(2, 642, 3840, 30, 8);
        EXPECT(mmax == 128 && eb >= 2 * 3 * 642 * 38 * sizeof(double) && dvm_eigenbasis_workspace_bytes(1, 4096, 1, 100, mmax - 100) > 0);
        EXPECT(dvm_eigenbasis_workspace_bytes(0, 642, 3840, 30, 8) == 0 && dvm_eigenbasis_workspace_bytes(65536, 642, 3840, 30, 8) == 0 &&
               dvm_eigenbasis_workspace_bytes(2, (1 << 24) + 1, 3840, 30, 8) == 0 && dvm_eigenbasis_workspace_bytes(2, 642, 0, 30, 8) == 0 &&
               dvm_eigenbasis_workspace_bytes(2, 642, 3840, 0, 8) == 0 && dvm_eigenbasis_workspace_bytes(2, 642, 3840, 30, 0) == 0 &&
               dvm_eigenbasis_workspace_bytes(2, 642, 3840, 100, mmax - 99) == 0 && dvm_eigenbasis_workspace_bytes(2, 37, 3840, 30, 8) == 0 &&
               dvm_eigenbasis_workspace_bytes(2, 642, 3840, 2147483647, 8) == 0);
#define EIG(k, guard, degree, iters, tol, wsb) \
    dvm_eigenbasis_f64(Ii, Ii, Ff, Ff, 2, 642, 3840, k, guard, degree, iters, tol, Dd, Dd, Dd, Ii, Dd, wsb, nullptr)
        EXPECT(dvm_eigenbasis_f64(nullptr, Ii, Ff, nullptr, 2, 642, 3840, 30, 8, 20, 200, 1e-10, Dd, Dd, Dd, Ii, Dd, eb, nullptr) == DVM_EINVAL);
        EXPECT(EIG(0, 8, 20, 200, 1e-10, eb) == DVM_EINVAL && EIG(30, 0, 20, 200, 1e-10, eb) == DVM_EINVAL);
        EXPECT(EIG(121, 8, 20, 200, 1e-10, (size_t)1 << 40) == DVM_EINVAL);
        EXPECT(EIG(30, 8, 0, 200, 1e-10, eb) == DVM_EINVAL && EIG(30, 8, 257, 200, 1e-10, eb) == DVM_EINVAL);
        EXPECT(EIG(30, 8, 20, 0, 1e-10, eb) == DVM_EINVAL && EIG(30, 8, 20, 200, 0.0, eb) == DVM_EINVAL);
        EXPECT(EIG(30, 8, 20, 200, 1e-10, eb - 1) == DVM_ENOSPACE);
#undef EIG
        const size_t pb = dvm_basis_project_workspace_bytes(2, 642, 30, 128);
        EXPECT(pb >= 2 * 21 * 30 * 128 * sizeof(double) && dvm_basis_project_workspace_bytes(2, 642, 129, 3) == 0 &&
               dvm_basis_project_workspace_bytes(2, 642, 30, 129) == 0 && dvm_basis_project_workspace_bytes(2, 0, 30, 3) == 0);
        EXPECT(dvm_basis_project_f64(Dd, nullptr, Ff, 2, 642, 30, 129, Dd, Dd, pb, nullptr) == DVM_EINVAL);
        EXPECT(dvm_basis_project_f64(Dd, nullptr, nullptr, 2, 642, 30, 128, Dd, Dd, pb, nullptr) == DVM_EINVAL);
        EXPECT(dvm_basis_project_f64(Dd, nullptr, Ff, 2, 642, 30, 128, Dd, Dd, pb - 1, nullptr) == DVM_ENOSPACE);
        EXPECT(dvm_basis_project_f64(Dd, nullptr, Ff, 2, 642, 30, 128, Dd, nullptr, 0, nullptr) == DVM_ENOSPACE);
    }
    {
        // the ZoomOut entries (dvm_zoomout.hip): workspace carves at the largest sizes, every limit exceeded by one, null pointers
        // and the short workspace, before a launch
        double *Dd = (double *)0x1000;
        int32_t *Ii = (int32_t *)0x1000;
        float *Ff = (float *)0x1000;
        const size_t big = (size_t)1 << 40;
        const size_t fb0 = dvm_fmap_from_pmap_workspace_bytes(2, 642, 600, 30, 0), fb1 = dvm_fmap_from_pmap_workspace_bytes(2, 642, 600, 30, 1);
        const size_t nb = dvm_spectral_nn_workspace_bytes(2, 642, 600, 30), tb = dvm_fmap_to_pmap_workspace_bytes(2, 642, 600, 30);
        const size_t zb = dvm_zoomout_workspace_bytes(2, 642, 600, 6, 30, 2, 1, 1);
        EXPECT(fb0 >= 2 * 21 * 900 * sizeof(double) && fb1 >= fb0 + 2 * 900 * sizeof(double));
        EXPECT(nb >= 2 * 642 * 12 && tb >= nb + 2 * 600 * 30 * sizeof(double) && zb >= fb1 + tb + 2 * 900 * sizeof(double));
        EXPECT(dvm_zoomout_workspace_bytes(65535, 1 << 24, 1 << 24, 1, 128, 1, 1, 1) > dvm_zoomout_workspace_bytes(1, 1 << 24, 1 << 24, 1, 128, 1, 1, 1));
        int32_t plan[4] = {0, 0, 0, 0};
        EXPECT(dvm_spectral_nn_plan(1, 4096, 4096, 128, plan) == DVM_OK && plan[0] == 64 && plan[1] == 64 && plan[2] >= 1 &&
               plan[3] % plan[1] == 0 && (long long)plan[2] * plan[3] >= 4096 && (long long)(plan[2] - 1) * plan[3] < 4096);
        EXPECT(dvm_spectral_nn_plan(65535, 1 << 24, 1 << 24, 128, plan) == DVM_OK && plan[2] == 1 && plan[3] >= (1 << 24));
        EXPECT(dvm_spectral_nn_plan(1, 4096, 4096, 129, plan) == DVM_EINVAL && dvm_spectral_nn_plan(1, 4096, 4096, 30, nullptr) == DVM_EINVAL);
        EXPECT(dvm_fmap_from_pmap_workspace_bytes(0, 642, 600, 30, 0) == 0 && dvm_fmap_from_pmap_workspace_bytes(2, 642, 600, 129, 0) == 0 &&
               dvm_fmap_from_pmap_workspace_bytes(2, 642, 600, 30, 2) == 0 && dvm_fmap_from_pmap_workspace_bytes(2, (1 << 24) + 1, 600, 30, 0) == 0);
        EXPECT(dvm_spectral_nn_workspace_bytes(65536, 642, 600, 30) == 0 && dvm_spectral_nn_workspace_bytes(2, 0, 600, 30) == 0 &&
               dvm_spectral_nn_workspace_bytes(2, 642, (1 << 24) + 1, 30) == 0 && dvm_spectral_nn_workspace_bytes(2, 642, 600, 0) == 0);
        EXPECT(dvm_fmap_to_pmap_workspace_bytes(2, 642, 0, 30) == 0 && dvm_fmap_to_pmap_workspace_bytes(2, 642, 600, 129) == 0);
        EXPECT(dvm_zoomout_workspace_bytes(2, 642, 600, 0, 30, 2, 1, 0) == 0 && dvm_zoomout_workspace_bytes(2, 642, 600, 31, 30, 2, 1, 0) == 0 &&
               dvm_zoomout_workspace_bytes(2, 642, 600, 6, 129, 2, 1, 0) == 0 && dvm_zoomout_workspace_bytes(2, 642, 600, 6, 30, 0, 1, 0) == 0 &&
               dvm_zoomout_workspace_bytes(2, 642, 600, 6, 30, 2, 0, 0) == 0 && dvm_zoomout_workspace_bytes(2, 642, 600, 6, 30, 2, 1, 2) == 0);
#define FROM(ldx, ldy, k, mode, info, wsb) dvm_fmap_from_pmap_f64(Dd, ldx, Ff, Dd, ldy, Ii, 2, 642, 600, k, mode, Dd, info, Dd, wsb, nullptr)
        EXPECT(FROM(40, 40, 0, 0, Ii, big) == DVM_EINVAL && FROM(40, 40, 129, 0, Ii, big) == DVM_EINVAL && FROM(29, 40, 30, 0, Ii, big) == DVM_EINVAL);
        EXPECT(FROM(40, 29, 30, 0, Ii, big) == DVM_EINVAL && FROM(40, 40, 30, 2, Ii, big) == DVM_EINVAL && FROM(40, 40, 30, 1, nullptr, big) == DVM_EINVAL);
        EXPECT(FROM(40, 40, 30, 1, Ii, fb1 - 1) == DVM_ENOSPACE && FROM(40, 40, 30, 0, Ii, fb0 - 1) == DVM_ENOSPACE);
#undef FROM
        EXPECT(dvm_fmap_embed_f64(Dd, 40, Dd, 2, 600, 30, Dd, 29, nullptr) == DVM_EINVAL && dvm_fmap_embed_f64(Dd, 29, Dd, 2, 600, 30, Dd, 30, nullptr) == DVM_EINVAL);
        EXPECT(dvm_fmap_embed_f64(Dd, 40, nullptr, 2, 600, 30, Dd, 30, nullptr) == DVM_EINVAL && dvm_fmap_embed_f64(Dd, 40, Dd, 0, 600, 30, Dd, 30, nullptr) == DVM_EINVAL);
        EXPECT(dvm_spectral_nn_f64(Dd, 29, Dd, 40, 2, 642, 600, 30, Ii, nullptr, Dd, big, nullptr) == DVM_EINVAL);
        EXPECT(dvm_spectral_nn_f64(Dd, 40, Dd, 40, 2, 642, 600, 30, nullptr, nullptr, Dd, big, nullptr) == DVM_EINVAL);
        EXPECT(dvm_spectral_nn_f64(Dd, 40, Dd, 40, 2, 642, 600, 30, Ii, nullptr, Dd, nb - 1, nullptr) == DVM_ENOSPACE);
        EXPECT(dvm_spectral_nn_f64(Dd, 40, Dd, 40, 2, 642, 600, 30, Ii, nullptr, nullptr, 0, nullptr) == DVM_ENOSPACE);
        EXPECT(dvm_fmap_to_pmap_f64(Dd, 40, Dd, 40, nullptr, 2, 642, 600, 30, Ii, nullptr, nullptr, Dd, big, nullptr) == DVM_EINVAL);
        EXPECT(dvm_fmap_to_pmap_f64(Dd, 40, Dd, 29, Dd, 2, 642, 600, 30, Ii, nullptr, nullptr, Dd, big, nullptr) == DVM_EINVAL);
        EXPECT(dvm_fmap_to_pmap_f64(Dd, 40, Dd, 40, Dd, 2, 642, 600, 30, Ii, nullptr, nullptr, Dd, tb - 1, nullptr) == DVM_ENOSPACE);
#define ZOOM(ki, kf, ks, ni, mode, wsb) dvm_zoomout_f64(Dd, 40, Ff, Dd, 40, Ii, 2, 642, 600, ki, kf, ks, ni, mode, Dd, Ii, Ii, Dd, wsb, nullptr)
        EXPECT(ZOOM(0, 30, 2, 1, 1, big) == DVM_EINVAL && ZOOM(31, 30, 2, 1, 1, big) == DVM_EINVAL && ZOOM(6, 41, 2, 1, 1, big) == DVM_EINVAL);
        EXPECT(ZOOM(6, 30, 0, 1, 1, big) == DVM_EINVAL && ZOOM(6, 30, 2, 0, 1, big) == DVM_EINVAL && ZOOM(6, 30, 2, 1, -1, big) == DVM_EINVAL);
        EXPECT(dvm_zoomout_f64(Dd, 40, nullptr, Dd, 40, nullptr, 2, 642, 600, 6, 30, 2, 1, 1, Dd, Ii, Ii, Dd, big, nullptr) == DVM_EINVAL);
        EXPECT(ZOOM(6, 30, 2, 1, 1, zb - 1) == DVM_ENOSPACE && strstr(dvm_last_error(), "dvm_zoomout_f64") != nullptr);
#undef ZOOM
    }
    EXPECT(dvm_profile_read(nullptr, nullptr) == DVM_EINVAL);
    EXPECT(dvm_profile_enable(0) == DVM_EINVAL);
    // context registry: destroying with nothing registered, twice, is fine; set_overlap returns the previous value
    EXPECT(dvm_pair_destroy() == DVM_OK && dvm_pair_destroy() == DVM_OK);
    const int prev_ov = dvm_pair_set_overlap(0);
    EXPECT(dvm_pair_set_overlap(prev_ov) == 0);
    printf(fails ? "san_host: %d check(s) failed\n" : "san_host: ok\n", fails);
    return fails ? 1 : 0;
}
