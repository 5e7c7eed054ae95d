// dvm_frob.hip — the last step of every sparse Frobenius-norm term (dvm_frob.h): F^2 -> the loss and the gradients' scale.
#include "dvm_frob.h"

namespace dvm {

// f2 [B] = F^2 -> loss [B] = F; g_val [B][E] *= num / F, 0 where F == 0 (num = 1/2: g_val = dF^2 / d pi_val -> dF / d pi_val)
__global__ void frob_finish_kernel(const float *__restrict__ f2, size_t E, double num, float *__restrict__ loss, float *__restrict__ g_val) {
    const int b = blockIdx.y;
    const double F = sqrt((double)f2[b]);
    if (blockIdx.x == 0 && threadIdx.x == 0) loss[b] = (float)F;
    if (g_val == nullptr) return;
    const double sc = F > 0.0 ? num / F : 0.0;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < E; e += (size_t)gridDim.x * blockDim.x)
        g_val[(size_t)b * E + e] = (float)((double)g_val[(size_t)b * E + e] * sc);
}

static void launch_frob_finish(const float *f2, int B, size_t E, double num, float *loss, float *g_val, hipStream_t s) {
    const unsigned fblocks = g_val ? (unsigned)((E + 1023) / 1024) : 1u;
    hipLaunchKernelGGL(frob_finish_kernel, dim3(fblocks, B), dim3(256), 0, s, f2, E, num, loss, g_val);
}

int frob_finish(const FrobSums &w, int B, int N, double num, float *loss, std::initializer_list<FrobGrad> grads, const char *name, hipStream_t s) {
    launch_reduce_partials(w.partial, B, N, 1.f, w.f2, 1, 0, s);
    for (const FrobGrad *g = grads.begin(); g != grads.end(); ++g)
        if (g == grads.begin() || g->g) launch_frob_finish(w.f2, B, g->E, num, loss, g->g, s);
    DVM_CHECK_LAUNCH(name);
    return DVM_OK;
}

}  // namespace dvm
