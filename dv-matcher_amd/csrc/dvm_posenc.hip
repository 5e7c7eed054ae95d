// dvm_posenc.hip — the positional sin/cos encoding of LG-Net.  Reference: models/model.py:544-561 (pos_encoding_sin_wave).
#include "dvm_common.h"

namespace dvm {

__global__ void minmax_partial_kernel(const float *__restrict__ x, long n, float *__restrict__ part) {
    __shared__ float smn[256], smx[256];
    float mn = INFINITY, mx = -INFINITY;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        float v = x[i];
        mn = fminf(mn, v);
        mx = fmaxf(mx, v);
    }
    smn[threadIdx.x] = mn;
    smx[threadIdx.x] = mx;
    __syncthreads();
    for (int o = blockDim.x / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            smn[threadIdx.x] = fminf(smn[threadIdx.x], smn[threadIdx.x + o]);
            smx[threadIdx.x] = fmaxf(smx[threadIdx.x], smx[threadIdx.x + o]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        part[2 * blockIdx.x] = smn[0];
        part[2 * blockIdx.x + 1] = smx[0];
    }
}

__global__ void minmax_final_kernel(const float *__restrict__ part, int nparts, float *__restrict__ out2) {
    float mn = INFINITY, mx = -INFINITY;
    for (int q = 0; q < nparts; ++q) mn = fminf(mn, part[2 * q]), mx = fmaxf(mx, part[2 * q + 1]);
    out2[0] = mn, out2[1] = mx;
}

// out[b, c*128 + j, n] = sin(nc * f_j), out[b, c*128 + 64 + j, n] = cos(nc * f_j);
// nc = 2*((x - mn)/(mx - mn)) - 1, f_j = fl32(pi) * 2^j.   x, out are (B,3,N) / (B,384,N).
__global__ void posenc_kernel(const float *__restrict__ x, const float *__restrict__ part, int nparts, int B, int N,
                              float *__restrict__ out) {
    float mn = INFINITY, mx = -INFINITY;
    for (int q = 0; q < nparts; ++q) {
        mn = fminf(mn, part[2 * q]);
        mx = fmaxf(mx, part[2 * q + 1]);
    }
    const long total = (long)B * 3 * 64 * N;
    const float range = mx - mn;
    for (long g = (long)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (long)gridDim.x * blockDim.x) {
        int n = (int)(g % N);
        int j = (int)((g / N) % 64);
        int c = (int)((g / ((long)N * 64)) % 3);
        int b = (int)(g / ((long)N * 64 * 3));
        float v = x[((size_t)b * 3 + c) * N + n];
        float t = __fdiv_rn(v - mn, range);
        float nc = 2.f * t - 1.f;
        float f = __uint_as_float(0x40490fdbu) * __uint_as_float((unsigned)(127 + j) << 23);  // fl32(pi) * 2^j, exact
        float kk = nc * f;
        size_t o = ((size_t)b * 384 + c * 128 + j) * N + n;
        out[o] = sinf(kk);
        out[o + (size_t)64 * N] = cosf(kk);
    }
}

static size_t carve_pos_encoding(Arena &ar, float *&part) {   // min / max partials of up to 256 workgroups
    part = ar.take<float>(2 * 256);
    return ar.off;
}

}  // namespace dvm

using namespace dvm;

DVM_EXPORT size_t dvm_pos_encoding_workspace_bytes(void) { return null_carve<float *>(carve_pos_encoding); }

DVM_EXPORT int dvm_pos_encoding_f32(const float *x, int B, int N, float *out, void *ws, size_t ws_bytes, void *stream) {
    DVM_REQUIRE(x && out && B >= 1 && N >= 1, "dvm_pos_encoding_f32: bad arguments");
    float *part;
    if (!carve_ws(ws, ws_bytes, "dvm_pos_encoding_f32", part, carve_pos_encoding)) return DVM_ENOSPACE;
    hipStream_t s = (hipStream_t)stream;
    long n = (long)B * 3 * N;
    int nparts = (int)((n + 255) / 256 < 256 ? (n + 255) / 256 : 256);
    hipLaunchKernelGGL(minmax_partial_kernel, dim3(nparts), dim3(256), 0, s, x, n, part);
    long total = (long)B * 3 * 64 * N;
    int blocks = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
    hipLaunchKernelGGL(posenc_kernel, dim3(blocks), dim3(256), 0, s, x, part, nparts, B, N, out);
    DVM_CHECK_LAUNCH("pos_encoding");
    return DVM_OK;
}

// The same encoding with the range taken over ALL ranks' tensors (models/model.py:548 normalises with the min / max of the whole
// batch: under data parallelism that is the global batch): this rank's min / max go to minmax2 (two floats of caller-owned device
// memory), the caller's collective combines them (MIN on the first, MAX on the second, enqueued on `stream`), then the encoding.
DVM_EXPORT int dvm_pos_encoding_sync_f32(const float *x, int B, int N, float *out, void *ws, size_t ws_bytes, const dvm_collective *coll,
                                         float *minmax2, void *stream) {
    DVM_REQUIRE(x && out && B >= 1 && N >= 1 && coll && coll->allreduce && minmax2, "dvm_pos_encoding_sync_f32: bad arguments");
    float *part;
    if (!carve_ws(ws, ws_bytes, "dvm_pos_encoding_sync_f32", part, carve_pos_encoding)) return DVM_ENOSPACE;
    hipStream_t s = (hipStream_t)stream;
    long n = (long)B * 3 * N;
    int nparts = (int)((n + 255) / 256 < 256 ? (n + 255) / 256 : 256);
    hipLaunchKernelGGL(minmax_partial_kernel, dim3(nparts), dim3(256), 0, s, x, n, part);
    hipLaunchKernelGGL(minmax_final_kernel, dim3(1), dim3(1), 0, s, part, nparts, minmax2);
    int rc = coll->allreduce(coll->user, minmax2, 1, 0, 1, stream);
    if (rc == 0) rc = coll->allreduce(coll->user, minmax2 + 1, 1, 0, 2, stream);
    DVM_REQUIRE(rc == 0, "dvm_pos_encoding_sync_f32: the caller's all-reduce failed (%d)", rc);
    return dvm_pos_encoding_minmax_f32(x, minmax2, B, N, out, stream);
}

DVM_EXPORT int dvm_pos_encoding_minmax_f32(const float *x, const float *minmax, int B, int N, float *out, void *stream) {
    DVM_REQUIRE(x && minmax && out && B >= 1 && N >= 1, "dvm_pos_encoding_minmax_f32: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    long total = (long)B * 3 * 64 * N;
    int blocks = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
    hipLaunchKernelGGL(posenc_kernel, dim3(blocks), dim3(256), 0, s, x, minmax, 1, B, N, out);
    DVM_CHECK_LAUNCH("pos_encoding_minmax");
    return DVM_OK;
}
