// The library's one "out[0] = scale * sum of the partials" kernel (wm_reduce.h): the second launch of wm_recon_finalize, wm_ssim3_finalize,
// wm_advloss_finalize and wm_cw_margin.
#include "wm_reduce.h"

namespace {

__global__ __launch_bounds__(256) void sum_finalize_kernel(const double* __restrict__ partials, size_t n, double scale, float* __restrict__ out) {
    __shared__ double s[4];
    double a = 0.0;
    for (size_t i = threadIdx.x; i < n; i += 256) a += partials[i];
    a = block_sum_f64(a, s);
    if (threadIdx.x == 0) out[0] = (float)(a * scale);
}

}  // namespace

void wm_sum_finalize(const double* partials, size_t n, double scale, float* out, hipStream_t stream) {
    hipLaunchKernelGGL(sum_finalize_kernel, dim3(1), dim3(256), 0, stream, partials, n, scale, out);
}
