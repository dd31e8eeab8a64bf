// Image-quality and mask metrics on the device (pytorch_ssim/__init__.py:7-40, metrics.py:5-46, calculate_f1.py:5-41 of the reference):
//   pytorch_ssim._ssim     wm_ssim_fwd (+ wm_ssim_finalize)   11-tap Gaussian window (sigma 1.5), zero padding 5, C1 = 0.01^2, C2 = 0.03^2
//   its autograd backward  wm_ssim_bwd                        wrt the first image; the second by swapping the arguments (S is symmetric)
//   metrics.PSNR(max_val)  wm_psnr_partials + wm_psnr_finalize
//   getLabels / EdgeAccuracy's sums   wm_confusion_counts     exact integer TN, TP, FN, FP per image and in total
// f32 NCHW planes.  No atomics anywhere: every kernel writes per-workgroup partials that a finalise launch sums in a fixed order, so every
// result is bitwise reproducible.
//
// SSIM forward, one launch: a workgroup owns a 64 x 16 tile of one plane.  It stages both images' (16+10) x 80 window (the 5-pixel halo,
// widened to whole float4s: columns tx0-8 .. tx0+71) in LDS, runs the horizontal 11-tap pass for x, y, x^2, y^2, xy into LDS (26 x 64 x 5),
// then each thread runs the vertical pass for 4 rows of one column from LDS, forms the SSIM value in registers and adds it to a double.
// The map is never written.  With dplanes != NULL the thread also writes dS/dp, dS/dq, dS/dr (p = w*x, q = w*x^2, r = w*xy): the three
// planes the backward convolves.  LDS: 2*26*80*4 + 5*26*64*4 = 49,920 B static -> 3 workgroups per CU.
//
// SSIM backward, one launch: the same tile; stages the three derivative planes with their halo (zero outside the image: the adjoint of a
// zero-padded convolution with a symmetric window is the same convolution), horizontal then vertical pass, and
//   grad = g * (w*Dp + 2x . w*Dq + y . w*Dr)
// with g the upstream weight of the pixel's image (constant per image, so it multiplies after the convolution).  44,928 B of LDS.
//
// The float32 arithmetic, operation by operation (what tests/ssim_exact.py counts its roundings from; a compiler may contract a product
// and the sum after it into one fma, which only removes a rounding):
//   window sums   x^2, y^2, xy: one product each, before the window.  A window sum is 11 fmas along the row (taps in ascending order, from
//                 0) and 11 fmas down the column over those row sums: 22 roundings, the same chain for every pixel wherever its tile lies.
//   S             pm = p m, pp = p p, mm = m m; s1 = q - pp, s2 = q2 - mm, s12 = r - pm; A1 = 2 pm + C1, A2 = 2 s12 + C2 (times 2 is exact;
//                 C1, C2 the float32 of 0.01^2, 0.03^2); B1 = (pp + mm) + C1, B2 = (s1 + s2) + C2; S = (A1 A2) / (B1 B2).
//   planes        inv = 1 / (B1 B2), i1 = 1 / B1, i2 = 1 / B2 (three correctly rounded reciprocals);
//                 dS/dp = ((2 m) (A2 - A1)) inv - ((2 p) S) (i1 - i2);  dS/dq = -(S i2);  dS/dr = (2 A1) inv.
//   values        S is added to a double per thread; workgroup partials and the finalise stay in double; one division by the count and one
//                 rounding to float32 per value.
//   gradient      each plane's window sum as above (22); g = float32(gscale / (C H W [B])) formed in double on the host, then times
//                 gscale_dev[0], then times gout[b] (one rounding each that is present);
//                 v = g ((a0 + (2 x) a1) + y a2); accumulate: grad + v.
//   PSNR          d = a - b in float32; d d and every sum in double; mse = float32(sum / n);
//                 (20 logf(max_val)) / logf(10) - (10 logf(mse)) / logf(10).
#include "wm_common.h"
#include "wm_reduce.h"

namespace {

constexpr int TW = 64, TH = 16, R = 5, NT = 11;
constexpr int SH = TH + 2 * R;   // staged rows
constexpr int SW = TW + 16;      // staged columns tx0-8 .. tx0+71 (20 float4 per row); tap k of output column c reads column c + 3 + k
constexpr int SV = SW / 4;

struct Win11 { float w[NT]; };

// rows ty0-5 .. ty0+20, columns tx0-8 .. tx0+71 of plane p -> s (zero outside the image)
__device__ __forceinline__ void stage_plane(const float* __restrict__ p, int H, int W, int tx0, int ty0, bool vec, float (*s)[SW]) {
    if (vec) {   // W % 4 == 0 and a 16-byte aligned base: every float4 lies wholly inside or wholly outside the image
        for (int i = threadIdx.x; i < SH * SV; i += 256) {
            const int r = i / SV, c4 = i - r * SV;
            const int gy = ty0 - R + r, gx = tx0 - 8 + c4 * 4;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (gy >= 0 && gy < H && gx >= 0 && gx < W) v = *reinterpret_cast<const float4*>(p + (size_t)gy * W + gx);
            *reinterpret_cast<float4*>(&s[r][c4 * 4]) = v;
        }
    } else {
        for (int i = threadIdx.x; i < SH * SW; i += 256) {
            const int r = i / SW, c = i - r * SW;
            const int gy = ty0 - R + r, gx = tx0 - 8 + c;
            s[r][c] = (gy >= 0 && gy < H && gx >= 0 && gx < W) ? p[(size_t)gy * W + gx] : 0.f;
        }
    }
}

// vertical pass of NQ quantities for rows r0 .. r0+3 of column c: acc[o][q] = sum_k w[k] * h[q][r0 + o + k][c]
template <int NQ>
__device__ __forceinline__ void vpass4(const float (*h)[SH][TW], const Win11& win, int r0, int c, float (&acc)[4][NQ]) {
#pragma unroll
    for (int o = 0; o < 4; ++o)
#pragma unroll
        for (int q = 0; q < NQ; ++q) acc[o][q] = 0.f;
#pragma unroll
    for (int j = 0; j < NT + 3; ++j) {
        float v[NQ];
#pragma unroll
        for (int q = 0; q < NQ; ++q) v[q] = h[q][r0 + j][c];
#pragma unroll
        for (int o = 0; o < 4; ++o) {
            const int k = j - o;
            if (k >= 0 && k < NT) {
#pragma unroll
                for (int q = 0; q < NQ; ++q) acc[o][q] = __builtin_fmaf(win.w[k], v[q], acc[o][q]);
            }
        }
    }
}

__global__ __launch_bounds__(256) void ssim_fwd_kernel(const float* __restrict__ x, const float* __restrict__ y, int H, int W, Win11 win, int vec,
                                                       double* __restrict__ partials, float* __restrict__ dplanes, size_t plane_stride) {
    __shared__ __attribute__((aligned(16))) float sx[SH][SW];
    __shared__ __attribute__((aligned(16))) float sy[SH][SW];
    __shared__ float h[5][SH][TW];
    __shared__ double red[4];
    const int n = blockIdx.z, tx0 = blockIdx.x * TW, ty0 = blockIdx.y * TH;
    const size_t base = (size_t)n * H * W;
    stage_plane(x + base, H, W, tx0, ty0, vec != 0, sx);
    stage_plane(y + base, H, W, tx0, ty0, vec != 0, sy);
    __syncthreads();
    for (int i = threadIdx.x; i < SH * TW; i += 256) {
        const int r = i >> 6, c = i & 63;
        float p = 0.f, m = 0.f, q = 0.f, q2 = 0.f, rr = 0.f;
#pragma unroll
        for (int k = 0; k < NT; ++k) {
            const float a = sx[r][c + 3 + k], b = sy[r][c + 3 + k], wk = win.w[k];
            p = __builtin_fmaf(wk, a, p);
            m = __builtin_fmaf(wk, b, m);
            q = __builtin_fmaf(wk, a * a, q);
            q2 = __builtin_fmaf(wk, b * b, q2);
            rr = __builtin_fmaf(wk, a * b, rr);
        }
        h[0][r][c] = p; h[1][r][c] = m; h[2][r][c] = q; h[3][r][c] = q2; h[4][r][c] = rr;
    }
    __syncthreads();
    const int c = threadIdx.x & 63, r0 = (threadIdx.x >> 6) * 4;
    float acc[4][5];
    vpass4<5>(h, win, r0, c, acc);
    const float C1 = (float)(0.01 * 0.01), C2 = (float)(0.03 * 0.03);
    double sum = 0.0;
    const int gx = tx0 + c;
#pragma unroll
    for (int o = 0; o < 4; ++o) {
        const int gy = ty0 + r0 + o;
        if (gx < W && gy < H) {
            const float p = acc[o][0], m = acc[o][1];
            const float pm = p * m, pp = p * p, mm = m * m;
            const float s1 = acc[o][2] - pp, s2 = acc[o][3] - mm, s12 = acc[o][4] - pm;
            const float A1 = 2.f * pm + C1, A2 = 2.f * s12 + C2, B1 = pp + mm + C1, B2 = s1 + s2 + C2;
            const float S = (A1 * A2) / (B1 * B2);
            sum += (double)S;
            if (dplanes) {
                const float inv = 1.f / (B1 * B2), i1 = 1.f / B1, i2 = 1.f / B2;
                const size_t idx = base + (size_t)gy * W + gx;
                dplanes[idx] = 2.f * m * (A2 - A1) * inv - 2.f * p * S * (i1 - i2);
                dplanes[plane_stride + idx] = -S * i2;
                dplanes[2 * plane_stride + idx] = 2.f * A1 * inv;
            }
        }
    }
    sum = block_sum_f64(sum, red);
    if (threadIdx.x == 0) partials[((size_t)n * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = sum;
}

// block b < B: out[1 + b] = mean of image b (its per_image partials are contiguous); block B: out[0] = mean of everything
__global__ __launch_bounds__(256) void ssim_finalize_kernel(const double* __restrict__ partials, int B, int per_image, double count, float* __restrict__ out) {
    __shared__ double s[256];
    const int b = blockIdx.x;
    const size_t lo = b < B ? (size_t)b * per_image : 0, n = b < B ? (size_t)per_image : (size_t)B * per_image;
    double a = 0.0;
    for (size_t i = threadIdx.x; i < n; i += 256) a += partials[lo + i];
    s[threadIdx.x] = a;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) s[threadIdx.x] += s[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[b < B ? 1 + b : 0] = (float)(s[0] / (b < B ? count : count * (double)B));
}

__global__ __launch_bounds__(256) void ssim_bwd_kernel(const float* __restrict__ dplanes, size_t plane_stride, const float* __restrict__ x,
                                                       const float* __restrict__ y, float* __restrict__ grad, int C, int H, int W, Win11 win, int vec,
                                                       const float* __restrict__ gout, int per_image, float gscale,
                                                       const float* __restrict__ gscale_dev, int accumulate) {
    __shared__ __attribute__((aligned(16))) float sd[3][SH][SW];
    __shared__ float h[3][SH][TW];
    const int n = blockIdx.z, tx0 = blockIdx.x * TW, ty0 = blockIdx.y * TH;
    const size_t base = (size_t)n * H * W;
#pragma unroll
    for (int q = 0; q < 3; ++q) stage_plane(dplanes + q * plane_stride + base, H, W, tx0, ty0, vec != 0, sd[q]);
    __syncthreads();
    for (int i = threadIdx.x; i < SH * TW; i += 256) {
        const int r = i >> 6, c = i & 63;
        float a0 = 0.f, a1 = 0.f, a2 = 0.f;
#pragma unroll
        for (int k = 0; k < NT; ++k) {
            const float wk = win.w[k];
            a0 = __builtin_fmaf(wk, sd[0][r][c + 3 + k], a0);
            a1 = __builtin_fmaf(wk, sd[1][r][c + 3 + k], a1);
            a2 = __builtin_fmaf(wk, sd[2][r][c + 3 + k], a2);
        }
        h[0][r][c] = a0; h[1][r][c] = a1; h[2][r][c] = a2;
    }
    __syncthreads();
    const int c = threadIdx.x & 63, r0 = (threadIdx.x >> 6) * 4;
    float acc[4][3];
    vpass4<3>(h, win, r0, c, acc);
    float g = gscale;
    if (gscale_dev) g *= gscale_dev[0];
    if (gout) g *= gout[per_image ? n / C : 0];
    const int gx = tx0 + c;
#pragma unroll
    for (int o = 0; o < 4; ++o) {
        const int gy = ty0 + r0 + o;
        if (gx < W && gy < H) {
            const size_t idx = base + (size_t)gy * W + gx;
            const float v = g * (acc[o][0] + 2.f * x[idx] * acc[o][1] + y[idx] * acc[o][2]);
            grad[idx] = accumulate ? grad[idx] + v : v;
        }
    }
}

// sum of (a - b)^2, the difference in f32 (a.float() - b.float()), squared and summed in double
__global__ __launch_bounds__(256) void psnr_kernel(const float* __restrict__ a, const float* __restrict__ b, size_t n, double* __restrict__ partials) {
    double acc = 0.0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const double d = (double)(a[i] - b[i]);
        acc += d * d;
    }
    __shared__ double s[256];
    s[threadIdx.x] = acc;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) s[threadIdx.x] += s[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) partials[blockIdx.x] = s[0];
}

// metrics.py:30-46: 20 log(max_val) / log(10) - 10 log(mse) / log(10) in f32; 0 when the images are equal
__global__ void psnr_finalize_kernel(const double* __restrict__ partials, int nparts, double n, float max_val, float* __restrict__ out) {
    __shared__ double s[256];
    double a = 0.0;
    for (int i = threadIdx.x; i < nparts; i += 256) a += partials[i];
    s[threadIdx.x] = a;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) s[threadIdx.x] += s[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float mse = (float)(s[0] / n);
        const float base10 = logf(10.0f);
        out[0] = mse == 0.f ? 0.f : 20.f * logf(max_val) / base10 - 10.f * logf(mse) / base10;
    }
}

template <typename T> __device__ __forceinline__ bool above(const T* p, size_t i, float thr) { return (float)p[i] > thr; }

// grid (P, B): block (j, b) counts its grid-stride share of image b -> partials[(b*P + j)*4 + {TN, TP, FN, FP}]
template <typename TP_, typename TG_>
__global__ __launch_bounds__(256) void confusion_kernel(const TP_* __restrict__ pred, const TG_* __restrict__ gt, size_t per_image, float thr_pred,
                                                        float thr_gt, long long* __restrict__ partials) {
    const size_t base = (size_t)blockIdx.y * per_image;
    int cnt[4] = {0, 0, 0, 0};
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < per_image; i += (size_t)gridDim.x * 256) {
        const bool p = above(pred, base + i, thr_pred), g = above(gt, base + i, thr_gt);
        cnt[0] += (!p && !g); cnt[1] += (p && g); cnt[2] += (!p && g); cnt[3] += (p && !g);
    }
    __shared__ int s[4][4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) cnt[k] += __shfl_xor(cnt[k], o, 64);
    }
    if ((threadIdx.x & 63) == 0)
        for (int k = 0; k < 4; ++k) s[threadIdx.x >> 6][k] = cnt[k];
    __syncthreads();
    if (threadIdx.x < 4)
        partials[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 4 + threadIdx.x] =
            (long long)s[0][threadIdx.x] + s[1][threadIdx.x] + s[2][threadIdx.x] + s[3][threadIdx.x];
}

// block b < B: out[4*(1+b) + k] = counts of image b; block B: out[k] = totals
__global__ __launch_bounds__(256) void confusion_finalize_kernel(const long long* __restrict__ partials, int B, int P, long long* __restrict__ out) {
    __shared__ long long s[64][4];
    const int b = blockIdx.x, k = threadIdx.x & 3, t = threadIdx.x >> 2;
    const size_t lo = b < B ? (size_t)b * P : 0, n = b < B ? (size_t)P : (size_t)B * P;
    long long a = 0;
    for (size_t i = t; i < n; i += 64) a += partials[(lo + i) * 4 + k];
    s[t][k] = a;
    __syncthreads();
    if (threadIdx.x < 4) {
        long long tot = 0;
        for (int i = 0; i < 64; ++i) tot += s[i][threadIdx.x];
        out[(b < B ? 4 * (1 + b) : 0) + threadIdx.x] = tot;
    }
}

inline bool vec_ok(const void* a, const void* b, int W) {
    return W % 4 == 0 && (((uintptr_t)a | (uintptr_t)b) & 15) == 0;
}
inline int conf_parts(size_t per_image) {
    const size_t g = (per_image + 4095) / 4096;
    return (int)(g > 64 ? 64 : (g < 1 ? 1 : g));
}

}  // namespace

extern "C" int wm_ssim_nparts(int C, int H, int W) {
    if (C <= 0 || H <= 0 || W <= 0) return 0;
    return C * wm_cdiv(H, TH) * wm_cdiv(W, TW);
}

extern "C" int wm_ssim_fwd(const float* x, const float* y, int B, int C, int H, int W, const float* win11, double* partials, float* dplanes,
                           void* stream) {
    WM_REQUIRE(x && y && win11 && partials && B > 0 && C > 0 && H > 0 && W > 0 && (long)B * C <= 65535 && wm_cdiv(H, TH) <= 65535,
               WM_E_BADARG, "wm_ssim_fwd: bad arguments (B*C <= 65535, H <= 16*65535)");
    Win11 win;
    for (int k = 0; k < NT; ++k) win.w[k] = win11[k];
    const size_t plane_stride = (size_t)B * C * H * W;
    const int vec = vec_ok(x, y, W) ? 1 : 0;
    hipLaunchKernelGGL(ssim_fwd_kernel, dim3(wm_cdiv(W, TW), wm_cdiv(H, TH), B * C), dim3(256), 0, (hipStream_t)stream, x, y, H, W, win, vec, partials,
                       dplanes, plane_stride);
    WM_LAUNCH_CHECK("wm_ssim_fwd");
    return WM_OK;
}

extern "C" int wm_ssim_finalize(const double* partials, int B, int C, int H, int W, float* out, void* stream) {
    WM_REQUIRE(partials && out && B > 0 && C > 0 && H > 0 && W > 0, WM_E_BADARG, "wm_ssim_finalize: bad arguments");
    hipLaunchKernelGGL(ssim_finalize_kernel, dim3(B + 1), dim3(256), 0, (hipStream_t)stream, partials, B, wm_ssim_nparts(C, H, W),
                       (double)C * H * W, out);
    WM_LAUNCH_CHECK("wm_ssim_finalize");
    return WM_OK;
}

extern "C" int wm_ssim_bwd(const float* dplanes, const float* x, const float* y, float* grad, int B, int C, int H, int W, const float* win11,
                           const float* gout_dev, int per_image, float gscale, const float* gscale_dev, int accumulate, void* stream) {
    WM_REQUIRE(dplanes && x && y && grad && win11 && B > 0 && C > 0 && H > 0 && W > 0 && (long)B * C <= 65535 && wm_cdiv(H, TH) <= 65535,
               WM_E_BADARG, "wm_ssim_bwd: bad arguments (B*C <= 65535, H <= 16*65535)");
    Win11 win;
    for (int k = 0; k < NT; ++k) win.w[k] = win11[k];
    const size_t plane_stride = (size_t)B * C * H * W;
    const int vec = vec_ok(dplanes, dplanes, W) && plane_stride % 4 == 0 ? 1 : 0;
    // the mean's weight of a pixel: 1 / (B C H W), or 1 / (C H W) of its image's own mean
    const float g = (float)((double)gscale / ((double)C * H * W * (per_image ? 1.0 : (double)B)));
    hipLaunchKernelGGL(ssim_bwd_kernel, dim3(wm_cdiv(W, TW), wm_cdiv(H, TH), B * C), dim3(256), 0, (hipStream_t)stream, dplanes, plane_stride, x, y, grad,
                       C, H, W, win, vec, gout_dev, per_image, g, gscale_dev, accumulate);
    WM_LAUNCH_CHECK("wm_ssim_bwd");
    return WM_OK;
}

extern "C" int wm_psnr_partials(const float* a, const float* b, size_t n, double* partials, int nparts, void* stream) {
    WM_REQUIRE(a && b && partials && n > 0 && nparts > 0 && nparts <= 2048, WM_E_BADARG, "wm_psnr_partials: bad arguments");
    hipLaunchKernelGGL(psnr_kernel, dim3(nparts), dim3(256), 0, (hipStream_t)stream, a, b, n, partials);
    WM_LAUNCH_CHECK("wm_psnr_partials");
    return WM_OK;
}

extern "C" int wm_psnr_finalize(const double* partials, int nparts, double n, float max_val, float* out, void* stream) {
    WM_REQUIRE(partials && out && nparts > 0 && n > 0 && max_val > 0.f, WM_E_BADARG, "wm_psnr_finalize: bad arguments");
    hipLaunchKernelGGL(psnr_finalize_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, partials, nparts, n, max_val, out);
    WM_LAUNCH_CHECK("wm_psnr_finalize");
    return WM_OK;
}

extern "C" int wm_confusion_nparts(size_t per_image) { return per_image > 0 ? conf_parts(per_image) : 0; }

extern "C" int wm_confusion_counts(const void* pred, int pred_u8, const void* gt, int gt_u8, float thr_pred, float thr_gt, int B, size_t per_image,
                                   long long* partials, long long* out, void* stream) {
    WM_REQUIRE(pred && gt && partials && out && B > 0 && B <= 65535 && per_image > 0, WM_E_BADARG, "wm_confusion_counts: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    const int P = conf_parts(per_image);
    const dim3 grid(P, B);
    if (pred_u8 && gt_u8)
        hipLaunchKernelGGL((confusion_kernel<uint8_t, uint8_t>), grid, dim3(256), 0, s, (const uint8_t*)pred, (const uint8_t*)gt, per_image, thr_pred, thr_gt, partials);
    else if (pred_u8)
        hipLaunchKernelGGL((confusion_kernel<uint8_t, float>), grid, dim3(256), 0, s, (const uint8_t*)pred, (const float*)gt, per_image, thr_pred, thr_gt, partials);
    else if (gt_u8)
        hipLaunchKernelGGL((confusion_kernel<float, uint8_t>), grid, dim3(256), 0, s, (const float*)pred, (const uint8_t*)gt, per_image, thr_pred, thr_gt, partials);
    else
        hipLaunchKernelGGL((confusion_kernel<float, float>), grid, dim3(256), 0, s, (const float*)pred, (const float*)gt, per_image, thr_pred, thr_gt, partials);
    hipLaunchKernelGGL(confusion_finalize_kernel, dim3(B + 1), dim3(256), 0, s, partials, B, P, out);
    WM_LAUNCH_CHECK("wm_confusion_counts");
    return WM_OK;
}
