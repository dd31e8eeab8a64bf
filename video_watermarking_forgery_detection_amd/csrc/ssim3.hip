// The reference's local structure loss and its mask / gray losses (loss.py:9-39 = models/modules/loss.py:44-74 SSIM_Loss, loss.py:363-376
// ExtendedL1Loss, :379-388 NonBlurryLoss, :403-410 GrayLoss), each with its autograd backward:
//   SSIM_Loss        wm_ssim3_fwd (the map, and / or the partial sums of its mean) + wm_ssim3_finalize, wm_ssim3_bwd
//       both images padded by 1 with reflection (index -1 -> 1, H -> H-2), nine-tap means mu_x, mu_y, E[x^2], E[y^2], E[xy] (sum / 9),
//       n = (2 mu_x mu_y + C1)(2 sigma_xy + C2), d = (mu_x^2 + mu_y^2 + C1)(sigma_x + sigma_y + C2), out = clamp((1 - n/d) / 2, 0, 1)
//   ExtendedL1Loss   mean |m a - m b| / mean |m|       NonBlurryLoss  1 - mean (x - 1/2)^2       GrayLoss  1 / mean |x - 1/2|
//       wm_pixloss_sums / _finalize / _bwd
// f32 NCHW planes.  No atomics and no host synchronisation: per-workgroup partial sums in double, a one-workgroup finalise that adds them in
// a fixed order.  Every result is bitwise reproducible and independent of how the grid is scheduled.
//
// SSIM_Loss forward, one launch: a workgroup owns a 16 x 64 tile of one plane and stages both images' tile with a one-pixel halo in LDS,
// the reflection applied while staging (2 x 18 x 66 x 4 = 9,504 B).  A thread forms four rows of one column: the nine taps are added row by
// row in f32 and divided by 9, the reference's order (AvgPool2d), then the value.  8 B read and 4 B written per element; the halo comes from L2.
//
// Backward, one launch, gather form: the tile's images with a halo of 2 (2 x 20 x 68 x 4 B), then the per-output coefficients
// g * d out / d{mu_x, mu_y, E[x^2] (= the one of E[y^2]), E[xy]} of the tile plus a halo of 1 (4 x 18 x 66 x 4 B; zero outside the image
// and where the clamp cuts).  Input pixel i then adds the coefficients of the outputs p in [i-1, i+1]^2 inside the image, each times the
// number of taps of p's window that the reflection maps to i: per axis 1, +1 for p = i-1 when i = 1 (tap -1), +1 for p = i+1 when i = H-2
// (tap H).  At H = 2 both hold.  The same arithmetic serves the map's backward (g a tensor) and the mean's (g one weight): where the
// tensor holds that weight the two gradients are bit-identical.
#include "wm_common.h"

#pragma clang fp contract(off)   // x = y must give n == d bit for bit: the two sides are the same operations only while none is fused
#include "wm_reduce.h"          // (below the pragma: it holds for the shared helpers as well)

namespace {

constexpr int TW = 64, TH = 16;

// ------------------------------------------------------------------------------------------------ SSIM_Loss
// ReflectionPad2d(1): padded index -1 -> 1, n -> n - 2 (n >= 2); only called for -1 <= i <= n
__device__ __forceinline__ int refl(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }

// rows ty0-HB .. ty0+TH+HB-1, columns tx0-HB .. tx0+TW+HB-1 of the PADDED plane -> s; 0 beyond the one-pixel pad (never read by a pixel of
// the image)
template <int HB>
__device__ __forceinline__ void stage_refl(const float* __restrict__ p, int H, int W, int tx0, int ty0, float (*s)[TW + 2 * HB]) {
    constexpr int SW = TW + 2 * HB, SH = TH + 2 * HB;
    for (int i = threadIdx.x; i < SH * SW; i += 256) {
        const int r = i / SW, c = i - r * SW;
        const int py = ty0 - HB + r, px = tx0 - HB + c;
        float v = 0.f;
        if (py >= -1 && py <= H && px >= -1 && px <= W) v = p[(size_t)refl(py, H) * W + refl(px, W)];
        s[r][c] = v;
    }
}

struct Stats { float mx, my, ex2, ey2, exy; };

// the five nine-tap means of the window whose top-left tap is s[r][c]: added row by row, then / 9
template <int SW>
__device__ __forceinline__ Stats stats9(const float (*sx)[SW], const float (*sy)[SW], int r, int c) {
    float a = 0.f, b = 0.f, aa = 0.f, bb = 0.f, ab = 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const float u = sx[r + i][c + j], v = sy[r + i][c + j];
            a += u; b += v; aa += u * u; bb += v * v; ab += u * v;
        }
    return {a / 9.f, b / 9.f, aa / 9.f, bb / 9.f, ab / 9.f};
}

struct Terms { float A1, A2, B1, B2; };
__device__ __forceinline__ Terms ssim3_terms(const Stats& s) {
    const float C1 = (float)(0.01 * 0.01), C2 = (float)(0.03 * 0.03);
    const float mxy = s.mx * s.my, mxx = s.mx * s.mx, myy = s.my * s.my;
    const float sgx = s.ex2 - mxx, sgy = s.ey2 - myy, sgxy = s.exy - mxy;
    return {2.f * mxy + C1, 2.f * sgxy + C2, mxx + myy + C1, sgx + sgy + C2};
}
// the unclamped value (1 - n/d) / 2
__device__ __forceinline__ float ssim3_value(const Terms& t) { return (1.f - (t.A1 * t.A2) / (t.B1 * t.B2)) / 2.f; }

// grid (tiles_x, tiles_y, N): out (may be NULL) = the map; partials (may be NULL) [(n * tiles_y + ty) * tiles_x + tx] = the tile's sum
__global__ __launch_bounds__(256) void ssim3_fwd_kernel(const float* __restrict__ x, const float* __restrict__ y, float* __restrict__ out,
                                                        double* __restrict__ partials, int H, int W) {
    __shared__ float sx[TH + 2][TW + 2];
    __shared__ float sy[TH + 2][TW + 2];
    __shared__ double red[4];
    const int tx0 = blockIdx.x * TW, ty0 = blockIdx.y * TH;
    const size_t base = (size_t)blockIdx.z * H * W;
    stage_refl<1>(x + base, H, W, tx0, ty0, sx);
    stage_refl<1>(y + base, H, W, tx0, ty0, sy);
    __syncthreads();
    const int c = threadIdx.x & 63, r0 = (threadIdx.x >> 6) * 4, gx = tx0 + c;
    double sum = 0.0;
#pragma unroll
    for (int o = 0; o < 4; ++o) {
        const int gy = ty0 + r0 + o;
        if (gx < W && gy < H) {
            const float v = ssim3_value(ssim3_terms(stats9<TW + 2>(sx, sy, r0 + o, c)));
            const float cl = fminf(fmaxf(v, 0.f), 1.f);
            if (out) out[base + (size_t)gy * W + gx] = cl;
            sum += (double)cl;
        }
    }
    if (partials) {
        sum = block_sum_f64(sum, red);
        if (threadIdx.x == 0) partials[((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = sum;
    }
}

// grid (tiles_x, tiles_y, N).  g != NULL: the upstream map, times the scalar weight; g == NULL: the mean's weight, scalar * (1 / count)
__global__ __launch_bounds__(256) void ssim3_bwd_kernel(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ g,
                                                        float* __restrict__ gradx, float* __restrict__ grady, int H, int W, float count,
                                                        const float* __restrict__ gout, float gscale, const float* __restrict__ gscale_dev,
                                                        int accumulate) {
    __shared__ float sx[TH + 4][TW + 4];
    __shared__ float sy[TH + 4][TW + 4];
    __shared__ float cf[4][TH + 2][TW + 2];      // d / d mu_x, d / d mu_y, d / d E[x^2] = d / d E[y^2], d / d E[xy], each times g
    const int tx0 = blockIdx.x * TW, ty0 = blockIdx.y * TH;
    const size_t base = (size_t)blockIdx.z * H * W;
    stage_refl<2>(x + base, H, W, tx0, ty0, sx);
    stage_refl<2>(y + base, H, W, tx0, ty0, sy);
    const float k = (float)upstream(gscale, gscale_dev, gout);
    const float kmean = k * (1.f / count);
    __syncthreads();
    for (int i = threadIdx.x; i < (TH + 2) * (TW + 2); i += 256) {
        const int r = i / (TW + 2), c = i - r * (TW + 2);
        const int py = ty0 - 1 + r, px = tx0 - 1 + c;
        float dmx = 0.f, dmy = 0.f, dq = 0.f, dr = 0.f;
        if (py >= 0 && py < H && px >= 0 && px < W) {
            const Stats s = stats9<TW + 4>(sx, sy, r, c);
            const Terms t = ssim3_terms(s);
            const float v = ssim3_value(t);
            if (v >= 0.f && v <= 1.f) {       // torch.clamp's backward: the bounds pass
                const float gp = g ? g[base + (size_t)py * W + px] * k : kmean;
                const float w = gp * -0.5f / 9.f;             // out = (1 - S) / 2, a mean = sum / 9
                const float inv = 1.f / (t.B1 * t.B2), i1 = 1.f / t.B1, i2 = 1.f / t.B2, S = (t.A1 * t.A2) * inv;
                const float da = 2.f * (t.A2 - t.A1) * inv, db = 2.f * S * (i1 - i2);
                dmx = w * (s.my * da - s.mx * db);
                dmy = w * (s.mx * da - s.my * db);
                dq = w * -(S * i2);
                dr = w * (2.f * t.A1 * inv);
            }
        }
        cf[0][r][c] = dmx; cf[1][r][c] = dmy; cf[2][r][c] = dq; cf[3][r][c] = dr;
    }
    __syncthreads();
    const int c = threadIdx.x & 63, r0 = (threadIdx.x >> 6) * 4, ix = tx0 + c;
    if (ix >= W) return;
    const float wx[3] = {ix >= 1 ? (ix == 1 ? 2.f : 1.f) : 0.f, 1.f, ix + 1 < W ? (ix == W - 2 ? 2.f : 1.f) : 0.f};
#pragma unroll
    for (int o = 0; o < 4; ++o) {
        const int iy = ty0 + r0 + o;
        if (iy >= H) continue;
        const float wy[3] = {iy >= 1 ? (iy == 1 ? 2.f : 1.f) : 0.f, 1.f, iy + 1 < H ? (iy == H - 2 ? 2.f : 1.f) : 0.f};
        float ax = 0.f, ay = 0.f, q = 0.f, rr = 0.f;
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) {
                const float m = wy[dy] * wx[dx];
                ax += m * cf[0][r0 + o + dy][c + dx];
                ay += m * cf[1][r0 + o + dy][c + dx];
                q += m * cf[2][r0 + o + dy][c + dx];
                rr += m * cf[3][r0 + o + dy][c + dx];
            }
        const float xv = sx[r0 + o + 2][c + 2], yv = sy[r0 + o + 2][c + 2];
        const size_t idx = base + (size_t)iy * W + ix;
        if (gradx) {
            const float v = ax + 2.f * xv * q + yv * rr;
            gradx[idx] = accumulate ? gradx[idx] + v : v;
        }
        if (grady) {
            const float v = ay + 2.f * yv * q + xv * rr;
            grady[idx] = accumulate ? grady[idx] + v : v;
        }
    }
}

inline bool ssim3_dims_ok(int N, int H, int W) { return N > 0 && N <= 65535 && H >= 2 && W >= 2 && wm_cdiv(H, TH) <= 65535; }
inline dim3 ssim3_grid(int N, int H, int W) { return dim3(wm_cdiv(W, TW), wm_cdiv(H, TH), N); }

// ------------------------------------------------------------------------------------------------ the three reductions
constexpr int MASKL1 = WM_PIXLOSS_MASKL1, NONBLURRY = WM_PIXLOSS_NONBLURRY, GRAY = WM_PIXLOSS_GRAY;

__device__ __forceinline__ int sgn(double d) { return (d > 0.0) - (d < 0.0); }   // 0 at 0, as torch's abs / L1 backward

// one element's terms: s0 += |m a - m b| (the two products are exact in double, their difference is rounded once), s1 += |m|;  or s0 += (x - 1/2)^2;  or s0 += |x - 1/2|
template <int KIND> __device__ __forceinline__ void pix_acc(float a, float b, float m, double& s0, double& s1) {
    if (KIND == MASKL1) { s0 += fabs((double)m * (double)a - (double)m * (double)b); s1 += fabs((double)m); }
    else { const double d = (double)a - 0.5; s0 += KIND == NONBLURRY ? d * d : fabs(d); }
}

// grid (P): block j takes its grid-stride share -> partials[2 j + {0, 1}]
template <int KIND>
__global__ __launch_bounds__(256) void pix_sums_kernel(const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ m, size_t n,
                                                       double* __restrict__ partials) {
    const Split sp = split16(n, a, b, m);
    double s0 = 0.0, s1 = 0.0;
    stream16(sp, n,
             [&](size_t at) {
                 const float4 p = ld16(a + at);
                 float4 q = p, w = p;
                 if (KIND == MASKL1) { q = ld16(b + at); w = ld16(m + at); }
                 pix_acc<KIND>(p.x, q.x, w.x, s0, s1); pix_acc<KIND>(p.y, q.y, w.y, s0, s1);
                 pix_acc<KIND>(p.z, q.z, w.z, s0, s1); pix_acc<KIND>(p.w, q.w, w.w, s0, s1);
             },
             [&](size_t idx) { pix_acc<KIND>(a[idx], KIND == MASKL1 ? b[idx] : 0.f, KIND == MASKL1 ? m[idx] : 0.f, s0, s1); });
    __shared__ double s[2][4];
    s0 = block_sum_f64(s0, s[0]);
    s1 = block_sum_f64(s1, s[1]);
    if (threadIdx.x == 0) { partials[2 * (size_t)blockIdx.x] = s0; partials[2 * (size_t)blockIdx.x + 1] = s1; }
}

// one workgroup: coef[0] = mean of the first sum, coef[1] = of the second; the loss from them
template <int KIND>
__global__ __launch_bounds__(256) void pix_finalize_kernel(const double* __restrict__ partials, int nparts, double n, double* __restrict__ coef,
                                                           float* __restrict__ out) {
    __shared__ double s[2][4];
    double s0 = 0.0, s1 = 0.0;
    for (int i = threadIdx.x; i < nparts; i += 256) { s0 += partials[2 * i]; s1 += partials[2 * i + 1]; }
    s0 = block_sum_f64(s0, s[0]);
    s1 = block_sum_f64(s1, s[1]);
    if (threadIdx.x == 0) {
        const double m0 = s0 / n, m1 = s1 / n;
        coef[0] = m0; coef[1] = m1;
        out[0] = (float)(KIND == MASKL1 ? m0 / m1 : (KIND == NONBLURRY ? 1.0 - m0 : 1.0 / m0));   // (a zero mask: 0 / 0, as the reference)
    }
}

// d loss / d (a, b) of one element, times k:  MASKL1: k = g / (n mean|m|), +-sign(m a - m b) m;  NONBLURRY: k = -2 g / n, (x - 1/2);
// GRAY: k = -g / (n mean^2), sign(x - 1/2)
template <int KIND> __device__ __forceinline__ float pix_d(float a, float b, float m, double k) {
    if (KIND == MASKL1) return (float)(k * ((double)sgn((double)m * (double)a - (double)m * (double)b) * (double)m));
    const double d = (double)a - 0.5;
    return (float)(k * (KIND == NONBLURRY ? d : (double)sgn(d)));
}

template <int KIND>
__global__ __launch_bounds__(256) void pix_bwd_kernel(const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ m,
                                                      const double* __restrict__ coef, float* __restrict__ ga, float* __restrict__ gb, size_t n,
                                                      const float* __restrict__ gout, float gscale, const float* __restrict__ gscale_dev,
                                                      int accumulate) {
    const double g = upstream(gscale, gscale_dev, gout);
    const double k = KIND == MASKL1 ? g / ((double)n * coef[1]) : (KIND == NONBLURRY ? -2.0 * g / (double)n : -g / ((double)n * coef[0] * coef[0]));
    const Split sp = split16(n, a, b, m, ga, gb);
    stream16(sp, n,
             [&](size_t at) {
                 const float4 p = ld16(a + at);
                 float4 q = p, w = p;
                 if (KIND == MASKL1) { q = ld16(b + at); w = ld16(m + at); }
                 const float4 r = make_float4(pix_d<KIND>(p.x, q.x, w.x, k), pix_d<KIND>(p.y, q.y, w.y, k), pix_d<KIND>(p.z, q.z, w.z, k),
                                              pix_d<KIND>(p.w, q.w, w.w, k));
                 if (ga) store4<float>(ga + at, r.x, r.y, r.z, r.w, accumulate);
                 if (gb) store4<float>(gb + at, -r.x, -r.y, -r.z, -r.w, accumulate);
             },
             [&](size_t idx) {
                 const float r = pix_d<KIND>(a[idx], KIND == MASKL1 ? b[idx] : 0.f, KIND == MASKL1 ? m[idx] : 0.f, k);
                 if (ga) store1<float>(ga + idx, r, accumulate);
                 if (gb) store1<float>(gb + idx, -r, accumulate);
             });
}

inline int pix_parts(size_t n) { return wm_groups(n, 4096, 256); }
inline int pix_bwd_groups(size_t n) { return wm_groups(n, 1024, 2048); }
inline bool pix_kind_ok(int k) { return k == MASKL1 || k == NONBLURRY || k == GRAY; }

}  // namespace

#define PIX_DISPATCH(KERNEL, grid, ...)                                                                           \
    do {                                                                                                          \
        if (kind == MASKL1) hipLaunchKernelGGL(KERNEL<MASKL1>, grid, dim3(256), 0, s, __VA_ARGS__);               \
        else if (kind == NONBLURRY) hipLaunchKernelGGL(KERNEL<NONBLURRY>, grid, dim3(256), 0, s, __VA_ARGS__);    \
        else hipLaunchKernelGGL(KERNEL<GRAY>, grid, dim3(256), 0, s, __VA_ARGS__);                                \
    } while (0)

extern "C" int wm_ssim3_nparts(int N, int H, int W) {
    if (N <= 0 || H <= 0 || W <= 0) return 0;
    const size_t n = (size_t)N * wm_cdiv(H, TH) * wm_cdiv(W, TW);
    return n > 0x7fffffffu ? 0 : (int)n;
}

extern "C" int wm_ssim3_fwd(const float* x, const float* y, float* out_map, double* partials, int N, int H, int W, void* stream) {
    WM_REQUIRE(x && y && (out_map || partials) && ssim3_dims_ok(N, H, W), WM_E_BADARG,
               "wm_ssim3_fwd: bad arguments (the map or the partials or both; B*C <= 65535; H, W >= 2: the reflection needs two pixels)");
    hipLaunchKernelGGL(ssim3_fwd_kernel, ssim3_grid(N, H, W), dim3(256), 0, (hipStream_t)stream, x, y, out_map, partials, H, W);
    WM_LAUNCH_CHECK("wm_ssim3_fwd");
    return WM_OK;
}

extern "C" int wm_ssim3_finalize(const double* partials, int N, int H, int W, float* loss_out, void* stream) {
    WM_REQUIRE(partials && loss_out && ssim3_dims_ok(N, H, W), WM_E_BADARG, "wm_ssim3_finalize: bad arguments");
    wm_sum_finalize(partials, (size_t)wm_ssim3_nparts(N, H, W), 1.0 / ((double)N * H * W), loss_out, (hipStream_t)stream);
    WM_LAUNCH_CHECK("wm_ssim3_finalize");
    return WM_OK;
}

extern "C" int wm_ssim3_bwd(const float* x, const float* y, const float* g, float* gx, float* gy, int N, int H, int W, const float* gout_dev,
                            float gscale, const float* gscale_dev, int accumulate, void* stream) {
    WM_REQUIRE(x && y && (gx || gy) && ssim3_dims_ok(N, H, W), WM_E_BADARG,
               "wm_ssim3_bwd: bad arguments (at least one gradient buffer; B*C <= 65535; H, W >= 2)");
    hipLaunchKernelGGL(ssim3_bwd_kernel, ssim3_grid(N, H, W), dim3(256), 0, (hipStream_t)stream, x, y, g, gx, gy, H, W, (float)((double)N * H * W),
                       gout_dev, gscale, gscale_dev, accumulate);
    WM_LAUNCH_CHECK("wm_ssim3_bwd");
    return WM_OK;
}

extern "C" int wm_pixloss_nparts(size_t n) { return n > 0 ? pix_parts(n) : 0; }

extern "C" int wm_pixloss_sums(int kind, const float* a, const float* b, const float* mask, size_t n, double* partials, void* stream) {
    WM_REQUIRE(pix_kind_ok(kind) && a && partials && n > 0 && (kind != MASKL1 || (b && mask)), WM_E_BADARG,
               "wm_pixloss_sums: bad arguments (kind WM_PIXLOSS_MASKL1 / NONBLURRY / GRAY; b and mask with MASKL1)");
    hipStream_t s = (hipStream_t)stream;
    if (kind != MASKL1) { b = nullptr; mask = nullptr; }
    PIX_DISPATCH(pix_sums_kernel, dim3(pix_parts(n)), a, b, mask, n, partials);
    WM_LAUNCH_CHECK("wm_pixloss_sums");
    return WM_OK;
}

extern "C" int wm_pixloss_finalize(int kind, const double* partials, size_t n, double* coef, float* loss_out, void* stream) {
    WM_REQUIRE(pix_kind_ok(kind) && partials && coef && loss_out && n > 0, WM_E_BADARG, "wm_pixloss_finalize: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    PIX_DISPATCH(pix_finalize_kernel, dim3(1), partials, pix_parts(n), (double)n, coef, loss_out);
    WM_LAUNCH_CHECK("wm_pixloss_finalize");
    return WM_OK;
}

extern "C" int wm_pixloss_bwd(int kind, const float* a, const float* b, const float* mask, const double* coef, float* ga, float* gb, size_t n,
                              const float* gout_dev, float gscale, const float* gscale_dev, int accumulate, void* stream) {
    WM_REQUIRE(pix_kind_ok(kind) && a && coef && n > 0 && (kind == MASKL1 ? (b && mask && (ga || gb)) : (ga && gb == nullptr)), WM_E_BADARG,
               "wm_pixloss_bwd: bad arguments (MASKL1: b, mask and at least one of ga, gb; otherwise ga alone)");
    hipStream_t s = (hipStream_t)stream;
    if (kind != MASKL1) { b = nullptr; mask = nullptr; }
    PIX_DISPATCH(pix_bwd_kernel, dim3(pix_bwd_groups(n)), a, b, mask, coef, ga, gb, n, gout_dev, gscale, gscale_dev, accumulate);
    WM_LAUNCH_CHECK("wm_pixloss_bwd");
    return WM_OK;
}
