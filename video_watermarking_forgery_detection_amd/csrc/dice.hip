// Dice (overlap) loss of the tamper localiser and its multi-class form (dice_loss.py:44-61 BinaryDiceLoss.forward, :81-96 DiceLoss.forward of
// the reference, and the autograd backward of both):
//   sum(p*t), sum(p^pw), sum(t^pw) per sample (:49-50)     wm_dice_sums           f32 [B, per_sample] probabilities and targets
//   the same per (sample, class) of softmax(logits, 1)      wm_dice_softmax_sums   f32 NCHW logits [B,C,HW]; the softmax (:85) is never written
//   num, den, 1 - num/den, the reduction, the class loop    wm_dice_finalize       (:52-59, :87-96: ignore_index, weight, / C)
//   d loss / d p (optionally through the sigmoid)           wm_dice_bwd            grad (+)= g * (num*pw*p^(pw-1) - t*den) / den^2 [* p(1-p)]
//   d loss / d logits                                       wm_dice_softmax_bwd    dz_c = s_c * (g_c - sum_k g_k s_k), softmax recomputed
// No atomics and no host synchronisation: every sums kernel writes per-workgroup partials in double (unit u = sample, or sample*C + class:
// its wm_dice_nparts(per_sample) <= 64 partials of 3 doubles are contiguous), the finalise launch sums each unit's partials in one wave in a
// fixed order and keeps num / den in double for the backward.  Every result is bitwise reproducible.
//
// Elements are multiplied in f32 (as the reference's f32 run does) and added in double.  pw = 1 and pw = 2 are compile-time paths without
// powf; any other positive exponent goes through powf.
#include "wm_common.h"
#include "wm_reduce.h"

namespace {

constexpr int RED_MEAN = WM_DICE_MEAN, RED_NONE = WM_DICE_NONE;
constexpr int MAXC = 32;        // classes of the softmax form
constexpr int TILE = 1024;      // pixels a workgroup of the softmax kernels handles per iteration: 4 per thread

template <int PW> __device__ __forceinline__ float pow_p(float x, float pw) {
    if (PW == 1) return x;
    if (PW == 2) return x * x;
    return powf(x, pw);
}
// x^(pw-1): the factor of d x^pw / dx = pw * x^(pw-1)
template <int PW> __device__ __forceinline__ float pow_pm1(float x, float pw) {
    if (PW == 1) return 1.f;
    if (PW == 2) return x;
    return powf(x, pw - 1.f);
}

// grid (P, B): block (j, b) takes its grid-stride share of sample b -> partials[(b*P + j)*3 + {sum p*t, sum p^pw, sum t^pw}]
template <int PW>
__global__ __launch_bounds__(256) void dice_sums_kernel(const float* __restrict__ p, const float* __restrict__ t, size_t per, float pw,
                                                        double* __restrict__ partials) {
    const float* pb = p + (size_t)blockIdx.y * per;
    const float* tb = t + (size_t)blockIdx.y * per;
    const Split sp = split16(per, pb, tb);
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    stream16(sp, per,
             [&](size_t at) {
                 const float4 x = ld16(pb + at), y = ld16(tb + at);
                 a0 += (double)(x.x * y.x); a0 += (double)(x.y * y.y); a0 += (double)(x.z * y.z); a0 += (double)(x.w * y.w);
                 a1 += (double)pow_p<PW>(x.x, pw); a1 += (double)pow_p<PW>(x.y, pw); a1 += (double)pow_p<PW>(x.z, pw); a1 += (double)pow_p<PW>(x.w, pw);
                 a2 += (double)pow_p<PW>(y.x, pw); a2 += (double)pow_p<PW>(y.y, pw); a2 += (double)pow_p<PW>(y.z, pw); a2 += (double)pow_p<PW>(y.w, pw);
             },
             [&](size_t idx) {
                 const float x = pb[idx], y = tb[idx];
                 a0 += (double)(x * y); a1 += (double)pow_p<PW>(x, pw); a2 += (double)pow_p<PW>(y, pw);
             });
    __shared__ double s[3][4];
    a0 = block_sum_f64(a0, s[0]); a1 = block_sum_f64(a1, s[1]); a2 = block_sum_f64(a2, s[2]);
    if (threadIdx.x == 0) {
        double* q = partials + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 3;
        q[0] = a0; q[1] = a1; q[2] = a2;
    }
}

// ---- the softmax form: a thread owns 4 pixels of a 1024-pixel tile.  VEC (HW % 4 == 0, 16-byte aligned bases): pixels pix0 .. pix0+3 as one
// float4 per plane; otherwise pixels pix0 + {0, 256, 512, 768}, each its own coalesced load.  Pixels past HW read as 0 and are masked out.
template <bool VEC> __device__ __forceinline__ size_t tile_pix0(size_t tile) {
    return tile * TILE + (VEC ? (size_t)threadIdx.x * 4 : (size_t)threadIdx.x);
}
template <bool VEC> __device__ __forceinline__ bool pix_ok(size_t pix0, int k, size_t HW) { return pix0 + (VEC ? k : k * 256) < HW; }
template <bool VEC> __device__ __forceinline__ void ld4(const float* __restrict__ plane, size_t pix0, size_t HW, float (&v)[4]) {
    if (VEC) {
        float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
        if (pix0 < HW) x = *reinterpret_cast<const float4*>(plane + pix0);
        v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = pix0 + k * 256 < HW ? plane[pix0 + k * 256] : 0.f;
    }
}
template <bool VEC> __device__ __forceinline__ void st4(float* __restrict__ plane, size_t pix0, size_t HW, const float (&v)[4], int accumulate) {
    if (VEC) {
        if (pix0 < HW) {
            float4* q = reinterpret_cast<float4*>(plane + pix0);
            float4 x = make_float4(v[0], v[1], v[2], v[3]);
            if (accumulate) { const float4 o = *q; x.x += o.x; x.y += o.y; x.z += o.z; x.w += o.w; }
            *q = x;
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (pix0 + k * 256 < HW) plane[pix0 + k * 256] = accumulate ? plane[pix0 + k * 256] + v[k] : v[k];
    }
}
// max over the C planes and 1 / sum exp(z - max) of the thread's 4 pixels
template <bool VEC> __device__ __forceinline__ void softmax_stats(const float* __restrict__ zb, int C, size_t HW, size_t pix0, float (&m)[4], float (&inv)[4]) {
    float v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) m[k] = -INFINITY;
    for (int c = 0; c < C; ++c) {
        ld4<VEC>(zb + (size_t)c * HW, pix0, HW, v);
#pragma unroll
        for (int k = 0; k < 4; ++k) m[k] = fmaxf(m[k], v[k]);
    }
    float d[4] = {0.f, 0.f, 0.f, 0.f};
    for (int c = 0; c < C; ++c) {
        ld4<VEC>(zb + (size_t)c * HW, pix0, HW, v);
#pragma unroll
        for (int k = 0; k < 4; ++k) d[k] += expf(v[k] - m[k]);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) inv[k] = 1.f / d[k];
}

// grid (P, B): block (j, b) takes tiles j, j+P, ... of sample b -> partials[((b*C + c)*P + j)*3 + q].  Each wave keeps its running sums of
// the C classes in its own LDS row (written by its lane 0 only), so the tile loop needs no barrier.
template <int PW, bool VEC>
__global__ __launch_bounds__(256) void dice_softmax_sums_kernel(const float* __restrict__ z, const float* __restrict__ t, int C, size_t HW, float pw,
                                                                double* __restrict__ partials) {
    __shared__ double red[MAXC][4][3];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0)
        for (int c = 0; c < C; ++c) { red[c][w][0] = 0.0; red[c][w][1] = 0.0; red[c][w][2] = 0.0; }
    const float* zb = z + (size_t)blockIdx.y * C * HW;
    const float* tb = t + (size_t)blockIdx.y * C * HW;
    const size_t ntiles = (HW + TILE - 1) / TILE;
    for (size_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const size_t pix0 = tile_pix0<VEC>(tile);
        float m[4], inv[4], v[4], y[4];
        softmax_stats<VEC>(zb, C, HW, pix0, m, inv);
        for (int c = 0; c < C; ++c) {
            ld4<VEC>(zb + (size_t)c * HW, pix0, HW, v);
            ld4<VEC>(tb + (size_t)c * HW, pix0, HW, y);
            double a0 = 0.0, a1 = 0.0, a2 = 0.0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (pix_ok<VEC>(pix0, k, HW)) {
                    const float s = expf(v[k] - m[k]) * inv[k];
                    a0 += (double)(s * y[k]); a1 += (double)pow_p<PW>(s, pw); a2 += (double)pow_p<PW>(y[k], pw);
                }
            }
            a0 = wave_sum_f64(a0); a1 = wave_sum_f64(a1); a2 = wave_sum_f64(a2);
            if (lane == 0) { red[c][w][0] += a0; red[c][w][1] += a1; red[c][w][2] += a2; }
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < 3 * C) {
        const int c = threadIdx.x / 3, q = threadIdx.x - 3 * c;
        partials[(((size_t)blockIdx.y * C + c) * gridDim.x + blockIdx.x) * 3 + q] = (red[c][0][q] + red[c][1][q]) + (red[c][2][q] + red[c][3][q]);
    }
}

// the weight of unit (b, c)'s loss in the result, without the reduction's 1/B: (c == ignore_index ? 0 : weight[c]) / C
__device__ __forceinline__ double class_weight(int c, int C, int ignore_index, const float* __restrict__ weight) {
    if (c == ignore_index) return 0.0;
    return (weight ? (double)weight[c] : 1.0) / (double)C;
}

// one workgroup.  Wave w sums the P <= 64 partials of units w, w+4, ... (lane j holds partial j: a fixed butterfly) and writes
// coef[u] = {num, den}; then the loss: reduction none -> out[b] = sum_c weight_c (1 - num/den) / C, mean / sum -> out[0] over all units.
__global__ __launch_bounds__(256) void dice_finalize_kernel(const double* __restrict__ partials, int B, int C, int P, double smooth, int reduction,
                                                            int ignore_index, const float* __restrict__ weight, double* __restrict__ coef,
                                                            float* __restrict__ out) {
    __shared__ double s[256];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, U = B * C;
    for (int u = w; u < U; u += 4) {
        double v0 = 0.0, v1 = 0.0, v2 = 0.0;
        if (lane < P) {
            const double* q = partials + ((size_t)u * P + lane) * 3;
            v0 = q[0]; v1 = q[1]; v2 = q[2];
        }
        v0 = wave_sum_f64(v0); v1 = wave_sum_f64(v1); v2 = wave_sum_f64(v2);
        if (lane == 0) { coef[2 * (size_t)u] = v0 + smooth; coef[2 * (size_t)u + 1] = (v1 + v2) + smooth; }
    }
    __syncthreads();   // coef is read back below by other threads of this workgroup
    if (reduction == RED_NONE) {
        for (int b = threadIdx.x; b < B; b += 256) {
            double a = 0.0;
            for (int c = 0; c < C; ++c) {
                const size_t u = (size_t)b * C + c;
                a += class_weight(c, C, ignore_index, weight) * (1.0 - coef[2 * u] / coef[2 * u + 1]);
            }
            out[b] = (float)a;
        }
        return;
    }
    double a = 0.0;
    for (int u = threadIdx.x; u < U; u += 256) a += class_weight(u % C, C, ignore_index, weight) * (1.0 - coef[2 * (size_t)u] / coef[2 * (size_t)u + 1]);
    s[threadIdx.x] = a;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) s[threadIdx.x] += s[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = (float)(reduction == RED_MEAN ? s[0] / (double)B : s[0]);
}

// the upstream weight of sample b's loss: gscale * gscale_dev[0] * gout[none ? b : 0], / B for the mean
__device__ __forceinline__ double upstream_b(int b, int B, int reduction, float gscale, const float* __restrict__ gscale_dev, const float* __restrict__ gout) {
    const double g = upstream(gscale, gscale_dev, gout, reduction == RED_NONE ? b : 0);
    return reduction == RED_MEAN ? g / (double)B : g;
}

// grid (G, B).  d (1 - num/den) / d p_i = (num * pw * p_i^(pw-1) - t_i * den) / den^2 = kp * p_i^(pw-1) - kt * t_i
template <int PW>
__global__ __launch_bounds__(256) void dice_bwd_kernel(const float* __restrict__ p, const float* __restrict__ t, const double* __restrict__ coef,
                                                       float* __restrict__ grad, int B, size_t per, float pw, int reduction,
                                                       const float* __restrict__ gout, float gscale, const float* __restrict__ gscale_dev,
                                                       int chain_sigmoid, int accumulate) {
    const int b = blockIdx.y;
    const double g = upstream_b(b, B, reduction, gscale, gscale_dev, gout), num = coef[2 * b], den = coef[2 * b + 1];
    const float kt = (float)(g / den), kp = (float)(g * num * (double)pw / (den * den));
    const float* pb = p + (size_t)b * per;
    const float* tb = t + (size_t)b * per;
    float* gb = grad + (size_t)b * per;
    const Split sp = split16(per, pb, tb, gb);
    auto one = [&](float x, float y) {
        float v = kp * pow_pm1<PW>(x, pw) - kt * y;
        if (chain_sigmoid) v *= x * (1.f - x);
        return v;
    };
    stream16(sp, per,
             [&](size_t at) {
                 const float4 x = ld16(pb + at), y = ld16(tb + at);
                 store4<float>(gb + at, one(x.x, y.x), one(x.y, y.y), one(x.z, y.z), one(x.w, y.w), accumulate);
             },
             [&](size_t idx) { store1<float>(gb + idx, one(pb[idx], tb[idx]), accumulate); });
}

// grid (G, B).  g_c = d L / d s_c = kp[c] * s_c^(pw-1) - kt[c] * t_c with the class weight and the upstream weight folded into kp, kt
// (an ignored class has g_c = 0 but still receives -s_c * sum_k g_k s_k through the softmax);  dz_c = s_c * (g_c - sum_k g_k s_k)
template <int PW, bool VEC>
__global__ __launch_bounds__(256) void dice_softmax_bwd_kernel(const float* __restrict__ z, const float* __restrict__ t, const double* __restrict__ coef,
                                                               float* __restrict__ grad, int B, int C, size_t HW, float pw, int reduction,
                                                               int ignore_index, const float* __restrict__ weight, const float* __restrict__ gout,
                                                               float gscale, const float* __restrict__ gscale_dev, int accumulate) {
    __shared__ float kt[MAXC], kp[MAXC];
    const int b = blockIdx.y;
    if ((int)threadIdx.x < C) {
        const int c = threadIdx.x;
        const double g = upstream_b(b, B, reduction, gscale, gscale_dev, gout) * class_weight(c, C, ignore_index, weight);
        const double num = coef[2 * ((size_t)b * C + c)], den = coef[2 * ((size_t)b * C + c) + 1];
        kt[c] = (float)(g / den);
        kp[c] = (float)(g * num * (double)pw / (den * den));
    }
    __syncthreads();
    const float* zb = z + (size_t)b * C * HW;
    const float* tb = t + (size_t)b * C * HW;
    float* gb = grad + (size_t)b * C * HW;
    const size_t ntiles = (HW + TILE - 1) / TILE;
    for (size_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const size_t pix0 = tile_pix0<VEC>(tile);
        float m[4], inv[4], v[4], y[4], dot[4] = {0.f, 0.f, 0.f, 0.f};
        softmax_stats<VEC>(zb, C, HW, pix0, m, inv);
        for (int c = 0; c < C; ++c) {
            ld4<VEC>(zb + (size_t)c * HW, pix0, HW, v);
            ld4<VEC>(tb + (size_t)c * HW, pix0, HW, y);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float s = expf(v[k] - m[k]) * inv[k];
                dot[k] = __builtin_fmaf(kp[c] * pow_pm1<PW>(s, pw) - kt[c] * y[k], s, dot[k]);
            }
        }
        for (int c = 0; c < C; ++c) {
            ld4<VEC>(zb + (size_t)c * HW, pix0, HW, v);
            ld4<VEC>(tb + (size_t)c * HW, pix0, HW, y);
            float dz[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float s = expf(v[k] - m[k]) * inv[k];
                dz[k] = s * ((kp[c] * pow_pm1<PW>(s, pw) - kt[c] * y[k]) - dot[k]);
            }
            st4<VEC>(gb + (size_t)c * HW, pix0, HW, dz, accumulate);
        }
    }
}

inline int dice_parts(size_t per_sample) { return wm_groups(per_sample, 4096, 64); }
// workgroups per sample of an elementwise pass with `unit` elements per workgroup and iteration
inline int bwd_groups(size_t per_sample, size_t unit) { return wm_groups(per_sample, unit, 256); }
inline bool planes_vec(const void* a, const void* b, const void* c, size_t HW) {
    return HW % 4 == 0 && (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15) == 0;
}
inline bool reduction_ok(int r) { return r == WM_DICE_MEAN || r == WM_DICE_SUM || r == WM_DICE_NONE; }
inline int pw_path(float pw) { return pw == 1.f ? 1 : (pw == 2.f ? 2 : 0); }

}  // namespace

extern "C" int wm_dice_nparts(size_t per_sample) { return per_sample > 0 ? dice_parts(per_sample) : 0; }

extern "C" int wm_dice_sums(const float* p, const float* target, int B, size_t per_sample, float pw, double* partials, void* stream) {
    WM_REQUIRE(p && target && partials && B > 0 && B <= 65535 && per_sample > 0 && pw > 0.f, WM_E_BADARG,
               "wm_dice_sums: bad arguments (B <= 65535, pw > 0)");
    const dim3 grid(dice_parts(per_sample), B);
    hipStream_t s = (hipStream_t)stream;
    switch (pw_path(pw)) {
        case 1: hipLaunchKernelGGL(dice_sums_kernel<1>, grid, dim3(256), 0, s, p, target, per_sample, pw, partials); break;
        case 2: hipLaunchKernelGGL(dice_sums_kernel<2>, grid, dim3(256), 0, s, p, target, per_sample, pw, partials); break;
        default: hipLaunchKernelGGL(dice_sums_kernel<0>, grid, dim3(256), 0, s, p, target, per_sample, pw, partials); break;
    }
    WM_LAUNCH_CHECK("wm_dice_sums");
    return WM_OK;
}

#define DICE_SOFTMAX_DISPATCH(KERNEL, ...)                                                                            \
    do {                                                                                                              \
        const int path_ = pw_path(pw);                                                                                \
        if (vec) {                                                                                                    \
            if (path_ == 1) hipLaunchKernelGGL((KERNEL<1, true>), grid, dim3(256), 0, s, __VA_ARGS__);               \
            else if (path_ == 2) hipLaunchKernelGGL((KERNEL<2, true>), grid, dim3(256), 0, s, __VA_ARGS__);          \
            else hipLaunchKernelGGL((KERNEL<0, true>), grid, dim3(256), 0, s, __VA_ARGS__);                          \
        } else {                                                                                                      \
            if (path_ == 1) hipLaunchKernelGGL((KERNEL<1, false>), grid, dim3(256), 0, s, __VA_ARGS__);              \
            else if (path_ == 2) hipLaunchKernelGGL((KERNEL<2, false>), grid, dim3(256), 0, s, __VA_ARGS__);         \
            else hipLaunchKernelGGL((KERNEL<0, false>), grid, dim3(256), 0, s, __VA_ARGS__);                         \
        }                                                                                                             \
    } while (0)

extern "C" int wm_dice_softmax_sums(const float* logits, const float* target, int B, int C, size_t HW, float pw, double* partials, void* stream) {
    WM_REQUIRE(logits && target && partials && B > 0 && B <= 65535 && C > 0 && C <= MAXC && HW > 0 && pw > 0.f, WM_E_BADARG,
               "wm_dice_softmax_sums: bad arguments (B <= 65535, 1 <= C <= 32, pw > 0)");
    const dim3 grid(dice_parts(HW), B);
    hipStream_t s = (hipStream_t)stream;
    const bool vec = planes_vec(logits, target, nullptr, HW);
    DICE_SOFTMAX_DISPATCH(dice_softmax_sums_kernel, logits, target, C, HW, pw, partials);
    WM_LAUNCH_CHECK("wm_dice_softmax_sums");
    return WM_OK;
}

extern "C" int wm_dice_finalize(const double* partials, int B, int C, size_t per_sample, double smooth, int reduction, int ignore_index,
                                const float* weight, double* coef, float* loss_out, void* stream) {
    WM_REQUIRE(partials && coef && loss_out && B > 0 && C > 0 && C <= MAXC && per_sample > 0 && reduction_ok(reduction), WM_E_BADARG,
               "wm_dice_finalize: bad arguments (1 <= C <= 32, reduction WM_DICE_MEAN / SUM / NONE)");
    hipLaunchKernelGGL(dice_finalize_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, partials, B, C, dice_parts(per_sample), smooth, reduction,
                       ignore_index, weight, coef, loss_out);
    WM_LAUNCH_CHECK("wm_dice_finalize");
    return WM_OK;
}

extern "C" int wm_dice_bwd(const float* p, const float* target, const double* coef, float* grad, int B, size_t per_sample, float pw, int reduction,
                           const float* gout_dev, float gscale, const float* gscale_dev, int chain_sigmoid, int accumulate, void* stream) {
    WM_REQUIRE(p && target && coef && grad && B > 0 && B <= 65535 && per_sample > 0 && pw > 0.f && reduction_ok(reduction), WM_E_BADARG,
               "wm_dice_bwd: bad arguments (B <= 65535, pw > 0, reduction WM_DICE_MEAN / SUM / NONE)");
    const dim3 grid(bwd_groups(per_sample, 1024), B);
    hipStream_t s = (hipStream_t)stream;
    switch (pw_path(pw)) {
        case 1: hipLaunchKernelGGL(dice_bwd_kernel<1>, grid, dim3(256), 0, s, p, target, coef, grad, B, per_sample, pw, reduction, gout_dev, gscale, gscale_dev, chain_sigmoid, accumulate); break;
        case 2: hipLaunchKernelGGL(dice_bwd_kernel<2>, grid, dim3(256), 0, s, p, target, coef, grad, B, per_sample, pw, reduction, gout_dev, gscale, gscale_dev, chain_sigmoid, accumulate); break;
        default: hipLaunchKernelGGL(dice_bwd_kernel<0>, grid, dim3(256), 0, s, p, target, coef, grad, B, per_sample, pw, reduction, gout_dev, gscale, gscale_dev, chain_sigmoid, accumulate); break;
    }
    WM_LAUNCH_CHECK("wm_dice_bwd");
    return WM_OK;
}

extern "C" int wm_dice_softmax_bwd(const float* logits, const float* target, const double* coef, float* grad, int B, int C, size_t HW, float pw,
                                   int reduction, int ignore_index, const float* weight, const float* gout_dev, float gscale,
                                   const float* gscale_dev, int accumulate, void* stream) {
    WM_REQUIRE(logits && target && coef && grad && B > 0 && B <= 65535 && C > 0 && C <= MAXC && HW > 0 && pw > 0.f && reduction_ok(reduction),
               WM_E_BADARG, "wm_dice_softmax_bwd: bad arguments (B <= 65535, 1 <= C <= 32, pw > 0, reduction WM_DICE_MEAN / SUM / NONE)");
    const dim3 grid(bwd_groups(HW, TILE), B);
    hipStream_t s = (hipStream_t)stream;
    const bool vec = planes_vec(logits, target, grad, HW);
    DICE_SOFTMAX_DISPATCH(dice_softmax_bwd_kernel, logits, target, coef, grad, B, C, HW, pw, reduction, ignore_index, weight, gout_dev, gscale,
                          gscale_dev, accumulate);
    WM_LAUNCH_CHECK("wm_dice_softmax_bwd");
    return WM_OK;
}
