// nn.InstanceNorm2d (+ ReLU) on NHWC activations [B,H,W,CP]: the normalisation of the reference's instance-normalised coupling subnet
// (models/modules/Subnet_constructor.py ResBlock: conv -> InstanceNorm2d -> ReLU), of FBCNN's conv() letter I and of networks.py's
// use_spectral_norm=False branches.  Statistics per (sample, channel) over the H*W plane, biased variance, no running statistics.
//
// Every kernel streams 16-byte channel vectors: thread t of a 256-thread workgroup owns channel vector t % NV (NV = CP / VE vectors per pixel,
// VE = 4 f32 / 8 16-bit values) and pixel slot t / NV, and walks its share of the workgroup's pixel chunk in steps of 256 / NV pixels -- a
// wave's loads are consecutive 16-byte vectors, and the per-channel constants stay in registers.  grid = (splits of the plane, B).
//   forward : wm_instnorm_stats  (sum x, sum x^2 -> mean, rstd)            + wm_instnorm_apply      x read twice, y written once
//   backward: wm_instnorm_bwd_sums (sum g, sum g xhat -> their means, dgamma, dbeta) + wm_instnorm_bwd_apply   x, dy read twice, dx written once
// A plane of more than IN_CHUNK pixels spans several workgroups; their partial sums (double) are then combined by a one-thread-per-channel
// finalise launch in split order.  The backward's finalise also runs when the layer is affine: dgamma / dbeta sum over the samples.
// No atomics: every sum is a double accumulated in a fixed order (thread's pixels, slot_sum_f64's slots, the splits, the samples), so two
// runs agree bit for bit.  xhat = (x - mean) * rstd is recomputed from x in the backward, and so is the ReLU mask: z > 0 on the value AS
// STORED (z rounded to the activation type), from the same expressions as the forward.
#include "wm_reduce.h"

namespace {

constexpr size_t IN_CHUNK = 256;     // pixels of a plane per workgroup ...
constexpr size_t IN_MAX_SPLIT = 64;  // ... unless that makes more than this many splits: then ceil(hw / 64)

inline size_t in_chunk(size_t hw) {
    const size_t c = (hw + IN_MAX_SPLIT - 1) / IN_MAX_SPLIT;
    return c > IN_CHUNK ? c : IN_CHUNK;
}
inline int in_splits(size_t hw) { return (int)((hw + in_chunk(hw) - 1) / in_chunk(hw)); }

// xhat = (x - mean) * rstd, the difference and the product in double and ONE rounding to f32: the f32 difference alone loses up to half an
// ulp of x - mean before rstd (up to 316) scales it, and the invertible embedder's reverse pass magnifies what its subnets lose.  One
// definition for the forward, the backward and the backward's mask
__device__ __forceinline__ float in_xhat(float x, float mean, float rstd) { return (float)(((double)x - (double)mean) * (double)rstd); }
// z = xhat * gamma + beta (affine) or xhat; one definition for the forward and the backward's mask
__device__ __forceinline__ float in_z(float xh, bool affine, float gamma, float beta) { return affine ? __builtin_fmaf(xh, gamma, beta) : xh; }

// the per-channel constants of a thread's channel vector.  Channels >= C: real false, everything zero
template <int VE> struct InChan {
    float mean[VE], rstd[VE], gamma[VE], beta[VE];
    bool real[VE];
    __device__ __forceinline__ void load(const float* __restrict__ m, const float* __restrict__ r, const float* __restrict__ g, const float* __restrict__ b,
                                         size_t row, int c0, int C) {
#pragma unroll
        for (int e = 0; e < VE; ++e) {
            real[e] = c0 + e < C;
            mean[e] = real[e] ? m[row + c0 + e] : 0.f;
            rstd[e] = real[e] ? r[row + c0 + e] : 0.f;
            gamma[e] = (g && real[e]) ? g[c0 + e] : 0.f;
            beta[e] = (b && real[e]) ? b[c0 + e] : 0.f;
        }
    }
};

// mean, rstd of one (sample, channel) from its sums
__device__ __forceinline__ void in_finish(double s1, double s2, double n, double eps, float& mean, float& rstd) {
    const double m = s1 / n;
    double var = s2 / n - m * m;
    var = var > 0.0 ? var : 0.0;
    mean = (float)m;
    rstd = (float)(1.0 / sqrt(var + eps));
}

template <typename T>
__global__ __launch_bounds__(256) void instnorm_stats_kernel(const T* __restrict__ x, size_t hw, int C, int CP, size_t chunk, double eps,
                                                             double* __restrict__ part, float* __restrict__ mean, float* __restrict__ rstd) {
    constexpr int VE = 16 / sizeof(T);
    const int NV = CP / VE, slots = 256 / NV;
    const int v = threadIdx.x % NV, slot = threadIdx.x / NV, b = blockIdx.y;
    const size_t p0 = blockIdx.x * chunk, p1 = p0 + chunk < hw ? p0 + chunk : hw;
    double s1[VE], s2[VE];
#pragma unroll
    for (int e = 0; e < VE; ++e) s1[e] = s2[e] = 0.0;
    if (slot < slots) {
        const T* px = x + (size_t)b * hw * CP + (size_t)v * VE;
        for (size_t p = p0 + slot; p < p1; p += slots) {
            const vec16<T> t = *reinterpret_cast<const vec16<T>*>(px + p * CP);
#pragma unroll
            for (int e = 0; e < VE; ++e) {
                const double f = (double)t.get(e);
                s1[e] += f;
                s2[e] += f * f;
            }
        }
    }
    __shared__ double sh[256 * VE];
    slot_sum_f64<VE>(s1, sh, NV, slots);
    slot_sum_f64<VE>(s2, sh, NV, slots);
    if ((int)threadIdx.x < NV) {
#pragma unroll
        for (int e = 0; e < VE; ++e) {
            const int c = v * VE + e;
            if (gridDim.x == 1) {
                float m = 0.f, r = 0.f;
                if (c < C) in_finish(s1[e], s2[e], (double)hw, eps, m, r);
                mean[(size_t)b * CP + c] = m;
                rstd[(size_t)b * CP + c] = r;
            } else {
                double* q = part + ((size_t)b * gridDim.x + blockIdx.x) * 2 * CP + c;
                q[0] = s1[e];
                q[CP] = s2[e];
            }
        }
    }
}

// grid (ceil(CP / 256), B): one thread per (sample, channel) adds the S splits in order
__global__ __launch_bounds__(256) void instnorm_stats_finalize_kernel(const double* __restrict__ part, int S, size_t hw, int C, int CP, double eps,
                                                                      float* __restrict__ mean, float* __restrict__ rstd) {
    const int c = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (c >= CP) return;
    double s1 = 0.0, s2 = 0.0;
    for (int s = 0; s < S; ++s) {
        const double* q = part + ((size_t)b * S + s) * 2 * CP + c;
        s1 += q[0];
        s2 += q[CP];
    }
    float m = 0.f, r = 0.f;
    if (c < C) in_finish(s1, s2, (double)hw, eps, m, r);
    mean[(size_t)b * CP + c] = m;
    rstd[(size_t)b * CP + c] = r;
}

template <typename T>
__global__ __launch_bounds__(256) void instnorm_apply_kernel(const T* __restrict__ x, const float* __restrict__ mean, const float* __restrict__ rstd,
                                                             const float* __restrict__ gamma, const float* __restrict__ beta, T* __restrict__ y,
                                                             size_t hw, int C, int CP, size_t chunk, int act) {
    constexpr int VE = 16 / sizeof(T);
    const int NV = CP / VE, slots = 256 / NV;
    const int v = threadIdx.x % NV, slot = threadIdx.x / NV, b = blockIdx.y;
    if (slot >= slots) return;
    const size_t p0 = blockIdx.x * chunk, p1 = p0 + chunk < hw ? p0 + chunk : hw;
    InChan<VE> k;
    k.load(mean, rstd, gamma, beta, (size_t)b * CP, v * VE, C);
    const bool affine = gamma != nullptr;
    const size_t base = (size_t)b * hw * CP + (size_t)v * VE;
    for (size_t p = p0 + slot; p < p1; p += slots) {
        const vec16<T> t = *reinterpret_cast<const vec16<T>*>(x + base + p * CP);
        vec16<T> o;
#pragma unroll
        for (int e = 0; e < VE; ++e) {
            float z = in_z(in_xhat(t.get(e), k.mean[e], k.rstd[e]), affine, k.gamma[e], k.beta[e]);
            if (act) z = z < 0.f ? 0.f : z;
            o.set(e, k.real[e] ? z : 0.f);
        }
        *reinterpret_cast<vec16<T>*>(y + base + p * CP) = o;
    }
}

// g = dy * act'(y) and xhat of one element; real false: both zero
template <typename T, int VE>
__device__ __forceinline__ void in_g_xhat(const InChan<VE>& k, int e, float x, float dy, bool affine, int act, float& g, float& xh) {
    xh = k.real[e] ? in_xhat(x, k.mean[e], k.rstd[e]) : 0.f;
    g = k.real[e] ? dy : 0.f;
    if (act && !(to_f32(from_f32<T>(in_z(xh, affine, k.gamma[e], k.beta[e]))) > 0.f)) g = 0.f;
}

template <typename T>
__global__ __launch_bounds__(256) void instnorm_bwd_sums_kernel(const T* __restrict__ x, const T* __restrict__ dy, const float* __restrict__ mean,
                                                                const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                                const float* __restrict__ beta, size_t hw, int C, int CP, size_t chunk, int act,
                                                                int direct, double* __restrict__ part, float* __restrict__ mg, float* __restrict__ mgx) {
    constexpr int VE = 16 / sizeof(T);
    const int NV = CP / VE, slots = 256 / NV;
    const int v = threadIdx.x % NV, slot = threadIdx.x / NV, b = blockIdx.y;
    const size_t p0 = blockIdx.x * chunk, p1 = p0 + chunk < hw ? p0 + chunk : hw;
    double s1[VE], s2[VE];
#pragma unroll
    for (int e = 0; e < VE; ++e) s1[e] = s2[e] = 0.0;
    if (slot < slots) {
        InChan<VE> k;
        k.load(mean, rstd, gamma, beta, (size_t)b * CP, v * VE, C);
        const bool affine = gamma != nullptr;
        const size_t base = (size_t)b * hw * CP + (size_t)v * VE;
        for (size_t p = p0 + slot; p < p1; p += slots) {
            const vec16<T> t = *reinterpret_cast<const vec16<T>*>(x + base + p * CP);
            const vec16<T> d = *reinterpret_cast<const vec16<T>*>(dy + base + p * CP);
#pragma unroll
            for (int e = 0; e < VE; ++e) {
                float g, xh;
                in_g_xhat<T, VE>(k, e, t.get(e), d.get(e), affine, act, g, xh);
                s1[e] += (double)g;
                s2[e] += (double)g * (double)xh;
            }
        }
    }
    __shared__ double sh[256 * VE];
    slot_sum_f64<VE>(s1, sh, NV, slots);
    slot_sum_f64<VE>(s2, sh, NV, slots);
    if ((int)threadIdx.x < NV) {
#pragma unroll
        for (int e = 0; e < VE; ++e) {
            const int c = v * VE + e;
            if (direct) {      // (one split and no parameter gradients: the means the apply pass reads, at once)
                mg[(size_t)b * CP + c] = (float)(s1[e] / (double)hw);
                mgx[(size_t)b * CP + c] = (float)(s2[e] / (double)hw);
            } else {
                double* q = part + ((size_t)b * gridDim.x + blockIdx.x) * 2 * CP + c;
                q[0] = s1[e];
                q[CP] = s2[e];
            }
        }
    }
}

// grid ceil(CP / 256): one thread per channel adds the S splits of every sample in order, then the samples
__global__ __launch_bounds__(256) void instnorm_bwd_finalize_kernel(const double* __restrict__ part, int B, int S, size_t hw, int C, int CP,
                                                                    float* __restrict__ mg, float* __restrict__ mgx, float* __restrict__ dgamma,
                                                                    float* __restrict__ dbeta) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= CP) return;
    double t1 = 0.0, t2 = 0.0;
    for (int b = 0; b < B; ++b) {
        double s1 = 0.0, s2 = 0.0;
        for (int s = 0; s < S; ++s) {
            const double* q = part + ((size_t)b * S + s) * 2 * CP + c;
            s1 += q[0];
            s2 += q[CP];
        }
        mg[(size_t)b * CP + c] = (float)(s1 / (double)hw);
        mgx[(size_t)b * CP + c] = (float)(s2 / (double)hw);
        t1 += s1;
        t2 += s2;
    }
    if (dgamma && c < C) {
        dgamma[c] = (float)t2;
        dbeta[c] = (float)t1;
    }
}

template <typename T>
__global__ __launch_bounds__(256) void instnorm_bwd_apply_kernel(const T* __restrict__ x, const T* __restrict__ dy, const float* __restrict__ mean,
                                                                 const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                                 const float* __restrict__ beta, const float* __restrict__ mg,
                                                                 const float* __restrict__ mgx, T* __restrict__ dx, size_t hw, int C, int CP,
                                                                 size_t chunk, int act) {
    constexpr int VE = 16 / sizeof(T);
    const int NV = CP / VE, slots = 256 / NV;
    const int v = threadIdx.x % NV, slot = threadIdx.x / NV, b = blockIdx.y;
    if (slot >= slots) return;
    const size_t p0 = blockIdx.x * chunk, p1 = p0 + chunk < hw ? p0 + chunk : hw;
    InChan<VE> k;
    k.load(mean, rstd, gamma, beta, (size_t)b * CP, v * VE, C);
    const bool affine = gamma != nullptr;
    float a[VE], m1[VE], m2[VE];      // gamma * rstd, mean(g), mean(g xhat)
#pragma unroll
    for (int e = 0; e < VE; ++e) {
        a[e] = affine ? k.gamma[e] * k.rstd[e] : k.rstd[e];
        m1[e] = k.real[e] ? mg[(size_t)b * CP + v * VE + e] : 0.f;
        m2[e] = k.real[e] ? mgx[(size_t)b * CP + v * VE + e] : 0.f;
    }
    const size_t base = (size_t)b * hw * CP + (size_t)v * VE;
    for (size_t p = p0 + slot; p < p1; p += slots) {
        const vec16<T> t = *reinterpret_cast<const vec16<T>*>(x + base + p * CP);
        const vec16<T> d = *reinterpret_cast<const vec16<T>*>(dy + base + p * CP);
        vec16<T> o;
#pragma unroll
        for (int e = 0; e < VE; ++e) {
            float g, xh;
            in_g_xhat<T, VE>(k, e, t.get(e), d.get(e), affine, act, g, xh);
            o.set(e, k.real[e] ? a[e] * __builtin_fmaf(-xh, m2[e], g - m1[e]) : 0.f);
        }
        *reinterpret_cast<vec16<T>*>(dx + base + p * CP) = o;
    }
}

int in_check(const char* name, int B, size_t hw, int C, int CP, int act, int dtype, const void* a, const void* b, const void* c) {
    WM_REQUIRE(B > 0 && B <= 65535 && hw > 0 && C > 0 && C <= CP && CP % 16 == 0, WM_E_BADARG, "%s: bad shape (B %d, hw %zu, C %d, CP %d)", name, B, hw, C, CP);
    WM_REQUIRE(act == 0 || act == 1, WM_E_BADARG, "%s: act %d (0 none, 1 ReLU)", name, act);
    WM_REQUIRE(dtype == WM_F32 || dtype == WM_BF16 || dtype == WM_F16, WM_E_BADARG, "%s: unsupported dtype %d", name, dtype);
    WM_REQUIRE(CP / (dtype == WM_F32 ? 4 : 8) <= 256, WM_E_SHAPE, "%s: channel stride %d exceeds a workgroup's 256 16-byte vectors", name, CP);
    WM_REQUIRE((((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15) == 0, WM_E_SHAPE, "%s: activations must be 16-byte aligned", name);
    return 0;
}

}  // namespace

extern "C" int wm_instnorm_splits(size_t hw) { return hw > 0 ? in_splits(hw) : 0; }

extern "C" size_t wm_instnorm_scratch_doubles(int B, size_t hw, int CP) {
    return (B > 0 && hw > 0 && CP > 0) ? (size_t)B * in_splits(hw) * 2 * CP : 0;
}

extern "C" int wm_instnorm_stats(const void* x, double* partial, float* mean, float* rstd, int B, size_t hw, int C, int CP, double eps, int dtype,
                                 void* stream) {
    WM_REQUIRE(x && partial && mean && rstd && eps >= 0.0, WM_E_BADARG, "wm_instnorm_stats: null pointer or negative eps");
    if (int rc = in_check("wm_instnorm_stats", B, hw, C, CP, 0, dtype, x, nullptr, nullptr)) return rc;
    const int S = in_splits(hw);
    WM_DISPATCH_DTYPE(dtype, "wm_instnorm_stats", {
        hipLaunchKernelGGL(instnorm_stats_kernel<T>, dim3(S, B), dim3(256), 0, (hipStream_t)stream, (const T*)x, hw, C, CP, in_chunk(hw), eps, partial, mean, rstd);
    });
    WM_LAUNCH_CHECK("wm_instnorm_stats");
    if (S > 1) {
        hipLaunchKernelGGL(instnorm_stats_finalize_kernel, dim3(wm_cdiv(CP, 256), B), dim3(256), 0, (hipStream_t)stream, partial, S, hw, C, CP, eps, mean, rstd);
        WM_LAUNCH_CHECK("wm_instnorm_stats (finalise)");
    }
    return 0;
}

extern "C" int wm_instnorm_apply(const void* x, const float* mean, const float* rstd, const float* gamma, const float* beta, void* y, int B,
                                 size_t hw, int C, int CP, int act, int dtype, void* stream) {
    WM_REQUIRE(x && mean && rstd && y && (gamma == nullptr) == (beta == nullptr), WM_E_BADARG, "wm_instnorm_apply: null pointer, or gamma without beta");
    if (int rc = in_check("wm_instnorm_apply", B, hw, C, CP, act, dtype, x, y, nullptr)) return rc;
    WM_DISPATCH_DTYPE(dtype, "wm_instnorm_apply", {
        hipLaunchKernelGGL(instnorm_apply_kernel<T>, dim3(in_splits(hw), B), dim3(256), 0, (hipStream_t)stream, (const T*)x, mean, rstd, gamma, beta, (T*)y, hw, C,
                           CP, in_chunk(hw), act);
    });
    WM_LAUNCH_CHECK("wm_instnorm_apply");
    return 0;
}

extern "C" int wm_instnorm_bwd_sums(const void* x, const void* dy, const float* mean, const float* rstd, const float* gamma, const float* beta,
                                    double* partial, float* mg, float* mgx, float* dgamma, float* dbeta, int B, size_t hw, int C, int CP, int act,
                                    int dtype, void* stream) {
    WM_REQUIRE(x && dy && mean && rstd && partial && mg && mgx, WM_E_BADARG, "wm_instnorm_bwd_sums: null pointer");
    WM_REQUIRE((gamma == nullptr) == (beta == nullptr) && (dgamma == nullptr) == (dbeta == nullptr), WM_E_BADARG,
               "wm_instnorm_bwd_sums: gamma / beta and dgamma / dbeta come in pairs");
    if (int rc = in_check("wm_instnorm_bwd_sums", B, hw, C, CP, act, dtype, x, dy, nullptr)) return rc;
    const int S = in_splits(hw), direct = (S == 1 && dgamma == nullptr) ? 1 : 0;
    WM_DISPATCH_DTYPE(dtype, "wm_instnorm_bwd_sums", {
        hipLaunchKernelGGL(instnorm_bwd_sums_kernel<T>, dim3(S, B), dim3(256), 0, (hipStream_t)stream, (const T*)x, (const T*)dy, mean, rstd, gamma, beta, hw, C, CP,
                           in_chunk(hw), act, direct, partial, mg, mgx);
    });
    WM_LAUNCH_CHECK("wm_instnorm_bwd_sums");
    if (!direct) {
        hipLaunchKernelGGL(instnorm_bwd_finalize_kernel, dim3(wm_cdiv(CP, 256)), dim3(256), 0, (hipStream_t)stream, partial, B, S, hw, C, CP, mg, mgx, dgamma, dbeta);
        WM_LAUNCH_CHECK("wm_instnorm_bwd_sums (finalise)");
    }
    return 0;
}

extern "C" int wm_instnorm_bwd_apply(const void* x, const void* dy, const float* mean, const float* rstd, const float* gamma, const float* beta,
                                     const float* mg, const float* mgx, void* dx, int B, size_t hw, int C, int CP, int act, int dtype, void* stream) {
    WM_REQUIRE(x && dy && mean && rstd && mg && mgx && dx && (gamma == nullptr) == (beta == nullptr), WM_E_BADARG,
               "wm_instnorm_bwd_apply: null pointer, or gamma without beta");
    if (int rc = in_check("wm_instnorm_bwd_apply", B, hw, C, CP, act, dtype, x, dy, dx)) return rc;
    WM_DISPATCH_DTYPE(dtype, "wm_instnorm_bwd_apply", {
        hipLaunchKernelGGL(instnorm_bwd_apply_kernel<T>, dim3(in_splits(hw), B), dim3(256), 0, (hipStream_t)stream, (const T*)x, (const T*)dy, mean, rstd, gamma, beta,
                           mg, mgx, (T*)dx, hw, C, CP, in_chunk(hw), act);
    });
    WM_LAUNCH_CHECK("wm_instnorm_bwd_apply");
    return 0;
}
