// What the streaming loss kernels (dice.hip, imgloss.hip, advloss.hip, ssim3.hip, ssim.hip) share: the fixed-order sums in double, the
// 16-byte split of a range with its grid-stride loop, the upstream weight, the (accumulating) gradient store and the one-workgroup
// "scale * sum of the partials" launch.  One definition each: the order of every addition is part of the results' bits.
#pragma once
#include "wm_common.h"

// wave-level sum (64 lanes) in double: a fixed butterfly
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// 256 threads -> the sum (fixed order); s: 4 doubles of LDS.  Contains one __syncthreads()
__device__ __forceinline__ double block_sum_f64(double v, double* s) {
    v = wave_sum_f64(v);
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
    __syncthreads();
    return (s[0] + s[1]) + (s[2] + s[3]);
}

// per-channel sums of an NHWC stream: thread t of 256 holds, for the VE channels of channel vector t % nv, the partial sums of pixel slot
// t / nv (slots = 256 / nv of them; threads past slots * nv take no part).  Afterwards threads t < nv hold in v[] the sums over the slots,
// added in slot order.  sh: 256 * VE doubles of LDS.  Contains two __syncthreads(): sh may be reused at once
template <int VE> __device__ __forceinline__ void slot_sum_f64(double (&v)[VE], double* sh, int nv, int slots) {
#pragma unroll
    for (int e = 0; e < VE; ++e) sh[threadIdx.x * VE + e] = v[e];
    __syncthreads();
    if ((int)threadIdx.x < nv)
        for (int k = 1; k < slots; ++k)
#pragma unroll
            for (int e = 0; e < VE; ++e) v[e] += sh[(k * nv + threadIdx.x) * VE + e];
    __syncthreads();
}

// [0, n) split for 16-byte access: a scalar head up to the first 16-byte boundary of `a`, nv float4s, a scalar tail.  The other pointers
// (nullptr = absent) share the split only when they reach a boundary at the same element; otherwise (nv = 0) everything is scalar
struct Split { size_t head, nv, tail0; };
__device__ __forceinline__ bool same16(const void* a, const void* b) { return b == nullptr || (((uintptr_t)a ^ (uintptr_t)b) & 15) == 0; }
template <typename... P> __device__ __forceinline__ Split split16(size_t n, const void* a, const P*... others) {
    Split s;
    s.head = ((16 - ((uintptr_t)a & 15)) & 15) >> 2;
    if (s.head > n) s.head = n;
    s.nv = (same16(a, others) && ...) ? (n - s.head) / 4 : 0;
    if (s.nv == 0) s.head = 0;
    s.tail0 = s.head + s.nv * 4;
    return s;
}

// A workgroup's grid-stride share (gridDim.x workgroups of 256 threads) of the split: body4(at) for the four elements from `at` (16-byte
// aligned in every pointer of the split), then body1(idx) for single elements of the head and the tail.  Per thread the float4s come first
template <typename F4, typename F1> __device__ __forceinline__ void stream16(const Split& sp, size_t n, F4 body4, F1 body1) {
    const size_t stride = (size_t)gridDim.x * 256, first = (size_t)blockIdx.x * 256 + threadIdx.x;
    for (size_t v = first; v < sp.nv; v += stride) body4(sp.head + 4 * v);
    const size_t nscalar = sp.head + (n - sp.tail0);
    for (size_t i = first; i < nscalar; i += stride) body1(i < sp.head ? i : sp.tail0 + (i - sp.head));
}

__device__ __forceinline__ float4 ld16(const float* p) { return *reinterpret_cast<const float4*>(p); }

// the upstream weight of a loss: gscale * gscale_dev[0] * gout[i]
__device__ __forceinline__ double upstream(float gscale, const float* __restrict__ gscale_dev, const float* __restrict__ gout, int i = 0) {
    double g = (double)gscale;
    if (gscale_dev) g *= (double)gscale_dev[0];
    if (gout) g *= (double)gout[i];
    return g;
}

// the gradient store: *q = v, or with accumulate *q + v.  T (float or double) is the type the addition is made in, rounded to f32 after it
template <typename T> __device__ __forceinline__ void store1(float* q, T v, int accumulate) {
    if (accumulate) v += (T)*q;
    *q = (float)v;
}
template <typename T> __device__ __forceinline__ void store4(float* q, T x, T y, T z, T w, int accumulate) {
    if (accumulate) { const float4 o = ld16(q); x += (T)o.x; y += (T)o.y; z += (T)o.z; w += (T)o.w; }
    *reinterpret_cast<float4*>(q) = make_float4((float)x, (float)y, (float)z, (float)w);
}

// workgroups of a pass over n elements with `unit` elements per workgroup and iteration: ceil(n / unit) within [1, cap]
inline int wm_groups(size_t n, size_t unit, size_t cap) {
    const size_t g = (n + unit - 1) / unit;
    return (int)(g > cap ? cap : (g < 1 ? 1 : g));
}

// one workgroup: out[0] = scale * sum of the n partials (thread i adds partials i, i+256, ...; then block_sum_f64).  Launch only: the
// caller checks (reduce.hip)
void wm_sum_finalize(const double* partials, size_t n, double scale, float* out, hipStream_t stream);
