// nn.ReflectionPad2d(p) on NHWC activations and its adjoint (networks.py:1387-1421 ResnetBlock pads with it before both of its valid 3x3
// convolutions): x [B,H,W,CP] -> out [B,H+2p,W+2p,CP], the edge pixel not repeated, p <= min(H, W) - 1; f32 / bf16 / f16.
// Both directions are GATHERS of 16-byte channel vectors (CP a multiple of 4 f32 / 8 16-bit elements), one read and one write of the larger tensor:
//   forward : out[b, y, x, :] = in[b, r(y - p, H), r(x - p, W), :],  r(i, n) = i < 0 ? -i : (i >= n ? 2 (n - 1) - i : i)
//   backward: along an axis of length n the input index i receives from the padded positions i + p (itself), p - i (the low mirror, when
//             1 <= i <= p) and 2 (n - 1) - i + p (the high mirror, when n - 1 - p <= i <= n - 2): at most 3 x 3 = 9 terms per pixel, added in
//             f32 in that fixed order (rows outer, columns inner) and rounded once to the dtype.  No atomics: two runs agree bit for bit.
#include "wm_common.h"

namespace {

__device__ __forceinline__ int reflect(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * (n - 1) - i : i); }

// the padded positions that input index i of an axis of length n feeds; returns their number (1..3)
__device__ __forceinline__ int sources(int i, int n, int p, int* s) {
    int k = 0;
    s[k++] = i + p;
    if (i >= 1 && i <= p) s[k++] = p - i;
    if (i >= n - 1 - p && i <= n - 2) s[k++] = 2 * (n - 1) - i + p;
    return k;
}

// a thread per 16-byte vector of the OUTPUT, grid-stride
template <typename T>
__global__ __launch_bounds__(256) void reflect_pad_fwd_kernel(const T* __restrict__ x, T* __restrict__ out, int B, int H, int W, int CP, int p) {
    constexpr int VE = 16 / sizeof(T);
    const int nv = CP / VE, OH = H + 2 * p, OW = W + 2 * p;
    const size_t total = (size_t)B * OH * OW * nv;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int v = (int)(i % nv);
        size_t pix = i / nv;
        const int ox = (int)(pix % OW); pix /= OW;
        const int oy = (int)(pix % OH);
        const int b = (int)(pix / OH);
        const int sy = reflect(oy - p, H), sx = reflect(ox - p, W);
        const vec16<T> t = *reinterpret_cast<const vec16<T>*>(x + (((size_t)b * H + sy) * W + sx) * CP + (size_t)v * VE);
        *reinterpret_cast<vec16<T>*>(out + i * VE) = t;
    }
}

// a thread per 16-byte vector of the INPUT gradient, grid-stride
template <typename T>
__global__ __launch_bounds__(256) void reflect_pad_bwd_kernel(const T* __restrict__ g, T* __restrict__ gx, int B, int H, int W, int CP, int p) {
    constexpr int VE = 16 / sizeof(T);
    const int nv = CP / VE, OH = H + 2 * p, OW = W + 2 * p;
    const size_t total = (size_t)B * H * W * nv;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int v = (int)(i % nv);
        size_t pix = i / nv;
        const int ix = (int)(pix % W); pix /= W;
        const int iy = (int)(pix % H);
        const int b = (int)(pix / H);
        int ys[3], xs[3];
        const int ny = sources(iy, H, p, ys), nx = sources(ix, W, p, xs);
        float acc[VE];
#pragma unroll
        for (int e = 0; e < VE; ++e) acc[e] = 0.f;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            if (a < ny) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    if (c < nx) {
                        const vec16<T> t = *reinterpret_cast<const vec16<T>*>(g + (((size_t)b * OH + ys[a]) * OW + xs[c]) * CP + (size_t)v * VE);
#pragma unroll
                        for (int e = 0; e < VE; ++e) acc[e] += t.get(e);
                    }
                }
            }
        }
        vec16<T> o;
#pragma unroll
        for (int e = 0; e < VE; ++e) o.set(e, acc[e]);
        *reinterpret_cast<vec16<T>*>(gx + i * VE) = o;
    }
}

inline int pad_grid(size_t nvec) {   // memory-bound: at most 2048 workgroups, the rest by the grid-stride loop
    const size_t g = (nvec + 255) / 256;
    return (int)(g > 2048 ? 2048 : (g < 1 ? 1 : g));
}

int check_pad(const char* name, const void* a, const void* b, int B, int H, int W, int CP, int pad, int dtype) {
    WM_REQUIRE(a && b && B > 0 && H > 0 && W > 0 && CP > 0, WM_E_BADARG, "%s: bad arguments", name);
    WM_REQUIRE(dtype == WM_F32 || dtype == WM_BF16 || dtype == WM_F16, WM_E_BADARG, "%s: unsupported dtype %d", name, dtype);
    const int ve = dtype == WM_F32 ? 4 : 8;
    WM_REQUIRE(CP % ve == 0, WM_E_SHAPE, "%s: the channel stride %d must be a multiple of %d (16-byte vectors)", name, CP, ve);
    WM_REQUIRE(pad >= 0 && pad <= H - 1 && pad <= W - 1, WM_E_SHAPE, "%s: reflection pad %d needs min(H, W) - 1 >= pad, got %dx%d", name, pad, H, W);
    WM_REQUIRE((((uintptr_t)a | (uintptr_t)b) & 15) == 0, WM_E_SHAPE, "%s: pointers must be 16-byte aligned", name);
    return WM_OK;
}

}  // namespace

extern "C" int wm_reflect_pad_fwd(const void* x, void* out, int B, int H, int W, int CP, int pad, int dtype, void* stream) {
    int rc = check_pad("wm_reflect_pad_fwd", x, out, B, H, W, CP, pad, dtype);
    if (rc) return rc;
    WM_DISPATCH_DTYPE(dtype, "wm_reflect_pad_fwd", {
        const size_t nvec = (size_t)B * (H + 2 * pad) * (W + 2 * pad) * (CP / (16 / sizeof(T)));
        hipLaunchKernelGGL(reflect_pad_fwd_kernel<T>, dim3(pad_grid(nvec)), dim3(256), 0, (hipStream_t)stream, (const T*)x, (T*)out, B, H, W, CP, pad);
    });
    WM_LAUNCH_CHECK("wm_reflect_pad_fwd");
    return WM_OK;
}

extern "C" int wm_reflect_pad_bwd(const void* g, void* gx, int B, int H, int W, int CP, int pad, int dtype, void* stream) {
    int rc = check_pad("wm_reflect_pad_bwd", g, gx, B, H, W, CP, pad, dtype);
    if (rc) return rc;
    WM_DISPATCH_DTYPE(dtype, "wm_reflect_pad_bwd", {
        const size_t nvec = (size_t)B * H * W * (CP / (16 / sizeof(T)));
        hipLaunchKernelGGL(reflect_pad_bwd_kernel<T>, dim3(pad_grid(nvec)), dim3(256), 0, (hipStream_t)stream, (const T*)g, (T*)gx, B, H, W, CP, pad);
    });
    WM_LAUNCH_CHECK("wm_reflect_pad_bwd");
    return WM_OK;
}
