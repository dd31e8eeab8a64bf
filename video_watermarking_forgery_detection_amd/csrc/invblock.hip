// InvBlockExp, the coupling of the reference's rescaling generator (models/modules/Inv_arch.py:55-88), without its three subnets:
//   rev 0:  y1 = x1 + F(x2);  s = clamp * (2 sigmoid(H(y1)) - 1);  y2 = x2 * exp(s) + G(y1);  out = cat(y1, y2)
//   rev 1:  s = clamp * (2 sigmoid(H(x1)) - 1);  y2 = (x2 - G(x1)) / exp(s);  y1 = x1 - F(y2);  out = cat(y1, y2)
//   jacobian: +- sum(s) / B (:82-88)
// as two launches each way beside the subnets (composed from chan_slice / add / coupling / chan_cat it is five, with four intermediate
// tensors, and has no place for sum(s)):
//   wm_invblock_shift   v = x[:, :n1] + sign * f              alone (y1, the input of H and G) or as cat(v, other) (the reverse's block output)
//   wm_invblock_affine  v = x[:, n1:] * e + g or (.. - g) / e  as cat(other, v) (the forward's block output) or alone (y2, the input of F);
//                       optionally jac[b] = sum of s over sample b
// and their backward kernels.  x is read in place through its stride: x1 = channels [0, n1), x2 = channels [n1, n1 + n2).
// NHWC tensors of dtype T (f32 / bf16 / f16), f32 arithmetic, every channel stride a multiple of 16, padding channels of every output
// written as zero, padding channels of an input never used.  exp(s) is coupling_e's expression (inn.hip) with eps = 0.
//
// Every kernel walks the channels of its widest output in 16-byte vectors (VEC) or one by one (a base pointer off a 16-byte boundary).  An
// operand whose channels line up with that walk (its shift is a multiple of the vector) is loaded / stored as vectors; one that sits n1
// channels off it -- n1 = 3 in every network of the reference -- element by element.  Both paths do the same arithmetic: the same bits.
#include "wm_common.h"
#include "wm_reduce.h"

namespace {

inline int grid1(size_t n, int cap = 8192) {
    const size_t g = (n + 255) / 256;
    return (int)(g > (size_t)cap ? cap : (g < 1 ? 1 : g));
}
inline int cpad16(int c) { return (c + 15) / 16 * 16; }
inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// an operand as the walk sees it: walk channel c in [lo, hi) is element p[pixel * stride + c + shift]; any other channel reads as 0
struct Win { const void* p; int stride, shift, lo, hi; };
inline Win win(const void* p, int stride, int shift, int lo, int hi) { Win w; w.p = p; w.stride = stride; w.shift = shift; w.lo = lo; w.hi = hi; return w; }

template <typename T, int VE> __device__ __forceinline__ void ld_win(const Win& w, size_t pix, int c0, float (&v)[VE]) {
#pragma unroll
    for (int e = 0; e < VE; ++e) v[e] = 0.f;
    if (!w.p || c0 + VE <= w.lo || c0 >= w.hi) return;
    const T* row = (const T*)w.p + pix * w.stride;
    const int i0 = c0 + w.shift;
    if (VE > 1 && w.shift % VE == 0 && i0 >= 0 && i0 + VE <= w.stride) {
        vec16<T> q;
        q.v = *reinterpret_cast<const decltype(q.v)*>(row + i0);     // (may cover padding channels: masked below)
#pragma unroll
        for (int e = 0; e < VE; ++e)
            if (c0 + e >= w.lo && c0 + e < w.hi) v[e] = q.get(e);
    } else {
#pragma unroll
        for (int e = 0; e < VE; ++e)
            if (c0 + e >= w.lo && c0 + e < w.hi) v[e] = to_f32(row[i0 + e]);
    }
}
// the f32 result as it is stored: the value is pinned in a register before its conversion, so the compiler cannot merge the conversion
// with the operation before it.  For f16 it otherwise may (v_fma_mixlo_f16: the product rounded to f16 once, not to f32 and then to f16),
// and it did so in the element-wise instantiation of affine_bwd_kernel only: the two paths' gh then differed in a last bit
__device__ __forceinline__ float pinned(float v) {
    asm volatile("" : "+v"(v));
    return v;
}
// dst: the first of VE consecutive elements, 16-byte aligned when VE > 1
template <typename T, int VE> __device__ __forceinline__ void st_run(T* dst, const float (&v)[VE]) {
    if constexpr (VE > 1) {
        vec16<T> q;
#pragma unroll
        for (int e = 0; e < VE; ++e) q.set(e, pinned(v[e]));
        *reinterpret_cast<decltype(q.v)*>(dst) = q.v;
    } else {
        dst[0] = from_f32<T>(pinned(v[0]));
    }
}

// s = clamp * (2 sigmoid(h) - 1) and exp(s): coupling_e's expression
__device__ __forceinline__ float coupling_s(float h, float clamp) { return clamp * (2.f / (1.f + expf(-h)) - 1.f); }

// ---- shift.  out [npix][ostride]: channel c < n1 = x + sign * f, c in [n1, n1 + n2) = other (whole form), zero elsewhere
struct ShiftArgs { Win x, f, other; void* out; size_t npix; int ostride, n1; float sign; };
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void shift_fwd_kernel(ShiftArgs a) {
    constexpr int VE = VEC ? 16 / (int)sizeof(T) : 1;
    const int per = a.ostride / VE;
    const size_t total = a.npix * per;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int c0 = (int)(i % per) * VE;
        const size_t pix = i / per;
        float xv[VE], fv[VE], ov[VE], r[VE];
        ld_win<T, VE>(a.x, pix, c0, xv);
        ld_win<T, VE>(a.f, pix, c0, fv);
        ld_win<T, VE>(a.other, pix, c0, ov);
#pragma unroll
        for (int e = 0; e < VE; ++e) r[e] = c0 + e < a.n1 ? xv[e] + a.sign * fv[e] : ov[e];
        st_run<T, VE>((T*)a.out + pix * a.ostride + c0, r);
    }
}
// g = dL/dout [npix][g.stride].  gx [npix][gxs] = g in channels < n1, zero elsewhere; gf [npix][cp1] = sign * g; gother [npix][cp2] =
// g's channels [n1, n1 + n2) (whole form).  Walk: the channels of gx
struct ShiftBwdArgs { Win g; void* gx; void* gf; void* gother; size_t npix; int gxs, cp1, cp2, n1, n2; float sign; };
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void shift_bwd_kernel(ShiftBwdArgs a) {
    constexpr int VE = VEC ? 16 / (int)sizeof(T) : 1;
    const int per = a.gxs / VE;
    const size_t total = a.npix * per;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int c0 = (int)(i % per) * VE;
        const size_t pix = i / per;
        float gv[VE], r[VE];
        ld_win<T, VE>(a.g, pix, c0, gv);
#pragma unroll
        for (int e = 0; e < VE; ++e) r[e] = c0 + e < a.n1 ? gv[e] : 0.f;
        st_run<T, VE>((T*)a.gx + pix * a.gxs + c0, r);
        if (c0 < a.cp1) {
#pragma unroll
            for (int e = 0; e < VE; ++e) r[e] = c0 + e < a.n1 ? a.sign * gv[e] : 0.f;
            st_run<T, VE>((T*)a.gf + pix * a.cp1 + c0, r);
        }
        if (a.gother) {
            T* q = (T*)a.gother + pix * a.cp2;
#pragma unroll
            for (int e = 0; e < VE; ++e) {
                const int c = c0 + e, j = c < a.n1 ? a.gxs - a.n1 + c : c - a.n1;     // (channels < n1 zero what the walk's end leaves of the padding)
                if (j < a.cp2) q[j] = from_f32<T>(pinned(c >= a.n1 && j < a.n2 ? gv[e] : 0.f));
            }
        }
    }
}

// ---- affine.  out [B * hw][ostride]: channel c in [vo, vo + n2) = v(c - vo), c < n1 = other (whole form: vo = n1), zero elsewhere.
// grid (P, B): workgroup (j, b) takes its grid-stride share of sample b; JAC: -> partials[b * P + j] = its sum of s, in double
struct AffArgs { Win x, h, g, other; void* out; double* partials; size_t hw; int ostride, vo, n2, rev; float clamp; };
template <typename T, bool VEC, bool JAC>
__global__ __launch_bounds__(256) void affine_fwd_kernel(AffArgs a) {
    constexpr int VE = VEC ? 16 / (int)sizeof(T) : 1;
    const int per = a.ostride / VE;
    const size_t total = a.hw * per, pix0 = (size_t)blockIdx.y * a.hw;
    double acc = 0.0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int c0 = (int)(i % per) * VE;
        const size_t pix = pix0 + i / per;
        float xv[VE], hv[VE], gv[VE], ov[VE], r[VE];
        ld_win<T, VE>(a.x, pix, c0, xv);
        ld_win<T, VE>(a.h, pix, c0, hv);
        ld_win<T, VE>(a.g, pix, c0, gv);
        ld_win<T, VE>(a.other, pix, c0, ov);
#pragma unroll
        for (int e = 0; e < VE; ++e) {
            const int c = c0 + e;
            if (c >= a.vo && c < a.vo + a.n2) {
                const float s = coupling_s(hv[e], a.clamp), ex = expf(s);
                r[e] = a.rev ? (xv[e] - gv[e]) / ex : ex * xv[e] + gv[e];
                if (JAC) acc += (double)s;
            } else {
                r[e] = ov[e];
            }
        }
        st_run<T, VE>((T*)a.out + pix * a.ostride + c0, r);
    }
    if (JAC) {
        __shared__ double sh[4];
        acc = block_sum_f64(acc, sh);
        if (threadIdx.x == 0) a.partials[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = acc;
    }
}
// one workgroup: wave w sums the P <= 64 partials of samples w, w + 4, ... (lane j holds partial j: a fixed butterfly) -> jac[b]
__global__ __launch_bounds__(256) void jac_finalize_kernel(const double* __restrict__ partials, int B, int P, float* __restrict__ jac) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int b = w; b < B; b += 4) {
        double v = lane < P ? partials[(size_t)b * P + lane] : 0.0;
        v = wave_sum_f64(v);
        if (lane == 0) jac[b] = (float)v;
    }
}

// go = dL/dout (its v channels), v = x (rev 0) or the stored output (rev 1), both as windows over [n1, n1 + n2) of the walk = the
// channels of gx [npix][gxs].  gx = zero outside that window; gh, gg [npix][cp2]; gother [npix][cp1] = dL/dout's channels < n1 (whole form).
// The expressions are affine_bwd_kernel's (inn.hip) with eps = 0
struct AffBwdArgs { Win go, v, h, g1; void* gx; void* gh; void* gg; void* gother; size_t npix; int gxs, cp1, cp2, n1, n2, rev; float clamp; };
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void affine_bwd_kernel(AffBwdArgs a) {
    constexpr int VE = VEC ? 16 / (int)sizeof(T) : 1;
    const int per = a.gxs / VE;
    const size_t total = a.npix * per;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int c0 = (int)(i % per) * VE;
        const size_t pix = i / per;
        float gov[VE], vv[VE], hv[VE], rx[VE], rh[VE], rg[VE];
        ld_win<T, VE>(a.go, pix, c0, gov);
        ld_win<T, VE>(a.v, pix, c0, vv);
        ld_win<T, VE>(a.h, pix, c0, hv);
#pragma unroll
        for (int e = 0; e < VE; ++e) {
            const int c = c0 + e;
            rx[e] = 0.f; rh[e] = 0.f; rg[e] = 0.f;
            if (c >= a.n1 && c < a.n1 + a.n2) {
                const float sg = 1.f / (1.f + expf(-hv[e]));
                const float ex = expf(a.clamp * (2.f * sg - 1.f));
                const float de = ex * a.clamp * 2.f * sg * (1.f - sg);
                if (!a.rev) {
                    rx[e] = ex * gov[e];
                    rg[e] = gov[e];
                    rh[e] = gov[e] * vv[e] * de;
                } else {
                    const float ge = gov[e] / ex;
                    rx[e] = ge;
                    rg[e] = -ge;
                    rh[e] = -ge * vv[e] * de;
                }
            }
        }
        st_run<T, VE>((T*)a.gx + pix * a.gxs + c0, rx);
        T* qh = (T*)a.gh + pix * a.cp2;
        T* qg = (T*)a.gg + pix * a.cp2;
#pragma unroll
        for (int e = 0; e < VE; ++e) {
            const int c = c0 + e, j = c < a.n1 ? a.gxs - a.n1 + c : c - a.n1;     // (channels < n1 zero what the walk's end leaves of the padding)
            if (j < a.cp2) { qh[j] = from_f32<T>(pinned(rh[e])); qg[j] = from_f32<T>(pinned(rg[e])); }
        }
        if (a.gother && c0 < a.cp1) {
            float o[VE];
            ld_win<T, VE>(a.g1, pix, c0, o);
            st_run<T, VE>((T*)a.gother + pix * a.cp1 + c0, o);
        }
    }
}

inline int jac_parts(size_t hw, int ostride) { return wm_groups(hw * (size_t)ostride, 4096, 64); }

#define INVBLOCK_LAUNCH(KERNEL, vec, grid, s, args)                                                   \
    do {                                                                                              \
        if (vec) hipLaunchKernelGGL((KERNEL<T, true>), grid, dim3(256), 0, s, args);                  \
        else hipLaunchKernelGGL((KERNEL<T, false>), grid, dim3(256), 0, s, args);                     \
    } while (0)

}  // namespace

extern "C" int wm_invblock_shift(const void* x, int xstride, const void* f, const void* other, void* out, size_t npix, int n1, int n2, float sign,
                                 int dtype, void* stream) {
    WM_REQUIRE(x && f && out && npix > 0 && n1 > 0 && n2 > 0 && (sign == 1.f || sign == -1.f), WM_E_BADARG,
               "wm_invblock_shift: bad arguments (n1, n2 > 0, sign +-1)");
    WM_REQUIRE(xstride % 16 == 0 && n1 + n2 <= xstride, WM_E_BADARG, "wm_invblock_shift: channels [0,%d) outside x's stride %d (a multiple of 16)",
               n1 + n2, xstride);
    const int cp1 = cpad16(n1), cp2 = cpad16(n2);
    ShiftArgs a;
    a.x = win(x, xstride, 0, 0, n1);
    a.f = win(f, cp1, 0, 0, n1);
    a.other = win(other, cp2, -n1, n1, n1 + n2);
    a.out = out; a.npix = npix; a.ostride = other ? cpad16(n1 + n2) : cp1; a.n1 = n1; a.sign = sign;
    const bool vec = aligned16(x) && aligned16(f) && aligned16(other) && aligned16(out);
    hipStream_t s = (hipStream_t)stream;
    WM_DISPATCH_DTYPE(dtype, "wm_invblock_shift", {
        const size_t total = npix * (size_t)(vec ? a.ostride / (16 / (int)sizeof(T)) : a.ostride);
        INVBLOCK_LAUNCH(shift_fwd_kernel, vec, dim3(grid1(total)), s, a);
    });
    WM_LAUNCH_CHECK("wm_invblock_shift");
    return WM_OK;
}

extern "C" int wm_invblock_shift_bwd(const void* gout, int whole, void* gx, int gxstride, void* gf, void* gother, size_t npix, int n1, int n2,
                                     float sign, int dtype, void* stream) {
    WM_REQUIRE(gout && gx && gf && npix > 0 && n1 > 0 && n2 > 0 && (sign == 1.f || sign == -1.f) && (whole ? gother != nullptr : gother == nullptr),
               WM_E_BADARG, "wm_invblock_shift_bwd: bad arguments (n1, n2 > 0, sign +-1, gother with the whole form only)");
    WM_REQUIRE(gxstride % 16 == 0 && n1 + n2 <= gxstride, WM_E_BADARG,
               "wm_invblock_shift_bwd: channels [0,%d) outside gx's stride %d (a multiple of 16)", n1 + n2, gxstride);
    ShiftBwdArgs a;
    a.g = whole ? win(gout, cpad16(n1 + n2), 0, 0, n1 + n2) : win(gout, cpad16(n1), 0, 0, n1);
    a.gx = gx; a.gf = gf; a.gother = gother; a.npix = npix; a.gxs = gxstride; a.cp1 = cpad16(n1); a.cp2 = cpad16(n2); a.n1 = n1; a.n2 = n2;
    a.sign = sign;
    const bool vec = aligned16(gout) && aligned16(gx) && aligned16(gf);
    hipStream_t s = (hipStream_t)stream;
    WM_DISPATCH_DTYPE(dtype, "wm_invblock_shift_bwd", {
        const size_t total = npix * (size_t)(vec ? gxstride / (16 / (int)sizeof(T)) : gxstride);
        INVBLOCK_LAUNCH(shift_bwd_kernel, vec, dim3(grid1(total)), s, a);
    });
    WM_LAUNCH_CHECK("wm_invblock_shift_bwd");
    return WM_OK;
}

extern "C" size_t wm_invblock_scratch_doubles(int B, size_t hw, int n1, int n2) {
    if (B <= 0 || hw == 0 || n1 <= 0 || n2 <= 0) return 0;
    return (size_t)B * 64;      // at most 64 partials per sample, whichever form the call takes
}

extern "C" int wm_invblock_affine(const void* x, int xstride, const void* h, const void* g, const void* other, void* out, float* jac,
                                  double* scratch, int B, size_t hw, int n1, int n2, float clamp, int rev, int dtype, void* stream) {
    WM_REQUIRE(x && h && g && out && B > 0 && B <= 65535 && hw > 0 && n1 > 0 && n2 > 0 && (rev == 0 || rev == 1) && (!jac || scratch), WM_E_BADARG,
               "wm_invblock_affine: bad arguments (B <= 65535, n1, n2 > 0, rev 0 / 1, jac needs scratch)");
    WM_REQUIRE(xstride % 16 == 0 && n1 + n2 <= xstride, WM_E_BADARG, "wm_invblock_affine: channels [%d,%d) outside x's stride %d (a multiple of 16)",
               n1, n1 + n2, xstride);
    const int cp1 = cpad16(n1), cp2 = cpad16(n2), vo = other ? n1 : 0;
    AffArgs a;
    a.x = win(x, xstride, n1 - vo, vo, vo + n2);
    a.h = win(h, cp2, -vo, vo, vo + n2);
    a.g = win(g, cp2, -vo, vo, vo + n2);
    a.other = win(other, cp1, 0, 0, n1);
    a.out = out; a.partials = scratch; a.hw = hw; a.ostride = other ? cpad16(n1 + n2) : cp2; a.vo = vo; a.n2 = n2; a.rev = rev; a.clamp = clamp;
    const bool vec = aligned16(x) && aligned16(h) && aligned16(g) && aligned16(other) && aligned16(out);
    hipStream_t s = (hipStream_t)stream;
    const int P = jac_parts(hw, a.ostride);
    WM_DISPATCH_DTYPE(dtype, "wm_invblock_affine", {
        const size_t total = hw * (size_t)(vec ? a.ostride / (16 / (int)sizeof(T)) : a.ostride);
        if (jac) {
            const dim3 grid(P, B);
            if (vec) hipLaunchKernelGGL((affine_fwd_kernel<T, true, true>), grid, dim3(256), 0, s, a);
            else hipLaunchKernelGGL((affine_fwd_kernel<T, false, true>), grid, dim3(256), 0, s, a);
        } else {
            const dim3 grid(wm_groups(total, 256, 2048), B);
            if (vec) hipLaunchKernelGGL((affine_fwd_kernel<T, true, false>), grid, dim3(256), 0, s, a);
            else hipLaunchKernelGGL((affine_fwd_kernel<T, false, false>), grid, dim3(256), 0, s, a);
        }
    });
    WM_LAUNCH_CHECK("wm_invblock_affine");
    if (jac) {
        hipLaunchKernelGGL(jac_finalize_kernel, dim3(1), dim3(256), 0, s, (const double*)scratch, B, P, jac);
        WM_LAUNCH_CHECK("wm_invblock_affine (jac)");
    }
    return WM_OK;
}

extern "C" int wm_invblock_affine_bwd(const void* gout, int whole, const void* v, int vstride, int voff, const void* h, void* gx, int gxstride,
                                      void* gh, void* gg, void* gother, size_t npix, int n1, int n2, float clamp, int rev, int dtype,
                                      void* stream) {
    WM_REQUIRE(gout && v && h && gx && gh && gg && npix > 0 && n1 > 0 && n2 > 0 && (rev == 0 || rev == 1) &&
                   (whole ? gother != nullptr : gother == nullptr),
               WM_E_BADARG, "wm_invblock_affine_bwd: bad arguments (n1, n2 > 0, rev 0 / 1, gother with the whole form only)");
    WM_REQUIRE(gxstride % 16 == 0 && n1 + n2 <= gxstride, WM_E_BADARG,
               "wm_invblock_affine_bwd: channels [%d,%d) outside gx's stride %d (a multiple of 16)", n1, n1 + n2, gxstride);
    WM_REQUIRE(vstride % 16 == 0 && voff >= 0 && voff + n2 <= vstride, WM_E_BADARG,
               "wm_invblock_affine_bwd: channels [%d,%d) outside v's stride %d (a multiple of 16)", voff, voff + n2, vstride);
    const int cp1 = cpad16(n1), cp2 = cpad16(n2), cp = cpad16(n1 + n2);
    AffBwdArgs a;
    a.go = whole ? win(gout, cp, 0, n1, n1 + n2) : win(gout, cp2, -n1, n1, n1 + n2);
    a.v = win(v, vstride, voff - n1, n1, n1 + n2);
    a.h = win(h, cp2, -n1, n1, n1 + n2);
    a.g1 = win(whole ? gout : nullptr, cp, 0, 0, n1);
    a.gx = gx; a.gh = gh; a.gg = gg; a.gother = gother; a.npix = npix; a.gxs = gxstride; a.cp1 = cp1; a.cp2 = cp2; a.n1 = n1; a.n2 = n2;
    a.rev = rev; a.clamp = clamp;
    const bool vec = aligned16(gout) && aligned16(v) && aligned16(h) && aligned16(gx) && aligned16(gother);
    hipStream_t s = (hipStream_t)stream;
    WM_DISPATCH_DTYPE(dtype, "wm_invblock_affine_bwd", {
        const size_t total = npix * (size_t)(vec ? gxstride / (16 / (int)sizeof(T)) : gxstride);
        INVBLOCK_LAUNCH(affine_bwd_kernel, vec, dim3(grid1(total)), s, a);
    });
    WM_LAUNCH_CHECK("wm_invblock_affine_bwd");
    return WM_OK;
}
