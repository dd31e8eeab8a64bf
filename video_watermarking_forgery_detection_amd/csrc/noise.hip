// Stochastic attack kernels on NCHW f32 planes (gfx950), forward + backward, with the random numbers drawn on the device.
//   drop      : per-element dropout against the cover    noise_layers/crop.py:136-147 (the Dropout noise_layers exports)
//   gauss     : clamp(x + N(mean, std), 0, 1)            noise_layers/gaussian.py:4-17
//   gn        : x + N(mean, sqrt(var))                   noise_layers/gaussian_noise.py:6-20
//   saltpepper: u > 1-p/2 -> 0, then u < p/2 -> 1        noise_layers/salt_pepper_noise.py:5-23
//   dropout   : one H x W keep mask shared over B and C  noise_layers/dropout.py:4-27
//
// Generator: Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11), a counter-based generator.  The
// draw for element index i of a call is a pure function of (seed, offset, i):
//     key = (seed lo, seed hi), counter = (lo(i/4), hi(i/4), offset lo, offset hi), element i takes word i%4 of the block,
// so it does not depend on the grid, the CU count or the stream, and a thread that owns four consecutive elements runs Philox once.
//   uniform: (word >> 8) * 2^-24 in [0,1)  (24-bit floats, exact)
//   normal : Box-Muller on the word pairs (0,1) and (2,3): u1 = ((w >> 8) + 1) * 2^-24 in (0,1] (log(0) cannot occur),
//            u2 = (w' >> 8) * 2^-24, r = sqrt(-2 log u1), element 4k+2j gets r cos(2 pi u2), 4k+2j+1 gets r sin(2 pi u2); accurate
//            logf / sincosf / sqrtf (the library is built without fast-math).
//
// State: a caller-owned device array of WM_RNG_STATE_WORDS 64-bit words {seed, offset, 0, 0}; the kernels read it through a pointer
// (a captured launch stays valid and draws fresh numbers at every replay).  A forward call first launches rng_reserve_kernel (one
// thread): it copies {seed, offset} of the state into the call's record `rec` and advances the state's offset by the counter blocks the
// call uses, in stream order.  The attack kernel then reads only `rec`, never the live state, so no workgroup can see a half-advanced
// state; the backward regenerates the same draws from the same `rec` (16 bytes per call, no mask stored).  (A reservation inside the
// attack kernel itself -- every workgroup reads the state, the last to take a ticket advances it -- costs one agent-scope fence and one
// same-address atomic per workgroup: 70 us instead of 10 us at 16x3x256x256 on MI355X.)
#include "wm_common.h"

namespace {

constexpr uint32_t PH_M0 = 0xD2511F53u, PH_M1 = 0xCD9E8D57u, PH_W0 = 0x9E3779B9u, PH_W1 = 0xBB67AE85u;

struct U4 { uint32_t v[4]; };

__device__ __forceinline__ U4 philox4x32_10(uint64_t q, uint64_t off, uint64_t seed) {
    uint32_t c0 = (uint32_t)q, c1 = (uint32_t)(q >> 32), c2 = (uint32_t)off, c3 = (uint32_t)(off >> 32);
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        if (r) { k0 += PH_W0; k1 += PH_W1; }
        const uint32_t hi0 = __umulhi(PH_M0, c0), lo0 = PH_M0 * c0;
        const uint32_t hi1 = __umulhi(PH_M1, c2), lo1 = PH_M1 * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
    }
    U4 o;
    o.v[0] = c0; o.v[1] = c1; o.v[2] = c2; o.v[3] = c3;
    return o;
}

__device__ __forceinline__ float u01(uint32_t w) { return (float)(w >> 8) * 0x1p-24f; }          // [0,1)
__device__ __forceinline__ float u01_open0(uint32_t w) { return (float)((w >> 8) + 1u) * 0x1p-24f; }  // (0,1]

template <int DIST>
__device__ __forceinline__ void draws4(uint64_t seed, uint64_t off, uint64_t q, float (&d)[4]) {
    const U4 w = philox4x32_10(q, off, seed);
    if (DIST == WM_RNG_UNIFORM) {
#pragma unroll
        for (int j = 0; j < 4; ++j) d[j] = u01(w.v[j]);
    } else {
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const float r = sqrtf(-2.0f * logf(u01_open0(w.v[2 * p])));
            float s, c;
            sincosf(6.28318530717958647692f * u01(w.v[2 * p + 1]), &s, &c);
            d[2 * p] = r * c;
            d[2 * p + 1] = r * s;
        }
    }
}

// the call's record {seed, offset} and the state's advance, in stream order before the attack kernel
__global__ void rng_reserve_kernel(unsigned long long* state, unsigned long long* rec, unsigned reserve) {
    const unsigned long long sd = state[0], o = state[1];
    rec[0] = sd;
    rec[1] = o;
    state[1] = o + reserve;
}

// ---- per-element attacks: a thread owns elements 4q .. 4q+3 of the flat tensor (one Philox block)
template <int OP> struct ElemOp;
template <> struct ElemOp<WM_NOISE_DROP> {            // where(u > prob, cover, image); a = prob
    static constexpr int DIST = WM_RNG_UNIFORM;
    __device__ static float fwd(float x, float c, float d, float a, float) { return d > a ? c : x; }
    __device__ static float bwd(float, float g, float d, float a, float) { return d > a ? 0.f : g; }
};
template <> struct ElemOp<WM_NOISE_GAUSS> {           // clamp(x + (mean + std n), 0, 1); a = mean, b = std
    static constexpr int DIST = WM_RNG_NORMAL;
    __device__ static float fwd(float x, float, float d, float a, float b) {
        const float s = x + __builtin_fmaf(b, d, a);
        return s < 0.f ? 0.f : (s > 1.f ? 1.f : s);    // NaN passes through, as torch.clamp
    }
    __device__ static float bwd(float x, float g, float d, float a, float b) {
        const float s = x + __builtin_fmaf(b, d, a);
        return (s >= 0.f && s <= 1.f) ? g : 0.f;       // torch's clamp backward: the gradient passes where min <= s <= max
    }
};
template <> struct ElemOp<WM_NOISE_GN> {              // x + (mean + sd n); a = mean, b = sd.  Backward: the identity (no launch)
    static constexpr int DIST = WM_RNG_NORMAL;
    __device__ static float fwd(float x, float, float d, float a, float b) { return x + __builtin_fmaf(b, d, a); }
    __device__ static float bwd(float, float g, float, float, float) { return g; }
};
template <> struct ElemOp<WM_NOISE_SP> {              // a = prob/2, b = 1 - prob/2 (f32, as torch compares an f32 tensor with them)
    static constexpr int DIST = WM_RNG_UNIFORM;
    __device__ static float fwd(float x, float, float d, float a, float b) {
        const float o = d > b ? 0.f : x;
        return d < a ? 1.f : o;
    }
    __device__ static float bwd(float, float g, float d, float a, float b) { return (d > b || d < a) ? 0.f : g; }
};

template <int OP>
__global__ __launch_bounds__(256) void noise_fwd_kernel(const float* __restrict__ x, const float* __restrict__ cover,
                                                        float* __restrict__ y, size_t n, float a, float b, int vec,
                                                        const unsigned long long* __restrict__ rec) {
    const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x, i0 = q * 4;
    if (i0 >= n) return;
    const uint64_t seed = rec[0], off = rec[1];
    float d[4];
    draws4<ElemOp<OP>::DIST>(seed, off, q, d);
    if (vec && i0 + 4 <= n) {
        const float4 xv = *reinterpret_cast<const float4*>(x + i0);
        const float4 cv = cover ? *reinterpret_cast<const float4*>(cover + i0) : make_float4(0.f, 0.f, 0.f, 0.f);
        float4 o;
        o.x = ElemOp<OP>::fwd(xv.x, cv.x, d[0], a, b);
        o.y = ElemOp<OP>::fwd(xv.y, cv.y, d[1], a, b);
        o.z = ElemOp<OP>::fwd(xv.z, cv.z, d[2], a, b);
        o.w = ElemOp<OP>::fwd(xv.w, cv.w, d[3], a, b);
        *reinterpret_cast<float4*>(y + i0) = o;
        return;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (i0 + j < n) y[i0 + j] = ElemOp<OP>::fwd(x[i0 + j], cover ? cover[i0 + j] : 0.f, d[j], a, b);
}

// gx = d out / d image . g; gc (WM_NOISE_DROP only, may be NULL) = d out / d cover . g.  x is read by WM_NOISE_GAUSS only
template <int OP>
__global__ __launch_bounds__(256) void noise_bwd_kernel(const float* __restrict__ x, const float* __restrict__ g, float* __restrict__ gx,
                                                        float* __restrict__ gc, size_t n, float a, float b, int vec,
                                                        const unsigned long long* __restrict__ rec) {
    const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x, i0 = q * 4;
    if (i0 >= n) return;
    const uint64_t seed = rec[0], off = rec[1];
    float d[4];
    draws4<ElemOp<OP>::DIST>(seed, off, q, d);
    constexpr bool NX = OP == WM_NOISE_GAUSS;
    if (vec && i0 + 4 <= n) {
        const float4 gv = *reinterpret_cast<const float4*>(g + i0);
        const float4 xv = NX ? *reinterpret_cast<const float4*>(x + i0) : make_float4(0.f, 0.f, 0.f, 0.f);
        float4 o;
        o.x = ElemOp<OP>::bwd(xv.x, gv.x, d[0], a, b);
        o.y = ElemOp<OP>::bwd(xv.y, gv.y, d[1], a, b);
        o.z = ElemOp<OP>::bwd(xv.z, gv.z, d[2], a, b);
        o.w = ElemOp<OP>::bwd(xv.w, gv.w, d[3], a, b);
        *reinterpret_cast<float4*>(gx + i0) = o;
        if (OP == WM_NOISE_DROP && gc) {
            *reinterpret_cast<float4*>(gc + i0) = make_float4(d[0] > a ? gv.x : 0.f, d[1] > a ? gv.y : 0.f, d[2] > a ? gv.z : 0.f,
                                                              d[3] > a ? gv.w : 0.f);
        }
        return;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (i0 + j >= n) break;
        const float gi = ElemOp<OP>::bwd(NX ? x[i0 + j] : 0.f, g[i0 + j], d[j], a, b);
        gx[i0 + j] = gi;
        if (OP == WM_NOISE_DROP && gc) gc[i0 + j] = d[j] > a ? g[i0 + j] : 0.f;
    }
}

// ---- dropout.Dropout: keep = keep_min + span * u (counter block 0 at `offset`), mask m = [u < keep] over the H x W plane (counters at
// offset + 1), shared by the N = B*C planes; out = x*m + cover*(1-m).  grid = (pixel groups of 4 / 256, planes)
__device__ __forceinline__ void dropout_mask4(uint64_t seed, uint64_t off, uint64_t q, float kmin, float span, float (&m)[4]) {
    const float keep = __builtin_fmaf(span, u01(philox4x32_10(0, off, seed).v[0]), kmin);
    const U4 w = philox4x32_10(q, off + 1, seed);
#pragma unroll
    for (int j = 0; j < 4; ++j) m[j] = u01(w.v[j]) < keep ? 1.f : 0.f;
}

__global__ __launch_bounds__(256) void dropout_fwd_kernel(const float* __restrict__ x, const float* __restrict__ cover, float* __restrict__ y,
                                                          int N, int HW, float kmin, float span, int vec,
                                                          const unsigned long long* __restrict__ rec) {
    const int q = blockIdx.x * 256 + threadIdx.x, p0 = q * 4;
    if (p0 >= HW) return;
    float m[4];
    dropout_mask4(rec[0], rec[1], (uint64_t)q, kmin, span, m);
    for (int n = blockIdx.y; n < N; n += gridDim.y) {
        const size_t base = (size_t)n * HW + p0;
        if (vec && p0 + 4 <= HW) {
            const float4 xv = *reinterpret_cast<const float4*>(x + base), cv = *reinterpret_cast<const float4*>(cover + base);
            float4 o;
            o.x = xv.x * m[0] + cv.x * (1.f - m[0]);
            o.y = xv.y * m[1] + cv.y * (1.f - m[1]);
            o.z = xv.z * m[2] + cv.z * (1.f - m[2]);
            o.w = xv.w * m[3] + cv.w * (1.f - m[3]);
            *reinterpret_cast<float4*>(y + base) = o;
            continue;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (p0 + j < HW) y[base + j] = x[base + j] * m[j] + cover[base + j] * (1.f - m[j]);
    }
}

__global__ __launch_bounds__(256) void dropout_bwd_kernel(const float* __restrict__ g, float* __restrict__ gx, float* __restrict__ gc, int N,
                                                          int HW, float kmin, float span, int vec, const unsigned long long* __restrict__ rec) {
    const int q = blockIdx.x * 256 + threadIdx.x, p0 = q * 4;
    if (p0 >= HW) return;
    float m[4];
    dropout_mask4(rec[0], rec[1], (uint64_t)q, kmin, span, m);
    for (int n = blockIdx.y; n < N; n += gridDim.y) {
        const size_t base = (size_t)n * HW + p0;
        if (vec && p0 + 4 <= HW) {
            const float4 gv = *reinterpret_cast<const float4*>(g + base);
            *reinterpret_cast<float4*>(gx + base) = make_float4(gv.x * m[0], gv.y * m[1], gv.z * m[2], gv.w * m[3]);
            if (gc)
                *reinterpret_cast<float4*>(gc + base) =
                    make_float4(gv.x * (1.f - m[0]), gv.y * (1.f - m[1]), gv.z * (1.f - m[2]), gv.w * (1.f - m[3]));
            continue;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (p0 + j >= HW) break;
            gx[base + j] = g[base + j] * m[j];
            if (gc) gc[base + j] = g[base + j] * (1.f - m[j]);
        }
    }
}

// ---- the test entry point: out[i] = draw i of the stream at (seed, offset) = state[0], state[1]; the state is only read
template <int DIST>
__global__ __launch_bounds__(256) void rng_fill_kernel(const unsigned long long* __restrict__ state, float* __restrict__ out, size_t n) {
    const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x, i0 = q * 4;
    if (i0 >= n) return;
    float d[4];
    draws4<DIST>(state[0], state[1], q, d);
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (i0 + j < n) out[i0 + j] = d[j];
}

inline bool al16(const void* p) { return p == nullptr || ((uintptr_t)p & 15u) == 0; }

inline unsigned groups_grid(size_t n) { return (unsigned)(((n + 3) / 4 + 255) / 256); }

}  // namespace

extern "C" int wm_rng_fill(const void* state, float* out, size_t n, int dist, void* stream) {
    WM_REQUIRE(state && out && n > 0 && (dist == WM_RNG_UNIFORM || dist == WM_RNG_NORMAL), WM_E_BADARG, "wm_rng_fill: bad arguments");
    WM_REQUIRE((n + 3) / 4 <= (size_t)0x7fffffff * 256, WM_E_SHAPE, "wm_rng_fill: n too large");
    const auto* st = static_cast<const unsigned long long*>(state);
    if (dist == WM_RNG_UNIFORM)
        hipLaunchKernelGGL(rng_fill_kernel<WM_RNG_UNIFORM>, dim3(groups_grid(n)), dim3(256), 0, (hipStream_t)stream, st, out, n);
    else
        hipLaunchKernelGGL(rng_fill_kernel<WM_RNG_NORMAL>, dim3(groups_grid(n)), dim3(256), 0, (hipStream_t)stream, st, out, n);
    WM_LAUNCH_CHECK("wm_rng_fill");
    return WM_OK;
}

extern "C" int wm_noise_fwd(int op, const float* x, const float* cover, float* y, size_t n, float a, float b, void* state, void* rec,
                            void* stream) {
    WM_REQUIRE(x && y && state && rec && n > 0, WM_E_BADARG, "wm_noise_fwd: bad arguments");
    WM_REQUIRE(op != WM_NOISE_DROP || cover, WM_E_BADARG, "wm_noise_fwd: WM_NOISE_DROP needs the cover");
    WM_REQUIRE((n + 3) / 4 <= (size_t)0x7fffffff * 256, WM_E_SHAPE, "wm_noise_fwd: n too large");
    const int vec = al16(x) && al16(cover) && al16(y);
    WM_REQUIRE(op >= WM_NOISE_DROP && op <= WM_NOISE_SP, WM_E_BADARG, "wm_noise_fwd: unknown op %d", op);
    auto* rc = static_cast<unsigned long long*>(rec);
    const dim3 grid(groups_grid(n)), blk(256);
    const hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(rng_reserve_kernel, dim3(1), dim3(1), 0, s, static_cast<unsigned long long*>(state), rc, 1u);
    switch (op) {
        case WM_NOISE_DROP: hipLaunchKernelGGL(noise_fwd_kernel<WM_NOISE_DROP>, grid, blk, 0, s, x, cover, y, n, a, b, vec, rc); break;
        case WM_NOISE_GAUSS: hipLaunchKernelGGL(noise_fwd_kernel<WM_NOISE_GAUSS>, grid, blk, 0, s, x, nullptr, y, n, a, b, vec, rc); break;
        case WM_NOISE_GN: hipLaunchKernelGGL(noise_fwd_kernel<WM_NOISE_GN>, grid, blk, 0, s, x, nullptr, y, n, a, b, vec, rc); break;
        default: hipLaunchKernelGGL(noise_fwd_kernel<WM_NOISE_SP>, grid, blk, 0, s, x, nullptr, y, n, a, b, vec, rc); break;
    }
    WM_LAUNCH_CHECK("wm_noise_fwd");
    return WM_OK;
}

extern "C" int wm_noise_bwd(int op, const float* x, const float* g, float* gx, float* gcover, size_t n, float a, float b, const void* rec,
                            void* stream) {
    WM_REQUIRE(g && gx && rec && n > 0, WM_E_BADARG, "wm_noise_bwd: bad arguments");
    WM_REQUIRE(op != WM_NOISE_GAUSS || x, WM_E_BADARG, "wm_noise_bwd: WM_NOISE_GAUSS needs the forward's input");
    WM_REQUIRE((n + 3) / 4 <= (size_t)0x7fffffff * 256, WM_E_SHAPE, "wm_noise_bwd: n too large");
    const int vec = al16(x) && al16(g) && al16(gx) && al16(gcover);
    const auto* rc = static_cast<const unsigned long long*>(rec);
    const dim3 grid(groups_grid(n)), blk(256);
    const hipStream_t s = (hipStream_t)stream;
    switch (op) {
        case WM_NOISE_DROP: hipLaunchKernelGGL(noise_bwd_kernel<WM_NOISE_DROP>, grid, blk, 0, s, nullptr, g, gx, gcover, n, a, b, vec, rc); break;
        case WM_NOISE_GAUSS: hipLaunchKernelGGL(noise_bwd_kernel<WM_NOISE_GAUSS>, grid, blk, 0, s, x, g, gx, nullptr, n, a, b, vec, rc); break;
        case WM_NOISE_SP: hipLaunchKernelGGL(noise_bwd_kernel<WM_NOISE_SP>, grid, blk, 0, s, nullptr, g, gx, nullptr, n, a, b, vec, rc); break;
        default: WM_REQUIRE(false, WM_E_BADARG, "wm_noise_bwd: op %d has no backward kernel", op);
    }
    WM_LAUNCH_CHECK("wm_noise_bwd");
    return WM_OK;
}

extern "C" int wm_dropout_fwd(const float* x, const float* cover, float* y, int N, int H, int W, float keep_min, float keep_span,
                              void* state, void* rec, void* stream) {
    WM_REQUIRE(x && cover && y && state && rec && N > 0 && H > 0 && W > 0, WM_E_BADARG, "wm_dropout_fwd: bad arguments");
    WM_REQUIRE((long)H * W < (1l << 30), WM_E_SHAPE, "wm_dropout_fwd: plane too large");
    const int HW = H * W;
    const int vec = al16(x) && al16(cover) && al16(y) && HW % 4 == 0;
    const dim3 grid((unsigned)((HW + 1023) / 1024), (unsigned)(N < 65535 ? N : 65535));
    auto* rc = static_cast<unsigned long long*>(rec);
    hipLaunchKernelGGL(rng_reserve_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, static_cast<unsigned long long*>(state), rc, 2u);
    hipLaunchKernelGGL(dropout_fwd_kernel, grid, dim3(256), 0, (hipStream_t)stream, x, cover, y, N, HW, keep_min, keep_span, vec, rc);
    WM_LAUNCH_CHECK("wm_dropout_fwd");
    return WM_OK;
}

extern "C" int wm_dropout_bwd(const float* g, float* gx, float* gcover, int N, int H, int W, float keep_min, float keep_span,
                              const void* rec, void* stream) {
    WM_REQUIRE(g && gx && rec && N > 0 && H > 0 && W > 0, WM_E_BADARG, "wm_dropout_bwd: bad arguments");
    WM_REQUIRE((long)H * W < (1l << 30), WM_E_SHAPE, "wm_dropout_bwd: plane too large");
    const int HW = H * W;
    const int vec = al16(g) && al16(gx) && al16(gcover) && HW % 4 == 0;
    const dim3 grid((unsigned)((HW + 1023) / 1024), (unsigned)(N < 65535 ? N : 65535));
    hipLaunchKernelGGL(dropout_bwd_kernel, grid, dim3(256), 0, (hipStream_t)stream, g, gx, gcover, N, HW, keep_min, keep_span, vec,
                       static_cast<const unsigned long long*>(rec));
    WM_LAUNCH_CHECK("wm_dropout_bwd");
    return WM_OK;
}
