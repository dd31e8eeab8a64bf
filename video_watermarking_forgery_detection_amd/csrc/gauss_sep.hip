// Separable k x k blur (k odd, 3..15) with a zero or a reflected border, and Cropout, on NCHW f32 planes (gfx950), forward + backward.
//   gauss_sep : noise_layers/gaussian_blur.py:44-56 at any kernel size (zero padding (k-1)/2) and noise_layers/gaussian_filter.py
//               (kornia GaussianBlur2d: reflected border); the 2-D weights are outer(taps, taps)
//   cropout   : noise_layers/crop.py:121-134 (image inside the rectangle, cover elsewhere)
//
// gauss_sep is ONE launch each way.  A workgroup of 256 threads owns a TH x TW = 32 x 64 output tile:
//   1. stage the tile and its halo of r = k/2 pixels, border already applied, in LDS: S[TH + 2r][SW];
//   2. row pass LDS -> LDS: Rw[row][c] = sum_j taps[j] * S[row][c + j], for the TH + 2r staged rows;
//   3. column pass LDS -> registers -> HBM: y[h][c] = sum_i taps[i] * Rw[h + i][c].
// Each sum is a chain of k fmaf from 0, taps left to right: that order is the contract the tests' bound model follows.
// The kernel is HBM-bound (one read and one write of the plane; a tile's halo is its neighbours' interior and comes from L2).  The tile is sized
// from that: 32 x 64 keeps a row of the tile at 256 B (four full 64-B global lines per row, one LDS bank row per Rw row, so the 16 lanes of a
// ds_read_b128 group read one contiguous bank row), at k = 15 the staged area is 1.75 x the tile and both arrays take 26.5 KB of LDS.  Workgroups
// per CU in flight to cover the HBM latency = the smaller of the LDS and the VGPR limit (a workgroup puts one wave on each SIMD): forward 8
// at k = 3 down to 5 at k = 15 (85 VGPRs), folded backward 7 down to 3 (135 VGPRs).  A larger tile would cut the L2 re-reads but not the HBM bytes.
// S columns start PADL = 8 pixels left of the tile, so a staged 16-byte vector is 16-byte aligned in LDS and -- where the plane's rows are
// (W % 4 == 0 and an aligned base) -- in global memory too: such vectors are fetched as float4, every other one element by element.  Both ways
// stage the same values and the arithmetic after staging is shared, so the two paths agree bit for bit.
//
// Backward = the exact transpose, in gather form (deterministic, no atomics).  Zero border: the forward with reversed taps.  Reflected
// border: with G = gy extended by zeros, Z(p) = sum_i rev[i] * G[p + i - r] is the gradient of the PADDED pixel p in [-r, n + r), and the
// padded pixels -q and 2(n-1) - q are copies of pixel q, so gx[q] = Z(q) + [1 <= q <= r] Z(-q) + [n-1-r <= q <= n-2] Z(2(n-1) - q), per axis
// (row axis first, then column axis; each Z a chain of k fmaf from 0, the fold terms added in that order).  Every G the fold terms read lies
// within r of the image border, hence inside the tile's staged halo.
#include "wm_common.h"

namespace {

constexpr int TH = 32, TW = 64, PADL = 8, SW = TW + 2 * PADL;
static_assert(PADL >= WM_GAUSS_SEP_MAX_K / 2 && PADL % 4 == 0, "the halo must fit the aligned padding");

struct Taps { float t[WM_GAUSS_SEP_MAX_K]; };

// index of the source pixel behind padded position p of an axis of n pixels, -1 for a zero
__device__ __forceinline__ int src_index(int p, int n, int r, int border) {
    if (p >= 0 && p < n) return p;
    if (border != WM_BORDER_REFLECT) return -1;
    if (p < 0) return p >= -r ? -p : -1;
    return p <= n - 1 + r ? 2 * (n - 1) - p : -1;
}

template <int K, bool FOLD>
__global__ __launch_bounds__(256) void gauss_sep_kernel(const float* __restrict__ x, float* __restrict__ y, int N, int H, int W, Taps tp,
                                                        int border, int vec_in, int vec_out) {
    constexpr int R = K / 2, ROWS = TH + 2 * R;
    // the row pass reads S through aligned 16-byte vectors: the first one at column A0, the tile's first tap O elements into it
    constexpr int A0 = ((PADL - R) / 4) * 4, O = (PADL - R) % 4, NV = (O + K + 3 + 3) / 4;
    static_assert(TW - 4 + A0 + NV * 4 <= SW, "row pass reads past the staged row");
    __shared__ __attribute__((aligned(16))) float S[ROWS * SW];
    __shared__ __attribute__((aligned(16))) float Rw[ROWS * TW];
    const int tid = threadIdx.x;
    const int w0 = blockIdx.x * TW, h0 = blockIdx.y * TH;

    for (int n = blockIdx.z; n < N; n += gridDim.z) {
        const float* px = x + (size_t)n * H * W;
        float* py = y + (size_t)n * H * W;
        // ---- 1. stage
        for (int it = tid; it < ROWS * (SW / 4); it += 256) {
            const int row = it / (SW / 4), q = it % (SW / 4);
            const int gr = src_index(h0 - R + row, H, R, border);
            const int gc0 = w0 - PADL + q * 4;
            float v[4] = {0.f, 0.f, 0.f, 0.f};
            if (gr >= 0 && gc0 + 3 >= w0 - R && gc0 < w0 + TW + R) {
                const float* rp = px + (size_t)gr * W;
                if (vec_in && gc0 >= 0 && gc0 + 3 < W) {
                    const float4 f = *reinterpret_cast<const float4*>(rp + gc0);
                    v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int gc = src_index(gc0 + e, W, R, border);
                        if (gc >= 0 && gc0 + e >= w0 - R && gc0 + e < w0 + TW + R) v[e] = rp[gc];
                    }
                }
            }
            *reinterpret_cast<float4*>(&S[row * SW + q * 4]) = make_float4(v[0], v[1], v[2], v[3]);
        }
        __syncthreads();
        // ---- 2. row pass
        for (int it = tid; it < ROWS * (TW / 4); it += 256) {
            const int row = it / (TW / 4), c4 = it % (TW / 4);
            const float* srow = &S[row * SW];
            float v[NV * 4];
#pragma unroll
            for (int i = 0; i < NV; ++i) {
                const float4 f = *reinterpret_cast<const float4*>(srow + c4 * 4 + A0 + 4 * i);
                v[4 * i] = f.x; v[4 * i + 1] = f.y; v[4 * i + 2] = f.z; v[4 * i + 3] = f.w;
            }
            float o[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float acc = 0.f;
#pragma unroll
                for (int j = 0; j < K; ++j) acc = __builtin_fmaf(tp.t[j], v[O + e + j], acc);
                if (FOLD) {
                    const int gc = w0 + c4 * 4 + e;
                    for (int f = 0; f < 2; ++f) {
                        if (f == 0 ? !(gc >= 1 && gc <= R) : !(gc >= W - 1 - R && gc <= W - 2)) continue;
                        const int p = f == 0 ? -gc : 2 * (W - 1) - gc;
                        float a = 0.f;
#pragma unroll
                        for (int j = 0; j < K; ++j) {
                            const int g = p + j - R, lc = g - w0 + PADL;
                            if (g >= 0 && g < W && lc >= 0 && lc < SW) a = __builtin_fmaf(tp.t[j], srow[lc], a);
                        }
                        acc += a;
                    }
                }
                o[e] = acc;
            }
            *reinterpret_cast<float4*>(&Rw[row * TW + c4 * 4]) = make_float4(o[0], o[1], o[2], o[3]);
        }
        __syncthreads();
        // ---- 3. column pass: a thread owns 2 rows x 4 columns
        {
            const int c4 = tid % (TW / 4), lh = (tid / (TW / 4)) * 2;
            float u[K + 1][4];
#pragma unroll
            for (int i = 0; i < K + 1; ++i) {
                const float4 f = *reinterpret_cast<const float4*>(&Rw[(lh + i) * TW + c4 * 4]);
                u[i][0] = f.x; u[i][1] = f.y; u[i][2] = f.z; u[i][3] = f.w;
            }
#pragma unroll
            for (int rr = 0; rr < 2; ++rr) {
                const int gh = h0 + lh + rr;
                float o[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float acc = 0.f;
#pragma unroll
                    for (int i = 0; i < K; ++i) acc = __builtin_fmaf(tp.t[i], u[rr + i][e], acc);
                    if (FOLD) {
                        for (int f = 0; f < 2; ++f) {
                            if (f == 0 ? !(gh >= 1 && gh <= R) : !(gh >= H - 1 - R && gh <= H - 2)) continue;
                            const int p = f == 0 ? -gh : 2 * (H - 1) - gh;
                            float a = 0.f;
#pragma unroll
                            for (int i = 0; i < K; ++i) {
                                const int g = p + i - R, lr = g - h0 + R;
                                if (g >= 0 && g < H && lr >= 0 && lr < ROWS) a = __builtin_fmaf(tp.t[i], Rw[lr * TW + c4 * 4 + e], a);
                            }
                            acc += a;
                        }
                    }
                    o[e] = acc;
                }
                const int gc0 = w0 + c4 * 4;
                if (gh < H) {
                    float* yp = py + (size_t)gh * W;
                    if (vec_out && gc0 + 3 < W) {
                        *reinterpret_cast<float4*>(yp + gc0) = make_float4(o[0], o[1], o[2], o[3]);
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if (gc0 + e < W) yp[gc0 + e] = o[e];
                    }
                }
            }
        }
        __syncthreads();   // S and Rw are staged again for the next plane
    }
}

template <bool FOLD>
int launch_gauss_sep(const float* x, float* y, int N, int H, int W, const Taps& tp, int k, int border, hipStream_t stream) {
    const dim3 grid((unsigned)wm_cdiv(W, TW), (unsigned)wm_cdiv(H, TH), (unsigned)(N < 65535 ? N : 65535)), block(256);
    const int vec_in = (W % 4 == 0 && ((uintptr_t)x & 15) == 0) ? 1 : 0, vec_out = (W % 4 == 0 && ((uintptr_t)y & 15) == 0) ? 1 : 0;
#define WM_GS_CASE(KK) \
    case KK: hipLaunchKernelGGL((gauss_sep_kernel<KK, FOLD>), grid, block, 0, stream, x, y, N, H, W, tp, border, vec_in, vec_out); break;
    switch (k) {
        WM_GS_CASE(3) WM_GS_CASE(5) WM_GS_CASE(7) WM_GS_CASE(9) WM_GS_CASE(11) WM_GS_CASE(13) WM_GS_CASE(15)
        default: return WM_E_BADARG;
    }
#undef WM_GS_CASE
    return WM_OK;
}

int gauss_sep_check(const char* name, const void* x, const void* y, int N, int H, int W, const float* taps, int k, int border) {
    WM_REQUIRE(x && y && taps && N > 0 && H > 0 && W > 0, WM_E_BADARG, "%s: bad arguments", name);
    WM_REQUIRE(k >= 3 && k <= WM_GAUSS_SEP_MAX_K && (k & 1), WM_E_BADARG, "%s: kernel size must be odd and in 3..%d (got %d)", name,
               WM_GAUSS_SEP_MAX_K, k);
    WM_REQUIRE(border == WM_BORDER_ZERO || border == WM_BORDER_REFLECT, WM_E_BADARG, "%s: border must be WM_BORDER_ZERO or WM_BORDER_REFLECT (got %d)",
               name, border);
    WM_REQUIRE(border != WM_BORDER_REFLECT || (k / 2 < H && k / 2 < W), WM_E_BADARG,
               "%s: a reflected border of %d pixels needs a plane larger than that in both directions (got %d x %d)", name, k / 2, H, W);
    WM_REQUIRE(wm_cdiv(H, TH) <= 65535, WM_E_BADARG, "%s: H = %d is above the launch grid's limit", name, H);
    return WM_OK;
}

// ---- Cropout.  grid = (column blocks, rows, planes) like the stencils; VEC: a thread owns 4 consecutive pixels of a 16-byte aligned row
template <bool VEC>
__global__ __launch_bounds__(256) void cropout_fwd_kernel(const float* __restrict__ x, const float* __restrict__ cover, float* __restrict__ y,
                                                          int N, int H, int W, int h0, int h1, int w0, int w1) {
    constexpr int V = VEC ? 4 : 1;
    const int c = (blockIdx.x * 256 + threadIdx.x) * V;
    if (c >= W) return;
    for (int n = blockIdx.z; n < N; n += gridDim.z) {
        for (int h = blockIdx.y; h < H; h += gridDim.y) {
            const size_t at = ((size_t)n * H + h) * W + c;
            const bool in_row = h >= h0 && h < h1;
            if (VEC) {
                const bool all_in = in_row && c >= w0 && c + 3 < w1, none_in = !in_row || c + 3 < w0 || c >= w1;
                float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
                if (!none_in) a = *reinterpret_cast<const float4*>(x + at);
                if (!all_in) b = *reinterpret_cast<const float4*>(cover + at);
                float4 o;
                o.x = (in_row && c >= w0 && c < w1) ? a.x : b.x;
                o.y = (in_row && c + 1 >= w0 && c + 1 < w1) ? a.y : b.y;
                o.z = (in_row && c + 2 >= w0 && c + 2 < w1) ? a.z : b.z;
                o.w = (in_row && c + 3 >= w0 && c + 3 < w1) ? a.w : b.w;
                *reinterpret_cast<float4*>(y + at) = o;
            } else {
                y[at] = (in_row && c >= w0 && c < w1) ? x[at] : cover[at];
            }
        }
    }
}

template <bool VEC>
__global__ __launch_bounds__(256) void cropout_bwd_kernel(const float* __restrict__ g, float* __restrict__ gx, float* __restrict__ gcover,
                                                          int N, int H, int W, int h0, int h1, int w0, int w1) {
    constexpr int V = VEC ? 4 : 1;
    const int c = (blockIdx.x * 256 + threadIdx.x) * V;
    if (c >= W) return;
    for (int n = blockIdx.z; n < N; n += gridDim.z) {
        for (int h = blockIdx.y; h < H; h += gridDim.y) {
            const size_t at = ((size_t)n * H + h) * W + c;
            const bool in_row = h >= h0 && h < h1;
            if (VEC) {
                const float4 v = *reinterpret_cast<const float4*>(g + at);
                const bool i0 = in_row && c >= w0 && c < w1, i1 = in_row && c + 1 >= w0 && c + 1 < w1;
                const bool i2 = in_row && c + 2 >= w0 && c + 2 < w1, i3 = in_row && c + 3 >= w0 && c + 3 < w1;
                *reinterpret_cast<float4*>(gx + at) = make_float4(i0 ? v.x : 0.f, i1 ? v.y : 0.f, i2 ? v.z : 0.f, i3 ? v.w : 0.f);
                if (gcover) *reinterpret_cast<float4*>(gcover + at) = make_float4(i0 ? 0.f : v.x, i1 ? 0.f : v.y, i2 ? 0.f : v.z, i3 ? 0.f : v.w);
            } else {
                const bool in = in_row && c >= w0 && c < w1;
                const float v = g[at];
                gx[at] = in ? v : 0.f;
                if (gcover) gcover[at] = in ? 0.f : v;
            }
        }
    }
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

inline dim3 cropout_grid(int N, int H, int W, bool vec) {
    return dim3((unsigned)wm_cdiv(vec ? W / 4 : W, 256), (unsigned)(H < 65535 ? H : 65535), (unsigned)(N < 65535 ? N : 65535));
}

}  // namespace

extern "C" int wm_gauss_sep_fwd(const float* x, float* y, int N, int H, int W, const float* taps, int k, int border, void* stream) {
    const int rc = gauss_sep_check("wm_gauss_sep_fwd", x, y, N, H, W, taps, k, border);
    if (rc != WM_OK) return rc;
    Taps tp = {};
    for (int i = 0; i < k; ++i) tp.t[i] = taps[i];
    launch_gauss_sep<false>(x, y, N, H, W, tp, k, border, (hipStream_t)stream);
    WM_LAUNCH_CHECK("wm_gauss_sep_fwd");
    return WM_OK;
}

extern "C" int wm_gauss_sep_bwd(const float* gy, float* gx, int N, int H, int W, const float* taps, int k, int border, void* stream) {
    const int rc = gauss_sep_check("wm_gauss_sep_bwd", gy, gx, N, H, W, taps, k, border);
    if (rc != WM_OK) return rc;
    Taps tp = {};
    for (int i = 0; i < k; ++i) tp.t[i] = taps[k - 1 - i];   // the transpose of a correlation: reversed taps
    if (border == WM_BORDER_REFLECT) launch_gauss_sep<true>(gy, gx, N, H, W, tp, k, WM_BORDER_ZERO, (hipStream_t)stream);
    else launch_gauss_sep<false>(gy, gx, N, H, W, tp, k, WM_BORDER_ZERO, (hipStream_t)stream);
    WM_LAUNCH_CHECK("wm_gauss_sep_bwd");
    return WM_OK;
}

extern "C" int wm_cropout_fwd(const float* x, const float* cover, float* y, int N, int H, int W, int h0, int h1, int w0, int w1, void* stream) {
    WM_REQUIRE(x && cover && y && N > 0 && H > 0 && W > 0, WM_E_BADARG, "wm_cropout_fwd: bad arguments");
    WM_REQUIRE(0 <= h0 && h0 < h1 && h1 <= H && 0 <= w0 && w0 < w1 && w1 <= W, WM_E_BADARG,
               "wm_cropout_fwd: rectangle [%d,%d) x [%d,%d) is empty or not inside the %d x %d plane", h0, h1, w0, w1, H, W);
    const bool vec = W % 4 == 0 && aligned16(x) && aligned16(cover) && aligned16(y);
    if (vec) hipLaunchKernelGGL(cropout_fwd_kernel<true>, cropout_grid(N, H, W, true), dim3(256), 0, (hipStream_t)stream, x, cover, y, N, H, W, h0, h1, w0, w1);
    else hipLaunchKernelGGL(cropout_fwd_kernel<false>, cropout_grid(N, H, W, false), dim3(256), 0, (hipStream_t)stream, x, cover, y, N, H, W, h0, h1, w0, w1);
    WM_LAUNCH_CHECK("wm_cropout_fwd");
    return WM_OK;
}

extern "C" int wm_cropout_bwd(const float* g, float* gx, float* gcover, int N, int H, int W, int h0, int h1, int w0, int w1, void* stream) {
    WM_REQUIRE(g && gx && N > 0 && H > 0 && W > 0, WM_E_BADARG, "wm_cropout_bwd: bad arguments");
    WM_REQUIRE(0 <= h0 && h0 < h1 && h1 <= H && 0 <= w0 && w0 < w1 && w1 <= W, WM_E_BADARG,
               "wm_cropout_bwd: rectangle [%d,%d) x [%d,%d) is empty or not inside the %d x %d plane", h0, h1, w0, w1, H, W);
    const bool vec = W % 4 == 0 && aligned16(g) && aligned16(gx) && aligned16(gcover);
    if (vec) hipLaunchKernelGGL(cropout_bwd_kernel<true>, cropout_grid(N, H, W, true), dim3(256), 0, (hipStream_t)stream, g, gx, gcover, N, H, W, h0, h1, w0, w1);
    else hipLaunchKernelGGL(cropout_bwd_kernel<false>, cropout_grid(N, H, W, false), dim3(256), 0, (hipStream_t)stream, g, gx, gcover, N, H, W, h0, h1, w0, w1);
    WM_LAUNCH_CHECK("wm_cropout_bwd");
    return WM_OK;
}
