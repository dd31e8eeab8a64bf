// Pixel- and gradient-domain image losses of the reference's trainers, each with its autograd backward:
//   ReconstructionLoss (models/modules/loss.py:5-22)  mean_b sum_chw f(x - t)                  wm_recon_sums / _finalize / _bwd
//       f = d^2 (WM_RECON_L2) | sqrt(d^2 + eps) (WM_RECON_LCHAR) | d (WM_RECON_L1: the reference's SIGNED sum, no abs)
//   GradientLoss (loss.py:413-423)   mean |a[..,:-1] - a[..,1:]| + mean |a[..,:-1,:] - a[..,1:,:]|   wm_gradloss_sums / _finalize / _bwd
//   ExclusionLoss (loss.py:309-360)  per level, direction and channel pair mean(s1^2 s2^2) ** 0.25,  wm_excl_fwd / _finalize / _bwd
//       s = 2 sigmoid(diff) - 1, 2 x 2 average pooling between the levels
// f32 NCHW contiguous tensors.  No atomics and no host synchronisation: every forward writes per-workgroup partial sums in double, a
// one-workgroup finalise adds them in a fixed order.  Every result is bitwise reproducible.
//
// The two streaming losses difference and square in double (x - t is exact there) and round once; the exclusion loss evaluates its
// sigmoids in f32 as 2 * (1 / (1 + expf(-d))) - 1, the reference's expression, multiplies in f32 and adds in double.
//
// Exclusion: a workgroup owns a 16 x 32 tile of level-0 pixels of one sample.  It loads the tile of every channel of both images into LDS
// with a 4-pixel halo below and right (the backward: on all four sides), pools levels 1 and 2 there, and handles every difference whose
// FIRST pixel lies in its tile: tile origins are multiples of 4, so a pooled pixel of any level belongs to exactly one tile, and the second
// pixel of a difference is at most 4 level-0 pixels further.  Pooled images and difference maps exist in LDS only.
#include "wm_common.h"
#include "wm_reduce.h"

namespace {

constexpr int L2 = WM_RECON_L2, LCHAR = WM_RECON_LCHAR, L1 = WM_RECON_L1;
constexpr int TH = 16, TW = 32;        // the exclusion tile (level-0 pixels)
constexpr int HALO = 4;                // = one pixel of level 2
constexpr int MAXC = 4, MAXL = 3, MAXSLOTS = MAXL * 2 * MAXC * MAXC;

// ------------------------------------------------------------------------------------------------ reconstruction
template <int KIND> __device__ __forceinline__ double recon_f(float x, float t, double eps) {
    const double d = (double)x - (double)t;
    if (KIND == L2) return d * d;
    if (KIND == LCHAR) return sqrt(d * d + eps);
    return d;
}
// f'(d) * k
template <int KIND> __device__ __forceinline__ float recon_df(float x, float t, double eps, double k) {
    const double d = (double)x - (double)t;
    if (KIND == L2) return (float)(2.0 * d * k);
    if (KIND == LCHAR) return (float)(d / sqrt(d * d + eps) * k);
    return (float)k;
}

// grid (P, B): block (j, b) takes its grid-stride share of sample b -> partials[b*P + j]
template <int KIND>
__global__ __launch_bounds__(256) void recon_sums_kernel(const float* __restrict__ x, const float* __restrict__ t, size_t per, double eps,
                                                         double* __restrict__ partials) {
    const float* xb = x + (size_t)blockIdx.y * per;
    const float* tb = t + (size_t)blockIdx.y * per;
    const Split sp = split16(per, xb, tb);
    double a = 0.0;
    stream16(sp, per,
             [&](size_t at) {
                 const float4 p = ld16(xb + at), q = ld16(tb + at);
                 a += recon_f<KIND>(p.x, q.x, eps); a += recon_f<KIND>(p.y, q.y, eps); a += recon_f<KIND>(p.z, q.z, eps); a += recon_f<KIND>(p.w, q.w, eps);
             },
             [&](size_t idx) { a += recon_f<KIND>(xb[idx], tb[idx], eps); });
    __shared__ double s[4];
    a = block_sum_f64(a, s);
    if (threadIdx.x == 0) partials[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = a;
}

// grid (G, B): grad (+)= g / B * f'(x - t)
template <int KIND>
__global__ __launch_bounds__(256) void recon_bwd_kernel(const float* __restrict__ x, const float* __restrict__ t, float* __restrict__ grad, int B,
                                                        size_t per, double eps, const float* __restrict__ gout, float gscale,
                                                        const float* __restrict__ gscale_dev, int accumulate) {
    const double k = upstream(gscale, gscale_dev, gout) / (double)B;
    const float* xb = x + (size_t)blockIdx.y * per;
    const float* tb = t + (size_t)blockIdx.y * per;
    float* gb = grad + (size_t)blockIdx.y * per;
    const Split sp = split16(per, xb, tb, gb);
    stream16(sp, per,
             [&](size_t at) {
                 const float4 p = ld16(xb + at), q = ld16(tb + at);
                 store4<float>(gb + at, recon_df<KIND>(p.x, q.x, eps, k), recon_df<KIND>(p.y, q.y, eps, k), recon_df<KIND>(p.z, q.z, eps, k),
                               recon_df<KIND>(p.w, q.w, eps, k), accumulate);
             },
             [&](size_t idx) { store1<float>(gb + idx, recon_df<KIND>(xb[idx], tb[idx], eps, k), accumulate); });
}

inline int stream_parts(size_t per_sample) { return wm_groups(per_sample, 4096, 64); }
inline int bwd_groups(size_t per_sample) { return wm_groups(per_sample, 1024, 256); }
inline bool kind_ok(int k) { return k == L2 || k == LCHAR || k == L1; }

// ------------------------------------------------------------------------------------------------ gradient loss
// grid (P, N), N = B*C planes of H x W: block (j, n) takes its grid-stride share of plane n's pixels; pixel (y, x) owns the differences to
// its right and lower neighbours -> partials[(n*P + j)*2 + {sum |d/dx|, sum |d/dy|}]
__global__ __launch_bounds__(256) void gradloss_sums_kernel(const float* __restrict__ a, int H, int W, double* __restrict__ partials) {
    const size_t HW = (size_t)H * W;
    const float* p = a + (size_t)blockIdx.y * HW;
    double sx = 0.0, sy = 0.0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < HW; i += (size_t)gridDim.x * 256) {
        const int y = (int)(i / W), x = (int)(i - (size_t)y * W);
        const double v = (double)p[i];
        if (x + 1 < W) sx += fabs(v - (double)p[i + 1]);
        if (y + 1 < H) sy += fabs(v - (double)p[i + W]);
    }
    __shared__ double s[2][4];
    sx = block_sum_f64(sx, s[0]);
    sy = block_sum_f64(sy, s[1]);
    if (threadIdx.x == 0) {
        double* q = partials + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 2;
        q[0] = sx; q[1] = sy;
    }
}

// one workgroup: partials [n][2] -> out[0] = sum_x / cx + sum_y / cy
__global__ __launch_bounds__(256) void gradloss_finalize_kernel(const double* __restrict__ partials, size_t n, double cx, double cy, float* __restrict__ out) {
    __shared__ double s[2][4];
    double sx = 0.0, sy = 0.0;
    for (size_t i = threadIdx.x; i < n; i += 256) { sx += partials[2 * i]; sy += partials[2 * i + 1]; }
    sx = block_sum_f64(sx, s[0]);
    sy = block_sum_f64(sy, s[1]);
    if (threadIdx.x == 0) out[0] = (float)(sx / cx + sy / cy);
}

__device__ __forceinline__ int sgn(float d) { return (d > 0.f) - (d < 0.f); }   // 0 at 0, as torch's abs backward

// gather form: pixel (y, x) collects the four differences it is part of
__global__ __launch_bounds__(256) void gradloss_bwd_kernel(const float* __restrict__ a, float* __restrict__ grad, int H, int W, double cx, double cy,
                                                           const float* __restrict__ gout, float gscale, const float* __restrict__ gscale_dev,
                                                           int accumulate) {
    const double g = upstream(gscale, gscale_dev, gout), gx = g / cx, gy = g / cy;
    const size_t HW = (size_t)H * W;
    const float* p = a + (size_t)blockIdx.y * HW;
    float* q = grad + (size_t)blockIdx.y * HW;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < HW; i += (size_t)gridDim.x * 256) {
        const int y = (int)(i / W), x = (int)(i - (size_t)y * W);
        const float v = p[i];
        int nx = 0, ny = 0;
        if (x + 1 < W) nx += sgn(v - p[i + 1]);
        if (x > 0) nx -= sgn(p[i - 1] - v);
        if (y + 1 < H) ny += sgn(v - p[i + W]);
        if (y > 0) ny -= sgn(p[i - W] - v);
        const float r = (float)((double)nx * gx + (double)ny * gy);
        q[i] = accumulate ? q[i] + r : r;
    }
}

// ------------------------------------------------------------------------------------------------ exclusion
// LDS tile of HB + T + HALO level-0 rows / columns per channel, and its two pooled levels; level l's array starts (HB >> l) level-l pixels
// before the tile's first.  Channels 0 .. C1-1 are img1's, C1 .. C1+C2-1 img2's.
template <int HB> struct Tile {
    static constexpr int R0 = HB + TH + HALO, C0 = HB + TW + HALO;
    static constexpr int R1 = R0 / 2, C1 = C0 / 2, R2 = R0 / 4, C2 = C0 / 4;
    alignas(16) float l0[2 * MAXC][R0][C0];     // (rows are a multiple of 16 bytes: load_tile stores float4s)
    float l1[2 * MAXC][R1][C1];
    float l2[2 * MAXC][R2][C2];
};

struct ExclDims {
    int B, C1, C2, H, W, levels;
};

// the whole tile, zero outside the image.  vec: W % 4 == 0 and both bases 16-byte aligned -- a group of 4 columns is then inside or outside
// the image as a whole (tile origins and the halo are multiples of 4)
template <int HB>
__device__ __forceinline__ void load_tile(Tile<HB>& t, const float* __restrict__ img1, const float* __restrict__ img2, const ExclDims& d, int b,
                                          int y0, int x0, bool vec) {
    using T = Tile<HB>;
    const int nch = d.C1 + d.C2;
    const size_t HW = (size_t)d.H * d.W;
    if (vec) {
        constexpr int Q = T::C0 / 4;
        for (int i = threadIdx.x; i < nch * T::R0 * Q; i += 256) {
            const int ch = i / (T::R0 * Q), r = (i / Q) % T::R0, q = i % Q;
            const int gy = y0 - HB + r, gx = x0 - HB + 4 * q;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (gy >= 0 && gy < d.H && gx >= 0 && gx < d.W) {
                const float* plane = ch < d.C1 ? img1 + ((size_t)b * d.C1 + ch) * HW : img2 + ((size_t)b * d.C2 + (ch - d.C1)) * HW;
                v = *reinterpret_cast<const float4*>(plane + (size_t)gy * d.W + gx);
            }
            *reinterpret_cast<float4*>(&t.l0[ch][r][4 * q]) = v;
        }
    } else {
        for (int i = threadIdx.x; i < nch * T::R0 * T::C0; i += 256) {
            const int ch = i / (T::R0 * T::C0), r = (i / T::C0) % T::R0, c = i % T::C0;
            const int gy = y0 - HB + r, gx = x0 - HB + c;
            float v = 0.f;
            if (gy >= 0 && gy < d.H && gx >= 0 && gx < d.W) {
                const float* plane = ch < d.C1 ? img1 + ((size_t)b * d.C1 + ch) * HW : img2 + ((size_t)b * d.C2 + (ch - d.C1)) * HW;
                v = plane[(size_t)gy * d.W + gx];
            }
            t.l0[ch][r][c] = v;
        }
    }
}

// AvgPool2d(2, stride 2) of one level into the next: the four values added row by row, then * 0.25
template <int RS, int CS, int RD, int CD>
__device__ __forceinline__ void pool_level(const float (&src)[2 * MAXC][RS][CS], float (&dst)[2 * MAXC][RD][CD], int nch) {
    for (int i = threadIdx.x; i < nch * RD * CD; i += 256) {
        const int ch = i / (RD * CD), r = (i / CD) % RD, c = i % CD;
        dst[ch][r][c] = (((src[ch][2 * r][2 * c] + src[ch][2 * r][2 * c + 1]) + src[ch][2 * r + 1][2 * c]) + src[ch][2 * r + 1][2 * c + 1]) * 0.25f;
    }
}

template <int HB>
__device__ __forceinline__ void fill_levels(Tile<HB>& t, const float* __restrict__ img1, const float* __restrict__ img2, const ExclDims& d, int b,
                                            int y0, int x0, bool vec) {
    load_tile<HB>(t, img1, img2, d, b, y0, x0, vec);
    __syncthreads();
    if (d.levels > 1) pool_level(t.l0, t.l1, d.C1 + d.C2);
    __syncthreads();
    if (d.levels > 2) pool_level(t.l1, t.l2, d.C1 + d.C2);
    __syncthreads();
}

// s = 2 sigmoid(d) - 1 in the reference's form
__device__ __forceinline__ float sig2m1(float d) { return (1.f / (1.f + expf(-d))) * 2.f - 1.f; }

// a level's plane as (base of channel 0, row pitch, channel pitch)
struct LevelView { const float* p; int pitch, plane; };
template <int HB> __device__ __forceinline__ LevelView level_view(const Tile<HB>& t, int l) {
    using T = Tile<HB>;
    if (l == 0) return {&t.l0[0][0][0], T::C0, T::R0 * T::C0};
    if (l == 1) return {&t.l1[0][0][0], T::C1, T::R1 * T::C1};
    return {&t.l2[0][0][0], T::C2, T::R2 * T::C2};
}

// s of every channel for the difference second - first (LDS offsets within a channel's plane)
__device__ __forceinline__ void link_s(const LevelView& v, int first, int second, int C1, int C2, float (&sa)[MAXC], float (&sb)[MAXC]) {
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
        sa[c] = 0.f; sb[c] = 0.f;
        if (c < C1) sa[c] = sig2m1(v.p[c * v.plane + second] - v.p[c * v.plane + first]);
        if (c < C2) sb[c] = sig2m1(v.p[(C1 + c) * v.plane + second] - v.p[(C1 + c) * v.plane + first]);
    }
}

// grid (tiles_x, tiles_y, B) -> partials[slot * nwg + wg], slot = (level*2 + dir)*C1*C2 + i2*C1 + i1, dir 0 = gradx (rows), 1 = grady (columns)
__global__ __launch_bounds__(256) void excl_fwd_kernel(const float* __restrict__ img1, const float* __restrict__ img2, ExclDims d, int vec,
                                                       double* __restrict__ partials) {
    __shared__ Tile<0> t;
    __shared__ double red[4][MAXSLOTS];
    const int b = blockIdx.z, y0 = blockIdx.y * TH, x0 = blockIdx.x * TW;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, CC = d.C1 * d.C2;
    fill_levels<0>(t, img1, img2, d, b, y0, x0, vec != 0);
    for (int l = 0; l < d.levels; ++l) {
        const LevelView v = level_view<0>(t, l);
        const int Hl = d.H >> l, Wl = d.W >> l, th = TH >> l, tw = TW >> l, Y0 = y0 >> l, X0 = x0 >> l;
        double acc[2][MAXC * MAXC];
#pragma unroll
        for (int k = 0; k < MAXC * MAXC; ++k) { acc[0][k] = 0.0; acc[1][k] = 0.0; }
        for (int i = threadIdx.x; i < th * tw; i += 256) {
            const int r = i / tw, c = i - r * tw, Y = Y0 + r, X = X0 + c;
            if (Y >= Hl || X >= Wl) continue;
            const int o = r * v.pitch + c;
#pragma unroll
            for (int dir = 0; dir < 2; ++dir) {
                if (dir == 0 ? Y + 1 >= Hl : X + 1 >= Wl) continue;
                float sa[MAXC], sb[MAXC];
                link_s(v, o, dir == 0 ? o + v.pitch : o + 1, d.C1, d.C2, sa, sb);
#pragma unroll
                for (int i2 = 0; i2 < MAXC; ++i2)
#pragma unroll
                    for (int i1 = 0; i1 < MAXC; ++i1)
                        if (i1 < d.C1 && i2 < d.C2) acc[dir][i2 * MAXC + i1] += (double)((sa[i1] * sa[i1]) * (sb[i2] * sb[i2]));
            }
        }
#pragma unroll
        for (int dir = 0; dir < 2; ++dir)
#pragma unroll
            for (int i2 = 0; i2 < MAXC; ++i2)
#pragma unroll
                for (int i1 = 0; i1 < MAXC; ++i1)
                    if (i1 < d.C1 && i2 < d.C2) {
                        const double s = wave_sum_f64(acc[dir][i2 * MAXC + i1]);
                        if (lane == 0) red[w][(l * 2 + dir) * CC + i2 * d.C1 + i1] = s;
                    }
    }
    __syncthreads();
    const int nslots = d.levels * 2 * CC;
    const size_t nwg = (size_t)gridDim.x * gridDim.y * gridDim.z, wg = ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    if ((int)threadIdx.x < nslots)
        partials[(size_t)threadIdx.x * nwg + wg] = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}

// number of differences of one channel pair at (level, dir): the mean's divisor
__device__ __forceinline__ double excl_count(const ExclDims& d, int l, int dir) {
    const double Hl = (double)(d.H >> l), Wl = (double)(d.W >> l);
    return (double)d.B * (dir == 0 ? (Hl - 1.0) * Wl : Hl * (Wl - 1.0));
}

// one workgroup.  Wave w sums the nwg partials of slots w, w+4, ... (lane j adds partials j, j+64, ...: a fixed order, then the butterfly):
// means[slot] = sum / count, coef[slot] = d loss / d (one product of that slot) = 0.25 mean^-0.75 / (levels * 18) / count, 0 where the mean
// is 0 (the term vanishes and contributes no gradient).  Then loss = sum_slots mean^0.25 / (levels * 9) / 2 -- 9 whatever C1*C2 is.
__global__ __launch_bounds__(256) void excl_finalize_kernel(const double* __restrict__ partials, size_t nwg, ExclDims d, double* __restrict__ means,
                                                            double* __restrict__ coef, float* __restrict__ loss) {
    __shared__ double term[MAXSLOTS];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, CC = d.C1 * d.C2, nslots = d.levels * 2 * CC;
    const double norm = (double)d.levels * 18.0;
    for (int s = w; s < nslots; s += 4) {
        double a = 0.0;
        for (size_t i = lane; i < nwg; i += 64) a += partials[(size_t)s * nwg + i];
        a = wave_sum_f64(a);
        if (lane == 0) {
            const int ld = s / CC;
            const double cnt = excl_count(d, ld >> 1, ld & 1), m = a / cnt, r = sqrt(sqrt(m));
            means[s] = m;
            coef[s] = m > 0.0 ? 0.25 / (r * r * r) / norm / cnt : 0.0;
            term[s] = r;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double a = 0.0;
        for (int s = 0; s < nslots; ++s) a += term[s];
        loss[0] = (float)(a / norm);
    }
}

// the gradient one difference (first -> second, of level l and direction dir) sends to each channel of both images, ADDED with `sign` (+1: the
// pixel is the difference's second, -1: its first):  d (s1^2 s2^2) / d diff1 = s1 (1 - s1^2) s2^2   (ds / d diff = (1 - s^2) / 2)
__device__ __forceinline__ void link_grad(const LevelView& v, int first, int second, int C1, int C2, const float* __restrict__ cf, float sign,
                                          float (&g1)[MAXC], float (&g2)[MAXC]) {
    float sa[MAXC], sb[MAXC];
    link_s(v, first, second, C1, C2, sa, sb);
    float ta[MAXC] = {0.f, 0.f, 0.f, 0.f}, tb[MAXC] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i2 = 0; i2 < MAXC; ++i2)
#pragma unroll
        for (int i1 = 0; i1 < MAXC; ++i1)
            if (i1 < C1 && i2 < C2) {
                const float c = cf[i2 * C1 + i1];
                ta[i1] = __builtin_fmaf(c, sb[i2] * sb[i2], ta[i1]);
                tb[i2] = __builtin_fmaf(c, sa[i1] * sa[i1], tb[i2]);
            }
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
        g1[c] = __builtin_fmaf(sign * (sa[c] * (1.f - sa[c] * sa[c])), ta[c], g1[c]);
        g2[c] = __builtin_fmaf(sign * (sb[c] * (1.f - sb[c] * sb[c])), tb[c], g2[c]);
    }
}

// the gradient wrt level-l pixel (Y, X) of every channel: as the first and as the second pixel of its differences in both directions.
// o: the pixel's offset within a channel's LDS plane; cf: [levels][2][C1*C2] coefficients, already times the upstream weight
__device__ __forceinline__ void pixel_grad(const LevelView& v, int o, int Y, int X, int Hl, int Wl, int l, int C1, int C2, const float* __restrict__ cf,
                                           float (&g1)[MAXC], float (&g2)[MAXC]) {
    const int CC = C1 * C2;
    const float* cx = cf + (l * 2 + 0) * CC;
    const float* cy = cf + (l * 2 + 1) * CC;
    if (Y + 1 < Hl) link_grad(v, o, o + v.pitch, C1, C2, cx, -1.f, g1, g2);
    if (Y > 0) link_grad(v, o - v.pitch, o, C1, C2, cx, 1.f, g1, g2);
    if (X + 1 < Wl) link_grad(v, o, o + 1, C1, C2, cy, -1.f, g1, g2);
    if (X > 0) link_grad(v, o - 1, o, C1, C2, cy, 1.f, g1, g2);
}

// grid (tiles_x, tiles_y, B), gather form: levels 2 and 1 of the tile first (their gradients, times 4^-level, into LDS), then every level-0
// pixel adds its own gradient and those of the pooled pixels above it
__global__ __launch_bounds__(256) void excl_bwd_kernel(const float* __restrict__ img1, const float* __restrict__ img2, const double* __restrict__ coef,
                                                       float* __restrict__ grad1, float* __restrict__ grad2, ExclDims d, int vec,
                                                       const float* __restrict__ gout, float gscale, const float* __restrict__ gscale_dev,
                                                       int accumulate) {
    __shared__ Tile<HALO> t;
    __shared__ float cf[MAXSLOTS];
    __shared__ float up1[2 * MAXC][TH / 2][TW / 2], up2[2 * MAXC][TH / 4][TW / 4];
    const int b = blockIdx.z, y0 = blockIdx.y * TH, x0 = blockIdx.x * TW, C1 = d.C1, C2 = d.C2;
    const int nslots = d.levels * 2 * C1 * C2;
    if ((int)threadIdx.x < nslots) cf[threadIdx.x] = (float)(coef[threadIdx.x] * upstream(gscale, gscale_dev, gout));
    fill_levels<HALO>(t, img1, img2, d, b, y0, x0, vec != 0);      // (its barriers also publish cf)
    for (int l = d.levels - 1; l >= 1; --l) {
        const LevelView v = level_view<HALO>(t, l);
        const int Hl = d.H >> l, Wl = d.W >> l, th = TH >> l, tw = TW >> l, Y0 = y0 >> l, X0 = x0 >> l, hb = HALO >> l;
        const float scale = l == 1 ? 0.25f : 0.0625f;
        for (int i = threadIdx.x; i < th * tw; i += 256) {
            const int r = i / tw, c = i - r * tw, Y = Y0 + r, X = X0 + c;
            float g1[MAXC] = {0.f, 0.f, 0.f, 0.f}, g2[MAXC] = {0.f, 0.f, 0.f, 0.f};
            if (Y < Hl && X < Wl) pixel_grad(v, (r + hb) * v.pitch + c + hb, Y, X, Hl, Wl, l, C1, C2, cf, g1, g2);
#pragma unroll
            for (int ch = 0; ch < MAXC; ++ch) {
                if (l == 1) { up1[ch][r][c] = g1[ch] * scale; up1[MAXC + ch][r][c] = g2[ch] * scale; }
                else { up2[ch][r][c] = g1[ch] * scale; up2[MAXC + ch][r][c] = g2[ch] * scale; }
            }
        }
    }
    __syncthreads();
    const LevelView v = level_view<HALO>(t, 0);
    const size_t HW = (size_t)d.H * d.W;
    for (int i = threadIdx.x; i < TH * TW; i += 256) {
        const int r = i / TW, c = i - r * TW, Y = y0 + r, X = x0 + c;
        if (Y >= d.H || X >= d.W) continue;
        float g1[MAXC] = {0.f, 0.f, 0.f, 0.f}, g2[MAXC] = {0.f, 0.f, 0.f, 0.f};
        pixel_grad(v, (r + HALO) * v.pitch + c + HALO, Y, X, d.H, d.W, 0, C1, C2, cf, g1, g2);
#pragma unroll
        for (int ch = 0; ch < MAXC; ++ch) {
            // (a pooled pixel that does not exist -- the odd last row / column -- holds 0)
            if (d.levels > 1) { g1[ch] += up1[ch][r >> 1][c >> 1]; g2[ch] += up1[MAXC + ch][r >> 1][c >> 1]; }
            if (d.levels > 2) { g1[ch] += up2[ch][r >> 2][c >> 2]; g2[ch] += up2[MAXC + ch][r >> 2][c >> 2]; }
            const size_t px = (size_t)Y * d.W + X;
            if (grad1 && ch < C1) {
                float* q = grad1 + ((size_t)b * C1 + ch) * HW + px;
                *q = accumulate ? *q + g1[ch] : g1[ch];
            }
            if (grad2 && ch < C2) {
                float* q = grad2 + ((size_t)b * C2 + ch) * HW + px;
                *q = accumulate ? *q + g2[ch] : g2[ch];
            }
        }
    }
}

inline bool excl_dims_ok(int B, int C1, int C2, int H, int W, int levels) {
    if (!(B > 0 && B <= 65535 && C1 >= 1 && C1 <= MAXC && C2 >= 1 && C2 <= MAXC && levels >= 1 && levels <= MAXL)) return false;
    const int need = 2 << (levels - 1);      // two pixels at the last level: below that the reference takes the mean of an empty tensor
    return H >= need && W >= need && (H + TH - 1) / TH <= 65535;
}
inline dim3 excl_grid(int B, int H, int W) { return dim3((W + TW - 1) / TW, (H + TH - 1) / TH, B); }
inline bool excl_vec(const void* a, const void* b, int W) { return W % 4 == 0 && (((uintptr_t)a | (uintptr_t)b) & 15) == 0; }

}  // namespace

extern "C" int wm_recon_nparts(size_t per_sample) { return per_sample > 0 ? stream_parts(per_sample) : 0; }

#define RECON_DISPATCH(KERNEL, ...)                                                                       \
    do {                                                                                                  \
        if (kind == L2) hipLaunchKernelGGL(KERNEL<L2>, grid, dim3(256), 0, s, __VA_ARGS__);               \
        else if (kind == LCHAR) hipLaunchKernelGGL(KERNEL<LCHAR>, grid, dim3(256), 0, s, __VA_ARGS__);    \
        else hipLaunchKernelGGL(KERNEL<L1>, grid, dim3(256), 0, s, __VA_ARGS__);                          \
    } while (0)

extern "C" int wm_recon_sums(const float* x, const float* target, int B, size_t per_sample, int kind, float eps, double* partials, void* stream) {
    WM_REQUIRE(x && target && partials && B > 0 && B <= 65535 && per_sample > 0 && kind_ok(kind) && eps >= 0.f, WM_E_BADARG,
               "wm_recon_sums: bad arguments (B <= 65535, kind WM_RECON_L2 / LCHAR / L1, eps >= 0)");
    const dim3 grid(stream_parts(per_sample), B);
    hipStream_t s = (hipStream_t)stream;
    RECON_DISPATCH(recon_sums_kernel, x, target, per_sample, (double)eps, partials);
    WM_LAUNCH_CHECK("wm_recon_sums");
    return WM_OK;
}

extern "C" int wm_recon_finalize(const double* partials, int B, size_t per_sample, float* loss_out, void* stream) {
    WM_REQUIRE(partials && loss_out && B > 0 && per_sample > 0, WM_E_BADARG, "wm_recon_finalize: bad arguments");
    wm_sum_finalize(partials, (size_t)B * stream_parts(per_sample), 1.0 / (double)B, loss_out, (hipStream_t)stream);
    WM_LAUNCH_CHECK("wm_recon_finalize");
    return WM_OK;
}

extern "C" int wm_recon_bwd(const float* x, const float* target, float* grad, int B, size_t per_sample, int kind, float eps, const float* gout_dev,
                            float gscale, const float* gscale_dev, int accumulate, void* stream) {
    WM_REQUIRE(x && target && grad && B > 0 && B <= 65535 && per_sample > 0 && kind_ok(kind) && eps >= 0.f, WM_E_BADARG,
               "wm_recon_bwd: bad arguments (B <= 65535, kind WM_RECON_L2 / LCHAR / L1, eps >= 0)");
    const dim3 grid(bwd_groups(per_sample), B);
    hipStream_t s = (hipStream_t)stream;
    RECON_DISPATCH(recon_bwd_kernel, x, target, grad, B, per_sample, (double)eps, gout_dev, gscale, gscale_dev, accumulate);
    WM_LAUNCH_CHECK("wm_recon_bwd");
    return WM_OK;
}

extern "C" int wm_gradloss_nparts(int H, int W) { return H > 0 && W > 0 ? stream_parts((size_t)H * W) : 0; }

extern "C" int wm_gradloss_sums(const float* a, int N, int H, int W, double* partials, void* stream) {
    WM_REQUIRE(a && partials && N > 0 && N <= 65535 && H >= 2 && W >= 2, WM_E_BADARG,
               "wm_gradloss_sums: bad arguments (B*C <= 65535, H, W >= 2: below that a mean is over nothing)");
    hipLaunchKernelGGL(gradloss_sums_kernel, dim3(stream_parts((size_t)H * W), N), dim3(256), 0, (hipStream_t)stream, a, H, W, partials);
    WM_LAUNCH_CHECK("wm_gradloss_sums");
    return WM_OK;
}

extern "C" int wm_gradloss_finalize(const double* partials, int N, int H, int W, float* loss_out, void* stream) {
    WM_REQUIRE(partials && loss_out && N > 0 && H >= 2 && W >= 2, WM_E_BADARG, "wm_gradloss_finalize: bad arguments");
    hipLaunchKernelGGL(gradloss_finalize_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, partials, (size_t)N * stream_parts((size_t)H * W),
                       (double)N * H * (W - 1.0), (double)N * (H - 1.0) * W, loss_out);
    WM_LAUNCH_CHECK("wm_gradloss_finalize");
    return WM_OK;
}

extern "C" int wm_gradloss_bwd(const float* a, float* grad, int N, int H, int W, const float* gout_dev, float gscale, const float* gscale_dev,
                               int accumulate, void* stream) {
    WM_REQUIRE(a && grad && N > 0 && N <= 65535 && H >= 2 && W >= 2, WM_E_BADARG, "wm_gradloss_bwd: bad arguments (B*C <= 65535, H, W >= 2)");
    hipLaunchKernelGGL(gradloss_bwd_kernel, dim3(bwd_groups((size_t)H * W), N), dim3(256), 0, (hipStream_t)stream, a, grad, H, W,
                       (double)N * H * (W - 1.0), (double)N * (H - 1.0) * W, gout_dev, gscale, gscale_dev, accumulate);
    WM_LAUNCH_CHECK("wm_gradloss_bwd");
    return WM_OK;
}

extern "C" int wm_excl_nparts(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    const dim3 g = excl_grid(B, H, W);
    const size_t n = (size_t)g.x * g.y * g.z;
    return n > 0x7fffffffu ? 0 : (int)n;
}

extern "C" int wm_excl_fwd(const float* img1, const float* img2, int B, int C1, int C2, int H, int W, int levels, double* partials, void* stream) {
    WM_REQUIRE(img1 && img2 && partials && excl_dims_ok(B, C1, C2, H, W, levels), WM_E_BADARG,
               "wm_excl_fwd: bad arguments (B <= 65535, 1 <= C1, C2 <= 4, 1 <= levels <= 3, H and W >= 2 << (levels - 1))");
    const ExclDims d{B, C1, C2, H, W, levels};
    hipLaunchKernelGGL(excl_fwd_kernel, excl_grid(B, H, W), dim3(256), 0, (hipStream_t)stream, img1, img2, d, excl_vec(img1, img2, W) ? 1 : 0, partials);
    WM_LAUNCH_CHECK("wm_excl_fwd");
    return WM_OK;
}

extern "C" int wm_excl_finalize(const double* partials, int B, int C1, int C2, int H, int W, int levels, double* means, double* coef, float* loss_out,
                                void* stream) {
    WM_REQUIRE(partials && means && coef && loss_out && excl_dims_ok(B, C1, C2, H, W, levels), WM_E_BADARG, "wm_excl_finalize: bad arguments");
    const ExclDims d{B, C1, C2, H, W, levels};
    const dim3 g = excl_grid(B, H, W);
    hipLaunchKernelGGL(excl_finalize_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, partials, (size_t)g.x * g.y * g.z, d, means, coef, loss_out);
    WM_LAUNCH_CHECK("wm_excl_finalize");
    return WM_OK;
}

extern "C" int wm_excl_bwd(const float* img1, const float* img2, const double* coef, float* grad1, float* grad2, int B, int C1, int C2, int H, int W,
                           int levels, const float* gout_dev, float gscale, const float* gscale_dev, int accumulate, void* stream) {
    WM_REQUIRE(img1 && img2 && coef && (grad1 || grad2) && excl_dims_ok(B, C1, C2, H, W, levels), WM_E_BADARG,
               "wm_excl_bwd: bad arguments (at least one gradient buffer; B <= 65535, 1 <= C1, C2 <= 4, 1 <= levels <= 3, H and W >= 2 << (levels - 1))");
    const ExclDims d{B, C1, C2, H, W, levels};
    hipLaunchKernelGGL(excl_bwd_kernel, excl_grid(B, H, W), dim3(256), 0, (hipStream_t)stream, img1, img2, coef, grad1, grad2, d,
                       excl_vec(img1, img2, W) ? 1 : 0, gout_dev, gscale, gscale_dev, accumulate);
    WM_LAUNCH_CHECK("wm_excl_bwd");
    return WM_OK;
}
