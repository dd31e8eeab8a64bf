// JpegCompression (HiDDeN's "JPEG-Drop" attack, noise_layers/jpeg_compression.py:65-159) on [B,3,H,W] f32 NCHW planes (gfx950),
// forward and its exact adjoint, one launch each.  Per 8x8 block of the image zero-padded to a multiple of 8:
//     out = yuv2rgb . IDCT2 . mask . DCT2 . rgb2yuv (x)
//   rgb2yuv / yuv2rgb : the analog YUV coefficients of the reference (.299 .587 .114 / -.14713 -.28886 .436 / .615 -.51499 -.10001)
//   DCT2              : unnormalised DCT-II, C[k][n] = cos(pi/8 (n + 1/2) k), on rows and columns (gen_filters(8, 8, dct_coeff))
//   IDCT2             : D[k][n] = (-1/2 [n == 0] + cos(pi/8 (k + 1/2) n)) sqrt(1/16), spatial k from coefficient n (idct_coeff)
//   mask              : the first yuv_keep_weights[c] coefficients of the zig-zag order of get_jpeg_yuv_filter_mask, per channel
// then un-padding.  The backward is the transpose, x-bar = rgb2yuv^T . DCT2^T . mask . IDCT2^T . yuv2rgb^T (g) on the zero-padded g:
// the same kernel with the transposed matrices (set up on the host).  HBM-bound: 24 B/px (one 3-channel read, one write); the four
// 8-point transforms run out of LDS.  Workgroup = 4 horizontally adjacent blocks: 8 rows x 32 columns, one thread per pixel.
#include <math.h>

#include "wm_common.h"

namespace {

struct JdMats {
    float a[9];        // colour transform applied first (rgb2yuv, or yuv2rgb^T in the backward)
    float t1[64];      // first 8-point transform, t1[k*8 + n] (C, or D^T)
    float t2[64];      // second (D, or C^T)
    float b[9];        // colour transform applied last (yuv2rgb, or rgb2yuv^T)
    uint64_t keep[3];  // coefficient mask per channel, bit ky*8 + kx
};

__global__ __launch_bounds__(256) void jpeg_drop_kernel(const float* __restrict__ x, float* __restrict__ y, int H, int W, int Hb, int Wb,
                                                        JdMats m) {
    __shared__ float s[3][8][33];
    const int t = threadIdx.x, r = t >> 5, col = t & 31, j = col >> 3, cc = col & 7;
    const int bx = blockIdx.x * 4 + j, h = blockIdx.y * 8 + r, w = bx * 8 + cc;
    const size_t plane = (size_t)H * W;
    const float* xb = x + (size_t)blockIdx.z * 3 * plane;
    const bool in = bx < Wb && h < H && w < W;
    float v[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = in ? xb[c * plane + (size_t)h * W + w] : 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) s[c][r][col] = m.a[c * 3] * v[0] + m.a[c * 3 + 1] * v[1] + m.a[c * 3 + 2] * v[2];
    __syncthreads();
    // pass 1: along the columns of the block (row frequency k = r)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float acc = 0.f;
#pragma unroll
        for (int n = 0; n < 8; ++n) acc += m.t1[r * 8 + n] * s[c][n][col];
        v[c] = acc;
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 3; ++c) s[c][r][col] = v[c];
    __syncthreads();
    // pass 2: along the rows (column frequency cc), then the coefficient mask
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float acc = 0.f;
#pragma unroll
        for (int n = 0; n < 8; ++n) acc += m.t1[cc * 8 + n] * s[c][r][j * 8 + n];
        v[c] = (m.keep[c] >> (r * 8 + cc)) & 1u ? acc : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 3; ++c) s[c][r][col] = v[c];
    __syncthreads();
    // pass 3 and 4: the second transform, columns then rows
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float acc = 0.f;
#pragma unroll
        for (int n = 0; n < 8; ++n) acc += m.t2[r * 8 + n] * s[c][n][col];
        v[c] = acc;
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 3; ++c) s[c][r][col] = v[c];
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float acc = 0.f;
#pragma unroll
        for (int n = 0; n < 8; ++n) acc += m.t2[cc * 8 + n] * s[c][r][j * 8 + n];
        v[c] = acc;
    }
    if (!in) return;
    float* yb = y + (size_t)blockIdx.z * 3 * plane;
#pragma unroll
    for (int c = 0; c < 3; ++c) yb[c * plane + (size_t)h * W + w] = m.b[c * 3] * v[0] + m.b[c * 3 + 1] * v[1] + m.b[c * 3 + 2] * v[2];
}

const double RGB2YUV[9] = {0.299, 0.587, 0.114, -0.14713, -0.28886, 0.436, 0.615, -0.51499, -0.10001};
const double YUV2RGB[9] = {1.0, 0.0, 1.13983, 1.0, -0.39465, -0.58060, 1.0, 2.03211, 0.0};

// zig-zag order of get_jpeg_yuv_filter_mask: (x, y) sorted by (x + y, -y if (x + y) odd else y); mask[x][y] = 1 for the first `count`
uint64_t zigzag_keep(int count) {
    uint64_t bits = 0;
    int taken = 0;
    for (int d = 0; d <= 14 && taken < count; ++d) {
        for (int i = 0; i < 8 && taken < count; ++i) {
            const int yy = (d % 2) ? d - i : i;   // odd diagonal: y descending (key -y), even: ascending
            const int xx = d - yy;
            if (xx < 0 || xx > 7 || yy < 0 || yy > 7) continue;
            bits |= 1ull << (xx * 8 + yy);
            ++taken;
        }
    }
    return bits;
}

JdMats make_mats(int adjoint, const int* keep) {
    float C[64], D[64];
    const double pi = 3.14159265358979323846;
    for (int k = 0; k < 8; ++k)
        for (int n = 0; n < 8; ++n) {
            C[k * 8 + n] = (float)cos(pi / 8 * (n + 0.5) * k);
            D[k * 8 + n] = (float)(((n == 0) ? -0.5 : 0.0) + cos(pi / 8 * (k + 0.5) * n)) * (float)sqrt(1.0 / 16.0);
        }
    JdMats m;
    for (int i = 0; i < 3; ++i)
        for (int q = 0; q < 3; ++q) {
            m.a[i * 3 + q] = (float)(adjoint ? YUV2RGB[q * 3 + i] : RGB2YUV[i * 3 + q]);
            m.b[i * 3 + q] = (float)(adjoint ? RGB2YUV[q * 3 + i] : YUV2RGB[i * 3 + q]);
        }
    for (int k = 0; k < 8; ++k)
        for (int n = 0; n < 8; ++n) {
            m.t1[k * 8 + n] = adjoint ? D[n * 8 + k] : C[k * 8 + n];
            m.t2[k * 8 + n] = adjoint ? C[n * 8 + k] : D[k * 8 + n];
        }
    for (int c = 0; c < 3; ++c) m.keep[c] = zigzag_keep(keep[c]);
    return m;
}

int launch(const char* name, const float* x, float* y, int B, int H, int W, const int* keep, int adjoint, void* stream) {
    WM_REQUIRE(x && y && keep && B > 0 && H > 0 && W > 0, WM_E_BADARG, "%s: bad arguments", name);
    for (int c = 0; c < 3; ++c) WM_REQUIRE(keep[c] >= 0 && keep[c] <= 64, WM_E_BADARG, "%s: keep count %d not in [0, 64]", name, keep[c]);
    WM_REQUIRE(B < 65536 && H < 65536 * 8, WM_E_SHAPE, "%s: shape too large", name);
    const int Hb = (H + 7) / 8, Wb = (W + 7) / 8;
    const JdMats m = make_mats(adjoint, keep);
    hipLaunchKernelGGL(jpeg_drop_kernel, dim3((unsigned)((Wb + 3) / 4), (unsigned)Hb, (unsigned)B), dim3(256), 0, (hipStream_t)stream, x, y,
                       H, W, Hb, Wb, m);
    WM_LAUNCH_CHECK(name);
    return WM_OK;
}

}  // namespace

extern "C" int wm_jpeg_drop_fwd(const float* x, float* y, int B, int H, int W, const int* keep, void* stream) {
    return launch("wm_jpeg_drop_fwd", x, y, B, H, W, keep, 0, stream);
}

extern "C" int wm_jpeg_drop_bwd(const float* gy, float* gx, int B, int H, int W, const int* keep, void* stream) {
    return launch("wm_jpeg_drop_bwd", gy, gx, B, H, W, keep, 1, stream);
}
