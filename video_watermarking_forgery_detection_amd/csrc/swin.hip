// The Swin block's two operators that the conv / norm families cannot express (the reference's network/SUNet_detail.py): nn.LayerNorm over the
// channels of every token, and the (shifted-)window multi-head attention core.  Tensors are the token grids [B,H,W,CP] the layer toolkit
// already uses (CP = channels rounded up to 16, padding channels read as zero and written as zero).
//
// LayerNorm: one wave per token.  mean = sum(x) / C and var = sum((x - mean)^2) / C are two passes over the token's row in f32 (the second
// pass re-reads the row from cache: no E[x^2] - E[x]^2 cancellation), wave butterflies in a fixed order.  The backward's dx is one pass
// (one wave per token); dgamma / dbeta are per-workgroup partial rows in double over a slice of the tokens (one thread per channel), added
// in slice order by a finalise launch.  No atomics.
//
// Window attention: one 256-thread workgroup per (window, head).  The cyclic shift, window_partition, the head split, window_reverse and the
// reverse roll are the token's address: token n = (iy, ix) of window (wy, wx) lives at grid position ((wy ws + iy + shift) % H,
// (wx ws + ix + shift) % W) of qkv, out, g_out, g_qkv and the LSE alike.  The relative-position index and the shifted-window mask are
// computed from (ws, shift, H, W); no index or mask tensor is read.  The head dimension is walked in chunks of 32 channels (the MFMA depth),
// staged in LDS with their padding zeroed, so any hd works and the LDS footprint does not depend on it:
//   forward : S = scale Q K^T (+ table + mask) summed over the chunks -> row softmax in f32 (max subtracted), LSE saved -> O chunk = P V chunk
//   backward: S and dP = dO V^T summed over the chunks -> P = exp(S - LSE), dS = P (dP - rowsum(dP P)) -> per chunk dV = P^T dO,
//             dQ = scale dS K, dK = scale dS^T Q; the workgroup's dS summed by relative index (fixed order) is its partial table.
// Both products run on v_mfma_f32_16x16x32 for bf16 / f16 (P and dS rounded to the activation type as operands, f32 accumulate) and on f32
// FMAs for f32.  The operand fragments are gathered from LDS element by element through one accessor per matrix: the same accessors serve
// the f32 path, and a transposed operand is a different accessor, not a second copy.  (Wide / transposing fragment reads are a later step.)
#include "wm_reduce.h"

namespace {

// ------------------------------------------------------------------------------------------------------------------ LayerNorm
constexpr int LN_WAVES = 4;            // tokens per workgroup (one wave each)
constexpr size_t LN_SLICE = 64;        // tokens per partial row of dgamma / dbeta ...
constexpr size_t LN_MAX_SLICES = 256;  // ... unless that makes more than this many rows

inline size_t ln_slice(size_t tokens) {
    const size_t c = (tokens + LN_MAX_SLICES - 1) / LN_MAX_SLICES;
    return c > LN_SLICE ? c : LN_SLICE;
}
inline int ln_slices(size_t tokens) { return (int)((tokens + ln_slice(tokens) - 1) / ln_slice(tokens)); }

template <typename T>
__global__ __launch_bounds__(64 * LN_WAVES) void layernorm_fwd_kernel(const T* __restrict__ x, const float* __restrict__ gamma,
                                                                      const float* __restrict__ beta, T* __restrict__ y, float* __restrict__ mean,
                                                                      float* __restrict__ rstd, size_t tokens, int C, int CP, float eps) {
    const size_t t = (size_t)blockIdx.x * LN_WAVES + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (t >= tokens) return;
    const T* px = x + t * CP;
    float s = 0.f;
    for (int c = lane; c < C; c += 64) s += to_f32(px[c]);
    const float m = wave_sum(s) / (float)C;
    float q = 0.f;
    for (int c = lane; c < C; c += 64) {
        const float d = to_f32(px[c]) - m;
        q = __builtin_fmaf(d, d, q);
    }
    const float r = 1.f / sqrtf(wave_sum(q) / (float)C + eps);
    T* py = y + t * CP;
    for (int c = lane; c < CP; c += 64)
        py[c] = from_f32<T>(c < C ? __builtin_fmaf((to_f32(px[c]) - m) * r, gamma[c], beta[c]) : 0.f);
    if (lane == 0) {
        mean[t] = m;
        rstd[t] = r;
    }
}

// dx = rstd (g gamma - mean_c(g gamma) - xhat mean_c(g gamma xhat))
template <typename T>
__global__ __launch_bounds__(64 * LN_WAVES) void layernorm_bwd_dx_kernel(const T* __restrict__ x, const T* __restrict__ dy, const float* __restrict__ gamma,
                                                                         const float* __restrict__ mean, const float* __restrict__ rstd,
                                                                         T* __restrict__ dx, size_t tokens, int C, int CP) {
    const size_t t = (size_t)blockIdx.x * LN_WAVES + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (t >= tokens) return;
    const T* px = x + t * CP;
    const T* pg = dy + t * CP;
    const float m = mean[t], r = rstd[t];
    float s1 = 0.f, s2 = 0.f;
    for (int c = lane; c < C; c += 64) {
        const float gg = to_f32(pg[c]) * gamma[c];
        s1 += gg;
        s2 = __builtin_fmaf(gg, (to_f32(px[c]) - m) * r, s2);
    }
    const float m1 = wave_sum(s1) / (float)C, m2 = wave_sum(s2) / (float)C;
    T* pd = dx + t * CP;
    for (int c = lane; c < CP; c += 64) {
        float v = 0.f;
        if (c < C) {
            const float xh = (to_f32(px[c]) - m) * r;
            v = r * (__builtin_fmaf(-xh, m2, to_f32(pg[c]) * gamma[c] - m1));
        }
        pd[c] = from_f32<T>(v);
    }
}

// grid (ceil(C / 256), slices): thread = channel, walks its slice of the tokens in order; partial [slice][2][C] doubles
template <typename T>
__global__ __launch_bounds__(256) void layernorm_bwd_param_kernel(const T* __restrict__ x, const T* __restrict__ dy, const float* __restrict__ mean,
                                                                  const float* __restrict__ rstd, double* __restrict__ part, size_t tokens,
                                                                  size_t slice, int C, int CP) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    const size_t t0 = blockIdx.y * slice, t1 = t0 + slice < tokens ? t0 + slice : tokens;
    double sg = 0.0, sb = 0.0;
    for (size_t t = t0; t < t1; ++t) {
        const float g = to_f32(dy[t * CP + c]);
        const float xh = (to_f32(x[t * CP + c]) - mean[t]) * rstd[t];
        sg += (double)g * (double)xh;
        sb += (double)g;
    }
    part[((size_t)blockIdx.y * 2 + 0) * C + c] = sg;
    part[((size_t)blockIdx.y * 2 + 1) * C + c] = sb;
}

__global__ __launch_bounds__(256) void layernorm_bwd_finalize_kernel(const double* __restrict__ part, int S, int C, float* __restrict__ dgamma,
                                                                     float* __restrict__ dbeta) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    double sg = 0.0, sb = 0.0;
    for (int s = 0; s < S; ++s) {
        sg += part[((size_t)s * 2 + 0) * C + c];
        sb += part[((size_t)s * 2 + 1) * C + c];
    }
    dgamma[c] = (float)sg;
    dbeta[c] = (float)sb;
}

// ------------------------------------------------------------------------------------------------------------------ window attention
constexpr int WA_N = 64;    // tokens of a window at most (ws <= 8)
constexpr int WA_HC = 32;   // channels of a head per chunk = the MFMA depth
constexpr int WA_LDS = 65;  // row stride of the f32 score tiles (odd: a column walk touches every bank)
constexpr int WA_TBL = 225; // (2 ws - 1)^2 at most

struct WaGeo {
    int H, W, C, nH, hd, ws, shift, N, nWx, nWy, CP3, CPO;
    float scale;
};

// chunk row stride: 32 channels + a pad that makes the stride an odd number of dwords
template <typename T> struct wa_ld { static constexpr int v = WA_HC + (sizeof(T) == 4 ? 1 : 2); };

// C[row][col] = sum_k a(row, k) b(k, col) for rows < 16 MT, cols < 16 NT, k < 32 KS; st(row, col, value).  Every accessor must be defined
// (zero in the padding) on that whole range
template <typename T> struct WaMM {   // bf16 / f16: one 16x16 tile per wave and turn, v_mfma_f32_16x16x32
    template <typename FA, typename FB, typename FS> static __device__ __forceinline__ void run(int MT, int NT, int KS, FA a, FB b, FS st) {
        typedef typename h16<T>::x8 x8;
        const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, l15 = lane & 15, kq = (lane >> 4) * 8;
        for (int t = wave; t < MT * NT; t += 4) {
            const int r0 = (t / NT) * 16, c0 = (t % NT) * 16;
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            for (int ks = 0; ks < KS; ++ks) {
                x8 fa, fb;     // lane l: A[row l & 15][k = 8 (l >> 4) + j], B[k = 8 (l >> 4) + j][col l & 15]
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    fa[j] = (T)a(r0 + l15, ks * 32 + kq + j);
                    fb[j] = (T)b(ks * 32 + kq + j, c0 + l15);
                }
                acc = h16<T>::mfma16(fa, fb, acc);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) st(r0 + (lane >> 4) * 4 + r, c0 + l15, acc[r]);   // C: col = lane & 15, row = 4 (lane >> 4) + r
        }
    }
};
template <> struct WaMM<float> {      // f32: one output element per thread and turn, FMAs in k order
    template <typename FA, typename FB, typename FS> static __device__ __forceinline__ void run(int MT, int NT, int KS, FA a, FB b, FS st) {
        const int cols = NT * 16, n = MT * 16 * cols;
        for (int i = threadIdx.x; i < n; i += 256) {
            const int row = i / cols, col = i % cols;
            float acc = 0.f;
            for (int k = 0; k < KS * 32; ++k) acc = __builtin_fmaf(a(row, k), b(k, col), acc);
            st(row, col, acc);
        }
    }
};

struct WaWin {
    int b, y0, x0, head;   // sample, the window's first row / column on the SHIFTED grid, head
};

// offset (in tokens) of window token n on the un-shifted grid
__device__ __forceinline__ size_t wa_token(const WaGeo& g, const WaWin& w, int n) {
    int y = w.y0 + n / g.ws + g.shift, x = w.x0 + n % g.ws + g.shift;
    y = y >= g.H ? y - g.H : y;
    x = x >= g.W ? x - g.W : x;
    return ((size_t)w.b * g.H + y) * g.W + x;
}
// region id of a position on the shifted grid: the reference's img_mask (h_slices x w_slices: [0, L - ws), [L - ws, L - shift), [L - shift, L))
__device__ __forceinline__ int wa_region(const WaGeo& g, const WaWin& w, int n) {
    const int y = w.y0 + n / g.ws, x = w.x0 + n % g.ws;
    const int ry = y < g.H - g.ws ? 0 : (y < g.H - g.shift ? 1 : 2), rx = x < g.W - g.ws ? 0 : (x < g.W - g.shift ? 1 : 2);
    return ry * 3 + rx;
}
__device__ __forceinline__ int wa_rel(const WaGeo& g, int i, int j) {
    return (i / g.ws - j / g.ws + g.ws - 1) * (2 * g.ws - 1) + (i % g.ws - j % g.ws + g.ws - 1);
}

// chunk [c0, c0 + 32) of q / k / v (which = 0 / 1 / 2) of this (window, head) -> dst [64][LD], zeros beyond N and hd
template <typename T>
__device__ __forceinline__ void wa_stage(const WaGeo& g, const WaWin& w, const T* __restrict__ src, int stride, int chan0, int c0, T* dst) {
    constexpr int LD = wa_ld<T>::v;
    for (int i = threadIdx.x; i < WA_N * WA_HC; i += 256) {
        const int n = i / WA_HC, d = i % WA_HC;
        T v = from_f32<T>(0.f);
        if (n < g.N && c0 + d < g.hd) v = src[wa_token(g, w, n) * stride + chan0 + c0 + d];
        dst[n * LD + d] = v;
    }
}

__device__ __forceinline__ WaWin wa_window(const WaGeo& g) {
    WaWin w;
    const int per = g.nWy * g.nWx, wi = blockIdx.x % per;
    w.b = blockIdx.x / per;
    w.y0 = (wi / g.nWx) * g.ws;
    w.x0 = (wi % g.nWx) * g.ws;
    w.head = blockIdx.y;
    return w;
}

// S += scale Q K^T of one chunk, then (last chunk) + table + mask.  sS [64][65]
template <typename T>
__device__ __forceinline__ void wa_scores(const WaGeo& g, const WaWin& w, const T* sQ, const T* sK, float* sS, const float* sTbl, bool first, bool last) {
    constexpr int LD = wa_ld<T>::v;
    const int MT = (g.N + 15) / 16;
    WaMM<T>::run(MT, MT, 1,
                 [&](int r, int k) { return to_f32(sQ[r * LD + k]); },
                 [&](int k, int c) { return to_f32(sK[c * LD + k]); },
                 [&](int r, int c, float v) {
                     float s = g.scale * v + (first ? 0.f : sS[r * WA_LDS + c]);
                     if (last && r < g.N && c < g.N) {
                         s += sTbl[wa_rel(g, r, c)];
                         if (g.shift > 0 && wa_region(g, w, r) != wa_region(g, w, c)) s += -100.f;
                     }
                     sS[r * WA_LDS + c] = s;
                 });
}

__device__ __forceinline__ void wa_load_table(const WaGeo& g, const WaWin& w, const float* __restrict__ table, float* sTbl) {
    const int nt = (2 * g.ws - 1) * (2 * g.ws - 1);
    for (int i = threadIdx.x; i < nt; i += 256) sTbl[i] = table[(size_t)i * g.nH + w.head];
}

template <typename T>
__global__ __launch_bounds__(256) void winattn_fwd_kernel(const T* __restrict__ qkv, const float* __restrict__ table, T* __restrict__ out,
                                                          float* __restrict__ lse, WaGeo g) {
    constexpr int LD = wa_ld<T>::v;
    __shared__ __attribute__((aligned(16))) float sS[WA_N * WA_LDS];
    __shared__ __attribute__((aligned(16))) T sA[WA_N * LD];
    __shared__ __attribute__((aligned(16))) T sB[WA_N * LD];
    __shared__ float sTbl[WA_TBL];
    const WaWin w = wa_window(g);
    const int nchunk = (g.hd + WA_HC - 1) / WA_HC, MT = (g.N + 15) / 16, KS = (g.N + 31) / 32;
    wa_load_table(g, w, table, sTbl);
    for (int c = 0; c < nchunk; ++c) {
        __syncthreads();
        wa_stage<T>(g, w, qkv, g.CP3, 0 * g.C + w.head * g.hd, c * WA_HC, sA);
        wa_stage<T>(g, w, qkv, g.CP3, 1 * g.C + w.head * g.hd, c * WA_HC, sB);
        __syncthreads();
        wa_scores<T>(g, w, sA, sB, sS, sTbl, c == 0, c == nchunk - 1);
    }
    __syncthreads();
    {   // row softmax: 4 neighbouring lanes per row; the whole [64][64] tile is written (zeros outside N x N)
        const int r = threadIdx.x >> 2, p = threadIdx.x & 3;
        float m = -INFINITY;
        if (r < g.N)
            for (int j = p; j < g.N; j += 4) m = fmaxf(m, sS[r * WA_LDS + j]);
        m = fmaxf(m, __shfl_xor(m, 1, 64));
        m = fmaxf(m, __shfl_xor(m, 2, 64));
        float s = 0.f;
        if (r < g.N)
            for (int j = p; j < g.N; j += 4) {
                const float e = expf(sS[r * WA_LDS + j] - m);
                sS[r * WA_LDS + j] = e;
                s += e;
            }
        s += __shfl_xor(s, 1, 64);
        s += __shfl_xor(s, 2, 64);
        const float inv = r < g.N ? 1.f / s : 0.f;
        for (int j = p; j < WA_N; j += 4) sS[r * WA_LDS + j] = (r < g.N && j < g.N) ? sS[r * WA_LDS + j] * inv : 0.f;
        if (r < g.N && p == 0) lse[((size_t)w.b * g.nH + w.head) * g.H * g.W + (wa_token(g, w, r) - (size_t)w.b * g.H * g.W)] = m + logf(s);
    }
    for (int c = 0; c < nchunk; ++c) {
        __syncthreads();
        wa_stage<T>(g, w, qkv, g.CP3, 2 * g.C + w.head * g.hd, c * WA_HC, sA);
        __syncthreads();
        WaMM<T>::run(MT, WA_HC / 16, KS,
                     [&](int r, int k) { return sS[r * WA_LDS + k]; },
                     [&](int k, int d) { return to_f32(sA[k * LD + d]); },
                     [&](int r, int d, float v) {
                         if (r < g.N && c * WA_HC + d < g.hd) out[wa_token(g, w, r) * g.CPO + w.head * g.hd + c * WA_HC + d] = from_f32<T>(v);
                     });
    }
    if (w.head == g.nH - 1 && g.CPO > g.C) {      // the padding channels of this window's tokens
        const int np = g.CPO - g.C;
        for (int i = threadIdx.x; i < g.N * np; i += 256) out[wa_token(g, w, i / np) * g.CPO + g.C + i % np] = from_f32<T>(0.f);
    }
}

template <typename T>
__global__ __launch_bounds__(256) void winattn_bwd_kernel(const T* __restrict__ gout, const T* __restrict__ qkv, const float* __restrict__ table,
                                                          const float* __restrict__ lse, T* __restrict__ gqkv, float* __restrict__ part, WaGeo g) {
    constexpr int LD = wa_ld<T>::v;
    __shared__ __attribute__((aligned(16))) float sS[WA_N * WA_LDS];   // S, then P
    __shared__ __attribute__((aligned(16))) float sD[WA_N * WA_LDS];   // dP, then dS
    __shared__ __attribute__((aligned(16))) T sQ[WA_N * LD];           // Q; dO in the second half of a first-pass chunk
    __shared__ __attribute__((aligned(16))) T sK[WA_N * LD];           // K; V in the second half of a first-pass chunk
    __shared__ __attribute__((aligned(16))) T sG[WA_N * LD];           // dO (second pass)
    __shared__ float sTbl[WA_TBL];
    const WaWin w = wa_window(g);
    const int nchunk = (g.hd + WA_HC - 1) / WA_HC, MT = (g.N + 15) / 16, KS = (g.N + 31) / 32;
    const int chq = 0 * g.C + w.head * g.hd, chk = 1 * g.C + w.head * g.hd, chv = 2 * g.C + w.head * g.hd;
    wa_load_table(g, w, table, sTbl);
    for (int c = 0; c < nchunk; ++c) {
        __syncthreads();
        wa_stage<T>(g, w, qkv, g.CP3, chq, c * WA_HC, sQ);
        wa_stage<T>(g, w, qkv, g.CP3, chk, c * WA_HC, sK);
        __syncthreads();
        wa_scores<T>(g, w, sQ, sK, sS, sTbl, c == 0, c == nchunk - 1);
        __syncthreads();
        wa_stage<T>(g, w, gout, g.CPO, w.head * g.hd, c * WA_HC, sQ);
        wa_stage<T>(g, w, qkv, g.CP3, chv, c * WA_HC, sK);
        __syncthreads();
        const bool first = c == 0;
        WaMM<T>::run(MT, MT, 1,                                  // dP += dO V^T
                     [&](int r, int k) { return to_f32(sQ[r * LD + k]); },
                     [&](int k, int j) { return to_f32(sK[j * LD + k]); },
                     [&](int r, int j, float v) { sD[r * WA_LDS + j] = v + (first ? 0.f : sD[r * WA_LDS + j]); });
    }
    __syncthreads();
    {   // P = exp(S - LSE), dS = P (dP - rowsum(dP P)); both [64][64] tiles written whole (zeros outside N x N)
        const int r = threadIdx.x >> 2, p = threadIdx.x & 3;
        const float l = r < g.N ? lse[((size_t)w.b * g.nH + w.head) * g.H * g.W + (wa_token(g, w, r) - (size_t)w.b * g.H * g.W)] : 0.f;
        float s = 0.f;
        if (r < g.N)
            for (int j = p; j < g.N; j += 4) {
                const float pv = expf(sS[r * WA_LDS + j] - l);
                sS[r * WA_LDS + j] = pv;
                s = __builtin_fmaf(pv, sD[r * WA_LDS + j], s);
            }
        s += __shfl_xor(s, 1, 64);
        s += __shfl_xor(s, 2, 64);
        for (int j = p; j < WA_N; j += 4) {
            const bool in = r < g.N && j < g.N;
            const float pv = in ? sS[r * WA_LDS + j] : 0.f;
            sS[r * WA_LDS + j] = pv;
            sD[r * WA_LDS + j] = in ? pv * (sD[r * WA_LDS + j] - s) : 0.f;
        }
    }
    __syncthreads();
    {   // this workgroup's row of the table gradient: dS summed by relative index, (i, j) in row-major order
        const int span = 2 * g.ws - 1, nt = span * span;
        for (int t = threadIdx.x; t < nt; t += 256) {
            const int dy = t / span - (g.ws - 1), dx = t % span - (g.ws - 1);
            float acc = 0.f;
            for (int iy = dy > 0 ? dy : 0; iy < g.ws + (dy < 0 ? dy : 0); ++iy)
                for (int ix = dx > 0 ? dx : 0; ix < g.ws + (dx < 0 ? dx : 0); ++ix)
                    acc += sD[(iy * g.ws + ix) * WA_LDS + (iy - dy) * g.ws + (ix - dx)];
            part[((size_t)blockIdx.x * g.nH + w.head) * nt + t] = acc;
        }
    }
    for (int c = 0; c < nchunk; ++c) {
        __syncthreads();
        wa_stage<T>(g, w, qkv, g.CP3, chq, c * WA_HC, sQ);
        wa_stage<T>(g, w, qkv, g.CP3, chk, c * WA_HC, sK);
        wa_stage<T>(g, w, gout, g.CPO, w.head * g.hd, c * WA_HC, sG);
        __syncthreads();
        const int d0 = c * WA_HC;
        auto store = [&](int chan, float mul) {
            return [&g, &w, gqkv, chan, mul, d0](int r, int d, float v) {
                if (r < g.N && d0 + d < g.hd) gqkv[wa_token(g, w, r) * g.CP3 + chan + d0 + d] = from_f32<T>(mul * v);
            };
        };
        WaMM<T>::run(MT, WA_HC / 16, KS,                         // dV = P^T dO
                     [&](int j, int i) { return sS[i * WA_LDS + j]; },
                     [&](int i, int d) { return to_f32(sG[i * LD + d]); }, store(chv, 1.f));
        WaMM<T>::run(MT, WA_HC / 16, KS,                         // dQ = scale dS K
                     [&](int i, int j) { return sD[i * WA_LDS + j]; },
                     [&](int j, int d) { return to_f32(sK[j * LD + d]); }, store(chq, g.scale));
        WaMM<T>::run(MT, WA_HC / 16, KS,                         // dK = scale dS^T Q
                     [&](int j, int i) { return sD[i * WA_LDS + j]; },
                     [&](int i, int d) { return to_f32(sQ[i * LD + d]); }, store(chk, g.scale));
    }
    if (w.head == g.nH - 1 && g.CP3 > 3 * g.C) {
        const int np = g.CP3 - 3 * g.C;
        for (int i = threadIdx.x; i < g.N * np; i += 256) gqkv[wa_token(g, w, i / np) * g.CP3 + 3 * g.C + i % np] = from_f32<T>(0.f);
    }
}

// one thread per (relative index, head): the partial rows of every (sample, window) in order
__global__ __launch_bounds__(256) void winattn_table_finalize_kernel(const float* __restrict__ part, int nwin, int nH, int nt, float* __restrict__ gtable) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nt * nH) return;
    const int t = i / nH, h = i % nH;
    double acc = 0.0;
    for (int wdx = 0; wdx < nwin; ++wdx) acc += (double)part[((size_t)wdx * nH + h) * nt + t];
    gtable[(size_t)t * nH + h] = (float)acc;
}

int ln_check(const char* name, size_t tokens, int C, int CP, int dtype) {
    WM_REQUIRE(tokens > 0 && C > 0 && C <= CP && CP % 16 == 0, WM_E_BADARG, "%s: bad shape (tokens %zu, C %d, CP %d)", name, tokens, C, CP);
    WM_REQUIRE(dtype == WM_F32 || dtype == WM_BF16 || dtype == WM_F16, WM_E_BADARG, "%s: unsupported dtype %d", name, dtype);
    WM_REQUIRE((tokens + LN_WAVES - 1) / LN_WAVES <= 0x7fffffffu, WM_E_SHAPE, "%s: %zu tokens exceed the grid", name, tokens);
    return 0;
}

int wa_check(const char* name, int B, int H, int W, int C, int nH, int ws, int shift, int CP3, int CPO, int dtype, WaGeo& g) {
    WM_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0 && nH > 0 && nH <= 65535, WM_E_BADARG, "%s: bad shape (B %d, H %d, W %d, C %d, heads %d)", name, B, H, W, C, nH);
    WM_REQUIRE(dtype == WM_F32 || dtype == WM_BF16 || dtype == WM_F16, WM_E_BADARG, "%s: unsupported dtype %d", name, dtype);
    WM_REQUIRE(C % nH == 0 && C / nH <= 96, WM_E_SHAPE, "%s: %d channels over %d heads (a head has at most 96 channels, and C must divide)", name, C, nH);
    WM_REQUIRE(ws >= 1 && ws <= 8 && H % ws == 0 && W % ws == 0, WM_E_SHAPE, "%s: window %d on a %d x %d grid (1 <= ws <= 8, H and W multiples of ws)", name, ws, H, W);
    WM_REQUIRE(shift >= 0 && shift < ws, WM_E_SHAPE, "%s: shift %d outside [0, %d)", name, shift, ws);
    WM_REQUIRE(CP3 >= 3 * C && CPO >= C && CP3 % 16 == 0 && CPO % 16 == 0, WM_E_BADARG, "%s: channel strides %d / %d for 3 x %d / %d channels", name, CP3, CPO, C, C);
    WM_REQUIRE((long)B * (H / ws) * (W / ws) <= 0x7fffffffL, WM_E_SHAPE, "%s: too many windows", name);
    g = WaGeo{H, W, C, nH, C / nH, ws, shift, ws * ws, W / ws, H / ws, CP3, CPO, 0.f};
    return 0;
}

}  // namespace

extern "C" size_t wm_layernorm_scratch_doubles(size_t tokens, int C) { return (tokens > 0 && C > 0) ? (size_t)ln_slices(tokens) * 2 * C : 0; }

extern "C" int wm_layernorm_fwd(const void* x, const float* gamma, const float* beta, void* y, float* mean, float* rstd, size_t tokens, int C,
                                int CP, float eps, int dtype, void* stream) {
    WM_REQUIRE(x && gamma && beta && y && mean && rstd && eps >= 0.f, WM_E_BADARG, "wm_layernorm_fwd: null pointer or negative eps");
    if (int rc = ln_check("wm_layernorm_fwd", tokens, C, CP, dtype)) return rc;
    WM_DISPATCH_DTYPE(dtype, "wm_layernorm_fwd", {
        hipLaunchKernelGGL(layernorm_fwd_kernel<T>, dim3((unsigned)((tokens + LN_WAVES - 1) / LN_WAVES)), dim3(64 * LN_WAVES), 0, (hipStream_t)stream, (const T*)x,
                           gamma, beta, (T*)y, mean, rstd, tokens, C, CP, eps);
    });
    WM_LAUNCH_CHECK("wm_layernorm_fwd");
    return 0;
}

extern "C" int wm_layernorm_bwd(const void* x, const void* dy, const float* gamma, const float* mean, const float* rstd, void* dx, float* dgamma,
                                float* dbeta, double* scratch, size_t tokens, int C, int CP, int dtype, void* stream) {
    WM_REQUIRE(x && dy && gamma && mean && rstd && dx, WM_E_BADARG, "wm_layernorm_bwd: null pointer");
    WM_REQUIRE((dgamma == nullptr) == (dbeta == nullptr) && (dgamma == nullptr || scratch), WM_E_BADARG,
               "wm_layernorm_bwd: dgamma and dbeta come together, with their scratch");
    if (int rc = ln_check("wm_layernorm_bwd", tokens, C, CP, dtype)) return rc;
    const int S = ln_slices(tokens);
    WM_DISPATCH_DTYPE(dtype, "wm_layernorm_bwd", {
        hipLaunchKernelGGL(layernorm_bwd_dx_kernel<T>, dim3((unsigned)((tokens + LN_WAVES - 1) / LN_WAVES)), dim3(64 * LN_WAVES), 0, (hipStream_t)stream,
                           (const T*)x, (const T*)dy, gamma, mean, rstd, (T*)dx, tokens, C, CP);
        if (dgamma)
            hipLaunchKernelGGL(layernorm_bwd_param_kernel<T>, dim3(wm_cdiv(C, 256), S), dim3(256), 0, (hipStream_t)stream, (const T*)x, (const T*)dy, mean, rstd,
                               scratch, tokens, ln_slice(tokens), C, CP);
    });
    WM_LAUNCH_CHECK("wm_layernorm_bwd");
    if (dgamma) {
        hipLaunchKernelGGL(layernorm_bwd_finalize_kernel, dim3(wm_cdiv(C, 256)), dim3(256), 0, (hipStream_t)stream, scratch, S, C, dgamma, dbeta);
        WM_LAUNCH_CHECK("wm_layernorm_bwd (finalise)");
    }
    return 0;
}

extern "C" size_t wm_winattn_scratch_floats(int B, int H, int W, int nH, int ws) {
    if (B <= 0 || H <= 0 || W <= 0 || nH <= 0 || ws < 1 || ws > 8 || H % ws || W % ws) return 0;
    return (size_t)B * (H / ws) * (W / ws) * nH * (2 * ws - 1) * (2 * ws - 1);
}

extern "C" int wm_winattn_fwd(const void* qkv, const float* table, void* out, float* lse, int B, int H, int W, int C, int nH, int ws, int shift,
                              float scale, int CP3, int CPO, int dtype, void* stream) {
    WM_REQUIRE(qkv && table && out && lse, WM_E_BADARG, "wm_winattn_fwd: null pointer");
    WaGeo g;
    if (int rc = wa_check("wm_winattn_fwd", B, H, W, C, nH, ws, shift, CP3, CPO, dtype, g)) return rc;
    g.scale = scale;
    WM_DISPATCH_DTYPE(dtype, "wm_winattn_fwd", {
        hipLaunchKernelGGL(winattn_fwd_kernel<T>, dim3(B * g.nWy * g.nWx, nH), dim3(256), 0, (hipStream_t)stream, (const T*)qkv, table, (T*)out, lse, g);
    });
    WM_LAUNCH_CHECK("wm_winattn_fwd");
    return 0;
}

extern "C" int wm_winattn_bwd(const void* g_out, const void* qkv, const float* table, const float* lse, void* g_qkv, float* g_table, float* scratch,
                              int B, int H, int W, int C, int nH, int ws, int shift, float scale, int CP3, int CPO, int dtype, void* stream) {
    WM_REQUIRE(g_out && qkv && table && lse && g_qkv && g_table && scratch, WM_E_BADARG, "wm_winattn_bwd: null pointer");
    WaGeo g;
    if (int rc = wa_check("wm_winattn_bwd", B, H, W, C, nH, ws, shift, CP3, CPO, dtype, g)) return rc;
    g.scale = scale;
    const int nwin = B * g.nWy * g.nWx, nt = (2 * ws - 1) * (2 * ws - 1);
    WM_DISPATCH_DTYPE(dtype, "wm_winattn_bwd", {
        hipLaunchKernelGGL(winattn_bwd_kernel<T>, dim3(nwin, nH), dim3(256), 0, (hipStream_t)stream, (const T*)g_out, (const T*)qkv, table, lse, (T*)g_qkv,
                           scratch, g);
    });
    WM_LAUNCH_CHECK("wm_winattn_bwd");
    hipLaunchKernelGGL(winattn_table_finalize_kernel, dim3(wm_cdiv((long)nt * nH, 256)), dim3(256), 0, (hipStream_t)stream, scratch, nwin, nH, nt, g_table);
    WM_LAUNCH_CHECK("wm_winattn_bwd (table)");
    return 0;
}
