// The per-frame convex mix of K attacked copies of a clip -- the "HYBRID ATTACKS" block of the reference's video model
// (models/IRNcrop_model.py:347-373): alpha = softmax(randn(B, T, K), dim = 2), attacked = sum_k alpha[..., k] * attacked_k, then
// clamp_with_grad + Quantization.  (The reference's loop :369 adds the bare weights and never multiplies them in; the mix above is what
// it means to compute.)  f32 tensors [N][frame] (N = B*T frames), weights [N][K], 1 <= K <= 8.
//   forward : acc = 0; for k in 0..K-1: acc = fma(w[n][k], x_k[i], acc), in that order; y = acc, or wm_clamp_quant(acc)   -- one launch
//   backward: gx_k[i] = w[n][k] * g[i] (the clamp and the quantisation are identities backwards)                            -- one launch
// Both are HBM streams of (K+1) * 4 bytes per element: K reads and a write, or a read and K writes.  The K tensor pointers travel by value in
// the kernel arguments (no pointer table in device memory).  A thread moves 16 bytes per tensor per turn of a grid-stride loop when every
// pointer is 16-byte aligned (4 bytes otherwise).  The weight row comes from the element index; frame need not be a multiple of 4, so a
// 16-byte vector may lie across the boundary of two (frame < 4: up to four) frames, and then each of its elements takes its own row.
#include "wm_common.h"

namespace {

constexpr int MIX_MAX_K = 8;
struct MixIn { const float* p[MIX_MAX_K]; };
struct MixOut { float* p[MIX_MAX_K]; };

template <int V> struct mix_vec;
template <> struct mix_vec<4> { typedef f32x4 type; };
template <> struct mix_vec<1> { typedef float type; };

template <int V> __device__ __forceinline__ void mix_load(const float* p, float (&v)[V]) {
    const typename mix_vec<V>::type t = *reinterpret_cast<const typename mix_vec<V>::type*>(p);
#pragma unroll
    for (int j = 0; j < V; ++j) v[j] = reinterpret_cast<const float*>(&t)[j];
}
template <int V> __device__ __forceinline__ void mix_store(float* p, const float (&v)[V]) {
    typename mix_vec<V>::type t;
#pragma unroll
    for (int j = 0; j < V; ++j) reinterpret_cast<float*>(&t)[j] = v[j];
    *reinterpret_cast<typename mix_vec<V>::type*>(p) = t;
}

// wv[k][j] = weight k of the frame that element j of a vector lies in; the vector starts at element `rem` (< frame) of frame `row`
template <int K, int V>
__device__ __forceinline__ void mix_weights(const float* __restrict__ w, size_t row, size_t rem, size_t frame, float (&wv)[K][V]) {
    if (V == 1 || rem + (V - 1) < frame) {   // the whole vector inside one frame
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const float a = w[row * K + k];
#pragma unroll
            for (int j = 0; j < V; ++j) wv[k][j] = a;
        }
    } else {                                  // across a frame boundary: walk the elements
        size_t r = row, m = rem;
#pragma unroll
        for (int j = 0; j < V; ++j) {
#pragma unroll
            for (int k = 0; k < K; ++k) wv[k][j] = w[r * K + k];
            if (++m == frame) { m = 0; ++r; }
        }
    }
}

__device__ __forceinline__ float mix_finish(float acc, int quant) { return quant ? wm_clamp_quant(acc) : acc; }

// A thread's vector index advances by the grid's `stride` vectors per turn; stride * V = qstride * frame + rstride (rstride < frame, from the
// host), so (row, rem) of the vector's first element follow with an add and a compare: one division per thread, none in the loop.
#define MIX_WALK_BEGIN                                                                   \
    const size_t nv = n / V, stride = (size_t)gridDim.x * 256;                           \
    size_t v = (size_t)blockIdx.x * 256 + threadIdx.x;                                   \
    size_t row = (v * V) / frame, rem = v * V - row * frame;                             \
    for (; v < nv; v += stride) {
#define MIX_WALK_END                                                                     \
        row += qstride; rem += rstride;                                                  \
        if (rem >= frame) { rem -= frame; ++row; }                                       \
    }

template <int K, int V>
__global__ __launch_bounds__(256) void mix_fwd_kernel(MixIn in, const float* __restrict__ w, float* __restrict__ y, size_t n, size_t frame,
                                                      size_t qstride, size_t rstride, int quant) {
    MIX_WALK_BEGIN
        float x[K][V], wv[K][V], o[V];
#pragma unroll
        for (int k = 0; k < K; ++k) mix_load<V>(in.p[k] + v * V, x[k]);
        mix_weights<K, V>(w, row, rem, frame, wv);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            float acc = 0.f;
#pragma unroll
            for (int k = 0; k < K; ++k) acc = __fmaf_rn(wv[k][j], x[k][j], acc);
            o[j] = mix_finish(acc, quant);
        }
        mix_store<V>(y + v * V, o);
    MIX_WALK_END
    if (V > 1) {   // the n % V elements behind the last whole vector
        const size_t i = nv * V + (size_t)blockIdx.x * 256 + threadIdx.x;
        if (i < n) {
            const size_t r = i / frame;
            float acc = 0.f;
#pragma unroll
            for (int k = 0; k < K; ++k) acc = __fmaf_rn(w[r * K + k], in.p[k][i], acc);
            y[i] = mix_finish(acc, quant);
        }
    }
}

template <int K, int V>
__global__ __launch_bounds__(256) void mix_bwd_kernel(const float* __restrict__ g, const float* __restrict__ w, MixOut out, size_t n, size_t frame,
                                                      size_t qstride, size_t rstride) {
    MIX_WALK_BEGIN
        float gv[V], wv[K][V];
        mix_load<V>(g + v * V, gv);
        mix_weights<K, V>(w, row, rem, frame, wv);
#pragma unroll
        for (int k = 0; k < K; ++k) {
            if (out.p[k] == nullptr) continue;   // this input needs no gradient
            float o[V];
#pragma unroll
            for (int j = 0; j < V; ++j) o[j] = wv[k][j] * gv[j];
            mix_store<V>(out.p[k] + v * V, o);
        }
    MIX_WALK_END
    if (V > 1) {
        const size_t i = nv * V + (size_t)blockIdx.x * 256 + threadIdx.x;
        if (i < n) {
            const size_t r = i / frame;
            const float gi = g[i];
#pragma unroll
            for (int k = 0; k < K; ++k)
                if (out.p[k] != nullptr) out.p[k][i] = w[r * K + k] * gi;
        }
    }
}

struct MixGrid { int blocks; size_t qstride, rstride; };

inline MixGrid mix_grid(size_t n, size_t frame, int V) {
    const size_t nv = n / (size_t)V, want = (nv + 255) / 256;
    MixGrid g;
    g.blocks = (int)(want > 2048 ? 2048 : (want < 1 ? 1 : want));   // (block 0 alone covers the < V elements of the tail)
    const size_t step = (size_t)g.blocks * 256 * (size_t)V;
    g.qstride = step / frame;
    g.rstride = step - g.qstride * frame;
    return g;
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

#define MIX_DISPATCH_K(K_, ...)                          \
    switch (K_) {                                        \
        case 1: { constexpr int KK = 1; __VA_ARGS__; } break; \
        case 2: { constexpr int KK = 2; __VA_ARGS__; } break; \
        case 3: { constexpr int KK = 3; __VA_ARGS__; } break; \
        case 4: { constexpr int KK = 4; __VA_ARGS__; } break; \
        case 5: { constexpr int KK = 5; __VA_ARGS__; } break; \
        case 6: { constexpr int KK = 6; __VA_ARGS__; } break; \
        case 7: { constexpr int KK = 7; __VA_ARGS__; } break; \
        default: { constexpr int KK = 8; __VA_ARGS__; } break; \
    }

}  // namespace

extern "C" int wm_mix_fwd(const float* const* xs_host, int K, const float* w, float* y, int N, size_t frame, int quant, void* stream) {
    WM_REQUIRE(K >= 1 && K <= MIX_MAX_K, WM_E_BADARG, "wm_mix_fwd: K = %d outside 1..%d", K, MIX_MAX_K);
    WM_REQUIRE(xs_host && w && y && N > 0 && frame > 0, WM_E_BADARG, "wm_mix_fwd: bad arguments");
    WM_REQUIRE(quant == 0 || quant == 1, WM_E_BADARG, "wm_mix_fwd: quant = %d (0 or 1)", quant);
    MixIn in = {};
    bool vec = aligned16(y);
    for (int k = 0; k < K; ++k) {
        WM_REQUIRE(xs_host[k] != nullptr, WM_E_BADARG, "wm_mix_fwd: input %d is null", k);
        in.p[k] = xs_host[k];
        vec = vec && aligned16(xs_host[k]);
    }
    const size_t n = (size_t)N * frame;
    const MixGrid g = mix_grid(n, frame, vec ? 4 : 1);
    hipStream_t s = (hipStream_t)stream;
    if (vec) {
        MIX_DISPATCH_K(K, mix_fwd_kernel<KK, 4><<<dim3(g.blocks), dim3(256), 0, s>>>(in, w, y, n, frame, g.qstride, g.rstride, quant));
    } else {
        MIX_DISPATCH_K(K, mix_fwd_kernel<KK, 1><<<dim3(g.blocks), dim3(256), 0, s>>>(in, w, y, n, frame, g.qstride, g.rstride, quant));
    }
    WM_LAUNCH_CHECK("wm_mix_fwd");
    return WM_OK;
}

extern "C" int wm_mix_bwd(const float* g, const float* w, float* const* gxs_host, int K, int N, size_t frame, void* stream) {
    WM_REQUIRE(K >= 1 && K <= MIX_MAX_K, WM_E_BADARG, "wm_mix_bwd: K = %d outside 1..%d", K, MIX_MAX_K);
    WM_REQUIRE(g && w && gxs_host && N > 0 && frame > 0, WM_E_BADARG, "wm_mix_bwd: bad arguments");
    MixOut out = {};
    bool vec = aligned16(g), any = false;
    for (int k = 0; k < K; ++k) {
        out.p[k] = gxs_host[k];
        if (gxs_host[k]) {
            any = true;
            vec = vec && aligned16(gxs_host[k]);
        }
    }
    if (!any) return WM_OK;   // no input needs a gradient: nothing to write
    const size_t n = (size_t)N * frame;
    const MixGrid gr = mix_grid(n, frame, vec ? 4 : 1);
    hipStream_t s = (hipStream_t)stream;
    if (vec) {
        MIX_DISPATCH_K(K, mix_bwd_kernel<KK, 4><<<dim3(gr.blocks), dim3(256), 0, s>>>(g, w, out, n, frame, gr.qstride, gr.rstride));
    } else {
        MIX_DISPATCH_K(K, mix_bwd_kernel<KK, 1><<<dim3(gr.blocks), dim3(256), 0, s>>>(g, w, out, n, frame, gr.qstride, gr.rstride));
    }
    WM_LAUNCH_CHECK("wm_mix_bwd");
    return WM_OK;
}
