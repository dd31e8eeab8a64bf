// Two-source mask head: the full-resolution tail of the tamper localiser (models/networks.py UNetDiscriminator, the reference's
// networks.py:1005-1013,1100-1110): decoder_0 = nn.Conv2d(2 dim, Cout, 1) on torch.cat((e0, d1), 1), the sigmoid, NCHW f32 out --
//   out[b,co,p] = act(bias[co] + sum_c w[co,c] a[b,p,c] + sum_c w[co,na+c] b[b,p,c])
// read from the two NHWC sources IN PLACE (each with its own channel stride): no concatenated tensor, no 16-wide padded logit tensor, no
// activation pass, no layout pass.  Cout <= 4, so like heads.hip this is a bandwidth-bound reduction, not a GEMM: G lanes share one pixel
// (G = the larger source's 16-byte vectors per pixel, rounded up to a power of two), each lane loads one 16-byte channel vector of either
// source (a wave reads 64/G whole pixels of each, contiguous), forms its partial dot products in f32 and the lanes of a pixel combine with
// wave shuffles; one lane per pixel and output channel stores the f32 plane value (consecutive pixels, consecutive addresses).
// The backward reads gout (and, chained through the sigmoid, the saved out) the same way, writes ga / gb as whole 16-byte vectors -- padding
// channels zero -- and leaves per-workgroup partial sums of dw and dbias in double; wm_head2_finalize adds them in double in a fixed order
// and rounds once.  No atomics anywhere: two runs give the same bits.  LDS only for the workgroup's reduction.
#include "wm_common.h"
#include "wm_reduce.h"

namespace {

constexpr int MAXG = 16;    // lanes per pixel: a source's channel stride is at most 16 vectors of 16 bytes (128 channels at 16 bits, 64 in f32)
constexpr int MAXCO = 4;

// one source's share of a lane: its 16-byte vector of the pixel row (vv < V) and the COUT filter rows over those channels (0 past n)
template <typename T, int COUT> struct Src {
    static constexpr int VE = vec16<T>::N;
    const T* p; int ld, n, V; bool mine;
    float w[COUT][VE];
    __device__ __forceinline__ void init(const T* p_, int ld_, int n_, const float* __restrict__ wrow, int nab, int vv) {
        p = p_; ld = ld_; n = n_; V = ld_ / VE; mine = vv < V;
#pragma unroll
        for (int co = 0; co < COUT; ++co)
#pragma unroll
            for (int e = 0; e < VE; ++e) w[co][e] = (mine && vv * VE + e < n) ? wrow[co * nab + vv * VE + e] : 0.f;
    }
    __device__ __forceinline__ vec16<T> load(size_t pix, int vv) const {   // (a lane without a vector of this source re-reads vector 0: in bounds, unused)
        return *reinterpret_cast<const vec16<T>*>(p + pix * ld + (mine ? vv : 0) * VE);
    }
    // the value of channel vv*VE + e as the head sees it: padding channels are ignored, whatever they hold
    __device__ __forceinline__ float val(const vec16<T>& v, int vv, int e) const { return (mine && vv * VE + e < n) ? v.get(e) : 0.f; }
};

__device__ __forceinline__ float sigmoidf(float v) { return 1.f / (1.f + expf(-v)); }

template <typename T, int COUT>
__global__ __launch_bounds__(256) void head2_fwd_kernel(const T* __restrict__ a, int lda, int na, const T* __restrict__ b, int ldb, int nb,
                                                        const float* __restrict__ w, const float* __restrict__ bias, float* __restrict__ out,
                                                        size_t npix, size_t hw, int G, int act) {
    constexpr int VE = vec16<T>::N;
    const int PPB = 256 / G, vv = threadIdx.x % G, ps = threadIdx.x / G;
    Src<T, COUT> sa, sb;
    sa.init(a, lda, na, w, na + nb, vv);
    sb.init(b, ldb, nb, w + na, na + nb, vv);
    float bs[COUT];
#pragma unroll
    for (int co = 0; co < COUT; ++co) bs[co] = bias ? bias[co] : 0.f;
    constexpr int UN = 4;   // pixels per thread and trip, every load issued before the arithmetic
    for (size_t base = (size_t)blockIdx.x * PPB * UN; base < npix; base += (size_t)gridDim.x * PPB * UN) {
        vec16<T> av[UN], bv[UN];
        bool valid[UN];
#pragma unroll
        for (int u = 0; u < UN; ++u) {
            const size_t p = base + (size_t)u * PPB + ps;
            valid[u] = p < npix;
            av[u] = sa.load(valid[u] ? p : npix - 1, vv);
            bv[u] = sb.load(valid[u] ? p : npix - 1, vv);
        }
#pragma unroll
        for (int u = 0; u < UN; ++u) {
            const size_t p = base + (size_t)u * PPB + ps;
            float part[COUT];
#pragma unroll
            for (int co = 0; co < COUT; ++co) part[co] = 0.f;
#pragma unroll
            for (int e = 0; e < VE; ++e) {
                const float x = sa.val(av[u], vv, e), y = sb.val(bv[u], vv, e);
#pragma unroll
                for (int co = 0; co < COUT; ++co) part[co] = __builtin_fmaf(sb.w[co][e], y, __builtin_fmaf(sa.w[co][e], x, part[co]));
            }
            for (int o = G >> 1; o > 0; o >>= 1) {
#pragma unroll
                for (int co = 0; co < COUT; ++co) part[co] += __shfl_xor(part[co], o, 64);
            }
            if (valid[u]) {   // lane vv of the pixel's group stores output channel vv (a group of fewer lanes than COUT walks the rest too)
                const size_t bi = p / hw, q = p - bi * hw;
                for (int oc = vv; oc < COUT; oc += G) {
                    float v = 0.f;
#pragma unroll
                    for (int co = 0; co < COUT; ++co) v = (oc == co) ? part[co] + bs[co] : v;
                    if (act == 1) v = sigmoidf(v);
                    out[(bi * COUT + oc) * hw + q] = v;
                }
            }
        }
    }
}

// partial row of a workgroup: [COUT][na+nb] dw, then [COUT] dbias, doubles
template <typename T, int COUT>
__global__ __launch_bounds__(256) void head2_bwd_kernel(const T* __restrict__ a, int lda, int na, const T* __restrict__ b, int ldb, int nb,
                                                        const float* __restrict__ w, const float* __restrict__ gout,
                                                        const float* __restrict__ out, T* __restrict__ ga, int ldga, T* __restrict__ gb, int ldgb,
                                                        double* __restrict__ partials, size_t npix, size_t hw, int G) {
    constexpr int VE = vec16<T>::N;
    const int PPB = 256 / G, vv = threadIdx.x % G, ps = threadIdx.x / G;
    const int nab = na + nb;
    Src<T, COUT> sa, sb;
    sa.init(a, lda, na, w, nab, vv);
    sb.init(b, ldb, nb, w + na, nab, vv);
    float dwa[COUT][VE], dwb[COUT][VE], db[COUT];
#pragma unroll
    for (int co = 0; co < COUT; ++co) {
        db[co] = 0.f;
#pragma unroll
        for (int e = 0; e < VE; ++e) { dwa[co][e] = 0.f; dwb[co][e] = 0.f; }
    }
    for (size_t p = (size_t)blockIdx.x * PPB + ps; p < npix; p += (size_t)gridDim.x * PPB) {
        const size_t bi = p / hw, q = p - bi * hw;
        const vec16<T> av = sa.load(p, vv), bv = sb.load(p, vv);
        float go[COUT];
#pragma unroll
        for (int co = 0; co < COUT; ++co) {
            go[co] = gout[(bi * COUT + co) * hw + q];
            if (out) { const float s = out[(bi * COUT + co) * hw + q]; go[co] *= s * (1.f - s); }   // gout is wrt the sigmoid output
        }
        vec16<T> gav, gbv;
#pragma unroll
        for (int e = 0; e < VE; ++e) {
            const float x = sa.val(av, vv, e), y = sb.val(bv, vv, e);
            float sx = 0.f, sy = 0.f;
#pragma unroll
            for (int co = 0; co < COUT; ++co) {
                sx = __builtin_fmaf(go[co], sa.w[co][e], sx);
                sy = __builtin_fmaf(go[co], sb.w[co][e], sy);
                dwa[co][e] = __builtin_fmaf(go[co], x, dwa[co][e]);
                dwb[co][e] = __builtin_fmaf(go[co], y, dwb[co][e]);
            }
            gav.set(e, vv * VE + e < na ? sx : 0.f);    // padding channels: exactly zero
            gbv.set(e, vv * VE + e < nb ? sy : 0.f);
        }
        if (vv == 0) {
#pragma unroll
            for (int co = 0; co < COUT; ++co) db[co] += go[co];
        }
        if (sa.mine) *reinterpret_cast<vec16<T>*>(ga + p * ldga + vv * VE) = gav;
        if (sb.mine) *reinterpret_cast<vec16<T>*>(gb + p * ldgb + vv * VE) = gbv;
    }
    // the workgroup's sums, in double from here on: the lanes of a wave that hold the same vector index combine by a fixed butterfly
    // (offsets 32 .. G), the four waves through LDS in the order 0, 1, 2, 3
    constexpr int NK = 2 * COUT * VE + COUT;
    __shared__ double red[4][MAXG][NK];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    auto fold = [&](float v, int k) {
        double d = (double)v;
        for (int o = 32; o >= G; o >>= 1) d += __shfl_xor(d, o, 64);
        if (lane < G) red[wave][lane][k] = d;
    };
#pragma unroll
    for (int co = 0; co < COUT; ++co) {
#pragma unroll
        for (int e = 0; e < VE; ++e) { fold(dwa[co][e], co * VE + e); fold(dwb[co][e], (COUT + co) * VE + e); }
        fold(db[co], 2 * COUT * VE + co);
    }
    __syncthreads();
    double* prow = partials + (size_t)blockIdx.x * COUT * (nab + 1);
    for (int i = threadIdx.x; i < COUT * (nab + 1); i += 256) {
        int g, k;
        if (i < COUT * nab) {
            const int co = i / nab, c = i - co * nab;
            const int cs = c < na ? c : c - na;            // channel within its source
            g = cs / VE;
            k = ((c < na ? 0 : COUT) + co) * VE + (cs - g * VE);
        } else {
            g = 0;
            k = 2 * COUT * VE + (i - COUT * nab);
        }
        prow[i] = (red[0][g][k] + red[1][g][k]) + (red[2][g][k] + red[3][g][k]);
    }
}

// one wave per column of the partial rows: lane l adds rows l, l+64, ... in double, the fixed butterfly joins the lanes, one rounding
__global__ __launch_bounds__(256) void head2_finalize_kernel(const double* __restrict__ partials, int nparts, int Cout, int nab,
                                                             float* __restrict__ dw, float* __restrict__ dbias, int accumulate) {
    const int ncol = Cout * (nab + 1);
    const int col = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (col >= ncol) return;     // (a whole wave leaves together: no barrier follows)
    double s = 0.0;
    for (int p = lane; p < nparts; p += 64) s += partials[(size_t)p * ncol + col];
    s = wave_sum_f64(s);
    if (lane == 0) {
        float* q = col < Cout * nab ? dw + col : dbias + (col - Cout * nab);
        store1<double>(q, s, accumulate);
    }
}

inline int pow2_ceil(int v) { int g = 1; while (g < v) g <<= 1; return g; }
// lanes per pixel, or 0 when the strides do not fit (multiples of the 16-byte vector, at most MAXG vectors)
inline int group_lanes(int lda, int ldb, int dtype) {
    const int ve = dtype != WM_F32 ? 8 : 4;
    if (lda <= 0 || ldb <= 0 || lda % ve || ldb % ve) return 0;
    const int g = pow2_ceil(lda / ve > ldb / ve ? lda / ve : ldb / ve);
    return g <= MAXG ? g : 0;
}
inline int head2_parts(size_t npix) { return wm_groups(npix, 128, 1024); }   // (128 pixels: 1..8 trips of a workgroup, by its lanes per pixel)
inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

#define HEAD2_DISPATCH(NAME, KERNEL, GRID, ...)                                                                       \
    WM_DISPATCH_DTYPE(dtype, NAME, switch (Cout) {                                                                     \
        case 1: hipLaunchKernelGGL((KERNEL<T, 1>), dim3(GRID), dim3(256), 0, s, __VA_ARGS__); break;                  \
        case 2: hipLaunchKernelGGL((KERNEL<T, 2>), dim3(GRID), dim3(256), 0, s, __VA_ARGS__); break;                  \
        case 3: hipLaunchKernelGGL((KERNEL<T, 3>), dim3(GRID), dim3(256), 0, s, __VA_ARGS__); break;                  \
        default: hipLaunchKernelGGL((KERNEL<T, 4>), dim3(GRID), dim3(256), 0, s, __VA_ARGS__); break;                 \
    })

}  // namespace

extern "C" int wm_head2_fwd(const void* a, int lda, int na, const void* b, int ldb, int nb, const float* w, const float* bias, float* out,
                            int B, size_t hw, int Cout, int act, int dtype, void* stream) {
    WM_REQUIRE(a && b && w && out && B > 0 && hw > 0 && na > 0 && nb > 0 && na <= lda && nb <= ldb && (act == 0 || act == 1), WM_E_BADARG,
               "wm_head2_fwd: bad arguments (non-null a, b, w, out; 0 < na <= lda, 0 < nb <= ldb; act 0 or 1)");
    WM_REQUIRE(Cout >= 1 && Cout <= MAXCO, WM_E_SHAPE, "wm_head2_fwd: Cout must be 1..4 (got %d)", Cout);
    const int G = group_lanes(lda, ldb, dtype);
    WM_REQUIRE(G > 0 && aligned16(a) && aligned16(b), WM_E_SHAPE,
               "wm_head2_fwd: channel strides %d / %d must be multiples of the 16-byte vector, at most 16 vectors, on 16-byte aligned bases", lda, ldb);
    const size_t npix = (size_t)B * hw;
    const int grid = wm_groups(npix, (size_t)(256 / G) * 4, 2048);
    hipStream_t s = (hipStream_t)stream;
    HEAD2_DISPATCH("wm_head2_fwd", head2_fwd_kernel, grid, (const T*)a, lda, na, (const T*)b, ldb, nb, w, bias, out, npix, hw, G, act);
    WM_LAUNCH_CHECK("wm_head2_fwd");
    return WM_OK;
}

extern "C" int wm_head2_nparts(size_t npix) { return npix > 0 ? head2_parts(npix) : 0; }

extern "C" int wm_head2_bwd(const void* a, int lda, int na, const void* b, int ldb, int nb, const float* w, const float* gout, const float* out,
                            int chain_sigmoid, void* ga, int ldga, void* gb, int ldgb, double* partials, int B, size_t hw, int Cout, int dtype,
                            void* stream) {
    WM_REQUIRE(a && b && w && gout && ga && gb && partials && B > 0 && hw > 0 && na > 0 && nb > 0 && na <= lda && nb <= ldb, WM_E_BADARG,
               "wm_head2_bwd: bad arguments (non-null a, b, w, gout, ga, gb, partials; 0 < na <= lda, 0 < nb <= ldb)");
    WM_REQUIRE(!chain_sigmoid || out, WM_E_BADARG, "wm_head2_bwd: chain_sigmoid needs the saved forward output");
    WM_REQUIRE(Cout >= 1 && Cout <= MAXCO, WM_E_SHAPE, "wm_head2_bwd: Cout must be 1..4 (got %d)", Cout);
    const int G = group_lanes(lda, ldb, dtype);
    WM_REQUIRE(G > 0 && ldga == lda && ldgb == ldb && aligned16(a) && aligned16(b) && aligned16(ga) && aligned16(gb), WM_E_SHAPE,
               "wm_head2_bwd: channel strides %d / %d must be multiples of the 16-byte vector, at most 16 vectors, the gradients' strides equal "
               "to them, all on 16-byte aligned bases", lda, ldb);
    const size_t npix = (size_t)B * hw;
    hipStream_t s = (hipStream_t)stream;
    HEAD2_DISPATCH("wm_head2_bwd", head2_bwd_kernel, head2_parts(npix), (const T*)a, lda, na, (const T*)b, ldb, nb, w, gout,
                   chain_sigmoid ? out : (const float*)nullptr, (T*)ga, ldga, (T*)gb, ldgb, partials, npix, hw, G);
    WM_LAUNCH_CHECK("wm_head2_bwd");
    return WM_OK;
}

extern "C" int wm_head2_finalize(const double* partials, int nparts, int Cout, int nab, float* dw, float* dbias, int accumulate, void* stream) {
    WM_REQUIRE(partials && dw && dbias && nparts > 0 && Cout >= 1 && Cout <= MAXCO && nab > 0, WM_E_BADARG,
               "wm_head2_finalize: bad arguments (non-null partials, dw, dbias; nparts > 0; 1 <= Cout <= 4)");
    const int ncol = Cout * (nab + 1);
    hipLaunchKernelGGL(head2_finalize_kernel, dim3((ncol + 3) / 4), dim3(256), 0, (hipStream_t)stream, partials, nparts, Cout, nab, dw, dbias,
                       accumulate);
    WM_LAUNCH_CHECK("wm_head2_finalize");
    return WM_OK;
}
