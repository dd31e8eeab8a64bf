// The GAN objectives of the reference's trainers, each with its autograd backward:
//   AdversarialLoss (loss.py:41-88)            nsgan = mean BCE(x, t) on probabilities, lsgan = mean (x - t)^2, hinge = mean relu(1 -+ x) for
//                                              the discriminator and -mean(x) for the generator; t a scalar label or the masked labels
//                                              real_label * (1 - bilinear(mask)) of :83-85
//   GANLoss (models/modules/loss.py:77-109)    gan / ragan = mean BCE-with-logits(x, t), lsgan, wgan-gp = -+mean(x); any label value
//   CWLoss (models/modules/loss.py:24-42)      sum_b max(+-(other_b - real_b), kappa), the Carlini-Wagner margin on logits
// f32 contiguous tensors.  No atomics and no host synchronisation: one streaming launch writes per-workgroup partial sums in double and,
// when asked, the gradient wrt the input; a one-workgroup finalise adds the partials in a fixed order.  Forward and gradient together are
// two launches, and every result is bitwise reproducible.
//
// Every element is evaluated in double from the f32 input and rounded once (the gradient: after the upstream factor, and with accumulate
// after the addition to the old value).  The masked labels are sampled inside the loss kernel -- bilinear, align_corners = False, no
// antialiasing: torch's F.upsample(mask, size, mode="bilinear") -- so the resized mask is never written to memory.
//
// CW margin: one wave per row.  The row's `other` is the maximum of (1 - onehot) * logits - onehot * 10000 restated literally (the target's
// slot holds -10000, not -inf) together with the lowest column that attains it, which is where torch.max(x, 1) sends its gradient.
#include "wm_common.h"
#include "wm_reduce.h"

namespace {

constexpr int BCE_PROB = WM_ADV_BCE_PROB, BCE_LOGITS = WM_ADV_BCE_LOGITS, MSE = WM_ADV_MSE, HINGE_DISC = WM_ADV_HINGE_DISC,
              NEG_MEAN = WM_ADV_NEG_MEAN, POS_MEAN = WM_ADV_POS_MEAN;

// the label of element i: the scalar, or real * (1 - the bilinear sample of the mask at i's pixel)
struct Labels {
    const float* mask;       // nullptr: the scalar label
    double label, real, sy, sx;   // sy = Hm / H, sx = Wm / W
    int C, H, W, Cm, Hm, Wm;
};
__device__ __forceinline__ void source(double scale, int dst, int size, int& i0, int& i1, double& lam) {
    double f = scale * ((double)dst + 0.5) - 0.5;
    if (f < 0.0) f = 0.0;
    i0 = (int)f;
    if (i0 > size - 1) i0 = size - 1;
    i1 = i0 + (i0 < size - 1 ? 1 : 0);
    lam = f - (double)i0;
    lam = lam < 0.0 ? 0.0 : (lam > 1.0 ? 1.0 : lam);
}
__device__ __forceinline__ double label_at(const Labels& L, size_t i) {
    if (!L.mask) return L.label;
    const size_t HW = (size_t)L.H * L.W, plane = i / HW;
    const int r = (int)(i - plane * HW), y = r / L.W, x = r - y * L.W;
    const size_t b = plane / L.C;
    const int c = L.Cm == 1 ? 0 : (int)(plane - b * L.C);
    const float* m = L.mask + (b * L.Cm + c) * ((size_t)L.Hm * L.Wm);
    int y0, y1, x0, x1;
    double ly, lx;
    source(L.sy, y, L.Hm, y0, y1, ly);
    source(L.sx, x, L.Wm, x0, x1, lx);
    const double top = (1.0 - lx) * (double)m[(size_t)y0 * L.Wm + x0] + lx * (double)m[(size_t)y0 * L.Wm + x1];
    const double bot = (1.0 - lx) * (double)m[(size_t)y1 * L.Wm + x0] + lx * (double)m[(size_t)y1 * L.Wm + x1];
    return L.real * (1.0 - ((1.0 - ly) * top + ly * bot));
}

// one element: its value v and, with GRAD, dv = d v / d x.  t: the label (HINGE_DISC: the sign s of relu(1 + s x))
template <int OBJ, bool GRAD> __device__ __forceinline__ void elem(float xf, double t, double& v, double& dv) {
    const double x = (double)xf;
    dv = 0.0;
    if (OBJ == BCE_PROB) {          // nn.BCELoss: both logs clamped at -100; backward (x - t) / max(x (1 - x), 1e-12).  x outside [0, 1]: NaN
        double lx = log(x), l1 = log1p(-x);
        lx = lx < -100.0 ? -100.0 : lx;
        l1 = l1 < -100.0 ? -100.0 : l1;
        v = -(t * lx + (1.0 - t) * l1);
        if (GRAD) {
            const double den = (1.0 - x) * x;
            constexpr double EPS = (double)1e-12f;      // torch's backward holds its 1e-12 as a float
            dv = (x - t) / (den < EPS ? EPS : den);
        }
    } else if (OBJ == BCE_LOGITS) { // nn.BCEWithLogitsLoss: (1 - t) x + max(-x, 0) + log(1 + exp(-|x|))
        const double e = exp(-fabs(x));
        v = (1.0 - t) * x + (x < 0.0 ? -x : 0.0) + log1p(e);
        if (GRAD) dv = (x >= 0.0 ? 1.0 / (1.0 + e) : e / (1.0 + e)) - t;
    } else if (OBJ == MSE) {
        const double d = x - t;
        v = d * d;
        if (GRAD) dv = 2.0 * d;
    } else if (OBJ == HINGE_DISC) { // nn.ReLU: the subgradient at 0 is 0
        const double z = 1.0 + t * x;
        v = z > 0.0 ? z : 0.0;
        if (GRAD) dv = z > 0.0 ? t : 0.0;
    } else if (OBJ == NEG_MEAN) {
        v = -x;
        if (GRAD) dv = -1.0;
    } else {
        v = x;
        if (GRAD) dv = 1.0;
    }
}

// grid (P): block j takes its grid-stride share of the n elements -> partials[j]; GRAD: grad (+)= g / n * dv
template <int OBJ, bool GRAD>
__global__ __launch_bounds__(256) void advloss_elem_kernel(const float* __restrict__ x, size_t n, Labels L, double* __restrict__ partials,
                                                           float* __restrict__ grad, const float* __restrict__ gout, float gscale,
                                                           const float* __restrict__ gscale_dev, int accumulate) {
    const double k = GRAD ? upstream(gscale, gscale_dev, gout) / (double)n : 0.0;
    const Split sp = split16(n, x, GRAD ? grad : nullptr);
    double a = 0.0;
    stream16(sp, n,
             [&](size_t i) {
                 const float4 p = ld16(x + i);
                 double v0, v1, v2, v3, d0, d1, d2, d3;
                 elem<OBJ, GRAD>(p.x, label_at(L, i), v0, d0);
                 elem<OBJ, GRAD>(p.y, label_at(L, i + 1), v1, d1);
                 elem<OBJ, GRAD>(p.z, label_at(L, i + 2), v2, d2);
                 elem<OBJ, GRAD>(p.w, label_at(L, i + 3), v3, d3);
                 a += v0; a += v1; a += v2; a += v3;
                 if (GRAD) store4<double>(grad + i, d0 * k, d1 * k, d2 * k, d3 * k, accumulate);
             },
             [&](size_t i) {
                 double v, d;
                 elem<OBJ, GRAD>(x[i], label_at(L, i), v, d);
                 a += v;
                 if (GRAD) store1<double>(grad + i, d * k, accumulate);
             });
    __shared__ double s[4];
    a = block_sum_f64(a, s);
    if (threadIdx.x == 0) partials[blockIdx.x] = a;
}

inline int elem_parts(size_t n) { return wm_groups(n, 4096, 256); }
inline bool obj_ok(int o) { return o >= BCE_PROB && o <= POS_MEAN; }
inline bool obj_has_label(int o) { return o == BCE_PROB || o == BCE_LOGITS || o == MSE; }

// ------------------------------------------------------------------------------------------------ Carlini-Wagner margin
// 4 waves per workgroup, wave w of block j owns row 4 j + w -> terms[row] (double), and with grad the row's gradient
__global__ __launch_bounds__(256) void cw_margin_kernel(const float* __restrict__ logits, const long long* __restrict__ target, int B, int K,
                                                        int targeted, float kappa, double* __restrict__ terms, float* __restrict__ grad,
                                                        const float* __restrict__ gout, float gscale, const float* __restrict__ gscale_dev,
                                                        int accumulate) {
    const int lane = threadIdx.x & 63;
    const size_t row = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= (size_t)B) return;
    const float* z = logits + row * K;
    float* g = grad ? grad + row * K : nullptr;
    const long long t = target[row];
    if (t < 0 || t >= (long long)K) {      // a label outside [0, K): nothing is read at it; the loss and this row's gradient become NaN
        if (lane == 0) terms[row] = __builtin_nan("");
        if (g)
            for (int j = lane; j < K; j += 64) g[j] = __builtin_nanf("");
        return;
    }
    // other = max_j (1 - onehot_j) z_j - onehot_j * 10000, and the lowest j that attains it
    float best = -__builtin_inff();
    int arg = 0x7fffffff;
    for (int j = lane; j < K; j += 64) {
        const float oh = j == (int)t ? 1.f : 0.f;
        const float v = (1.f - oh) * z[j] - oh * 10000.f;
        if (v > best || arg == 0x7fffffff) { best = v; arg = j; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ob = __shfl_xor(best, o, 64);
        const int oa = __shfl_xor(arg, o, 64);
        if (oa != 0x7fffffff && (arg == 0x7fffffff || ob > best || (ob == best && oa < arg))) { best = ob; arg = oa; }
    }
    const double d = targeted ? (double)best - (double)z[t] : (double)z[t] - (double)best;
    const double kp = (double)kappa;
    if (lane == 0) terms[row] = d > kp ? d : kp;
    if (g) {
        // torch.max(d, kappa) sends 1 to the larger argument and 1/2 to each at a tie; the clamp's share goes nowhere.  The target's own slot
        // of `other` is a constant: when it is the maximum, only `real` carries a gradient
        const double w = (d > kp ? 1.0 : (d == kp ? 0.5 : 0.0)) * upstream(gscale, gscale_dev, gout);
        const double wo = targeted ? w : -w;
        for (int j = lane; j < K; j += 64) {
            double r = 0.0;
            if (j == (int)t) r = -wo;
            else if (j == arg) r = wo;
            if (accumulate) r += (double)g[j];
            g[j] = (float)r;
        }
    }
}

}  // namespace

extern "C" int wm_advloss_nparts(size_t n) { return n > 0 ? elem_parts(n) : 0; }

#define ADV_LAUNCH(OBJ)                                                                                                                   \
    do {                                                                                                                                  \
        if (grad) hipLaunchKernelGGL((advloss_elem_kernel<OBJ, true>), grid, dim3(256), 0, s, x, n, L, partials, grad, gout_dev, gscale,  \
                                     gscale_dev, accumulate);                                                                             \
        else hipLaunchKernelGGL((advloss_elem_kernel<OBJ, false>), grid, dim3(256), 0, s, x, n, L, partials, grad, gout_dev, gscale,      \
                                gscale_dev, accumulate);                                                                                  \
    } while (0)

extern "C" int wm_advloss_elem(int objective, const float* x, size_t n, float label, const float* mask, int B, int C, int H, int W, int Cm, int Hm,
                               int Wm, float real_label, double* partials, float* grad, const float* gout_dev, float gscale,
                               const float* gscale_dev, int accumulate, void* stream) {
    WM_REQUIRE(x && partials && n > 0 && obj_ok(objective), WM_E_BADARG,
               "wm_advloss_elem: bad arguments (x, partials, n > 0, objective one of WM_ADV_*)");
    WM_REQUIRE(objective != HINGE_DISC || label == 1.f || label == -1.f, WM_E_BADARG,
               "wm_advloss_elem: WM_ADV_HINGE_DISC takes its sign in label: -1 (real) or +1 (fake)");
    Labels L{};
    L.label = (double)label;
    if (mask) {
        WM_REQUIRE(obj_has_label(objective), WM_E_BADARG, "wm_advloss_elem: masked labels need an objective with a label (bce_prob, bce_logits, mse)");
        WM_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0 && Hm > 0 && Wm > 0 && (Cm == 1 || Cm == C) && (size_t)B * C * H * W == n &&
                       (size_t)H * W <= 0x7fffffffu && (size_t)Hm * Wm <= 0x7fffffffu, WM_E_BADARG,
                   "wm_advloss_elem: masked labels: x is [B,C,H,W] with B*C*H*W == n, mask [B,Cm,Hm,Wm] with Cm 1 or C (H*W, Hm*Wm < 2^31)");
        L.mask = mask;
        L.real = (double)real_label;
        L.sy = (double)Hm / (double)H;
        L.sx = (double)Wm / (double)W;
        L.C = C; L.H = H; L.W = W; L.Cm = Cm; L.Hm = Hm; L.Wm = Wm;
    }
    const dim3 grid(elem_parts(n));
    hipStream_t s = (hipStream_t)stream;
    switch (objective) {
        case BCE_PROB: ADV_LAUNCH(BCE_PROB); break;
        case BCE_LOGITS: ADV_LAUNCH(BCE_LOGITS); break;
        case MSE: ADV_LAUNCH(MSE); break;
        case HINGE_DISC: ADV_LAUNCH(HINGE_DISC); break;
        case NEG_MEAN: ADV_LAUNCH(NEG_MEAN); break;
        default: ADV_LAUNCH(POS_MEAN); break;
    }
    WM_LAUNCH_CHECK("wm_advloss_elem");
    return WM_OK;
}

extern "C" int wm_advloss_finalize(const double* partials, size_t n, float* loss_out, void* stream) {
    WM_REQUIRE(partials && loss_out && n > 0, WM_E_BADARG, "wm_advloss_finalize: bad arguments");
    wm_sum_finalize(partials, (size_t)elem_parts(n), 1.0 / (double)n, loss_out, (hipStream_t)stream);
    WM_LAUNCH_CHECK("wm_advloss_finalize");
    return WM_OK;
}

extern "C" int wm_cw_margin(const float* logits, const long long* target, int B, int K, int is_targeted, float kappa, double* terms,
                            float* loss_out, float* grad, const float* gout_dev, float gscale, const float* gscale_dev, int accumulate,
                            void* stream) {
    WM_REQUIRE(logits && target && terms && loss_out && B > 0, WM_E_BADARG, "wm_cw_margin: bad arguments");
    WM_REQUIRE(K >= 2, WM_E_BADARG, "wm_cw_margin: K >= 2 classes expected (with one class there is no other logit)");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(cw_margin_kernel, dim3((unsigned)(((size_t)B + 3) / 4)), dim3(256), 0, s, logits, target, B, K, is_targeted ? 1 : 0, kappa,
                       terms, grad, gout_dev, gscale, gscale_dev, accumulate);
    wm_sum_finalize(terms, (size_t)B, 1.0, loss_out, s);
    WM_LAUNCH_CHECK("wm_cw_margin");
    return WM_OK;
}
