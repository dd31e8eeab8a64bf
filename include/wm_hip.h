/*
 * wm_hip.h -- C ABI of libwm_hip.so, the MI355X (gfx950) kernel library behind the
 * watermark embed -> attack -> extract training step.
 *
 * The reference (yingqichao/video-watermarking-forgery-detection) has no native code and
 * no FFI: every GPU kernel it runs is reached through torch.nn modules.  The entry points
 * below are therefore the operator boundary a maintainer of the reference would bind with
 * ctypes to replace, module by module, the torch ops listed next to
 * each function ("replaces:" = reference file:line, paths relative to the reference root).
 *
 * Conventions
 *   - plain C: raw device pointers + explicit sizes, no torch / C++ types;
 *   - the caller owns every buffer (inputs, outputs, workspaces); the library never
 *     allocates, frees or keeps a pointer after the call returns;
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*), re-entrant, and the library
 *     holds no mutable state between calls (no knobs, no environment variables, no set-then-call hints; the
 *     only per-thread datum is the text of the last error); safe under hipGraph capture.  The A/B switches
 *     (wm_debug_* setters) of tools/ and the tests exist only in the -DWM_DEBUG build lib/libwm_hip_dbg.so;
 *     neither build reads an environment variable;
 *   - return value: 0 = ok, <0 = error (WM_E_*); wm_last_error_string() gives the text of
 *     the last error on the calling thread.  No C++ exception crosses the boundary.  A function that can fail
 *     takes at least one pointer; an int function with scalar parameters only is a query whose int is its answer;
 *   - activations are NHWC ("pixel-major"): element (b,h,w,c) lives at
 *     base[((b*H + h)*W + w) * ld + c], ld >= C the per-pixel channel stride (lets a tensor
 *     be a channel-slice of a wider one).  dtype of activations/packed weights:
 *     WM_F32 (parity path, exact f32 MFMA) or WM_BF16 (production path, f32 accumulate).
 *     Parameters, gradients of parameters, statistics and images at the attack boundary
 *     are always f32; images at the attack boundary are NCHW planes like the reference.
 */
#ifndef WM_HIP_H
#define WM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* the library is compiled with -fvisibility=hidden: the functions declared here are its whole export table */
#pragma GCC visibility push(default)

#define WM_F32 0
#define WM_BF16 1
#define WM_F16 2   /* the reference's autocast dtype (IRNcrop_model.py:340); same kernels and rates as WM_BF16, 10-bit mantissa, needs loss scaling */

#define WM_OK 0
#define WM_E_BADARG (-1)   /* null pointer, non-positive size, unsupported dtype */
#define WM_E_SHAPE (-2)    /* shape / alignment the kernels do not support */
#define WM_E_HIP (-3)      /* a HIP runtime call or launch failed */

const char* wm_last_error_string(void);
int wm_abi_version(void);

/* A BatchNorm-backward finalisation that rides on another launch (wm_conv3x3_wgrad_fin: a few extra workgroups of the
 * weight-gradient slab reduction) instead of costing one of its own.  Same arguments and result as wm_bn_bwd_finalize_raw
 * (mean != NULL: rows hold sum(gz), sum(gz*y)) / wm_bn_bwd_finalize (mean == NULL); nparts <= 256. */
typedef struct WmBnBwdFin {
    const float* partials; int nparts; int C; int CP; double count; const float* gamma; const float* mean; const float* invstd;
    float* dgamma; float* dbeta; int accumulate; float* coef;
} WmBnBwdFin;

/* ------------------------------------------------------------------ block-JPEG attack
 * replaces: noise_layers/jpeg.py:226-240 (Jpeg.forward), :259-273 (JpegSS), :295-306 (JpegMask)
 * with helpers :52-211.  x,y: [B,3,H,W] f32 NCHW.  mode 0 = round, 1 = round_ss, 2 = mask.
 * tables: host pointer to 128 floats = luminance[64] then chrominance[64] quantisation
 * tables, already scaled/rounded/clamped as std_quantization does (ignored for mode 2).
 * subsample: 0 or 2.  One fused kernel: x255, pad, RGB->YUV, (subsample), DCT, quantise,
 * de-quantise, IDCT, YUV->RGB, crop, /255.  Algorithmic traffic 24 B/px. */
#define WM_JPEG_ROUND 0
#define WM_JPEG_SS 1
#define WM_JPEG_MASK 2
int wm_jpeg_fwd(const float* x, float* y, int B, int H, int W, int mode, const float* tables,
                int subsample, void* stream);
/* ... and, act16 non-NULL, the attacked image a second time as [B][H][W][16] pixels of dtype act_dtype (channels 0..2, zero tail): the
 * input of the decoder's image-fed first layer (hidden_models/decoder.py:15), without wm_nchw_to_nhwc's launch. */
int wm_jpeg_fwd_act(const float* x, float* y, void* act16, int act_dtype, int B, int H, int W, int mode, const float* tables,
                    int subsample, void* stream);
/* gx = d(sum(gy*y))/dx.  x is read only for mode 1 (derivative of round_ss needs the
 * pre-rounding coefficient); mode 0 writes zeros (torch.round has zero gradient). */
int wm_jpeg_bwd(const float* x, const float* gy, float* gx, int B, int H, int W, int mode,
                const float* tables, int subsample, void* stream);

/* ------------------------------------------------------------------ DiffJPEG
 * replaces: utils/JPEG.py:256-291 (compress_jpeg) + :431-469 (decompress_jpeg) as composed
 * by DiffJPEG.forward :535-540.  H,W multiples of 16.  rounding 0 = torch.round,
 * 1 = round_only_at_0, 2 = diff_round.  factor = quality_to_factor(quality). */
int wm_diffjpeg_fwd(const float* x, float* y, int B, int H, int W, int rounding, float factor,
                    void* stream);
int wm_diffjpeg_bwd(const float* x, const float* gy, float* gx, int B, int H, int W, int rounding,
                    float factor, void* stream);

/* ------------------------------------------------------------------ stencil / resample attacks
 * All on [B,C,H,W] f32 NCHW planes (N = B*C planes of H x W).
 * gauss3: replaces noise_layers/gaussian_blur.py:53-56 (depthwise 3x3, zero pad 1); w9 = host
 *         pointer to the 9 weights.  Backward of a symmetric stencil = the same stencil. */
int wm_stencil3_fwd(const float* x, float* y, int N, int H, int W, const float* w9, void* stream);
/* median k x k (k = 3 or 5), zero padding: replaces noise_layers/middle_filter.py:5-13
 * (kornia MedianBlur).  idx (int8 per pixel, may be NULL) records which window tap was
 * selected so the backward can route the gradient to it. */
int wm_median_fwd(const float* x, float* y, int8_t* idx, int N, int H, int W, int k, void* stream);
int wm_median_bwd(const float* gy, const int8_t* idx, float* gx, int N, int H, int W, int k,
                  void* stream);
/* bicubic (A=-0.75, align_corners=False, no antialias) and bilinear resampling of the
 * sub-rectangle [h0,h0+hs) x [w0,w0+ws) of x[N,H,W] to y[N,OH,OW]; replaces
 * F.interpolate in noise_layers/resize.py:42-51 and noise_layers/crop.py:48-53.
 * clamp01 != 0 clamps the output to [0,1] (resize.py:53).  The backward is the transpose in
 * gather form (deterministic, no atomics): gx[N,H,W] gets zero outside the rectangle;
 * y_clamped (may be NULL) is the clamped forward output: where it is not strictly inside (0,1)
 * the clamp was active and the incoming gradient is dropped. */
#define WM_BILINEAR 0
#define WM_BICUBIC 1
int wm_resample_fwd(const float* x, float* y, int N, int H, int W, int h0, int hs, int w0, int ws,
                    int OH, int OW, int kind, int clamp01, void* stream);
int wm_resample_bwd(const float* gy, const float* y_clamped, float* gx, int N, int H, int W,
                    int h0, int hs, int w0, int ws, int OH, int OW, int kind, void* stream);
/* The same backward (replaces: autograd of the same F.interpolate calls) in two separable passes through a caller-owned workspace
 * tmp[N][OH][W] floats: x pass (gy, y_clamped -> tmp), y pass (tmp -> gx); 3x faster at the Resize attack's ratios; deterministic;
 * sums in a different order than the gather form (agreement ~1e-7 relative). */
int wm_resample_bwd_sep(const float* gy, const float* y_clamped, float* gx, float* tmp, int N, int H, int W,
                        int h0, int hs, int w0, int ws, int OH, int OW, int kind, void* stream);
/* Quantization: round(255 x)/255; replaces models/modules/Quantization.py:7-14 (the backward
 * is the identity and needs no kernel). */
int wm_quant_fwd(const float* x, float* y, size_t n, void* stream);
/* Separable k x k blur, k odd in 3..WM_GAUSS_SEP_MAX_K, r = k/2: replaces noise_layers/gaussian_blur.py:44-56 at any kernel size
 * (WM_BORDER_ZERO: Conv2d padding (k-1)/2) and noise_layers/gaussian_filter.py (kornia GaussianBlur2d, WM_BORDER_REFLECT); the 2-D weights
 * are outer(taps, taps).  taps = host pointer to k f32 values, read before the call returns.
 *   y[h,w] = sum_i taps[i] * (sum_j taps[j] * xpad[h+i-r, w+j-r]),  inner (row) sum first, each sum a chain of fmaf from 0, left to right.
 * One launch: a workgroup stages its tile and halo in LDS, row pass LDS -> LDS, column pass LDS -> registers -> y; float4 global access
 * where W % 4 == 0 and the base is 16-byte aligned, element by element elsewhere, same bits either way.
 * Backward = the exact transpose in gather form (deterministic): zero border = the forward with reversed taps; reflected border = with
 * Z(p) = sum_i taps[k-1-i] * G[p+i-r] on the zero-extended gradient G, gx[q] = Z(q) + [1<=q<=r] Z(-q) + [n-1-r<=q<=n-2] Z(2(n-1)-q) per axis
 * (row axis first).  Any other k, or WM_BORDER_REFLECT with r >= H or r >= W (torch's reflect-pad limit): WM_E_BADARG, nothing is launched. */
#define WM_BORDER_ZERO 0
#define WM_BORDER_REFLECT 1
#define WM_GAUSS_SEP_MAX_K 15
int wm_gauss_sep_fwd(const float* x, float* y, int N, int H, int W, const float* taps, int k, int border, void* stream);
int wm_gauss_sep_bwd(const float* gy, float* gx, int N, int H, int W, const float* taps, int k, int border, void* stream);
/* Cropout: replaces noise_layers/crop.py:128-134.  y = x inside [h0,h1) x [w0,w1) and cover elsewhere (a fresh tensor: cover is only read).
 * Backward: gx = g inside, 0 outside; gcover (may be NULL) = 0 inside, g outside, in the same launch.  Selections: every output is bit-exact.
 * An empty rectangle, or one not inside the plane: WM_E_BADARG. */
int wm_cropout_fwd(const float* x, const float* cover, float* y, int N, int H, int W, int h0, int h1, int w0, int w1, void* stream);
int wm_cropout_bwd(const float* g, float* gx, float* gcover, int N, int H, int W, int h0, int h1, int w0, int w1, void* stream);

/* The clip loader's device path (replaces: /root/reference/data/Dataloader.py:22-57, the per-frame numpy -> cv2.resize -> torch chain):
 * decoded frames uint8 x[N][H][W][C] (C <= 4) -> float planes y[N][C][H][W] = x * scale (1/255 for images); the resize itself is
 * wm_resample_fwd(WM_BILINEAR) over the whole frame (half-pixel centres, no antialias = cv2.INTER_LINEAR's float arithmetic). */
int wm_u8_hwc_to_planes(const unsigned char* x, float* y, int N, int H, int W, int C, float scale, void* stream);
/* ------------------------------------------------------------------ layout / packing
 * image planes [B,C,H,W] f32 -> NHWC dtype with per-pixel stride ld, written at channel
 * offset c0; channels [c0+C, c0+C+zero_tail) are zero-filled (padding for MFMA K). */
int wm_nchw_to_nhwc(const float* x, void* y, int B, int C, int H, int W, int ld, int c0,
                    int zero_tail, int dtype, void* stream);
/* NHWC dtype (stride ld, offset c0) -> [B,C,H,W] f32 */
int wm_nhwc_to_nchw(const void* x, float* y, int B, int C, int H, int W, int ld, int c0, int dtype,
                    void* stream);
/* per-sample vector v[B,L] f32 broadcast over H x W into NHWC at channel offset c0
 * (the expanded message of hidden_models/encoder.py:34-37). */
int wm_broadcast_to_nhwc(const float* v, void* y, int B, int L, int H, int W, int ld, int c0,
                         int dtype, void* stream);
/* the tail of the encoder's concat tensor in one pass: channels [c0, c0+tail) of every pixel =
 * [message v[b, 0..L) | image planes img[b, 0..3) | zeros]  (encoder.py:34-40).  c0, tail, ld multiples of
 * the 16-byte vector width. */
int wm_concat_tail(const float* msg, const float* img, void* y, int B, int L, int H, int W, int ld, int c0,
                   int tail, int dtype, void* stream);
/* the whole concat row in one pass: y[..., :C] = relu(scale*x+shift) (the encoder features, fused BN+ReLU),
 * y[..., C:] = [message(L) | image(3) | 0]; x NHWC stride ldx, y NHWC stride ld. */
int wm_concat_full(const void* x, int ldx, const float* scale, const float* shift, const float* msg, const float* img,
                   void* y, int B, int C, int L, int H, int W, int ld, int dtype, void* stream);
/* relu(scale*x+shift) of an NHWC tensor copied into another NHWC tensor (channel slice):
 * materialises a BatchNorm+ReLU output where a consumer cannot fuse it (concat). */
int wm_bnrelu_copy(const void* x, int ldx, const float* scale, const float* shift, void* y, int ldy,
                   int c0, size_t npix, int C, int dtype, void* stream);
/* conv weight [Cout,Cin,3,3] f32 (PyTorch layout) -> packed [9][CoutP][CinP] dtype, zero padded.
 * perm (host int[Cin], may be NULL): packed input channel perm[ci] holds reference channel ci.
 * transpose != 0 builds the dgrad operand instead: [9][CinP][CoutP] with taps flipped. */
int wm_pack_w3x3(const float* w, void* wp, int Cout, int Cin, int CoutP, int CinP, const int* perm,
                 int transpose, int dtype, void* stream);
/* batched form: all convs of a network in ONE launch (the weights change every optimiser step, so every
 * step re-packs them).  jobs_dev: DEVICE array of njobs records of 48 bytes each,
 *   { const float* w; void* wp; const int* perm ( DEVICE int[Cin] or NULL ); int Cout, Cin, CoutP, CinP, transpose, pad; }
 * with the meaning of wm_pack_w3x3's arguments; max_elems = the largest 9*RowsP*ColsP among the jobs. */
int wm_pack_w3x3_batch(const void* jobs_dev, int njobs, size_t max_elems, int dtype, void* stream);

/* ------------------------------------------------------------------ conv 3x3, stride 1, pad 1
 * replaces: nn.Conv2d(…,3,1,padding=1) inside hidden_models/conv_bn_relu.py:11-15 and
 * network/UNet.py:67-97, as an implicit GEMM on MFMA (M = pixels, N = Cout, K = 9*Cin).
 *   x  : NHWC [B,H,W,Cin] stride ldx.  If in_scale/in_shift != NULL the kernel applies
 *        relu(in_scale[c]*x+in_shift[c]) while staging (fused BatchNorm+ReLU of the producer);
 *        zero padding is applied after that transform, as the reference pads the activated map.
 *   wp : packed weights from wm_pack_w3x3 (transpose=0), [9][CoutP][CinP]; CinP == Cin here.
 *   bias: f32[nbias] (nbias <= CoutP, the real Cout) or NULL.   y: NHWC [B,H,W,CoutP] stride ldy (raw conv output).
 *   stat_partials: NULL, or f32[wm_conv3x3_nparts(B,H,W,Cin,CoutP,dtype)][2][CoutP]: per-workgroup sums of y
 *        and y^2 (from the f32 accumulators) for the BatchNorm batch statistics.
 * Cin multiple of 16 (bf16, f16) / 4 (f32); CoutP multiple of 32.  The same entry point computes
 * dgrad when given dy and the transposed pack. */
int wm_conv3x3_nparts(int B, int H, int W, int Cin, int CoutP, int dtype);
int wm_conv3x3_fwd(const void* x, int ldx, const void* wp, const float* bias, int nbias,
                   const float* in_scale, const float* in_shift, void* y, int ldy, float* stat_partials, int B, int H,
                   int W, int Cin, int CoutP, int dtype, int sweep_reverse, void* stream);
/* sweep_reverse (wm_conv3x3_fwd, wm_conv3x3_dgrad_applyfused / _bwdstats, wm_conv3x3_wgrad_fin): != 0 sweeps the pixel tiles
 * backwards.  A kernel that starts where the producer of its input stopped finds the freshest part of that tensor in the
 * Infinity Cache (256 MB against 134 MB per tensor at B=16, 256x256); the host alternates the direction along a chain of
 * layers.  Results do not depend on it except for the summation order inside the per-workgroup statistics rows.
 * weight gradient: dW[co,ci,kh,kw] = sum_{b,h,w} a[b,h+kh-1,w+kw-1,ci] * dy[b,h,w,co], with
 * a = x or relu(in_scale*x+in_shift).  Writes f32 partial slabs ws[nslabs][9][CinP][CoutP]
 * (nslabs = wm_conv3x3_wgrad_nslabs) and reduces them into dw[Cout,Cin,3,3] (PyTorch layout,
 * overwritten or accumulated).  perm as in wm_pack_w3x3 (device int[Cin] or NULL). */
int wm_conv3x3_wgrad_nslabs(int B, int H, int W);
size_t wm_conv3x3_wgrad_ws_bytes(int B, int H, int W, int CinX, int CoutY);
/* CinX / CoutY: channel counts of the x / dy tensors (padded, packed order);
 * Cin / Cout: the reference parameter's dims (dw is [Cout,Cin,3,3]). */
int wm_conv3x3_wgrad(const void* x, int ldx, int CinX, const float* in_scale, const float* in_shift,
                     const void* dy, int lddy, int CoutY, float* ws, float* dw, int accumulate, int B,
                     int H, int W, int Cin, int Cout, const int* perm_dev, int dtype, void* stream);
/* wm_conv3x3_wgrad / wm_conv3x3_wgrad_gvfused whose slab-reduction launch also carries a BatchNorm-backward finalisation of
 * ANOTHER layer (fin may be NULL): in a backward sweep the input-gradient kernel of layer l emits the sums of layer l-1
 * (wm_conv3x3_dgrad_bwdstats / _applyfused), and layer l's weight gradient is the next launch anyway. */
int wm_fin_rider_enabled(void);
int wm_conv3x3_wgrad_fin(const void* x, int ldx, int CinX, const float* in_scale, const float* in_shift, const void* dy, int lddy,
                         int CoutY, float* ws, float* dw, int accumulate, int B, int H, int W, int Cin, int Cout,
                         const int* perm_dev, int dtype, const WmBnBwdFin* fin, int sweep_reverse, void* stream);
/* The same with the BatchNorm-backward APPLY pass fused, for bf16 image-fed first layers (CinX <= 16) whose input needs
 * no gradient: dy is formed from g (gradient wrt the ReLU output, stride ldg), y (the raw conv output, stride ldy),
 * stats4 = f32[4][CoutY] = scale | shift | mean | invstd and coef = wm_bn_bwd_finalize's f32[3][CoutY] while the tile is
 * staged, and never written to memory (no wm_bn_bwd_apply, no dy tensor). */
int wm_conv3x3_wgrad_bnfused_supported(int CinX, int CoutY, int dtype);
int wm_conv3x3_wgrad_bnfused(const void* x, int ldx, int CinX, const void* g, int ldg, const void* y, int ldy, int CoutY,
                             const float* stats4, const float* coef, float* ws, float* dw, int accumulate, int B, int H, int W,
                             int Cin, int Cout, int dtype, void* stream);
/* The pair for a ConvBNRelu whose output was globally pooled (hidden_models/decoder.py:16-24, discriminator.py:14-22:
 * the gradient wrt its ReLU output is one row per sample, gvec f32[B][CoutY], already divided by H*W).  Both kernels
 * read the layer's raw conv output y instead of dy and apply the BatchNorm backward while staging (bf16, CinX = 64,
 * CoutY in {64, 32}); results are bit-identical to wm_bn_bwd_apply followed by wm_conv3x3_wgrad / wm_conv3x3_fwd.
 * wpt: the transposed packed filter (wm_pack_w3x3 with transpose = 1), dx: [B,H,W,CinP] dense. */
int wm_conv3x3_gvfused_supported(int CinX, int CoutY, int dtype);
int wm_conv3x3_wgrad_gvfused(const void* x, int ldx, int CinX, const float* in_scale, const float* in_shift, const float* gvec,
                             const void* y, int ldy, int CoutY, const float* stats4, const float* coef, float* ws, float* dw,
                             int accumulate, int B, int H, int W, int Cin, int Cout, int dtype, void* stream);
int wm_conv3x3_wgrad_gvfused_fin(const void* x, int ldx, int CinX, const float* in_scale, const float* in_shift, const float* gvec,
                                 const void* y, int ldy, int CoutY, const float* stats4, const float* coef, float* ws, float* dw,
                                 int accumulate, int B, int H, int W, int Cin, int Cout, int dtype, const WmBnBwdFin* fin, void* stream);
int wm_conv3x3_dgrad_gvfused(const void* y, int ldy, int CoutY, const void* wpt, const float* gvec, const float* stats4,
                             const float* coef, void* dx, int B, int H, int W, int CinP, int dtype, void* stream);
/* Input gradient (bf16, CoutY in {64,32} -> CinP = 64) whose epilogue also reduces the BatchNorm-backward sums of the
 * ConvBNRelu that FEEDS this layer (conv_bn_relu.py:11-15 stacked as in decoder.py:16-24): dx is that layer's g, and with
 * its raw output ry [B,H,W,64] and r_scale / r_shift the kernel emits partials f32[wm_conv3x3_nparts(..)][2][64] =
 * sum(gz), sum(gz*y) per channel (gz = bf16(dx)*[r_scale*ry + r_shift > 0]) -- wm_bn_bwd_reduce over (dx, ry) is not
 * needed; finish with wm_bn_bwd_finalize_raw.  dx is WRITTEN as gz (multiplied by the feeding layer's ReLU mask, like
 * wm_conv3x3_bwd_fused's; every consumer applies that mask itself, twice is the identity), so it may be handed to
 * wm_conv3x3_bwd_fused with g_premasked = 1.  src = this layer's dy, or (gvec, stats4, coef non-NULL) this layer's raw
 * output with the apply pass fused as in wm_conv3x3_dgrad_gvfused. */
/* The ordinary 64 -> 64 layer (gradient g a dense bf16 tensor [B,H,W,64]): input gradient with the BatchNorm-backward APPLY
 * pass fused.  The kernel reads g and the layer's raw output y (dense), forms dy from stats4 / coef while staging, writes
 * dy_out [B,H,W,64] (bit-identical to wm_bn_bwd_apply's; input of the wm_conv3x3_wgrad that follows; NULL: not written -- an input
 * gradient whose weight gradient nobody reads, e.g. the discriminator under the generator's loss, hidden.py:85-103) and dx = conv(dy, wpt)
 * [B,H,W,CinP], CinP = 64, or 32 for an image-fed layer (wpt [9][CinP][64]).
 * ry / r_scale / r_shift / partials: optional, all or none -- the sums of the feeding layer as in
 * wm_conv3x3_dgrad_bwdstats. */
int wm_conv3x3_dgrad_applyfused_supported(int CoutY, int CinP, int dtype);
int wm_conv3x3_dgrad_applyfused(const void* g, const void* y, const float* stats4, const float* coef, const void* wpt,
                                void* dy_out, void* dx, const void* ry, const float* r_scale, const float* r_shift,
                                float* partials, int B, int H, int W, int CinP, int dtype, int sweep_reverse, void* stream);
/* The whole backward of a 64 -> 64 body layer fed by another ConvBNRelu (16-bit activations), in ONE pass over its operands:
 * wm_conv3x3_bwd_fused reads g, y (this layer: gradient wrt its ReLU output, raw conv output) and xr (the FEEDING layer's raw conv
 * output, with its BatchNorm in_scale / in_shift), forms dy while staging and produces
 *   dx [B,H,W,64]              = conv(dy, wpt) * [in_scale * xr + in_shift > 0]: the gradient wrt the feeding layer's ReLU output,
 *                                already multiplied by that ReLU's mask (every consumer applies the mask itself; twice is the identity),
 *   partials [nwg][2][64]      = the feeding layer's BatchNorm-backward sums of dx (as wm_conv3x3_dgrad_bwdstats),
 *   ws [nwg][9][64][64]        = per-workgroup slabs of the weight gradient sum dy (x) ReLU(in_scale * xr + in_shift),
 * without writing dy or re-reading xr (537 MB instead of 939 MB per layer at B = 16, 256x256).  g_premasked != 0: g is such a masked
 * gradient (the staging then skips the mask arithmetic; the results are the same).  Exactly one of g and gvec is non-NULL: gvec
 * f32 [B][64] is the gradient of a globally pooled layer, one row per sample (B <= wm_conv3x3_bwd_fused_gvec_max_batch(); dy is then
 * formed from y alone, as in wm_conv3x3_dgrad_gvfused).  nwg = wm_conv3x3_bwd_fused_nwg(B,H,W).
 * wm_conv3x3_bwd_fused_reduce: dw [Cout][Cin][3][3] (+)= the sum of the slabs (wm_conv3x3_wgrad_fin's reduction, incl. `fin`). */
int wm_conv3x3_bwd_fused_supported(int dtype);
int wm_conv3x3_bwd_fused_supported_shape(int B, int H, int W, int dtype);   /* ... and B*H*W*64 < 2^31 (32-bit element offsets) */
int wm_conv3x3_bwd_fused_nwg(int B, int H, int W);
int wm_conv3x3_bwd_fused_gvec_max_batch(void);
/* which kernel wm_conv3x3_bwd_fused launches for these arguments: 8 = the role-split 8-wave form (csrc/bwd_ws8.hip: whole 8x16 tiles and a
 * premasked tensor gradient or a per-sample gradient), 1 = the single-role form (csrc/bwd_ws.hip: everything else) */
int wm_conv3x3_bwd_fused_kernel(int H, int W, int g_premasked, int has_gvec);
int wm_conv3x3_bwd_fused(const void* g, const float* gvec, const void* y, const float* stats4, const float* coef, const void* wpt,
                         const void* xr, const float* in_scale, const float* in_shift, void* dx, float* partials, float* ws, int B,
                         int H, int W, int dtype, int g_premasked, int sweep_reverse, void* stream);
int wm_conv3x3_bwd_fused_reduce(float* ws, float* dw, int accumulate, int B, int H, int W, int Cin, int Cout, const WmBnBwdFin* fin,
                                void* stream);
/* The encoder's after-concat layer WITHOUT the concat (16-bit dtypes).  replaces: /root/reference/hidden_models/encoder.py:34-41
 * (expand the message to [B,L,H,W], torch.cat([message, features, image]), then the 97 -> 64 ConvBNRelu of encoder.py:25).
 * A 3x3 conv is linear in its input channels and a message plane is constant over the image, so
 *   conv(cat) = conv64(features) + P,   P = conv3(image) + bias + sum_{taps inside the image} sum_l W[:, c_msg + l, tap] * msg[b, l].
 * wm_concat_side_fwd writes P [B,H,W,64] (dtype) in one pass from the f32 NCHW image planes img [B,3,H,W]; w [64][Cin][3][3] is the
 * layer's f32 weight in the reference's layout, the message channels are [c_msg, c_msg + L), the image channels [c_img, c_img + 3);
 * bias f32[64] or NULL; msg f32 [B][L].  Scratch owned by the caller: wside (4 KB, 16-byte aligned), mbias f32 [B][9][64].
 * wm_conv3x3_fwd_addin: y = conv3x3(relu(in_scale * x + in_shift), wp) + addend, dense [B,H,W,64] tensors, wp [9][64][64] from
 * wm_pack_w3x3 (the feature channels of w through its channel map); the BatchNorm statistics partials
 * f32[wm_conv3x3_nparts(B,H,W,64,64,dtype)][2][64] are taken AFTER the sum, so (y, partials) are the after-concat layer's.
 * Backward of the message channels: wm_concat_side_msg_wgrad, dw[:, c_msg + l, tap] (+)= sum_b msg[b,l] * S[b,tap,:], S = the sums of
 * dy [B,H,W,64] over the pixels for which `tap` lies inside the image; scratch: partial f32 [B][wm_concat_side_partial_rows()][64],
 * S f32 [B][9][64]; dw f32 [64][Cin][3][3].  (Feature and image channels of dw: wm_conv3x3_wgrad with a channel map.)
 * H, W >= 2; L <= 64; dtype WM_BF16 or WM_F16. */
int wm_concat_side_partial_rows(void);
int wm_concat_side_fwd(const float* img, const float* w, const float* bias, const float* msg, void* wside, float* mbias, void* P,
                       int B, int H, int W, int Cin, int c_msg, int L, int c_img, int dtype, void* stream);
int wm_concat_side_msg_wgrad(const void* dy, const float* msg, float* partial, float* S, float* dw, int accumulate, int B, int H,
                             int W, int Cin, int c_msg, int L, int dtype, void* stream);
int wm_conv3x3_fwd_addin(const void* x, const void* wp, const float* in_scale, const float* in_shift, const void* addend, void* y,
                         float* stat_partials, int B, int H, int W, int dtype, int sweep_reverse, void* stream);
/* conv + bias + ELU as ONE launch and that layer's backward in two (16-bit dtypes; rows f1 / f2).  replaces: the coupling subnets'
 * `elu(conv(x))` pairs, /root/reference/models/invertible_net.py:326-366 (ResBlock: conv1..conv4 + nn.ELU), whose autograd backward is
 * elu' * g, a bias column sum, the input gradient and the weight gradient -- five passes over the data here before.
 *   wm_conv3x3_fwd_elu       : out [B,H,W,64] = elu(conv3x3(x, wp) + bias); x [B,H,W,Cin] stride ldx, Cin in {16, 32, 64}; the pre-activation
 *                              is not stored: elu'(z) = out > 0 ? 1 : out + 1.
 *   wm_conv3x3_dgrad_elufused: g [B,H,W,64] = the gradient wrt out; forms gz = g * (out > 0 ? 1 : out + 1) while staging, writes
 *                              dx [B,H,W,CinP] = conv3x3(gz, wpt) (wpt from wm_pack_w3x3, transposed; CinP in {64, 32}; or CinP = 16 with
 *                              wpt packed to 32 rows, the upper 16 zero -- dx keeps its 16-channel stride), gz_out [B,H,W,64]
 *                              (NULL: not wanted) and bias_partials f32 [wm_conv3x3_dgrad_elufused_nparts(B,H,W)][64]: per-workgroup
 *                              column sums of gz (before its rounding to 16 bits).
 *   wm_conv3x3_wgrad_bias    : dw [Cout][Cin][3][3] (+)= the weight gradient from (x, gz) as wm_conv3x3_wgrad (ws: the same scratch), and in
 *                              the same reduction launch db [Cout] (+)= the column sums of bias_partials [nparts][CoutY]. */
int wm_conv3x3_fwd_elu_supported(int Cin, int CoutP, int dtype);
int wm_conv3x3_fwd_elu(const void* x, int ldx, const void* wp, const float* bias, int nbias, void* out, int B, int H, int W, int Cin,
                       int dtype, int sweep_reverse, void* stream);
int wm_conv3x3_dgrad_elufused_supported(int CinP, int dtype);
int wm_conv3x3_dgrad_elufused_nparts(int B, int H, int W);
int wm_conv3x3_dgrad_elufused(const void* g, const void* out, const void* wpt, void* dx, void* gz_out, float* bias_partials, int B,
                              int H, int W, int CinP, int dtype, int sweep_reverse, void* stream);
int wm_conv3x3_wgrad_bias(const void* x, int ldx, int CinX, const void* gz, int ldgz, int CoutY, float* ws, float* dw, int accumulate,
                          int B, int H, int W, int Cin, int Cout, int dtype, const float* bias_partials, int nparts, float* db,
                          int db_accumulate, void* stream);
/* The backward of an IMAGE-FED first ConvBNRelu (3 -> 64 channels; replaces autograd's backward of conv_bn_relu.py:11-15 for the layers of
 * decoder.py:16 / discriminator.py:13, whose input image needs a gradient) in ONE pass (csrc/bwd_ws16.hip): reads g, y [B,H,W,64] (gradient
 * wrt the layer's ReLU output, its raw conv output; stats4 / coef as wm_conv3x3_dgrad_applyfused) and the layer's input x [B,H,W,16] (the
 * image, 3 real channels), forms dy while staging and produces dx [B,H,W,16] = conv(dy, wpt) (wpt [9][16][64] from wm_pack_w3x3, transposed)
 * and dw [Cout][Cin][3][3] (+)= sum dy (x) x through ws (f32 [wm_conv3x3_bwd_fused16_nwg][9][16][64] slabs + wm_conv3x3_wgrad's reduction).
 * dy is never written: 335 MB per launch at B = 16, 256x256 instead of the two-kernel form's 637.  Whole-tile shapes only
 * (_supported: H % 8 == 0, W % 16 == 0, 16-bit dtype); g_premasked as wm_conv3x3_bwd_fused. */
int wm_conv3x3_bwd_fused16_supported(int B, int H, int W, int dtype);
int wm_conv3x3_bwd_fused16_nwg(int B, int H, int W);
int wm_conv3x3_bwd_fused16(const void* g, const void* y, const float* stats4, const float* coef, const void* wpt, const void* x, void* dx,
                           float* ws, float* dw, int accumulate, int B, int H, int W, int Cin, int Cout, int dtype, int g_premasked,
                           int sweep_reverse, void* stream);
int wm_conv3x3_dgrad_bwdstats_supported(int CoutY, int CinP, int dtype);
int wm_conv3x3_dgrad_bwdstats(const void* src, int lds, int CoutY, const void* wpt, const float* gvec, const float* stats4,
                              const float* coef, const void* ry, const float* r_scale, const float* r_shift, void* dx,
                              float* partials, int B, int H, int W, int CinP, int dtype, int sweep_reverse, void* stream);

/* ------------------------------------------------------------------ BatchNorm2d (training)
 * replaces nn.BatchNorm2d + nn.ReLU of conv_bn_relu.py:12-14 / UNet.py:67-97.
 * finalize: partial sums -> batch mean / biased var; scale = gamma*invstd,
 * (every *_finalize / colsum call treats its `partials` buffer as scratch: with more than 256 rows
 * it first folds them in place, in float32, to 64 rows, so the pointer is const only in name),
 * shift = beta - mean*scale; running stats updated with `momentum` and the unbiased var
 * (count/(count-1)), as torch does.  C real channels, CP padded (scale=shift=0 there). */
int wm_bn_finalize(const float* partials, int nparts, int C, int CP, double count, const float* gamma,
                   const float* beta, float* running_mean, float* running_var, float momentum,
                   float eps, float* scale, float* shift, float* mean, float* invstd, void* stream);
/* backward through ReLU + BatchNorm given g = dL/d(relu output) and the raw conv output y:
 *   pass 1 (reduce): partial sums of gz = g*[scale*y+shift>0] and gz*xhat   -> partials
 *   finalize       : dgamma, dbeta (f32[C], overwritten or accumulated), coefficient vectors
 *   pass 2 (apply) : dy = scale*(gz - c1 - xhat*c2), written as NHWC dtype; also column sums
 *                    of dy for the conv bias gradient.
 * g may be a per-sample vector gvec[B,CP] (gradient of a global average pool, already
 * divided by H*W) instead of a tensor: pass g=NULL and gvec. */
int wm_bn_bwd_nparts(size_t npix);
int wm_bn_bwd_reduce(const void* g, int ldg, const float* gvec, const void* y, int ldy,
                     const float* scale, const float* shift, const float* mean, const float* invstd,
                     float* partials, int B, size_t hw, int CP, int dtype, void* stream);
int wm_bn_bwd_finalize(const float* partials, int nparts, int C, int CP, double count,
                       const float* gamma, const float* invstd, float* dgamma, float* dbeta,
                       int accumulate, float* coef /* [3][CP]: a=gamma*invstd, c1, c2 */, void* stream);
/* the same for partial rows that hold sum(gz), sum(gz*y) (wm_conv3x3_dgrad_bwdstats): xhat is applied here */
int wm_bn_bwd_finalize_raw(const float* partials, int nparts, int C, int CP, double count, const float* gamma,
                           const float* mean, const float* invstd, float* dgamma, float* dbeta, int accumulate,
                           float* coef, void* stream);
int wm_bn_bwd_apply(const void* g, int ldg, const float* gvec, const void* y, int ldy,
                    const float* scale, const float* shift, const float* mean, const float* invstd,
                    const float* coef, void* dy, int lddy, float* dbias_partials, int B, size_t hw,
                    int CP, int dtype, void* stream);
/* column sums of partial rows: out[c] (+)= sum_p partials[p][c] (bias gradients). */
int wm_colsum_finalize(const float* partials, int nparts, int C, int ldp, float* out, int accumulate,
                       void* stream);

/* ------------------------------------------------------------------ heads
 * global average pool of relu(scale*y+shift): replaces nn.AdaptiveAvgPool2d((1,1)) at
 * hidden_models/decoder.py:24 / discriminator.py:16.  out f32[B,CP]. */
int wm_avgpool_slices(size_t hw);
int wm_bnrelu_avgpool(const void* y, int ldy, const float* scale, const float* shift, float* out,
                      float* ws /* f32[B * wm_avgpool_slices(hw) * CP] */, int B, size_t hw, int CP, int dtype,
                      void* stream);
/* Training form: out3 f32[3][B][CP] = the pooled mean, and per (sample, channel) the number of active pixels N+ = #[z > 0]
 * and S+ = the sum of y over them (ws: 3x the size above).  The pooled layer's gradient is one value per (sample, channel),
 * so its BatchNorm-backward sums follow from N+ / S+ without a pass over y: wm_pooled_bn_bwd_rows writes the B partial rows
 * rows f32[B][2][CP] = (gvec*N+, gvec*S+) for wm_bn_bwd_finalize_raw (replaces wm_bn_bwd_reduce with gvec). */
int wm_bnrelu_avgpool_stats(const void* y, int ldy, const float* scale, const float* shift, float* out3, float* ws, int B,
                            size_t hw, int CP, int dtype, void* stream);
int wm_pooled_bn_bwd_rows(const float* gvec, const float* npos, const float* ysum, int B, int CP, float* rows, void* stream);
/* the two steps in one launch: dgamma, dbeta, coef of the pooled layer straight from (gvec, N+, S+) */
int wm_bn_bwd_finalize_pooled(const float* gvec, const float* npos, const float* ysum, int B, int C, int CP, double count,
                              const float* gamma, const float* mean, const float* invstd, float* dgamma, float* dbeta,
                              int accumulate, float* coef, void* stream);
/* 1x1 conv Cin->Cout (Cout <= 4) on relu(scale*y+shift): replaces nn.Conv2d(64,3,1) at
 * hidden_models/encoder.py:28,42 and the sigmoid head of network/UNet.py:41-43,65.
 * w f32[Cout,Cin], bias f32[Cout]; out f32 NCHW [B,Cout,H,W]; act 0 = none, 1 = sigmoid. */
int wm_conv1x1_head_fwd(const void* y, int ldy, const float* scale, const float* shift, const float* w,
                        const float* bias, float* out, int B, size_t hw, int Cin, int Cout, int act,
                        int dtype, void* stream);
/* ... and, act16 non-NULL (act == 0): the result a second time as [B][HW][16] pixels of the activation dtype (channels 0..Cout-1, zero
 * tail) -- the tensor the image-fed first layers of the decoder / discriminator read (hidden_models/decoder.py:15, discriminator.py:12),
 * which wm_nchw_to_nhwc would otherwise make from `out` in a launch of its own. */
int wm_conv1x1_head_fwd_act(const void* y, int ldy, const float* scale, const float* shift, const float* w,
                            const float* bias, float* out, void* act16, int B, size_t hw, int Cin, int Cout, int act,
                            int dtype, void* stream);
/* backward: gout f32 NCHW [B,Cout,H,W] (for act=1 the caller passes the gradient wrt the
 * pre-sigmoid logits) -> g NHWC dtype [B,H,W,Cin] (gradient wrt the ReLU output), and
 * partial sums for dw[Cout,Cin], dbias[Cout]: partials f32[nparts][Cout*(Cin+1)].
 * bn_partials (may be NULL): f32[nparts][2][Cin] = per-workgroup sum(gz), sum(gz*y) of the ConvBNRelu that produced y (gz = g as
 * stored * [scale*y+shift > 0]) -- the rows wm_bn_bwd_finalize_raw takes, so that layer needs no wm_bn_bwd_reduce pass. */
int wm_conv1x1_head_nparts(size_t npix);
int wm_conv1x1_head_bwd(const void* y, int ldy, const float* scale, const float* shift, const float* w,
                        const float* gout, void* g, int ldg, float* partials, float* bn_partials, int B, size_t hw, int Cin,
                        int Cout, int dtype, void* stream);

/* ------------------------------------------------------------------ UNet pieces
 * 2x2 max pool of relu(scale*y+shift): replaces nn.MaxPool2d(2,2) (network/UNet.py:14-20).
 * Writes the activated full-resolution map too when act_out != NULL (the skip tensor). */
int wm_bnrelu_maxpool2(const void* y, int ldy, const float* scale, const float* shift, void* pooled,
                       int ldp, void* act_out, int lda, int c0a, int B, int H, int W, int C, int dtype,
                       void* stream);
/* gradient of the pool scattered back to full resolution, added to g_skip when given. */
int wm_maxpool2_bwd(const void* y, int ldy, const float* scale, const float* shift, const void* gpooled,
                    int ldgp, const void* g_skip, int ldgs, void* g, int ldg, int B, int H, int W, int C,
                    int dtype, void* stream);
/* ConvTranspose2d k=2 s=2 (network/UNet.py:24-38) on relu(scale*x+shift):
 * w f32[Cin,Cout,2,2], bias f32[Cout]; y NHWC [B,2H,2W,*] at channel offset c0. */
int wm_upconv2x2_fwd(const void* x, int ldx, const float* scale, const float* shift, const float* w,
                     const float* bias, void* y, int ldy, int c0, int B, int H, int W, int Cin, int Cout,
                     int dtype, void* stream);
/* backward: gx = gradient wrt the (activated) input, NHWC [B,H,W,Cin]; w_t = the weight
 * rearranged to [(i,j,co)][Cin] f32 (weight.permute(2,3,1,0)); dw_partials f32
 * [wm_upconv2x2_dw_chunks(B,H,W)][Cin+1][4*Cout]: per-chunk partial sums of the weight gradient in
 * PyTorch order (row ci, column co*4+i*2+j) with the per-column sums of gy in the extra row Cin
 * (bias gradient = sum over the 4 taps); reduce with wm_colsum_finalize. */
int wm_upconv2x2_dw_chunks(int B, int H, int W);
int wm_upconv2x2_bwd(const void* x, int ldx, const float* scale, const float* shift, const float* w_t,
                     const void* gy, int ldgy, int c0, void* gx, int ldgx, float* dw_partials,
                     int B, int H, int W, int Cin, int Cout, int dtype, void* stream);
/* MFMA form of the same layer for bf16 with Cin % 64 == 0 and Cout % 16 == 0 (network/UNet.py:14-38 at every level):
 * four 1x1 GEMMs over the input pixels + pixel shuffle.  wm_upconv2x2_pack builds the two 16-bit (bf16 / f16) operands from the
 * PyTorch weight [Cin][Cout][2][2]: wf [(ij,co)][Cin] (forward) and wb [Cin][(ij,co)] (dgrad).
 *   fwd  : y[b,2h+i,2w+j,c0+co] = bias[co] + sum_ci relu(scale*x+shift)[b,h,w,ci] * w[ci,co,i,j]
 *   dgrad: gx[b,h,w,ci] = sum_(i,j,co) gy[b,2h+i,2w+j,c0+co] * w[ci,co,i,j]   (gradient wrt the ACTIVATED input)
 *   wgrad: dw[ci,co,i,j] (+)= sum_(b,h,w) relu(scale*x+shift)[b,h,w,ci] * gy[b,2h+i,2w+j,c0+co];  dbias[co] (+)= sum gy
 *          partial: f32[wm_upconv2x2_wgrad_nsplit][Cin][4*Cout], bias_partial: f32[nsplit][4*Cout] (scratch). */
int wm_upconv2x2_mfma_supported(int Cin, int Cout, int dtype);
int wm_upconv2x2_pack(const float* w, void* wf, void* wb, int Cin, int Cout, int dtype, void* stream);   /* dtype: WM_BF16 or WM_F16 */
int wm_upconv2x2_fwd_mfma(const void* x, int ldx, const float* scale, const float* shift, const void* wf, const float* bias,
                          void* y, int ldy, int c0, int B, int H, int W, int Cin, int Cout, int dtype, void* stream);
int wm_upconv2x2_dgrad_mfma(const void* gy, int ldgy, int c0, const void* wb, void* gx, int ldgx, int B, int H, int W, int Cin,
                            int Cout, int dtype, void* stream);
int wm_upconv2x2_wgrad_nsplit(int B, int H, int W, int Cin, int Cout);
int wm_upconv2x2_wgrad_mfma(const void* x, int ldx, const float* scale, const float* shift, const void* gy, int ldgy, int c0,
                            float* partial, float* bias_partial, float* dw, float* dbias, int accumulate, int B, int H, int W,
                            int Cin, int Cout, int dtype, void* stream);

/* ------------------------------------------------------------------ losses / optimiser
 * sum((a-b)^2) partials and gradient 2*w*(a-b)/n of nn.MSELoss (hidden.py:37,90).
 * gscale_dev (here and in wm_bce_logits / wm_message_loss / wm_bce_logits_target / wm_mse_fwd_bwd_gated; may be NULL): a device
 * scalar multiplied into gscale -- the loss scale of mixed-precision training (wm_amp_*), which lives on the device. */
int wm_mse_fwd_bwd(const float* a, const float* b, float* grad_a, float gscale, const float* gscale_dev, float* loss_partials,
                   int nparts, size_t n, void* stream);
/* hidden.py:85-101 at the encoded image, one pass: out [B][C][HW] f32 = (f32)g[b][q][c0 + c] + gscale * (a - b), with g the NHWC input
 * gradient of the discriminator's first layer (dtype, pixel stride ld; C <= 4 real channels from c0), a = encoded, b = cover (f32 NCHW);
 * loss_partials [nparts] = partial sums of (a - b)^2 over the blocks (wm_hidden_metrics adds them).  Same values as wm_nhwc_to_nchw +
 * wm_mse_fwd_bwd + wm_axpy(1.0). */
int wm_image_grad_mse(const void* g, int ld, int c0, const float* a, const float* b, float* out, float gscale, const float* gscale_dev,
                      float* loss_partials, int nparts, int B, int C, int H, int W, int dtype, void* stream);
/* y = a + s*b (f32), used to combine image-space gradients. */
int wm_axpy(float* a, const float* b, float s, size_t n, void* stream);
/* Adam / AdamW step over one flat f32 parameter buffer (torch.optim.Adam semantics,
 * hidden.py:24-25: lr 1e-3, betas (0.9,0.999), eps 1e-8, weight_decay 0, no amsgrad).
 * step = 1-based step count.  decoupled != 0 gives AdamW. */
int wm_adam_step(float* p, const float* g, float* m, float* v, size_t n, float lr, float beta1,
                 float beta2, float eps, float weight_decay, int decoupled, int step, float grad_scale,
                 void* stream);
/* The same step for a hipGraph-captured training step (a Python step per batch per rank, /root/reference/train.py:99-109, replayed
 * instead of re-enqueued): every number that may change between replays -- the step-count-dependent constants and the hyperparameters
 * a scheduler or a loaded state_dict changes -- comes from DEVICE memory instead of the argument list.
 * wm_adam_hyper (host, no launch): out[WM_ADAM_HYPER] = {lr / (1 - beta1^step), sqrt(1 - beta2^step), lr, beta1, beta2, eps,
 * weight_decay, 0} -- the first two exactly the values wm_adam_step derives; wm_adam_step_dev reads the block from hyper_dev
 * (device float[WM_ADAM_HYPER]), which the caller refreshes before each replay: bit-identical to wm_adam_step(step).  Only
 * `decoupled`, which selects a code path, stays a launch argument. */
#define WM_ADAM_HYPER 8
int wm_adam_hyper(float lr, float beta1, float beta2, float eps, float weight_decay, int step, float* out);
int wm_adam_step_dev(float* p, const float* g, float* m, float* v, size_t n, int decoupled, const float* hyper_dev, float grad_scale,
                     void* stream);
/* sum of squares partials (clip_grad_norm_) */
/* nn.Linear after the global average pool (hidden_models/decoder.py:26,32-34, discriminator.py:18,24-26), B ~ 16, I,O <= 64:
 * fwd: out[B,O] = pooled[:, :I] @ w[O,I]^T + bias.
 * bwd: dw[O,I] (+)= g_out^T @ pooled, db[O] (+)= sum_b g_out, gvec[B,CP] = (g_out @ w) * inv_hw zero padded to CP -- the
 *      per-sample gradient vector wm_bn_bwd_* take for a globally pooled output. */
int wm_linear_head_fwd(const float* pooled, int ldp, const float* w, const float* bias, float* out, int B, int I, int O,
                       void* stream);
int wm_linear_head_bwd(const float* pooled, int ldp, const float* w, const float* g_out, float* dw, float* db,
                       int accumulate, float* gvec, int CP, float inv_hw, int B, int I, int O, void* stream);
/* The four small launches a pooled head runs in a row -- wm_linear_head_fwd, the loss (kind 0: wm_bce_logits against the constant label
 * `target`; kind 1: wm_message_loss against messages [B][O]), wm_linear_head_bwd and wm_bn_bwd_finalize_pooled of the pooled ConvBNRelu --
 * as ONE launch of one workgroup, each stage with the arithmetic (and operation order) of the kernel it replaces.
 * out3 [3][B][CP] = wm_bnrelu_avgpool_stats' result (pooled mean, N+, S+); logits [B][O]; loss_out [1] (kind 0) / [2] (kind 1: MSE, bitwise
 * error); dw [O][I], db [O] (+)=; gvec [B][CP]; C, count, gamma, mean, invstd, dgamma, dbeta, coef [3][CP] as wm_bn_bwd_finalize_pooled.
 * wm_pooled_head_supported: the sizes one workgroup's LDS holds (B*CP <= 2048, O*I <= 4096, B*O <= 1024). */
int wm_pooled_head_supported(int B, int CP, int I, int O);
int wm_pooled_head(const float* out3, int B, int CP, int I, int O, const float* w, const float* bias, int kind, float target,
                   const float* messages, float gscale, const float* gscale_dev, float* logits, float* loss_out, float* dw, float* db,
                   int accumulate, float* gvec, float inv_hw, int C, double count, const float* gamma, const float* mean,
                   const float* invstd, float* dgamma, float* dbeta, float* coef, void* stream);
/* nn.BCEWithLogitsLoss (mean) of n logits against a constant label (hidden_models/hidden.py:68-97): *loss_out = the
 * loss, grad_out[n] (may be NULL) = gscale * d loss / d logits.  One small launch. */
int wm_bce_logits(const float* logits, float target, int n, float gscale, const float* gscale_dev, float* loss_out, float* grad_out,
                  void* stream);
/* decoder message loss (hidden.py:96-99,109-111) on n = B*L values: out2[0] = mean (d-m)^2,
 * out2[1] = mean |clip(round(d),0,1) - m| (the bitwise error), grad_out[n] (may be NULL) = gscale * (d - m). */
int wm_message_loss(const float* decoded, const float* messages, int n, float gscale, const float* gscale_dev, float* out2,
                    float* grad_out, void* stream);
/* the seven scalars hidden.py:105-113 logs, in one launch: out7 = [w_adv*adv + w_enc*enc + w_dec*dec, enc, dec, bit error,
 * adv, d_cover, d_encoded] with enc = sum(enc_partials[nparts]) / n_img (wm_mse_fwd_bwd's rows), msg2 = wm_message_loss's
 * out2, adv / d_cover / d_enc = device scalars written by wm_bce_logits. */
int wm_hidden_metrics(const float* enc_partials, int nparts, double n_img, const float* msg2, const float* adv,
                      const float* d_cover, const float* d_enc, float w_adv, float w_enc, float w_dec, float* out7, void* stream);
int wm_sumsq(const float* x, size_t n, float* partials, int nparts, void* stream);

/* ------------------------------------------------------------------ mixed precision: torch.cuda.amp.GradScaler on the device
 * replaces: models/IRNcrop_model.py:143 (GradScaler()), :407 (scaler.scale(loss).backward()), :413-416 (scaler.step x2, scaler.update()).
 * state: f32[WM_AMP_STATE] device array = [0] loss scale, [1] growth tracker, [2] growth_factor, [3] backoff_factor,
 * [4] growth_interval, [8+k] found_inf of optimiser k, [12+k] step count of optimiser k (k < 4).  The loss kernels take &state[0]
 * as gscale_dev, so every gradient of the backward is multiplied by the scale; then, per optimiser,
 *   wm_nonfinite     : partials[nparts] = per block, 1 if any of its elements of x is inf / nan, else 0
 *   wm_amp_found_inf : found_inf[k] = any of its wm_nonfinite rows != 0         (GradScaler.unscale_'s per-element inf check; a finite
 *                      gradient whose square overflows f32 is stepped, as torch steps it)
 *   wm_adam_step_amp : the Adam step on g / scale, skipped when found_inf[k]; bias corrections from the device step count,
 *                      which a skipped step does not advance (like torch's per-parameter `step`).  hyper_dev (may be NULL: the
 *                      arguments hold): a wm_adam_hyper block whose lr, beta1, beta2, eps and weight_decay replace the arguments
 *                      (a captured step); its two step-count-dependent entries are not read
 * and once per iteration wm_amp_update: GradScaler.update() (backoff on any inf, growth after growth_interval clean iterations),
 * advances the step counts of the optimisers that stepped and clears the flags.  No host synchronisation anywhere. */
#define WM_AMP_STATE 16
int wm_nonfinite(const float* x, size_t n, float* partials, int nparts, void* stream);
int wm_amp_found_inf(const float* const* nonfinite_partials, const int* nparts, int ngroups, float* state, int k, void* stream);
int wm_adam_step_amp(float* p, const float* g, float* m, float* v, size_t n, float lr, float beta1, float beta2, float eps,
                     float weight_decay, int decoupled, float grad_scale, const float* amp_state, int k, const float* hyper_dev,
                     void* stream);
int wm_amp_update(float* state, int noptimizers, void* stream);

/* ------------------------------------------------------------------ tamper-localisation branch (elementwise, f32 NCHW planes)
 * replaces: models/IRNcrop_model.py:320-322 (clamp_with_grad), :344-345 / :372-373 (Quantization after the clamp),
 * :348 (splice), :379-388 (PSNR of the int-truncated images, metrics.py:30-46, and the 1.0 / 0.8 forward weight at 33 dB),
 * :378,391-393 (BCEWithLogitsLoss on the predicted mask), :410-412 (clip_grad_norm_).
 * wm_clamp_quant_fwd: y = round(255*clamp(x,0,1))/255 (backward of both = identity: nothing to launch).
 * wm_splice_fwd: q = clamp_quant(enc); fwd_q (may be NULL) = q; tampered (may be NULL) = q*(1-mask) + prev*mask with mask
 *   [B,1,HW] broadcast over the C planes; psnr_partials [wm_splice_nparts(B*C*HW)] doubles (with real; both may be NULL) =
 *   partial sums of (int(255*real) - int(255*q))^2.
 * wm_copymove_fwd (models/IRNp_model.py:561-598, :1007-1037, the copy-move forgery): q = clamp_quant(enc) [B,C,H,W];
 *   mask_shifted[b,0,i,j] = clamp01(mask[b,0,i-sx_b,j-sy_b]) and t[b,c,i,j] = q[b,c,i-sx_b,j-sy_b], both 0 where the source pixel lies
 *   outside the frame; tampered = q*(1-mask_shifted) + t*mask_shifted; fwd_q (may be NULL) = q.  shifts: device int32 [B][2] = (sx_b rows,
 *   sy_b columns), clamped to [-H,H] x [-W,W] by the kernel (a larger magnitude has the same effect).  partials (may be NULL without real)
 *   = [2][wm_splice_nparts(B*C*H*W)] doubles: row 0 as wm_splice_fwd's psnr_partials (zeros when real is NULL), row 1 partial sums of
 *   mask_shifted (valid = their sum / (B*H*W)).  Not in place; B*C*H < 2^31 (WM_E_SHAPE).
 * wm_copymove_valid: out[0] = (sum of row 1 of wm_copymove_fwd's partials [2][nparts]) / count, added in double in a fixed order
 *   (IRNp_model.py:592 valid = torch.mean(masks), count = B*H*W); wm_psnr_gate reads row 0 as it reads wm_splice_fwd's partials.
 * wm_psnr_gate: out2[0] = PSNR (0 when the images are equal, like metrics.py:41-42), out2[1] = PSNR < threshold ? w_below : w_above.
 * wm_mse_fwd_bwd_gated: wm_mse_fwd_bwd with the gradient scale multiplied by the device scalar gate_dev[0].
 * wm_bce_logits_target: *loss_out = mean BCE-with-logits(p, target), grad_out (may be NULL) = gscale * d loss / d p;
 *   partials = scratch [nparts <= 2048]; chain_sigmoid != 0: p is a sigmoid output s(z) (the UNet head, network/UNet.py:65) and
 *   grad_out is taken wrt z (multiplied by p*(1-p)).
 * wm_masked_axpy: a += g * (1 - mask) (the splice's backward onto the gradient of the encoded image).
 * wm_mask_threshold: out[i] = p[i] > threshold (uint8 tamper mask).
 * wm_clip_coef: partials[k][nparts[k]] = wm_sumsq rows of up to 4 flat gradient buffers clipped TOGETHER;
 *   out2[0] = min(1, max_norm / (total_norm + 1e-6)), out2[1] = total_norm; a nan norm gives a nan coefficient, as torch.clamp does.   wm_scale_dev: x *= scale_dev[0]. */
int wm_clamp_quant_fwd(const float* x, float* y, size_t n, void* stream);
int wm_splice_nparts(size_t n);
int wm_splice_fwd(const float* enc, const float* real, const float* prev, const float* mask, float* fwd_q, float* tampered,
                  double* psnr_partials, int B, int C, size_t HW, void* stream);
int wm_copymove_fwd(const float* enc, const float* real, const float* mask, const int* shifts, float* fwd_q, float* tampered,
                    float* mask_shifted, double* partials, int B, int C, int H, int W, void* stream);
int wm_copymove_valid(const double* partials, int nparts, double count, float* out, void* stream);
int wm_psnr_gate(const double* psnr_partials, int nparts, double n, float threshold, float w_below, float w_above, float* out2,
                 void* stream);
int wm_mse_fwd_bwd_gated(const float* a, const float* b, float* grad_a, float gscale, const float* gate_dev, const float* gscale_dev,
                         float* loss_partials, int nparts, size_t n, void* stream);
int wm_bce_logits_target(const float* p, const float* target, size_t n, float gscale, const float* gscale_dev, float* partials, int nparts,
                         float* loss_out, float* grad_out, int chain_sigmoid, void* stream);
int wm_masked_axpy(float* a, const float* g, const float* mask, int B, int C, size_t HW, void* stream);
int wm_mask_threshold(const float* p, float threshold, uint8_t* out, size_t n, void* stream);
int wm_clip_coef(const float* const* partials, const int* nparts, int ngroups, float max_norm, float* out2, void* stream);
int wm_scale_dev(float* x, size_t n, const float* scale_dev, void* stream);

/* ------------------------------------------------------------------ general layer family
 * replaces, for models/networks.py:631-749 (Discriminator), models/conditional_jpeg_generator.py:40-79 (conv()), :83-96 (ResBlock),
 * :185-200 (QFAttention), :202-374 (FBCNN), :697-826 (QF_predictor): nn.Conv2d / nn.ConvTranspose2d / nn.Linear of any kernel size
 * up to 5x5, stride 1 or 2, zero padding, with bias; their input and weight gradients; the activations; AdaptiveAvgPool2d((1,1));
 * symm_pad (:865-885) / ReplicationPad2d; nn.utils.spectral_norm (networks.py:1381-1385); the Bayar constraint (:814-817).
 * Activations NHWC [B,H,W,Cp] of `dtype` (WM_F32 / WM_BF16 / WM_F16) with the channel stride Cp a multiple of 16 and the padding
 * channels ignored by every consumer; parameters, per-sample vectors and their gradients f32 in torch's layouts.
 * wm_gconv_pack : w [Cout][Cin][KH][KW] f32 -> wp [KH*KW][RP][CP] dtype, rows = Cout, cols = Cin (transpose 0) or rows = Cin,
 *                 cols = Cout (transpose 1: the operand of the input gradient / of ConvTranspose2d's forward); padding zero.
 * wm_gconv_fwd  : dgrad 0: out [B,OH,OW,NC] = conv(in [B,IH,IW,KC], w [taps][NC][KC]) + bias [NC] (may be NULL);
 *                 dgrad 1: in = the conv's output-side tensor [B,IH,IW,KC], out = its input-side tensor [B,OH,OW,NC]
 *                 (the conv's input gradient, or ConvTranspose2d's forward), w packed with transpose 1.
 * wm_gconv_wgrad: dw [Cout][Cin][KH][KW] (+)= sum_pixels dout x in; dbias [Cout] (+)= column sums of dout (may be NULL);
 *                 partial = f32 scratch of wm_gconv_wgrad_scratch_floats(..) floats.  IH/IW/KC describe `in`, OH/OW/NC `dout`.
 * wm_gcolsum    : out [Creal] (+)= column sums of x [npix][C]; scratch: wm_gcolsum_scratch_floats(npix, C) floats.
 * wm_gcolsum_f64: the same sums accumulated in double in a fixed order and rounded to f32 once (no scratch): the bias gradient of a
 *                 network's output convolution, a sum over every pixel of the loss gradient.
 * wm_unary_fwd / _bwd: kind 0 ReLU, 1 LeakyReLU(0.2), 2 GELU (erf), 3 ELU, 4 Sigmoid, 5 Tanh; the backward reads the INPUT x --
 *                 except kind 6 (backward only): the ELU derivative from the layer's OUTPUT, out > 0 ? 1 : out + 1 (wm_conv3x3_fwd_elu keeps no input).
 * wm_add_scaled : out = a + alpha * b.
 * wm_qfatt_fwd  : out = x + gamma[b,c] * res + beta[b,c] (gamma / beta f32 [B][ldv]); wm_qfatt_bwd: gres = gamma * g,
 *                 ggamma[b,c] = sum_p g * res, gbeta[b,c] = sum_p g (the gradient wrt x is g itself); scratch:
 *                 wm_qfatt_bwd_scratch_floats(B, hw, ldv) floats.  Both need ldv >= C; wm_qfatt_bwd also needs C % 16 == 0 (it walks
 *                 16-byte vectors of 64-channel blocks, like wm_unary_bwd_colsum) and returns WM_E_BADARG otherwise; columns [C, ldv)
 *                 of ggamma / gbeta are left as they were.
 * wm_gpool_fwd  : out f32 [B][C] = mean over the hw pixels of x [B,hw,C]; wm_gpool_bwd: gx = g / hw.
 * wm_pad_nchw_to_nhwc(_bwd): x [B,C,H,W] f32 -> out [B,H+top+bottom,W+left+right,CP], mode 0 symmetric, 1 replicate (pads may
 *                 be 0: a plain layout change); the backward sums every padded position back onto its source pixel.
 * wm_gunpack_nchw(_bwd): the top-left H x W window and first C channels of x [B,PH,PW,CP] -> [B,C,H,W] f32, and its adjoint.
 * wm_spectral_norm_fwd: W [M][N] = weight_orig.view(Cout,-1); do_iter != 0 (training): v = normalize(W^T u), u = normalize(W v)
 *                 in place (eps 1e-12); sigma = u.(W v); Wsn = W / sigma; scratch: wm_spectral_norm_scratch_floats(M, N) floats.
 *                 wm_spectral_norm_bwd: gW (+)= (G - <G,Wsn> u v^T)/sigma
 *                 (u, v detached, as torch computes them under no_grad); partial = f32[256] scratch.
 * wm_bayar_constrain: every 5x5 filter of w [nfilters][25] in place: centre := 0, filter *= 1 / its sum, centre := -1; the sum is
 *                 a left-to-right f32 sum of the 25 taps, a zero sum gives inf / nan as in the reference.
 *                 wm_bayar_constrain_torch_order (networks.py:1059-1061): the same with the f32 sum in the order torch.sum over the
 *                 last two axes takes on the CPU, l_j = (x[j] + x[j+8]) + x[j+16] for j < 8, then x[24] + l_0 + ... + l_7: the reference's
 *                 float32 result bit for bit.
 * wm_gconv_dil_fwd / wm_gconv_dil_wgrad: wm_gconv_fwd / wm_gconv_wgrad with a dilation `dil` (1..8; dil > 1 needs stride 1, else
 *                 WM_E_BADARG): forward source pixel oy*stride - pad + ky*dil, input-gradient source pixel oy + pad - ky*dil
 *                 (networks.py:1387-1421 ResnetBlock).  Same packed filters, same scratch (wm_gconv_wgrad_scratch_floats); with dil > 1 the
 *                 output grid must be the one the geometry gives.  dil = 1 is wm_gconv_fwd / wm_gconv_wgrad bit for bit.
 * wm_reflect_pad_fwd / _bwd: nn.ReflectionPad2d(pad) on x [B,H,W,CP] -> out [B,H+2pad,W+2pad,CP] (pad <= min(H,W) - 1, else
 *                 WM_E_SHAPE) and its adjoint g [B,H+2pad,W+2pad,CP] -> gx [B,H,W,CP]; both gather 16-byte channel vectors, the adjoint
 *                 adds its <= 9 terms in f32 in a fixed order (no atomics). */
int wm_gconv_pack(const float* w, void* wp, int Cout, int Cin, int KH, int KW, int RP, int CP, int transpose, int dtype, void* stream);
int wm_gconv_fwd(const void* in, const void* w, const float* bias, void* out, int B, int IH, int IW, int KC, int OH, int OW, int NC,
                 int KH, int KW, int stride, int pad, int dgrad, int dtype, void* stream);
int wm_gconv_wgrad_nsplit(int B, int OH, int OW, int KC, int NC, int KH, int KW);
int wm_gconv_wgrad(const void* dout, const void* in, float* partial, float* dw, float* dbias, int accumulate, int B, int IH, int IW,
                   int KC, int OH, int OW, int NC, int KH, int KW, int stride, int pad, int Cout, int Cin, int dtype, void* stream);
size_t wm_gconv_wgrad_scratch_floats(int B, int OH, int OW, int KC, int NC, int KH, int KW);
size_t wm_gcolsum_scratch_floats(size_t npix, int C);
int wm_gcolsum(const void* x, size_t npix, int C, float* out, int Creal, int accumulate, float* scratch, int dtype, void* stream);
int wm_gcolsum_f64(const void* x, size_t npix, int C, float* out, int Creal, int accumulate, int dtype, void* stream);
int wm_unary_fwd(const void* x, void* y, size_t n, int kind, int dtype, void* stream);
int wm_unary_bwd(const void* x, const void* gy, void* gx, size_t n, int kind, int dtype, void* stream);
/* gx = gy * act'(x) over x [npix][C] AND out [Creal] (+)= the column sums of gx as stored -- the bias gradient of the nn.Conv2d whose
 * output the activation took (conditional_jpeg_generator.py / invertible_net.py:326-366's conv -> ELU / ReLU pairs): one pass over the
 * data + a reduce of the split partials.  part: wm_unary_bwd_colsum_scratch_floats(npix, C) floats. */
size_t wm_unary_bwd_colsum_scratch_floats(size_t npix, int C);
int wm_unary_bwd_colsum(const void* x, const void* gy, void* gx, size_t npix, int C, int kind, float* part, float* out, int Creal,
                        int accumulate, int dtype, void* stream);
int wm_add_scaled(const void* a, const void* b, void* out, size_t n, float alpha, int dtype, void* stream);
int wm_qfatt_fwd(const void* x, const void* res, const float* gamma, const float* beta, void* out, int B, size_t hw, int C, int ldv,
                 int dtype, void* stream);
size_t wm_qfatt_bwd_scratch_floats(int B, size_t hw, int ldv);
int wm_qfatt_bwd(const void* g, const void* res, const float* gamma, void* gres, float* ggamma, float* gbeta, float* scratch, int B, size_t hw,
                 int C, int ldv, int dtype, void* stream);
int wm_gpool_fwd(const void* x, float* out, int B, size_t hw, int C, int dtype, void* stream);
int wm_gpool_bwd(const float* g, void* gx, int B, size_t hw, int C, int dtype, void* stream);
int wm_pad_nchw_to_nhwc(const float* x, void* out, int B, int C, int H, int W, int left, int right, int top, int bottom, int mode,
                        int CP, int dtype, void* stream);
int wm_pad_nchw_to_nhwc_bwd(const void* gp, float* gx, int B, int C, int H, int W, int left, int right, int top, int bottom, int mode,
                            int CP, int dtype, void* stream);
int wm_gunpack_nchw(const void* x, float* out, int B, int C, int H, int W, int PH, int PW, int CP, int dtype, void* stream);
int wm_gunpack_nchw_bwd(const float* g, void* gx, int B, int C, int H, int W, int PH, int PW, int CP, int dtype, void* stream);
size_t wm_spectral_norm_scratch_floats(int M, int N);
int wm_spectral_norm_fwd(const float* W, float* u, float* v, float* sigma, float* Wsn, float* scratch, int M, int N, int do_iter, void* stream);
int wm_spectral_norm_bwd(const float* G, const float* Wsn, const float* u, const float* v, const float* sigma, float* partial,
                         float* gW, int M, int N, int accumulate, void* stream);
int wm_bayar_constrain(float* w, int nfilters, void* stream);
int wm_bayar_constrain_torch_order(float* w, int nfilters, void* stream);
int wm_gconv_dil_fwd(const void* in, const void* w, const float* bias, void* out, int B, int IH, int IW, int KC, int OH, int OW, int NC,
                     int KH, int KW, int stride, int pad, int dil, int dgrad, int dtype, void* stream);
int wm_gconv_dil_wgrad(const void* dout, const void* in, float* partial, float* dw, float* dbias, int accumulate, int B, int IH, int IW,
                       int KC, int OH, int OW, int NC, int KH, int KW, int stride, int pad, int dil, int Cout, int Cin, int dtype, void* stream);
int wm_reflect_pad_fwd(const void* x, void* out, int B, int H, int W, int CP, int pad, int dtype, void* stream);
int wm_reflect_pad_bwd(const void* g, void* gx, int B, int H, int W, int CP, int pad, int dtype, void* stream);

/* ------------------------------------------------------------------ invertible embedder pieces
 * replaces, for models/invertible_net.py: HaarDownsampling / HaarUpsampling (:178-292: F.conv2d / F.conv_transpose2d with the fixed
 * 2x2 Haar filters, groups = channels), RNVPCouplingBlock's affine (:140-141,153-173), and the channel narrow / cat around the
 * subnets (:150-151,175,318-322,363).  NHWC tensors of `dtype`; the coupling subnets' convolutions are wm_gconv_*.
 * wm_haar: up 0 (analysis): in [B,2H,2W,CPin] with C channels -> out [B,H,W,CPout], channel 4c+k = fac * (Haar filter k of channel c),
 *          k = 0 sum, 1 horizontal, 2 vertical, 3 diagonal difference; up 1 (synthesis): in [B,H,W,CPin] with 4C channels ->
 *          out [B,2H,2W,CPout] with C channels, scaled by fac.  Each is the other's adjoint (= its backward) for equal fac; padding
 *          channels of `out` are written as zero.  Bit 1 of `up` (values 2, 3): HaarDownsampling(order_by_wavelet=True) (:207-218,
 *          :225-233) -- the 4C channels ordered wavelet-major, k C + c.
 * wm_chan_copy: dst[p][doff + c] = src[p][soff + c] for c < n over npix pixels (strides in elements).
 * wm_coupling_fwd: rev 0: y = e(s) * x + t; rev 1: y = (x - t) / e(s); e(s) = exp(clamp * (2 sigmoid(s) - 1)) + eps.
 * wm_coupling_bwd: gradients wrt x, s, t from g = dL/dy; v = x for rev 0, v = the forward's OUTPUT y for rev 1. */
int wm_haar(const void* in, void* out, int B, int H, int W, int C, int CPin, int CPout, float fac, int up, int dtype, void* stream);
int wm_chan_copy(const void* src, void* dst, size_t npix, int sstride, int soff, int dstride, int doff, int n, int dtype, void* stream);
/* dst [npix][dstride] written WHOLE in one launch: a's channel window [aoff, aoff + na) lands at channel adst, b's (b may be NULL) at bdst,
 * zero elsewhere: x.narrow / torch.cat on the channel dimension (invertible_net.py:135-145, :358) and their adjoints on stride-padded NHWC. */
int wm_chan_place(const void* a, int astride, int aoff, int adst, int na, const void* b, int bstride, int boff, int bdst, int nb, void* dst,
                  int dstride, size_t npix, int dtype, void* stream);
int wm_coupling_fwd(const void* x, const void* s, const void* t, void* y, size_t n, float clamp, float eps, int rev, int dtype, void* stream);
int wm_coupling_bwd(const void* g, const void* v, const void* s, void* gx, void* gs, void* gt, size_t n, float clamp, float eps, int rev,
                    int dtype, void* stream);

/* ------------------------------------------------------------------ InvBlockExp couplings (csrc/invblock.hip)
 * replaces, for models/modules/Inv_arch.py InvBlockExp (:55-88), everything but the subnets F, G, H: x.narrow, the add, sigmoid / exp /
 * mul / div, torch.cat and torch.sum(self.s).  n1 = split_len1, n2 = split_len2, cp(n) = n rounded up to 16.  NHWC tensors of `dtype`, f32
 * arithmetic; x is the block's input [npix][xstride], read in place: x1 = channels [0, n1), x2 = channels [n1, n1 + n2) (WM_E_BADARG when
 * they do not fit the stride, or a stride is no multiple of 16).  Padding channels of every output are written as zero, those of an input
 * are never used.  16-byte accesses when every base pointer is 16-byte aligned, element accesses otherwise: the same bits either way.
 * wm_invblock_shift : v = x1 + sign * f (sign +1 / -1), f [npix][cp(n1)].  other == NULL: out [npix][cp(n1)] = v (the forward's y1);
 *                     other [npix][cp(n2)]: out [npix][cp(n1+n2)] = cat(v, other[:, :n2]) (the reverse's block output).
 * wm_invblock_affine: s = clamp * (2 sigmoid(h) - 1); rev 0: v = x2 * exp(s) + g; rev 1: v = (x2 - g) / exp(s); h, g [npix][cp(n2)].
 *                     other [npix][cp(n1)]: out [npix][cp(n1+n2)] = cat(other[:, :n1], v) (the forward's block output); other == NULL:
 *                     out [npix][cp(n2)] = v (the reverse's y2).  npix = B * hw.  jac != NULL: jac[b] = the sum of s over sample b's hw pixels
 *                     and n2 channels, added in double in a fixed order (per-workgroup partials in `scratch`, wm_invblock_scratch_doubles
 *                     doubles, then one small launch) and stored as f32: two calls give the same bits.  exp(s) is wm_coupling_fwd's e(s), eps = 0.
 * wm_invblock_shift_bwd : gout = dL/dout, whole != 0: [npix][cp(n1+n2)] as the forward wrote it with `other`, else [npix][cp(n1)].
 *                     gx [npix][gxstride] = dL/dx (gout in channels < n1, zero elsewhere), gf [npix][cp(n1)] = sign * gout,
 *                     gother [npix][cp(n2)] = gout's channels [n1, n1+n2) (whole only, NULL otherwise).
 * wm_invblock_affine_bwd: gout as above (whole: the v channels are read in place at n1; else [npix][cp(n2)]).  v = x for rev 0 (vstride =
 *                     xstride, voff = n1), the forward's stored OUTPUT for rev 1 (voff = n1 in the whole form, 0 otherwise) -- wm_coupling_bwd's
 *                     rule.  gx [npix][gxstride] (zero outside [n1, n1+n2)), gh, gg [npix][cp(n2)], gother [npix][cp(n1)] = gout's
 *                     channels < n1 (whole only). */
int wm_invblock_shift(const void* x, int xstride, const void* f, const void* other, void* out, size_t npix, int n1, int n2, float sign,
                      int dtype, void* stream);
int wm_invblock_shift_bwd(const void* gout, int whole, void* gx, int gxstride, void* gf, void* gother, size_t npix, int n1, int n2,
                          float sign, int dtype, void* stream);
size_t wm_invblock_scratch_doubles(int B, size_t hw, int n1, int n2);
int wm_invblock_affine(const void* x, int xstride, const void* h, const void* g, const void* other, void* out, float* jac,
                       double* scratch, int B, size_t hw, int n1, int n2, float clamp, int rev, int dtype, void* stream);
int wm_invblock_affine_bwd(const void* gout, int whole, const void* v, int vstride, int voff, const void* h, void* gx, int gxstride,
                           void* gh, void* gg, void* gother, size_t npix, int n1, int n2, float clamp, int rev, int dtype,
                           void* stream);

/* ------------------------------------------------------------------ instance normalisation (csrc/instnorm.hip)
 * replaces nn.InstanceNorm2d(C, eps, affine, track_running_stats=False) and the nn.ReLU behind it: models/modules/Subnet_constructor.py:149-169
 * (ResBlock, the coupling subnet 'Resnet'), models/conditional_jpeg_generator.py conv() letter I, models/networks.py's use_spectral_norm=False
 * branches.  x, y, dy, dx: NHWC [B,hw,CP] of `dtype` (WM_F32 / WM_BF16 / WM_F16), 16-byte aligned, C real channels of a stride CP that is a
 * multiple of 16 and at most 256 16-byte vectors (WM_E_SHAPE above); mean, rstd, mg, mgx: f32 [B][CP]; gamma, beta, dgamma, dbeta: f32 [C],
 * NULL together for affine=False.  act 0 none, 1 ReLU.  partial: scratch of wm_instnorm_scratch_doubles(B, hw, CP) doubles.
 * wm_instnorm_stats    : mean and rstd = 1 / sqrt(max(var, 0) + eps) of every (sample, channel) plane, biased variance; 0 in channels >= C.
 * wm_instnorm_apply    : y = act((x - mean) * rstd * gamma + beta); channels >= C are written as zeros.
 * wm_instnorm_bwd_sums : with g = dy * act'(y) (ReLU: y > 0 on the value as stored) and xhat = (x - mean) * rstd recomputed from x:
 *                        mg = mean of g, mgx = mean of g * xhat per plane; dgamma = sum over samples and pixels of g * xhat, dbeta = of g.
 * wm_instnorm_bwd_apply: dx = gamma * rstd * (g - mg - xhat * mgx); zeros in channels >= C.
 * Every sum is accumulated in double in a fixed order (no atomics): two calls give the same bits.  A plane of more than 256 pixels is
 * summed by wm_instnorm_splits(hw) workgroups (<= 64) whose partial sums a small second launch adds in order; so are dgamma / dbeta. */
int wm_instnorm_splits(size_t hw);
size_t wm_instnorm_scratch_doubles(int B, size_t hw, int CP);
int wm_instnorm_stats(const void* x, double* partial, float* mean, float* rstd, int B, size_t hw, int C, int CP, double eps, int dtype,
                      void* stream);
int wm_instnorm_apply(const void* x, const float* mean, const float* rstd, const float* gamma, const float* beta, void* y, int B, size_t hw,
                      int C, int CP, int act, int dtype, void* stream);
int wm_instnorm_bwd_sums(const void* x, const void* dy, const float* mean, const float* rstd, const float* gamma, const float* beta,
                         double* partial, float* mg, float* mgx, float* dgamma, float* dbeta, int B, size_t hw, int C, int CP, int act,
                         int dtype, void* stream);
int wm_instnorm_bwd_apply(const void* x, const void* dy, const float* mean, const float* rstd, const float* gamma, const float* beta,
                          const float* mg, const float* mgx, void* dx, int B, size_t hw, int C, int CP, int act, int dtype, void* stream);

/* ------------------------------------------------------------------ LayerNorm and Swin window attention (csrc/swin.hip)
 * replaces, in network/SUNet_detail.py: nn.LayerNorm (norm1 / norm2, :192,198) and, in one launch each way, the roll (:238,255),
 * window_partition / window_reverse (:27-56), the head split, q*scale @ k^T, the relative-position bias gather, the shifted-window mask add,
 * the softmax and attn @ v of WindowAttention.forward (:113-135).  Activations of `dtype` (WM_F32 / WM_BF16 / WM_F16) are token grids
 * [tokens][CP] = [B][H][W][CP], C real channels of a stride CP that is a multiple of 16; padding channels are written as zeros.
 * wm_layernorm_fwd : y = (x - mean) * rstd * gamma + beta over the C channels of every token, biased variance, rstd = 1 / sqrt(var + eps);
 *                    mean and var in f32 (two passes over the row); mean, rstd: f32 [tokens], kept for the backward.  gamma, beta: f32 [C].
 * wm_layernorm_bwd : dx = rstd * (dy gamma - mean_c(dy gamma) - xhat mean_c(dy gamma xhat)); dgamma = sum over tokens of dy * xhat, dbeta = of dy
 *                    (NULL together: not computed), summed in double over slices of the tokens whose partial rows a finalise launch adds in
 *                    order: no atomics, two calls give the same bits.  scratch: wm_layernorm_scratch_doubles(tokens, C) doubles.
 * wm_winattn_fwd   : qkv [B][H][W][CP3], the qkv Linear's output on the un-partitioned grid, channel = (q|k|v) * C + head * hd + d with
 *                    hd = C / nH <= 96; out [B][H][W][CPO], channel = head * hd + d.  Per window of ws x ws tokens (1 <= ws <= 8, H and W
 *                    multiples of ws) of the grid rolled by -shift (0 <= shift < ws) and per head:
 *                    out = softmax(scale * q k^T + table[rel_index] + mask) v.  table: f32 [(2 ws - 1)^2][nH]; rel_index and mask (-100 where
 *                    the two tokens' regions of the rolled grid differ, shift > 0 only) are the reference's (:86-96, :202-221), computed in
 *                    the kernel.  lse: f32 [B][nH][H][W], the row log-sum-exp, kept for the backward.
 * wm_winattn_bwd   : g_qkv [B][H][W][CP3] and g_table [(2 ws - 1)^2][nH] for the output gradient g_out [B][H][W][CPO]; the probabilities are
 *                    recomputed from qkv and lse.  g_table sums dS over samples, windows and token pairs by relative index: per-workgroup
 *                    partial tables in scratch (wm_winattn_scratch_floats floats) added in order; no atomics, two calls give the same bits.
 * bf16 / f16: both products of each direction run on MFMA with f32 accumulation; f32: FMAs.  The softmax is f32 with the row maximum
 * subtracted. */
size_t wm_layernorm_scratch_doubles(size_t tokens, int C);
int wm_layernorm_fwd(const void* x, const float* gamma, const float* beta, void* y, float* mean, float* rstd, size_t tokens, int C, int CP,
                     float eps, int dtype, void* stream);
int wm_layernorm_bwd(const void* x, const void* dy, const float* gamma, const float* mean, const float* rstd, void* dx, float* dgamma,
                     float* dbeta, double* scratch, size_t tokens, int C, int CP, int dtype, void* stream);
size_t wm_winattn_scratch_floats(int B, int H, int W, int nH, int ws);
int wm_winattn_fwd(const void* qkv, const float* table, void* out, float* lse, int B, int H, int W, int C, int nH, int ws, int shift,
                   float scale, int CP3, int CPO, int dtype, void* stream);
int wm_winattn_bwd(const void* g_out, const void* qkv, const float* table, const float* lse, void* g_qkv, float* g_table, float* scratch,
                   int B, int H, int W, int C, int nH, int ws, int shift, float scale, int CP3, int CPO, int dtype, void* stream);

/* ------------------------------------------------------------------ losses of the literal IRNrhi step
 * replaces, in models/IRNrhi_model.py:425-560: nn.SmoothL1Loss (:148,476,481), nn.BCELoss (:147,492-493,505), nn.CrossEntropyLoss
 * (:156,454,485), torch.clamp(x,0,1) with its gradient mask (:430,472), PSNR of the postprocess()ed images (:527, metrics.py:30-46).
 * Each loss call writes the mean loss to a device scalar and, when grad_out != NULL, d loss / d input for an upstream gradient of 1
 * (the host scales it by the loss weight with wm_scale_dev).  partials: f32 scratch [nparts <= 2048] (doubles for the PSNR: feed
 * them to wm_psnr_gate).  f32 only. */
int wm_smooth_l1(const float* a, const float* b, size_t n, float beta, float* partials, int nparts, float* loss_out, float* grad_out,
                 void* stream);
int wm_bce_prob(const float* p, float target, size_t n, float* partials, int nparts, float* loss_out, float* grad_out, void* stream);
int wm_cross_entropy(const float* logits, const long long* labels, int B, int K, int ld, float* loss_out, float* grad_out, void* stream);
int wm_clamp01_fwd(const float* x, float* y, size_t n, void* stream);
int wm_clamp01_bwd(const float* x, const float* g, float* gx, size_t n, void* stream);
int wm_psnr255_partials(const float* a, const float* b, size_t n, double* partials, int nparts, void* stream);

/* ------------------------------------------------------------------ device RNG and the stochastic attacks (csrc/noise.hip)
 * Philox4x32-10.  The draw for element index i is a pure function of (seed, offset, i): key = seed, counter = (i / 4, offset), word i % 4.
 * uniform = 24-bit floats in [0,1); normal = Box-Muller (u1 in (0,1], accurate logf / sincosf) on the word pairs (0,1) and (2,3).
 * state: device array of WM_RNG_STATE_WORDS int64 {seed, offset, 0, 0} owned by the caller (a layer).  Each forward call uses the counters
 * [offset, offset + reserve) (reserve = 1; 2 for wm_dropout_fwd: the keep ratio at offset, the mask at offset + 1): a one-thread launch copies
 * {seed, offset} into rec[2] (device, int64) and advances the state's offset, in stream order, then the attack kernel reads rec only; the
 * backward regenerates the same draws from rec.  Safe under hipGraph capture: every replay draws fresh numbers.
 * wm_rng_fill (test entry point): out[i] = draw i, i < n, of the stream at (state[0], state[1]) -- exactly what a kernel consumes for element
 * index i; the state is only read (a rec array is a valid state). */
#define WM_RNG_STATE_WORDS 4
#define WM_RNG_UNIFORM 0
#define WM_RNG_NORMAL 1
int wm_rng_fill(const void* state, float* out, size_t n, int dist, void* stream);
/* per-element attacks on n f32 elements (u uniform, z normal of element i):
 *   WM_NOISE_DROP  y = u > a ? cover : x            replaces noise_layers/crop.py:136-147 (Dropout, a = prob)
 *   WM_NOISE_GAUSS y = clamp(x + fma(b, z, a), 0, 1) replaces noise_layers/gaussian.py:11-17 (a = mean, b = stddev)
 *   WM_NOISE_GN    y = x + fma(b, z, a)              replaces noise_layers/gaussian_noise.py:12-20 (a = mean, b = sqrt(var))
 *   WM_NOISE_SP    y = u > b ? 0 : x, then u < a ? 1  replaces noise_layers/salt_pepper_noise.py:10-19 (a = prob/2, b = 1 - prob/2)
 * wm_noise_bwd: gx = dy/dx . g (x = the forward's input, read by WM_NOISE_GAUSS only; WM_NOISE_GN has no kernel: the identity);
 * gcover (WM_NOISE_DROP, may be NULL) = dy/dcover . g. */
#define WM_NOISE_DROP 0
#define WM_NOISE_GAUSS 1
#define WM_NOISE_GN 2
#define WM_NOISE_SP 3
int wm_noise_fwd(int op, const float* x, const float* cover, float* y, size_t n, float a, float b, void* state, void* rec, void* stream);
int wm_noise_bwd(int op, const float* x, const float* g, float* gx, float* gcover, size_t n, float a, float b, const void* rec, void* stream);
/* replaces noise_layers/dropout.py:4-27 on N = B*C planes of H x W: keep = fma(keep_span, u, keep_min) from counter block 0 at offset,
 * one mask m = [u < keep] over H x W (element h*W + w at offset + 1) shared by every plane; y = x*m + cover*(1-m);
 * backward gx = g*m, gcover (may be NULL) = g*(1-m). */
int wm_dropout_fwd(const float* x, const float* cover, float* y, int N, int H, int W, float keep_min, float keep_span, void* state, void* rec,
                   void* stream);
int wm_dropout_bwd(const float* g, float* gx, float* gcover, int N, int H, int W, float keep_min, float keep_span, const void* rec,
                   void* stream);
/* JpegCompression ("JPEG-Drop", replaces noise_layers/jpeg_compression.py:65-159) on [B,3,H,W] f32: zero pad to a multiple of 8, analog
 * rgb2yuv, unnormalised 8x8 DCT-II, zig-zag keep mask of keep[3] (host pointer: coefficients kept in Y, U, V), IDCT (scaled sqrt(1/16), -1/2
 * on DC), yuv2rgb, un-pad.  wm_jpeg_drop_bwd is its exact transpose (rgb2yuv^T DCT^T mask IDCT^T yuv2rgb^T). */
int wm_jpeg_drop_fwd(const float* x, float* y, int B, int H, int W, const int* keep, void* stream);
int wm_jpeg_drop_bwd(const float* gy, float* gx, int B, int H, int W, const int* keep, void* stream);

/* ------------------------------------------------------------------ image-quality and mask metrics (csrc/ssim.hip)
 * replaces pytorch_ssim/__init__.py:7-40 (_ssim and its autograd backward: the fidelity loss of models/IRN_model.py:569-570),
 * metrics.py:5-46 (EdgeAccuracy's sums, PSNR) and calculate_f1.py:5-41 (TN / TP / FN / FP of a thresholded mask).  f32 NCHW images
 * [B,C,H,W], any H, W >= 1, B*C <= 65535.  No atomics: per-workgroup partials and a fixed-order finalise, bitwise reproducible.
 * win11: HOST pointer to the 11 window coefficients (gauss / gauss.sum() evaluated in float32, as the reference builds them).
 * wm_ssim_fwd: one fused launch (both images' tiles with a 5-pixel halo in LDS, separable passes for x, y, x^2, y^2, xy, the map formed
 *   in registers and never written).  partials [B * wm_ssim_nparts(C,H,W)] doubles, image b's contiguous.  dplanes (may be NULL)
 *   [3][B,C,H,W] = dS/dp, dS/dq, dS/dr of every pixel (p = w*x, q = w*x^2, r = w*xy): what wm_ssim_bwd convolves.
 * wm_ssim_finalize: out[0] = mean over everything (size_average=True), out[1 + b] = mean of image b (size_average=False).
 * wm_ssim_bwd: grad (+)= g * (w*Dp + 2x . w*Dq + y . w*Dr), the gradient wrt the FIRST image x of the forward that wrote dplanes;
 *   g = gscale * gscale_dev[0] (device, may be NULL) * gout_dev[per_image ? b : 0] (device, may be NULL = 1) / (per_image ? CHW : BCHW);
 *   accumulate != 0 adds into grad.  For the second image call the forward and this with the images swapped.
 * wm_psnr_partials: partials [nparts <= 2048] doubles of sum (a - b)^2 (float images, no truncation; wm_psnr255_partials is the int form);
 * wm_psnr_finalize: out[0] = 20 log10(max_val) - 10 log10(mse), 0 when mse == 0 (metrics.py:41-42).
 * wm_confusion_counts: pred / gt masks of B images x per_image elements, f32 or (pred_u8 / gt_u8 != 0) uint8; P = pred > thr_pred,
 *   G = gt > thr_gt; partials [B * wm_confusion_nparts(per_image) * 4] int64 scratch; out [(1 + B) * 4] int64 = {TN, TP, FN, FP} in total,
 *   then of each image (TN: !P !G, TP: P G, FN: !P G, FP: P !G). */
int wm_ssim_nparts(int C, int H, int W);
int wm_ssim_fwd(const float* x, const float* y, int B, int C, int H, int W, const float* win11, double* partials, float* dplanes,
                void* stream);
int wm_ssim_finalize(const double* partials, int B, int C, int H, int W, float* out, void* stream);
int wm_ssim_bwd(const float* dplanes, const float* x, const float* y, float* grad, int B, int C, int H, int W, const float* win11,
                const float* gout_dev, int per_image, float gscale, const float* gscale_dev, int accumulate, void* stream);
int wm_psnr_partials(const float* a, const float* b, size_t n, double* partials, int nparts, void* stream);
int wm_psnr_finalize(const double* partials, int nparts, double n, float max_val, float* out, void* stream);
int wm_confusion_nparts(size_t per_image);
int wm_confusion_counts(const void* pred, int pred_u8, const void* gt, int gt_u8, float thr_pred, float thr_gt, int B, size_t per_image,
                        long long* partials, long long* out, void* stream);

/* ------------------------------------------------------------------ Dice (overlap) loss (csrc/dice.hip)
 * replaces dice_loss.py:44-61 (BinaryDiceLoss.forward: the mask-head loss tianchi_model.py:48,101 constructs), :81-96 (DiceLoss.forward: softmax
 * over the classes, the class loop with ignore_index and weight, / C) and the autograd backward of both.  Everything f32; no atomics, no
 * host synchronisation: double partials per workgroup and a fixed-order finalise, bitwise reproducible.  B <= 65535.
 * pw (the reference's p): 1 and 2 take paths without powf, any other positive value goes through powf.
 * reduction: WM_DICE_MEAN / WM_DICE_SUM (one device scalar) / WM_DICE_NONE ([B]).
 * wm_dice_sums: p, target [B, per_sample] (any per_sample: 16-byte loads with a scalar head and tail) ->
 *   partials [B * wm_dice_nparts(per_sample) * 3] doubles, sample b's contiguous: {sum p*t, sum p^pw, sum t^pw} per workgroup.
 * wm_dice_softmax_sums: logits, target [B,C,HW] (NCHW planes, C <= 32, WM_E_BADARG above); s = softmax over the C planes, formed per pixel
 *   and never written -> partials [B*C * wm_dice_nparts(HW) * 3] doubles, unit (b, c)'s contiguous: the same three sums of (s_c, t_c).
 * wm_dice_finalize: C = 1 (with ignore_index < 0, weight NULL) for wm_dice_sums' partials.  coef [B*C][2] doubles = {num = sum p*t + smooth,
 *   den = sum p^pw + sum t^pw + smooth} per unit (what the backward reads); loss_b = sum_c w_c (1 - num/den) / C with
 *   w_c = (c == ignore_index ? 0 : weight ? weight[c] (device, [C]) : 1) -- the division is by C even when a class is ignored, as :96 --;
 *   loss_out = [B] (none), or one scalar: sum_b loss_b (sum), that / B (mean).
 * wm_dice_bwd: grad (+)= g * (num * pw * p^(pw-1) - t * den) / den^2, g = gscale * gscale_dev[0] (device, may be NULL) *
 *   gout_dev[none ? b : 0] (device, may be NULL = 1) / (mean ? B : 1); chain_sigmoid != 0: p is a sigmoid output s(z) (the UNet head) and the
 *   gradient is taken wrt z (multiplied by p*(1-p)), as wm_bce_logits_target does; accumulate != 0 adds into grad.
 * wm_dice_softmax_bwd: grad (+)= d loss / d logits: dz_c = s_c * (g_c - sum_k g_k s_k), g_c = g * w_c / C * (the binary derivative of unit
 *   (b, c) at s_c); the softmax is recomputed per pixel.  Same g, ignore_index and weight as the finalise call. */
#define WM_DICE_MEAN 0
#define WM_DICE_SUM 1
#define WM_DICE_NONE 2
int wm_dice_nparts(size_t per_sample);
int wm_dice_sums(const float* p, const float* target, int B, size_t per_sample, float pw, double* partials, void* stream);
int wm_dice_softmax_sums(const float* logits, const float* target, int B, int C, size_t HW, float pw, double* partials, void* stream);
int wm_dice_finalize(const double* partials, int B, int C, size_t per_sample, double smooth, int reduction, int ignore_index,
                     const float* weight, double* coef, float* loss_out, void* stream);
int wm_dice_bwd(const float* p, const float* target, const double* coef, float* grad, int B, size_t per_sample, float pw, int reduction,
                const float* gout_dev, float gscale, const float* gscale_dev, int chain_sigmoid, int accumulate, void* stream);
int wm_dice_softmax_bwd(const float* logits, const float* target, const double* coef, float* grad, int B, int C, size_t HW, float pw,
                        int reduction, int ignore_index, const float* weight, const float* gout_dev, float gscale, const float* gscale_dev,
                        int accumulate, void* stream);

/* ------------------------------------------------------------------ pixel- and gradient-domain image losses (csrc/imgloss.hip)
 * replaces models/modules/loss.py:5-22 (ReconstructionLoss), loss.py:413-423 (GradientLoss), loss.py:309-360 (ExclusionLoss) and the autograd
 * backward of each.  f32 NCHW contiguous tensors; no atomics, no host synchronisation: double partials per workgroup and a fixed-order
 * one-workgroup finalise, bitwise reproducible.  Every loss is one device scalar.  In every backward g = gscale * gscale_dev[0] (device, may
 * be NULL) * gout_dev[0] (device, may be NULL = 1) and accumulate != 0 adds into the gradient buffer.
 * wm_recon_sums: x, target [B, per_sample] (any per_sample: 16-byte loads with a scalar head and tail) -> partials [B * wm_recon_nparts(per_sample)]
 *   doubles of sum f(x - t): f = d^2 (WM_RECON_L2), sqrt(d^2 + eps) (WM_RECON_LCHAR), d (WM_RECON_L1: the reference's signed sum, no abs).
 * wm_recon_finalize: loss_out[0] = sum of the partials / B.
 * wm_recon_bwd: grad (+)= g / B * f'(x - t); a negative gscale gives the gradient wrt the target.
 * wm_gradloss_sums: a = N = B*C planes [H, W], H, W >= 2 -> partials [N * wm_gradloss_nparts(H, W) * 2] doubles {sum |a[y][x] - a[y][x+1]|,
 *   sum |a[y][x] - a[y+1][x]|};  wm_gradloss_finalize: loss_out[0] = sum_x / (N H (W-1)) + sum_y / (N (H-1) W);
 *   wm_gradloss_bwd: gather form, the subgradient of |.| at 0 is 0.
 * wm_excl_fwd: img1 [B,C1,H,W], img2 [B,C2,H,W], 1 <= C1, C2 <= 4, 1 <= levels <= 3, H and W >= 2 << (levels - 1) (WM_E_BADARG otherwise: the
 *   reference would take the mean of an empty tensor).  Level l is the image 2 x 2 average-pooled l times (floor); per level, direction
 *   (0 = gradx, rows: img[y+1] - img[y]; 1 = grady, columns) and channel pair, s = 2 sigmoid(diff) - 1 and the sum of s1^2 s2^2 ->
 *   partials [levels*2*C1*C2][wm_excl_nparts(B, H, W)] doubles.  Both images are read once (16 x 32 tiles with a 4-pixel halo, pooled in LDS).
 * wm_excl_finalize: means [levels][2][C1*C2] doubles (term k = i2*C1 + i1 pairs img1's channel i1 with img2's i2: the reference's list order),
 *   loss_out[0] = sum means^0.25 / (levels * 9) / 2 (9 whatever C1*C2 is, as the reference), coef [levels][2][C1*C2] doubles =
 *   d loss / d (one product of that term) -- 0 for a term whose mean is 0: it contributes no gradient (the reference: NaN).
 * wm_excl_bwd: gather form, one launch; grad1 / grad2 (either may be NULL) (+)= g * d loss / d img1, img2. */
#define WM_RECON_L2 0
#define WM_RECON_LCHAR 1
#define WM_RECON_L1 2
int wm_recon_nparts(size_t per_sample);
int wm_recon_sums(const float* x, const float* target, int B, size_t per_sample, int kind, float eps, double* partials, void* stream);
int wm_recon_finalize(const double* partials, int B, size_t per_sample, float* loss_out, void* stream);
int wm_recon_bwd(const float* x, const float* target, float* grad, int B, size_t per_sample, int kind, float eps, const float* gout_dev,
                 float gscale, const float* gscale_dev, int accumulate, void* stream);
int wm_gradloss_nparts(int H, int W);
int wm_gradloss_sums(const float* a, int N, int H, int W, double* partials, void* stream);
int wm_gradloss_finalize(const double* partials, int N, int H, int W, float* loss_out, void* stream);
int wm_gradloss_bwd(const float* a, float* grad, int N, int H, int W, const float* gout_dev, float gscale, const float* gscale_dev,
                    int accumulate, void* stream);
int wm_excl_nparts(int B, int H, int W);
int wm_excl_fwd(const float* img1, const float* img2, int B, int C1, int C2, int H, int W, int levels, double* partials, void* stream);
int wm_excl_finalize(const double* partials, int B, int C1, int C2, int H, int W, int levels, double* means, double* coef, float* loss_out,
                     void* stream);
int wm_excl_bwd(const float* img1, const float* img2, const double* coef, float* grad1, float* grad2, int B, int C1, int C2, int H, int W,
                int levels, const float* gout_dev, float gscale, const float* gscale_dev, int accumulate, void* stream);

/* ------------------------------------------------------------------ local structure loss, mask and gray losses (csrc/ssim3.hip)
 * replaces loss.py:9-39 = models/modules/loss.py:44-74 (SSIM_Loss: a per-pixel MAP), loss.py:363-376 (ExtendedL1Loss), :379-388
 * (NonBlurryLoss), :403-410 (GrayLoss) and the autograd backward of each.  f32 contiguous tensors; no atomics, no host synchronisation: double
 * partials per workgroup and a fixed-order one-workgroup finalise, bitwise reproducible.  In every backward the scalar weight is
 * s = gscale * gscale_dev[0] (device, may be NULL) * gout_dev[0] (device, may be NULL = 1) and accumulate != 0 adds into the gradient buffers.
 * wm_ssim3_fwd: x, y = N = B*C planes [H, W], H, W >= 2, N <= 65535 (WM_E_BADARG otherwise: ReflectionPad2d(1) needs two pixels).  Both are
 *   padded by 1 with reflection (index -1 -> 1, H -> H-2); nine-tap means mu_x, mu_y, E[x^2], E[y^2], E[xy] (row by row, / 9);
 *   n = (2 mu_x mu_y + C1)(2 (E[xy] - mu_x mu_y) + C2), d = (mu_x^2 + mu_y^2 + C1)(E[x^2] - mu_x^2 + E[y^2] - mu_y^2 + C2), C1 = 0.01^2,
 *   C2 = 0.03^2; out_map (may be NULL) [N,H,W] = clamp((1 - n/d) / 2, 0, 1); partials (may be NULL) [wm_ssim3_nparts(N,H,W)] doubles = the
 *   sum of the map over each 16 x 64 tile.  One launch: 8 B read, 4 B written per element.  x == y gives exactly 0.
 * wm_ssim3_finalize: loss_out[0] = sum of the partials / (N H W) = mean(map).
 * wm_ssim3_bwd: gather form, one launch; gx / gy (either may be NULL) (+)= d/dx, d/dy of sum(g * map) * s with g [N,H,W] the upstream map, or
 *   with g == NULL of mean(map) * s (every pixel's weight is (float)s * (1.f / (float)(N H W)): a g filled with that value gives the same
 *   bits).  The clamp passes the gradient where 0 <= (1 - n/d)/2 <= 1, bounds included, as torch.clamp; the reflection's adjoint is exact (a
 *   border pixel is counted once per tap that maps to it, also at H = 2 or W = 2).
 * wm_pixloss_sums: a (and with WM_PIXLOSS_MASKL1 b, mask) [n] (any n and alignment: 16-byte access with a scalar head and tail) ->
 *   partials [wm_pixloss_nparts(n) * 2] doubles: MASKL1 {sum |mask*a - mask*b|, sum |mask|} (the products exact in double, the difference rounded
 *   once), NONBLURRY {sum (a - 1/2)^2, 0}, GRAY {sum |a - 1/2|, 0}; b and mask are ignored for the last two.
 * wm_pixloss_finalize: coef [2] doubles = the two sums / n (what the backward reads); loss_out[0] = coef0 / coef1 (MASKL1; a zero mask gives
 *   0/0 = NaN as the reference, unguarded), 1 - coef0 (NONBLURRY), 1 / coef0 (GRAY).
 * wm_pixloss_bwd: MASKL1: ga / gb (either may be NULL) (+)= +- s sign(mask*a - mask*b) mask / (n coef1), sign(0) = 0 as torch's L1Loss; no
 *   gradient goes to the mask.  NONBLURRY: ga (+)= -2 s (a - 1/2) / n.  GRAY: ga (+)= -s sign(a - 1/2) / (n coef0^2).  gb must be NULL for
 *   the last two. */
#define WM_PIXLOSS_MASKL1 0
#define WM_PIXLOSS_NONBLURRY 1
#define WM_PIXLOSS_GRAY 2
int wm_ssim3_nparts(int N, int H, int W);
int wm_ssim3_fwd(const float* x, const float* y, float* out_map, double* partials, int N, int H, int W, void* stream);
int wm_ssim3_finalize(const double* partials, int N, int H, int W, float* loss_out, void* stream);
int wm_ssim3_bwd(const float* x, const float* y, const float* g, float* gx, float* gy, int N, int H, int W, const float* gout_dev,
                 float gscale, const float* gscale_dev, int accumulate, void* stream);
int wm_pixloss_nparts(size_t n);
int wm_pixloss_sums(int kind, const float* a, const float* b, const float* mask, size_t n, double* partials, void* stream);
int wm_pixloss_finalize(int kind, const double* partials, size_t n, double* coef, float* loss_out, void* stream);
int wm_pixloss_bwd(int kind, const float* a, const float* b, const float* mask, const double* coef, float* ga, float* gb, size_t n,
                   const float* gout_dev, float gscale, const float* gscale_dev, int accumulate, void* stream);

/* ------------------------------------------------------------------ GAN objectives (csrc/advloss.hip)
 * The reference's AdversarialLoss (loss.py:41-88), GANLoss and CWLoss (models/modules/loss.py:24-42, 77-109).  f32 contiguous tensors; no
 * atomics, no host synchronisation: one streaming launch writes double partials per workgroup and, when asked, the gradient; a fixed-order
 * one-workgroup finalise makes the device scalar.  Bitwise reproducible.  g = gscale * gscale_dev[0] (device, may be NULL) * gout_dev[0]
 * (device, may be NULL = 1); accumulate != 0 adds into the gradient buffer.  Elements are evaluated in double and rounded once.
 * wm_advloss_elem: x [n] (any n and alignment: 16-byte access with a scalar head and tail) -> partials [wm_advloss_nparts of n] doubles of
 *   sum f(x_i, t_i), and with grad != NULL grad (+)= g / n * df/dx.  objective:
 *     WM_ADV_BCE_PROB    -(t max(log x, -100) + (1 - t) max(log(1 - x), -100)), df/dx = (x - t) / max(x (1 - x), 1e-12): nn.BCELoss.
 *                        x outside [0, 1] gives NaN
 *     WM_ADV_BCE_LOGITS  (1 - t) x + max(-x, 0) + log(1 + exp(-|x|)): nn.BCEWithLogitsLoss, any label value
 *     WM_ADV_MSE         (x - t)^2
 *     WM_ADV_HINGE_DISC  relu(1 + s x) with the sign s passed in `label`: -1 (real) or +1 (fake); the subgradient at 0 is 0
 *     WM_ADV_NEG_MEAN    -x;   WM_ADV_POS_MEAN  x   (label unused)
 *   t = label when mask == NULL.  mask != NULL (the three objectives with a label): x is [B,C,H,W] with B*C*H*W == n, mask [B,Cm,Hm,Wm] with
 *   Cm 1 or C, and t = real_label * (1 - m) with m the bilinear sample of the mask at the element's pixel (align_corners = False, no
 *   antialiasing), taken inside the kernel; B, C, H, W, Cm, Hm, Wm, real_label are ignored otherwise.  No gradient goes to the mask.
 * wm_advloss_finalize: loss_out[0] = sum of the partials / n.
 * wm_cw_margin: logits [B,K] (K >= 2), target [B] int64 -> loss_out[0] = sum_b max(other_b - real_b, kappa) (is_targeted != 0) or
 *   max(real_b - other_b, kappa), real = logits[b][target_b], other = max_j of (1 - onehot) logits - onehot * 10000 (the target's slot holds
 *   -10000).  Two launches; terms = scratch [B] doubles.  grad (may be NULL) [B,K] (+)= g * d loss / d logits: -+w at the target column and
 *   +-w at the lowest column attaining `other` (none when that is the target's own slot), w = 1 where the margin exceeds kappa, 1/2 at a tie,
 *   0 where kappa wins.  A target outside [0, K) is never used as an index: that row's term and gradient row are NaN, so loss_out is NaN. */
#define WM_ADV_BCE_PROB 0
#define WM_ADV_BCE_LOGITS 1
#define WM_ADV_MSE 2
#define WM_ADV_HINGE_DISC 3
#define WM_ADV_NEG_MEAN 4
#define WM_ADV_POS_MEAN 5
int wm_advloss_nparts(size_t n);
int wm_advloss_elem(int objective, const float* x, size_t n, float label, const float* mask, int B, int C, int H, int W, int Cm, int Hm, int Wm,
                    float real_label, double* partials, float* grad, const float* gout_dev, float gscale, const float* gscale_dev,
                    int accumulate, void* stream);
int wm_advloss_finalize(const double* partials, size_t n, float* loss_out, void* stream);
int wm_cw_margin(const float* logits, const long long* target, int B, int K, int is_targeted, float kappa, double* terms, float* loss_out,
                 float* grad, const float* gout_dev, float gscale, const float* gscale_dev, int accumulate, void* stream);

/* ------------------------------------------------------------------ hybrid per-frame attack mix (csrc/hybrid.hip)
 * The "HYBRID ATTACKS" block of the reference's video model (models/IRNcrop_model.py:347-373): alpha = softmax(randn(B, T, K), dim = 2), the
 * localiser's input = sum_k alpha[..., k] * attacked_k per frame, then clamp_with_grad + Quantization (:372-373).  (The reference's loop body
 * :369 adds the bare weights and never multiplies them in; this is the mix it means.)  f32 contiguous tensors [N][frame], N = B*T frames, any
 * frame >= 1 (not only multiples of 4); w [N][K] f32 on the device, used as given (not required to sum to 1); 1 <= K <= 8.
 * wm_mix_fwd: xs_host = HOST array of K device pointers, passed to the kernel by value.  acc = 0; for k = 0..K-1: acc = fma(w[n][k], x_k[i], acc),
 *   in that order; quant 0: y = acc; quant 1: y = exactly wm_clamp_quant_fwd of acc (the same device function).  One launch, (K+1) * 4 bytes
 *   per element.  K outside 1..8, a null pointer, N <= 0 or frame == 0: WM_E_BADARG and nothing is launched.
 * wm_mix_bwd: gxs_host = HOST array of K device pointers; gx_k[i] = w[n][k] * g[i]; a NULL entry = that input needs no gradient: nothing is
 *   stored for it (all NULL: WM_OK, nothing is launched).  The clamp and the quantisation are identities backwards, so there is no quant here.
 * 16-byte accesses when every tensor pointer is 16-byte aligned, 4-byte accesses otherwise. */
int wm_mix_fwd(const float* const* xs_host, int K, const float* w, float* y, int N, size_t frame, int quant, void* stream);
int wm_mix_bwd(const float* g, const float* w, float* const* gxs_host, int K, int N, size_t frame, void* stream);

/* ------------------------------------------------------------------ two-source mask head (csrc/mask_head.hip)
 * The full-resolution tail of the tamper localiser UNetDiscriminator (the reference's models/networks.py:1005-1013,1100-1110): decoder_0 =
 * nn.Conv2d(na + nb, Cout, 1) on torch.cat((a, b), 1), optionally the sigmoid, as NCHW f32 -- in one pass that reads both sources in place:
 *   out[b,co,p] = act(bias[co] + sum_c w[co,c] a[b,p,c] + sum_c w[co,na+c] b[b,p,c])
 * a [B*hw][lda], b [B*hw][ldb]: NHWC activations of `dtype`, na <= lda and nb <= ldb real channels, the padding channels ignored whatever they
 * hold; lda and ldb multiples of the 16-byte vector (4 f32 / 8 16-bit values) and at most 16 vectors, 16-byte aligned bases (WM_E_SHAPE
 * otherwise).  w f32 [Cout][na+nb] (torch's decoder_0.0.weight), bias f32 [Cout] (NULL = 0), 1 <= Cout <= 4, accumulated in f32; out f32
 * [B][Cout][hw]; act 0 = none, 1 = sigmoid.  (na + nb) * sizeof(dtype) + 4 Cout bytes per pixel, nothing else.
 * wm_head2_bwd: gout f32 [B][Cout][hw]; chain_sigmoid != 0: gout is the gradient wrt the sigmoid OUTPUT and is multiplied by out (1 - out) of
 *   the saved forward result `out`; 0: gout is the gradient wrt the logits (out may be NULL).  Writes ga [B*hw][ldga = lda], gb [B*hw][ldgb =
 *   ldb] of `dtype` (padding channels exactly 0) and partials [wm_head2_nparts(B*hw)][Cout*(na+nb) + Cout] doubles: each workgroup's sums of
 *   gz x (a | b) and of gz.
 * wm_head2_finalize: dw [Cout][nab = na+nb], dbias [Cout] (+)= the partials added in double in a fixed order, rounded to f32 once (accumulate
 *   != 0: the old value joins that sum before the rounding).  No floating-point atomics: every result is bitwise reproducible.
 * The caller owns every buffer; the calls are asynchronous on `stream`. */
int wm_head2_fwd(const void* a, int lda, int na, const void* b, int ldb, int nb, const float* w, const float* bias, float* out, int B, size_t hw,
                 int Cout, int act, int dtype, void* stream);
int wm_head2_nparts(size_t npix);
int wm_head2_bwd(const void* a, int lda, int na, const void* b, int ldb, int nb, const float* w, const float* gout, const float* out,
                 int chain_sigmoid, void* ga, int ldga, void* gb, int ldgb, double* partials, int B, size_t hw, int Cout, int dtype, void* stream);
int wm_head2_finalize(const double* partials, int nparts, int Cout, int nab, float* dw, float* dbias, int accumulate, void* stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* WM_HIP_H */
