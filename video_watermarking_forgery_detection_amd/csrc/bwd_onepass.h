// What the two one-pass backward kernels of a 64 -> 64 ConvBNRelu body layer share: bwd_ws.hip (four waves, every wave all roles; any
// shape) and bwd_ws8.hip (the two GEMMs on different waves; whole-tile shapes).  bwd_ws.hip's header says what they compute.  Defined
// here, once: the tile constants, the argument struct, the LDS carve-up and the launchers' argument fill.  (The swizzles of the dy halo
// and of the a tile are wm_mfma.h's fsw and swz16.)
//
// NOT here, although both kernels hold the same text: the constant-table build, the filter's permuted commit, the tile decode, the
// epilogue's mask / pack / sum loop and the final partial-row reduction.  Each was tried as a __forceinline__ function of this header;
// each changed the instruction stream of bwd_ws_kernel (register allocation and schedule of a kernel that runs at its 512-register
// limit), and these kernels change only when the compiler's output provably does not.  Whoever changes one copy changes the other.
#pragma once
#include "wm_mfma.h"

namespace {

constexpr int TH = 8, TW = 16, HH = 10, HW = 18, NPX = HH * HW, C = 64;
constexpr int SW_BYTES = 9 * C * C * 2, SDY_BYTES = NPX * 128, SA_BYTES = TH * TW * 128, BUF_BYTES = SDY_BYTES + SA_BYTES;
constexpr int XV = (NPX * 8 + 255) / 256;        // dy halo vectors per staging thread (6; the last one partially live)
constexpr int AV = TH * TW * 8 / 256;            // a-tile vectors per staging thread (4)
constexpr int GV_MAXB = 24;                      // GVEC: samples whose k3g rows fit the LDS left over (24 x 256 B)

// The fields both kernels read, then each kernel's own tail.  (A kernel's scalar registers follow the order of its arguments: one struct
// with tq, trem for both, or the two appended to BwdArgs, renumbers the SGPRs of one kernel or the other.  The head ends on an 8-byte
// boundary -- `reverse` opens the tails -- so the derived structs have exactly the layout of one flat struct.)
struct BwdHead {
    const hx_t* g; const hx_t* y;                          // layer L: gradient wrt its ReLU output, its raw conv output [B,H,W,64]
    const float* gvec; int gv_ld;                          // GVEC: the gradient is one row per sample [B][gv_ld] (a globally pooled layer); g unused
    const float* stats4; int st_ld; const float* coef;     // [scale | shift | mean | invstd][st_ld], wm_bn_bwd_finalize's coef [3][st_ld]
    const hx_t* wpt;                                       // [9][64][64] filter packed for the input gradient (rows = input channels)
    const hx_t* xr; const float* in_scale; const float* in_shift;   // layer L-1: raw conv output, its BatchNorm scale / shift
    hx_t* dx;                                              // [B,H,W,64]
    float* stat;                                           // [gridDim.x][2][64]
    float* ws;                                             // [gridDim.x][9][64][64]
    int B, H, W, tilesX, tilesY, ntiles;
};
static_assert(sizeof(BwdHead) == 0x88, "no padding between the head and the tails");
// mX, mY, m2X: ceil(2^32 / d) of tilesX, tilesY, 2 tilesX (0 for d = 1): tile index / d = mulhi
struct BwdArgs : BwdHead { int reverse; unsigned mX, mY, m2X; };                      // bwd_ws.hip
struct Bwd8Args : BwdHead { int reverse, tq, trem; unsigned mX, mY, m2X; };       // bwd_ws8.hip; tq, trem: ntiles / gridDim.x, ntiles % gridDim.x

// ---- LDS carve-up (byte offsets): filter 73,728 B | 2 x (dy halo 10x18 px 23,040 B + a tile 8x16 px 16,384 B) | sRed: the four D waves'
// partial rows | sTab: in_scale | in_shift of the feeding layer (the epilogue's mask) | sK: per channel 8 floats -- scale, shift, ca,
// k2, k3 (wm_bn_fold) of layer L; in_scale, in_shift of layer L-1; 0 --, each 8-channel block shifted by 16 B (the + 32) | GVEC: sG
// [B][64] k3 + ca * gvec[b][c]
constexpr int LDS_BUF = SW_BYTES, LDS_RED = LDS_BUF + 2 * BUF_BYTES, LDS_TAB = LDS_RED + 4 * 2 * C * 4, LDS_K = LDS_TAB + 2 * C * 4;
constexpr int LDS_G = LDS_K + (C * 8 + 32) * 4;
template <bool GVEC> constexpr int LDS_BYTES = LDS_G + (GVEC ? GV_MAXB * C * 4 : 0);

// ---- host: the launchers' argument fill
template <typename Args>   // BwdArgs or Bwd8Args (whose tq, trem its launcher sets)
inline void onepass_fill_args(Args& a, const void* g, const void* y, const float* stats4, int st_ld, const float* coef, const void* wpt, const void* xr,
                              const float* in_scale, const float* in_shift, void* dx, float* stat, float* ws, int B, int H, int W, int reverse,
                              const float* gvec, int gv_ld) {
    a.g = (const hx_t*)g; a.y = (const hx_t*)y; a.stats4 = stats4; a.st_ld = st_ld; a.coef = coef; a.wpt = (const hx_t*)wpt;
    a.gvec = gvec; a.gv_ld = gv_ld;
    a.xr = (const hx_t*)xr; a.in_scale = in_scale; a.in_shift = in_shift; a.dx = (hx_t*)dx; a.stat = stat; a.ws = ws;
    a.B = B; a.H = H; a.W = W; a.tilesX = wm_cdiv(W, TW); a.tilesY = wm_cdiv(H, TH); a.ntiles = B * a.tilesX * a.tilesY;
    a.mX = wm_magic_u32(a.tilesX); a.mY = wm_magic_u32(a.tilesY); a.m2X = wm_magic_u32(2 * a.tilesX);
    a.reverse = reverse ? 1 : 0;
}

}  // namespace
