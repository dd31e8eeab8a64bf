// What the MFMA kernels share (conv3x3_ws.hip, bwd_ws.hip, bwd_ws8.hip, bwd_ws16.hip, wgrad_ws.hip, conv3x3_stream.hip, upconv_mfma.hip,
// concat_side.hip): the 16-bit-twin preamble, the small register vector types, the transposing fragment read and the LDS swizzles.
// The swizzles are DEFINED here, once: several kernels read an LDS tile that another kernel's scheme laid out (the one-pass backward
// reads its dy halo both as conv3x3_ws.hip's pixel fragments and as wgrad_ws.hip's transposed ones), so a layout has one definition.
#pragma once
#include "wm_common.h"

// ---- the twin preamble.  A file that includes this header is compiled twice (build.py TWICE): plain for bf16 (production), and with
// -DWM_H16_F16 for the f16 twin of every kernel in it (the reference's autocast dtype, BASELINE config C5).  Everything that depends on
// the 16-bit layout goes through h16<> (wm_common.h); WM_HSYM(name) is the twin's exported symbol.
#ifdef WM_H16_F16
typedef f16_t hx_t;
#define WM_HSYM(name) name##_f16
#else
typedef bf16_t hx_t;
#define WM_HSYM(name) name##_bf16
#endif
typedef h16<hx_t> HX;
typedef HX::x8 hx8;
typedef HX::x2 hx2;

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef short i16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

// ---- one MFMA operand fragment (8 values of K) through two transposing reads (ds_read_b64_tr_b16): p0, p1 are the lane's addresses in
// the two 4-pixel groups of its K range (pixels {c..c+3} and {c+8..c+11} in the weight-gradient kernels)
static __device__ __forceinline__ hx8 tr_frag(const char* p0, const char* p1) {
    typedef short s4 __attribute__((ext_vector_type(4)));
    const s4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s4*)(p0));
    const s4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s4*)(p1));
    typedef short s8 __attribute__((ext_vector_type(8)));
    s8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(hx8, v);
}

// ---- LDS swizzles of 128-byte rows (64 channels of 16 bits = eight 16-byte slots).
// swz128(row, slot): the slot index XORed with (row >> 1) & 7.  Guarantee: 16 consecutive rows hit 16 distinct 16-byte bank slots, for
// ds_read_b128 (lane = row, every lane the same logical slot) and for the ds_write_b128 that fills the rows.  Keyed on the filter row
// (conv3x3_ws.hip, bwd_ws.hip, bwd_ws8.hip, bwd_ws16.hip: the resident filter; upconv_mfma.hip: both operand tiles) or on the halo
// COLUMN of a pixel (conv3x3_ws.hip's swz_px: the key does not depend on the halo row).
constexpr __host__ __device__ __forceinline__ int swz128(int row, int slot) { return slot ^ ((row >> 1) & 7); }
// swz16(col): a BYTE-offset XOR, bit 1 of the pixel column -> bit 5, bit 3 -> bit 6.  Guarantee: the 8 pixels x 32 B one half-wave of a
// transposing read touches ({c..c+3} and {c+8..c+11}, any tap shift) fill a 256-byte bank row exactly once.  wgrad_ws.hip (x halo of
// CI = 64, dy tile), upconv_mfma.hip's weight gradient (both operand tiles), the a tile of bwd_ws.hip / bwd_ws8.hip.
constexpr __host__ __device__ __forceinline__ int swz16(int col) { return (((col >> 1) & 1) << 5) | (((col >> 3) & 1) << 6); }
// fsw(px): the slot XOR of a tile that is read BOTH ways -- the dy halo of bwd_ws.hip, bwd_ws8.hip and bwd_ws16.hip, read by the input
// gradient's ds_read_b128 (16 consecutive pixels, one 16-byte slot each) and by the weight gradient's transposing ds_read_b64_tr_b16
// (pixels {c..c+3, c+8..c+11}, 32 bytes each).  fsw(px) = bit2(px) | bit1(px) << 1 | bit3(px) << 2 -- a bit permutation of
// (px >> 1) & 7, so 16 consecutive pixels hit 16 distinct slots, and its upper two bits are swz16, so the transposing reads fill a
// bank row exactly once.
constexpr __host__ __device__ __forceinline__ int fsw(int px) { return ((px >> 2) & 1) | (((px >> 1) & 1) << 1) | (((px >> 3) & 1) << 2); }
constexpr bool wm_fsw_upper_bits_are_swz16() {
    for (int px = 0; px < 16; ++px)
        if (((fsw(px) >> 1) << 5) != swz16(px)) return false;   // slot bits 1-2 = byte-offset bits 5-6
    return true;
}
static_assert(wm_fsw_upper_bits_are_swz16(), "fsw's upper two slot bits must be swz16's byte-offset bits (the transposing reads of the dy halo rely on it)");

// ---- host side: ceil(2^32 / d) (0 for d = 1), the reciprocal with which a kernel divides a tile index by d as one mulhi -- exact while
// index * d < 2^32, and 3 scalar instructions instead of ~40
static inline unsigned wm_magic_u32(int d) { return d == 1 ? 0u : (unsigned)(((1ull << 32) + (unsigned)d - 1) / (unsigned)d); }
