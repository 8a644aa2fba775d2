// gfx950 device helpers of the MXFP6 kernels (mxfp6.hip) and of bin/cvtprobe:
// one 32-element block <-> its 24 bytes of e2m3 codes, bit-exact with
// core/mxfp6.h, around v_cvt_scalef32_pk32_fp6_bf16 / _pk32_bf16_fp6.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace dissem {
namespace kern {

typedef __bf16 mxfp6_bf16x32_t __attribute__((ext_vector_type(32)));
typedef unsigned int mxfp6_u32x16_t __attribute__((ext_vector_type(16)));
typedef unsigned int mxfp6_u32x6_t __attribute__((ext_vector_type(6)));
typedef unsigned int mxfp6_u32x4_t __attribute__((ext_vector_type(4)));

constexpr uint32_t kMxfp6NanScale = 0xFFu, kMxfp6NanPair = 0x7FC07FC0u;

// E of a block's scale from the bf16 bits of its finite amax: core/mxfp6.h scale_exp.
__device__ __forceinline__ int mxfp6_scale_exp(uint32_t amax_bf16) {
  if (amax_bf16 == 0) return 0;
  const int ef = int(amax_bf16 >> 7);
  if (ef == 0) return -126;
  const int e = ef - 127 - 2 + ((amax_bf16 & 0x7Fu) > 0x70u ? 1 : 0);
  return e < -126 ? -126 : e > 125 ? 125 : e;
}

// The converters as the hardware gives them. 32 bf16 (element 2k in the low
// half of dword k) and the scale 2^E -> 32 codes, element i at bits [6i, 6i + 6)
// of the 6 dwords read as one little-endian integer; and back with the scale
// as an f32 whose exponent field is the E8M0 byte. Measured on MI355X against
// integer code (bin/cvtprobe; the findings are listed in mxfp6.hip): they equal
// core/mxfp6.h for every finite input, +-inf and every scale byte 0..254; a NaN
// input saturates to +-7.5 and scale byte 0xFF gives NaNs other than 0x7FC0,
// the two cases mxfp6_pack_block and mxfp6_unpack_block handle in plain code.
__device__ __forceinline__ mxfp6_u32x6_t mxfp6_cvt_pack_raw(const mxfp6_u32x16_t& x, float scale) {
  return __builtin_amdgcn_cvt_scalef32_pk32_fp6_bf16(__builtin_bit_cast(mxfp6_bf16x32_t, x), scale);
}
__device__ __forceinline__ mxfp6_u32x16_t mxfp6_cvt_unpack_raw(const mxfp6_u32x6_t& c, float scale) {
  return __builtin_bit_cast(mxfp6_u32x16_t, __builtin_amdgcn_cvt_scalef32_pk32_bf16_fp6(c, scale));
}

// One block as the format defines it: the block's finite amax and its NaN flag
// from the bf16 bits (the bits of |x| order like the values), the scale from
// the integer rule, the codes from the converter. *scale_byte receives the E8M0
// byte (0xFF and 24 zero bytes for a block that holds a NaN).
__device__ __forceinline__ mxfp6_u32x6_t mxfp6_pack_block(const mxfp6_u32x16_t& x, uint32_t* scale_byte) {
  uint32_t amax = 0, nanacc = 0;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const uint32_t a = x[i] & 0x7FFF7FFFu;
    const uint32_t lo = a & 0xFFFFu, hi = a >> 16;
    amax = max(amax, lo < 0x7F80u ? lo : 0u);
    amax = max(amax, hi < 0x7F80u ? hi : 0u);
    nanacc |= a + 0x007F007Fu;  // bit 15 of a half: |x| > 0x7F80, a NaN
  }
  const bool nan = (nanacc & 0x80008000u) != 0;
  const int e = mxfp6_scale_exp(amax);
  const mxfp6_u32x6_t c = mxfp6_cvt_pack_raw(x, __uint_as_float(uint32_t(e + 127) << 23));
  *scale_byte = nan ? kMxfp6NanScale : uint32_t(e + 127);
  return nan ? mxfp6_u32x6_t{0, 0, 0, 0, 0, 0} : c;
}

// 24 bytes of codes with scale byte sb -> 32 bf16. Scale byte 0xFF marks a NaN
// block: its result is a constant, selected instead of converted.
__device__ __forceinline__ mxfp6_u32x16_t mxfp6_unpack_block(const mxfp6_u32x6_t& c, uint32_t sb) {
  mxfp6_u32x16_t o = mxfp6_cvt_unpack_raw(c, __uint_as_float(sb << 23));
  if (sb == kMxfp6NanScale) {
#pragma unroll
    for (int i = 0; i < 16; ++i) o[i] = kMxfp6NanPair;
  }
  return o;
}

// In-register 4x4 transpose across the 4 rows (16 lanes each) of a wave and 4
// registers of 16 B: afterwards register q of lane m + 16 r holds what register
// r of lane m + 16 q held (the pattern of crc32c.hip's row_transpose:
// v_permlane16_swap exchanges row bit 0 with register bit 0, v_permlane32_swap
// row bit 1 with register bit 1). Every lane of the wave must be active.
__device__ __forceinline__ void mxfp6_row_transpose(mxfp6_u32x4_t& r0, mxfp6_u32x4_t& r1, mxfp6_u32x4_t& r2,
                                                    mxfp6_u32x4_t& r3) {
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    const auto a = __builtin_amdgcn_permlane16_swap(r0[d], r1[d], false, false);
    const auto b = __builtin_amdgcn_permlane16_swap(r2[d], r3[d], false, false);
    const auto c = __builtin_amdgcn_permlane32_swap(a[0], b[0], false, false);
    const auto e = __builtin_amdgcn_permlane32_swap(a[1], b[1], false, false);
    r0[d] = c[0];
    r2[d] = c[1];
    r1[d] = e[0];
    r3[d] = e[1];
  }
}

}  // namespace kern
}  // namespace dissem
