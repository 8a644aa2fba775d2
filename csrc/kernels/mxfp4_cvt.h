// gfx950 device helpers shared by the MXFP4 kernels (mxfp4.hip, crc32c.hip):
// e2m1 codes + E8M0 scale byte -> bf16, bit-exact with core/mxfp4.h.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace dissem {
namespace kern {

// Scale byte 0xFF marks a NaN block: every element unpacks to 0x7FC0. Every
// other byte goes to the hardware converter. Measured on MI355X against integer
// code for every (code byte, scale byte) pair (bin/cvtprobe):
// v_cvt_scalef32_pk_bf16_fp4 applies the exponent of its f32 scale operand
// exactly - bf16-subnormal results (scale bytes 0 and 1) and overflow to inf
// (253, 254, never written by pack) included. For 0xFF it returns NaNs that
// carry the code's sign (0xFFC0), so that byte's result is selected, not converted.
constexpr uint32_t kMxfp4NanScale = 0xFFu, kMxfp4NanPair = 0x7FC07FC0u;

// E of a block's scale from the bf16 bits of its finite amax: core/mxfp4.h scale_exp.
__device__ __forceinline__ int mxfp4_scale_exp(uint32_t amax_bf16) {
  if (amax_bf16 == 0) return 0;
  const int ef = int(amax_bf16 >> 7);
  if (ef == 0) return -126;
  const int e = ef - 127 - 2 + ((amax_bf16 & 0x7Fu) > 0x40u ? 1 : 0);
  return e < -126 ? -126 : e > 125 ? 125 : e;
}

// The two codes of byte SEL of `w` times the scale (an f32 whose exponent
// field is the E8M0 byte) -> two bf16, the low nibble's value in the low half.
template <int SEL>
__device__ __forceinline__ uint32_t fp4x2_to_bf16x2(uint32_t w, float s) {
  return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, s, SEL));
}

// 8 codes (one dword of q) with scale byte sb -> 8 bf16 (o[0..3], element 0 in
// the low half of o[0]).
__device__ __forceinline__ void mxfp4_unpack8(uint32_t w, uint32_t sb, uint32_t (&o)[4]) {
  const float s = __uint_as_float(sb << 23);
  const bool nan = sb == kMxfp4NanScale;
  o[0] = nan ? kMxfp4NanPair : fp4x2_to_bf16x2<0>(w, s);
  o[1] = nan ? kMxfp4NanPair : fp4x2_to_bf16x2<1>(w, s);
  o[2] = nan ? kMxfp4NanPair : fp4x2_to_bf16x2<2>(w, s);
  o[3] = nan ? kMxfp4NanPair : fp4x2_to_bf16x2<3>(w, s);
}

}  // namespace kern
}  // namespace dissem
