// The pack side of kernels/fp8.hip as device code, shared with the activation
// quantizer (mxfp8_act.hip): the block scale of core/fp8.h from the finite amax
// of `block` = 8 * LANES elements and the e4m3fn codes of a thread's 8 of them,
// byte for byte fp8::pack_host. Everything here has internal linkage.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels/dpp.h"

namespace dissem {
namespace kern {
namespace {

__device__ inline float bf16_to_f32(uint16_t b) { return __uint_as_float(uint32_t(b) << 16); }

// E of the block scale 2^E from the block's finite amax: core/fp8.h scale_exp.
__device__ inline int scale_exp(uint32_t amax_bits) {
  if (amax_bits == 0) return 0;
  const int ef = int(amax_bits >> 23);
  if (ef == 0) return -126;
  const int e = ef - 127 - 8 + ((amax_bits & 0x7FFFFFu) > 0x600000u ? 1 : 0);
  return e < -126 ? -126 : e;
}

__device__ inline bool finite(float x) { return (__float_as_uint(x) & 0x7F800000u) != 0x7F800000u; }

// q: the codes of the four bf16 in words a and b. Where one of them is a NaN its code becomes
// 0x7F | sign, found on the bf16 bits two at a time.
__device__ inline uint32_t nan_codes(uint32_t a, uint32_t b, uint32_t q) {
  const uint32_t na = ((a & 0x7FFF7FFFu) + 0x007F007Fu) & 0x80008000u;  // bit 15 / 31: that half is a NaN
  const uint32_t nb = ((b & 0x7FFF7FFFu) + 0x007F007Fu) & 0x80008000u;
  const uint32_t n = __builtin_amdgcn_perm(nb, na, 0x07050301u);              // one byte per element: 0x80 if NaN
  const uint32_t s = __builtin_amdgcn_perm(b, a, 0x07050301u) & 0x80808080u;  // and its sign bit
  const uint32_t m = (n >> 7) * 0xFFu;                                        // 0xFF if NaN
  return (q & ~m) | (m & (0x7F7F7F7Fu | s));
}

// The codes of the 8 bf16 in `v` (element 0 in the low byte of .x) and E of their block's scale
// 2^E. The block is the 8 * LANES elements of LANES adjacent lanes, which reduce the amax with
// DPP / permlane swaps: every lane of the wave must call this (inactive ones with zeros).
template <int LANES>
__device__ inline uint2 fp8_pack8(uint4 v, int& e_out) {
  float x[8];
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    x[2 * i] = bf16_to_f32(uint16_t(w[i] & 0xFFFF));
    x[2 * i + 1] = bf16_to_f32(uint16_t(w[i] >> 16));
  }
  float amax = 0.f;
  bool special = false;  // an inf or a NaN among this thread's values
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const bool f = finite(x[i]);
    special |= !f;
    if (f) amax = fmaxf(amax, fabsf(x[i]));
  }
  amax = group_max<LANES>(amax);
  const int e = scale_exp(__float_as_uint(amax));
  const float inv = __uint_as_float(uint32_t(127 - e) << 23);  // 2^-E, E in [-126, 120]
  const float lim = e >= 120 ? 240.0f : 448.0f;                  // core/fp8.h sat_limit
  // Saturate finite and infinite values. A NaN may come out as anything: its code is rewritten below.
  float y[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) y[i] = __builtin_amdgcn_fmed3f(x[i] * inv, lim, -lim);
  int lo = __builtin_amdgcn_cvt_pk_fp8_f32(y[0], y[1], 0, false);
  lo = __builtin_amdgcn_cvt_pk_fp8_f32(y[2], y[3], lo, true);
  int hi = __builtin_amdgcn_cvt_pk_fp8_f32(y[4], y[5], 0, false);
  hi = __builtin_amdgcn_cvt_pk_fp8_f32(y[6], y[7], hi, true);
  // NaN -> 0x7F | the input's sign (core/fp8.h). Left to the hardware, the multiply and the
  // converter give 0xFF for a NaN of either sign (measured on MI355X), and keeping NaNs out of
  // v_med3 costs a compare and a select per element. NaNs are rare: threads without an inf or a
  // NaN skip this branch.
  if (special) {
    lo = int(nan_codes(w[0], w[1], uint32_t(lo)));
    hi = int(nan_codes(w[2], w[3], uint32_t(hi)));
  }
  e_out = e;
  return make_uint2(uint32_t(lo), uint32_t(hi));
}

}  // namespace
}  // namespace kern
}  // namespace dissem
