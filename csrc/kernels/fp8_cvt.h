// gfx950 device helpers shared by the fp8 kernels (fp8.hip, crc32c.hip) and the kernels of the
// MXFP8 KV cache (attn_decode_mxfp8.hip, attn_prefill_mxfp8.hip).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace dissem {
namespace kern {

// Two OCP e4m3fn codes (bytes 0-1 of `w`, or bytes 2-3 if HI) times the
// power-of-two block scale `s` -> two bf16 (first value in the low half):
// v_cvt_scalef32_pk_bf16_fp8, one VALU per pair. The instruction applies only
// the exponent of `s` (an E8M0 scale; profiles/r3_cvt), which is all a
// core/fp8.h scale has. The result is the product rounded to bf16 to nearest,
// ties to even, bf16 subnormals included: measured on MI355X for every code at
// every E in [-126, 120] against core/fp8.h's rule (tests/test_gpu_fp8.py).
template <bool HI>
__device__ __forceinline__ uint32_t fp8x2_to_bf16x2(uint32_t w, float s) {
  return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(int(w), s, HI));
}

// The f32 whose exponent field is the E8M0 byte `e`: 2^(e - 127), and the instruction reads nothing else of it.
__device__ __forceinline__ float e8m0_scale(uint32_t e) { return __uint_as_float((e & 0xFFu) << 23); }

// Four codes (one word) times `s` as four bf16 in two operand words (the MXFP8 KV cache's kernels).
__device__ __forceinline__ void dequant4(uint32_t codes, float s, uint32_t& w0, uint32_t& w1) {
  w0 = fp8x2_to_bf16x2<false>(codes, s);
  w1 = fp8x2_to_bf16x2<true>(codes, s);
}

}  // namespace kern
}  // namespace dissem
