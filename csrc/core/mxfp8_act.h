// MXFP8 activations: the x side of the W4A8 linears (kernels/mxfp4_mx.hip), which
// feed v_mfma_scale_f32_16x16x128_f8f6f4 an e4m3 operand with one E8M0 scale
// byte per 32 values along K.
//
// A row of K bf16 values (K a multiple of 32) becomes K OCP e4m3fn codes and
// K / 32 scale bytes; block b is elements [32 b, 32 b + 32) of the row. This is
// core/fp8.h at block = 32 and nothing else: E is scale_exp of the block's
// finite amax, the codes are f32_to_e4m3(x * 2^-E) saturated at sat_limit(E)
// (+-inf saturate, NaN -> 0x7F | sign), and the stored byte is E + 127, the
// exponent field of fp8's f32 scale 2^E (E in [-126, 120], so the byte is in
// [1, 247] and never the E8M0 NaN 0xFF). The dequantized value is
// code * 2^(byte - 127) in exact arithmetic; a NaN code stays NaN.
#pragma once

#include <cstdint>

namespace dissem {
namespace mxfp8 {

constexpr int kBlock = 32;

// n = rows * K elements (a multiple of 32) -> n codes, n / 32 scale bytes.
void quantize_host(const uint16_t* bf16, int64_t n, uint8_t* codes, uint8_t* scales);

}  // namespace mxfp8
}  // namespace dissem
