// MXFP4 wire/storage format of a layer (OCP MX: e2m1 elements, one E8M0 scale
// per 32): the format MI355X's block-scaled matrix instructions
// (v_mfma_scale_f32_*_f8f6f4) consume, and the densest one this project ships
// and stores - 17/64 of the bf16 bytes, against 33/64 for fp8 at block 32.
//
// A bf16 layer is cut on the source chunk grid (`src_chunk` bytes), exactly as
// in core/fp8.h. Source chunk c of n bf16 elements packs into one packed chunk:
//     [ q: n/2 bytes, two e2m1 codes per byte, element 2k in the low nibble ]
//     [ scales: n/32 bytes, E8M0 ]
// The scale block is fixed at 32 elements, so one 16-B word of q is exactly one
// scale block, and with a source chunk that is a multiple of 1024 B both the
// q/scale boundary and the packed chunk are multiples of 16 B. A layer must be
// a multiple of 64 B (one block); the tail chunk uses the same formula on its
// own length.
//
// Code: sign << 3 | m, with magnitudes of m = 0..7: 0, 0.5, 1, 1.5, 2, 3, 4, 6.
//
// Scale of a block: 2^E with E the smallest integer such that amax <= 6 * 2^E
// over the block's finite values, clamped to [-126, 125] - the no-clipping rule
// of core/fp8.h, not OCP's floor rule. E = 0 when amax is 0 or the block has no
// finite value, E = -126 for a subnormal amax. The stored byte is E + 127
// (1..252). The cap at 125 means a block whose amax exceeds 1.5 * 2^127
// saturates its top values to 6 * 2^125, which is finite in bf16: no element
// can overflow on unpack.
//
// Elements: y = x * 2^-E clamped to +-6 (so +-inf saturates), rounded to the
// nearest magnitude, ties to the even code (0.25 -> 0, 0.75 -> 1, 1.25 -> 1,
// 1.75 -> 2, 2.5 -> 2, 3.5 -> 4, 5 -> 4). The source's sign bit is always kept
// (-0.1 packs to code 8).
//
// NaN: e2m1 has none, so OCP's rule applies: a block that contains any NaN
// stores scale byte 0xFF and 16 zero q bytes, and unpacks to 32 NaNs (0x7FC0).
// A payload of random bytes therefore loses about one block in eight (a random
// bf16 is a NaN with probability 127/32768; 1 - (1 - 127/32768)^32 = 11.7 %):
// the format is for weights, not for opaque bytes.
//
// Unpack: value[m] * 2^(byte - 127) with the sign is exactly representable in
// bf16, subnormals included (byte 0 scales by 2^-127).
//
// As an MFMA operand: measured once on MI355X through kernels/mxfp4_linear.hip,
// v_mfma_f32_16x16x32_bf16 keeps bf16-subnormal operands and f32-subnormal
// sums - weights of 2^-127 (scale byte 0) times x = 2^120 over K = 32 gave
// exactly 0.25, x = 2^-130 times weights of 2^123 likewise, and 32 * 2^-136
// came out as 2^-131 - so the smallest scales are not flushed there. No test
// asserts it (the instruction's denormal handling is not documented).
//
// The host functions below define the format; the gfx950 kernels
// (kernels/mxfp4.hip, the fused check in kernels/crc32c.hip) produce the same
// bytes.
#pragma once

#include <cstdint>
#include <stdexcept>

namespace dissem {
namespace mxfp4 {

constexpr int kBlock = 32;  // elements per scale (OCP MX)

inline int64_t packed_len(int64_t src_bytes) {  // one chunk
  const int64_t n = src_bytes / 2;
  return n / 2 + n / kBlock;
}
inline int64_t packed_chunk(int64_t src_chunk) { return packed_len(src_chunk); }
inline void check(int64_t src_bytes, int64_t src_chunk) {
  if (src_chunk <= 0 || src_chunk % 1024)
    throw std::runtime_error("mxfp4 source chunk must be a multiple of 1024 B (16-B aligned packed chunks)");
  if (src_bytes % (2 * kBlock))
    throw std::runtime_error("mxfp4 packing needs a layer size that is a multiple of 64 B (32 bf16 per scale)");
}
inline int64_t packed_size(int64_t src_bytes, int64_t src_chunk) {
  const int64_t full = src_bytes / src_chunk, tail = src_bytes % src_chunk;
  return full * packed_chunk(src_chunk) + (tail ? packed_len(tail) : 0);
}
// Inverse of packed_size (throws if `packed` is not a packed layer size).
inline int64_t source_size(int64_t packed, int64_t src_chunk) {
  const int64_t pc = packed_chunk(src_chunk);
  const int64_t full = packed / pc, tail = packed % pc;
  // tail = 17 bytes per 64 source bytes
  const int64_t t = tail / 17 * 64;
  if (packed_len(t) != tail) throw std::runtime_error("size is not a packed mxfp4 layer size");
  return full * src_chunk + t;
}

// E of a block's scale 2^E from its finite amax (>= 0): exact integer logic on
// the f32 bits (6 = 1.5 * 2^2), identical in the gfx950 pack kernel.
inline int scale_exp(uint32_t amax_bits) {
  if (amax_bits == 0) return 0;
  const int ef = int(amax_bits >> 23);
  if (ef == 0) return -126;  // subnormal amax: the lowest scale
  const int e = ef - 127 - 2 + ((amax_bits & 0x7FFFFFu) > 0x400000u ? 1 : 0);
  return e < -126 ? -126 : e > 125 ? 125 : e;
}

constexpr uint8_t kNanScale = 0xFF;

// Host reference.
uint8_t f32_to_e2m1(float y, bool negative);  // |y| <= 6 expected (clamped), RNE to the even code
float e2m1_to_f32(uint8_t code);              // low 4 bits
void pack_host(const uint16_t* bf16, int64_t n, uint8_t* q, uint8_t* scales);
void unpack_host(const uint8_t* q, const uint8_t* scales, int64_t n, uint16_t* bf16);
// Whole layer: src_bytes of bf16 -> packed_size(...) bytes in the chunked layout.
void pack_layer_host(const uint8_t* src, int64_t src_bytes, int64_t src_chunk, uint8_t* dst);
void unpack_layer_host(const uint8_t* packed, int64_t src_bytes, int64_t src_chunk, uint8_t* dst);
// Elements [elem_off, elem_off + n) of a chunked packed layer -> n bf16: the one
// definition of where an element of the layer lives (chunk e / (src_chunk / 2),
// code and scale block at its offset in that chunk, the tail chunk on its own
// length). Any offset and length inside the layer; throws otherwise.
void unpack_range_host(const uint8_t* packed, int64_t src_bytes, int64_t src_chunk, int64_t elem_off, int64_t n,
                       uint16_t* out);

}  // namespace mxfp4
}  // namespace dissem
