// fp8 wire/storage format of a layer (BASELINE config #5: 126 x 3 GiB
// Llama-3.1-405B-sized layers, which only fit one MI355X's 288 GB of HBM as
// fp8; the reference has no packing, it moves opaque bytes).
//
// A bf16 layer is cut on the source chunk grid (`src_chunk` bytes). Source
// chunk c of n bf16 elements packs into one packed chunk:
//     [ q: n bytes of OCP e4m3fn ][ scales: n/block f32 ]
// with one scale per `block` consecutive elements. The scale is a power of two,
// 2^E with E the smallest integer such that amax <= 448 * 2^E over the block's
// finite values (E = 0 if none, E >= -126): an E8M0-valued scale (stored as
// f32), so gfx950's scaled conversions (v_cvt_scalef32_pk_bf16_fp8, which
// apply only the scale's exponent) dequantize a pair of values in one
// instruction. Packed chunks are laid end to end, so the packed layer has its
// own uniform chunk grid of packed_chunk(src_chunk) bytes and every transfer,
// CRC and retry runs on that grid unchanged.
//
// Unpack gives q * 2^E rounded to bf16, to nearest and ties to even. The
// product is exact (a 4-bit significand) wherever it is a multiple of bf16's
// smallest subnormal, 2^-133: for every code at E >= -124. It is rounded for
// 48 (code, E) pairs: at E = -126 the codes +-{1, 2, 3, 5, 6, 7, 9, 10, 11, 13,
// 14, 15, 17, 19, 21, 23} and at E = -125 the codes +-{1, 3, 5, 7, 9, 11, 13, 15}
// (2^-135 and 2^-134 steps; pack writes such codes for blocks of bf16
// subnormals). From E = -118 down many exact products are bf16 subnormals. The
// host codec (an f32 product, then round-to-nearest-even to bf16),
// v_cvt_scalef32_pk_bf16_fp8 in both kernels (measured on MI355X for every
// code at every E) and the tests' numpy reference agree on all of them bit for
// bit. sat_limit keeps every product pack can write finite; the codes
// +-0x78..0x7E at E = 120 (256 * 2^120 and more), which pack never writes,
// are outside the format and their value is unspecified (host and kernels
// happen to agree on +-inf).
//
// NaN packs to 0x7F | the input's sign. A NaN code of either sign unpacks to
// the bf16 NaN 0xFFC0: that is what v_cvt_scalef32_pk_bf16_fp8 gives for both,
// and the host codec writes the same bits. -0 and negative values that round
// to zero keep their sign (0x80).
#pragma once

#include <cstdint>
#include <stdexcept>

namespace dissem {
namespace fp8 {

inline int64_t packed_len(int64_t src_bytes, int block) {  // one chunk
  const int64_t n = src_bytes / 2;
  return n + (n / block) * 4;
}
inline int64_t packed_chunk(int64_t src_chunk, int block) { return packed_len(src_chunk, block); }
inline void check(int64_t src_bytes, int64_t src_chunk, int block) {
  if (block != 32 && block != 64 && block != 128 && block != 256 && block != 512)
    throw std::runtime_error("fp8 block must be 32, 64, 128, 256 or 512");
  if (src_chunk % (2 * block)) throw std::runtime_error("fp8 source chunk must hold whole scale blocks");
  if (src_bytes % (2 * block))
    throw std::runtime_error("fp8 packing needs a layer size that is a multiple of 2*block bytes");
}
inline int64_t packed_size(int64_t src_bytes, int64_t src_chunk, int block) {
  const int64_t full = src_bytes / src_chunk, tail = src_bytes % src_chunk;
  return full * packed_chunk(src_chunk, block) + (tail ? packed_len(tail, block) : 0);
}
// Inverse of packed_size (throws if `packed` is not a packed layer size).
inline int64_t source_size(int64_t packed, int64_t src_chunk, int block) {
  const int64_t pc = packed_chunk(src_chunk, block);
  const int64_t full = packed / pc, tail = packed % pc;
  // tail = t/2 + t/(2*block)*4 = t*(block+4)/(2*block) for t a multiple of 2*block
  const int64_t t = tail * 2 * block / (block + 4);
  if (packed_len(t, block) != tail) throw std::runtime_error("size is not a packed fp8 layer size");
  return full * src_chunk + t;
}

// E of a block's scale 2^E from its finite amax (>= 0): exact integer logic on
// the f32 bits (448 = 1.75 * 2^8), identical in the gfx950 pack kernel.
inline int scale_exp(uint32_t amax_bits) {
  if (amax_bits == 0) return 0;
  const int ef = int(amax_bits >> 23);
  if (ef == 0) return -126;  // f32 subnormal amax: the lowest normal scale
  const int e = ef - 127 - 8 + ((amax_bits & 0x7FFFFFu) > 0x600000u ? 1 : 0);
  return e < -126 ? -126 : e;
}

// Largest code magnitude of a block with scale 2^E: 448, except 240 at E = 120
// (only blocks whose amax is within 2^-4 of bf16's max get there), where
// 256 * 2^120 would overflow bf16 on unpack (the bf16 maximum is 255 * 2^120).
inline float sat_limit(int e) { return e >= 120 ? 240.0f : 448.0f; }

// Host reference, byte for byte the gfx950 pack kernel on every bf16 input:
// x * 2^-E has at most 8 significant bits, so it is either exactly on a
// rounding tie (1/16 of all values) or more than 2^-8 of its own magnitude
// away from one, and host and hardware round both cases alike. Only for general f32
// input (not reachable through pack) does v_cvt_pk_fp8_f32 double-round values
// within 2^-18 of a tie (168.0000153 -> 160, not 176), where f32_to_e4m3 does not.
uint8_t f32_to_e4m3(float x);  // RNE, finite |x| <= 448 expected, NaN -> 0x7F|sign
float e4m3_to_f32(uint8_t q);
void pack_host(const uint16_t* bf16, int64_t n, uint8_t* q, float* scales, int block);
void unpack_host(const uint8_t* q, const float* scales, int64_t n, uint16_t* bf16, int block);
// Whole layer: src_bytes of bf16 -> packed_size(...) bytes in the chunked layout.
void pack_layer_host(const uint8_t* src, int64_t src_bytes, int64_t src_chunk, int block, uint8_t* dst);
void unpack_layer_host(const uint8_t* packed, int64_t src_bytes, int64_t src_chunk, int block, uint8_t* dst);
// Elements [elem_off, elem_off + n) of the packed layer (any offset and length
// inside it; throws otherwise): the one definition of where an element lives.
// Element e is in chunk c = e / (src_chunk / 2); with r = e - c * (src_chunk / 2)
// and n_c the elements of that chunk (the tail chunk is laid out on its own
// length), its code is byte r of the packed chunk and its f32 scale is at byte
// n_c + 4 * (r / block). What a consumer of the packed bytes in place
// (kernels/fp8_linear.hip) reads; the values are unpack_host's.
void unpack_range_host(const uint8_t* packed, int64_t src_bytes, int64_t src_chunk, int block, int64_t elem_off,
                       int64_t n, uint16_t* out);

}  // namespace fp8
}  // namespace dissem
