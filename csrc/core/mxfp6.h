// MXFP6 wire/storage format of a layer (OCP MX: e2m3 elements, one E8M0 scale
// per 32): the middle format between fp8 and MXFP4 - 25/64 of the bf16 bytes,
// against 33/64 for fp8 at block 128 and 17/64 for MXFP4 - with an error in
// fp8's class (three mantissa bits, as e4m3 has). MI355X converts 32 of these
// per instruction (v_cvt_scalef32_pk32_{fp6_bf16,bf16_fp6}) and its
// block-scaled matrix instructions take the 24-byte blocks as they are stored.
//
// A bf16 layer is cut on the source chunk grid (`src_chunk` bytes), exactly as
// in core/mxfp4.h. Source chunk c of n bf16 elements packs into one packed chunk:
//     [ q: 3n/4 bytes, one 24-byte block per 32 elements ]
//     [ scales: n/32 bytes, E8M0 ]
// Block b of the chunk is the 24 bytes at 24 b. Element i of the block is bits
// [6i, 6i + 6) of those 24 bytes read as one little-endian integer: element 0
// is the low 6 bits of byte 0, element 1 the top 2 bits of byte 0 and the low 4
// of byte 1, and so on; four elements fill three bytes. With a source chunk
// that is a multiple of 1024 B the packed chunk (400 B per KiB) and its q/scale
// boundary (384 B per KiB) are multiples of 16 B. A layer must be a multiple of
// 64 B (one block); the tail chunk uses the same formula on its own length, so
// its scale region is only 8-B aligned and its block count may be odd.
//
// Code: sign << 5 | m, m = 0..31. Magnitude of m: (m & 7) / 8 for m < 8, else
// (1 + (m & 7) / 8) * 2^((m >> 3) - 1): 0, 0.125 .. 0.875, 1 .. 1.875,
// 2 .. 3.75 (steps of 0.25), 4 .. 7.5 (steps of 0.5).
//
// Scale of a block: 2^E with E the smallest integer such that amax <= 7.5 * 2^E
// over the block's finite values, clamped to [-126, 125] - the no-clipping rule
// of core/fp8.h and core/mxfp4.h. E = 0 when amax is 0 or the block has no
// finite value, E = -126 for a subnormal amax. The stored byte is E + 127
// (1..252). 7.5 * 2^125 = 1.875 * 2^127 is finite in bf16, so nothing packed
// unpacks to inf.
//
// Elements: y = x * 2^-E clamped to +-7.5 (so +-inf saturates), rounded to the
// nearest magnitude, ties to the even code. The source's sign bit is always
// kept (-0.1 in a block of E = 0 packs to 0.125 with the sign: code 33).
//
// NaN: e2m3 has none, so OCP's rule applies: a block that contains any NaN
// stores scale byte 0xFF and 24 zero q bytes. Scale byte 0xFF unpacks to 32
// NaNs (0x7FC0) whatever q holds.
//
// Unpack: +-magnitude * 2^(byte - 127), exact in bf16 for bytes 0..252,
// subnormals included (the smallest, 0.125 * 2^-127 = 2^-130, is a bf16
// subnormal). Bytes 253 and 254 are never written by pack; they unpack exactly
// where the product is finite and to +-inf beyond bf16's range.
//
// The host functions below define the format; the gfx950 kernels
// (kernels/mxfp6.hip) produce the same bytes.
#pragma once

#include <cstdint>
#include <stdexcept>

namespace dissem {
namespace mxfp6 {

constexpr int kBlock = 32;       // elements per scale (OCP MX)
constexpr int kBlockBytes = 24;  // 32 six-bit codes

inline int64_t packed_len(int64_t src_bytes) {  // one chunk
  const int64_t n = src_bytes / 2;
  return n / kBlock * kBlockBytes + n / kBlock;
}
inline int64_t packed_chunk(int64_t src_chunk) { return packed_len(src_chunk); }
inline void check(int64_t src_bytes, int64_t src_chunk) {
  if (src_chunk <= 0 || src_chunk % 1024)
    throw std::runtime_error("mxfp6 source chunk must be a multiple of 1024 B (16-B aligned packed chunks)");
  if (src_bytes % (2 * kBlock))
    throw std::runtime_error("mxfp6 packing needs a layer size that is a multiple of 64 B (32 bf16 per scale)");
}
inline int64_t packed_size(int64_t src_bytes, int64_t src_chunk) {
  const int64_t full = src_bytes / src_chunk, tail = src_bytes % src_chunk;
  return full * packed_chunk(src_chunk) + (tail ? packed_len(tail) : 0);
}
// Inverse of packed_size (throws if `packed` is not a packed layer size).
inline int64_t source_size(int64_t packed, int64_t src_chunk) {
  const int64_t pc = packed_chunk(src_chunk);
  const int64_t full = packed / pc, tail = packed % pc;
  // tail = 25 bytes per 64 source bytes
  const int64_t t = tail / 25 * 64;
  if (packed_len(t) != tail) throw std::runtime_error("size is not a packed mxfp6 layer size");
  return full * src_chunk + t;
}

// E of a block's scale 2^E from its finite amax (>= 0): exact integer logic on
// the f32 bits (7.5 = 1.875 * 2^2), identical in the gfx950 pack kernel.
inline int scale_exp(uint32_t amax_bits) {
  if (amax_bits == 0) return 0;
  const int ef = int(amax_bits >> 23);
  if (ef == 0) return -126;  // subnormal amax: the lowest scale
  const int e = ef - 127 - 2 + ((amax_bits & 0x7FFFFFu) > 0x700000u ? 1 : 0);
  return e < -126 ? -126 : e > 125 ? 125 : e;
}

constexpr uint8_t kNanScale = 0xFF;

// Code i (0..31) of a 24-byte block.
inline uint8_t get_code(const uint8_t* block, int i) {
  const int bit = 6 * i, byte = bit >> 3, sh = bit & 7;
  uint32_t v = block[byte];
  if (sh > 2) v |= uint32_t(block[byte + 1]) << 8;  // the code straddles two bytes (byte + 1 <= 23)
  return uint8_t((v >> sh) & 63u);
}

// Host reference.
uint8_t f32_to_e2m3(float y, bool negative);  // |y| <= 7.5 expected (clamped), RNE to the even code
float e2m3_to_f32(uint8_t code);              // low 6 bits
void pack_host(const uint16_t* bf16, int64_t n, uint8_t* q, uint8_t* scales);
void unpack_host(const uint8_t* q, const uint8_t* scales, int64_t n, uint16_t* bf16);
// Whole layer: src_bytes of bf16 -> packed_size(...) bytes in the chunked layout.
void pack_layer_host(const uint8_t* src, int64_t src_bytes, int64_t src_chunk, uint8_t* dst);
void unpack_layer_host(const uint8_t* packed, int64_t src_bytes, int64_t src_chunk, uint8_t* dst);
// Elements [elem_off, elem_off + n) of a chunked packed layer -> n bf16: the one
// definition of where an element of the layer lives (chunk e / (src_chunk / 2),
// block and scale at its offset in that chunk, the tail chunk on its own
// length). Any offset and length inside the layer; throws otherwise.
void unpack_range_host(const uint8_t* packed, int64_t src_bytes, int64_t src_chunk, int64_t elem_off, int64_t n,
                       uint16_t* out);

}  // namespace mxfp6
}  // namespace dissem
