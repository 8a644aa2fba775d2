#include "core/mxfp6.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace dissem {
namespace mxfp6 {

namespace {
inline float bf16_to_f32(uint16_t b) {
  uint32_t u = uint32_t(b) << 16;
  float f;
  memcpy(&f, &u, 4);
  return f;
}
// magnitude * 2^(byte - 127) is exact in f32 (the smallest is 2^-130) and in
// bf16 for byte <= 252; bytes 253 and 254 (never packed) overflow to inf where
// the product does.
inline uint16_t exact_f32_to_bf16(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  return uint16_t(u >> 16);
}
inline uint16_t unpack_one(const uint8_t* block, int i, uint8_t s) {
  if (s == kNanScale) return 0x7FC0;
  return exact_f32_to_bf16(std::ldexp(e2m3_to_f32(get_code(block, i)), int(s) - 127));
}
}  // namespace

uint8_t f32_to_e2m3(float y, bool negative) {
  const float a = std::fmin(std::fabs(y), 7.5f);
  // The magnitudes are linear in the code within each range: steps of 1/8 below
  // 2 (codes 0..16), 1/4 up to 4 (16..24), 1/2 up to 7.5 (24..31). The index is
  // rounded to nearest, a tie to the even index - which is the even code, since
  // every range starts at an even code.
  int base;
  float v;
  if (a < 2.0f) base = 0, v = a * 8.0f;
  else if (a < 4.0f) base = 16, v = (a - 2.0f) * 4.0f;
  else base = 24, v = (a - 4.0f) * 2.0f;
  const float fl = std::floor(v), fr = v - fl;  // exact: a has 8 significant bits or rounds far from a tie
  int k = int(fl);
  if (fr > 0.5f || (fr == 0.5f && (k & 1))) ++k;
  return uint8_t((negative ? 32 : 0) | (base + k));
}

float e2m3_to_f32(uint8_t code) {
  const int m = code & 31;
  const float v = m < 8 ? float(m) / 8.0f : std::ldexp(1.0f + float(m & 7) / 8.0f, (m >> 3) - 1);
  return (code & 32) ? -v : v;
}

void pack_host(const uint16_t* in, int64_t n, uint8_t* q, uint8_t* scales) {
  for (int64_t b = 0; b < n / kBlock; ++b) {
    const uint16_t* x = in + b * kBlock;
    uint8_t* qb = q + b * kBlockBytes;
    float amax = 0.f;
    bool nan = false;
    for (int i = 0; i < kBlock; ++i) {
      const float v = bf16_to_f32(x[i]);
      if (std::isnan(v)) nan = true;
      else if (std::isfinite(v)) amax = std::fmax(amax, std::fabs(v));
    }
    memset(qb, 0, kBlockBytes);
    if (nan) {
      scales[b] = kNanScale;
      continue;
    }
    uint32_t ab;
    memcpy(&ab, &amax, 4);
    const int e = scale_exp(ab);
    const float inv = std::ldexp(1.0f, -e);  // exact: x * 2^-E only moves the exponent
    for (int i = 0; i < kBlock; ++i) {
      const float y = std::fmin(std::fabs(bf16_to_f32(x[i])) * inv, 7.5f);  // +-inf saturates
      const uint32_t c = f32_to_e2m3(y, (x[i] & 0x8000) != 0);
      const int bit = 6 * i, byte = bit >> 3, sh = bit & 7;
      qb[byte] = uint8_t(qb[byte] | (c << sh));
      if (sh > 2) qb[byte + 1] = uint8_t(qb[byte + 1] | (c >> (8 - sh)));
    }
    scales[b] = uint8_t(e + 127);
  }
}

void unpack_host(const uint8_t* q, const uint8_t* scales, int64_t n, uint16_t* out) {
  for (int64_t i = 0; i < n; ++i) {
    const int64_t b = i / kBlock;
    out[i] = unpack_one(q + b * kBlockBytes, int(i % kBlock), scales[b]);
  }
}

void pack_layer_host(const uint8_t* src, int64_t src_bytes, int64_t src_chunk, uint8_t* dst) {
  check(src_bytes, src_chunk);
  for (int64_t off = 0; off < src_bytes; off += src_chunk) {
    const int64_t n = std::min(src_chunk, src_bytes - off) / 2;
    uint8_t* out = dst + (off / src_chunk) * packed_chunk(src_chunk);
    pack_host(reinterpret_cast<const uint16_t*>(src + off), n, out, out + n / kBlock * kBlockBytes);
  }
}

void unpack_layer_host(const uint8_t* packed, int64_t src_bytes, int64_t src_chunk, uint8_t* dst) {
  check(src_bytes, src_chunk);
  for (int64_t off = 0; off < src_bytes; off += src_chunk) {
    const int64_t n = std::min(src_chunk, src_bytes - off) / 2;
    const uint8_t* in = packed + (off / src_chunk) * packed_chunk(src_chunk);
    unpack_host(in, in + n / kBlock * kBlockBytes, n, reinterpret_cast<uint16_t*>(dst + off));
  }
}

void unpack_range_host(const uint8_t* packed, int64_t src_bytes, int64_t src_chunk, int64_t elem_off, int64_t n,
                       uint16_t* out) {
  check(src_bytes, src_chunk);
  const int64_t total = src_bytes / 2, ce = src_chunk / 2;
  if (elem_off < 0 || n < 0 || elem_off > total || n > total - elem_off)
    throw std::runtime_error("mxfp6 element range lies outside the layer");
  for (int64_t e = elem_off, end = elem_off + n; e < end;) {
    const int64_t c = e / ce, r = e - c * ce;
    const int64_t nc = std::min(ce, total - c * ce);  // elements of this chunk
    const int64_t take = std::min(end - e, nc - r);
    const uint8_t* q = packed + c * packed_chunk(src_chunk);
    const uint8_t* scales = q + nc / kBlock * kBlockBytes;
    uint16_t* o = out + (e - elem_off);
    for (int64_t i = r; i < r + take; ++i)
      o[i - r] = unpack_one(q + i / kBlock * kBlockBytes, int(i % kBlock), scales[i / kBlock]);
    e += take;
  }
}

}  // namespace mxfp6
}  // namespace dissem
