#include "core/mxfp4.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace dissem {
namespace mxfp4 {

namespace {
inline float bf16_to_f32(uint16_t b) {
  uint32_t u = uint32_t(b) << 16;
  float f;
  memcpy(&f, &u, 4);
  return f;
}
// value[m] * 2^(byte - 127) is exact in f32 (f32 subnormals reach 2^-149) and
// in bf16 for byte <= 252; bytes 253 and 254 (never packed) overflow to inf
// where the product does.
inline uint16_t exact_f32_to_bf16(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  return uint16_t(u >> 16);
}
}  // namespace

uint8_t f32_to_e2m1(float y, bool negative) {
  const float a = std::fabs(y);
  // midpoints between neighbours; a tie goes to the even code
  int m;
  if (a <= 0.25f) m = 0;
  else if (a < 0.75f) m = 1;
  else if (a <= 1.25f) m = 2;
  else if (a < 1.75f) m = 3;
  else if (a <= 2.5f) m = 4;
  else if (a < 3.5f) m = 5;
  else if (a <= 5.0f) m = 6;
  else m = 7;
  return uint8_t((negative ? 8 : 0) | m);
}

float e2m1_to_f32(uint8_t code) {
  static const float kMag[8] = {0.f, 0.5f, 1.f, 1.5f, 2.f, 3.f, 4.f, 6.f};
  const float v = kMag[code & 7];
  return (code & 8) ? -v : v;
}

void pack_host(const uint16_t* in, int64_t n, uint8_t* q, uint8_t* scales) {
  for (int64_t b = 0; b < n / kBlock; ++b) {
    const uint16_t* x = in + b * kBlock;
    uint8_t* qb = q + b * (kBlock / 2);
    float amax = 0.f;
    bool nan = false;
    for (int i = 0; i < kBlock; ++i) {
      const float v = bf16_to_f32(x[i]);
      if (std::isnan(v)) nan = true;
      else if (std::isfinite(v)) amax = std::fmax(amax, std::fabs(v));
    }
    if (nan) {
      memset(qb, 0, kBlock / 2);
      scales[b] = kNanScale;
      continue;
    }
    uint32_t ab;
    memcpy(&ab, &amax, 4);
    const int e = scale_exp(ab);
    const float inv = std::ldexp(1.0f, -e);  // exact: x * 2^-E only moves the exponent
    for (int i = 0; i < kBlock; i += 2) {
      uint8_t c[2];
      for (int k = 0; k < 2; ++k) {
        const float y = std::fmin(std::fabs(bf16_to_f32(x[i + k])) * inv, 6.0f);  // +-inf saturates
        c[k] = f32_to_e2m1(y, (x[i + k] & 0x8000) != 0);
      }
      qb[i / 2] = uint8_t(c[0] | (c[1] << 4));
    }
    scales[b] = uint8_t(e + 127);
  }
}

void unpack_host(const uint8_t* q, const uint8_t* scales, int64_t n, uint16_t* out) {
  for (int64_t i = 0; i < n; ++i) {
    const uint8_t s = scales[i / kBlock];
    if (s == kNanScale) {
      out[i] = 0x7FC0;
      continue;
    }
    const uint8_t code = (q[i / 2] >> (4 * (i & 1))) & 15;
    out[i] = exact_f32_to_bf16(std::ldexp(e2m1_to_f32(code), int(s) - 127));
  }
}

void pack_layer_host(const uint8_t* src, int64_t src_bytes, int64_t src_chunk, uint8_t* dst) {
  check(src_bytes, src_chunk);
  for (int64_t off = 0; off < src_bytes; off += src_chunk) {
    const int64_t n = std::min(src_chunk, src_bytes - off) / 2;
    uint8_t* out = dst + (off / src_chunk) * packed_chunk(src_chunk);
    pack_host(reinterpret_cast<const uint16_t*>(src + off), n, out, out + n / 2);
  }
}

void unpack_layer_host(const uint8_t* packed, int64_t src_bytes, int64_t src_chunk, uint8_t* dst) {
  check(src_bytes, src_chunk);
  for (int64_t off = 0; off < src_bytes; off += src_chunk) {
    const int64_t n = std::min(src_chunk, src_bytes - off) / 2;
    const uint8_t* in = packed + (off / src_chunk) * packed_chunk(src_chunk);
    unpack_host(in, in + n / 2, n, reinterpret_cast<uint16_t*>(dst + off));
  }
}

void unpack_range_host(const uint8_t* packed, int64_t src_bytes, int64_t src_chunk, int64_t elem_off, int64_t n,
                       uint16_t* out) {
  check(src_bytes, src_chunk);
  const int64_t total = src_bytes / 2, ce = src_chunk / 2;
  if (elem_off < 0 || n < 0 || elem_off > total || n > total - elem_off)
    throw std::runtime_error("mxfp4 element range lies outside the layer");
  for (int64_t e = elem_off, end = elem_off + n; e < end;) {
    const int64_t c = e / ce, r = e - c * ce;
    const int64_t nc = std::min(ce, total - c * ce);  // elements of this chunk
    const int64_t take = std::min(end - e, nc - r);
    const uint8_t* q = packed + c * packed_chunk(src_chunk);
    const uint8_t* scales = q + nc / 2;
    uint16_t* o = out + (e - elem_off);
    for (int64_t i = r; i < r + take; ++i) {
      const uint8_t s = scales[i / kBlock];
      if (s == kNanScale) {
        o[i - r] = 0x7FC0;
        continue;
      }
      const uint8_t code = (q[i / 2] >> (4 * (i & 1))) & 15;
      o[i - r] = exact_f32_to_bf16(std::ldexp(e2m1_to_f32(code), int(s) - 127));
    }
    e += take;
  }
}

}  // namespace mxfp4
}  // namespace dissem
