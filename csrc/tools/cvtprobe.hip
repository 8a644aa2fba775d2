// cvtprobe: what gfx950's scaled fp8 conversions compute (ISA semantics probe).
// Prints, for a few fp8 codes and scales, the bf16 results of
// v_cvt_scalef32_pk_bf16_fp8 next to code * scale, and the fp8 codes that
// v_cvt_scalef32_pk_fp8_bf16 produces for bf16 inputs.
//
// MXFP4 (core/mxfp4.h): exhaustive comparison of v_cvt_scalef32_pk_fp4_bf16 and
// v_cvt_scalef32_pk_bf16_fp4 with the integer reference of kernels/mxfp4_cvt.h
// - every bf16 pattern against every scale 2^E, E in [-126, 125], and every
// code byte against every scale byte - as mismatch counts per class of input.
//
// MXFP6 (core/mxfp6.h): the same for v_cvt_scalef32_pk32_fp6_bf16 and
// v_cvt_scalef32_pk32_bf16_fp6 (kernels/mxfp6_cvt.h): every bf16 pattern at
// every E in [-126, 125] (a lane converts 32 consecutive patterns, so each
// pattern is tried at one position and the positions see all patterns), every
// code in every one of the 32 positions under every scale byte, and the layout
// of the 6-dword operand (one element set, the others zero).
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>

#include "kernels/mxfp4_cvt.h"
#include "kernels/mxfp6_cvt.h"

typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef short i16x2 __attribute__((ext_vector_type(2)));

__global__ void unpack_probe(const int* codes, const float* scales, int n, uint32_t* out) {
  const int i = threadIdx.x;
  if (i >= n) return;
  bf16x2 r = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(codes[i], scales[i], false);
  out[i] = __builtin_bit_cast(uint32_t, r);
}

__global__ void pack_probe(const uint32_t* bf16pairs, const float* scales, int n, uint32_t* out) {
  const int i = threadIdx.x;
  if (i >= n) return;
  i16x2 old = {0, 0};
  auto r = __builtin_amdgcn_cvt_scalef32_pk_fp8_bf16(old, __builtin_bit_cast(bf16x2, bf16pairs[i]), scales[i], false);
  out[i] = uint32_t(__builtin_bit_cast(uint32_t, r));
}

// |x| (bf16 bits `a`, finite, at most 6 * 2^e) -> the e2m1 magnitude code of
// a * 2^-e, nearest with ties to the even code, in integer arithmetic: 4y =
// sig >> rs with a sticky bit, against the midpoints 0.25 ... 5 (all multiples
// of 0.25). The reference of the pack probe.
__device__ static uint32_t quant_bits(uint32_t a, int e) {
  const uint32_t ea = a >> 7;
  const uint32_t sig = ea ? 0x80u | (a & 0x7Fu) : a & 0x7Fu;
  const int rs0 = e + 132 - int(ea ? ea : 1u);  // >= 3 for |x| <= 6 * 2^e
  const uint32_t rs = uint32_t(rs0 > 31 ? 31 : rs0 < 0 ? 0 : rs0);
  const uint32_t key = ((sig >> rs) << 1) | ((sig & ((1u << rs) - 1u)) ? 1u : 0u);  // 2 * floor(4y), odd: a remainder
  return (key > 2u) + (key >= 6u) + (key > 10u) + (key >= 14u) + (key > 20u) + (key >= 28u) + (key > 40u);
}

// One code (low 4 bits) times 2^(sb - 127) as bf16 bits, in integer arithmetic.
__device__ static uint32_t bf16_bits(uint32_t code, uint32_t sb) {
  if (sb == 0xFFu) return 0x7FC0u;
  const uint32_t m = code & 7u, sign = (code & 8u) << 12;
  if (m == 0) return sign;
  // value = (1 + mant / 128) * 2^eo: 0.5, 1, 1.5, 2, 3, 4, 6
  const int eo = int(m >> 1) - 1;
  const uint32_t mant = (m & 1u) && m > 1 ? 0x40u : 0u;
  const int ee = int(sb) + eo;  // biased bf16 exponent
  if (ee >= 255) return sign | 0x7F80u;
  if (ee >= 1) return sign | (uint32_t(ee) << 7) | mant;
  return sign | ((0x80u | mant) >> (1 - ee));  // subnormal: exact, at most 2 bits shifted out of 0x80 / 1 of 0xC0
}

// ---- MXFP4. Classes of pack inputs (x, E), counted as [total, mismatches]:
enum { kInRange, kInRangeSub, kTie, kZero, kAbove, kInf, kNan, kPackClasses };
static const char* kPackClass[] = {"in_range_normal", "in_range_bf16_subnormal", "code_boundary", "zero",
                                   "above_6x2^E_finite", "inf", "nan"};

// blockIdx.y = E + 126; thread = bf16 pattern (the other half of the pair is its negation)
__global__ void fp4_pack_probe(unsigned long long* cnt, uint32_t* first_bad) {
  const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x;
  const int e = int(blockIdx.y) - 126;
  const uint32_t a = x & 0x7FFFu, lim = (uint32_t(e + 129) << 7) | 0x40u;
  const float s = __uint_as_float(uint32_t(e + 127) << 23);
  const uint32_t pair = x | ((x ^ 0x8000u) << 16);
  const uint32_t r = __builtin_amdgcn_cvt_scalef32_pk_fp4_bf16(0u, __builtin_bit_cast(bf16x2, pair), s, 0);
  int cls;
  uint32_t want;
  if (a > 0x7F80u) {
    cls = kNan, want = 7;  // no reference: counted as "mismatch" unless it saturates
  } else if (a == 0x7F80u) {
    cls = kInf, want = 7;
  } else if (a > lim) {
    cls = kAbove, want = 7;
  } else {
    want = quant_bits(a, e);
    // code_boundary: a bf16 neighbour of x rounds to another code (the ties are among these)
    const uint32_t up = quant_bits(a + 1 <= lim ? a + 1 : a, e);
    const uint32_t dn = quant_bits(a ? a - 1 : 0, e);
    cls = a == 0 ? kZero : (a < 0x80u ? kInRangeSub : ((up != want) != (dn != want) && up != dn ? kTie : kInRange));
  }
  const uint32_t lo = want | ((x >> 12) & 8u), hi = want | (((x ^ 0x8000u) >> 12) & 8u);
  const bool bad = (r & 0xFFu) != (lo | (hi << 4)) || (r >> 8) != 0;
  atomicAdd(&cnt[2 * cls], 1ull);
  if (bad) {
    if (atomicAdd(&cnt[2 * cls + 1], 1ull) == 0) {
      first_bad[3 * cls] = x;
      first_bad[3 * cls + 1] = uint32_t(e);
      first_bad[3 * cls + 2] = r;
    }
  }
}

// blockIdx.x = scale byte, thread = code byte (replicated in the 4 bytes, each SEL tried)
__global__ void fp4_unpack_probe(unsigned long long* bad_by_scale, uint32_t* first_bad) {
  const uint32_t sb = blockIdx.x, b = threadIdx.x;
  const float s = __uint_as_float(sb << 23);
  const uint32_t w = b * 0x01010101u;
  const uint32_t want = bf16_bits(b, sb) | (bf16_bits(b >> 4, sb) << 16);
  const uint32_t got[4] = {dissem::kern::fp4x2_to_bf16x2<0>(w, s), dissem::kern::fp4x2_to_bf16x2<1>(w, s),
                           dissem::kern::fp4x2_to_bf16x2<2>(w, s), dissem::kern::fp4x2_to_bf16x2<3>(w, s)};
  for (int k = 0; k < 4; ++k)
    if (got[k] != want && atomicAdd(&bad_by_scale[sb], 1ull) == 0) {
      first_bad[2 * sb] = b;
      first_bad[2 * sb + 1] = got[k];
    }
}

static void mxfp4_probe() {
  unsigned long long *cnt, *ubad;
  uint32_t *pfirst, *ufirst;
  hipMalloc(&cnt, 2 * kPackClasses * 8);
  hipMalloc(&pfirst, 3 * kPackClasses * 4);
  hipMalloc(&ubad, 256 * 8);
  hipMalloc(&ufirst, 512 * 4);
  hipMemset(cnt, 0, 2 * kPackClasses * 8);
  hipMemset(pfirst, 0, 3 * kPackClasses * 4);
  hipMemset(ubad, 0, 256 * 8);
  hipMemset(ufirst, 0, 512 * 4);
  fp4_pack_probe<<<dim3(256, 252), 256>>>(cnt, pfirst);
  fp4_unpack_probe<<<256, 256>>>(ubad, ufirst);
  unsigned long long hc[2 * kPackClasses], hu[256];
  uint32_t hp[3 * kPackClasses], hf[512];
  hipMemcpy(hc, cnt, sizeof hc, hipMemcpyDeviceToHost);
  hipMemcpy(hp, pfirst, sizeof hp, hipMemcpyDeviceToHost);
  hipMemcpy(hu, ubad, sizeof hu, hipMemcpyDeviceToHost);
  hipMemcpy(hf, ufirst, sizeof hf, hipMemcpyDeviceToHost);
  for (int c = 0; c < kPackClasses; ++c)
    printf("{\"op\": \"fp4_pack\", \"class\": \"%s\", \"inputs\": %llu, \"mismatches\": %llu, "
           "\"first\": {\"bf16\": \"0x%04x\", \"E\": %d, \"got\": \"0x%08x\"}}\n",
           kPackClass[c], hc[2 * c], hc[2 * c + 1], hp[3 * c], int(hp[3 * c + 1]), hp[3 * c + 2]);
  unsigned long long mid = 0;
  for (int sb = 2; sb <= 252; ++sb) mid += hu[sb];
  printf("{\"op\": \"fp4_unpack\", \"scale_bytes\": \"2..252\", \"mismatches\": %llu}\n", mid);
  for (int sb : {0, 1, 253, 254, 255})
    printf("{\"op\": \"fp4_unpack\", \"scale_bytes\": \"%d\", \"mismatches\": %llu, \"first\": "
           "{\"codes\": \"0x%02x\", \"got\": \"0x%08x\"}}\n", sb, hu[sb], hf[2 * sb], hf[2 * sb + 1]);
}

// ---- MXFP6.

// |x| (bf16 bits `a`, finite) -> the e2m3 magnitude code (0..31) of a * 2^-e
// clamped to 7.5, nearest with ties to the even code, in integer arithmetic:
// 8y as a 32.32 fixed-point number with a sticky bit, then the step of its range
// (1/8 below 2, 1/4 below 4, 1/2 above).
__device__ static uint32_t quant6_bits(uint32_t a, int e) {
  const uint32_t ea = a >> 7;
  const uint64_t sig = ea ? 0x80u | (a & 0x7Fu) : a & 0x7Fu;
  const int sh = int(ea ? ea : 1u) - 131 - e;  // 8y = sig * 2^sh
  uint64_t val;
  if (sh >= 0) {
    if (sh > 12) return sig ? 31u : 0u;  // sig >= 1: 8y >= 2^13 > 60
    val = sig << (32 + sh);
  } else {
    const int rs = -sh;
    if (rs >= 40) val = sig ? 1u : 0u;
    else val = ((sig << 32) >> rs) | ((((sig << 32) & ((1ull << rs) - 1ull)) != 0) ? 1ull : 0ull);
  }
  if (val >= (60ull << 32)) return 31u;
  uint64_t off, step;
  uint32_t base;
  if (val < (16ull << 32)) off = 0, step = 1, base = 0;
  else if (val < (32ull << 32)) off = 16, step = 2, base = 16;
  else off = 32, step = 4, base = 24;
  const uint64_t r = val - (off << 32), unit = step << 32, half = unit >> 1;
  uint32_t k = uint32_t(r / unit);
  const uint64_t rem = r % unit;
  if (rem > half || (rem == half && (k & 1u))) ++k;
  return base + k;
}

// One code (low 6 bits) times 2^(sb - 127) as bf16 bits, in integer arithmetic.
__device__ static uint32_t bf16_bits6(uint32_t code, uint32_t sb) {
  if (sb == 0xFFu) return 0x7FC0u;
  const uint32_t m = code & 31u, sign = (code & 32u) << 10;
  if (m == 0) return sign;
  int ee;
  uint32_t mant;
  if (m < 8) {  // m / 8: normalize on its top bit h
    const int h = m >= 4 ? 2 : m >= 2 ? 1 : 0;
    ee = int(sb) - 3 + h;
    mant = (m << (7 - h)) & 0x7Fu;
  } else {
    ee = int(sb) + int(m >> 3) - 1;
    mant = (m & 7u) << 4;
  }
  if (ee >= 255) return sign | 0x7F80u;
  if (ee >= 1) return sign | (uint32_t(ee) << 7) | mant;
  return sign | ((0x80u | mant) >> (1 - ee));  // subnormal: exact (at most 4 bits shifted out, the lowest set bit is bit 4)
}

__device__ static uint32_t code_at(const dissem::kern::mxfp6_u32x6_t& c, int i) {
  const int bit = 6 * i, d = bit >> 5, sh = bit & 31;
  uint64_t v = c[d];
  if (d + 1 < 6) v |= uint64_t(c[d + 1]) << 32;
  return uint32_t(v >> sh) & 63u;
}

// blockIdx.y = E + 126; thread t converts the bf16 patterns 32 t .. 32 t + 31 (element i = pattern 32 t + i)
__global__ void fp6_pack_probe(unsigned long long* cnt, uint32_t* first_bad) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;  // 0..2047
  const int e = int(blockIdx.y) - 126;
  const float s = __uint_as_float(uint32_t(e + 127) << 23);
  dissem::kern::mxfp6_u32x16_t x;
  for (int i = 0; i < 16; ++i) x[i] = (32u * t + 2u * i) | ((32u * t + 2u * i + 1u) << 16);
  const dissem::kern::mxfp6_u32x6_t r = dissem::kern::mxfp6_cvt_pack_raw(x, s);
  // 7.5 * 2^e = 1.875 * 2^(e + 2): bf16 bits (e + 129) << 7 | 0x70
  const uint32_t lim = (uint32_t(e + 129) << 7) | 0x70u;
  for (int i = 0; i < 32; ++i) {
    const uint32_t p = 32u * t + uint32_t(i), a = p & 0x7FFFu;
    int cls;
    uint32_t want;
    if (a > 0x7F80u) {
      cls = kNan, want = 31;  // no reference: counted as "mismatch" unless it saturates
    } else if (a == 0x7F80u) {
      cls = kInf, want = 31;
    } else if (a > lim) {
      cls = kAbove, want = 31;
    } else {
      want = quant6_bits(a, e);
      const uint32_t up = quant6_bits(a + 1 <= lim ? a + 1 : a, e);
      const uint32_t dn = quant6_bits(a ? a - 1 : 0, e);
      cls = a == 0 ? kZero : (a < 0x80u ? kInRangeSub : ((up != want) != (dn != want) && up != dn ? kTie : kInRange));
    }
    const uint32_t got = code_at(r, i);
    atomicAdd(&cnt[2 * cls], 1ull);
    if (got != (want | ((p >> 10) & 32u))) {
      if (atomicAdd(&cnt[2 * cls + 1], 1ull) == 0) {
        first_bad[3 * cls] = p;
        first_bad[3 * cls + 1] = uint32_t(e);
        first_bad[3 * cls + 2] = got;
      }
    }
  }
}

// Layout of the 6-dword operand: thread i packs a block whose element i is 1.0
// (code 8 at E = 0) and every other element 0; out[6 i .. 6 i + 5] = the raw dwords.
__global__ void fp6_layout_probe(uint32_t* out) {
  const int i = threadIdx.x;
  if (i >= 32) return;
  dissem::kern::mxfp6_u32x16_t x;
  for (int k = 0; k < 16; ++k) x[k] = k == (i >> 1) ? ((i & 1) ? 0x3F800000u : 0x00003F80u) : 0u;
  const dissem::kern::mxfp6_u32x6_t r = dissem::kern::mxfp6_cvt_pack_raw(x, 1.0f);
  for (int d = 0; d < 6; ++d) out[6 * i + d] = r[d];
}

// blockIdx.y = scale byte; thread = (code c, position p): element j of the block holds code (c + j - p) & 63
__global__ void fp6_unpack_probe(unsigned long long* bad_by_scale, uint32_t* first_bad) {
  const uint32_t sb = blockIdx.y, t = blockIdx.x * blockDim.x + threadIdx.x;  // t = 0..2047
  const uint32_t c = t >> 5, p = t & 31u;
  const float s = __uint_as_float(sb << 23);
  uint32_t w[7] = {0, 0, 0, 0, 0, 0, 0};
  for (uint32_t j = 0; j < 32; ++j) {
    const uint64_t code = (c + j - p) & 63u;
    const uint32_t bit = 6 * j, d = bit >> 5, sh = bit & 31u;
    w[d] |= uint32_t(code << sh);
    w[d + 1] |= uint32_t((code << sh) >> 32);
  }
  const dissem::kern::mxfp6_u32x16_t o =
      dissem::kern::mxfp6_cvt_unpack_raw(dissem::kern::mxfp6_u32x6_t{w[0], w[1], w[2], w[3], w[4], w[5]}, s);
  for (uint32_t j = 0; j < 32; ++j) {
    const uint32_t code = (c + j - p) & 63u;
    const uint32_t got = (o[j >> 1] >> (16 * (j & 1u))) & 0xFFFFu;
    if (got != bf16_bits6(code, sb) && atomicAdd(&bad_by_scale[sb], 1ull) == 0) {
      first_bad[3 * sb] = code;
      first_bad[3 * sb + 1] = j;
      first_bad[3 * sb + 2] = got;
    }
  }
}

static void mxfp6_probe() {
  unsigned long long *cnt, *ubad;
  uint32_t *pfirst, *ufirst, *lay;
  hipMalloc(&cnt, 2 * kPackClasses * 8);
  hipMalloc(&pfirst, 3 * kPackClasses * 4);
  hipMalloc(&ubad, 256 * 8);
  hipMalloc(&ufirst, 768 * 4);
  hipMalloc(&lay, 192 * 4);
  hipMemset(cnt, 0, 2 * kPackClasses * 8);
  hipMemset(pfirst, 0, 3 * kPackClasses * 4);
  hipMemset(ubad, 0, 256 * 8);
  hipMemset(ufirst, 0, 768 * 4);
  hipMemset(lay, 0, 192 * 4);
  fp6_pack_probe<<<dim3(8, 252), 256>>>(cnt, pfirst);
  fp6_layout_probe<<<1, 64>>>(lay);
  fp6_unpack_probe<<<dim3(8, 256), 256>>>(ubad, ufirst);
  unsigned long long hc[2 * kPackClasses], hu[256];
  uint32_t hp[3 * kPackClasses], hf[768], hl[192];
  hipMemcpy(hc, cnt, sizeof hc, hipMemcpyDeviceToHost);
  hipMemcpy(hp, pfirst, sizeof hp, hipMemcpyDeviceToHost);
  hipMemcpy(hu, ubad, sizeof hu, hipMemcpyDeviceToHost);
  hipMemcpy(hf, ufirst, sizeof hf, hipMemcpyDeviceToHost);
  hipMemcpy(hl, lay, sizeof hl, hipMemcpyDeviceToHost);
  static const char* kPackClass6[] = {"in_range_normal", "in_range_bf16_subnormal", "code_boundary", "zero",
                                      "above_7.5x2^E_finite", "inf", "nan"};
  for (int c = 0; c < kPackClasses; ++c)
    printf("{\"op\": \"fp6_pack\", \"class\": \"%s\", \"inputs\": %llu, \"mismatches\": %llu, "
           "\"first\": {\"bf16\": \"0x%04x\", \"E\": %d, \"got\": \"0x%02x\"}}\n",
           kPackClass6[c], hc[2 * c], hc[2 * c + 1], hp[3 * c], int(hp[3 * c + 1]), hp[3 * c + 2]);
  // element i = 1.0: code 8 at bits [6 i, 6 i + 6) of the dwords as one little-endian integer, nothing else set
  int lay_bad = 0, first_lay = -1;
  for (int i = 0; i < 32; ++i) {
    uint32_t want[7] = {0, 0, 0, 0, 0, 0, 0};
    const int bit = 6 * i, d = bit >> 5, sh = bit & 31;
    want[d] |= uint32_t(8ull << sh);
    want[d + 1] |= uint32_t((8ull << sh) >> 32);
    if (memcmp(want, hl + 6 * i, 24) != 0) {
      ++lay_bad;
      if (first_lay < 0) first_lay = i;
    }
  }
  printf("{\"op\": \"fp6_pack_layout\", \"positions\": 32, \"mismatches\": %d, \"first_position\": %d, "
         "\"position_1_dwords\": [\"0x%08x\", \"0x%08x\", \"0x%08x\", \"0x%08x\", \"0x%08x\", \"0x%08x\"]}\n",
         lay_bad, first_lay, hl[6], hl[7], hl[8], hl[9], hl[10], hl[11]);
  unsigned long long mid = 0;
  for (int sb = 2; sb <= 252; ++sb) mid += hu[sb];
  printf("{\"op\": \"fp6_unpack\", \"scale_bytes\": \"2..252\", \"elements_per_scale_byte\": 65536, "
         "\"mismatches\": %llu}\n", mid);
  for (int sb : {0, 1, 253, 254, 255})
    printf("{\"op\": \"fp6_unpack\", \"scale_bytes\": \"%d\", \"mismatches\": %llu, \"first\": "
           "{\"code\": \"0x%02x\", \"position\": %u, \"got\": \"0x%04x\"}}\n", sb, hu[sb], hf[3 * sb], hf[3 * sb + 1],
           hf[3 * sb + 2]);
}

static float bf16f(uint16_t b) {
  uint32_t u = uint32_t(b) << 16;
  float f;
  memcpy(&f, &u, 4);
  return f;
}
static uint16_t fbf16(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  return uint16_t(u >> 16);
}

int main() {
  // fp8 e4m3fn codes: 0x38 = 1.0, 0x40 = 2.0, 0x7E = 448, 0x01 = 2^-9 (subnormal)
  const int n = 8;
  int codes[n] = {0x3838, 0x4038, 0x7E38, 0x0138, 0x3838, 0x3838, 0x3838, 0x3838};
  float scales[n] = {1.0f, 1.0f, 1.0f, 1.0f, 3.0f, 0.75f, 1024.0f, 1.5f};
  int *dc;
  float* ds;
  uint32_t* dout;
  hipMalloc(&dc, sizeof codes);
  hipMalloc(&ds, sizeof scales);
  hipMalloc(&dout, n * 4);
  hipMemcpy(dc, codes, sizeof codes, hipMemcpyHostToDevice);
  hipMemcpy(ds, scales, sizeof scales, hipMemcpyHostToDevice);
  unpack_probe<<<1, 64>>>(dc, ds, n, dout);
  uint32_t out[n];
  hipMemcpy(out, dout, sizeof out, hipMemcpyDeviceToHost);
  for (int i = 0; i < n; ++i)
    printf("{\"op\": \"unpack\", \"codes\": \"0x%04x\", \"scale\": %g, \"lo\": %g, \"hi\": %g}\n", codes[i] & 0xFFFF,
           scales[i], bf16f(uint16_t(out[i] & 0xFFFF)), bf16f(uint16_t(out[i] >> 16)));
  uint32_t pairs[n];
  float vals[n][2] = {{1.0f, 2.0f}, {448.0f, -448.0f}, {3.0f, 5.0f}, {1000.0f, 0.1f},
                      {1.0f, 2.0f}, {1.0f, 2.0f}, {1.0f, 2.0f}, {1.0f, 2.0f}};
  float pscales[n] = {1.0f, 1.0f, 1.0f, 1.0f, 2.0f, 3.0f, 0.5f, 1.5f};
  for (int i = 0; i < n; ++i) pairs[i] = uint32_t(fbf16(vals[i][0])) | (uint32_t(fbf16(vals[i][1])) << 16);
  uint32_t* dp;
  hipMalloc(&dp, sizeof pairs);
  hipMemcpy(dp, pairs, sizeof pairs, hipMemcpyHostToDevice);
  hipMemcpy(ds, pscales, sizeof pscales, hipMemcpyHostToDevice);
  pack_probe<<<1, 64>>>(dp, ds, n, dout);
  hipMemcpy(out, dout, sizeof out, hipMemcpyDeviceToHost);
  for (int i = 0; i < n; ++i)
    printf("{\"op\": \"pack\", \"in\": [%g, %g], \"scale\": %g, \"codes\": \"0x%04x\"}\n", vals[i][0], vals[i][1],
           pscales[i], out[i] & 0xFFFF);
  mxfp4_probe();
  mxfp6_probe();
  return hipDeviceSynchronize() == hipSuccess ? 0 : 1;
}
