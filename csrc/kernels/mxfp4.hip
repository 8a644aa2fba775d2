// bf16 <-> MXFP4 (OCP e2m1 codes, one E8M0 scale byte per 32 elements)
// pack/unpack in the layout of core/mxfp4.h, bit-exact with its host reference.
//
// Shape of fp8.hip: each thread moves 8 elements - a 16-B bf16 load and a 4-B
// store of 8 codes (pack), or the reverse (unpack). A scale block of 32
// elements is 4 adjacent lanes, which reduce the block's amax with the DPP
// group_max<4>; the block's first lane writes the scale byte with an ordinary
// vector byte store. Stores are nontemporal (written once, read by a later
// pass or another GPU).
//
// Pack works on the bf16 bits, two per register: a block's finite amax and its
// NaN flag come from packed 16-bit integer arithmetic (the bits of |x| order
// like the values), the scale exponent from core/mxfp4.h's integer rule, and
// the codes from v_cvt_scalef32_pk_fp4_bf16: two bf16 and the scale 2^E -> two
// e2m1 codes in one byte of the destination.
//
// The converters against core/mxfp4.h, measured on MI355X for every bf16
// pattern at every scale 2^E, E in [-126, 125], and every (code byte, scale
// byte) pair (bin/cvtprobe, profiles/mxfp4/cvtprobe.jsonl):
//   * finite values up to 6 * 2^E: nearest code, ties to the even code, sign
//     kept (-0 and values that round to 0 included), bf16 subnormals exact -
//     the converter is used as it is;
//   * values above 6 * 2^E (a block whose E is capped at 125) and +-inf: the
//     converter saturates to +-6, which is the reference's clamp - used as it is;
//   * NaN: e2m1 has none, the converter saturates it to +-6. The reference
//     marks the whole block instead, so the kernel finds NaNs in the bit domain
//     and writes 16 zero bytes and scale byte 0xFF: the only case in plain code;
//   * unpack: exact for scale bytes 0..254, bf16-subnormal results and overflow
//     to inf included; for 0xFF the converter's NaN carries the code's sign
//     (0xFFC0) where the reference fixes 0x7FC0: that byte's result is a
//     constant, selected instead of converted (mxfp4_cvt.h).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kernels/dpp.h"
#include "kernels/kernels.h"
#include "kernels/mxfp4_cvt.h"

namespace dissem {
namespace kern {

namespace {

typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
typedef unsigned short u16x2_t __attribute__((ext_vector_type(2)));

__device__ __forceinline__ uint32_t pk_max_u16(uint32_t a, uint32_t b) {
  return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(u16x2_t, a),
                                                                 __builtin_bit_cast(u16x2_t, b)));
}

__global__ void __launch_bounds__(256) mxfp4_pack_kernel(const uint4* __restrict__ in, int64_t nthreads,
                                                         uint32_t* __restrict__ q, uint8_t* __restrict__ scales) {
  const int64_t t = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  const bool active = t < nthreads;
  const uint4 v = active ? in[t] : make_uint4(0, 0, 0, 0);
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
  uint32_t fmax2 = 0, nanacc = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const uint32_t a = w[i] & 0x7FFF7FFFu;
    // per half: 1 where |x| >= 0x7F80 (inf or NaN): those do not count for amax
    const uint32_t nf = ((a + 0x00800080u) >> 15) & 0x00010001u;
    fmax2 = pk_max_u16(fmax2, a & ~(nf * 0xFFFFu));
    nanacc |= a + 0x007F007Fu;  // bit 15 of a half: |x| > 0x7F80, a NaN
  }
  const uint32_t amax16 = max(fmax2 & 0xFFFFu, fmax2 >> 16);
  // reduced over the block's 4 lanes as a small integer-valued float (exact,
  // and independent of the f32 denormal mode); 65535 marks a NaN
  const float red = group_max<4>((nanacc & 0x80008000u) ? 65535.0f : float(amax16));
  const bool nan = red == 65535.0f;
  const int e = mxfp4_scale_exp(uint32_t(red));
  const float s = __uint_as_float(uint32_t(e + 127) << 23);  // 2^e, e in [-126, 125]
  uint32_t r = 0;
  r = __builtin_amdgcn_cvt_scalef32_pk_fp4_bf16(r, __builtin_bit_cast(bf16x2_t, w[0]), s, 0);
  r = __builtin_amdgcn_cvt_scalef32_pk_fp4_bf16(r, __builtin_bit_cast(bf16x2_t, w[1]), s, 1);
  r = __builtin_amdgcn_cvt_scalef32_pk_fp4_bf16(r, __builtin_bit_cast(bf16x2_t, w[2]), s, 2);
  r = __builtin_amdgcn_cvt_scalef32_pk_fp4_bf16(r, __builtin_bit_cast(bf16x2_t, w[3]), s, 3);
  if (!active) return;
  __builtin_nontemporal_store(nan ? 0u : r, q + t);
  if ((threadIdx.x & 3) == 0) scales[t >> 2] = nan ? uint8_t(0xFF) : uint8_t(e + 127);
}

// Two groups of 8 codes per thread, 256 threads apart: both 4-B loads are in
// flight before the first store, and every store instruction of a wave still
// writes 1 KiB of contiguous bf16.
__global__ void __launch_bounds__(256) mxfp4_unpack_kernel(const uint32_t* __restrict__ q,
                                                           const uint8_t* __restrict__ scales, int64_t nthreads,
                                                           uint4* __restrict__ out) {
  const int64_t t0 = int64_t(blockIdx.x) * 512 + threadIdx.x, t1 = t0 + 256;
  if (t0 >= nthreads) return;
  const bool two = t1 < nthreads;
  const uint32_t w0 = q[t0], w1 = two ? q[t1] : 0u;
  const uint32_t s0 = scales[t0 >> 2], s1 = two ? scales[t1 >> 2] : 0u;
  using v4 = unsigned int __attribute__((ext_vector_type(4)));
  uint32_t o[4];
  mxfp4_unpack8(w0, s0, o);
  __builtin_nontemporal_store(v4{o[0], o[1], o[2], o[3]}, reinterpret_cast<v4*>(out) + t0);
  if (!two) return;
  mxfp4_unpack8(w1, s1, o);
  __builtin_nontemporal_store(v4{o[0], o[1], o[2], o[3]}, reinterpret_cast<v4*>(out) + t1);
}

}  // namespace

hipError_t mxfp4_pack(const uint16_t* bf16, int64_t n, uint8_t* q, uint8_t* scales, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  if (n % 32 || (reinterpret_cast<uintptr_t>(bf16) & 15) || (reinterpret_cast<uintptr_t>(q) & 3))
    return hipErrorInvalidValue;
  const int64_t nt = n / 8;
  if ((nt + 255) / 256 > 0x7FFFFFFF) return hipErrorInvalidValue;
  mxfp4_pack_kernel<<<unsigned((nt + 255) / 256), 256, 0, s>>>(reinterpret_cast<const uint4*>(bf16), nt,
                                                                reinterpret_cast<uint32_t*>(q), scales);
  return hipGetLastError();
}

hipError_t mxfp4_unpack(const uint8_t* q, const uint8_t* scales, int64_t n, uint16_t* bf16, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  if (n % 32 || (reinterpret_cast<uintptr_t>(bf16) & 15) || (reinterpret_cast<uintptr_t>(q) & 3))
    return hipErrorInvalidValue;
  const int64_t nt = n / 8;
  if ((nt + 511) / 512 > 0x7FFFFFFF) return hipErrorInvalidValue;
  mxfp4_unpack_kernel<<<unsigned((nt + 511) / 512), 256, 0, s>>>(reinterpret_cast<const uint32_t*>(q), scales, nt,
                                                                  reinterpret_cast<uint4*>(bf16));
  return hipGetLastError();
}

hipError_t mxfp4_pack_chunks(const void* src, int64_t src_bytes, int64_t src_chunk, void* dst, hipStream_t s) {
  if (src_chunk <= 0 || src_chunk % 1024 || src_bytes % 64) return hipErrorInvalidValue;
  const int64_t pchunk = src_chunk / 4 + src_chunk / 64;
  for (int64_t off = 0, c = 0; off < src_bytes; off += src_chunk, ++c) {
    const int64_t n = std::min(src_chunk, src_bytes - off) / 2;
    uint8_t* out = static_cast<uint8_t*>(dst) + c * pchunk;
    hipError_t e = mxfp4_pack(reinterpret_cast<const uint16_t*>(static_cast<const uint8_t*>(src) + off), n, out,
                              out + n / 2, s);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace kern
}  // namespace dissem
