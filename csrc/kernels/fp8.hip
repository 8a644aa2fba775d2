// bf16 <-> OCP fp8 e4m3fn block-scaled pack/unpack (BASELINE config #5: the
// 405B-sized run ships layers as fp8 on the wire to halve xGMI bytes).
//
// OCP e4m3fn encoding (CDNA4's, not MI300's fnuz). One power-of-two scale 2^E
// per `block` elements (core/fp8.h: the smallest E with amax <= 448 * 2^E over
// the block's finite values), stored as f32. Pack scales by the exact 2^-E and
// converts with v_cvt_pk_fp8_f32 (+-inf saturate to +-448 - 240 in the top
// binade, core/fp8.h sat_limit - and NaN stays NaN, 0x7F with the input's
// sign - random bf16 payload bit patterns contain both); unpack is
// v_cvt_scalef32_pk_bf16_fp8: fp8 pair -> scaled bf16 pair in one instruction
// (the scale's exponent is applied and the product rounded to bf16, core/fp8.h),
// where the f32 path took 4 VALU per pair (convert, 2 multiplies, pack to bf16).
//
// Each thread moves 8 elements: a 16-B bf16 load and an 8-B fp8 store (pack),
// or the reverse (unpack). A block of `block` elements is handled by
// block/8 adjacent lanes that reduce the amax with DPP / permlane swaps.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kernels/dpp.h"
#include "kernels/fp8_cvt.h"
#include "kernels/kernels.h"

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

template <int LANES>  // lanes per scale block (block / 8)
__global__ void __launch_bounds__(256) fp8_pack_kernel(const uint4* __restrict__ in, int64_t nthreads,
                                                       uint2* __restrict__ out, float* __restrict__ scales) {
  const int64_t t = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  const bool active = t < nthreads;
  uint4 v = active ? in[t] : make_uint4(0, 0, 0, 0);
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
  if (!active) return;
  // written once, read by a later pass or another GPU: nontemporal (profiles/r4_nt)
  using v2 = unsigned int __attribute__((ext_vector_type(2)));
  __builtin_nontemporal_store(v2{uint32_t(lo), uint32_t(hi)}, reinterpret_cast<v2*>(out) + t);
  if ((threadIdx.x % LANES) == 0) scales[t / LANES] = __uint_as_float(uint32_t(127 + e) << 23);
}

template <int LANES>
__global__ void __launch_bounds__(256) fp8_unpack_kernel(const uint2* __restrict__ in,
                                                         const float* __restrict__ scales, int64_t nthreads,
                                                         uint4* __restrict__ out) {
  const int64_t t = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (t >= nthreads) return;
  const uint2 q = in[t];
  const float s = scales[t / LANES];
  using v4 = unsigned int __attribute__((ext_vector_type(4)));
  __builtin_nontemporal_store(v4{fp8x2_to_bf16x2<false>(q.x, s), fp8x2_to_bf16x2<true>(q.x, s),
                                 fp8x2_to_bf16x2<false>(q.y, s), fp8x2_to_bf16x2<true>(q.y, s)},
                              reinterpret_cast<v4*>(out) + t);
}

}  // namespace

hipError_t fp8_pack(const uint16_t* bf16, int64_t n, uint8_t* fp8, float* scales, int block, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  if (n % block || (reinterpret_cast<uintptr_t>(bf16) & 15) || (reinterpret_cast<uintptr_t>(fp8) & 7))
    return hipErrorInvalidValue;
  const int64_t nt = n / 8;
  const unsigned grid = unsigned((nt + 255) / 256);
  auto* in = reinterpret_cast<const uint4*>(bf16);
  auto* out = reinterpret_cast<uint2*>(fp8);
  switch (block) {
    case 32: fp8_pack_kernel<4><<<grid, 256, 0, s>>>(in, nt, out, scales); break;
    case 64: fp8_pack_kernel<8><<<grid, 256, 0, s>>>(in, nt, out, scales); break;
    case 128: fp8_pack_kernel<16><<<grid, 256, 0, s>>>(in, nt, out, scales); break;
    case 256: fp8_pack_kernel<32><<<grid, 256, 0, s>>>(in, nt, out, scales); break;
    case 512: fp8_pack_kernel<64><<<grid, 256, 0, s>>>(in, nt, out, scales); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t fp8_unpack(const uint8_t* fp8, const float* scales, int64_t n, uint16_t* bf16, int block, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  if (n % block || (reinterpret_cast<uintptr_t>(bf16) & 15) || (reinterpret_cast<uintptr_t>(fp8) & 7))
    return hipErrorInvalidValue;
  const int64_t nt = n / 8;
  const unsigned grid = unsigned((nt + 255) / 256);
  auto* in = reinterpret_cast<const uint2*>(fp8);
  auto* out = reinterpret_cast<uint4*>(bf16);
  switch (block) {
    case 32: fp8_unpack_kernel<4><<<grid, 256, 0, s>>>(in, scales, nt, out); break;
    case 64: fp8_unpack_kernel<8><<<grid, 256, 0, s>>>(in, scales, nt, out); break;
    case 128: fp8_unpack_kernel<16><<<grid, 256, 0, s>>>(in, scales, nt, out); break;
    case 256: fp8_unpack_kernel<32><<<grid, 256, 0, s>>>(in, scales, nt, out); break;
    case 512: fp8_unpack_kernel<64><<<grid, 256, 0, s>>>(in, scales, nt, out); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t fp8_pack_chunks(const void* src, int64_t src_bytes, int64_t src_chunk, int block, void* dst,
                           hipStream_t s) {
  if (src_chunk <= 0 || src_chunk % (2 * block) || src_bytes % (2 * block)) return hipErrorInvalidValue;
  const int64_t pchunk = src_chunk / 2 + src_chunk / 2 / block * 4;
  for (int64_t off = 0, c = 0; off < src_bytes; off += src_chunk, ++c) {
    const int64_t n = std::min(src_chunk, src_bytes - off) / 2;
    uint8_t* out = static_cast<uint8_t*>(dst) + c * pchunk;
    hipError_t e = fp8_pack(reinterpret_cast<const uint16_t*>(static_cast<const uint8_t*>(src) + off), n, out,
                            reinterpret_cast<float*>(out + n), block, s);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace kern
}  // namespace dissem
