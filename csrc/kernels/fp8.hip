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

#include "kernels/fp8_cvt.h"
#include "kernels/fp8_pack.h"
#include "kernels/kernels.h"

namespace dissem {
namespace kern {

namespace {

template <int LANES>  // lanes per scale block (block / 8)
__global__ void __launch_bounds__(256) fp8_pack_kernel(const uint4* __restrict__ in, int64_t nthreads,
                                                       uint2* __restrict__ out, float* __restrict__ scales) {
  const int64_t t = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  const bool active = t < nthreads;
  const uint4 v = active ? in[t] : make_uint4(0, 0, 0, 0);
  int e;
  const uint2 q = fp8_pack8<LANES>(v, e);
  if (!active) return;
  // written once, read by a later pass or another GPU: nontemporal (profiles/r4_nt)
  using v2 = unsigned int __attribute__((ext_vector_type(2)));
  __builtin_nontemporal_store(v2{q.x, q.y}, reinterpret_cast<v2*>(out) + t);
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
