// bf16 activations -> MXFP8 (core/mxfp8_act.h): e4m3fn codes and one E8M0 scale
// byte per 32 values along K, the A operand of the W4A8 linears (mxfp4_mx.hip).
// Rows are contiguous and K is a multiple of 32, so [M, K] is M * K / 32 blocks
// in a row: the kernel is fp8.hip's pack kernel at block = 32 (kernels/fp8_pack.h,
// the same scale and the same codes, byte for byte the host codec on every
// input) with the scale stored as its exponent byte. A thread moves 8 values - a
// 16-B load, an 8-B store - and four adjacent lanes share a block; one launch
// for any M. The codes are read again at once by the matmul, so the stores are
// plain ones.
#include <hip/hip_runtime.h>

#include "kernels/fp8_pack.h"
#include "kernels/kernels.h"

namespace dissem {
namespace kern {

namespace {

__global__ void __launch_bounds__(256) mxfp8_quantize_kernel(const uint4* __restrict__ in, int64_t nthreads,
                                                             uint2* __restrict__ codes, uint8_t* __restrict__ scales) {
  const int64_t t = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  const bool active = t < nthreads;
  const uint4 v = active ? in[t] : make_uint4(0, 0, 0, 0);
  int e;
  const uint2 q = fp8_pack8<4>(v, e);
  if (!active) return;
  codes[t] = q;
  if ((threadIdx.x & 3) == 0) scales[t >> 2] = uint8_t(127 + e);
}

}  // namespace

hipError_t mxfp8_quantize_rows(const uint16_t* x, int64_t M, int64_t K, uint8_t* codes, uint8_t* scales,
                               hipStream_t s) {
  if (M < 1 || K < 32 || K % 32 || M > INT64_MAX / K) return hipErrorInvalidValue;
  if ((reinterpret_cast<uintptr_t>(x) & 15) || (reinterpret_cast<uintptr_t>(codes) & 7)) return hipErrorInvalidValue;
  const int64_t nt = M * K / 8, grid = (nt + 255) / 256;
  if (grid > 0x7FFFFFFF) return hipErrorInvalidValue;
  mxfp8_quantize_kernel<<<unsigned(grid), 256, 0, s>>>(reinterpret_cast<const uint4*>(x), nt,
                                                       reinterpret_cast<uint2*>(codes), scales);
  return hipGetLastError();
}

}  // namespace kern
}  // namespace dissem
