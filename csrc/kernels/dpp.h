// gfx950 cross-lane reductions shared by the pack kernels (fp8.hip, mxfp4.hip).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace dissem {
namespace kern {

template <int CTRL>
__device__ __forceinline__ float dpp_f(float v) {
  return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), CTRL, 0xF, 0xF, false));
}

// Max over each aligned group of LANES lanes (4..64), result in every lane of
// the group, without LDS: DPP quad swaps and half-row / row mirrors inside a
// row of 16, then v_permlane16_swap / v_permlane32_swap of a value with itself
// across rows (replaces __shfl_xor's ds_bpermute + address math per step).
template <int LANES>
__device__ __forceinline__ float group_max(float v) {
  v = fmaxf(v, dpp_f<0xB1>(v));                      // quad_perm [1,0,3,2]
  v = fmaxf(v, dpp_f<0x4E>(v));                      // quad_perm [2,3,0,1]
  if constexpr (LANES >= 8) v = fmaxf(v, dpp_f<0x141>(v));   // row_half_mirror
  if constexpr (LANES >= 16) v = fmaxf(v, dpp_f<0x140>(v));  // row_mirror
  if constexpr (LANES >= 32) {
    const auto p = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    v = fmaxf(__uint_as_float(p[0]), __uint_as_float(p[1]));
  }
  if constexpr (LANES >= 64) {
    const auto p = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    v = fmaxf(__uint_as_float(p[0]), __uint_as_float(p[1]));
  }
  return v;
}

}  // namespace kern
}  // namespace dissem
