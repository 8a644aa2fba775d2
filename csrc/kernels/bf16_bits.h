// The one bf16 -> f32 widening of the device code, for the headers that used to
// carry a copy each (fp8_pack.h, attn_mma.h) and can now meet in one file.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace dissem {
namespace kern {
namespace {

__device__ __forceinline__ float bf16_to_f32(uint16_t h) { return __uint_as_float(uint32_t(h) << 16); }

}  // namespace
}  // namespace kern
}  // namespace dissem
