// Device code shared by the kernels that feed v_mfma_f32_16x16x32_bf16 from an
// fp8-packed layer in place (fp8_linear.hip, fp8_swiglu.hip): a lane's place in
// the chunked layout of core/fp8.h and the conversion of 8 codes into a B
// fragment. The fragment cast and the store of one result are mxfp4_mma.h's.
// Everything here has internal linkage.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels/fp8_cvt.h"
#include "kernels/mxfp4_mma.h"

namespace dissem {
namespace kern {
namespace {

struct Fp8Layout {
  const uint8_t* packed;
  int64_t pchunk;  // bytes of a full packed chunk
  int64_t full;    // full chunks of the layer
  int celem;       // elements of a full chunk
  int telem;       // elements of the tail chunk (0: none)
  int shift;       // log2 of the scale block
};

// One lane's place in the packed layer, in elements (always on the 32-element grid).
struct ElemPos {
  const uint8_t* base;  // the chunk
  int64_t c;            // its index
  int r;                // element within the chunk
  int nelem;            // elements of the chunk: as many bytes of codes, the scales follow
  __device__ __forceinline__ void init(const Fp8Layout& L, int64_t elem) {
    c = elem / L.celem;
    r = int(elem - c * L.celem);
    base = L.packed + c * L.pchunk;
    nelem = c < L.full ? L.celem : L.telem;
  }
  // d <= 128 elements forward. Past the end of the layer the position is
  // meaningless; the callers never read through such a position.
  __device__ __forceinline__ void advance(const Fp8Layout& L, int d) {
    r += d;
    if (r >= nelem) {
      r -= nelem;
      ++c;
      base += L.pchunk;
      nelem = c < L.full ? L.celem : L.telem;
    }
  }
  __device__ __forceinline__ const uint8_t* q() const { return base + r; }
  __device__ __forceinline__ float scale(const Fp8Layout& L) const {
    return *reinterpret_cast<const float*>(base + nelem + (int64_t(r >> L.shift) << 2));
  }
};

// 8 codes (two dwords) times the scale -> a B fragment
__device__ __forceinline__ bf16x8_t fp8_frag(uint32_t w0, uint32_t w1, float s) {
  const uint32_t o[4] = {fp8x2_to_bf16x2<false>(w0, s), fp8x2_to_bf16x2<true>(w0, s), fp8x2_to_bf16x2<false>(w1, s),
                         fp8x2_to_bf16x2<true>(w1, s)};
  return as_frag(o);
}

}  // namespace
}  // namespace kern
}  // namespace dissem
