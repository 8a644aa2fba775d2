// Device code shared by the kernels that feed v_mfma_f32_16x16x32_bf16 from an
// MXFP4-packed layer in place (mxfp4_linear.hip, mxfp4_swiglu.hip): a lane's
// place in the chunked layout of core/mxfp4.h, the fragment cast and the store
// of one result; the last two and the swiglu epilogue also serve the fp8 and
// MXFP6 kernels (fp8_mma.h, mxfp6_mma.h). Everything here has internal linkage.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace dissem {
namespace kern {
namespace {

typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef float f32x4_t __attribute__((ext_vector_type(4)));
typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));

struct Mxfp4Layout {
  const uint8_t* packed;
  int64_t pchunk;  // bytes of a full packed chunk
  int64_t full;    // full chunks of the layer
  int cblk;        // scale blocks of a full chunk
  int tblk;        // scale blocks of the tail chunk (0: none)
};

// One lane's place in the packed layer, in scale blocks.
struct BlockPos {
  const uint8_t* base;  // the chunk
  int64_t c;            // its index
  int r;                // block within the chunk
  int nblk;             // blocks of the chunk: q is 16 * nblk bytes, the scales follow
  __device__ __forceinline__ void init(const Mxfp4Layout& L, int64_t block) {
    c = block / L.cblk;
    r = int(block - c * L.cblk);
    base = L.packed + c * L.pchunk;
    nblk = c < L.full ? L.cblk : L.tblk;
  }
  // d <= 16 blocks forward. Past the end of the layer the position is
  // meaningless; the callers never read through such a position.
  __device__ __forceinline__ void advance(const Mxfp4Layout& L, int d) {
    r += d;
    if (r >= nblk) {
      r -= nblk;
      ++c;
      base += L.pchunk;
      nblk = c < L.full ? L.cblk : L.tblk;
    }
  }
  __device__ __forceinline__ const uint8_t* q() const { return base + int64_t(r) * 16; }
  __device__ __forceinline__ uint32_t scale() const { return base[int64_t(nblk) * 16 + r]; }
};

__device__ __forceinline__ bf16x8_t as_frag(const uint32_t (&o)[4]) {
  return __builtin_bit_cast(bf16x8_t, u32x4_t{o[0], o[1], o[2], o[3]});
}

__device__ __forceinline__ uint16_t f32_to_bf16_rne(float f) {
  const uint32_t u = __float_as_uint(f);
  if ((u & 0x7FFFFFFFu) > 0x7F800000u) return 0x7FC0;
  return uint16_t((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}

template <bool BF16>
__device__ __forceinline__ void store_y(void* y, int64_t idx, float v) {
  if (BF16) static_cast<uint16_t*>(y)[idx] = f32_to_bf16_rne(v);
  else static_cast<float*>(y)[idx] = v;
}

// The epilogue of the *_swiglu kernels on the f32 sums g and u: silu(g) * u.
__device__ __forceinline__ float swiglu(float g, float u) { return (g / (1.0f + expf(-g))) * u; }

// The layout of a layer of `src_bytes` bf16 bytes packed in chunks of `src_chunk`.
inline Mxfp4Layout mxfp4_layout(const void* packed, int64_t src_bytes, int64_t src_chunk) {
  Mxfp4Layout L;
  L.packed = static_cast<const uint8_t*>(packed);
  L.pchunk = src_chunk / 4 + src_chunk / 64;
  L.full = src_bytes / src_chunk;
  L.cblk = int(src_chunk / 64);
  L.tblk = int(src_bytes % src_chunk / 64);
  return L;
}

}  // namespace
}  // namespace kern
}  // namespace dissem
