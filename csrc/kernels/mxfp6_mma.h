// Device code shared by the kernels that feed v_mfma_f32_16x16x32_bf16 from an
// MXFP6-packed layer in place (mxfp6_linear.hip, mxfp6_swiglu.hip): a lane's
// place in the chunked layout of core/mxfp6.h and the layout of a layer. The
// fragment cast and the store of one result are mxfp4_mma.h's. Everything here
// has internal linkage.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels/mxfp4_mma.h"
#include "kernels/mxfp6_cvt.h"

namespace dissem {
namespace kern {
namespace {

struct Mxfp6Layout {
  const uint8_t* packed;
  int64_t pchunk;  // bytes of a full packed chunk
  int64_t full;    // full chunks of the layer
  int cblk;        // scale blocks of a full chunk
  int tblk;        // scale blocks of the tail chunk (0: none)
};

// One lane's place in the packed layer, in scale blocks.
struct BlockPos6 {
  const uint8_t* base;  // the chunk
  int64_t c;            // its index
  int r;                // block within the chunk
  int nblk;             // blocks of the chunk: the codes are 24 * nblk bytes, the scales follow
  __device__ __forceinline__ void init(const Mxfp6Layout& L, int64_t block) {
    c = block / L.cblk;
    r = int(block - c * L.cblk);
    base = L.packed + c * L.pchunk;
    nblk = c < L.full ? L.cblk : L.tblk;
  }
  // d <= 16 blocks forward. Past the end of the layer the position is
  // meaningless; the callers never read through such a position.
  __device__ __forceinline__ void advance(const Mxfp6Layout& L, int d) {
    r += d;
    if (r >= nblk) {
      r -= nblk;
      ++c;
      base += L.pchunk;
      nblk = c < L.full ? L.cblk : L.tblk;
    }
  }
  __device__ __forceinline__ const uint8_t* q() const { return base + int64_t(r) * 24; }
  __device__ __forceinline__ uint32_t scale() const { return base[int64_t(nblk) * 24 + r]; }
  // the block's 24 B of codes: 8-B aligned, three 8-B words
  __device__ __forceinline__ mxfp6_u32x6_t codes() const {
    const uint2* p = reinterpret_cast<const uint2*>(q());
    const uint2 a = p[0], b = p[1], d = p[2];
    return mxfp6_u32x6_t{a.x, a.y, b.x, b.y, d.x, d.y};
  }
};

// The layout of a layer of `src_bytes` bf16 bytes packed in chunks of `src_chunk`.
inline Mxfp6Layout mxfp6_layout(const void* packed, int64_t src_bytes, int64_t src_chunk) {
  Mxfp6Layout L;
  L.packed = static_cast<const uint8_t*>(packed);
  L.pchunk = src_chunk / 64 * 25;
  L.full = src_bytes / src_chunk;
  L.cblk = int(src_chunk / 64);
  L.tblk = int(src_bytes % src_chunk / 64);
  return L;
}

}  // namespace
}  // namespace kern
}  // namespace dissem
