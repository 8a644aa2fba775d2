// Device code shared by the many-row kernels of the fp8 and MXFP6 formats
// (fp8_tiled.hip, mxfp6_tiled.hip): the x side of mxfp4_tiled.hip, which does not
// depend on the weight format - the fragment-ordered, XOR-swizzled image of a K
// step of x in LDS, the pair that stages it (global -> registers before a step's
// MFMAs, registers -> LDS after them) and the XCD-aware workgroup id. The design
// and its reasons are in mxfp4_tiled.hip's header. Everything here has internal
// linkage.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels/mxfp4_mma.h"

namespace dissem {
namespace kern {
namespace {

constexpr int kTiledWaves = 4;  // 256 threads

// The 16-B slot of an x image that holds the A operand of lane (c, g) for row
// tile t and piece pc (MFMA u of a step in the main form, block tb of a
// block-wise tail step). A piece is 1 KiB, lane group g its 256-B row, and c is
// XORed with 2 pc + (g & 1): the fragment read (ds_read_b128, served in groups
// of 16 lanes that hold every c once, half from an even and half from an odd g)
// still finds 16 different slots, and the staging store of a main-form step (8
// consecutive lanes: one row's pc = 0..3 for two g) finds 8 different ones.
__device__ __forceinline__ int frag_slot(int t, int pc, int g, int c) {
  return (t * 4 + pc) * 64 + g * 16 + (c ^ (2 * pc + (g & 1)));
}

// The hardware deals workgroup ids round-robin over the 8 XCDs: ids b, b + 8,
// ... share an XCD and become consecutive (the bijective form for grids that are
// no multiple of 8). Placement changes speed only.
__device__ __forceinline__ unsigned xcd_remap(unsigned b, unsigned nwg) {
  const unsigned q8 = nwg >> 3, r8 = nwg & 7, xcd = b & 7;
  return xcd * q8 + min(xcd, r8) + (b >> 3);
}

// Staging of a step's image for a workgroup of BM rows: a wave-load takes 4 rows
// of the step's 128 columns, 16 lanes per row (256 contiguous bytes); load i of
// wave w covers rows (BM / 4) w + 4 i .. + 3. This lane's 16 B are columns 8 sl
// .. 8 sl + 7 of its row, in block sl >> 2 of the step: MFMA u = sl & 3 of lane
// group sl >> 2 in the main form, piece sl >> 2 and lane group sl & 3 in the
// block-wise form (the tail of the kernels that run one block per MFMA there).
// Rows at and beyond M, and in the step after the last full one the blocks at
// and beyond K, are zero-filled and never read from global memory.
template <int BM>
struct XStage {
  static constexpr int kN = BM / 16 * 4 / kTiledWaves;  // 1-KiB pieces a wave stages per step
  u32x4_t st[kN];
  int sl, sr;
  __device__ __forceinline__ void init(int lane, int wave) {
    sl = lane & 15;
    sr = wave * (4 * kN) + (lane >> 4);
  }
  __device__ __forceinline__ void load(const uint16_t* __restrict__ x, int64_t m0, int64_t M, int K, int s, int nsteps,
                                       int tail) {
    const bool kok = s < nsteps || (sl >> 2) < tail;
    const uint16_t* src = x + (m0 + sr) * K + ((s << 7) + 8 * sl);
#pragma unroll
    for (int i = 0; i < kN; ++i)
      st[i] = kok && m0 + sr + 4 * i < M ? *reinterpret_cast<const u32x4_t*>(src + int64_t(4 * i) * K)
                                         : u32x4_t{0u, 0u, 0u, 0u};
  }
  __device__ __forceinline__ void store(u32x4_t* img, bool blockwise) const {
    const int pc = blockwise ? sl >> 2 : sl & 3, gr = blockwise ? sl & 3 : sl >> 2;
#pragma unroll
    for (int i = 0; i < kN; ++i) {
      const int r = sr + 4 * i;
      img[frag_slot(r >> 4, pc, gr, r & 15)] = st[i];
    }
  }
};

}  // namespace
}  // namespace kern
}  // namespace dissem
