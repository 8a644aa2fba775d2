// W8A16 linear and gated linear for many rows of x, y = x * W^T and
// y = silu(x * Wg^T) * (x * Wu^T), with the weights read in place from an
// fp8-packed layer (core/fp8.h). fp8_linear.hip / fp8_swiglu.hip are the decode
// kernels: they pass over W once per 64 rows of x. This is mxfp4_tiled.hip's
// design for the fp8 format - read that file's header first: a workgroup of 4
// waves owns BM = 128 rows of x by BN = 128 rows of W (gated: 64 rows of Wg and
// of Wu, 64 columns of y), x is staged through LDS once per K step of 128
// (tiled_x.h: fragment-ordered, XOR-swizzled, two images, one barrier per step)
// and shared by the waves, W is read and dequantized once per 128 rows of x and
// never touches LDS, the grid is 1-D on the XCD-remapped id with the M tiles
// fastest. No split of K, no reduction, no atomics, no workspace.
//
// Weights: wave w owns the 16-row tiles 2w and 2w + 1 of the workgroup's rows of
// W (gated: gate tile w and up tile w). Per lane (c = l & 15, g = l >> 4), tile
// and step: the group of 32 at k = 128 step + 32g of weight row n0 + c - 32 B of
// codes as two 16-B loads and one f32 scale, through ElemPos - and fp8_frag
// (fp8_mma.h) converts 8 codes per MFMA. A group of 32 never straddles a scale
// block or a chunk, for any block in {32, 64, 128, 256, 512} and any offset on
// the 32-element grid; the argument is in fp8_linear.hip's header. The next
// step's codes and scales are in flight during this step's MFMAs.
//
// K order: that of fp8_linear.hip. In MFMA u of a main step the k slot 8g + j
// stands for k = 128 step + 32g + 8u + j; the K % 128 tail runs one group of 32
// per MFMA in the plain order, 8 B of codes at 8g per lane, against piece (t,
// tb) of the last image of x. Every output element has ONE f32 accumulator that
// takes step 0, 1, ... (u = 0..3 inside a step) and then the tail groups: the
// instruction sequence of the decode kernel with split_k = 1, so the f32
// results are that kernel's bit for bit, y[m][n] depends on row m of x and row
// n of W alone (batch invariance), and g and u of the gated kernel are the
// tiled linear's f32 bits.
//
// NaN codes take no special path, as in the decode kernel.
//
// Resources (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage; no
// scratch and no spills in any instantiation; LDS 65536 B, two workgroups per
// CU under __launch_bounds__(256, 2)):
//   <GATED, BF16>   VGPRs  AGPRs  occupancy (waves/SIMD)
//   <false, false>  222    0      2
//   <false, true>   222    0      2
//   <true,  false>  222    0      2
//   <true,  true>   222    0      2
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kernels/fp8_cvt.h"
#include "kernels/fp8_mma.h"
#include "kernels/kernels.h"
#include "kernels/mxfp4_mma.h"
#include "kernels/tiled_x.h"

namespace dissem {
namespace kern {

namespace {

constexpr int kBM = kFp8TiledBM, kBN = kFp8TiledBN;
constexpr int kWaves = kTiledWaves;
constexpr int kMT = kBM / 16;              // row tiles of x per workgroup
constexpr int kPieces = kMT * 4;           // 1-KiB pieces of a step's image
constexpr int kNT = kBN / 16 / kWaves;     // 16-row weight tiles per wave
static_assert(kBM % 16 == 0 && kBM >= 128 && kBN % (32 * kWaves) == 0 && kPieces % kWaves == 0, "tile shape");

// A wave's kNT weight tiles are P output tiles: in the linear kernel each tile
// is one (P = kNT); in the gated kernel tile q < P is gate tile q and tile P + q
// up tile q of the same rows (P = kNT / 2), as in mxfp4_tiled.hip.
template <bool GATED, bool BF16>
__global__ void __launch_bounds__(64 * kWaves, 2)
    fp8_tiled_kernel(Fp8Layout L, int64_t off0, int64_t off1, const uint16_t* __restrict__ x, int64_t M, int N, int K,
                     void* __restrict__ y, int64_t ldy, unsigned mblocks) {
  constexpr int NT = kNT, P = GATED ? kNT / 2 : kNT;
  __shared__ u32x4_t xs[2][kPieces * 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = lane & 15, g = lane >> 4;
  const unsigned lid = xcd_remap(blockIdx.x, gridDim.x);
  const unsigned nb = lid / mblocks, mb = lid - nb * mblocks;
  const int64_t m0 = int64_t(mb) * kBM;
  const int n0 = (int(nb) * kWaves + wave) * (16 * P);
  const int nsteps = K >> 7, tail = (K >> 5) & 3;
  const int total = nsteps + (tail ? 1 : 0);

  // first element of this lane's weight row per tile; tiles beyond N read and store nothing
  int64_t row_elem[NT];
  bool valid[P];
#pragma unroll
  for (int j = 0; j < P; ++j) {
    valid[j] = n0 + 16 * j < N;
    row_elem[j] = off0 + int64_t(n0 + 16 * j + c) * K;
    if (GATED) row_elem[P + j] = off1 + int64_t(n0 + 16 * j + c) * K;
  }

  f32x4_t acc[kMT][NT];
#pragma unroll
  for (int t = 0; t < kMT; ++t)
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[t][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  const u32x4_t zero4 = {0u, 0u, 0u, 0u};

  XStage<kBM> stg;
  stg.init(lane, wave);

  ElemPos pos[NT];
  u32x4_t qn[NT][2];
  float sn[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    qn[j][0] = qn[j][1] = zero4;
    sn[j] = 0.f;
  }
  if (nsteps > 0) {
#pragma unroll
    for (int j = 0; j < NT; ++j)
      if (valid[j % P]) {
        pos[j].init(L, row_elem[j] + (g << 5));
        const u32x4_t* q = reinterpret_cast<const u32x4_t*>(pos[j].q());
        qn[j][0] = q[0];
        qn[j][1] = q[1];
        sn[j] = pos[j].scale(L);
      }
  }
  stg.load(x, m0, M, K, 0, nsteps, tail);
  stg.store(xs[0], nsteps == 0);
  __syncthreads();

  for (int s = 0; s < nsteps; ++s) {
    const u32x4_t* xa = xs[s & 1];
    if (s + 1 < total) stg.load(x, m0, M, K, s + 1, nsteps, tail);
    u32x4_t qv[NT][2];
    float sb[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      qv[j][0] = qn[j][0];
      qv[j][1] = qn[j][1];
      sb[j] = sn[j];
    }
    if (s + 1 < nsteps) {  // the next step's weights are in flight during this one
#pragma unroll
      for (int j = 0; j < NT; ++j)
        if (valid[j % P]) {
          pos[j].advance(L, 128);
          const u32x4_t* q = reinterpret_cast<const u32x4_t*>(pos[j].q());
          qn[j][0] = q[0];
          qn[j][1] = q[1];
          sn[j] = pos[j].scale(L);
        }
    }
    // the fragments of MFMA u + 1 are read while MFMA u's tiles run; the fence
    // keeps the compiler from hoisting all four sets (128 registers)
    bf16x8_t a[2][kMT];
#pragma unroll
    for (int t = 0; t < kMT; ++t) a[0][t] = __builtin_bit_cast(bf16x8_t, xa[frag_slot(t, 0, g, c)]);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (u < 3) {
#pragma unroll
        for (int t = 0; t < kMT; ++t) a[(u + 1) & 1][t] = __builtin_bit_cast(bf16x8_t, xa[frag_slot(t, u + 1, g, c)]);
      }
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        const bf16x8_t b = fp8_frag(qv[j][u >> 1][2 * (u & 1)], qv[j][u >> 1][2 * (u & 1) + 1], sb[j]);
#pragma unroll
        for (int t = 0; t < kMT; ++t)
          acc[t][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[u & 1][t], b, acc[t][j], 0, 0, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    if (s + 1 < total) {
      stg.store(xs[(s + 1) & 1], s + 1 == nsteps);
      __syncthreads();
    }
  }
  if (tail) {  // K % 128, from the last image: one group of 32 per MFMA, 8 B of codes per lane
    const u32x4_t* xa = xs[nsteps & 1];
    ElemPos tp[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) tp[j].init(L, row_elem[j] + (int64_t(nsteps) << 7));
    for (int tb = 0; tb < tail; ++tb) {
      bf16x8_t a[kMT];
#pragma unroll
      for (int t = 0; t < kMT; ++t) a[t] = __builtin_bit_cast(bf16x8_t, xa[frag_slot(t, tb, g, c)]);
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        uint2 w = {0u, 0u};
        float sc = 0.f;
        if (valid[j % P]) {
          w = *reinterpret_cast<const uint2*>(tp[j].q() + 8 * g);
          sc = tp[j].scale(L);
          if (tb + 1 < tail) tp[j].advance(L, 32);
        }
        const bf16x8_t b = fp8_frag(w.x, w.y, sc);
#pragma unroll
        for (int t = 0; t < kMT; ++t) acc[t][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[t], b, acc[t][j], 0, 0, 0);
      }
    }
  }

#pragma unroll
  for (int j = 0; j < P; ++j) {
    if (!valid[j]) continue;
#pragma unroll
    for (int t = 0; t < kMT; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int64_t m = m0 + 16 * t + 4 * g + i;
        if (m < M)
          store_y<BF16>(y, m * ldy + n0 + 16 * j + c,
                        GATED ? swiglu(acc[t][j][i], acc[t][GATED ? P + j : j][i]) : acc[t][j][i]);
      }
  }
}

// fp8_linear's / fp8_swiglu's checks without those of split_k and row_tiles_per_wave
bool layer_ok(const void* packed, int64_t src_bytes, int64_t src_chunk, int block, const uint16_t* x, int64_t M,
              int64_t N, int64_t K, const void* y, int64_t ldy, bool y_bf16) {
  if (block != 32 && block != 64 && block != 128 && block != 256 && block != 512) return false;
  if (src_chunk <= 0 || src_chunk % (8 * block) || src_bytes <= 0 || src_bytes % (2 * block)) return false;
  if (M < 1 || N < 16 || N % 16 || K < 32 || K % 32 || K > 0x7FFFFF80 || N > 0x7FFFFFF0 || ldy < N) return false;
  if ((reinterpret_cast<uintptr_t>(packed) & 15) || (reinterpret_cast<uintptr_t>(x) & 15) ||
      (reinterpret_cast<uintptr_t>(y) & (y_bf16 ? 1 : 3)))
    return false;
  return src_chunk / 2 <= 0x7FFFFF00;  // ElemPos counts a chunk's elements in an int
}

bool param_ok(int64_t off, int64_t src_bytes, int64_t N, int64_t K) {
  return off >= 0 && off % 32 == 0 && N <= (src_bytes / 2 - off) / K;
}

template <bool GATED>
hipError_t launch(const void* packed, int64_t src_bytes, int64_t src_chunk, int block, int64_t off0, int64_t off1,
                  const uint16_t* x, int64_t M, int64_t N, int64_t K, void* y, int64_t ldy, bool y_bf16,
                  hipStream_t s) {
  constexpr int cols = GATED ? kBN / 2 : kBN;  // columns of y per workgroup
  const int64_t mblocks = (M + kBM - 1) / kBM, nblocks = (N + cols - 1) / cols;
  if (mblocks > 0x7FFFFFFF / nblocks) return hipErrorInvalidValue;  // one launch: the grid is 1-D
  Fp8Layout L;
  L.packed = static_cast<const uint8_t*>(packed);
  L.celem = int(src_chunk / 2);
  L.pchunk = src_chunk / 2 + src_chunk / 2 / block * 4;
  L.full = src_bytes / src_chunk;
  L.telem = int(src_bytes % src_chunk / 2);
  L.shift = __builtin_ctz(unsigned(block));
  const dim3 grid{unsigned(mblocks * nblocks)}, blk{64 * kWaves};
  if (y_bf16)
    fp8_tiled_kernel<GATED, true><<<grid, blk, 0, s>>>(L, off0, off1, x, M, int(N), int(K), y, ldy, unsigned(mblocks));
  else
    fp8_tiled_kernel<GATED, false><<<grid, blk, 0, s>>>(L, off0, off1, x, M, int(N), int(K), y, ldy, unsigned(mblocks));
  return hipGetLastError();
}

}  // namespace

hipError_t fp8_linear_tiled(const void* packed, int64_t src_bytes, int64_t src_chunk, int block, int64_t elem_off,
                            const uint16_t* x, int64_t M, int64_t N, int64_t K, void* y, int64_t ldy, bool y_bf16,
                            hipStream_t s) {
  if (!layer_ok(packed, src_bytes, src_chunk, block, x, M, N, K, y, ldy, y_bf16)) return hipErrorInvalidValue;
  if (!param_ok(elem_off, src_bytes, N, K)) return hipErrorInvalidValue;
  return launch<false>(packed, src_bytes, src_chunk, block, elem_off, elem_off, x, M, N, K, y, ldy, y_bf16, s);
}

hipError_t fp8_swiglu_tiled(const void* packed, int64_t src_bytes, int64_t src_chunk, int block, int64_t gate_off,
                            int64_t up_off, const uint16_t* x, int64_t M, int64_t N, int64_t K, void* y, int64_t ldy,
                            bool y_bf16, hipStream_t s) {
  if (!layer_ok(packed, src_bytes, src_chunk, block, x, M, N, K, y, ldy, y_bf16)) return hipErrorInvalidValue;
  if (!param_ok(gate_off, src_bytes, N, K) || !param_ok(up_off, src_bytes, N, K)) return hipErrorInvalidValue;
  return launch<true>(packed, src_bytes, src_chunk, block, gate_off, up_off, x, M, N, K, y, ldy, y_bf16, s);
}

}  // namespace kern
}  // namespace dissem
