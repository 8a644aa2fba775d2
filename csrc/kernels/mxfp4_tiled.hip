// W4A16 linear and gated linear for many rows of x, y = x * W^T and
// y = silu(x * Wg^T) * (x * Wu^T), with the weights read in place from an
// MXFP4-packed layer (core/mxfp4.h). mxfp4_linear.hip is the decode kernel: it
// passes over W once per 64 rows of x and every wave fetches x for itself. Here
// a workgroup owns an output tile of BM = 128 rows of x by BN = 128 rows of W,
// x is staged through LDS once per K step and shared by the four waves, and W
// is read and dequantized once per 128 rows of x.
//
// Fragment maps of v_mfma_f32_16x16x32_bf16 and the order of K are those of
// mxfp4_linear.hip: in the main loop (K in steps of 128) a lane (c = l & 15,
// g = l >> 4) takes a whole scale block of weight row n0 + c - 16 B of q, one
// scale byte, block 4 * step + g - and feeds its four dwords to four
// consecutive MFMAs, so in MFMA u the k slot 8g + j stands for
// k = 128 step + 32g + 8u + j; the K % 128 tail runs one block per MFMA in the
// plain order. Every output element has ONE accumulator, which takes step 0,
// 1, ... (u = 0..3 inside a step) and then the tail blocks: no split of K, no
// reduction, no atomics, no workspace. That order depends on nothing but K, so
// y[m][n] is a function of row m of x and row n of W alone - the same bits at
// M = 1 and M = 2048, in a merged q/k/v launch and a separate one, and for g
// and u of the gated kernel - which is the contract (batch invariance).
//
// Weights: registers only, as in the decode kernel (global -> dequantize ->
// MFMA operand). Wave w owns the 16-row tiles 2w and 2w + 1 of the workgroup's
// 128 rows of W (gated: gate tile w and up tile w of the workgroup's 64 columns
// of y, each tile with its own BlockPos) and applies each dequantized fragment
// to all 8 row tiles of x. A bf16 image of W in LDS would be written once and
// read once here (no two waves share a weight row): it could only add traffic.
//
// x in LDS: the image of a step is fragment-ordered. Piece (t, u) - row tile t,
// MFMA u - is 1 KiB and holds, 16 B per lane, what the 64 lanes of any wave need
// as their A operand for (t, u): lane (c, g) wants x[m0 + 16t + c][128 step +
// 32g + 8u ..]. Staging reads x coalesced - 16-B global loads, 16 lanes along
// the 256 B that a row has in the step, 4 rows per wave-load - and scatters the
// 16-B pieces into that order; the fragment read is one ds_read_b128 per (t, u).
// An XOR on c (frag_slot) keeps both sides free of bank conflicts. The tail
// step stores piece (t, block tb), lane (c, g) wanting x[..][128 steps + 32 tb
// + 8g ..] (its stores are 2-way conflicted, once per kernel). Rows beyond M and
// tail pieces beyond K are zero-filled in LDS and never read from global memory.
// Two images (2 * 32 KiB): the loads of step s + 1 (x into registers, the next
// weights) are issued before the MFMAs of step s and stored to the other image
// after them - one barrier per step.
//
// Grid: one workgroup per (M tile, N tile), M tiles fastest, on a remapped id:
// the hardware deals workgroup ids round-robin over the 8 XCDs, so id b is
// turned into xcd * (ids per XCD) + b / 8 (the bijective form for grids that
// are no multiple of 8). The workgroups that read the same 128 rows of W are
// then consecutive on one XCD and start together; all but the first find the
// weight tile in that XCD's L2. Placement changes speed only.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kernels/kernels.h"
#include "kernels/mxfp4_cvt.h"
#include "kernels/mxfp4_mma.h"

namespace dissem {
namespace kern {

namespace {

constexpr int kBM = kMxfp4TiledBM, kBN = kMxfp4TiledBN;
constexpr int kWaves = 4;                  // 256 threads
constexpr int kMT = kBM / 16;              // row tiles of x per workgroup
constexpr int kPieces = kMT * 4;           // 1-KiB pieces of a step's image
constexpr int kStage = kPieces / kWaves;   // pieces a wave stages per step
constexpr int kNT = kBN / 16 / kWaves;     // 16-row weight tiles per wave
static_assert(kBM % 16 == 0 && kBM >= 128 && kBN % (32 * kWaves) == 0 && kPieces % kWaves == 0, "tile shape");

// The 16-B slot of an x image that holds the A operand of lane (c, g) for row
// tile t and piece pc (MFMA u of a main step, block tb of the tail step). A
// piece is 1 KiB, lane group g its 256-B row, and c is XORed with 2 pc + (g & 1):
// the fragment read (ds_read_b128, served in groups of 16 lanes that hold every
// c once, half from an even and half from an odd g, each half keeping bits 3:2
// of c in {00, 11} or {01, 10}) still finds 16 different slots, and the staging
// store of a main step (8 consecutive lanes: one row's pc = 0..3 for two g) finds
// 8 different ones.
__device__ __forceinline__ int frag_slot(int t, int pc, int g, int c) {
  return (t * 4 + pc) * 64 + g * 16 + (c ^ (2 * pc + (g & 1)));
}

// A wave's kNT weight tiles are P output tiles: in the linear kernel each tile
// is one (P = kNT, the workgroup covers kBN columns of y); in the gated kernel
// tile q < P is gate tile q and tile P + q up tile q of the same rows (P = kNT /
// 2, the workgroup's kBN rows of W are kBN / 2 of Wg and of Wu and cover kBN / 2
// columns of y). Registers and the ratio of LDS reads to MFMAs are the same.
template <bool GATED, bool BF16>
__global__ void __launch_bounds__(64 * kWaves, 2)
    mxfp4_tiled_kernel(Mxfp4Layout L, int64_t off0, int64_t off1, const uint16_t* __restrict__ x, int64_t M, int N,
                       int K, void* __restrict__ y, int64_t ldy, unsigned mblocks) {
  constexpr int NT = kNT, P = GATED ? kNT / 2 : kNT;
  __shared__ u32x4_t xs[2][kPieces * 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = lane & 15, g = lane >> 4;
  // XCD-aware id: ids b, b + 8, ... share an XCD and become consecutive
  const unsigned nwg = gridDim.x, q8 = nwg >> 3, r8 = nwg & 7, xcd = blockIdx.x & 7;
  const unsigned lid = xcd * q8 + min(xcd, r8) + (blockIdx.x >> 3);
  const unsigned nb = lid / mblocks, mb = lid - nb * mblocks;
  const int64_t m0 = int64_t(mb) * kBM;
  const int n0 = (int(nb) * kWaves + wave) * (16 * P);
  const int nsteps = K >> 7, tail = (K >> 5) & 3;
  const int total = nsteps + (tail ? 1 : 0);

  // this lane's weight row per tile, in scale blocks; tiles beyond N read and store nothing
  int64_t row_blk[NT];
  bool valid[P];
#pragma unroll
  for (int j = 0; j < P; ++j) {
    valid[j] = n0 + 16 * j < N;
    row_blk[j] = (off0 + int64_t(n0 + 16 * j + c) * K) >> 5;
    if (GATED) row_blk[P + j] = (off1 + int64_t(n0 + 16 * j + c) * K) >> 5;
  }

  f32x4_t acc[kMT][NT];
#pragma unroll
  for (int t = 0; t < kMT; ++t)
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[t][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  const u32x4_t zero4 = {0u, 0u, 0u, 0u};

  // Staging: a wave-load takes 4 rows of the step's 128 columns, 16 lanes per
  // row (256 contiguous bytes); load i of wave w covers rows 32 w + 4 i .. + 3.
  // This lane's 16 B are columns 8 sl .. 8 sl + 7 of its row: MFMA u = sl & 3 of
  // lane group sl >> 2 in a main step, block sl >> 2 and lane group sl & 3 in
  // the tail step.
  const int sl = lane & 15, sr = wave * (4 * kStage) + (lane >> 4);
  u32x4_t st[kStage];
  auto stage_load = [&](int s) {
    const bool tl = s == nsteps;
    const bool kok = !tl || (sl >> 2) < tail;
    const uint16_t* src = x + (m0 + sr) * K + ((s << 7) + 8 * sl);
#pragma unroll
    for (int i = 0; i < kStage; ++i)
      st[i] = kok && m0 + sr + 4 * i < M ? *reinterpret_cast<const u32x4_t*>(src + int64_t(4 * i) * K) : zero4;
  };
  auto stage_store = [&](int buf, bool tl) {
    const int pc = tl ? sl >> 2 : sl & 3, gr = tl ? sl & 3 : sl >> 2;
#pragma unroll
    for (int i = 0; i < kStage; ++i) {
      const int r = sr + 4 * i;
      xs[buf][frag_slot(r >> 4, pc, gr, r & 15)] = st[i];
    }
  };

  BlockPos pos[NT];
  u32x4_t qn[NT];
  uint32_t sn[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    qn[j] = zero4;
    sn[j] = 0;
  }
  if (nsteps > 0) {
#pragma unroll
    for (int j = 0; j < NT; ++j)
      if (valid[j % P]) {
        pos[j].init(L, row_blk[j] + g);
        qn[j] = *reinterpret_cast<const u32x4_t*>(pos[j].q());
        sn[j] = pos[j].scale();
      }
  }
  stage_load(0);
  stage_store(0, nsteps == 0);
  __syncthreads();

  for (int s = 0; s < nsteps; ++s) {
    const u32x4_t* xa = xs[s & 1];
    if (s + 1 < total) stage_load(s + 1);
    u32x4_t qv[NT];
    uint32_t sb[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      qv[j] = qn[j];
      sb[j] = sn[j];
    }
    if (s + 1 < nsteps) {  // the next step's weights are in flight during this one
#pragma unroll
      for (int j = 0; j < NT; ++j)
        if (valid[j % P]) {
          pos[j].advance(L, 4);
          qn[j] = *reinterpret_cast<const u32x4_t*>(pos[j].q());
          sn[j] = pos[j].scale();
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
        uint32_t o[4];
        mxfp4_unpack8(qv[j][u], sb[j], o);
        const bf16x8_t b = as_frag(o);
#pragma unroll
        for (int t = 0; t < kMT; ++t)
          acc[t][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[u & 1][t], b, acc[t][j], 0, 0, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    if (s + 1 < total) {
      stage_store((s + 1) & 1, s + 1 == nsteps);
      __syncthreads();
    }
  }
  if (tail) {  // K % 128, from the last image: one block per MFMA, 4 B of q per lane
    const u32x4_t* xa = xs[nsteps & 1];
    BlockPos tp[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) tp[j].init(L, row_blk[j] + 4 * int64_t(nsteps));
    for (int tb = 0; tb < tail; ++tb) {
      bf16x8_t a[kMT];
#pragma unroll
      for (int t = 0; t < kMT; ++t) a[t] = __builtin_bit_cast(bf16x8_t, xa[frag_slot(t, tb, g, c)]);
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        uint32_t w = 0, sc = 0;
        if (valid[j % P]) {
          w = *reinterpret_cast<const uint32_t*>(tp[j].q() + 4 * g);
          sc = tp[j].scale();
          if (tb + 1 < tail) tp[j].advance(L, 1);
        }
        uint32_t o[4];
        mxfp4_unpack8(w, sc, o);
        const bf16x8_t b = as_frag(o);
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

bool layer_ok(const void* packed, int64_t src_bytes, int64_t src_chunk, const uint16_t* x, int64_t M, int64_t N,
              int64_t K, const void* y, int64_t ldy, bool y_bf16) {
  if (src_chunk <= 0 || src_chunk % 1024 || src_bytes <= 0 || src_bytes % 64) return false;
  if (M < 1 || N < 16 || N % 16 || K < 32 || K % 32 || K > 0x7FFFFF80 || N > 0x7FFFFFF0 || ldy < N) return false;
  if ((reinterpret_cast<uintptr_t>(packed) & 15) || (reinterpret_cast<uintptr_t>(x) & 15) ||
      (reinterpret_cast<uintptr_t>(y) & (y_bf16 ? 1 : 3)))
    return false;
  return src_chunk / 64 <= 0x7FFFFFFF;
}

bool param_ok(int64_t off, int64_t src_bytes, int64_t N, int64_t K) {
  return off >= 0 && off % 32 == 0 && N <= (src_bytes / 2 - off) / K;
}

template <bool GATED>
hipError_t launch(const void* packed, int64_t src_bytes, int64_t src_chunk, int64_t off0, int64_t off1,
                  const uint16_t* x, int64_t M, int64_t N, int64_t K, void* y, int64_t ldy, bool y_bf16,
                  hipStream_t s) {
  constexpr int cols = GATED ? kBN / 2 : kBN;  // columns of y per workgroup
  const int64_t mblocks = (M + kBM - 1) / kBM, nblocks = (N + cols - 1) / cols;
  if (mblocks > 0x7FFFFFFF / nblocks) return hipErrorInvalidValue;  // one launch: the grid is 1-D
  const Mxfp4Layout L = mxfp4_layout(packed, src_bytes, src_chunk);
  const dim3 grid{unsigned(mblocks * nblocks)}, block{64 * kWaves};
  if (y_bf16)
    mxfp4_tiled_kernel<GATED, true><<<grid, block, 0, s>>>(L, off0, off1, x, M, int(N), int(K), y, ldy, unsigned(mblocks));
  else
    mxfp4_tiled_kernel<GATED, false><<<grid, block, 0, s>>>(L, off0, off1, x, M, int(N), int(K), y, ldy, unsigned(mblocks));
  return hipGetLastError();
}

}  // namespace

hipError_t mxfp4_linear_tiled(const void* packed, int64_t src_bytes, int64_t src_chunk, int64_t elem_off,
                              const uint16_t* x, int64_t M, int64_t N, int64_t K, void* y, int64_t ldy, bool y_bf16,
                              hipStream_t s) {
  if (!layer_ok(packed, src_bytes, src_chunk, x, M, N, K, y, ldy, y_bf16)) return hipErrorInvalidValue;
  if (!param_ok(elem_off, src_bytes, N, K)) return hipErrorInvalidValue;
  return launch<false>(packed, src_bytes, src_chunk, elem_off, elem_off, x, M, N, K, y, ldy, y_bf16, s);
}

hipError_t mxfp4_swiglu_tiled(const void* packed, int64_t src_bytes, int64_t src_chunk, int64_t gate_off,
                              int64_t up_off, const uint16_t* x, int64_t M, int64_t N, int64_t K, void* y, int64_t ldy,
                              bool y_bf16, hipStream_t s) {
  if (!layer_ok(packed, src_bytes, src_chunk, x, M, N, K, y, ldy, y_bf16)) return hipErrorInvalidValue;
  if (!param_ok(gate_off, src_bytes, N, K) || !param_ok(up_off, src_bytes, N, K)) return hipErrorInvalidValue;
  return launch<true>(packed, src_bytes, src_chunk, gate_off, up_off, x, M, N, K, y, ldy, y_bf16, s);
}

}  // namespace kern
}  // namespace dissem
