// W6A16 linear, y = x * W^T, with W read in place from an MXFP6-packed layer
// (core/mxfp6.h): bf16 activations, e2m3 weights dequantized in registers by
// v_cvt_scalef32_pk32_bf16_fp6 (mxfp6_cvt.h), f32 accumulation in
// v_mfma_f32_16x16x32_bf16. No bf16 copy of W exists anywhere, and W never
// passes through LDS: global -> registers -> MFMA operand. The kernel has the
// shape of fp8_linear.hip; what differs is the weight format.
//
// Fragment maps of v_mfma_f32_16x16x32_bf16 (lane l, c = l & 15, g = l >> 4):
//   A[row c][k = 8g + j], B[k = 8g + j][col c], j = 0..7;  D[row 4g + i][col c], i = 0..3.
// With A = x (rows m) and B = W^T (columns n), lane l's B fragment is 8
// consecutive k of weight row n0 + c.
//
// One scale block per lane and step. elem_off and K are multiples of 32, so
// every weight row starts on the 32-element grid of the layer, which is the
// grid of the scale blocks; source chunks hold whole blocks. Lane group g
// takes the block at k = 128 step + 32g of its row: 24 B of codes at
// base + 24 r of its chunk and the E8M0 byte at base[24 nblk + r]. One
// conversion turns them into 32 bf16 in 16 dwords, dword d holding elements 2d
// and 2d + 1, so dwords 4t .. 4t + 3 are the B fragment of MFMA t (elements
// 8t .. 8t + 7 of the block). In MFMA t the k slot 8g + j therefore stands for
// k = 128 step + 32g + 8t + j; a sum over k is order-free, so the x fragment
// follows the same order (16 B at x[m][128 step + 32g + 8t]): fp8_linear's K
// order.
//
// Loads. A block is 8-B aligned and 16-B aligned only for an even r (packed
// chunks start 16-B aligned), so a lane reads its codes as three 8-B words; the
// scale is a byte load (the tail chunk's scale region is only 8-B aligned).
// The next step's codes and scale byte are in flight during this step's MFMAs.
// Three things make that true in the generated code (read in the ISA: the main
// loop waits with vmcnt(7..4), for x alone, where it first waited with
// vmcnt(0)): two steps per round on alternating register sets, so that nothing
// is copied from a "next" to a "current" set; x loaded ahead of the weights of
// the next step, since loads return in order; and the last one or two steps
// peeled, so that no load of the loop sits under a branch. On llama3-70b
// gate_proj at M = 1 this took the kernel from 64.4 to 60.1 us
// (profiles/mxfp6_linear/bench.txt against the first form in CHANGELOG.md).
//
// K tail (K % 128 != 0): one more step of the main form, run by the last wave,
// in which lane group g takes block 4 nsteps + g if g < tail and otherwise
// feeds zeros for both A and B. A masked lane reads nothing - neither codes nor
// scale nor x: its position may lie past the end of the row or of the layer.
// Chosen over fp8_linear's tail (8 elements of one block per lane group, here
// 48 bits at byte 6g: not dword aligned, to be cut out with 64-bit shifts, and
// four conversions of which a quarter of the result is used) because it is the
// main loop's code and data path: whole blocks, the same loads, one conversion.
//
// Position in the chunked layout: each lane keeps {chunk base, chunk index,
// block in the chunk, blocks of the chunk}, computed once per wave with one
// 64-bit division and then advanced by 4 blocks with a wrap. A full chunk holds
// at least 16 blocks (src_chunk is a multiple of 1024) and only the tail chunk
// may hold fewer, so a position inside the layer is reached with one wrap.
//
// Scale byte 0xFF (a NaN block): the converter returns a NaN in all 32
// elements (not 0x7FC0; mxfp6.hip). No special path: any NaN as a B element
// reaches exactly the outputs of its weight row. Scale bytes 0..254 convert
// exactly, bf16 subnormals and overflow to +-inf included.
//
// Work, K split and reduction are fp8_linear.hip's: one workgroup per 16 * NT
// weight rows, the waves of a workgroup split K in steps of 128 and reduce
// through LDS in the fixed order of the slices (no floating-point atomics), up
// to 4 accumulator tiles along M per pass over the weights.
//
// Registers (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage; no
// scratch and no spills in any instantiation, f32 / bf16 output), VGPRs by
// (MT, NT) under fp8_linear's launch bounds (1024 threads for MT * NT <= 2,
// else 512):
//   (1,1) 70   (1,2) 98   (1,4) 146  (2,1) 89   (2,2) 124  (2,4) 181
//   (3,1) 115  (3,2) 152  (4,1) 141  (4,2) 186
// so the bounds, max_slices and the NT set stay fp8_linear's: 128 VGPRs are
// there for a workgroup of 16 waves, 256 for one of 8.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kernels/kernels.h"
#include "kernels/mxfp4_mma.h"
#include "kernels/mxfp6_cvt.h"
#include "kernels/mxfp6_mma.h"

namespace dissem {
namespace kern {

namespace {

// MT: 16-row tiles of x in this pass (M <= 16 * MT); NT: 16-row tiles of W per
// wave. blockDim.x = 64 * (K slices).
template <int MT, int NT, bool BF16>
__global__ void __launch_bounds__(MT * NT <= 2 ? 1024 : 512)
    mxfp6_linear_kernel(Mxfp6Layout L, int64_t elem_off, const uint16_t* __restrict__ x, int M, int K,
                        void* __restrict__ y, int64_t ldy) {
  extern __shared__ float red[];  // [slice][MT * NT * 4][64], only with more than one slice
  constexpr int T = MT * NT;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, slices = blockDim.x >> 6;
  const int c = lane & 15, g = lane >> 4;
  const int n0 = blockIdx.x * (16 * NT);
  const int nsteps = K >> 7, tail = (K >> 5) & 3;
  const int per = (nsteps + slices - 1) / slices;
  const int s0 = min(wave * per, nsteps), s1 = min(s0 + per, nsteps);
  // first block of this lane's weight row in tile 0; tile j is 16 rows further
  const int64_t row_blk = (elem_off >> 5) + int64_t(n0 + c) * (K >> 5);
  const int64_t tile_blk = int64_t(K >> 5) << 4;

  f32x4_t acc[MT][NT];
  // This lane's row of x per tile. A row past M stands in as row 0: it only reaches the rows of
  // D past M, which are not stored.
  const uint16_t* xrow[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) {
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[t][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    xrow[t] = x + int64_t(16 * t + c < M ? 16 * t + c : 0) * K;
  }

  // The 32 elements of x at k for the four MFMAs of a step.
  auto load_x = [&](u32x4_t (&a)[MT][4], int k) {
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
      for (int u = 0; u < 4; ++u) a[t][u] = *reinterpret_cast<const u32x4_t*>(xrow[t] + k + 8 * u);
  };
  // One step: the block of every tile (codes qv, scale byte sb) against those elements of x.
  auto step = [&](const mxfp6_u32x6_t (&qv)[NT], const uint32_t (&sb)[NT], const u32x4_t (&a)[MT][4]) {
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const mxfp6_u32x16_t w = mxfp6_cvt_unpack_raw(qv[j], __uint_as_float(sb[j] << 23));
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const uint32_t o[4] = {w[4 * u], w[4 * u + 1], w[4 * u + 2], w[4 * u + 3]};
        const bf16x8_t b = as_frag(o);
#pragma unroll
        for (int t = 0; t < MT; ++t)
          acc[t][j] =
              __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a[t][u]), b, acc[t][j], 0, 0, 0);
      }
    }
  };

  if (s0 < s1) {
    BlockPos6 pos[NT];
    mxfp6_u32x6_t q0[NT], q1[NT];
    uint32_t b0[NT], b1[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      pos[j].init(L, row_blk + j * tile_blk + (int64_t(s0) << 2) + g);
      q0[j] = pos[j].codes();
      b0[j] = pos[j].scale();
    }
    auto fetch_next = [&](mxfp6_u32x6_t (&q)[NT], uint32_t (&b)[NT]) {
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        pos[j].advance(L, 4);
        q[j] = pos[j].codes();
        b[j] = pos[j].scale();
      }
    };
    // Two steps per round on alternating buffers: no register is copied from a "next" to a
    // "current" set (a copy would have to wait for the load). x is loaded first: loads return
    // in order, so waiting for x leaves the weights of the next step, issued behind it, in
    // flight during this step's MFMAs. The last one or two steps are peeled, so that no load
    // of the loop sits under a branch (where paths join, the wait counters take the worst).
    u32x4_t a[MT][4];
    int s = s0;
    for (; s + 2 < s1; s += 2) {
      load_x(a, (s << 7) + (g << 5));
      fetch_next(q1, b1);
      step(q0, b0, a);
      load_x(a, ((s + 1) << 7) + (g << 5));
      fetch_next(q0, b0);
      step(q1, b1, a);
    }
    load_x(a, (s << 7) + (g << 5));
    if (s + 2 == s1) {
      fetch_next(q1, b1);
      step(q0, b0, a);
      load_x(a, ((s + 1) << 7) + (g << 5));
      step(q1, b1, a);
    } else {
      step(q0, b0, a);
    }
  }
  if (tail && wave == slices - 1) {  // K % 128: one more step, lane groups past the tail masked
    const bool on = g < tail;
    mxfp6_u32x6_t qv[NT];
    uint32_t sb[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      qv[j] = mxfp6_u32x6_t{0u, 0u, 0u, 0u, 0u, 0u};
      sb[j] = 127u;  // zero codes under any finite scale: +0
      if (on) {
        BlockPos6 pos;
        pos.init(L, row_blk + j * tile_blk + (int64_t(nsteps) << 2) + g);
        qv[j] = pos.codes();
        sb[j] = pos.scale();
      }
    }
    u32x4_t a[MT][4];
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
      for (int u = 0; u < 4; ++u) a[t][u] = u32x4_t{0u, 0u, 0u, 0u};
    if (on) load_x(a, (nsteps << 7) + (g << 5));
    step(qv, sb, a);
  }

  if (slices == 1) {
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
      for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int m = 16 * t + 4 * g + i;
          if (m < M) store_y<BF16>(y, int64_t(m) * ldy + n0 + 16 * j + c, acc[t][j][i]);
        }
    return;
  }
  // fixed-order reduction over the K slices: element e = ((t NT + j) 4 + i) * 64 + lane
  float* mine = red + wave * (T * 256);
#pragma unroll
  for (int t = 0; t < MT; ++t)
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int i = 0; i < 4; ++i) mine[((t * NT + j) * 4 + i) * 64 + lane] = acc[t][j][i];
  __syncthreads();
  for (int e = threadIdx.x; e < T * 256; e += blockDim.x) {
    float sum = red[e];
    for (int s = 1; s < slices; ++s) sum += red[s * (T * 256) + e];
    const int el = e & 63, ri = e >> 6;
    const int tj = ri >> 2, t = tj / NT, j = tj - t * NT;
    const int m = 16 * t + 4 * (el >> 4) + (ri & 3);
    if (m < M) store_y<BF16>(y, int64_t(m) * ldy + n0 + 16 * j + (el & 15), sum);
  }
}

template <int MT, int NT>
void launch(bool bf16, dim3 grid, dim3 block, size_t lds, hipStream_t s, const Mxfp6Layout& L, int64_t elem_off,
            const uint16_t* x, int M, int K, void* y, int64_t ldy) {
  if (bf16) mxfp6_linear_kernel<MT, NT, true><<<grid, block, lds, s>>>(L, elem_off, x, M, K, y, ldy);
  else mxfp6_linear_kernel<MT, NT, false><<<grid, block, lds, s>>>(L, elem_off, x, M, K, y, ldy);
}

// Row tiles per wave and the most K slices for `mt` tiles along M: the
// accumulators, the x fragments, the 16 converted dwords of a tile and two
// steps of codes must fit the registers of a workgroup of that many waves (see
// the header), its partial sums 64 KiB of LDS.
int max_slices(int mt, int nt) { return std::min(mt * nt <= 2 ? 16 : 8, 64 / (mt * nt)); }

// fp8_linear.hip's rules, kept after a sweep on MI355X over the llama3-70b
// projections (scripts/mxfp6_linear_bench.py --sweep,
// profiles/mxfp6_linear/sweep.txt): in 12 of its 16 cells the rules' choice is
// within 1.5 % of the best forced (row_tiles, split_k), in the others within 3 %
// (gate_proj M = 1: 59.2 us with 2 tiles against 57.6 with 1, spreads 3-5 %).
// A wave takes 2 row tiles from 256 tiles on and 4 (from 2 up to 32 rows of x)
// from 1024 on ...
int row_tiles(int m, int mt, int64_t tiles) {
  if (m > 1 && mt <= 2 && tiles >= 1024 && tiles % 4 == 0) return 4;
  if (tiles >= 256 && tiles % 2 == 0) return 2;
  return 1;
}

// ... and K is split until the grid has about 4096 waves for up to 8 rows of
// x and 1024 beyond, with at least one step of 128 per slice.
int auto_slices(int m, int mt, int nt, int64_t wgs, int64_t nsteps) {
  const int64_t target = m <= 8 ? 4096 : 1024;
  int s = 1;
  while (2 * s <= max_slices(mt, nt) && wgs * s < target && 2 * s <= nsteps) s *= 2;
  return s;
}

}  // namespace

// One pass of m rows: the instantiation and the K slices, the only place the launcher below takes them from
// (kernels.h, DecodePlan).
DecodePlan mxfp6_linear_plan(int m, int64_t N, int64_t K, int split_k, int row_tiles_per_wave) {
  if (m < 1 || m > 64) return DecodePlan{0, 0, 0};
  const int rt = row_tiles_per_wave;
  const int mt = (m + 15) / 16;
  const int nt = rt ? std::min(rt, mt <= 2 ? 4 : 2) : row_tiles(m, mt, N / 16);
  const int64_t wgs = N / 16 / nt;
  const int slices = std::min(split_k ? split_k : auto_slices(m, mt, nt, wgs, K / 128), max_slices(mt, nt));
  return DecodePlan{mt, nt, slices};
}

int mxfp6_linear_slices(int64_t M, int64_t N, int64_t K) {
  return mxfp6_linear_plan(int(std::min<int64_t>(M, 64)), N, K, 0, 0).slices;
}

hipError_t mxfp6_linear(const void* packed, int64_t src_bytes, int64_t src_chunk, int64_t elem_off, const uint16_t* x,
                        int64_t M, int64_t N, int64_t K, void* y, int64_t ldy, bool y_bf16, int split_k,
                        int row_tiles_per_wave, hipStream_t s) {
  if (src_chunk <= 0 || src_chunk % 1024 || src_bytes <= 0 || src_bytes % 64) return hipErrorInvalidValue;
  if (M < 1 || N < 16 || N % 16 || K < 32 || K % 32 || K > 0x7FFFFF80 || N > 0x7FFFFFF0 || ldy < N)
    return hipErrorInvalidValue;
  if (elem_off < 0 || elem_off % 32 || N > (src_bytes / 2 - elem_off) / K) return hipErrorInvalidValue;
  if ((reinterpret_cast<uintptr_t>(packed) & 15) || (reinterpret_cast<uintptr_t>(x) & 15) ||
      (reinterpret_cast<uintptr_t>(y) & (y_bf16 ? 1 : 3)))
    return hipErrorInvalidValue;
  if (src_chunk / 64 > 0x7FFFFF00) return hipErrorInvalidValue;  // BlockPos6 counts a chunk's blocks in an int
  if (split_k < 0 || split_k > 16) return hipErrorInvalidValue;
  const int rt = row_tiles_per_wave;
  if ((rt != 0 && rt != 1 && rt != 2 && rt != 4) || (rt && N / 16 % rt)) return hipErrorInvalidValue;
  const Mxfp6Layout L = mxfp6_layout(packed, src_bytes, src_chunk);
  const size_t ysz = y_bf16 ? 2 : 4;
  for (int64_t m0 = 0; m0 < M; m0 += 64) {
    const int m = int(std::min<int64_t>(64, M - m0));
    const DecodePlan plan = mxfp6_linear_plan(m, N, K, split_k, rt);
    const int mt = plan.mt, nt = plan.nt, slices = plan.slices;
    const int64_t wgs = N / 16 / nt;
    const dim3 grid{unsigned(wgs)}, blk{unsigned(64 * slices)};
    const size_t lds = slices > 1 ? size_t(slices) * mt * nt * 256 * sizeof(float) : 0;
    const uint16_t* xp = x + m0 * K;
    void* yp = static_cast<uint8_t*>(y) + size_t(m0) * size_t(ldy) * ysz;
#define DISSEM_LINEAR_CASE(MT_, NT_) \
  case MT_ * 8 + NT_: launch<MT_, NT_>(y_bf16, grid, blk, lds, s, L, elem_off, xp, m, int(K), yp, ldy); break
    switch (mt * 8 + nt) {
      DISSEM_LINEAR_CASE(1, 1);
      DISSEM_LINEAR_CASE(1, 2);
      DISSEM_LINEAR_CASE(1, 4);
      DISSEM_LINEAR_CASE(2, 1);
      DISSEM_LINEAR_CASE(2, 2);
      DISSEM_LINEAR_CASE(2, 4);
      DISSEM_LINEAR_CASE(3, 1);
      DISSEM_LINEAR_CASE(3, 2);
      DISSEM_LINEAR_CASE(4, 1);
      DISSEM_LINEAR_CASE(4, 2);
      default: return hipErrorInvalidValue;
    }
#undef DISSEM_LINEAR_CASE
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace kern
}  // namespace dissem
