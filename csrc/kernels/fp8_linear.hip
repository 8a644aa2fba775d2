// W8A16 linear, y = x * W^T, with W read in place from an fp8-packed layer
// (core/fp8.h): bf16 activations, e4m3 weights dequantized in registers by
// v_cvt_scalef32_pk_bf16_fp8 (fp8_cvt.h), f32 accumulation in
// v_mfma_f32_16x16x32_bf16. No bf16 copy of W exists anywhere, and W never
// passes through LDS: global -> registers -> MFMA operand. The kernel has the
// shape of mxfp4_linear.hip; what differs is the weight format.
//
// Fragment maps of v_mfma_f32_16x16x32_bf16 (lane l, c = l & 15, g = l >> 4):
//   A[row c][k = 8g + j], B[k = 8g + j][col c], j = 0..7;  D[row 4g + i][col c], i = 0..3.
// With A = x (rows m) and B = W^T (columns n), lane l's B fragment is 8
// consecutive k of weight row n0 + c: 8 B of codes.
//
// One group of 32. A lane always reads 32 consecutive elements of one weight
// row that start on the 32-element grid of the layer: elem_off and K are
// multiples of 32, so every row starts on that grid, and the kernel steps along
// a row in 32s. A scale block holds 32, 64, 128, 256 or 512 elements and a
// source chunk (and the tail chunk) a whole number of blocks, so blocks and
// chunks both start on the 32-element grid and a group of 32 never straddles a
// block or a chunk: its 32 B of codes are contiguous in one packed chunk and
// share one f32 scale, whatever block, elem_off and K are. src_chunk is a
// multiple of 8 * block bytes, i.e. a chunk holds n = 4 j block elements and
// packs to n + 4 n / block = 4 j block + 16 j bytes: every packed chunk starts
// 16-B aligned, a group of 32 therefore 16-B aligned too (two 16-B loads), and
// the scales (at byte n of the chunk) 4-B aligned.
//
// Main loop, K in steps of 128: lane group g takes the group of 32 at
// k = 128 step + 32g of its row - 32 B of codes and one scale - converts it
// pairwise (16 conversions) and feeds four MFMAs with 8 elements each. In MFMA
// t the k slot 8g + j therefore stands for k = 128 step + 32g + 8t + j; a sum
// over k is order-free, so the x fragment follows the same order (16 B at
// x[m][128 step + 32g + 8t]). The K tail (K % 128 != 0) runs one group of 32
// per MFMA in the plain order, 8 B of codes per lane.
//
// Position in the chunked layout: each lane keeps {chunk base, chunk index,
// element in the chunk, elements of the chunk}, computed once per wave with one
// 64-bit division and then advanced by 128 (or 32) elements with a wrap. A full
// chunk holds at least 4 * 32 = 128 elements and only the tail chunk may hold
// fewer, so a position inside the layer is reached with one wrap per advance.
// The scale index is a shift (block is a power of two).
//
// NaN codes (0x7F, 0xFF) convert to the bf16 NaN 0xFFC0 (core/fp8.h) and take
// no special path: the NaN enters the MFMA as a B element of its weight row and
// reaches exactly the outputs of that row.
//
// Work, K split and reduction are mxfp4_linear.hip's: one workgroup per
// 16 * NT weight rows, the waves of a workgroup split K in steps of 128 and
// reduce through LDS in the fixed order of the slices (no floating-point
// atomics), up to 4 accumulator tiles along M per pass over the weights.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kernels/fp8_cvt.h"
#include "kernels/fp8_mma.h"
#include "kernels/kernels.h"
#include "kernels/mxfp4_mma.h"

namespace dissem {
namespace kern {

namespace {

// MT: 16-row tiles of x in this pass (M <= 16 * MT); NT: 16-row tiles of W per
// wave. blockDim.x = 64 * (K slices).
template <int MT, int NT, bool BF16>
__global__ void __launch_bounds__(MT * NT <= 2 ? 1024 : 512)
    fp8_linear_kernel(Fp8Layout L, int64_t elem_off, const uint16_t* __restrict__ x, int M, int K,
                      void* __restrict__ y, int64_t ldy) {
  extern __shared__ float red[];  // [slice][MT * NT * 4][64], only with more than one slice
  constexpr int T = MT * NT;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, slices = blockDim.x >> 6;
  const int c = lane & 15, g = lane >> 4;
  const int n0 = blockIdx.x * (16 * NT);
  const int nsteps = K >> 7, tail = (K >> 5) & 3;
  const int per = (nsteps + slices - 1) / slices;
  const int s0 = min(wave * per, nsteps), s1 = min(s0 + per, nsteps);
  // first element of this lane's weight row in tile 0; tile j is 16 rows further
  const int64_t row_elem = elem_off + int64_t(n0 + c) * K;
  const int64_t tile_elem = int64_t(K) << 4;

  f32x4_t acc[MT][NT];
  const uint16_t* xrow[MT];  // this lane's row of x per tile; rows past M read nothing
  bool live[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) {
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[t][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    live[t] = 16 * t + c < M;
    xrow[t] = x + int64_t(live[t] ? 16 * t + c : 0) * K;
  }
  const u32x4_t zero4 = {0u, 0u, 0u, 0u};

  if (s0 < s1) {
    ElemPos pos[NT];
    u32x4_t qn[NT][2];
    float sn[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      pos[j].init(L, row_elem + j * tile_elem + (int64_t(s0) << 7) + (g << 5));
      const u32x4_t* q = reinterpret_cast<const u32x4_t*>(pos[j].q());
      qn[j][0] = q[0];
      qn[j][1] = q[1];
      sn[j] = pos[j].scale(L);
    }
    for (int s = s0; s < s1; ++s) {
      u32x4_t qv[NT][2];
      float sb[NT];
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        qv[j][0] = qn[j][0];
        qv[j][1] = qn[j][1];
        sb[j] = sn[j];
      }
      if (s + 1 < s1) {  // the next step's weights are in flight during this one
#pragma unroll
        for (int j = 0; j < NT; ++j) {
          pos[j].advance(L, 128);
          const u32x4_t* q = reinterpret_cast<const u32x4_t*>(pos[j].q());
          qn[j][0] = q[0];
          qn[j][1] = q[1];
          sn[j] = pos[j].scale(L);
        }
      }
      const int k = (s << 7) + (g << 5);
      u32x4_t a[MT][4];
#pragma unroll
      for (int t = 0; t < MT; ++t)
#pragma unroll
        for (int u = 0; u < 4; ++u)
          a[t][u] = live[t] ? *reinterpret_cast<const u32x4_t*>(xrow[t] + k + 8 * u) : zero4;
#pragma unroll
      for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const bf16x8_t b = fp8_frag(qv[j][u >> 1][2 * (u & 1)], qv[j][u >> 1][2 * (u & 1) + 1], sb[j]);
#pragma unroll
          for (int t = 0; t < MT; ++t)
            acc[t][j] =
                __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a[t][u]), b, acc[t][j], 0, 0, 0);
        }
    }
  }
  if (tail && wave == slices - 1) {  // K % 128: one group of 32 per MFMA, 8 B of codes per lane
    ElemPos pos[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) pos[j].init(L, row_elem + j * tile_elem + (int64_t(nsteps) << 7));
    for (int tb = 0; tb < tail; ++tb) {
      const int k = ((4 * nsteps + tb) << 5) + 8 * g;
      u32x4_t a[MT];
#pragma unroll
      for (int t = 0; t < MT; ++t) a[t] = live[t] ? *reinterpret_cast<const u32x4_t*>(xrow[t] + k) : zero4;
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        const uint2 w = *reinterpret_cast<const uint2*>(pos[j].q() + 8 * g);
        const bf16x8_t b = fp8_frag(w.x, w.y, pos[j].scale(L));
#pragma unroll
        for (int t = 0; t < MT; ++t)
          acc[t][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a[t]), b, acc[t][j], 0, 0, 0);
        if (tb + 1 < tail) pos[j].advance(L, 32);
      }
    }
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
void launch(bool bf16, dim3 grid, dim3 block, size_t lds, hipStream_t s, const Fp8Layout& L, int64_t elem_off,
            const uint16_t* x, int M, int K, void* y, int64_t ldy) {
  if (bf16) fp8_linear_kernel<MT, NT, true><<<grid, block, lds, s>>>(L, elem_off, x, M, K, y, ldy);
  else fp8_linear_kernel<MT, NT, false><<<grid, block, lds, s>>>(L, elem_off, x, M, K, y, ldy);
}

// Row tiles per wave and the most K slices for `mt` tiles along M: the
// accumulators, the x fragments and two steps of weights must fit the
// registers of a workgroup of that many waves, its partial sums 64 KiB of LDS.
int max_slices(int mt, int nt) { return std::min(mt * nt <= 2 ? 16 : 8, 64 / (mt * nt)); }

// mxfp4_linear.hip's rules, retuned in two places from a sweep on MI355X over the
// llama3-70b projections (scripts/fp8_linear_bench.py --sweep,
// profiles/fp8_linear/sweep.txt): a wave takes 2 row tiles from 256 tiles on
// and 4 (from 2 up to 32 rows of x) from 1024 on. With a single row of x, 4
// lost to 2 (gate_proj, M = 1: 61.8 us with 4 and 8 slices, 56.8 with 2) ...
int row_tiles(int m, int mt, int64_t tiles) {
  if (m > 1 && mt <= 2 && tiles >= 1024 && tiles % 4 == 0) return 4;
  if (tiles >= 256 && tiles % 2 == 0) return 2;
  return 1;
}

// ... and K is split until the grid has about 4096 waves for up to 8 rows of
// x and 1024 beyond, with at least one step of 128 per slice. MXFP4 goes to
// 2048 up to 32 rows; here that lost at M = 16 (down_proj 81.4 us at 8 slices,
// 74.7 at 4; q_proj 24.8 and 23.7). 17 to 32 rows were not swept.
int auto_slices(int m, int mt, int nt, int64_t wgs, int64_t nsteps) {
  const int64_t target = m <= 8 ? 4096 : 1024;
  int s = 1;
  while (2 * s <= max_slices(mt, nt) && wgs * s < target && 2 * s <= nsteps) s *= 2;
  return s;
}

}  // namespace

// One pass of m rows: the instantiation and the K slices, the only place the launcher below takes them from
// (kernels.h, DecodePlan).
DecodePlan fp8_linear_plan(int m, int64_t N, int64_t K, int split_k, int row_tiles_per_wave) {
  if (m < 1 || m > 64) return DecodePlan{0, 0, 0};
  const int rt = row_tiles_per_wave;
  const int mt = (m + 15) / 16;
  const int nt = rt ? std::min(rt, mt <= 2 ? 4 : 2) : row_tiles(m, mt, N / 16);
  const int64_t wgs = N / 16 / nt;
  const int slices = std::min(split_k ? split_k : auto_slices(m, mt, nt, wgs, K / 128), max_slices(mt, nt));
  return DecodePlan{mt, nt, slices};
}

int fp8_linear_slices(int64_t M, int64_t N, int64_t K) {
  return fp8_linear_plan(int(std::min<int64_t>(M, 64)), N, K, 0, 0).slices;
}

hipError_t fp8_linear(const void* packed, int64_t src_bytes, int64_t src_chunk, int block, int64_t elem_off,
                      const uint16_t* x, int64_t M, int64_t N, int64_t K, void* y, int64_t ldy, bool y_bf16,
                      int split_k, int row_tiles_per_wave, hipStream_t s) {
  if (block != 32 && block != 64 && block != 128 && block != 256 && block != 512) return hipErrorInvalidValue;
  if (src_chunk <= 0 || src_chunk % (8 * block) || src_bytes <= 0 || src_bytes % (2 * block))
    return hipErrorInvalidValue;
  if (M < 1 || N < 16 || N % 16 || K < 32 || K % 32 || K > 0x7FFFFF80 || N > 0x7FFFFFF0 || ldy < N)
    return hipErrorInvalidValue;
  if (elem_off < 0 || elem_off % 32 || N > (src_bytes / 2 - elem_off) / K) return hipErrorInvalidValue;
  if ((reinterpret_cast<uintptr_t>(packed) & 15) || (reinterpret_cast<uintptr_t>(x) & 15) ||
      (reinterpret_cast<uintptr_t>(y) & (y_bf16 ? 1 : 3)))
    return hipErrorInvalidValue;
  if (src_chunk / 2 > 0x7FFFFF00) return hipErrorInvalidValue;  // ElemPos counts a chunk's elements in an int
  if (split_k < 0 || split_k > 16) return hipErrorInvalidValue;
  const int rt = row_tiles_per_wave;
  if ((rt != 0 && rt != 1 && rt != 2 && rt != 4) || (rt && N / 16 % rt)) return hipErrorInvalidValue;
  Fp8Layout L;
  L.packed = static_cast<const uint8_t*>(packed);
  L.celem = int(src_chunk / 2);
  L.pchunk = src_chunk / 2 + src_chunk / 2 / block * 4;
  L.full = src_bytes / src_chunk;
  L.telem = int(src_bytes % src_chunk / 2);
  L.shift = __builtin_ctz(unsigned(block));
  const size_t ysz = y_bf16 ? 2 : 4;
  for (int64_t m0 = 0; m0 < M; m0 += 64) {
    const int m = int(std::min<int64_t>(64, M - m0));
    const DecodePlan plan = fp8_linear_plan(m, N, K, split_k, rt);
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
