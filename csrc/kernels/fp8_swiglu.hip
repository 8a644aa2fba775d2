// The front half of a gated MLP from an fp8-packed layer in place:
//   y[m][n] = silu(g[m][n]) * u[m][n],  g = x * Wg^T,  u = x * Wu^T,
// with Wg and Wu two [N, K] parameters of one packed layer (core/fp8.h). Two
// existing kernels put together, nothing new in the numerics:
//
// Weight path: fp8_linear.hip's. Lane group g takes the group of 32 at
// k = 128 step + 32g of its row - two 16-B code loads and one f32 scale, its
// index a shift (ElemPos; scale blocks of 32, 64, 128, 256 and 512) - converts
// it pairwise (fp8_frag) and feeds four MFMAs, the next step's weights in
// flight during this one. The K % 128 tail runs one group of 32 per MFMA in the
// plain order, 8 B of codes per lane, with the last wave. Rows of x past M read
// nothing, as there.
//
// Work split and epilogue: mxfp4_swiglu.hip's. A wave owns P pairs of 16-row
// tiles, gate tile j and up tile j of the same rows n0 + 16 j .. + 15, all 2 P
// tiles fed from one x fragment; the two parameters lie anywhere in the layer,
// so every tile keeps its own ElemPos. The waves of a workgroup split K as the
// linear kernel does (per = ceil(steps / slices), the tail with the last wave)
// and reduce through LDS in the order of the slices: with equal slices, g and u
// are bit for bit what fp8_linear returns in f32. The thread that sums g and u
// of an element applies y = (g / (1 + expf(-g))) * u in f32 (swiglu(),
// mxfp4_mma.h) and stores once. No floating-point atomics.
//
// Registers (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage; no
// scratch and no spills in any instantiation, f32 / bf16 output): a wave with P
// pairs is a linear wave with NT = 2 P tiles, under
// __launch_bounds__(MT * P <= 1 ? 1024 : 512). VGPRs by (MT, P):
//   (1,1) 94   (1,2) 156  (2,1) 124  (2,2) 200  (3,1) 150  (4,1) 170
// 128 VGPRs are there for a workgroup of 16 waves, 256 for one of 8.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kernels/fp8_cvt.h"
#include "kernels/fp8_mma.h"
#include "kernels/kernels.h"
#include "kernels/mxfp4_mma.h"

namespace dissem {
namespace kern {

namespace {

// MT: 16-row tiles of x in this pass (M <= 16 * MT); P: pairs of 16-row tiles
// per wave. Tile q < P is gate tile q, tile P + q up tile q. blockDim.x = 64 *
// (K slices).
template <int MT, int P, bool BF16>
__global__ void __launch_bounds__(MT * P <= 1 ? 1024 : 512)
    fp8_swiglu_kernel(Fp8Layout L, int64_t gate_off, int64_t up_off, const uint16_t* __restrict__ x, int M, int K,
                      void* __restrict__ y, int64_t ldy) {
  extern __shared__ float red[];  // [slice][MT * 2 P * 4][64], only with more than one slice
  constexpr int NT = 2 * P, T = MT * NT;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, slices = blockDim.x >> 6;
  const int c = lane & 15, g = lane >> 4;
  const int n0 = blockIdx.x * (16 * P);
  const int nsteps = K >> 7, tail = (K >> 5) & 3;
  const int per = (nsteps + slices - 1) / slices;
  const int s0 = min(wave * per, nsteps), s1 = min(s0 + per, nsteps);
  // first element of this lane's weight row in every tile
  int64_t row_elem[NT];
#pragma unroll
  for (int j = 0; j < P; ++j) {
    row_elem[j] = gate_off + int64_t(n0 + 16 * j + c) * K;
    row_elem[P + j] = up_off + int64_t(n0 + 16 * j + c) * K;
  }

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
      pos[j].init(L, row_elem[j] + (int64_t(s0) << 7) + (g << 5));
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
    for (int j = 0; j < NT; ++j) pos[j].init(L, row_elem[j] + (int64_t(nsteps) << 7));
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
      for (int j = 0; j < P; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int m = 16 * t + 4 * g + i;
          if (m < M) store_y<BF16>(y, int64_t(m) * ldy + n0 + 16 * j + c, swiglu(acc[t][j][i], acc[t][P + j][i]));
        }
    return;
  }
  // fixed-order reduction over the K slices: a tile's element is at
  // ((t NT + q) 4 + i) * 64 + lane; a thread sums g and u of one result
  float* mine = red + wave * (T * 256);
#pragma unroll
  for (int t = 0; t < MT; ++t)
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int i = 0; i < 4; ++i) mine[((t * NT + j) * 4 + i) * 64 + lane] = acc[t][j][i];
  __syncthreads();
  for (int e = threadIdx.x; e < MT * P * 256; e += blockDim.x) {
    const int el = e & 63, ri = e >> 6;
    const int tj = ri >> 2, t = tj / P, j = tj - t * P, i = ri & 3;
    const int eg = ((t * NT + j) * 4 + i) * 64 + el, eu = eg + P * 256;
    float sg = red[eg], su = red[eu];
    for (int s = 1; s < slices; ++s) {
      sg += red[s * (T * 256) + eg];
      su += red[s * (T * 256) + eu];
    }
    const int m = 16 * t + 4 * (el >> 4) + i;
    if (m < M) store_y<BF16>(y, int64_t(m) * ldy + n0 + 16 * j + (el & 15), swiglu(sg, su));
  }
}

template <int MT, int P>
void launch(bool bf16, dim3 grid, dim3 block, size_t lds, hipStream_t s, const Fp8Layout& L, int64_t gate_off,
            int64_t up_off, const uint16_t* x, int M, int K, void* y, int64_t ldy) {
  if (bf16) fp8_swiglu_kernel<MT, P, true><<<grid, block, lds, s>>>(L, gate_off, up_off, x, M, K, y, ldy);
  else fp8_swiglu_kernel<MT, P, false><<<grid, block, lds, s>>>(L, gate_off, up_off, x, M, K, y, ldy);
}

// The most K slices for `mt` tiles along M and `p` pairs per wave: a wave holds
// the 2 p mt accumulator tiles of a linear wave with 2 p row tiles, so the
// linear kernel's register limit applies (see the header), and the partial
// sums, slices * mt * 2 p KiB, must fit 64 KiB of LDS.
int max_slices(int mt, int p) { return std::min(mt * p <= 1 ? 16 : 8, 32 / (mt * p)); }

// mxfp4_swiglu.hip's rule - 2 pairs (4 tiles, up to 32 rows of x) from 1024
// tiles on, otherwise 1 pair, and thin waves for few rows of x - retuned on
// MI355X over gate/up of llama3-70b (1792 pairs of tiles, K = 8192) and
// llama3-8b (896, K = 4096) at M = 1, 8, 16 and 64, scale blocks of 128 and 32,
// with scripts/packed_swiglu_bench.py --sweep (profiles/packed_swiglu/sweep.txt,
// spreads up to 8 %): at M = 1, 1 pair wins at both sizes (block 128: 97 against
// 112 us and 32.0 against 34.6), from M = 8 on 2 pairs win or tie (119 against
// 123 us, 36.7 against 37.0; at M = 16 by 11 to 15 %). M = 2 .. 7 and sizes
// between 896 and 1792 pairs were not measured.
int pairs(int m, int mt, int64_t tiles) {
  if (m <= 4) return 1;
  return mt <= 2 && 2 * tiles >= 1024 && tiles % 2 == 0 ? 2 : 1;
}

// K is split until the grid has about 8192 waves up to 4 rows of x, 2048 up to
// 8 and 896 beyond, never into more than 8 slices by choice: in the same sweep
// 16 slices never won by more than 1 %, and from M = 16 on few slices win (70b,
// M = 16, 2 pairs: 134 us unsplit, 137 at 4 slices; 8b, M = 64: 85 us unsplit,
// 89 at 2). The chosen slices are then the fastest measured or within 3 % of it,
// except 8b at M = 8 with block 32 (40.1 us at 8 slices, 38.4 at 2).
int auto_slices(int m, int mt, int p, int64_t wgs, int64_t nsteps) {
  const int64_t target = m <= 4 ? 8192 : m <= 8 ? 2048 : 896;
  const int most = std::min(8, max_slices(mt, p));
  int s = 1;
  while (2 * s <= most && wgs * s < target && 2 * s <= nsteps) s *= 2;
  return s;
}

bool param_ok(int64_t off, int64_t src_bytes, int64_t N, int64_t K) {
  return off >= 0 && off % 32 == 0 && N <= (src_bytes / 2 - off) / K;
}

}  // namespace

// One pass of m rows: the instantiation and the K slices, the only place the launcher below takes them from
// (kernels.h, DecodePlan).
DecodePlan fp8_swiglu_plan(int m, int64_t N, int64_t K, int split_k, int row_tiles_per_wave) {
  if (m < 1 || m > 64) return DecodePlan{0, 0, 0};
  const int rt = row_tiles_per_wave;
  const int mt = (m + 15) / 16;
  const int p = rt ? std::min(rt, mt <= 2 ? 2 : 1) : pairs(m, mt, N / 16);
  const int64_t wgs = N / 16 / p;
  const int slices = std::min(split_k ? split_k : auto_slices(m, mt, p, wgs, K / 128), max_slices(mt, p));
  return DecodePlan{mt, p, slices};
}

int fp8_swiglu_slices(int64_t M, int64_t N, int64_t K) {
  return fp8_swiglu_plan(int(std::min<int64_t>(M, 64)), N, K, 0, 0).slices;
}

hipError_t fp8_swiglu(const void* packed, int64_t src_bytes, int64_t src_chunk, int block, int64_t gate_off,
                      int64_t up_off, const uint16_t* x, int64_t M, int64_t N, int64_t K, void* y, int64_t ldy,
                      bool y_bf16, int split_k, int row_tiles_per_wave, hipStream_t s) {
  if (block != 32 && block != 64 && block != 128 && block != 256 && block != 512) return hipErrorInvalidValue;
  if (src_chunk <= 0 || src_chunk % (8 * block) || src_bytes <= 0 || src_bytes % (2 * block))
    return hipErrorInvalidValue;
  if (M < 1 || N < 16 || N % 16 || K < 32 || K % 32 || K > 0x7FFFFF80 || N > 0x7FFFFFF0 || ldy < N)
    return hipErrorInvalidValue;
  if (!param_ok(gate_off, src_bytes, N, K) || !param_ok(up_off, src_bytes, N, K)) return hipErrorInvalidValue;
  if ((reinterpret_cast<uintptr_t>(packed) & 15) || (reinterpret_cast<uintptr_t>(x) & 15) ||
      (reinterpret_cast<uintptr_t>(y) & (y_bf16 ? 1 : 3)))
    return hipErrorInvalidValue;
  if (src_chunk / 2 > 0x7FFFFF00) return hipErrorInvalidValue;  // ElemPos counts a chunk's elements in an int
  if (split_k < 0 || split_k > 16) return hipErrorInvalidValue;
  const int rt = row_tiles_per_wave;
  if ((rt != 0 && rt != 1 && rt != 2) || (rt && N / 16 % rt)) return hipErrorInvalidValue;
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
    const DecodePlan plan = fp8_swiglu_plan(m, N, K, split_k, rt);
    const int mt = plan.mt, p = plan.nt, slices = plan.slices;
    const int64_t wgs = N / 16 / p;
    const dim3 grid{unsigned(wgs)}, blk{unsigned(64 * slices)};
    const size_t lds = slices > 1 ? size_t(slices) * mt * 2 * p * 256 * sizeof(float) : 0;
    const uint16_t* xp = x + m0 * K;
    void* yp = static_cast<uint8_t*>(y) + size_t(m0) * size_t(ldy) * ysz;
#define DISSEM_SWIGLU_CASE(MT_, P_) \
  case MT_ * 4 + P_: launch<MT_, P_>(y_bf16, grid, blk, lds, s, L, gate_off, up_off, xp, m, int(K), yp, ldy); break
    switch (mt * 4 + p) {
      DISSEM_SWIGLU_CASE(1, 1);
      DISSEM_SWIGLU_CASE(1, 2);
      DISSEM_SWIGLU_CASE(2, 1);
      DISSEM_SWIGLU_CASE(2, 2);
      DISSEM_SWIGLU_CASE(3, 1);
      DISSEM_SWIGLU_CASE(4, 1);
      default: return hipErrorInvalidValue;
    }
#undef DISSEM_SWIGLU_CASE
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace kern
}  // namespace dissem
