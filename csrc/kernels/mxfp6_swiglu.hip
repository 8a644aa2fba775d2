// The front half of a gated MLP from an MXFP6-packed layer in place:
//   y[m][n] = silu(g[m][n]) * u[m][n],  g = x * Wg^T,  u = x * Wu^T,
// with Wg and Wu two [N, K] parameters of one packed layer (core/mxfp6.h). Two
// existing kernels put together, nothing new in the numerics:
//
// Weight path: mxfp6_linear.hip's. Lane group g takes the block at
// k = 128 step + 32g of its row - three 8-B code loads and the scale byte
// (BlockPos6), one v_cvt_scalef32_pk32_bf16_fp6 (mxfp6_cvt_unpack_raw), four
// MFMAs in the order of the block's dwords - two steps per round on alternating
// register sets with x loaded ahead of the next step's weights, the last one or
// two steps peeled, and the K % 128 tail as one more masked step of the last
// wave in which a masked lane group reads neither codes, scale nor x. A row of
// x past M stands in as row 0, as there.
//
// Work split and epilogue: mxfp4_swiglu.hip's. A wave owns P pairs of 16-row
// tiles, gate tile j and up tile j of the same rows n0 + 16 j .. + 15, all 2 P
// tiles fed from one x fragment; the two parameters lie anywhere in the layer,
// so every tile keeps its own BlockPos6. The waves of a workgroup split K as
// the linear kernel does (per = ceil(steps / slices), the tail with the last
// wave) and reduce through LDS in the order of the slices: with equal slices, g
// and u are bit for bit what mxfp6_linear returns in f32. The thread that sums
// g and u of an element applies y = (g / (1 + expf(-g))) * u in f32 (swiglu(),
// mxfp4_mma.h) and stores once. No floating-point atomics.
//
// Registers (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage; no
// scratch and no spills in any instantiation, f32 / bf16 output): a wave with P
// pairs is a linear wave with NT = 2 P tiles, under
// __launch_bounds__(MT * P <= 1 ? 1024 : 512). VGPRs by (MT, P):
//   (1,1) 100  (1,2) 152  (2,1) 126  (2,2) 187  (3,1) 154  (4,1) 188
// (the linear kernel's (MT, 2 P) within 6): 128 VGPRs are there for a
// workgroup of 16 waves, 256 for one of 8.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kernels/kernels.h"
#include "kernels/mxfp4_mma.h"
#include "kernels/mxfp6_cvt.h"
#include "kernels/mxfp6_mma.h"

namespace dissem {
namespace kern {

namespace {

// MT: 16-row tiles of x in this pass (M <= 16 * MT); P: pairs of 16-row tiles
// per wave. Tile q < P is gate tile q, tile P + q up tile q. blockDim.x = 64 *
// (K slices).
template <int MT, int P, bool BF16>
__global__ void __launch_bounds__(MT * P <= 1 ? 1024 : 512)
    mxfp6_swiglu_kernel(Mxfp6Layout L, int64_t gate_off, int64_t up_off, const uint16_t* __restrict__ x, int M, int K,
                        void* __restrict__ y, int64_t ldy) {
  extern __shared__ float red[];  // [slice][MT * 2 P * 4][64], only with more than one slice
  constexpr int NT = 2 * P, T = MT * NT;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, slices = blockDim.x >> 6;
  const int c = lane & 15, g = lane >> 4;
  const int n0 = blockIdx.x * (16 * P);
  const int nsteps = K >> 7, tail = (K >> 5) & 3;
  const int per = (nsteps + slices - 1) / slices;
  const int s0 = min(wave * per, nsteps), s1 = min(s0 + per, nsteps);
  // first block of this lane's weight row in every tile (the offsets and K are
  // multiples of 32)
  int64_t row_blk[NT];
#pragma unroll
  for (int j = 0; j < P; ++j) {
    row_blk[j] = (gate_off >> 5) + int64_t(n0 + 16 * j + c) * (K >> 5);
    row_blk[P + j] = (up_off >> 5) + int64_t(n0 + 16 * j + c) * (K >> 5);
  }

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
      pos[j].init(L, row_blk[j] + (int64_t(s0) << 2) + g);
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
    // mxfp6_linear.hip's loop: two steps per round on alternating buffers, x loaded ahead of
    // the next step's weights, the last one or two steps peeled.
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
        pos.init(L, row_blk[j] + (int64_t(nsteps) << 2) + g);
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
void launch(bool bf16, dim3 grid, dim3 block, size_t lds, hipStream_t s, const Mxfp6Layout& L, int64_t gate_off,
            int64_t up_off, const uint16_t* x, int M, int K, void* y, int64_t ldy) {
  if (bf16) mxfp6_swiglu_kernel<MT, P, true><<<grid, block, lds, s>>>(L, gate_off, up_off, x, M, K, y, ldy);
  else mxfp6_swiglu_kernel<MT, P, false><<<grid, block, lds, s>>>(L, gate_off, up_off, x, M, K, y, ldy);
}

// The most K slices for `mt` tiles along M and `p` pairs per wave: a wave holds
// the 2 p mt accumulator tiles of a linear wave with 2 p row tiles, so the
// linear kernel's register limit applies (see the header), and the partial
// sums, slices * mt * 2 p KiB, must fit 64 KiB of LDS.
int max_slices(int mt, int p) { return std::min(mt * p <= 1 ? 16 : 8, 32 / (mt * p)); }

// mxfp4_swiglu.hip's rule - 2 pairs (4 tiles, up to 32 rows of x) from 1024
// tiles on, otherwise 1 pair, and thin waves for few rows of x - retuned on
// MI355X over gate/up of llama3-70b (1792 pairs of tiles, K = 8192) and
// llama3-8b (896, K = 4096) at M = 1, 8, 16 and 64 with
// scripts/packed_swiglu_bench.py --sweep (profiles/packed_swiglu/sweep.txt,
// spreads up to 5 %): at M = 1, 1 pair wins at both sizes (102 against 117 us
// and 31.6 against 32.8), and at 1792 pairs it still wins at M = 8 (122 against
// 127 us); at 896 pairs from M = 8 on and at 1792 from M = 16 on 2 pairs win by
// 3 to 15 %. M = 2 .. 7 and sizes between 896 and 1792 pairs were not measured.
int pairs(int m, int mt, int64_t tiles) {
  if (m <= 4 || (m <= 8 && tiles >= 1792)) return 1;
  return mt <= 2 && 2 * tiles >= 1024 && tiles % 2 == 0 ? 2 : 1;
}

// mxfp4_swiglu.hip's targets in waves (8192 for thin waves, here up to 8 rows
// of x: 70b at M = 8 takes 122 us at 8 slices, 125 at 4; 2048 up to 32 rows,
// 1024 beyond), and never more than 8 slices by choice: in the same sweep 16
// slices lost to 8 in every cell (M = 1: 109 against 102 us and 36.5 against
// 31.6). The chosen slices are then the fastest measured or within 4 % of it
// (8b, M = 16: 38.1 us at 8 slices, 36.9 at 4).
int auto_slices(int m, int mt, int p, int64_t wgs, int64_t nsteps) {
  const int64_t target = m <= 8 ? 8192 : mt <= 2 ? 2048 : 1024;
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
DecodePlan mxfp6_swiglu_plan(int m, int64_t N, int64_t K, int split_k, int row_tiles_per_wave) {
  if (m < 1 || m > 64) return DecodePlan{0, 0, 0};
  const int rt = row_tiles_per_wave;
  const int mt = (m + 15) / 16;
  const int p = rt ? std::min(rt, mt <= 2 ? 2 : 1) : pairs(m, mt, N / 16);
  const int64_t wgs = N / 16 / p;
  const int slices = std::min(split_k ? split_k : auto_slices(m, mt, p, wgs, K / 128), max_slices(mt, p));
  return DecodePlan{mt, p, slices};
}

int mxfp6_swiglu_slices(int64_t M, int64_t N, int64_t K) {
  return mxfp6_swiglu_plan(int(std::min<int64_t>(M, 64)), N, K, 0, 0).slices;
}

hipError_t mxfp6_swiglu(const void* packed, int64_t src_bytes, int64_t src_chunk, int64_t gate_off, int64_t up_off,
                        const uint16_t* x, int64_t M, int64_t N, int64_t K, void* y, int64_t ldy, bool y_bf16,
                        int split_k, int row_tiles_per_wave, hipStream_t s) {
  if (src_chunk <= 0 || src_chunk % 1024 || src_bytes <= 0 || src_bytes % 64) return hipErrorInvalidValue;
  if (M < 1 || N < 16 || N % 16 || K < 32 || K % 32 || K > 0x7FFFFF80 || N > 0x7FFFFFF0 || ldy < N)
    return hipErrorInvalidValue;
  if (!param_ok(gate_off, src_bytes, N, K) || !param_ok(up_off, src_bytes, N, K)) return hipErrorInvalidValue;
  if ((reinterpret_cast<uintptr_t>(packed) & 15) || (reinterpret_cast<uintptr_t>(x) & 15) ||
      (reinterpret_cast<uintptr_t>(y) & (y_bf16 ? 1 : 3)))
    return hipErrorInvalidValue;
  if (src_chunk / 64 > 0x7FFFFF00) return hipErrorInvalidValue;  // BlockPos6 counts a chunk's blocks in an int
  if (split_k < 0 || split_k > 16) return hipErrorInvalidValue;
  const int rt = row_tiles_per_wave;
  if ((rt != 0 && rt != 1 && rt != 2) || (rt && N / 16 % rt)) return hipErrorInvalidValue;
  const Mxfp6Layout L = mxfp6_layout(packed, src_bytes, src_chunk);
  const size_t ysz = y_bf16 ? 2 : 4;
  for (int64_t m0 = 0; m0 < M; m0 += 64) {
    const int m = int(std::min<int64_t>(64, M - m0));
    const DecodePlan plan = mxfp6_swiglu_plan(m, N, K, split_k, rt);
    const int mt = plan.mt, p = plan.nt, slices = plan.slices;
    const int64_t wgs = N / 16 / p;
    const dim3 grid{unsigned(wgs)}, block{unsigned(64 * slices)};
    const size_t lds = slices > 1 ? size_t(slices) * mt * 2 * p * 256 * sizeof(float) : 0;
    const uint16_t* xp = x + m0 * K;
    void* yp = static_cast<uint8_t*>(y) + size_t(m0) * size_t(ldy) * ysz;
#define DISSEM_SWIGLU_CASE(MT_, P_) \
  case MT_ * 4 + P_: launch<MT_, P_>(y_bf16, grid, block, lds, s, L, gate_off, up_off, xp, m, int(K), yp, ldy); break
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
