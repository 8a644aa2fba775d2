// The front half of a gated MLP from an MXFP4-packed layer in place:
//   y[m][n] = silu(g[m][n]) * u[m][n],  g = x * Wg^T,  u = x * Wu^T,
// with Wg and Wu two [N, K] parameters of one packed layer (core/mxfp4.h). g and
// u are the sums of mxfp4_linear.hip - same fragment maps, same dequantization
// in registers (mxfp4_cvt.h), same f32 accumulation in v_mfma_f32_16x16x32_bf16,
// same partition of K - but they stay in the accumulators: nothing of size
// [M, N] is written except y, and x is read once for both.
//
// Work: a wave owns P pairs of 16-row tiles, gate tile j and up tile j of the
// same rows n0 + 16 j .. + 15, all 2 P tiles fed from one x fragment. The two
// parameters lie anywhere in the layer, so every tile keeps its own BlockPos.
// The waves of a workgroup split K in steps of 128 exactly as the linear kernel
// does (per = ceil(steps / slices), the K % 128 tail with the last wave) and
// reduce through LDS in the order of the slices: with equal slices, g and u are
// bit for bit what mxfp4_linear returns in f32. The thread that sums g and u of
// an element applies the epilogue
//   y = (g / (1 + expf(-g))) * u
// in f32 with the full-precision expf and the correctly rounded divide: for
// g >= 18 the denominator is 1 and y = g * u, for g <= -89 it is +inf and y = 0;
// no exp(g) / (1 + exp(g)), which is inf / inf from g = 89 on. It runs on M * N
// values against N * K weights; its cost does not show.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kernels/kernels.h"
#include "kernels/mxfp4_cvt.h"
#include "kernels/mxfp4_mma.h"

namespace dissem {
namespace kern {

namespace {

// MT: 16-row tiles of x in this pass (M <= 16 * MT); P: pairs of 16-row tiles
// per wave. Tile q < P is gate tile q, tile P + q up tile q. blockDim.x = 64 *
// (K slices).
template <int MT, int P, bool BF16>
__global__ void __launch_bounds__(MT * P <= 1 ? 1024 : 512)
    mxfp4_swiglu_kernel(Mxfp4Layout L, int64_t gate_off, int64_t up_off, const uint16_t* __restrict__ x, int M, int K,
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
  // multiples of 32; 16 rows are K / 2 blocks)
  int64_t row_blk[NT];
#pragma unroll
  for (int j = 0; j < P; ++j) {
    row_blk[j] = (gate_off + int64_t(n0 + 16 * j + c) * K) >> 5;
    row_blk[P + j] = (up_off + int64_t(n0 + 16 * j + c) * K) >> 5;
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
    BlockPos pos[NT];
    u32x4_t qn[NT];
    uint32_t sn[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      pos[j].init(L, row_blk[j] + 4 * int64_t(s0) + g);
      qn[j] = *reinterpret_cast<const u32x4_t*>(pos[j].q());
      sn[j] = pos[j].scale();
    }
    for (int s = s0; s < s1; ++s) {
      u32x4_t qv[NT];
      uint32_t sb[NT];
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        qv[j] = qn[j];
        sb[j] = sn[j];
      }
      if (s + 1 < s1) {  // the next step's weights are in flight during this one
#pragma unroll
        for (int j = 0; j < NT; ++j) {
          pos[j].advance(L, 4);
          qn[j] = *reinterpret_cast<const u32x4_t*>(pos[j].q());
          sn[j] = pos[j].scale();
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
          uint32_t o[4];
          mxfp4_unpack8(qv[j][u], sb[j], o);
          const bf16x8_t b = as_frag(o);
#pragma unroll
          for (int t = 0; t < MT; ++t)
            acc[t][j] =
                __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a[t][u]), b, acc[t][j], 0, 0, 0);
        }
    }
  }
  if (tail && wave == slices - 1) {  // K % 128: one block per MFMA, 4 B of q per lane
    BlockPos pos[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) pos[j].init(L, row_blk[j] + 4 * int64_t(nsteps));
    for (int tb = 0; tb < tail; ++tb) {
      const int k = ((4 * nsteps + tb) << 5) + 8 * g;
      u32x4_t a[MT];
#pragma unroll
      for (int t = 0; t < MT; ++t) a[t] = live[t] ? *reinterpret_cast<const u32x4_t*>(xrow[t] + k) : zero4;
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        const uint32_t w = *reinterpret_cast<const uint32_t*>(pos[j].q() + 4 * g);
        const uint32_t sb = pos[j].scale();
        uint32_t o[4];
        mxfp4_unpack8(w, sb, o);
        const bf16x8_t b = as_frag(o);
#pragma unroll
        for (int t = 0; t < MT; ++t)
          acc[t][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a[t]), b, acc[t][j], 0, 0, 0);
        if (tb + 1 < tail) pos[j].advance(L, 1);
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
void launch(bool bf16, dim3 grid, dim3 block, size_t lds, hipStream_t s, const Mxfp4Layout& L, int64_t gate_off,
            int64_t up_off, const uint16_t* x, int M, int K, void* y, int64_t ldy) {
  if (bf16) mxfp4_swiglu_kernel<MT, P, true><<<grid, block, lds, s>>>(L, gate_off, up_off, x, M, K, y, ldy);
  else mxfp4_swiglu_kernel<MT, P, false><<<grid, block, lds, s>>>(L, gate_off, up_off, x, M, K, y, ldy);
}

// The most K slices for `mt` tiles along M and `p` pairs per wave: a wave holds
// the 2 p mt accumulator tiles of a linear wave with 2 p row tiles, so the
// linear kernel's register limit applies, and the partial sums must fit
// 64 KiB of LDS.
int max_slices(int mt, int p) { return std::min(mt * p <= 1 ? 16 : 8, 32 / (mt * p)); }

// The linear kernel's rule for 2 N rows - 2 pairs (4 tiles, up to 32 rows of x)
// from 1024 tiles on, otherwise 1 pair - retuned on MI355X over gate/up of
// llama3-70b (1792 pairs of tiles, K = 8192) and llama3-8b (896, K = 4096) with
// scripts/mxfp4_swiglu_bench.py --sweep (profiles/mxfp4_swiglu/sweep.txt): up
// to 4 rows of x hardly any x is read, and at 1792 pairs thin waves win, 1 pair
// at 77 / 79 / 85 us for M = 1 / 2 / 4 against 85 / 86 / 89 with 2; from M = 8 on
// (98 against 95 us) and at 896 pairs for every M (by 1 to 10 %) 2 pairs win.
// Between 896 and 1792 pairs nothing was measured.
int pairs(int m, int mt, int64_t tiles) {
  if (m <= 4 && tiles >= 1792) return 1;
  return mt <= 2 && 2 * tiles >= 1024 && tiles % 2 == 0 ? 2 : 1;
}

// The linear kernel's targets in waves (4096 up to 8 rows of x, 2048 up to 32,
// 1024 beyond), a wave now reading two tiles per pair. In the same sweep the
// chosen slices are the fastest or within 4 % of it, except that the thin waves
// of up to 4 rows want twice as many: 1792 workgroups of 8 slices take 77 us at
// M = 1, of 4 slices 88, so there the target is 8192.
int auto_slices(int m, int mt, int p, int64_t wgs, int64_t nsteps) {
  const int64_t target = m <= 4 ? 8192 : m <= 8 ? 4096 : mt <= 2 ? 2048 : 1024;
  int s = 1;
  while (2 * s <= max_slices(mt, p) && wgs * s < target && 2 * s <= nsteps) s *= 2;
  return s;
}

bool param_ok(int64_t off, int64_t src_bytes, int64_t N, int64_t K) {
  return off >= 0 && off % 32 == 0 && N <= (src_bytes / 2 - off) / K;
}

}  // namespace

// One pass of m rows: the instantiation and the K slices, the only place the launcher below takes them from
// (kernels.h, DecodePlan).
DecodePlan mxfp4_swiglu_plan(int m, int64_t N, int64_t K, int split_k, int row_tiles_per_wave) {
  if (m < 1 || m > 64) return DecodePlan{0, 0, 0};
  const int rt = row_tiles_per_wave;
  const int mt = (m + 15) / 16;
  const int p = rt ? std::min(rt, mt <= 2 ? 2 : 1) : pairs(m, mt, N / 16);
  const int64_t wgs = N / 16 / p;
  const int slices = std::min(split_k ? split_k : auto_slices(m, mt, p, wgs, K / 128), max_slices(mt, p));
  return DecodePlan{mt, p, slices};
}

int mxfp4_swiglu_slices(int64_t M, int64_t N, int64_t K) {
  return mxfp4_swiglu_plan(int(std::min<int64_t>(M, 64)), N, K, 0, 0).slices;
}

hipError_t mxfp4_swiglu(const void* packed, int64_t src_bytes, int64_t src_chunk, int64_t gate_off, int64_t up_off,
                        const uint16_t* x, int64_t M, int64_t N, int64_t K, void* y, int64_t ldy, bool y_bf16,
                        int split_k, int row_tiles_per_wave, hipStream_t s) {
  if (src_chunk <= 0 || src_chunk % 1024 || src_bytes <= 0 || src_bytes % 64) return hipErrorInvalidValue;
  if (M < 1 || N < 16 || N % 16 || K < 32 || K % 32 || K > 0x7FFFFF80 || N > 0x7FFFFFF0 || ldy < N)
    return hipErrorInvalidValue;
  if (!param_ok(gate_off, src_bytes, N, K) || !param_ok(up_off, src_bytes, N, K)) return hipErrorInvalidValue;
  if ((reinterpret_cast<uintptr_t>(packed) & 15) || (reinterpret_cast<uintptr_t>(x) & 15) ||
      (reinterpret_cast<uintptr_t>(y) & (y_bf16 ? 1 : 3)))
    return hipErrorInvalidValue;
  if (src_chunk / 64 > 0x7FFFFFFF) return hipErrorInvalidValue;
  if (split_k < 0 || split_k > 16) return hipErrorInvalidValue;
  const int rt = row_tiles_per_wave;
  if ((rt != 0 && rt != 1 && rt != 2) || (rt && N / 16 % rt)) return hipErrorInvalidValue;
  const Mxfp4Layout L = mxfp4_layout(packed, src_bytes, src_chunk);
  const size_t ysz = y_bf16 ? 2 : 4;
  for (int64_t m0 = 0; m0 < M; m0 += 64) {
    const int m = int(std::min<int64_t>(64, M - m0));
    const DecodePlan plan = mxfp4_swiglu_plan(m, N, K, split_k, rt);
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
