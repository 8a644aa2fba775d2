// Device code shared by the attention kernels (attn_decode.hip,
// attn_decode_mxfp8.hip, attn_prefill.hip): the straight-line pieces between
// their own loads and epilogues, so that all have one set of numerics. All of
// internal linkage, except the declaration of the decode kernels' shared combine launch.
//
// Both kernels run a 32-position step of one KV head on v_mfma_f32_16x16x32_bf16
// with the same lane map (r = lane & 15, g = lane >> 4):
//
//   S^T = K Q^T: K is the A operand - lane holds 8 consecutive d, 32 ks + 8 g +
//   0..7, of position 16 tt + r of the step, for its two 16-position tiles tt -
//   and Q^T the B operand, column r. The accumulators then hold, for ONE column
//   r (a query head in attn_decode, a query row in attn_prefill), the scores of
//   8 of the step's 32 positions: slot j = 4 tt + i is register i of tile tt,
//   position 16 tt + 4 g + i. The online softmax of a column therefore needs two
//   xor shuffles (16, 32) for the maximum and nothing else across lanes; the
//   four lane groups keep partial sums of l, added up once at the end.
//
//   O^T = V^T P^T: those 8 bf16-rounded P are, as they lie, the lane's B operand
//   (the MFMA's sum over k does not care which position sits in which k slot, as
//   long as A agrees). For A a lane holds D / 16 consecutive d, at d = r * (D /
//   16), of its 8 positions and transposes them in registers - one 16-bit pack
//   per operand word - which gives row r of D / 16 tiles of V^T: tile t holds
//   d = row * (D / 16) + t. Accumulator register i of tile t is d = (4 g + i) *
//   (D / 16) + t of column r, so the softmax's rescale factor applies per lane.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels/bf16_bits.h"
#include "kernels/mxfp4_mma.h"

namespace dissem {
namespace kern {

// attn_decode.hip's second launch, which merges the chunk partials (m, l, o) of the workspace in ascending
// chunk order into y; the MXFP8 attention (attn_decode_mxfp8.hip) ends with the same launch.
hipError_t attn_decode_combine(int d, const int32_t* lens, int64_t B, int heads, int capacity, int group,
                               int nchunks, const float* ws_o, const float* ws_ml, void* y, bool y_bf16,
                               hipStream_t s);

namespace {

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// N 32-bit words of bf16 pairs, loaded in one piece.
template <int N>
struct Words;
template <>
struct Words<4> {
  uint32_t w[4];
  __device__ __forceinline__ void load(const uint16_t* p) {
    const uint4 u = *reinterpret_cast<const uint4*>(p);
    w[0] = u.x, w[1] = u.y, w[2] = u.z, w[3] = u.w;
  }
};
template <>
struct Words<2> {
  uint32_t w[2];
  __device__ __forceinline__ void load(const uint16_t* p) {
    const uint2 u = *reinterpret_cast<const uint2*>(p);
    w[0] = u.x, w[1] = u.y;
  }
};
template <>
struct Words<1> {
  uint32_t w[1];
  __device__ __forceinline__ void load(const uint16_t* p) { w[0] = *reinterpret_cast<const uint32_t*>(p); }
};

// What a q . k sum is multiplied by: 1 / sqrt(D), in log2 units for the exp2 below.
__device__ __forceinline__ float attn_score_scale(int D) { return 1.4426950408889634f / sqrtf(float(D)); }

// One step of the online softmax of the lane's column: `s` the 8 scaled scores of its slots, -inf where
// masked; (m, l) the running maximum and the lane group's sum. Gives `alpha`, which rescales what was summed
// before, and the 8 weights exp2(s - m), rounded to bf16, as the B operand's words; l is summed from the
// rounded weights. m stays finite as long as the column's first step holds an unmasked position.
__device__ __forceinline__ void attn_softmax_step(const float (&s)[8], float& m, float& l, float& alpha,
                                                  uint32_t (&pw)[4]) {
  float mx = s[0];
#pragma unroll
  for (int j = 1; j < 8; ++j) mx = fmaxf(mx, s[j]);
  mx = fmaxf(mx, __shfl_xor(mx, 16));
  mx = fmaxf(mx, __shfl_xor(mx, 32));
  const float m_new = fmaxf(m, mx);
  alpha = exp2f(m - m_new);
  float psum = 0.0f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const uint16_t a = f32_to_bf16_rne(exp2f(s[2 * i] - m_new));
    const uint16_t c = f32_to_bf16_rne(exp2f(s[2 * i + 1] - m_new));
    psum += bf16_to_f32(a);
    psum += bf16_to_f32(c);
    pw[i] = uint32_t(a) | (uint32_t(c) << 16);
  }
  l = l * alpha + psum;
  m = m_new;
}

// Row r of tile t of V^T, the A operand's words: element t of each of the lane's 8 pieces `vv` (slot order).
template <int N>
__device__ __forceinline__ void attn_vt_row(const Words<N> (&vv)[8], int t, uint32_t (&aw)[4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const uint32_t lo = vv[2 * i].w[t >> 1], hi = vv[2 * i + 1].w[t >> 1];
    aw[i] = (t & 1) ? ((lo >> 16) | (hi & 0xFFFF0000u)) : ((lo & 0xFFFFu) | (hi << 16));
  }
}

// The end of a single-token attention workgroup of WAVES waves (attn_decode.hip, attn_decode_mxfp8.hip): the
// waves' (m, l, ot) of the KV head's group meet in LDS and are merged in wave order into the partial rows
// blk * group + h of the workspace. Every thread of the workgroup calls it; wave 0 always had a valid step,
// so the maximum is finite.
template <int D, int WAVES>
__device__ __forceinline__ void attn_merge_waves(float m, float l, const f32x4_t (&ot)[D / 16], int group,
                                                 int64_t blk, float* __restrict__ ws_o, float* __restrict__ ws_ml) {
  constexpr int DT = D / 16;
  __shared__ float sm_o[WAVES][16][D];
  __shared__ float sm_m[WAVES][16], sm_l[WAVES][16];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, g = lane >> 4;
  // the lane groups' partial sums of l, the same value in all four
  l += __shfl_xor(l, 16);
  l += __shfl_xor(l, 32);

  // accumulator register i of tile t: row 4 g + i of the tile, d = (4 g + i) * DT + t; column r is the head
#pragma unroll
  for (int t = 0; t < DT; ++t)
#pragma unroll
    for (int i = 0; i < 4; ++i) sm_o[wave][r][(4 * g + i) * DT + t] = ot[t][i];
  if (g == 0) {
    sm_m[wave][r] = m;
    sm_l[wave][r] = l;
  }
  __syncthreads();

  for (int idx = threadIdx.x; idx < group * D; idx += 64 * WAVES) {
    const int h = idx / D, dd = idx % D;
    float mm = sm_m[0][h];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) mm = fmaxf(mm, sm_m[w][h]);
    float o = 0.0f, ll = 0.0f;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
      const float f = exp2f(sm_m[w][h] - mm);  // a wave without a step: exp2(-inf) = 0 times its zeros
      o += f * sm_o[w][h][dd];
      ll += f * sm_l[w][h];
    }
    const int64_t row = blk * group + h;
    ws_o[row * D + dd] = o;
    if (dd == 0) {
      ws_ml[row * 2] = mm;
      ws_ml[row * 2 + 1] = ll;
    }
  }
}

}  // namespace
}  // namespace kern
}  // namespace dissem
