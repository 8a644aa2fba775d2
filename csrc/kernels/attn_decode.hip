// One decode step's attention against a KV cache in HBM (kernels.h has the
// contract): rope_append rotates q and k at each sequence's position with the
// cache's cos / sin tables and appends k and v to the caches; attn_decode is
// grouped-query attention of one query token per sequence.
//
// attn_decode, the partial kernel: a workgroup of four waves serves one
// (sequence, KV head, chunk of kAttnDecodeChunk positions) and all the query
// heads of that KV head, padded to the 16 of an MFMA tile, so a K and a V row
// are fetched once per KV head. K and V go from global memory straight to the
// MFMA operands, 16 B a lane, with no LDS in between:
//
//   S^T = K Q^T on v_mfma_f32_16x16x32_bf16, K the A operand (a lane loads 8
//   consecutive d of one position), Q^T the B operand, loaded once. A lane then
//   holds, for ONE head (lane & 15), the scores of 8 of the step's 32 positions,
//   so the online softmax needs two xor shuffles for the maximum and nothing
//   else across lanes.
//
//   O^T = V^T P^T: those 8 bf16-rounded P are, as they lie, the lane's B operand
//   (the MFMA's sum over k does not care which position sits in which k slot, as
//   long as A agrees). For A a lane loads D / 16 consecutive d of its 8
//   positions and transposes them in registers - one 16-bit pack per operand
//   word - which gives row (lane & 15) of D / 16 tiles of V^T: tile t holds
//   d = row * (D / 16) + t. The accumulator's column is the head again, so the
//   softmax's rescale factor applies per lane.
//
// Wave w takes the 32-position steps w and w + 4 of the chunk; the four waves'
// (m, l, o) meet in LDS and are merged in wave order into the chunk's partial
// in the workspace. The combine kernel merges a sequence's chunks in ascending
// order. Every load is predicated by its position < lens[b] (clamped to the
// capacity): a position behind the length is never read, its score is -inf and
// its V operand zero. Nothing depends on the batch, the other sequences,
// max_len or the capacity except which workgroups exist.
#include <hip/hip_runtime.h>

#include "kernels/attn_decode_plan.h"
#include "kernels/kernels.h"
#include "kernels/mxfp4_mma.h"

namespace dissem {
namespace kern {

namespace {

constexpr int kC = kAttnDecodeChunk;
constexpr int kWaves = 4;
constexpr int kStep = 32;                         // positions of one wave step
constexpr int kStepsPerWave = kC / (kStep * kWaves);
static_assert(kC == kStep * kWaves * kStepsPerWave, "a chunk is a whole number of steps per wave");

__device__ __forceinline__ float bf16_to_f32(uint16_t h) { return __uint_as_float(uint32_t(h) << 16); }

// ---------------------------------------------------------------- rope_append
template <int D>
__global__ void __launch_bounds__(D) rope_append_kernel(const uint16_t* __restrict__ q, int64_t ldq,
                                                        const uint16_t* __restrict__ k, int64_t ldk,
                                                        const uint16_t* __restrict__ v, int64_t ldv,
                                                        const int32_t* __restrict__ pos, const float* __restrict__ cos,
                                                        const float* __restrict__ sin, int capacity, int heads,
                                                        int kv_heads, uint16_t* __restrict__ q_out,
                                                        uint16_t* __restrict__ k_cache, uint16_t* __restrict__ v_cache) {
  const int64_t b = blockIdx.x;
  const int slot = blockIdx.y, i = threadIdx.x;
  const int p = pos[b];
  const bool ok = p >= 0 && p < capacity;
  if (slot >= heads + kv_heads) {  // v: copied as it is
    if (!ok) return;
    const int h = slot - heads - kv_heads;
    v_cache[((b * kv_heads + h) * capacity + p) * D + i] = v[b * ldv + int64_t(h) * D + i];
    return;
  }
  const bool is_q = slot < heads;
  const int h = is_q ? slot : slot - heads;
  uint16_t* dst = is_q ? q_out + (b * heads + h) * D : k_cache + ((b * kv_heads + h) * capacity + (ok ? p : 0)) * D;
  if (!ok) {
    if (is_q) dst[i] = 0;  // no table row for this position: a defined q row, nothing in the caches
    return;
  }
  const uint16_t* src = is_q ? q + b * ldq + int64_t(h) * D : k + b * ldk + int64_t(h) * D;
  const float x = bf16_to_f32(src[i]);
  const float o = bf16_to_f32(src[i < D / 2 ? i + D / 2 : i - D / 2]);
  const float xr = i < D / 2 ? -o : o;
  const int64_t t = int64_t(p) * D + i;
  // x * cos + rot(x) * sin: two rounded products and one rounded sum, never an FMA
  dst[i] = f32_to_bf16_rne(__fadd_rn(__fmul_rn(x, cos[t]), __fmul_rn(xr, sin[t])));
}

// ---------------------------------------------------------------- attn_decode
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

template <int D>
__global__ void __launch_bounds__(64 * kWaves) attn_partial_kernel(const uint16_t* __restrict__ q,
                                                                   const uint16_t* __restrict__ k_cache,
                                                                   const uint16_t* __restrict__ v_cache,
                                                                   const int32_t* __restrict__ lens, int capacity,
                                                                   int heads, int kv_heads, int group, int nchunks,
                                                                   float* __restrict__ ws_o, float* __restrict__ ws_ml) {
  constexpr int KS = D / 32;  // MFMA k steps of q . k
  constexpr int DT = D / 16;  // 16-row tiles of V^T; also the d a lane loads of a V row
  __shared__ float sm_o[kWaves][16][D];
  __shared__ float sm_m[kWaves][16], sm_l[kWaves][16];

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int64_t blk = blockIdx.x;  // (b * kv_heads + kvh) * nchunks + chunk
  const int chunk = int(blk % nchunks);
  const int64_t bh = blk / nchunks;
  const int kvh = int(bh % kv_heads);
  const int64_t b = bh / kv_heads;
  int len = lens[b];
  len = len < 0 ? 0 : (len > capacity ? capacity : len);
  const int c0 = chunk * kC;
  if (c0 >= len) return;  // the whole chunk lies behind the length: nothing is loaded

  const uint16_t* kb = k_cache + bh * capacity * D;
  const uint16_t* vb = v_cache + bh * capacity * D;

  // Q^T, the B operand of S^T: lane holds Q[head r][32 ks + 8 g + 0..7]; heads past the group are zero rows
  bf16x8_t qf[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    Words<4> w;
    if (r < group) w.load(q + (b * heads + int64_t(kvh) * group + r) * D + 32 * ks + 8 * g);
    else w.w[0] = w.w[1] = w.w[2] = w.w[3] = 0;
    qf[ks] = as_frag(w.w);
  }

  const float sc = 1.4426950408889634f / sqrtf(float(D));  // scores in log2 units: exp2 below
  float m = -INFINITY, l = 0.0f;
  f32x4_t ot[DT];
#pragma unroll
  for (int t = 0; t < DT; ++t) ot[t] = f32x4_t{0.0f, 0.0f, 0.0f, 0.0f};

#pragma unroll
  for (int it = 0; it < kStepsPerWave; ++it) {
    const int p0 = c0 + kStep * (wave + kWaves * it);
    if (p0 >= len) break;  // wave-uniform
    // scores of the step's two 16-position tiles: rows are positions, columns heads
    f32x4_t st[2];
#pragma unroll
    for (int tt = 0; tt < 2; ++tt) {
      const int pk = p0 + 16 * tt + r;
      st[tt] = f32x4_t{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        Words<4> w;
        if (pk < len) w.load(kb + int64_t(pk) * D + 32 * ks + 8 * g);
        else w.w[0] = w.w[1] = w.w[2] = w.w[3] = 0;
        st[tt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_frag(w.w), qf[ks], st[tt], 0, 0, 0);
      }
    }
    // V of the lane's 8 positions (slot j: tile j >> 2, accumulator register j & 3), DT values at d = r * DT
    Words<DT / 2> vv[8];
    bool valid[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int pv = p0 + 16 * (j >> 2) + 4 * g + (j & 3);
      valid[j] = pv < len;
#pragma unroll
      for (int i = 0; i < DT / 2; ++i) vv[j].w[i] = 0;  // a position behind the length is a zero row, never a load
      if (valid[j]) vv[j].load(vb + int64_t(pv) * D + r * DT);
    }
    // online softmax for head r over the step
    float s[8];
    float mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      s[j] = valid[j] ? st[j >> 2][j & 3] * sc : -INFINITY;
      mx = fmaxf(mx, s[j]);
    }
    mx = fmaxf(mx, __shfl_xor(mx, 16));
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    const float m_new = fmaxf(m, mx);  // finite: position p0 is valid
    const float alpha = exp2f(m - m_new);
    uint32_t pw[4];
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
    const bf16x8_t pf = as_frag(pw);
#pragma unroll
    for (int t = 0; t < DT; ++t) {
      // row r of tile t of V^T: element t of each of the 8 loaded pieces
      uint32_t aw[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const uint32_t lo = vv[2 * i].w[t >> 1], hi = vv[2 * i + 1].w[t >> 1];
        aw[i] = (t & 1) ? ((lo >> 16) | (hi & 0xFFFF0000u)) : ((lo & 0xFFFFu) | (hi << 16));
      }
      ot[t] = ot[t] * alpha;
      ot[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_frag(aw), pf, ot[t], 0, 0, 0);
    }
  }
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

  // the four waves in wave order; wave 0 always had a valid step, so the maximum is finite
  for (int idx = threadIdx.x; idx < group * D; idx += 64 * kWaves) {
    const int h = idx / D, dd = idx % D;
    float mm = sm_m[0][h];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) mm = fmaxf(mm, sm_m[w][h]);
    float o = 0.0f, ll = 0.0f;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
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

template <int D, bool BF16>
__global__ void __launch_bounds__(D) attn_combine_kernel(const int32_t* __restrict__ lens, int capacity, int heads,
                                                         int group, int nchunks, const float* __restrict__ ws_o,
                                                         const float* __restrict__ ws_ml, void* __restrict__ y) {
  const int64_t bhq = blockIdx.x;  // b * heads + head
  const int64_t b = bhq / heads;
  const int h = int(bhq % heads), dd = threadIdx.x;
  int len = lens[b];
  len = len < 0 ? 0 : (len > capacity ? capacity : len);
  int nc = (len + kC - 1) / kC;
  if (nc > nchunks) nc = nchunks;  // lens above max_len break the caller's promise; stay inside the workspace
  const int64_t out = bhq * D + dd;
  if (nc == 0) {
    store_y<BF16>(y, out, 0.0f);
    return;
  }
  const int kv_heads = heads / group;
  // partial row of chunk c: ((b * kv_heads + kvh) * nchunks + c) * group + head in group
  const int64_t row0 = (b * kv_heads + h / group) * nchunks * group + h % group;
  float mm = -INFINITY;
  for (int c = 0; c < nc; ++c) mm = fmaxf(mm, ws_ml[(row0 + int64_t(c) * group) * 2]);
  float o = 0.0f, ll = 0.0f;
  for (int c = 0; c < nc; ++c) {  // ascending chunk order
    const int64_t row = row0 + int64_t(c) * group;
    const float f = exp2f(ws_ml[row * 2] - mm);
    o += f * ws_o[row * D + dd];
    ll += f * ws_ml[row * 2 + 1];
  }
  store_y<BF16>(y, out, o / ll);
}

template <int D>
hipError_t launch_rope(const uint16_t* q, int64_t ldq, const uint16_t* k, int64_t ldk, const uint16_t* v, int64_t ldv,
                       const int32_t* pos, const float* cos, const float* sin, int64_t B, int heads, int kv_heads,
                       int capacity, uint16_t* q_out, uint16_t* k_cache, uint16_t* v_cache, hipStream_t s) {
  rope_append_kernel<D><<<dim3(unsigned(B), unsigned(heads + 2 * kv_heads)), D, 0, s>>>(
      q, ldq, k, ldk, v, ldv, pos, cos, sin, capacity, heads, kv_heads, q_out, k_cache, v_cache);
  return hipGetLastError();
}

template <int D>
hipError_t launch_attn(const uint16_t* q, const uint16_t* k_cache, const uint16_t* v_cache, const int32_t* lens,
                       int64_t B, int heads, int kv_heads, int capacity, const AttnDecodePlan& p, float* ws, void* y,
                       bool y_bf16, hipStream_t s) {
  float* ws_o = ws;
  float* ws_ml = ws + p.o_floats;
  attn_partial_kernel<D><<<unsigned(p.blocks), 64 * kWaves, 0, s>>>(q, k_cache, v_cache, lens, capacity, heads,
                                                                    kv_heads, p.group, int(p.nchunks), ws_o, ws_ml);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const unsigned grid = unsigned(B * heads);
  if (y_bf16)
    attn_combine_kernel<D, true><<<grid, D, 0, s>>>(lens, capacity, heads, p.group, int(p.nchunks), ws_o, ws_ml, y);
  else
    attn_combine_kernel<D, false><<<grid, D, 0, s>>>(lens, capacity, heads, p.group, int(p.nchunks), ws_o, ws_ml, y);
  return hipGetLastError();
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

hipError_t attn_rope_append(const uint16_t* q, int64_t ldq, const uint16_t* k, int64_t ldk, const uint16_t* v,
                            int64_t ldv, const int32_t* pos, const float* cos, const float* sin, int64_t B,
                            int64_t heads, int64_t kv_heads, int64_t d, int64_t capacity, uint16_t* q_out,
                            uint16_t* k_cache, uint16_t* v_cache, hipStream_t s) {
  if (!attn_rope_plan(B, heads, kv_heads, d, capacity, ldq, ldk, ldv)) return hipErrorInvalidValue;
  if (!q || !k || !v || !pos || !cos || !sin || !q_out || !k_cache || !v_cache) return hipErrorInvalidValue;
  const int h = int(heads), kv = int(kv_heads), cap = int(capacity);
  if (d == 32) return launch_rope<32>(q, ldq, k, ldk, v, ldv, pos, cos, sin, B, h, kv, cap, q_out, k_cache, v_cache, s);
  if (d == 64) return launch_rope<64>(q, ldq, k, ldk, v, ldv, pos, cos, sin, B, h, kv, cap, q_out, k_cache, v_cache, s);
  return launch_rope<128>(q, ldq, k, ldk, v, ldv, pos, cos, sin, B, h, kv, cap, q_out, k_cache, v_cache, s);
}

int64_t attn_decode_workspace_bytes(int64_t B, int64_t heads, int64_t kv_heads, int64_t d, int64_t capacity,
                                    int64_t max_len) {
  const AttnDecodePlan p = attn_decode_plan(B, heads, kv_heads, d, capacity, max_len);
  return p.ok ? p.ws_bytes : -1;
}

hipError_t attn_decode(const uint16_t* q, const uint16_t* k_cache, const uint16_t* v_cache, const int32_t* lens,
                       int64_t B, int64_t heads, int64_t kv_heads, int64_t d, int64_t capacity, int64_t max_len,
                       void* ws, int64_t ws_bytes, void* y, bool y_bf16, hipStream_t s) {
  const AttnDecodePlan p = attn_decode_plan(B, heads, kv_heads, d, capacity, max_len);
  if (!p.ok || B * heads > 0x7FFFFFFF || ws_bytes < p.ws_bytes) return hipErrorInvalidValue;
  if (!q || !k_cache || !v_cache || !lens || !ws || !y) return hipErrorInvalidValue;
  if (!aligned16(q) || !aligned16(k_cache) || !aligned16(v_cache) || !aligned16(ws)) return hipErrorInvalidValue;
  const int h = int(heads), kv = int(kv_heads), cap = int(capacity);
  float* w = static_cast<float*>(ws);
  if (d == 32) return launch_attn<32>(q, k_cache, v_cache, lens, B, h, kv, cap, p, w, y, y_bf16, s);
  if (d == 64) return launch_attn<64>(q, k_cache, v_cache, lens, B, h, kv, cap, p, w, y, y_bf16, s);
  return launch_attn<128>(q, k_cache, v_cache, lens, B, h, kv, cap, p, w, y, y_bf16, s);
}

}  // namespace kern
}  // namespace dissem
