// One decode step's attention against an MXFP8 KV cache in HBM (kernels.h has
// the contract): OCP e4m3fn codes uint8 [B, kv_heads, capacity, d] and one E8M0
// scale byte per 32 d, uint8 [B, kv_heads, capacity, d / 32] - core/mxfp8_act.h's
// format, 33/64 of the bf16 cache's bytes at d = 128. attn_rope_append_mxfp8
// rotates q and k, quantizes k and v and appends them; attn_decode_mxfp8 attends.
//
// attn_decode_mxfp8 is attn_decode.hip's decomposition - a workgroup of four
// waves per (sequence, KV head, chunk of kAttnDecodeChunk positions), wave w the
// 32-position steps w and w + 4, attn_softmax_step, attn_merge_waves, the same
// workspace and the same combine launch - with an operand path of its own. An
// e4m3 code times a power of two is a bf16 value, so codes are dequantized in
// registers (fp8x2_to_bf16x2, one v_cvt_scalef32_pk_bf16_fp8 per pair) into the
// very operand words of the bf16 MFMA; no LDS in between. Lane (r = lane & 15,
// g = lane >> 4), the layout chosen so that no load is narrower than it has to be:
//
//   K, the A operand of S^T = K Q^T: 16 bytes of codes of position r, d [64 h +
//   16 g, + 16) for h < D / 64. The first 8 feed MFMA k-step 2 h, the last 8
//   k-step 2 h + 1, and Q^T is loaded once in the same permutation of d: the
//   MFMA sums over its k slots, so only the agreement of A and B matters. Two K
//   loads a position at d = 128 where 8 consecutive d a k-step would take four
//   of 8 bytes. All 16 codes lie in scale block 2 h + g / 2; the position's
//   scale bytes are one 4-byte (d = 64: 2-byte) load.
//   V, V^T the A operand of O^T = V^T P^T: the D / 16 consecutive d at r * (D /
//   16) of the lane's 8 positions, 8 (d = 64: 4) bytes each, which are attn_mma.h's
//   Words after dequantization; all in block r * (D / 16) / 32, one byte load.
//
// Every load of a code or a scale byte is predicated by its position < lens[b]
// (clamped to the capacity): a position behind the length reads neither tensor,
// its score is -inf and its V operand zero. Chunk and step boundaries are the
// bf16 kernel's, so a row's bits depend on the batch, the slot, max_len and the
// capacity as little as there.
//
// attn_rope_append_mxfp8, ONE launch: rope_append_seq's thread map - a thread
// owns 8 d of the lower half of a head and their partners of the upper half,
// 16-byte loads - so four adjacent lanes hold one 32-block of each half and
// fp8_pack8<4> (the quantizer of mxfp8_act.hip, byte for byte the host codec)
// gives the thread's 8 codes, an 8-byte store, and the block's scale. A
// workgroup of kAttnRopeMxThreads threads takes that many (head, piece) items of
// one sequence over q, k and v heads alike.
#include <hip/hip_runtime.h>

#include "kernels/attn_mma.h"
#include "kernels/attn_plan.h"
#include "kernels/fp8_cvt.h"
#include "kernels/fp8_pack.h"
#include "kernels/kernels.h"

namespace dissem {
namespace kern {

namespace {

constexpr int kC = kAttnDecodeChunk;
constexpr int kWaves = 4;
constexpr int kStep = 32;  // positions of one wave step
constexpr int kStepsPerWave = kC / (kStep * kWaves);
static_assert(kC == kStep * kWaves * kStepsPerWave, "a chunk is a whole number of steps per wave");

// ---------------------------------------------------------------- attn_decode_mxfp8
template <int D>
__global__ void __launch_bounds__(64 * kWaves)
    attn_partial_mxfp8_kernel(const uint16_t* __restrict__ q, const uint8_t* __restrict__ k_codes,
                              const uint8_t* __restrict__ k_scales, const uint8_t* __restrict__ v_codes,
                              const uint8_t* __restrict__ v_scales, const int32_t* __restrict__ lens, int capacity,
                              int heads, int kv_heads, int group, int nchunks, float* __restrict__ ws_o,
                              float* __restrict__ ws_ml) {
  constexpr int KS = D / 32;  // MFMA k steps of q . k
  constexpr int DT = D / 16;  // 16-row tiles of V^T; also the d (and code bytes) a lane loads of a V row
  constexpr int NB = D / 32;  // scale bytes of a row
  constexpr int NH = D / 64;  // 16-byte K loads of a position

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

  const uint8_t* kcb = k_codes + bh * capacity * D;
  const uint8_t* vcb = v_codes + bh * capacity * D;
  const uint8_t* ksb = k_scales + bh * capacity * NB;
  const uint8_t* vsb = v_scales + bh * capacity * NB + (r * DT) / 32;  // the lane's V block

  // Q^T, the B operand of S^T, in K's permutation of d: k-step 2 h + e holds Q[head r][64 h + 16 g + 8 e + 0..7];
  // heads past the group are zero rows
  bf16x8_t qf[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    Words<4> w;
    if (r < group) w.load(q + (b * heads + int64_t(kvh) * group + r) * D + 64 * (ks >> 1) + 16 * g + 8 * (ks & 1));
    else w.w[0] = w.w[1] = w.w[2] = w.w[3] = 0;
    qf[ks] = as_frag(w.w);
  }

  const float sc = attn_score_scale(D);
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
      const bool kvalid = pk < len;
      uint32_t sw = 0;  // the position's scale bytes, block j in byte j
      if (kvalid) {
        if constexpr (NB == 4) sw = *reinterpret_cast<const uint32_t*>(ksb + int64_t(pk) * NB);
        else sw = *reinterpret_cast<const uint16_t*>(ksb + int64_t(pk) * NB);
      }
      st[tt] = f32x4_t{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
      for (int h = 0; h < NH; ++h) {
        uint4 c = make_uint4(0, 0, 0, 0);  // behind the length: zero operands without a conversion
        uint32_t a0[4] = {0, 0, 0, 0}, a1[4] = {0, 0, 0, 0};
        if (kvalid) {
          c = *reinterpret_cast<const uint4*>(kcb + int64_t(pk) * D + 64 * h + 16 * g);
          const float s = e8m0_scale(sw >> (8 * (2 * h + (g >> 1))));
          dequant4(c.x, s, a0[0], a0[1]);
          dequant4(c.y, s, a0[2], a0[3]);
          dequant4(c.z, s, a1[0], a1[1]);
          dequant4(c.w, s, a1[2], a1[3]);
        }
        st[tt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_frag(a0), qf[2 * h], st[tt], 0, 0, 0);
        st[tt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_frag(a1), qf[2 * h + 1], st[tt], 0, 0, 0);
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
      if (valid[j]) {
        const float s = e8m0_scale(vsb[int64_t(pv) * NB]);
        const uint8_t* src = vcb + int64_t(pv) * D + r * DT;
        if constexpr (DT == 8) {
          const uint2 c = *reinterpret_cast<const uint2*>(src);
          dequant4(c.x, s, vv[j].w[0], vv[j].w[1]);
          dequant4(c.y, s, vv[j].w[2], vv[j].w[3]);
        } else {
          dequant4(*reinterpret_cast<const uint32_t*>(src), s, vv[j].w[0], vv[j].w[1]);
        }
      }
    }
    // online softmax for head r over the step; m stays finite: position p0 is valid
    float s[8], alpha;
#pragma unroll
    for (int j = 0; j < 8; ++j) s[j] = valid[j] ? st[j >> 2][j & 3] * sc : -INFINITY;
    uint32_t pw[4];
    float mi = m, li = l;  // through copies, as in attn_decode.hip
    attn_softmax_step(s, mi, li, alpha, pw);
    m = mi, l = li;
    const bf16x8_t pf = as_frag(pw);
#pragma unroll
    for (int t = 0; t < DT; ++t) {
      uint32_t aw[4];
      attn_vt_row(vv, t, aw);
      ot[t] = ot[t] * alpha;
      ot[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_frag(aw), pf, ot[t], 0, 0, 0);
    }
  }
  attn_merge_waves<D, kWaves>(m, l, ot, group, blk, ws_o, ws_ml);
}

// ---------------------------------------------------------------- rope_append_mxfp8
template <int D>
__global__ void __launch_bounds__(kAttnRopeMxThreads)
    rope_append_mxfp8_kernel(const uint16_t* __restrict__ q, int64_t ldq, const uint16_t* __restrict__ k, int64_t ldk,
                             const uint16_t* __restrict__ v, int64_t ldv, const int32_t* __restrict__ pos,
                             const float* __restrict__ cos, const float* __restrict__ sin, int items, int capacity,
                             int heads, int kv_heads, uint16_t* __restrict__ q_out, uint8_t* __restrict__ k_codes,
                             uint8_t* __restrict__ k_scales, uint8_t* __restrict__ v_codes,
                             uint8_t* __restrict__ v_scales) {
  constexpr int L = D / 16;  // threads of a head row: 4 or 8, so a quad of lanes never spans two rows
  const int64_t b = blockIdx.x;
  const int item = int(blockIdx.y) * kAttnRopeMxThreads + int(threadIdx.x);
  const bool active = item < items;
  const int c = item % L, slot = item / L;
  const int lo = 8 * c, hi = D / 2 + 8 * c;
  const bool is_q = slot < heads, is_k = !is_q && slot < heads + kv_heads;
  const int hh = is_q ? slot : (is_k ? slot - heads : slot - heads - kv_heads);
  const int p = pos[b];
  if (p < 0 || p >= capacity) {  // the whole workgroup: a defined q row, nothing in the caches
    if (active && is_q) {
      uint16_t* dst = q_out + (b * heads + hh) * D;
      *reinterpret_cast<uint4*>(dst + lo) = uint4{0u, 0u, 0u, 0u};
      *reinterpret_cast<uint4*>(dst + hi) = uint4{0u, 0u, 0u, 0u};
    }
    return;
  }
  union V8 {
    uint4 u;
    uint16_t e[8];
  };
  union F8 {
    float4 f4[2];
    float e[8];
  };
  V8 ol, oh;  // what goes out: q and k rotated, v as it is
  ol.u = oh.u = uint4{0u, 0u, 0u, 0u};
  if (active) {
    const uint16_t* src = is_q ? q + b * ldq : (is_k ? k + b * ldk : v + b * ldv);
    src += int64_t(hh) * D;
    ol.u = *reinterpret_cast<const uint4*>(src + lo);
    oh.u = *reinterpret_cast<const uint4*>(src + hi);
    if (is_q || is_k) {
      const V8 xl = ol, xh = oh;
      F8 cl, ch, sl, sh;
      const float* ct = cos + int64_t(p) * D;
      const float* stb = sin + int64_t(p) * D;
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        cl.f4[i] = *reinterpret_cast<const float4*>(ct + lo + 4 * i);
        ch.f4[i] = *reinterpret_cast<const float4*>(ct + hi + 4 * i);
        sl.f4[i] = *reinterpret_cast<const float4*>(stb + lo + 4 * i);
        sh.f4[i] = *reinterpret_cast<const float4*>(stb + hi + 4 * i);
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float a = bf16_to_f32(xl.e[e]), z = bf16_to_f32(xh.e[e]);
        // x * cos + rot(x) * sin, rot = (-upper, lower): two rounded products and one rounded sum, never an FMA
        ol.e[e] = f32_to_bf16_rne(__fadd_rn(__fmul_rn(a, cl.e[e]), __fmul_rn(-z, sl.e[e])));
        oh.e[e] = f32_to_bf16_rne(__fadd_rn(__fmul_rn(z, ch.e[e]), __fmul_rn(a, sh.e[e])));
      }
    }
    if (is_q) {
      uint16_t* dst = q_out + (b * heads + hh) * D;
      *reinterpret_cast<uint4*>(dst + lo) = ol.u;
      *reinterpret_cast<uint4*>(dst + hi) = oh.u;
    }
  }
  // fp8_pack8 reduces over the quad with DPP: every lane of the wave arrives here, q lanes and lanes without an
  // item with zeros. A quad holds block lo / 32 of the lower half and block hi / 32 of the upper.
  const bool to_cache = active && !is_q;
  const uint4 zero = uint4{0u, 0u, 0u, 0u};
  int el, eh;
  const uint2 cl = fp8_pack8<4>(to_cache ? ol.u : zero, el);
  const uint2 ch = fp8_pack8<4>(to_cache ? oh.u : zero, eh);
  if (!to_cache) return;
  const int64_t row = (b * kv_heads + hh) * capacity + p;
  uint8_t* codes = (is_k ? k_codes : v_codes) + row * D;
  uint8_t* scales = (is_k ? k_scales : v_scales) + row * (D / 32);
  *reinterpret_cast<uint2*>(codes + lo) = cl;
  *reinterpret_cast<uint2*>(codes + hi) = ch;
  if ((threadIdx.x & 3) == 0) {
    scales[lo / 32] = uint8_t(127 + el);
    scales[hi / 32] = uint8_t(127 + eh);
  }
}

template <int D>
hipError_t launch_attn_mxfp8(const uint16_t* q, const uint8_t* k_codes, const uint8_t* k_scales,
                             const uint8_t* v_codes, const uint8_t* v_scales, const int32_t* lens, int64_t B,
                             int heads, int kv_heads, int capacity, const AttnDecodePlan& p, float* ws, void* y,
                             bool y_bf16, hipStream_t s) {
  float* ws_o = ws;
  float* ws_ml = ws + p.o_floats;
  attn_partial_mxfp8_kernel<D><<<unsigned(p.blocks), 64 * kWaves, 0, s>>>(
      q, k_codes, k_scales, v_codes, v_scales, lens, capacity, heads, kv_heads, p.group, int(p.nchunks), ws_o, ws_ml);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  return attn_decode_combine(D, lens, B, heads, capacity, p.group, int(p.nchunks), ws_o, ws_ml, y, y_bf16, s);
}

template <int D>
hipError_t launch_rope_mxfp8(const uint16_t* q, int64_t ldq, const uint16_t* k, int64_t ldk, const uint16_t* v,
                             int64_t ldv, const int32_t* pos, const float* cos, const float* sin, int64_t B,
                             const AttnRopeMxPlan& p, int heads, int kv_heads, int capacity, uint16_t* q_out,
                             uint8_t* k_codes, uint8_t* k_scales, uint8_t* v_codes, uint8_t* v_scales, hipStream_t s) {
  rope_append_mxfp8_kernel<D><<<dim3(unsigned(B), unsigned(p.grid_y)), kAttnRopeMxThreads, 0, s>>>(
      q, ldq, k, ldk, v, ldv, pos, cos, sin, p.items, capacity, heads, kv_heads, q_out, k_codes, k_scales, v_codes,
      v_scales);
  return hipGetLastError();
}

inline bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }

}  // namespace

hipError_t attn_rope_append_mxfp8(const uint16_t* q, int64_t ldq, const uint16_t* k, int64_t ldk, const uint16_t* v,
                                  int64_t ldv, const int32_t* pos, const float* cos, const float* sin, int64_t B,
                                  int64_t heads, int64_t kv_heads, int64_t d, int64_t capacity, uint16_t* q_out,
                                  uint8_t* k_codes, uint8_t* k_scales, uint8_t* v_codes, uint8_t* v_scales,
                                  hipStream_t s) {
  const AttnRopeMxPlan p = attn_rope_mxfp8_plan(B, heads, kv_heads, d, capacity, ldq, ldk, ldv);
  if (!p.ok) return hipErrorInvalidValue;
  if (!q || !k || !v || !pos || !cos || !sin || !q_out || !k_codes || !k_scales || !v_codes || !v_scales)
    return hipErrorInvalidValue;
  if (!aligned16(q) || !aligned16(k) || !aligned16(v) || !aligned16(cos) || !aligned16(sin) || !aligned16(q_out) ||
      !aligned16(k_codes) || !aligned16(v_codes))
    return hipErrorInvalidValue;
  const int h = int(heads), kv = int(kv_heads), cap = int(capacity);
  if (d == 64)
    return launch_rope_mxfp8<64>(q, ldq, k, ldk, v, ldv, pos, cos, sin, B, p, h, kv, cap, q_out, k_codes, k_scales,
                                 v_codes, v_scales, s);
  return launch_rope_mxfp8<128>(q, ldq, k, ldk, v, ldv, pos, cos, sin, B, p, h, kv, cap, q_out, k_codes, k_scales,
                                v_codes, v_scales, s);
}

hipError_t attn_decode_mxfp8(const uint16_t* q, const uint8_t* k_codes, const uint8_t* k_scales,
                             const uint8_t* v_codes, const uint8_t* v_scales, const int32_t* lens, int64_t B,
                             int64_t heads, int64_t kv_heads, int64_t d, int64_t capacity, int64_t max_len, void* ws,
                             int64_t ws_bytes, void* y, bool y_bf16, hipStream_t s) {
  const AttnDecodePlan p = attn_decode_mxfp8_plan(B, heads, kv_heads, d, capacity, max_len);
  if (!p.ok || B * heads > 0x7FFFFFFF || ws_bytes < p.ws_bytes) return hipErrorInvalidValue;
  if (!q || !k_codes || !k_scales || !v_codes || !v_scales || !lens || !ws || !y) return hipErrorInvalidValue;
  if (!aligned16(q) || !aligned16(k_codes) || !aligned16(v_codes) || !aligned16(ws)) return hipErrorInvalidValue;
  if (!aligned4(k_scales) || !aligned4(v_scales)) return hipErrorInvalidValue;
  const int h = int(heads), kv = int(kv_heads), cap = int(capacity);
  float* w = static_cast<float*>(ws);
  if (d == 64)
    return launch_attn_mxfp8<64>(q, k_codes, k_scales, v_codes, v_scales, lens, B, h, kv, cap, p, w, y, y_bf16, s);
  return launch_attn_mxfp8<128>(q, k_codes, k_scales, v_codes, v_scales, lens, B, h, kv, cap, p, w, y, y_bf16, s);
}

}  // namespace kern
}  // namespace dissem
