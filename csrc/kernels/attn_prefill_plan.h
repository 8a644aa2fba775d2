// Host-side sizing of the causal prefill / extend attention and of the many-token
// rope and append (attn_prefill.hip): the shape and stride checks, the tile
// constants and the grids as plain integer arithmetic, with no HIP in it, so
// that a stand-alone program can run it under a sanitizer
// (csrc/tests/attn_prefill_selftest.cc).
#pragma once

#include <cstdint>

namespace dissem {
namespace kern {

// A workgroup serves kAttnPrefillBQ query rows of one (sequence, query head) and
// walks K and V in tiles of kAttnPrefillBK positions. Tile t of a sequence is
// positions [t * kAttnPrefillBK, (t + 1) * kAttnPrefillBK) whatever the batch,
// start, S, T and the strides are.
constexpr int kAttnPrefillBQ = 128;
constexpr int kAttnPrefillBK = 64;
constexpr int kAttnPrefillThreads = 256;
constexpr int64_t kAttnPrefillMaxT = int64_t(1) << 20;       // positions of K / V, and query rows of a sequence
constexpr int64_t kAttnPrefillMaxBatch = int64_t(1) << 20;
constexpr int64_t kAttnPrefillMaxStride = int64_t(1) << 40;  // elements

struct AttnPrefillPlan {
  bool ok = false;
  int group = 0;       // query heads per KV head
  int64_t qtiles = 0;  // tiles of kAttnPrefillBQ query rows that cover S
  int64_t blocks = 0;  // workgroups: B * heads * qtiles
};

// One stride of K or V in elements: a multiple of 8 (16-byte loads), not negative.
inline bool attn_prefill_stride_ok(int64_t s) { return s >= 0 && s <= kAttnPrefillMaxStride && s % 8 == 0; }

// ok only for a shape the kernel serves: d 32, 64 or 128; heads a multiple of
// kv_heads (any group); 1 <= S, T <= 2^20; kstride and vstride the (batch, head,
// position) element strides of K and V [B, kv_heads, T, d].
inline AttnPrefillPlan attn_prefill_plan(int64_t B, int64_t S, int64_t heads, int64_t kv_heads, int64_t d, int64_t T,
                                         const int64_t* kstride, const int64_t* vstride) {
  AttnPrefillPlan p;
  if (d != 32 && d != 64 && d != 128) return p;
  if (B < 1 || B > kAttnPrefillMaxBatch || kv_heads < 1 || kv_heads > 65535 || heads > (int64_t(1) << 20)) return p;
  if (heads < kv_heads || heads % kv_heads) return p;
  if (S < 1 || S > kAttnPrefillMaxT || T < 1 || T > kAttnPrefillMaxT) return p;
  for (int i = 0; i < 3; ++i)
    if (!attn_prefill_stride_ok(kstride[i]) || !attn_prefill_stride_ok(vstride[i])) return p;
  // the last element a load may touch: (B - 1) sb + (kv_heads - 1) sh + (T - 1) sp + d - 1
  // <= 2^20 2^40 + 2^16 2^40 + 2^20 2^40 + 2^7 < 2^62. In the kernel start[b] is clamped to [0, T], so start + S <=
  // 2^21 in 32 bits.
  p.group = int(heads / kv_heads);
  p.qtiles = (S + kAttnPrefillBQ - 1) / kAttnPrefillBQ;  // <= 2^13
  p.blocks = B * heads * p.qtiles;                       // <= 2^20 2^20 2^13 = 2^53
  if (p.blocks > 0x7FFFFFFF) return p;
  // with that, q and y [B, S, heads, d]: B S heads d <= blocks * BQ * d <= 2^31 2^7 2^7 = 2^45 elements
  p.ok = true;
  return p;
}

// The many-token rope and append: one thread per (row b * S + i, head of q, k or
// v, 16-byte piece of the lower half with its partner of the upper half).
struct AttnRopeSeqPlan {
  bool ok = false;
  int64_t threads = 0;  // B * S * (heads + 2 kv_heads) * (d / 16)
  int64_t blocks = 0;   // of kAttnPrefillThreads
};

inline AttnRopeSeqPlan attn_rope_seq_plan(int64_t B, int64_t S, int64_t heads, int64_t kv_heads, int64_t d,
                                          int64_t capacity, int64_t ldq, int64_t ldk, int64_t ldv) {
  AttnRopeSeqPlan p;
  if (d != 32 && d != 64 && d != 128) return p;
  if (B < 1 || B > kAttnPrefillMaxBatch || S < 1 || S > kAttnPrefillMaxT || B * S > (int64_t(1) << 31)) return p;
  if (kv_heads < 1 || kv_heads > 65535 || heads > 65535 || heads < kv_heads || heads % kv_heads) return p;
  if (capacity < 1 || capacity > kAttnPrefillMaxT) return p;
  if (ldq < heads * d || ldk < kv_heads * d || ldv < kv_heads * d) return p;
  if (ldq % 8 || ldk % 8 || ldv % 8) return p;  // 16-byte loads
  // a row's offset: (B S - 1) ld <= 2^31 2^31 = 2^62; a cache element: B kv_heads capacity d <= 2^20 2^16 2^20 2^7 = 2^63
  // would not do, so the (b, head) pairs are bounded as in attn_decode_plan.h
  if (ldq > (int64_t(1) << 31) || ldk > (int64_t(1) << 31) || ldv > (int64_t(1) << 31)) return p;
  if (B * kv_heads > (int64_t(1) << 31)) return p;
  p.threads = B * S * (heads + 2 * kv_heads) * (d / 16);  // <= 2^31 2^17 2^3 = 2^51
  p.blocks = (p.threads + kAttnPrefillThreads - 1) / kAttnPrefillThreads;
  if (p.blocks > 0x7FFFFFFF) return p;
  p.ok = true;
  return p;
}

}  // namespace kern
}  // namespace dissem
