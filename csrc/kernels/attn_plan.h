// Host-side sizing of the single-token attention and rope (attn_decode.hip; on
// an MXFP8 cache attn_decode_mxfp8.hip) and of the causal prefill / extend
// attention and many-token rope (attn_prefill.hip; on an MXFP8 cache attn_prefill_mxfp8.hip): the shape and stride checks, the tile constants, the grids and the workspace as
// plain integer arithmetic, with no HIP in it, so that stand-alone programs can run it
// under a sanitizer (csrc/tests/attn_decode_selftest.cc, attn_prefill_selftest.cc, attn_prefill_mxfp8_selftest.cc).
#pragma once

#include <cstdint>

namespace dissem {
namespace kern {

// Positions of a cache, of K / V, and query rows of a sequence.
constexpr int64_t kAttnMaxPositions = int64_t(1) << 20;

// Positions of one workgroup's chunk of the single-token attention. Chunk c of
// a sequence is positions [c * kAttnDecodeChunk, (c + 1) * kAttnDecodeChunk)
// whatever the batch, the lengths of the other sequences, max_len and the
// capacity are.
constexpr int kAttnDecodeChunk = 256;

// A prefill workgroup serves kAttnPrefillBQ query rows of one (sequence, query
// head) and walks K and V in tiles of kAttnPrefillBK positions. Tile t of a
// sequence is positions [t * kAttnPrefillBK, (t + 1) * kAttnPrefillBK) whatever
// the batch, start, S, T and the strides are.
constexpr int kAttnPrefillBQ = 128;
constexpr int kAttnPrefillBK = 64;
constexpr int kAttnPrefillThreads = 256;
constexpr int64_t kAttnPrefillMaxBatch = int64_t(1) << 20;
constexpr int64_t kAttnPrefillMaxStride = int64_t(1) << 40;  // elements

// d 32, 64 or 128; heads a multiple of kv_heads, both at least 1.
inline bool attn_heads_ok(int64_t heads, int64_t kv_heads, int64_t d) {
  if (d != 32 && d != 64 && d != 128) return false;
  return kv_heads >= 1 && heads >= kv_heads && heads % kv_heads == 0;
}

// The rows of q, k and v that a rope launch reads, ldq, ldk and ldv elements apart, and the caches
// [B, kv_heads, capacity, d] it appends to; the caller has bounded B by 2^31.
inline bool attn_rope_rows_ok(int64_t B, int64_t heads, int64_t kv_heads, int64_t d, int64_t capacity, int64_t ldq,
                              int64_t ldk, int64_t ldv) {
  if (!attn_heads_ok(heads, kv_heads, d) || kv_heads > 65535 || heads > 65535) return false;
  if (capacity < 1 || capacity > kAttnMaxPositions) return false;
  if (ldq < heads * d || ldk < kv_heads * d || ldv < kv_heads * d) return false;
  // a row's offset: (rows - 1) ld <= 2^31 2^31 = 2^62; a cache element: B kv_heads capacity d <= 2^20 2^16 2^20 2^7 = 2^63
  // would not do, so the (b, head) pairs are bounded as in attn_decode_plan
  if (ldq > (int64_t(1) << 31) || ldk > (int64_t(1) << 31) || ldv > (int64_t(1) << 31)) return false;
  return B * kv_heads <= (int64_t(1) << 31);
}

struct AttnDecodePlan {
  bool ok = false;
  int group = 0;          // query heads per KV head
  int64_t nchunks = 0;    // chunks that cover max_len
  int64_t blocks = 0;     // workgroups of the partial kernel: B * kv_heads * nchunks
  int64_t o_floats = 0;   // f32 of the partial outputs [B, kv_heads, nchunks, group, d]
  int64_t ml_floats = 0;  // f32 of the partial (m, l) pairs [B, kv_heads, nchunks, group, 2]
  int64_t ws_bytes = 0;   // the workspace: the outputs, then the pairs
};

// ok only for a shape the kernels serve: d 32, 64 or 128; heads a multiple of
// kv_heads with a group of 1..16; 1 <= max_len <= capacity <= 2^20; the caches
// [B, kv_heads, capacity, d] addressable in int64 elements and the grid in 31 bits.
inline AttnDecodePlan attn_decode_plan(int64_t B, int64_t heads, int64_t kv_heads, int64_t d, int64_t capacity,
                                       int64_t max_len) {
  AttnDecodePlan p;
  if (B < 1 || !attn_heads_ok(heads, kv_heads, d) || heads / kv_heads > 16) return p;
  if (capacity < 1 || capacity > kAttnMaxPositions || max_len < 1 || max_len > capacity) return p;
  // B * kv_heads * capacity * d (<= 2^27 per (b, head)) must stay an int64 element index with room to spare
  if (B > (int64_t(1) << 31) || kv_heads > (int64_t(1) << 16) || B * kv_heads > (int64_t(1) << 31)) return p;
  p.group = int(heads / kv_heads);
  p.nchunks = (max_len + kAttnDecodeChunk - 1) / kAttnDecodeChunk;  // <= 4096
  p.blocks = B * kv_heads * p.nchunks;                              // <= 2^43
  if (p.blocks > 0x7FFFFFFF) return p;
  p.o_floats = p.blocks * p.group * d;  // <= 2^31 * 16 * 128 = 2^42
  p.ml_floats = p.blocks * p.group * 2;
  p.ws_bytes = (p.o_floats + p.ml_floats) * 4;
  p.ok = true;
  return p;
}

// The rope_append launch: one workgroup per (sequence, head of q, k or v).
inline bool attn_rope_plan(int64_t B, int64_t heads, int64_t kv_heads, int64_t d, int64_t capacity, int64_t ldq,
                           int64_t ldk, int64_t ldv) {
  if (B < 1 || B > 0x7FFFFFFF || !attn_rope_rows_ok(B, heads, kv_heads, d, capacity, ldq, ldk, ldv)) return false;
  return heads + 2 * kv_heads <= 65535;  // grid.y
}

// ---- the MXFP8 KV cache (attn_decode_mxfp8.hip): e4m3 codes uint8 [B, kv_heads, capacity, d] and one E8M0
// scale byte per 32 d, uint8 [B, kv_heads, capacity, d / 32].

// d 64 or 128: at d = 32 half a head is half a scale block, which the rope's lane map does not serve.
inline bool attn_mxfp8_d_ok(int64_t d) { return d == 64 || d == 128; }

// attn_decode_plan for that cache: the same grid and workspace. The codes are B kv_heads capacity d <= 2^31
// 2^20 2^7 = 2^58 bytes and the scale bytes a 32nd of them, so both tensors' last byte is an int64 offset.
inline AttnDecodePlan attn_decode_mxfp8_plan(int64_t B, int64_t heads, int64_t kv_heads, int64_t d,
                                             int64_t capacity, int64_t max_len) {
  if (!attn_mxfp8_d_ok(d)) return AttnDecodePlan();
  return attn_decode_plan(B, heads, kv_heads, d, capacity, max_len);
}

// The MXFP8 rope_append launch: an item is one thread's work, a (head of q, k or v, piece of 8 d of the
// lower half with its partners of the upper half); workgroup (b, y) takes items [y * kAttnRopeMxThreads, ...)
// of sequence b. Rows are read 16 bytes at a time: ldq, ldk and ldv are multiples of 8 elements.
constexpr int kAttnRopeMxThreads = 256;

struct AttnRopeMxPlan {
  bool ok = false;
  int items = 0;   // (heads + 2 kv_heads) * (d / 16) <= 3 * 65535 * 8
  int grid_y = 0;  // workgroups of a sequence
};

inline AttnRopeMxPlan attn_rope_mxfp8_plan(int64_t B, int64_t heads, int64_t kv_heads, int64_t d, int64_t capacity,
                                           int64_t ldq, int64_t ldk, int64_t ldv) {
  AttnRopeMxPlan p;
  if (!attn_mxfp8_d_ok(d) || B < 1 || B > 0x7FFFFFFF) return p;
  if (!attn_rope_rows_ok(B, heads, kv_heads, d, capacity, ldq, ldk, ldv)) return p;
  if (ldq % 8 || ldk % 8 || ldv % 8) return p;
  p.items = int((heads + 2 * kv_heads) * (d / 16));
  p.grid_y = (p.items + kAttnRopeMxThreads - 1) / kAttnRopeMxThreads;  // <= 6144
  p.ok = true;
  return p;
}

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
  if (!attn_heads_ok(heads, kv_heads, d) || kv_heads > 65535 || heads > (int64_t(1) << 20)) return p;
  if (B < 1 || B > kAttnPrefillMaxBatch) return p;
  if (S < 1 || S > kAttnMaxPositions || T < 1 || T > kAttnMaxPositions) return p;
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
  if (B < 1 || B > kAttnPrefillMaxBatch || S < 1 || S > kAttnMaxPositions || B * S > (int64_t(1) << 31)) return p;
  if (!attn_rope_rows_ok(B, heads, kv_heads, d, capacity, ldq, ldk, ldv)) return p;
  if (ldq % 8 || ldk % 8 || ldv % 8) return p;            // 16-byte loads
  p.threads = B * S * (heads + 2 * kv_heads) * (d / 16);  // <= 2^31 2^17 2^3 = 2^51
  p.blocks = (p.threads + kAttnPrefillThreads - 1) / kAttnPrefillThreads;
  if (p.blocks > 0x7FFFFFFF) return p;
  p.ok = true;
  return p;
}

// ---- the same two against the MXFP8 KV cache (attn_prefill_mxfp8.hip).

// attn_prefill_plan for contiguous codes [B, kv_heads, T, d] and scale bytes [B, kv_heads, T, d / 32]: the
// same grid. The strides checked are the contiguous ones, so a sequence's codes stay within
// kAttnPrefillMaxStride bytes and the last code's offset, B kv_heads T d - 1 <= 2^20 2^40, within int64.
inline AttnPrefillPlan attn_prefill_mxfp8_plan(int64_t B, int64_t S, int64_t heads, int64_t kv_heads, int64_t d,
                                               int64_t T) {
  if (!attn_mxfp8_d_ok(d) || kv_heads < 1 || kv_heads > 65535 || T < 1 || T > kAttnMaxPositions)
    return AttnPrefillPlan();
  const int64_t st[3] = {kv_heads * T * d, T * d, d};  // <= 2^16 2^20 2^7
  return attn_prefill_plan(B, S, heads, kv_heads, d, T, st, st);
}

// The many-token MXFP8 rope and append: workgroup (n, y) takes items [y * kAttnRopeMxThreads, ...) - the items
// of attn_rope_mxfp8_plan - of row n = b * S + i, so a row's position is one value for the whole workgroup.
struct AttnRopeSeqMxPlan {
  bool ok = false;
  int64_t rows = 0;  // B * S: grid.x
  int items = 0;     // (heads + 2 kv_heads) * (d / 16)
  int grid_y = 0;    // workgroups of a row
};

inline AttnRopeSeqMxPlan attn_rope_seq_mxfp8_plan(int64_t B, int64_t S, int64_t heads, int64_t kv_heads, int64_t d,
                                                  int64_t capacity, int64_t ldq, int64_t ldk, int64_t ldv) {
  AttnRopeSeqMxPlan p;
  if (!attn_mxfp8_d_ok(d) || B < 1 || B > kAttnPrefillMaxBatch || S < 1 || S > kAttnMaxPositions) return p;
  if (B * S > 0x7FFFFFFF) return p;  // grid.x
  if (!attn_rope_rows_ok(B, heads, kv_heads, d, capacity, ldq, ldk, ldv)) return p;
  if (ldq % 8 || ldk % 8 || ldv % 8) return p;  // 16-byte loads
  p.rows = B * S;
  p.items = int((heads + 2 * kv_heads) * (d / 16));  // <= 3 * 65535 * 8
  p.grid_y = (p.items + kAttnRopeMxThreads - 1) / kAttnRopeMxThreads;  // <= 6144
  p.ok = true;
  return p;
}

}  // namespace kern
}  // namespace dissem
