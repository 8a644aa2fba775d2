// Host-side sizing of the single-token attention (attn_decode.hip): the checks,
// the grid and the workspace of a launch as plain integer arithmetic, with no
// HIP in it, so that a stand-alone program can run it under a sanitizer
// (csrc/tests/attn_decode_selftest.cc).
#pragma once

#include <cstdint>

namespace dissem {
namespace kern {

// Positions of one workgroup's chunk. Chunk c of a sequence is positions
// [c * kAttnDecodeChunk, (c + 1) * kAttnDecodeChunk) whatever the batch, the
// lengths of the other sequences, max_len and the capacity are.
constexpr int kAttnDecodeChunk = 256;
constexpr int64_t kAttnMaxCapacity = int64_t(1) << 20;

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
  if (d != 32 && d != 64 && d != 128) return p;
  if (B < 1 || kv_heads < 1 || heads < kv_heads || heads % kv_heads || heads / kv_heads > 16) return p;
  if (capacity < 1 || capacity > kAttnMaxCapacity || max_len < 1 || max_len > capacity) return p;
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
  if (d != 32 && d != 64 && d != 128) return false;
  if (B < 1 || B > 0x7FFFFFFF || kv_heads < 1 || kv_heads > 65535 || heads > 65535) return false;
  if (heads < kv_heads || heads % kv_heads || heads + 2 * kv_heads > 65535) return false;  // grid.y
  if (capacity < 1 || capacity > kAttnMaxCapacity) return false;
  if (B * kv_heads > (int64_t(1) << 31)) return false;
  if (ldq < heads * d || ldk < kv_heads * d || ldv < kv_heads * d) return false;
  if (ldq > (int64_t(1) << 31) || ldk > (int64_t(1) << 31) || ldv > (int64_t(1) << 31)) return false;
  return true;
}

}  // namespace kern
}  // namespace dissem
