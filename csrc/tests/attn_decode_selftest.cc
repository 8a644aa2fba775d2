// attn_decode_selftest: the host-side sizing of the single-token attention
// (kernels/attn_decode_plan.h) under Address and UndefinedBehavior sanitizer
// (make sanitize-attn). No GPU and no HIP:
//   * for small shapes the workspace is a heap allocation of exactly
//     plan.ws_bytes and every index the two kernels form - partial row
//     (b * kv_heads + kvh) * nchunks + chunk, its group rows of d outputs and of
//     (m, l) pairs - is written once and read once: an index past the plan's
//     size is an ASan report, a row written twice a failure;
//   * the largest cache the contract admits (2^20 positions, d 128) and the
//     largest grids: every product stays inside int64 (UBSan reports a signed
//     overflow) and the last cache element's index is what 64-bit arithmetic
//     gives;
//   * every shape outside the contract is refused.
#include <cstdint>
#include <cstdio>
#include <memory>

#include "kernels/attn_decode_plan.h"

using namespace dissem::kern;

static int failures = 0;
#define EXPECT(c)                                                    \
  do {                                                               \
    if (!(c)) {                                                      \
      ++failures;                                                    \
      fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);   \
    }                                                                \
  } while (0)

static void walk(int64_t B, int64_t heads, int64_t kv_heads, int64_t d, int64_t capacity, int64_t max_len) {
  const AttnDecodePlan p = attn_decode_plan(B, heads, kv_heads, d, capacity, max_len);
  EXPECT(p.ok);
  if (!p.ok) return;
  EXPECT(p.nchunks * kAttnDecodeChunk >= max_len && (p.nchunks - 1) * kAttnDecodeChunk < max_len);
  EXPECT(p.ws_bytes % 4 == 0);
  const size_t n = size_t(p.ws_bytes / 4);
  std::unique_ptr<float[]> ws(new float[n]);  // exactly the plan's size
  for (size_t i = 0; i < n; ++i) ws[i] = 0.0f;
  float* ws_o = ws.get();
  float* ws_ml = ws.get() + p.o_floats;
  // the partial kernel's stores
  for (int64_t blk = 0; blk < p.blocks; ++blk) {
    const int64_t chunk = blk % p.nchunks, bh = blk / p.nchunks, kvh = bh % kv_heads, b = bh / kv_heads;
    EXPECT(b < B && (b * kv_heads + kvh) * p.nchunks + chunk == blk);
    for (int h = 0; h < p.group; ++h) {
      const int64_t row = blk * p.group + h;
      for (int64_t dd = 0; dd < d; ++dd) ws_o[row * d + dd] += 1.0f;
      ws_ml[row * 2] += 1.0f;
      ws_ml[row * 2 + 1] += 1.0f;
    }
  }
  // the combine kernel's loads: every element exactly once
  for (int64_t bhq = 0; bhq < B * heads; ++bhq) {
    const int64_t b = bhq / heads, h = bhq % heads;
    const int64_t row0 = (b * kv_heads + h / p.group) * p.nchunks * p.group + h % p.group;
    for (int64_t c = 0; c < p.nchunks; ++c) {
      const int64_t row = row0 + c * p.group;
      for (int64_t dd = 0; dd < d; ++dd) ws_o[row * d + dd] += 1.0f;
      ws_ml[row * 2] += 1.0f;
      ws_ml[row * 2 + 1] += 1.0f;
    }
  }
  for (size_t i = 0; i < n; ++i) EXPECT(ws[i] == 2.0f);
}

int main() {
  EXPECT(kAttnDecodeChunk > 0 && kAttnDecodeChunk % 128 == 0);
  for (int64_t d : {32, 64, 128})
    for (int64_t group : {1, 2, 3, 8, 16})
      for (int64_t max_len : {int64_t(1), int64_t(kAttnDecodeChunk), int64_t(kAttnDecodeChunk + 1),
                              int64_t(2 * kAttnDecodeChunk + 3)})
        walk(3, 2 * group, 2, d, 2 * kAttnDecodeChunk + 8, max_len);
  walk(1, 1, 1, 32, 1, 1);

  // the extremes of the contract
  {
    const int64_t cap = kAttnMaxCapacity;
    AttnDecodePlan p = attn_decode_plan(64, 128, 8, 128, cap, cap);  // 4096 chunks of 64 * 8 (b, head)
    EXPECT(p.ok && p.nchunks == 4096 && p.blocks == int64_t(64) * 8 * 4096 && p.group == 16);
    EXPECT(p.ws_bytes == p.blocks * 16 * 130 * 4);
    p = attn_decode_plan(int64_t(1) << 31, 16, 1, 128, cap, 1);  // one block too many for a 31-bit grid
    EXPECT(!p.ok);
    p = attn_decode_plan((int64_t(1) << 31) - 1, 16, 1, 128, cap, 1);
    EXPECT(p.ok && p.blocks == 0x7FFFFFFF && p.o_floats == int64_t(0x7FFFFFFF) * 16 * 128);
    EXPECT(p.ws_bytes == int64_t(0x7FFFFFFF) * 16 * 130 * 4);
    p = attn_decode_plan(33, 4, 1, 64, cap, kAttnDecodeChunk + 1);
    EXPECT(p.ok && p.nchunks == 2);
    // the last element of the largest cache one (b, head) pair count admits
    const int64_t bh = (int64_t(1) << 31) - 1, last = (bh * cap + (cap - 1)) * 128 + 127;
    EXPECT(last == ((int64_t(1) << 31) * cap * 128) - 1);
    EXPECT(last > 0);
  }
  // outside the contract
  const int64_t C = kAttnDecodeChunk;
  EXPECT(!attn_decode_plan(1, 4, 2, 48, C, C).ok);      // d
  EXPECT(!attn_decode_plan(1, 4, 2, 256, C, C).ok);
  EXPECT(!attn_decode_plan(1, 34, 2, 64, C, C).ok);     // group 17
  EXPECT(!attn_decode_plan(1, 5, 2, 64, C, C).ok);      // heads % kv_heads
  EXPECT(!attn_decode_plan(1, 1, 2, 64, C, C).ok);      // heads < kv_heads
  EXPECT(!attn_decode_plan(0, 4, 2, 64, C, C).ok);
  EXPECT(!attn_decode_plan(1, 4, 0, 64, C, C).ok);
  EXPECT(!attn_decode_plan(1, 4, 2, 64, C, C + 1).ok);  // max_len > capacity
  EXPECT(!attn_decode_plan(1, 4, 2, 64, C, 0).ok);
  EXPECT(!attn_decode_plan(1, 4, 2, 64, kAttnMaxCapacity + 1, 1).ok);
  EXPECT(!attn_decode_plan(INT64_MAX, 4, 2, 64, C, C).ok);
  EXPECT(!attn_decode_plan(1, INT64_MAX, INT64_MAX, 64, C, C).ok);
  EXPECT(!attn_decode_plan(int64_t(1) << 30, 1 << 20, 1 << 16, 64, C, C).ok);

  EXPECT(attn_rope_plan(3, 4, 2, 64, 16, 512, 128, 128));
  EXPECT(attn_rope_plan(3, 4, 2, 64, 16, 256, 128, 128));
  EXPECT(!attn_rope_plan(3, 4, 2, 64, 16, 255, 128, 128));  // a row shorter than its heads
  EXPECT(!attn_rope_plan(3, 4, 2, 64, 16, 512, 127, 128));
  EXPECT(!attn_rope_plan(3, 4, 2, 64, 16, 512, 128, 64));
  EXPECT(!attn_rope_plan(3, 4, 2, 48, 16, 512, 128, 128));
  EXPECT(!attn_rope_plan(3, 5, 2, 64, 16, 512, 128, 128));
  EXPECT(!attn_rope_plan(3, 65534, 2, 32, 16, int64_t(65534) * 32, 64, 64));  // grid.y
  EXPECT(!attn_rope_plan(int64_t(1) << 31, 4, 2, 64, 16, 512, 128, 128));
  EXPECT(!attn_rope_plan(3, 4, 2, 64, 0, 512, 128, 128));
  EXPECT(!attn_rope_plan(3, 4, 2, 64, 16, INT64_MAX, 128, 128));
  EXPECT(!attn_rope_plan(INT64_MAX, INT64_MAX, INT64_MAX, 64, 16, 512, 128, 128));

  if (failures) {
    fprintf(stderr, "attn_decode_selftest: %d failure(s)\n", failures);
    return 1;
  }
  printf("attn_decode_selftest ok\n");
  return 0;
}
