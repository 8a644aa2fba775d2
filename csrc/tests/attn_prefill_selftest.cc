// attn_prefill_selftest: the host-side sizing of the prefill attention and of the
// many-token rope (kernels/attn_plan.h) under ASan + UBSan (make
// sanitize-attn-prefill), no GPU: every workgroup of the plan's grid marks, with
// the kernel's own index arithmetic, its rows of an exact-size y (a row outside
// is an ASan report, one served twice or never a failure); the contract's
// extremes stay inside int64; everything outside the contract is refused.
#include <cstdint>
#include <cstdio>
#include <memory>

#include "kernels/attn_plan.h"

using namespace dissem::kern;

static int failures = 0;
#define EXPECT(c)                                                  \
  do {                                                             \
    if (!(c)) {                                                    \
      ++failures;                                                  \
      fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); \
    }                                                              \
  } while (0)

static void walk(int64_t B, int64_t S, int64_t heads, int64_t kv_heads, int64_t d) {
  const int64_t ks[3] = {kv_heads * 300 * d, 300 * d, d}, ld = (heads + 2 * kv_heads) * d;
  const AttnPrefillPlan p = attn_prefill_plan(B, S, heads, kv_heads, d, 300, ks, ks);
  const AttnRopeSeqPlan r = attn_rope_seq_plan(B, S, heads, kv_heads, d, 300, ld, ld, ld);
  EXPECT(p.ok && r.ok && r.threads == B * S * (heads + 2 * kv_heads) * (d / 16));
  EXPECT(r.blocks * kAttnPrefillThreads >= r.threads && (r.blocks - 1) * kAttnPrefillThreads < r.threads);
  if (!p.ok) return;
  std::unique_ptr<int[]> rows(new int[size_t(B * S * heads)]());  // exactly y's rows
  for (int64_t blk = 0; blk < p.blocks; ++blk) {
    const int64_t h = blk % heads, rest = blk / heads, b = rest % B, q0 = (p.qtiles - 1 - rest / B) * kAttnPrefillBQ;
    EXPECT(q0 >= 0 && q0 < S && h / p.group < kv_heads);
    for (int64_t iq = 0; iq < kAttnPrefillBQ && q0 + iq < S; ++iq) rows[(b * S + q0 + iq) * heads + h] += 1;
  }
  for (int64_t i = 0; i < B * S * heads; ++i) EXPECT(rows[i] == 1);
}

int main() {
  const int64_t BQ = kAttnPrefillBQ, T = kAttnMaxPositions, M = kAttnPrefillMaxStride;
  for (int64_t d : {32, 64, 128})
    for (int64_t group : {1, 3, 8})
      for (int64_t S : {int64_t(1), BQ, BQ + 1, 2 * BQ + 3}) walk(3, S, 2 * group, 2, d);
  // the extremes of the contract
  const int64_t big[3] = {M, M, M};
  AttnPrefillPlan p = attn_prefill_plan(1, T, 64, 8, 128, T, big, big);
  EXPECT(p.ok && p.qtiles == 8192 && p.blocks == 64 * 8192 && p.group == 8);
  p = attn_prefill_plan(kAttnPrefillMaxBatch, 1, 2047, 1, 128, T, big, big);  // 2^20 * 2047 < 2^31
  EXPECT(p.ok && p.blocks == kAttnPrefillMaxBatch * 2047);
  EXPECT(!attn_prefill_plan(kAttnPrefillMaxBatch, 1, 2048, 1, 128, T, big, big).ok);  // one grid too many
  EXPECT((kAttnPrefillMaxBatch - 1) * M + 65534 * M + (T - 1) * M + 127 < (int64_t(1) << 62));  // the last element
  const int64_t L = int64_t(1) << 31;
  const AttnRopeSeqPlan r = attn_rope_seq_plan(512, T, 64, 8, 128, T, L, L, L);
  EXPECT(r.ok && r.threads == 512 * T * 80 * 8 && r.blocks == r.threads / kAttnPrefillThreads);
  EXPECT(!attn_rope_seq_plan(2048, T, 64, 8, 128, T, 10240, 10240, 10240).ok);  // more than 2^31 - 1 workgroups
  EXPECT(!attn_rope_seq_plan(4096, T, 64, 8, 128, T, 10240, 10240, 10240).ok);  // B * S above 2^31
  // outside the contract
  const int64_t ok[3] = {2 * 300 * 64, 300 * 64, 64}, odd[3] = {ok[0], ok[1], 68}, neg[3] = {ok[0], -64, 64};
  const int64_t huge[3] = {M + 8, ok[1], 64}, X = INT64_MAX;
  EXPECT(attn_prefill_plan(2, 5, 4, 2, 64, 300, ok, ok).ok);
  EXPECT(!attn_prefill_plan(2, 5, 4, 2, 48, 300, ok, ok).ok && !attn_prefill_plan(2, 5, 4, 2, 256, 300, ok, ok).ok);  // d
  EXPECT(!attn_prefill_plan(2, 5, 5, 2, 64, 300, ok, ok).ok && !attn_prefill_plan(2, 5, 1, 2, 64, 300, ok, ok).ok);   // heads
  EXPECT(!attn_prefill_plan(0, 5, 4, 2, 64, 300, ok, ok).ok && !attn_prefill_plan(2, 0, 4, 2, 64, 300, ok, ok).ok);
  EXPECT(!attn_prefill_plan(2, 5, 4, 0, 64, 300, ok, ok).ok && !attn_prefill_plan(2, 5, 4, 2, 64, 0, ok, ok).ok);
  EXPECT(!attn_prefill_plan(2, 5, 4, 2, 64, T + 1, ok, ok).ok && !attn_prefill_plan(2, T + 1, 4, 2, 64, 300, ok, ok).ok);
  EXPECT(!attn_prefill_plan(2, 5, 4, 2, 64, 300, odd, ok).ok && !attn_prefill_plan(2, 5, 4, 2, 64, 300, ok, odd).ok);  // % 8
  EXPECT(!attn_prefill_plan(2, 5, 4, 2, 64, 300, neg, ok).ok && !attn_prefill_plan(2, 5, 4, 2, 64, 300, ok, huge).ok);
  EXPECT(!attn_prefill_plan(X, X, X, X, 64, 300, ok, ok).ok);
  EXPECT(attn_rope_seq_plan(3, 5, 4, 2, 64, 16, 512, 128, 128).ok);
  EXPECT(!attn_rope_seq_plan(3, 5, 4, 2, 64, 16, 248, 128, 128).ok);  // a row shorter than its heads
  EXPECT(!attn_rope_seq_plan(3, 5, 4, 2, 64, 16, 516, 128, 128).ok && !attn_rope_seq_plan(3, 5, 4, 2, 64, 16, 512, 132, 128).ok);
  EXPECT(!attn_rope_seq_plan(3, 5, 4, 2, 64, 16, 512, 128, 64).ok && !attn_rope_seq_plan(3, 5, 4, 2, 48, 16, 512, 128, 128).ok);
  EXPECT(!attn_rope_seq_plan(3, 5, 5, 2, 64, 16, 512, 128, 128).ok && !attn_rope_seq_plan(3, 0, 4, 2, 64, 16, 512, 128, 128).ok);
  EXPECT(!attn_rope_seq_plan(3, 5, 4, 2, 64, 0, 512, 128, 128).ok && !attn_rope_seq_plan(3, 5, 4, 2, 64, 16, X, 128, 128).ok);
  EXPECT(!attn_rope_seq_plan(X, X, X, X, 64, 16, 512, 128, 128).ok);
  if (failures) {
    fprintf(stderr, "attn_prefill_selftest: %d failure(s)\n", failures);
    return 1;
  }
  printf("attn_prefill_selftest ok\n");
  return 0;
}
