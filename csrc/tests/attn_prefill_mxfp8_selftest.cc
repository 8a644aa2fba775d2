// attn_prefill_mxfp8_selftest: the host-side sizing of the MXFP8 prefill attention
// and of the many-token MXFP8 rope (kernels/attn_plan.h) under ASan + UBSan (make
// sanitize-attn-prefill-mxfp8), no GPU. Every workgroup of the two grids walks,
// with the kernels' own index arithmetic (attn_prefill_mxfp8.hip), exact-size
// buffers: the codes and scale bytes a tile's fetch loads, the LDS tile its stash
// fills, y's rows; q_out and the four cache tensors of the rope. An index outside
// is an ASan report, a byte served twice or never a failure.
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

template <typename T>
static std::unique_ptr<T[]> zeros(int64_t n) { return std::unique_ptr<T[]>(new T[size_t(n)]()); }

// kv_off<D> of the kernel: element offset of 16-byte piece `piece` of row `row` of a [BK][D] bf16 tile
static int kv_off(int D, int row, int piece) {
  return row * D + 8 * (piece ^ ((row >> (D == 128 ? 0 : 1)) & (D / 8 - 1)));
}

static void walk_prefill(int64_t B, int64_t S, int64_t heads, int64_t kv_heads, int D, int T, const int* start) {
  const AttnPrefillPlan p = attn_prefill_mxfp8_plan(B, S, heads, kv_heads, D, T);
  EXPECT(p.ok);
  if (!p.ok) return;
  const int BQ = kAttnPrefillBQ, BK = kAttnPrefillBK, PC = D / 16, NB = D / 32, NC = BK * PC / kAttnPrefillThreads;
  const int64_t ncodes = B * kv_heads * T * D;
  auto codes = zeros<uint8_t>(ncodes), scales = zeros<uint8_t>(ncodes / 32);  // loaded or not
  auto rows = zeros<int>(B * S * heads);
  auto lds = zeros<int>(BK * D / 8);  // 16-byte pieces of a tile
  for (int64_t blk = 0; blk < p.blocks; ++blk) {
    const int h = int(blk % heads), b = int(blk / heads % B), q0 = int((p.qtiles - 1 - blk / heads / B) * BQ);
    int st = start[b] < 0 ? 0 : (start[b] > T ? T : start[b]);
    const int nrows = S - q0 < BQ ? int(S - q0) : BQ, kv_end = st + S < T ? int(st + S) : T, pos0 = st + q0;
    const int pos_end = pos0 + nrows < T ? pos0 + nrows : T, ntiles = pos_end > pos0 ? (pos_end - 1) / BK + 1 : 0;
    const int64_t bh = int64_t(b) * kv_heads + h / p.group;
    EXPECT(q0 >= 0 && q0 < S && h / p.group < kv_heads);
    for (int t = 0; t < ntiles; ++t) {
      for (int i = 0; i < BK * D / 8; ++i) lds[i] = 0;
      for (int tid = 0; tid < kAttnPrefillThreads; ++tid)
        for (int n = 0; n < NC; ++n) {
          const int idx = tid + kAttnPrefillThreads * n, row = idx / PC, c = idx % PC, pos = t * BK + row;
          if (pos < kv_end) {
            for (int e = 0; e < 16; ++e) codes[(bh * T + pos) * D + 16 * c + e] = 1;
            scales[(bh * T + pos) * NB + (c >> 1)] = 1;
          }
          lds[kv_off(D, row, 2 * c) / 8] += 1;
          lds[kv_off(D, row, 2 * c + 1) / 8] += 1;
        }
      for (int i = 0; i < BK * D / 8; ++i) EXPECT(lds[i] == 1);
    }
    for (int iq = 0; iq < nrows; ++iq) rows[(int64_t(b) * S + q0 + iq) * heads + h] += 1;
  }
  for (int64_t i = 0; i < B * S * heads; ++i) EXPECT(rows[i] == 1);
  // loaded: exactly the positions below min(start + S, T) - of the KV heads, all of whose groups have a head
  for (int64_t i = 0; i < ncodes; ++i) {
    const int b = int(i / (kv_heads * T * D)), pos = int(i / D % T), st = start[b] < 0 ? 0 : (start[b] > T ? T : start[b]);
    const bool want = pos < (st + S < T ? st + S : T) && st < T;
    EXPECT(codes[i] == want && scales[i / 32] == want);
  }
}

static void walk_rope(int64_t B, int64_t S, int heads, int kv_heads, int D, int cap, const int* start) {
  const int64_t ld = int64_t(heads + 2 * kv_heads) * D;
  const AttnRopeSeqMxPlan p = attn_rope_seq_mxfp8_plan(B, S, heads, kv_heads, D, cap, ld, ld, ld);
  EXPECT(p.ok && p.rows == B * S && p.items == (heads + 2 * kv_heads) * (D / 16));
  EXPECT(int64_t(p.grid_y) * kAttnRopeMxThreads >= p.items && int64_t(p.grid_y - 1) * kAttnRopeMxThreads < p.items);
  if (!p.ok) return;
  const int L = D / 16;
  auto src = zeros<int>(B * S * ld / 8), qo = zeros<int>(B * S * heads * D / 8);  // 16-byte pieces
  const int64_t ncodes = B * kv_heads * cap * D;
  auto kc = zeros<int>(ncodes / 8), vc = zeros<int>(ncodes / 8), ks = zeros<int>(ncodes / 32), vs = zeros<int>(ncodes / 32);
  for (int64_t n = 0; n < p.rows; ++n)
    for (int y = 0; y < p.grid_y; ++y)
      for (int tid = 0; tid < kAttnRopeMxThreads; ++tid) {
        const int item = y * kAttnRopeMxThreads + tid, c = item % L, slot = item / L, lo = 8 * c, hi = D / 2 + 8 * c;
        if (item >= p.items) continue;
        const bool is_q = slot < heads, is_k = !is_q && slot < heads + kv_heads;
        const int hh = is_q ? slot : (is_k ? slot - heads : slot - heads - kv_heads);
        const int64_t b = n / S, pos = int64_t(start[b]) + (n - b * S);
        const bool ok = pos >= 0 && pos < cap;
        if (ok) src[(n * ld + int64_t(slot) * D + lo) / 8] += 1, src[(n * ld + int64_t(slot) * D + hi) / 8] += 1;
        if (is_q) qo[((n * heads + hh) * D + lo) / 8] += 1, qo[((n * heads + hh) * D + hi) / 8] += 1;
        if (is_q || !ok) continue;
        const int64_t row = (b * kv_heads + hh) * cap + pos;
        (is_k ? kc : vc)[(row * D + lo) / 8] += 1, (is_k ? kc : vc)[(row * D + hi) / 8] += 1;
        if ((tid & 3) == 0) (is_k ? ks : vs)[row * (D / 32) + lo / 32] += 1, (is_k ? ks : vs)[row * (D / 32) + hi / 32] += 1;
      }
  for (int64_t i = 0; i < B * S * heads * D / 8; ++i) EXPECT(qo[i] == 1);
  for (int64_t i = 0; i < ncodes / 8; ++i) {
    const int64_t b = i * 8 / (int64_t(kv_heads) * cap * D), pos = i * 8 / D % cap;
    const int want = pos >= start[b] && pos < start[b] + S;
    EXPECT(kc[i] == want && vc[i] == want && ks[i / 4] == want && vs[i / 4] == want);
  }
  for (int64_t i = 0; i < B * S * ld / 8; ++i) EXPECT(src[i] <= 1);
}

int main() {
  const int BQ = kAttnPrefillBQ, BK = kAttnPrefillBK;
  const int64_t T = kAttnMaxPositions;
  const int start[4] = {0, -3, BK - 1, 400}, rstart[4] = {0, 5, 33, -2};
  for (int d : {64, 128})
    for (int group : {1, 3, 8})
      for (int S : {1, BK + 1, BQ + 1, 2 * BQ + 3}) walk_prefill(4, S, 2 * group, 2, d, BK + 5 + S + 3, start);
  for (int d : {64, 128}) {
    walk_rope(4, 7, 4, 2, d, 37, rstart);
    walk_rope(4, 7, 30, 3, d, 37, rstart);  // more than one workgroup a row
  }
  // the extremes of the contract, and what lies outside it
  AttnPrefillPlan p = attn_prefill_mxfp8_plan(1, T, 64, 8, 128, T);
  EXPECT(p.ok && p.qtiles == 8192 && p.blocks == 64 * 8192 && p.group == 8);
  EXPECT(attn_prefill_mxfp8_plan(kAttnPrefillMaxBatch, 1, 2047, 1, 128, T).ok);
  EXPECT(!attn_prefill_mxfp8_plan(kAttnPrefillMaxBatch, 1, 2048, 1, 128, T).ok);  // one grid too many
  EXPECT(attn_prefill_mxfp8_plan(2, 5, 8192, 8192, 128, T).ok && !attn_prefill_mxfp8_plan(2, 5, 16384, 16384, 128, T).ok);  // a sequence's codes: 2^40 bytes
  EXPECT(!attn_prefill_mxfp8_plan(2, 5, 4, 2, 32, 300).ok && !attn_prefill_mxfp8_plan(2, 5, 4, 2, 256, 300).ok);  // d
  EXPECT(!attn_prefill_mxfp8_plan(2, 5, 5, 2, 64, 300).ok && !attn_prefill_mxfp8_plan(2, 5, 4, 0, 64, 300).ok);
  EXPECT(!attn_prefill_mxfp8_plan(0, 5, 4, 2, 64, 300).ok && !attn_prefill_mxfp8_plan(2, 0, 4, 2, 64, 300).ok);
  EXPECT(!attn_prefill_mxfp8_plan(2, 5, 4, 2, 64, 0).ok && !attn_prefill_mxfp8_plan(2, 5, 4, 2, 64, T + 1).ok);
  EXPECT(!attn_prefill_mxfp8_plan(INT64_MAX, INT64_MAX, INT64_MAX, INT64_MAX, 64, INT64_MAX).ok);
  const int64_t L = int64_t(1) << 31;
  EXPECT(attn_rope_seq_mxfp8_plan(2047, T, 64, 8, 128, T, L, L, L).ok);
  EXPECT(!attn_rope_seq_mxfp8_plan(2048, T, 64, 8, 128, T, L, L, L).ok);  // B * S = 2^31: grid.x
  EXPECT(!attn_rope_seq_mxfp8_plan(3, 5, 4, 2, 32, 16, 256, 64, 64).ok);  // d
  EXPECT(!attn_rope_seq_mxfp8_plan(3, 5, 4, 2, 64, 16, 260, 128, 128).ok && !attn_rope_seq_mxfp8_plan(3, 5, 4, 2, 64, 16, 248, 128, 128).ok);
  EXPECT(!attn_rope_seq_mxfp8_plan(3, 5, 5, 2, 64, 16, 512, 128, 128).ok && !attn_rope_seq_mxfp8_plan(3, 0, 4, 2, 64, 16, 512, 128, 128).ok);
  EXPECT(!attn_rope_seq_mxfp8_plan(INT64_MAX, INT64_MAX, INT64_MAX, INT64_MAX, 64, 16, 512, 128, 128).ok);
  if (failures) {
    fprintf(stderr, "attn_prefill_mxfp8_selftest: %d failure(s)\n", failures);
    return 1;
  }
  printf("attn_prefill_mxfp8_selftest ok\n");
  return 0;
}
