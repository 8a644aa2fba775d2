// Causal grouped-query attention of S new tokens per sequence against K and V in
// HBM - a prefill from position 0, or an extend behind start[b] positions a
// cache already holds - and the rope and cache append of those S tokens
// (kernels.h has the contracts).
//
// attn_prefill: a workgroup of four waves serves one (sequence, query head, tile
// of BQ = 128 query rows); wave w owns rows 32 w .. 32 w + 31 as two 16-column
// MFMA blocks. Workgroup index = (reversed query tile, sequence, head): the heads
// of a KV group are neighbours and walk the same K / V at the same time (they
// meet in L2), and the last query tile, whose K walk is the longest, is issued
// first.
//
// K and V move in tiles of BK = 64 positions at absolute positions 0, BK, 2 BK,
// ...: the 256 lanes fetch a tile together, 16 B a lane, into registers and then
// into LDS, once per workgroup. Two LDS buffers: the global loads of tile t + 1
// are issued before tile t's MFMAs and stored behind them, one barrier per tile
// (buffer (t + 1) & 1 was last read in iteration t - 1, which every wave left
// through that iteration's barrier). 2 buffers x (K, V) x 64 x d x 2 B = 64 KiB
// at d = 128, so two workgroups share a CU's 160 KiB.
//
// LDS rows are unpadded and XOR-swizzled by 16-byte piece: piece c of row p lies
// at c ^ ((p >> s) & (d / 8 - 1)), s = 0, 1, 2 for d = 128, 64, 32 (a row is 256,
// 128, 64 B: 2^s rows share the 64 banks). Checked by hand for 64 banks of 4 B
// and 16 consecutive lanes a pass: the K operand reads (16 rows r, one piece
// each: banks 4 (c ^ r) at d = 128, 32 (r & 1) + 4 (c ^ (r >> 1)) at d = 64, 16 (r
// & 3) + 4 (c ^ (r >> 2)) at d = 32 - all distinct), the V reads (16 lanes read
// the d / 16 elements at d = r * d / 16 of ONE row: the whole row, a permutation
// of its pieces) and the fetch's stores (consecutive lanes, consecutive pieces
// of a row). The epilogue's f32 rows are swizzled the same way by 4-float piece.
//
// Scores, softmax and output follow the lane map and the numerics of attn_mma.h,
// which attn_decode.hip shares: S^T = K Q^T with K rows from LDS and the Q^T
// fragments loaded once and kept in registers, a column a query row of one of
// the wave's two column blocks; the online softmax per 32-position step; O^T =
// V^T P^T with V^T built in registers from the V tile in LDS.
// [Departure from the plan of a transposing LDS read: gfx950's ds_read_b64_tr_b16
// is exposed by the compiler, but its lane mapping could not be verified on a
// device while this was written; the packs share one proven mapping with
// attn_decode.hip.] The end is o / l.
//
// Causality: a 32-position step that crosses the wave's diagonal gets score -inf
// per lane from the position; a step wholly behind the wave's last row is
// skipped (wave-uniform; the wave still fetches and meets the barrier); the loop
// ends at the tile that holds the workgroup's last row. Positions at or behind
// min(start + S, T) are zero operands and never loaded.
//
// Invariance: a row's steps are the 32-position steps at absolute positions 0,
// 32, ... up to its own; a step wholly behind the row has weights exp2(-inf) = 0,
// a rescale factor exp2(0) = 1, and changes no bit of (m, l, o); an MFMA column
// is a function of that column's operands. So a row's bits depend on its q row,
// its position and the K / V prefix alone - not on B, S, start, the slot, T, the
// strides, or the tile, wave and column it falls into.
#include <hip/hip_runtime.h>

#include "kernels/attn_mma.h"
#include "kernels/attn_plan.h"
#include "kernels/kernels.h"

namespace dissem {
namespace kern {

namespace {

constexpr int BQ = kAttnPrefillBQ, BK = kAttnPrefillBK, kThreads = kAttnPrefillThreads, kWaves = 4;
static_assert(BQ == 32 * kWaves && BK == 64 && kThreads == 64 * kWaves, "the work split below");

// Element offset of 16-byte piece `piece` of row `row` of a [BK][D] bf16 tile in LDS.
template <int D>
__device__ __forceinline__ int kv_off(int row, int piece) {
  constexpr int PR = D / 8, SH = D == 128 ? 0 : (D == 64 ? 1 : 2);
  return row * D + 8 * (piece ^ ((row >> SH) & (PR - 1)));
}

// Float offset of element dd of row `row` of a wave's [32][D] f32 result in LDS.
template <int D>
__device__ __forceinline__ int o_off(int row, int dd) {
  constexpr int SH = D == 32 ? 1 : 0, MASK = D == 32 ? 7 : 15;
  return row * D + 4 * ((dd >> 2) ^ ((row >> SH) & MASK)) + (dd & 3);
}

// ---------------------------------------------------------------- attn_prefill
template <int D, bool BF16>
__global__ void __launch_bounds__(kThreads) attn_prefill_kernel(
    const uint16_t* __restrict__ q, const uint16_t* __restrict__ k, const uint16_t* __restrict__ v,
    const int32_t* __restrict__ start, int B, int S, int heads, int group, int T, int64_t ksb, int64_t ksh,
    int64_t ksp, int64_t vsb, int64_t vsh, int64_t vsp, void* __restrict__ y) {
  constexpr int KS = D / 32;             // MFMA k steps of q . k
  constexpr int DT = D / 16;             // 16-row tiles of V^T; also the d a lane reads of a V row
  constexpr int PR = D / 8;              // 16-byte pieces of a K / V row
  constexpr int NP = BK * PR / kThreads; // pieces of a K (and of a V) tile a lane fetches
  __shared__ __attribute__((aligned(16))) uint16_t sm[2][2][BK * D];  // [buffer][K, V]; the epilogue's f32 rows
  static_assert(sizeof(sm) == size_t(kWaves) * 32 * D * sizeof(float), "the epilogue reuses the tiles");

  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 15, g = lane >> 4;
  const int64_t blk = blockIdx.x;  // (reversed query tile * B + b) * heads + head
  const int h = int(blk % heads);
  const int64_t rest = blk / heads;
  const int b = int(rest % B);
  const int nqt = (S + BQ - 1) / BQ;
  const int q0 = (nqt - 1 - int(rest / B)) * BQ;  // the last tile first: its K walk is the longest
  int st = start ? start[b] : 0;
  st = st < 0 ? 0 : (st > T ? T : st);             // at most 2^20: st + S stays far inside 32 bits
  const int rows = S - q0 < BQ ? S - q0 : BQ;      // rows of this tile that exist
  const int kv_end = st + S < T ? st + S : T;      // nothing at or behind it is loaded
  const int pos0 = st + q0;                        // position of the tile's row 0
  const int pos_end = pos0 + rows < T ? pos0 + rows : T;  // one behind the last position with a row here
  const int ntiles = pos_end > pos0 ? (pos_end - 1) / BK + 1 : 0;
  const int wpos0 = pos0 + 32 * wave;              // position of the wave's row 0
  const bool wave_on = wpos0 < pos_end;            // the wave has a row with a position below T

  const uint16_t* kb = k + b * ksb + int64_t(h / group) * ksh;
  const uint16_t* vb = v + b * vsb + int64_t(h / group) * vsh;

  // Q^T, the B operand of S^T: per column block, lane holds Q[row 16 cb + r][32 ks + 8 g + 0..7]; a row that
  // does not exist or whose position is >= T is a zero row and is not loaded
  bf16x8_t qf[2][KS];
  int prow[2];
  bool rvalid[2];
#pragma unroll
  for (int cb = 0; cb < 2; ++cb) {
    const int iq = 32 * wave + 16 * cb + r;
    prow[cb] = pos0 + iq;
    rvalid[cb] = iq < rows && prow[cb] < T;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      Words<4> w;
      if (rvalid[cb]) w.load(q + ((int64_t(b) * S + q0 + iq) * heads + h) * D + 32 * ks + 8 * g);
      else w.w[0] = w.w[1] = w.w[2] = w.w[3] = 0;
      qf[cb][ks] = as_frag(w.w);
    }
  }

  const float sc = attn_score_scale(D);
  float m[2] = {-INFINITY, -INFINITY}, l[2] = {0.0f, 0.0f};
  f32x4_t ot[2][DT];
#pragma unroll
  for (int cb = 0; cb < 2; ++cb)
#pragma unroll
    for (int t = 0; t < DT; ++t) ot[cb][t] = f32x4_t{0.0f, 0.0f, 0.0f, 0.0f};

  // the lane's pieces of a tile: piece tid + kThreads n is row (.) / PR, 16 bytes (.) % PR of it
  uint4 kr[NP], vr[NP];
#define ATTN_PREFILL_FETCH(tile)                                                        \
  _Pragma("unroll") for (int n = 0; n < NP; ++n) {                                      \
    const int idx = tid + kThreads * n, pos = (tile) * BK + idx / PR, c8 = 8 * (idx % PR); \
    kr[n] = vr[n] = uint4{0u, 0u, 0u, 0u};                                              \
    if (pos < kv_end) {                                                                 \
      kr[n] = *reinterpret_cast<const uint4*>(kb + int64_t(pos) * ksp + c8);            \
      vr[n] = *reinterpret_cast<const uint4*>(vb + int64_t(pos) * vsp + c8);            \
    }                                                                                   \
  }
#define ATTN_PREFILL_STASH(buf)                                                         \
  _Pragma("unroll") for (int n = 0; n < NP; ++n) {                                      \
    const int idx = tid + kThreads * n, off = kv_off<D>(idx / PR, idx % PR);            \
    *reinterpret_cast<uint4*>(&sm[buf][0][off]) = kr[n];                                \
    *reinterpret_cast<uint4*>(&sm[buf][1][off]) = vr[n];                                \
  }

  if (ntiles > 0) {
    ATTN_PREFILL_FETCH(0)
    ATTN_PREFILL_STASH(0)
  }
  __syncthreads();

  for (int t = 0; t < ntiles; ++t) {
    const bool more = t + 1 < ntiles;
    if (more) { ATTN_PREFILL_FETCH(t + 1) }  // in flight while this tile's MFMAs run
    const uint16_t* sk = sm[t & 1][0];
    const uint16_t* sv = sm[t & 1][1];
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      const int p0 = t * BK + 32 * half;               // the step's first position
      if (!wave_on || p0 > wpos0 + 31) continue;       // wholly behind the wave's last row (wave-uniform)
      const bool diag = p0 + 31 > wpos0;               // some lane's row ends inside the step
      // scores of the step's two 16-position tiles, per column block: rows are positions, columns query rows
      f32x4_t s4[2][2];
#pragma unroll
      for (int tt = 0; tt < 2; ++tt) {
        s4[0][tt] = s4[1][tt] = f32x4_t{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          Words<4> w;
          w.load(sk + kv_off<D>(32 * half + 16 * tt + r, 4 * ks + g));
          const bf16x8_t kf = as_frag(w.w);
          s4[0][tt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[0][ks], s4[0][tt], 0, 0, 0);
          s4[1][tt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[1][ks], s4[1][tt], 0, 0, 0);
        }
      }
      // V of the lane's 8 positions (slot j: tile j >> 2, accumulator register j & 3), DT values at d = r * DT
      Words<DT / 2> vv[8];
#pragma unroll
      for (int j = 0; j < 8; ++j)
        vv[j].load(sv + kv_off<D>(32 * half + 16 * (j >> 2) + 4 * g + (j & 3), (r * DT) / 8) + (r * DT) % 8);
      // online softmax of row r of each column block over the step
      float alpha[2];
      bf16x8_t pf[2];
#pragma unroll
      for (int cb = 0; cb < 2; ++cb) {
        float s[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) s[j] = s4[cb][j >> 2][j & 3] * sc;
        if (diag) {
#pragma unroll
          for (int j = 0; j < 8; ++j)
            if (p0 + 16 * (j >> 2) + 4 * g + (j & 3) > prow[cb]) s[j] = -INFINITY;
        }
        uint32_t pw[4];  // m stays finite: the first step holds position 0, which every row sees
        attn_softmax_step(s, m[cb], l[cb], alpha[cb], pw);
        pf[cb] = as_frag(pw);
      }
#pragma unroll
      for (int tv = 0; tv < DT; ++tv) {
        uint32_t aw[4];
        attn_vt_row(vv, tv, aw);
        const bf16x8_t af = as_frag(aw);
#pragma unroll
        for (int cb = 0; cb < 2; ++cb) {
          ot[cb][tv] = ot[cb][tv] * alpha[cb];
          ot[cb][tv] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, pf[cb], ot[cb][tv], 0, 0, 0);
        }
      }
    }
    if (more) { ATTN_PREFILL_STASH((t + 1) & 1) }
    __syncthreads();
  }
#undef ATTN_PREFILL_FETCH
#undef ATTN_PREFILL_STASH

  // Epilogue, through LDS (every wave is past the last barrier, the tiles are dead): the wave's [32][D] f32
  // rows, then y in 16-byte row pieces. Accumulator register i of tile tv: d = (4 g + i) * DT + tv, column r.
  float* so = reinterpret_cast<float*>(&sm[0][0][0]) + wave * 32 * D;
#pragma unroll
  for (int cb = 0; cb < 2; ++cb) {
    float lt = l[cb];  // the lane groups' partial sums, the same value in all four
    lt += __shfl_xor(lt, 16);
    lt += __shfl_xor(lt, 32);
#pragma unroll
    for (int tv = 0; tv < DT; ++tv)
#pragma unroll
      for (int i = 0; i < 4; ++i)
        so[o_off<D>(16 * cb + r, (4 * g + i) * DT + tv)] = rvalid[cb] ? ot[cb][tv][i] / lt : 0.0f;
  }
  __syncthreads();
  constexpr int PO = BF16 ? D / 8 : D / 4;  // 16-byte pieces of an output row
#pragma unroll
  for (int n = 0; n < 32 * PO / 64; ++n) {
    const int idx = lane + 64 * n, row = idx / PO, c = idx % PO, iq = 32 * wave + row;
    if (iq >= rows) continue;  // no such row
    const int64_t out = ((int64_t(b) * S + q0 + iq) * heads + h) * D;
    if (BF16) {
      const float4 a = *reinterpret_cast<const float4*>(so + o_off<D>(row, 8 * c));
      const float4 e = *reinterpret_cast<const float4*>(so + o_off<D>(row, 8 * c + 4));
      uint4 u;
      u.x = uint32_t(f32_to_bf16_rne(a.x)) | (uint32_t(f32_to_bf16_rne(a.y)) << 16);
      u.y = uint32_t(f32_to_bf16_rne(a.z)) | (uint32_t(f32_to_bf16_rne(a.w)) << 16);
      u.z = uint32_t(f32_to_bf16_rne(e.x)) | (uint32_t(f32_to_bf16_rne(e.y)) << 16);
      u.w = uint32_t(f32_to_bf16_rne(e.z)) | (uint32_t(f32_to_bf16_rne(e.w)) << 16);
      *reinterpret_cast<uint4*>(static_cast<uint16_t*>(y) + out + 8 * c) = u;
    } else {
      *reinterpret_cast<float4*>(static_cast<float*>(y) + out + 4 * c) =
          *reinterpret_cast<const float4*>(so + o_off<D>(row, 4 * c));
    }
  }
}

// ---------------------------------------------------------------- rope_append_seq
// One thread per (row n = b * S + i, head slot of q, k or v, piece c): 8 d of the lower half at 8 c and
// the matching 8 of the upper half, everything in 16-byte loads and stores.
template <int D>
__global__ void __launch_bounds__(kThreads) rope_append_seq_kernel(
    const uint16_t* __restrict__ q, int64_t ldq, const uint16_t* __restrict__ k, int64_t ldk,
    const uint16_t* __restrict__ v, int64_t ldv, const int32_t* __restrict__ start, const float* __restrict__ cos,
    const float* __restrict__ sin, int64_t total, int S, int capacity, int heads, int kv_heads,
    uint16_t* __restrict__ q_out, uint16_t* __restrict__ k_cache, uint16_t* __restrict__ v_cache) {
  constexpr int L = D / 16;  // threads of a head row
  const int64_t idx = int64_t(blockIdx.x) * kThreads + threadIdx.x;
  if (idx >= total) return;
  const int c = int(idx % L);
  const int64_t hr = idx / L;
  const int slots = heads + 2 * kv_heads, slot = int(hr % slots);
  const int64_t n = hr / slots, b = n / S;
  const int64_t p = int64_t(start ? start[b] : 0) + (n - b * S);
  const bool ok = p >= 0 && p < capacity;
  const int lo = 8 * c, hi = D / 2 + 8 * c;
  if (slot >= heads + kv_heads) {  // v: copied as it is
    if (!ok) return;
    const int hh = slot - heads - kv_heads;
    const uint16_t* src = v + n * ldv + int64_t(hh) * D;
    uint16_t* dst = v_cache + ((b * kv_heads + hh) * capacity + p) * D;
    *reinterpret_cast<uint4*>(dst + lo) = *reinterpret_cast<const uint4*>(src + lo);
    *reinterpret_cast<uint4*>(dst + hi) = *reinterpret_cast<const uint4*>(src + hi);
    return;
  }
  const bool is_q = slot < heads;
  const int hh = is_q ? slot : slot - heads;
  if (!ok) {  // no table row for this position: a defined q row, nothing in the caches
    if (is_q) {
      uint16_t* dst = q_out + (n * heads + hh) * D;
      *reinterpret_cast<uint4*>(dst + lo) = uint4{0u, 0u, 0u, 0u};
      *reinterpret_cast<uint4*>(dst + hi) = uint4{0u, 0u, 0u, 0u};
    }
    return;
  }
  const uint16_t* src = is_q ? q + n * ldq + int64_t(hh) * D : k + n * ldk + int64_t(hh) * D;
  uint16_t* dst = is_q ? q_out + (n * heads + hh) * D : k_cache + ((b * kv_heads + hh) * capacity + p) * D;
  union V8 {
    uint4 u;
    uint16_t e[8];
  };
  union F8 {
    float4 f4[2];
    float e[8];
  };
  V8 xl, xh, ol, oh;
  xl.u = *reinterpret_cast<const uint4*>(src + lo);
  xh.u = *reinterpret_cast<const uint4*>(src + hi);
  F8 cl, ch, sl, sh;
  const float* ct = cos + p * D;
  const float* stb = sin + p * D;
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
  *reinterpret_cast<uint4*>(dst + lo) = ol.u;
  *reinterpret_cast<uint4*>(dst + hi) = oh.u;
}

template <int D>
hipError_t launch_prefill(const uint16_t* q, const uint16_t* k, const uint16_t* v, const int32_t* start, int B, int S,
                          int heads, int T, const AttnPrefillPlan& p, const int64_t* ks, const int64_t* vs, void* y,
                          bool y_bf16, hipStream_t s) {
  if (y_bf16)
    attn_prefill_kernel<D, true><<<unsigned(p.blocks), kThreads, 0, s>>>(q, k, v, start, B, S, heads, p.group, T, ks[0],
                                                                        ks[1], ks[2], vs[0], vs[1], vs[2], y);
  else
    attn_prefill_kernel<D, false><<<unsigned(p.blocks), kThreads, 0, s>>>(q, k, v, start, B, S, heads, p.group, T, ks[0],
                                                                         ks[1], ks[2], vs[0], vs[1], vs[2], y);
  return hipGetLastError();
}

template <int D>
hipError_t launch_rope_seq(const uint16_t* q, int64_t ldq, const uint16_t* k, int64_t ldk, const uint16_t* v,
                           int64_t ldv, const int32_t* start, const float* cos, const float* sin,
                           const AttnRopeSeqPlan& p, int S, int capacity, int heads, int kv_heads, uint16_t* q_out,
                           uint16_t* k_cache, uint16_t* v_cache, hipStream_t s) {
  rope_append_seq_kernel<D><<<unsigned(p.blocks), kThreads, 0, s>>>(q, ldq, k, ldk, v, ldv, start, cos, sin, p.threads, S,
                                                                   capacity, heads, kv_heads, q_out, k_cache, v_cache);
  return hipGetLastError();
}

}  // namespace

hipError_t attn_prefill(const uint16_t* q, const uint16_t* k, const uint16_t* v, const int32_t* start, int64_t B,
                        int64_t S, int64_t heads, int64_t kv_heads, int64_t d, int64_t T, const int64_t* kstride,
                        const int64_t* vstride, void* y, bool y_bf16, hipStream_t s) {
  if (!kstride || !vstride) return hipErrorInvalidValue;
  const AttnPrefillPlan p = attn_prefill_plan(B, S, heads, kv_heads, d, T, kstride, vstride);
  if (!p.ok || !q || !k || !v || !y) return hipErrorInvalidValue;
  if (!aligned16(q) || !aligned16(k) || !aligned16(v) || !aligned16(y)) return hipErrorInvalidValue;
  const int b = int(B), ss = int(S), h = int(heads), t = int(T);
  if (d == 32) return launch_prefill<32>(q, k, v, start, b, ss, h, t, p, kstride, vstride, y, y_bf16, s);
  if (d == 64) return launch_prefill<64>(q, k, v, start, b, ss, h, t, p, kstride, vstride, y, y_bf16, s);
  return launch_prefill<128>(q, k, v, start, b, ss, h, t, p, kstride, vstride, y, y_bf16, s);
}

hipError_t attn_rope_append_seq(const uint16_t* q, int64_t ldq, const uint16_t* k, int64_t ldk, const uint16_t* v,
                                int64_t ldv, const int32_t* start, const float* cos, const float* sin, int64_t B,
                                int64_t S, int64_t heads, int64_t kv_heads, int64_t d, int64_t capacity,
                                uint16_t* q_out, uint16_t* k_cache, uint16_t* v_cache, hipStream_t s) {
  const AttnRopeSeqPlan p = attn_rope_seq_plan(B, S, heads, kv_heads, d, capacity, ldq, ldk, ldv);
  if (!p.ok || !q || !k || !v || !cos || !sin || !q_out || !k_cache || !v_cache) return hipErrorInvalidValue;
  if (!aligned16(q) || !aligned16(k) || !aligned16(v) || !aligned16(cos) || !aligned16(sin) || !aligned16(q_out) ||
      !aligned16(k_cache) || !aligned16(v_cache))
    return hipErrorInvalidValue;
  const int ss = int(S), cap = int(capacity), h = int(heads), kv = int(kv_heads);
  if (d == 32)
    return launch_rope_seq<32>(q, ldq, k, ldk, v, ldv, start, cos, sin, p, ss, cap, h, kv, q_out, k_cache, v_cache, s);
  if (d == 64)
    return launch_rope_seq<64>(q, ldq, k, ldk, v, ldv, start, cos, sin, p, ss, cap, h, kv, q_out, k_cache, v_cache, s);
  return launch_rope_seq<128>(q, ldq, k, ldk, v, ldv, start, cos, sin, p, ss, cap, h, kv, q_out, k_cache, v_cache, s);
}

}  // namespace kern
}  // namespace dissem
