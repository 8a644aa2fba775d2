// Causal grouped-query attention of S new tokens per sequence against an MXFP8
// KV cache in HBM - e4m3fn codes uint8 [B, kv_heads, T, d] and one E8M0 scale
// byte per 32 d, uint8 [B, kv_heads, T, d / 32], both contiguous, d 64 or 128 -
// and the rope, quantization and append of those S tokens (kernels.h has the
// contracts).
//
// attn_prefill_mxfp8 is attn_prefill.hip's decomposition - a workgroup of four
// waves per (sequence, query head, tile of BQ = 128 rows), the last query tile
// first, K / V tiles of BK = 64 positions at absolute positions, two LDS buffers
// and one barrier a tile, the same swizzle, MFMA loop, causal masking and
// epilogue - with an operand path of its own: a tile is DEQUANTIZED ONCE PER
// WORKGROUP, ON THE WAY FROM REGISTERS INTO LDS. (attn_decode_mxfp8.hip converts
// in registers at every use, because there a code is used once; here 128 query
// rows use it.) LDS then holds the very bf16 tile attn_prefill.hip holds for the
// dequantized cache, every instruction from the first LDS read on is that
// kernel's, and so are the result's bits.
//
// The fetch: a lane's 16-byte global load is 16 codes, d [16 c, 16 c + 16) of
// one position - code piece idx = tid + 256 n is row idx / (d / 16), c = idx % (d
// / 16) - all of scale block c / 2, whose byte the lane loads as well. A K tile
// is 64 d bytes: two loads a lane for K and two for V at d = 128 (the bf16 kernel:
// four and four), one and one at d = 64. Codes and scale bytes of tile t + 1 are
// loaded before tile t's MFMAs and held in registers, half the bf16 fetch's.
// The stash: fp8x2_to_bf16x2 (one v_cvt_scalef32_pk_bf16_fp8 a pair) turns the 16
// codes into the two 16-byte bf16 pieces 2 c and 2 c + 1 of the row, stored at
// kv_off<D>(row, piece). Positions at or behind min(start + S, T) load neither
// codes nor scale bytes: zero codes under a scale of 1 are stashed, bf16 +0.
//
// Bank check of the stash's stores, by hand as in attn_prefill.hip (64 banks of
// 4 B, 16 consecutive lanes a pass, a 16-byte slot = 4 banks, 16 slots): a lane
// stores every OTHER piece of its row in a pass - the even pieces 2 c, then the
// odd ones.
//   d = 128 (a row is the 16 slots; slot = piece ^ (row & 15)): 16 lanes are c =
//   0..7 of rows p and p + 1, p even. Pieces 2 c are the 8 even numbers; the XOR
//   with an even row keeps them even, with an odd row makes them odd: row p fills
//   the even slots, row p + 1 the odd ones. The second pass swaps the two.
//   d = 64 (two rows share the 16 slots; slot = 8 (row & 1) + (piece ^ ((row >> 1)
//   & 7))): 16 lanes are c = 0..3 of rows p .. p + 3, p a multiple of 4. Pieces 2 c
//   are 0, 2, 4, 6; x = (p >> 1) & 7 is even for rows p, p + 1 and x + 1 for p + 2, p
//   + 3: the four rows fill (lower half, even), (upper, even), (lower, odd),
//   (upper, odd). The second pass again swaps even and odd.
// Sixteen distinct slots in every pass, so the plain lane map stays. The LDS reads
// are attn_prefill.hip's and checked there.
//
// kv_off, o_off and the tile loop are repeated here and not shared through a
// header: attn_prefill.hip stays untouched, and with it its generated code.
//
// attn_rope_append_seq_mxfp8 is rope_append_mxfp8_kernel (attn_decode_mxfp8.hip)
// for S tokens a sequence: the same thread map - a thread owns 8 d of the lower
// half of a head and their partners of the upper half, 16-byte loads, a quad of
// lanes one 32-block of each half, fp8_pack8<4> the quantizer, 8-byte code
// stores - with one workgroup per (row b * S + i, slice of kAttnRopeMxThreads
// items): whether the row's position lies in the cache is one answer for the
// workgroup, and every lane reaches the quantizer's DPP reduction whatever it is.
#include <hip/hip_runtime.h>

#include "kernels/attn_mma.h"
#include "kernels/attn_plan.h"
#include "kernels/fp8_cvt.h"
#include "kernels/fp8_pack.h"
#include "kernels/kernels.h"

namespace dissem {
namespace kern {

namespace {

constexpr int BQ = kAttnPrefillBQ, BK = kAttnPrefillBK, kThreads = kAttnPrefillThreads, kWaves = 4;
static_assert(BQ == 32 * kWaves && BK == 64 && kThreads == 64 * kWaves, "the work split below");

// Element offset of 16-byte piece `piece` of row `row` of a [BK][D] bf16 tile in LDS (attn_prefill.hip's).
template <int D>
__device__ __forceinline__ int kv_off(int row, int piece) {
  constexpr int PR = D / 8, SH = D == 128 ? 0 : 1;
  return row * D + 8 * (piece ^ ((row >> SH) & (PR - 1)));
}

// Float offset of element dd of row `row` of a wave's [32][D] f32 result in LDS.
template <int D>
__device__ __forceinline__ int o_off(int row, int dd) {
  return row * D + 4 * ((dd >> 2) ^ (row & 15)) + (dd & 3);
}

// ---------------------------------------------------------------- attn_prefill_mxfp8
template <int D, bool BF16>
__global__ void __launch_bounds__(kThreads) attn_prefill_mxfp8_kernel(
    const uint16_t* __restrict__ q, const uint8_t* __restrict__ k_codes, const uint8_t* __restrict__ k_scales,
    const uint8_t* __restrict__ v_codes, const uint8_t* __restrict__ v_scales, const int32_t* __restrict__ start,
    int B, int S, int heads, int kv_heads, int group, int T, void* __restrict__ y) {
  constexpr int KS = D / 32;              // MFMA k steps of q . k
  constexpr int DT = D / 16;              // 16-row tiles of V^T; also the d a lane reads of a V row
  constexpr int PC = D / 16;              // 16-byte pieces of a row of codes
  constexpr int NB = D / 32;              // scale bytes of a row
  constexpr int NC = BK * PC / kThreads;  // code pieces of a K (and of a V) tile a lane fetches: 2 or 1
  __shared__ __attribute__((aligned(16))) uint16_t sm[2][2][BK * D];  // [buffer][K, V] as bf16; the epilogue's f32 rows
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

  const int64_t bh = int64_t(b) * kv_heads + h / group;  // the (sequence, KV head)'s rows: [bh * T, bh * T + T)
  const uint8_t* kcb = k_codes + bh * T * D;
  const uint8_t* vcb = v_codes + bh * T * D;
  const uint8_t* ksb = k_scales + bh * T * NB;
  const uint8_t* vsb = v_scales + bh * T * NB;

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

  // the lane's code pieces of a tile: piece tid + kThreads n is row (.) / PC, codes 16 ((.) % PC) .. + 15 of it,
  // with the byte of their scale block ((.) % PC) / 2. Behind kv_end: zero codes under 2^0, never a load.
  uint4 kr[NC], vr[NC];
  uint32_t ke[NC], ve[NC];
#define ATTN_PREFILL_MX_FETCH(tile)                                                       \
  _Pragma("unroll") for (int n = 0; n < NC; ++n) {                                        \
    const int idx = tid + kThreads * n, pos = (tile) * BK + idx / PC, c = idx % PC;       \
    kr[n] = vr[n] = uint4{0u, 0u, 0u, 0u};                                                \
    ke[n] = ve[n] = 127u;                                                                 \
    if (pos < kv_end) {                                                                   \
      kr[n] = *reinterpret_cast<const uint4*>(kcb + int64_t(pos) * D + 16 * c);           \
      vr[n] = *reinterpret_cast<const uint4*>(vcb + int64_t(pos) * D + 16 * c);           \
      ke[n] = ksb[int64_t(pos) * NB + (c >> 1)];                                          \
      ve[n] = vsb[int64_t(pos) * NB + (c >> 1)];                                          \
    }                                                                                     \
  }
  // dequantized on the way into LDS: codes 0..7 are bf16 piece 2 c of the row, codes 8..15 piece 2 c + 1
#define ATTN_PREFILL_MX_STASH(buf)                                                        \
  _Pragma("unroll") for (int n = 0; n < NC; ++n) {                                        \
    const int idx = tid + kThreads * n, row = idx / PC, c = idx % PC;                     \
    const float fk = e8m0_scale(ke[n]), fv = e8m0_scale(ve[n]);                           \
    uint4 k0, k1, v0, v1;                                                                 \
    dequant4(kr[n].x, fk, k0.x, k0.y);                                                    \
    dequant4(kr[n].y, fk, k0.z, k0.w);                                                    \
    dequant4(kr[n].z, fk, k1.x, k1.y);                                                    \
    dequant4(kr[n].w, fk, k1.z, k1.w);                                                    \
    dequant4(vr[n].x, fv, v0.x, v0.y);                                                    \
    dequant4(vr[n].y, fv, v0.z, v0.w);                                                    \
    dequant4(vr[n].z, fv, v1.x, v1.y);                                                    \
    dequant4(vr[n].w, fv, v1.z, v1.w);                                                    \
    const int off0 = kv_off<D>(row, 2 * c), off1 = kv_off<D>(row, 2 * c + 1);             \
    *reinterpret_cast<uint4*>(&sm[buf][0][off0]) = k0;                                    \
    *reinterpret_cast<uint4*>(&sm[buf][1][off0]) = v0;                                    \
    *reinterpret_cast<uint4*>(&sm[buf][0][off1]) = k1;                                    \
    *reinterpret_cast<uint4*>(&sm[buf][1][off1]) = v1;                                    \
  }

  if (ntiles > 0) {
    ATTN_PREFILL_MX_FETCH(0)
    ATTN_PREFILL_MX_STASH(0)
  }
  __syncthreads();

  // From here to the end: attn_prefill.hip's tile loop and epilogue, on the same LDS contents.
  for (int t = 0; t < ntiles; ++t) {
    const bool more = t + 1 < ntiles;
    if (more) { ATTN_PREFILL_MX_FETCH(t + 1) }  // in flight while this tile's MFMAs run
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
    if (more) { ATTN_PREFILL_MX_STASH((t + 1) & 1) }
    __syncthreads();
  }
#undef ATTN_PREFILL_MX_FETCH
#undef ATTN_PREFILL_MX_STASH

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

// ---------------------------------------------------------------- rope_append_seq_mxfp8
// Workgroup (n, y): items [y * kAttnRopeMxThreads, ...) of row n = b * S + i, an item a (head slot of q, k or
// v, piece c): 8 d of the lower half at 8 c and the matching 8 of the upper half.
template <int D>
__global__ void __launch_bounds__(kAttnRopeMxThreads)
    rope_append_seq_mxfp8_kernel(const uint16_t* __restrict__ q, int64_t ldq, const uint16_t* __restrict__ k,
                                 int64_t ldk, const uint16_t* __restrict__ v, int64_t ldv,
                                 const int32_t* __restrict__ start, const float* __restrict__ cos,
                                 const float* __restrict__ sin, int items, int S, int capacity, int heads,
                                 int kv_heads, uint16_t* __restrict__ q_out, uint8_t* __restrict__ k_codes,
                                 uint8_t* __restrict__ k_scales, uint8_t* __restrict__ v_codes,
                                 uint8_t* __restrict__ v_scales) {
  constexpr int L = D / 16;  // threads of a head row: 4 or 8, so a quad of lanes never spans two rows
  const int64_t n = blockIdx.x, b = n / S;
  const int item = int(blockIdx.y) * kAttnRopeMxThreads + int(threadIdx.x);
  const bool active = item < items;
  const int c = item % L, slot = item / L;
  const int lo = 8 * c, hi = D / 2 + 8 * c;
  const bool is_q = slot < heads, is_k = !is_q && slot < heads + kv_heads;
  const int hh = is_q ? slot : (is_k ? slot - heads : slot - heads - kv_heads);
  const int64_t p = int64_t(start ? start[b] : 0) + (n - b * S);
  const bool ok = p >= 0 && p < capacity;  // the whole workgroup's answer; outside: a zero q row, no load
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
  if (active && ok) {
    const uint16_t* src = is_q ? q + n * ldq : (is_k ? k + n * ldk : v + n * ldv);
    src += int64_t(hh) * D;
    ol.u = *reinterpret_cast<const uint4*>(src + lo);
    oh.u = *reinterpret_cast<const uint4*>(src + hi);
    if (is_q || is_k) {
      const V8 xl = ol, xh = oh;
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
    }
  }
  if (active && is_q) {  // rotated, or the zero row of a position outside the cache
    uint16_t* dst = q_out + (n * heads + hh) * D;
    *reinterpret_cast<uint4*>(dst + lo) = ol.u;
    *reinterpret_cast<uint4*>(dst + hi) = oh.u;
  }
  // fp8_pack8 reduces over the quad with DPP: every lane of every wave arrives here - q lanes, lanes without an
  // item and the lanes of a row outside the cache with zeros. No return stands before it.
  const bool to_cache = active && ok && !is_q;
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
hipError_t launch_prefill_mxfp8(const uint16_t* q, const uint8_t* k_codes, const uint8_t* k_scales,
                                const uint8_t* v_codes, const uint8_t* v_scales, const int32_t* start, int B, int S,
                                int heads, int kv_heads, int T, const AttnPrefillPlan& p, void* y, bool y_bf16,
                                hipStream_t s) {
  if (y_bf16)
    attn_prefill_mxfp8_kernel<D, true><<<unsigned(p.blocks), kThreads, 0, s>>>(
        q, k_codes, k_scales, v_codes, v_scales, start, B, S, heads, kv_heads, p.group, T, y);
  else
    attn_prefill_mxfp8_kernel<D, false><<<unsigned(p.blocks), kThreads, 0, s>>>(
        q, k_codes, k_scales, v_codes, v_scales, start, B, S, heads, kv_heads, p.group, T, y);
  return hipGetLastError();
}

template <int D>
hipError_t launch_rope_seq_mxfp8(const uint16_t* q, int64_t ldq, const uint16_t* k, int64_t ldk, const uint16_t* v,
                                 int64_t ldv, const int32_t* start, const float* cos, const float* sin,
                                 const AttnRopeSeqMxPlan& p, int S, int capacity, int heads, int kv_heads,
                                 uint16_t* q_out, uint8_t* k_codes, uint8_t* k_scales, uint8_t* v_codes,
                                 uint8_t* v_scales, hipStream_t s) {
  rope_append_seq_mxfp8_kernel<D><<<dim3(unsigned(p.rows), unsigned(p.grid_y)), kAttnRopeMxThreads, 0, s>>>(
      q, ldq, k, ldk, v, ldv, start, cos, sin, p.items, S, capacity, heads, kv_heads, q_out, k_codes, k_scales,
      v_codes, v_scales);
  return hipGetLastError();
}

}  // namespace

hipError_t attn_prefill_mxfp8(const uint16_t* q, const uint8_t* k_codes, const uint8_t* k_scales,
                              const uint8_t* v_codes, const uint8_t* v_scales, const int32_t* start, int64_t B,
                              int64_t S, int64_t heads, int64_t kv_heads, int64_t d, int64_t T, void* y, bool y_bf16,
                              hipStream_t s) {
  const AttnPrefillPlan p = attn_prefill_mxfp8_plan(B, S, heads, kv_heads, d, T);
  if (!p.ok || !q || !k_codes || !k_scales || !v_codes || !v_scales || !y) return hipErrorInvalidValue;
  if (!aligned16(q) || !aligned16(k_codes) || !aligned16(v_codes) || !aligned16(y)) return hipErrorInvalidValue;
  const int b = int(B), ss = int(S), h = int(heads), kv = int(kv_heads), t = int(T);
  if (d == 64)
    return launch_prefill_mxfp8<64>(q, k_codes, k_scales, v_codes, v_scales, start, b, ss, h, kv, t, p, y, y_bf16, s);
  return launch_prefill_mxfp8<128>(q, k_codes, k_scales, v_codes, v_scales, start, b, ss, h, kv, t, p, y, y_bf16, s);
}

hipError_t attn_rope_append_seq_mxfp8(const uint16_t* q, int64_t ldq, const uint16_t* k, int64_t ldk,
                                      const uint16_t* v, int64_t ldv, const int32_t* start, const float* cos,
                                      const float* sin, int64_t B, int64_t S, int64_t heads, int64_t kv_heads,
                                      int64_t d, int64_t capacity, uint16_t* q_out, uint8_t* k_codes,
                                      uint8_t* k_scales, uint8_t* v_codes, uint8_t* v_scales, hipStream_t s) {
  const AttnRopeSeqMxPlan p = attn_rope_seq_mxfp8_plan(B, S, heads, kv_heads, d, capacity, ldq, ldk, ldv);
  if (!p.ok) return hipErrorInvalidValue;
  if (!q || !k || !v || !cos || !sin || !q_out || !k_codes || !k_scales || !v_codes || !v_scales)
    return hipErrorInvalidValue;
  if (!aligned16(q) || !aligned16(k) || !aligned16(v) || !aligned16(cos) || !aligned16(sin) || !aligned16(q_out) ||
      !aligned16(k_codes) || !aligned16(v_codes))
    return hipErrorInvalidValue;
  const int ss = int(S), cap = int(capacity), h = int(heads), kv = int(kv_heads);
  if (d == 64)
    return launch_rope_seq_mxfp8<64>(q, ldq, k, ldk, v, ldv, start, cos, sin, p, ss, cap, h, kv, q_out, k_codes,
                                     k_scales, v_codes, v_scales, s);
  return launch_rope_seq_mxfp8<128>(q, ldq, k, ldk, v, ldv, start, cos, sin, p, ss, cap, h, kv, q_out, k_codes,
                                    k_scales, v_codes, v_scales, s);
}

}  // namespace kern
}  // namespace dissem
